// Nuclei by region (gfx950): an exact point-in-polygon census of a slide's nucleus centres against annotated regions (tumour, stroma,
// the tissue outline) -- which regions hold each nucleus, and how many nuclei of each class every region holds.
//
// Definition (nuhtc_amd/regions.py holds it in full, with the int64 brute-force restatement `regions_reference`): n points in HALF
// pixels (|p| < 2^27, n <= 2^24), one label each, C classes (1 .. 14), and G regions (<= 2^16) as a flat table of E edges (<= 2^22)
// (ax, ay, bx, by) in half pixels with edge_region non-decreasing.  Even-odd and half-open: an edge straddles p when exactly one end has
// y <= p.y, and is crossed when p lies strictly on the -x side of the upward-oriented edge (region_crossed of cellgrid_host.h, an exact
// int64 cross product); p is inside a region when an odd number of its edges are crossed, and on the boundary when it lies on an edge
// of any region (region_on_edge).  region = the largest index that holds the point (-1: none), depth = how many hold it, census[g][c] =
// the points of label c inside g.  Integer compares and integer adds only: a pure function of the input, bitwise the same on every call.
//
// This is the first analysis of the family whose second input is not the points: the points are binned as ever, the EDGES are binned
// by the slab (grid row) they meet, and a point is tested against edges.  Stages, all on the caller's stream:
//   geometry   on the HOST from the caller's bounding box (cell_grid_side): cells of side >= slab, at most 2^22 of them.  A grid row is
//              a horizontal SLAB of the box, and with one key per cell its points are one contiguous run of the records.
//   binning    cellbin.h, reach slab, one key per cell.
//   edges      celledges.h (shared with cellmargin.hip), with region_slab_range as the slabs an edge has a record in: clipped to the
//              box; an edge wholly above, below or left of the box meets none.  rg_check_kernel states M, the (edge, slab) records the
//              call needs, and every later kernel first compares M with the caller's slot_cap (rg_go); count, scan, emit, place leave
//              every slab's records in edge order, hence grouped by region, ascending.
//   crossing   rg_cross_kernel  one workgroup per 256 consecutive point records.  For each slab that holds some of them (the records are
//                               in row order, so these are few) the slab's edge records go through LDS 256 at a time -- coordinates and
//                               region gathered once per workgroup -- and every thread of that slab takes each staged edge by a broadcast
//                               LDS read.  The edge sequence, and with it the region changes, are the same for every thread of the
//                               workgroup: each thread carries (parity, depth, top, on-boundary), and at a region change the waves add
//                               their odd lanes to census, one integer atomic per (wave, class present) -- a ballot per class, as the
//                               cluster tables do.
//   outputs    every kernel that writes an output tests the flag and M first: a refused call leaves every output untouched, and so does a
//              call whose slot_cap is below M (it returns 0 and reports M: the caller calls once more).  With n == 0 the edges are still
//              checked and census is cleared.
// No kernel waits on another workgroup; every loop runs over a range of a table.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, profiles/cell_regions_resources.txt): no scratch in any kernel; the crossing
// kernel holds 256 x (16 + 4) B of staged edges and one int, 5124 B of LDS, so LDS never bounds the occupancy (160 KiB per CU); a
// larger stage would only lengthen the time between barriers.
//
// Everything that decides an index, a side or a limit -- region_crossed, region_on_edge, region_slab_range, region_edge_ok,
// region_call_ok (cellgrid_host.h) -- is plain C++, and tools/dev/cellregion_host_check.cpp runs exactly those functions on the host
// under -fsanitize=address,undefined against __int128 arithmetic and a direct loop.  The kernel code itself is not sanitized.
#include <climits>
#include <cstring>

#include "celledges.h"

namespace {

struct CellRegionArgs {
  CellBin b;                          // the points, the grid and the records in cell order (cellbin.h, one key per cell)
  const int4* edges;                  // [E] (ax, ay, bx, by) half pixels
  const int32_t* edge_region;         // [E] non-decreasing
  int E, G, C;
  int have_grid;                      // 0 with n == 0: the edges are checked, no slab is counted
  unsigned long long slot_cap;        // the (edge, slab) records the caller left room for
  unsigned long long* total;          // M: the records the call needs
  int* slab_count;                    // [nchunk * CB_CHUNK] per slab, zero past them; counted up, and down again by the emit
  int* slab_start;                    // [nchunk * CB_CHUNK] entry k = records in front of slab k (entry ncy: all of them)
  int2* emitted;                      // [slot_cap] (edge, slab) in arrival order inside a slab's segment
  int* slots;                         // [slot_cap] the edge of every record, slab by slab, in edge order
  int32_t* region;                    // [n]
  int32_t* depth;                     // [n]
  uint8_t* on_boundary;               // [n]
  unsigned long long* census;         // [G][C]
};

__device__ __forceinline__ bool rg_range(const CellRegionArgs& a, const int4 e, int* s0, int* s1) {
  return region_slab_range(e.x, e.y, e.z, e.w, a.b.x_min, a.b.y_min, a.b.y_max, a.b.side, s0, s1);
}

__global__ __launch_bounds__(256) void rg_zero_kernel(CellRegionArgs a) {
  if (!rg_go(a)) return;
  const size_t cells = (size_t)a.G * a.C;
  for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < cells; k += (size_t)gridDim.x * 256) a.census[k] = 0;
}

// the end of a region's run of edges: the odd lanes are inside it.  Called by every thread of the workgroup at once (the edge sequence is
// the workgroup's), so the ballots see whole waves.
__device__ __forceinline__ void rg_flush(const CellRegionArgs& a, int cur, bool odd, int cls, int& depth, int& top) {
  if (cur < 0) return;
  if (odd) { depth += 1; top = cur; }                   // the regions come in ascending order: the last one is the largest
  if (__ballot(odd && cls >= 0) == 0) return;
  for (int c = 0; c < a.C; ++c) {
    const int k = __popcll(__ballot(odd && cls == c));
    if (k && (threadIdx.x & 63) == 0) atomicAdd(&a.census[(size_t)cur * a.C + c], (unsigned long long)k);
  }
}

__global__ __launch_bounds__(REGION_STAGE) void rg_cross_kernel(CellRegionArgs a) {
  __shared__ int4 st_edge[REGION_STAGE];
  __shared__ int st_region[REGION_STAGE];
  __shared__ int next_row;
  if (!rg_go(a)) return;                                 // uniform
  const CellBin& g = a.b;
  const int tid = threadIdx.x, j = blockIdx.x * REGION_STAGE + tid;
  const bool have = j < g.n;
  const int4 me = have ? g.recs[j] : make_int4(0, 0, -1, -1);
  const int my_row = have ? (me.y - g.y_min) / g.side : INT_MAX;
  const int cls = have && (unsigned)me.z < (unsigned)a.C ? me.z : -1;
  int top = -1, depth = 0, onb = 0;
  if (tid == 0) next_row = my_row;                       // thread 0 has a record: the grid is ceil(n / 256) workgroups
  __syncthreads();
  int row = next_row;
  while (row != INT_MAX) {                               // the slabs that hold records of this workgroup, ascending
    const bool mine = my_row == row;
    const int k0 = a.slab_start[row], k1 = a.slab_start[row + 1];
    int cur = -1, parity = 0;
    for (int base = k0; base < k1; base += REGION_STAGE) {
      __syncthreads();                                   // the chunk before this one has been read by everyone
      if (base + tid < k1) {
        const int e = a.slots[base + tid];
        st_edge[tid] = a.edges[e];
        st_region[tid] = a.edge_region[e];
      }
      __syncthreads();
      const int m = min(REGION_STAGE, k1 - base);
      for (int k = 0; k < m; ++k) {
        const int r = __builtin_amdgcn_readfirstlane(st_region[k]);
        if (r != cur) {                                  // the same for every thread of the workgroup
          rg_flush(a, cur, mine && parity, cls, depth, top);
          cur = r; parity = 0;
        }
        const int4 ed = st_edge[k];
        if (mine) {
          parity ^= (int)region_crossed(ed.x, ed.y, ed.z, ed.w, me.x, me.y);
          onb |= (int)region_on_edge(ed.x, ed.y, ed.z, ed.w, me.x, me.y);
        }
      }
    }
    rg_flush(a, cur, mine && parity, cls, depth, top);
    __syncthreads();                                     // everyone has read next_row
    if (tid == 0) next_row = INT_MAX;
    __syncthreads();
    if (have && my_row > row) atomicMin(&next_row, my_row);
    __syncthreads();
    row = next_row;
  }
  if (have) { a.region[me.w] = top; a.depth[me.w] = depth; a.on_boundary[me.w] = (uint8_t)onb; }
}

}  // namespace

extern "C" int nuhtc_cell_regions(int device, const int32_t* points, const int32_t* labels, int64_t n, int num_classes, const int32_t* edges,
                                  const int32_t* edge_region, int64_t E, int64_t G, int slab, int64_t slot_cap, int x_min, int y_min, int x_max,
                                  int y_max, int32_t* region, int32_t* depth, uint8_t* on_boundary, int64_t* census, int64_t* slots, void* stream) {
  if (!cell_call_ok(n, MST_MAX_POINTS, num_classes, slab, x_min, y_min, x_max, y_max) || !region_call_ok(E, G, slab, slot_cap)) return NUHTC_E_INVALID;
  if (!slots || (n > 0 && (!points || !labels || !region || !depth || !on_boundary)) || (E > 0 && (!edges || !edge_region)) || (G > 0 && !census))
    return NUHTC_E_INVALID;
  if (reinterpret_cast<uintptr_t>(edges) & 15) return NUHTC_E_INVALID;        // an edge is one 16-byte load
  if (hipSetDevice(device) != hipSuccess) return NUHTC_E_HIP;
  hipStream_t st = (hipStream_t)stream;
  CellRegionArgs a;
  memset(&a, 0, sizeof(a));
  a.edges = reinterpret_cast<const int4*>(edges); a.edge_region = edge_region;
  a.E = (int)E; a.G = (int)G; a.C = num_classes; a.slot_cap = (unsigned long long)slot_cap;
  a.region = region; a.depth = depth; a.on_boundary = on_boundary; a.census = reinterpret_cast<unsigned long long*>(census);
  DevScratch tmp;      // every temporary of the call, freed on the way out
  int nchunk, schunk, *chunk_base;
  if (!edge_tables(a, points, labels, n, x_min, y_min, x_max, y_max, slab, slot_cap, tmp, st, &nchunk, &schunk, &chunk_base)) return NUHTC_E_HIP;
  if (n > 0) {
    ProfScope ps("cell_regions_bin", 0, 0, st);
    cellbin_launch(a.b, nchunk, st);
  }
  {
    ProfScope ps("cell_regions_edges", 0, 0, st);
    edge_launch(a, E, n, slot_cap, schunk, chunk_base, st);
  }
  {
    ProfScope ps("cell_regions_cross", 0, 0, st);
    if (G > 0) hipLaunchKernelGGL(rg_zero_kernel, dim3((unsigned)((G * num_classes + 255) / 256)), dim3(256), 0, st, a);
    if (n > 0) hipLaunchKernelGGL(rg_cross_kernel, dim3((unsigned)((n + REGION_STAGE - 1) / REGION_STAGE)), dim3(REGION_STAGE), 0, st, a);
  }
  return edge_finish(a, st, slots);
}
