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
//   edges      celledges.h (shared with cellmargin.hip), with edge_slab_range at R = 0 as the slabs an edge has a record in: clipped to
//              the box; an edge wholly above, below or left of the box meets none.  rg_check_kernel states M, the (edge, slab) records
//              the call needs, and every later kernel first compares M with the caller's slot_cap (rg_go); count, scan, emit, place
//              leave every slab's records in edge order, hence grouped by region, ascending.
//   crossing   rg_cross_kernel  rg_walk of celledges.h -- one workgroup per 256 consecutive point records, the edge records of each of
//                               their slabs staged through LDS 256 at a time, the region changes the same for every thread of the
//                               workgroup -- around RgCross: each thread carries (parity, depth, top, on-boundary), and at a region
//                               change the waves add their odd lanes to census, one integer atomic per (wave, class present) -- a
//                               ballot per class, as the cluster tables do.
//   outputs    every kernel that writes an output tests the flag and M first: a refused call leaves every output untouched, and so does a
//              call whose slot_cap is below M (it returns 0 and reports M: the caller calls once more).  With n == 0 the edges are still
//              checked and census is cleared.
// No kernel waits on another workgroup; every loop runs over a range of a table.  The entry point is edge_front and edge_run of
// celledges.h around its own checks, its four fields and its two launches.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, profiles/cell_regions_resources.txt): no scratch in any kernel; the crossing
// kernel holds 256 x (16 + 4) B of staged edges and one int, 5124 B of LDS, so LDS never bounds the occupancy (160 KiB per CU); a
// larger stage would only lengthen the time between barriers.
//
// Everything that decides an index, a side or a limit -- region_crossed, region_on_edge, edge_slab_range, region_edge_ok,
// region_call_ok (cellgrid_host.h) -- is plain C++, and tools/dev/cellregion_host_check.cpp runs exactly those functions on the host
// under -fsanitize=address,undefined against __int128 arithmetic and a direct loop.  The kernel code itself is not sanitized.
#include "celledges.h"

namespace {

struct CellRegionArgs : EdgeSlabs {   // grow == 0
  int32_t* region;                    // [n]
  int32_t* depth;                     // [n]
  uint8_t* on_boundary;               // [n]
  unsigned long long* census;         // [G][C]
};

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

// what a lane carries through rg_walk: the parity of the current region, and (depth, top, on-boundary) over all of them
struct RgCross {
  const CellRegionArgs& a;
  int parity, top, depth, onb;
  __device__ __forceinline__ void begin(int) {}
  __device__ __forceinline__ void stage(int, const int4&) {}
  __device__ __forceinline__ void reset() { parity = 0; }
  __device__ __forceinline__ void edge(int, const int4 ed, const int4 me) {
    parity ^= (int)region_crossed(ed.x, ed.y, ed.z, ed.w, me.x, me.y);
    onb |= (int)region_on_edge(ed.x, ed.y, ed.z, ed.w, me.x, me.y);
  }
  __device__ __forceinline__ void flush(int cur, bool mine, int cls) { rg_flush(a, cur, mine && parity, cls, depth, top); }
};

__global__ __launch_bounds__(REGION_STAGE) void rg_cross_kernel(CellRegionArgs a) {
  if (!rg_go(a)) return;                                 // uniform
  RgCross w{a, 0, -1, 0, 0};
  const int4 me = rg_walk(a, w);
  if (me.w >= 0) { a.region[me.w] = w.top; a.depth[me.w] = w.depth; a.on_boundary[me.w] = (uint8_t)w.onb; }
}

}  // namespace

extern "C" int nuhtc_cell_regions(int device, const int32_t* points, const int32_t* labels, int64_t n, int num_classes, const int32_t* edges,
                                  const int32_t* edge_region, int64_t E, int64_t G, int slab, int64_t slot_cap, int x_min, int y_min, int x_max,
                                  int y_max, int32_t* region, int32_t* depth, uint8_t* on_boundary, int64_t* census, int64_t* slots, void* stream) {
  if (!cell_call_ok(n, MST_MAX_POINTS, num_classes, slab, x_min, y_min, x_max, y_max) || !region_call_ok(E, G, slab, slot_cap)) return NUHTC_E_INVALID;
  if ((n > 0 && (!region || !depth || !on_boundary)) || (G > 0 && !census)) return NUHTC_E_INVALID;
  CellRegionArgs a{};
  EdgeCall h;
  const int rc = edge_front(a, h, device, points, labels, n, num_classes, edges, edge_region, E, G, 0, slab, slot_cap, x_min, y_min, x_max, y_max, slots, stream);
  if (rc) return rc;
  a.region = region; a.depth = depth; a.on_boundary = on_boundary; a.census = reinterpret_cast<unsigned long long*>(census);
  return edge_run(a, h, EdgeTags{"cell_regions_bin", "cell_regions_edges", "cell_regions_cross"},
                  [&] { hipLaunchKernelGGL(rg_zero_kernel, dim3((unsigned)((G * num_classes + 255) / 256)), dim3(256), 0, h.st, a); },
                  [&] { hipLaunchKernelGGL(rg_cross_kernel, dim3((unsigned)((n + REGION_STAGE - 1) / REGION_STAGE)), dim3(REGION_STAGE), 0, h.st, a); });
}
