// Margin bands (gfx950): the nuclei of each class by distance to the boundary of an annotated region, inside it and outside it -- the
// invasive-margin or infiltration profile ("how many lymphocytes lie within 0-50, 50-100, .. um of the tumour boundary").  A sibling of
// the region census (cellregion.hip).
//
// Definition (nuhtc_amd/margin.py holds it in full, with the brute-force restatement `margin_reference`): the inputs of the region census
// -- n points in HALF pixels (|p| < 2^27, n <= 2^24), one label each, C classes (1 .. 14), G regions (<= 2^16) as a flat table of E edges
// (<= 2^22) with edge_region non-decreasing -- and B thresholds (1 .. 32), strictly increasing within 1 .. 16384 half pixels.
// near(p, edge, e) is "the distance from p to the segment is at most e" in exact integers (margin_near of cellgrid_host.h: an int64
// compare past the ends of the edge, a 128-bit compare cross^2 <= e^2 * len^2 beside it).  band(p, g) = the smallest t with some edge of
// g near at e_t, B when none; inside(p, g) is the census's even-odd, half-open rule (region_crossed).  band_census[g][side][t][c] = the
// points of label c with band(p, g) == t and inside(p, g) == side; census[g][c] = the points inside g; per point the smallest band over
// the regions, the smallest region that attains it and the side there.  Integer compares and integer adds only: a pure function of the
// input, bitwise the same on every call.
//
// Stages, all on the caller's stream:
//   binning    cellbin.h, reach slab, one key per cell: a grid row is a slab and its points are one contiguous run of the records.
//   edges      celledges.h with margin_slab_range: an edge has one record per slab of the box that its y-range GROWN by R = e_{B-1}
//              meets, none when the grown range misses the box in y or the edge lies wholly left of x_min - R.  A point of a slab
//              therefore sees every edge that can straddle it and every edge within R of it.  M, slot_cap and *slots as in the census.
//   sweep      mg_sweep_kernel  one workgroup per 256 consecutive point records; the slab's edge records go through LDS 256 at a time
//                               (the edge, its bounding box and its region, gathered once per workgroup) in edge order, so the region
//                               changes are uniform over the workgroup.  Each lane carries (parity, best band) for the current region.
//                               Per edge: the parity as in the census; a box reject against the threshold below the lane's best band
//                               (four compares); only then margin_measure once and margin_within downwards while the band improves.
//                               At a region change the lanes with a band add to band_census and the odd lanes to census -- per wave,
//                               one int64 atomic per (side, band, class) present, the count a popcount of a ballot, so no 32-bit
//                               counter exists at all -- and each lane folds (band, region, side) into its per-nucleus minimum.
//   outputs    every kernel that writes an output tests the flag and M first: a refused call leaves every output untouched, and so does
//              a call whose slot_cap is below M (it returns 0 and reports M).  With n == 0 the edges are still checked and the two
//              tables are cleared.
// No kernel waits on another workgroup; every loop runs over a range of a table.  The thresholds travel in the argument block and sit
// in LDS during the sweep.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, profiles/cell_margin_resources.txt): no scratch in any kernel.
//
// Everything that decides a distance, an index or a limit -- margin_measure, margin_within, margin_box_near, margin_slab_range,
// margin_thresholds_ok, margin_call_ok (cellgrid_host.h) -- is plain C++, and tools/dev/cellmargin_host_check.cpp runs exactly those
// functions on the host under -fsanitize=address,undefined against __int128 arithmetic and direct loops.  The kernel code itself is not
// sanitized.
#include <climits>
#include <cstring>

#include "celledges.h"

namespace {

struct CellMarginArgs {
  CellBin b;                          // the points, the grid and the records in cell order (cellbin.h, one key per cell)
  const int4* edges;                  // [E] (ax, ay, bx, by) half pixels
  const int32_t* edge_region;         // [E] non-decreasing
  int E, G, C;
  int have_grid;                      // 0 with n == 0: the edges are checked, no slab is counted
  unsigned long long slot_cap;        // the (edge, slab) records the caller left room for
  unsigned long long* total;          // M: the records the call needs
  int* slab_count;                    // as in CellRegionArgs
  int* slab_start;
  int2* emitted;
  int* slots;
  int B, R;                           // the thresholds and the largest of them
  int thr[MARGIN_MAX_BANDS];          // [B] strictly increasing
  unsigned long long* band_census;    // [G][2][B][C]
  unsigned long long* census;         // [G][C]
  int32_t* band;                      // [n]
  int32_t* band_region;               // [n]
  uint8_t* band_inside;               // [n]
};

__device__ __forceinline__ bool rg_range(const CellMarginArgs& a, const int4 e, int* s0, int* s1) {
  return margin_slab_range(e.x, e.y, e.z, e.w, a.R, a.b.x_min, a.b.y_min, a.b.y_max, a.b.side, s0, s1);
}

__global__ __launch_bounds__(256) void mg_zero_kernel(CellMarginArgs a) {
  if (!rg_go(a)) return;
  const size_t bands = (size_t)a.G * 2 * a.B * a.C, cells = bands + (size_t)a.G * a.C;
  for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < cells; k += (size_t)gridDim.x * 256) {
    if (k < bands) a.band_census[k] = 0; else a.census[k - bands] = 0;
  }
}

// table[key] += the lanes of this wave that hold `key`, for every key >= 0 present: one int64 atomic per (wave, key), the count a
// popcount of a ballot (at most 64).  Called by whole waves.
__device__ __forceinline__ void mg_wave_add(unsigned long long* table, int key) {
  unsigned long long left = __ballot(key >= 0);
  while (left) {                                        // uniform over the wave
    const int lead = __ffsll((long long)left) - 1;
    const int k = __shfl(key, lead, 64);
    const unsigned long long same = __ballot(key == k);
    if ((int)(threadIdx.x & 63) == lead) atomicAdd(&table[k], (unsigned long long)__popcll(same));
    left &= ~same;
  }
}

// the end of a region's run of edges.  Called by every thread of the workgroup at once (the edge sequence is the workgroup's).
__device__ __forceinline__ void mg_flush(const CellMarginArgs& a, int cur, bool mine, int parity, int best, int cls, int& nb, int& nr, int& ni) {
  if (cur < 0) return;
  const bool near = mine && best < a.B;
  if (near && best < nb) { nb = best; nr = cur; ni = parity; }     // the regions come ascending: a tie keeps the smaller one
  mg_wave_add(a.band_census + (size_t)cur * 2 * a.B * a.C, near && cls >= 0 ? (parity * a.B + best) * a.C + cls : -1);
  mg_wave_add(a.census + (size_t)cur * a.C, mine && parity && cls >= 0 ? cls : -1);
}

__global__ __launch_bounds__(REGION_STAGE) void mg_sweep_kernel(CellMarginArgs a) {
  __shared__ int4 st_edge[REGION_STAGE];
  __shared__ int4 st_box[REGION_STAGE];
  __shared__ int st_region[REGION_STAGE];
  __shared__ int thr[MARGIN_MAX_BANDS];
  __shared__ int next_row;
  if (!rg_go(a)) return;                                 // uniform
  const CellBin& g = a.b;
  const int tid = threadIdx.x, j = blockIdx.x * REGION_STAGE + tid;
  const bool have = j < g.n;
  const int4 me = have ? g.recs[j] : make_int4(0, 0, -1, -1);
  const int my_row = have ? (me.y - g.y_min) / g.side : INT_MAX;
  const int cls = have && (unsigned)me.z < (unsigned)a.C ? me.z : -1;
  const int B = a.B;
  int nb = B, nr = -1, ni = 0;
  if (tid < B) thr[tid] = a.thr[tid];
  if (tid == 0) next_row = my_row;                       // thread 0 has a record: the grid is ceil(n / 256) workgroups
  __syncthreads();
  int row = next_row;
  while (row != INT_MAX) {                               // the slabs that hold records of this workgroup, ascending
    const bool mine = my_row == row;
    const int k0 = a.slab_start[row], k1 = a.slab_start[row + 1];
    int cur = -1, parity = 0, best = B;
    for (int base = k0; base < k1; base += REGION_STAGE) {
      __syncthreads();                                   // the chunk before this one has been read by everyone
      if (base + tid < k1) {
        const int e = a.slots[base + tid];
        const int4 ed = a.edges[e];
        st_edge[tid] = ed;
        st_box[tid] = make_int4(min(ed.x, ed.z), min(ed.y, ed.w), max(ed.x, ed.z), max(ed.y, ed.w));
        st_region[tid] = a.edge_region[e];
      }
      __syncthreads();
      const int m = min(REGION_STAGE, k1 - base);
      for (int k = 0; k < m; ++k) {
        const int r = __builtin_amdgcn_readfirstlane(st_region[k]);
        if (r != cur) {                                  // the same for every thread of the workgroup
          mg_flush(a, cur, mine, parity, best, cls, nb, nr, ni);
          cur = r; parity = 0; best = B;
        }
        if (mine) {
          const int4 ed = st_edge[k];
          parity ^= (int)region_crossed(ed.x, ed.y, ed.z, ed.w, me.x, me.y);
          if (best > 0) {
            const int4 bx = st_box[k];
            if (margin_box_near(bx.x, bx.y, bx.z, bx.w, me.x, me.y, thr[best - 1])) {
              uint64_t q, l2;
              margin_measure(ed.x, ed.y, ed.z, ed.w, me.x, me.y, &q, &l2);
              while (best > 0 && margin_within(q, l2, thr[best - 1])) --best;
            }
          }
        }
      }
    }
    mg_flush(a, cur, mine, parity, best, cls, nb, nr, ni);
    __syncthreads();                                     // everyone has read next_row
    if (tid == 0) next_row = INT_MAX;
    __syncthreads();
    if (have && my_row > row) atomicMin(&next_row, my_row);
    __syncthreads();
    row = next_row;
  }
  if (have) { a.band[me.w] = nb; a.band_region[me.w] = nr; a.band_inside[me.w] = (uint8_t)ni; }
}

}  // namespace

extern "C" int nuhtc_cell_margin(int device, const int32_t* points, const int32_t* labels, int64_t n, int num_classes, const int32_t* edges,
                                 const int32_t* edge_region, int64_t E, int64_t G, const int32_t* thresholds, int B, int slab, int64_t slot_cap,
                                 int x_min, int y_min, int x_max, int y_max, int64_t* band_census, int64_t* census, int32_t* band,
                                 int32_t* band_region, uint8_t* band_inside, int64_t* slots, void* stream) {
  if (!cell_call_ok(n, MST_MAX_POINTS, num_classes, slab, x_min, y_min, x_max, y_max) || !margin_call_ok(E, G, slab, slot_cap, thresholds, B))
    return NUHTC_E_INVALID;
  if (!slots || (n > 0 && (!points || !labels || !band || !band_region || !band_inside)) || (E > 0 && (!edges || !edge_region)) ||
      (G > 0 && (!band_census || !census)))
    return NUHTC_E_INVALID;
  if (reinterpret_cast<uintptr_t>(edges) & 15) return NUHTC_E_INVALID;        // an edge is one 16-byte load
  if (hipSetDevice(device) != hipSuccess) return NUHTC_E_HIP;
  hipStream_t st = (hipStream_t)stream;
  CellMarginArgs a;
  memset(&a, 0, sizeof(a));
  a.edges = reinterpret_cast<const int4*>(edges); a.edge_region = edge_region;
  a.E = (int)E; a.G = (int)G; a.C = num_classes; a.slot_cap = (unsigned long long)slot_cap;
  a.B = B; a.R = thresholds[B - 1];
  for (int k = 0; k < B; ++k) a.thr[k] = thresholds[k];
  a.band_census = reinterpret_cast<unsigned long long*>(band_census); a.census = reinterpret_cast<unsigned long long*>(census);
  a.band = band; a.band_region = band_region; a.band_inside = band_inside;
  DevScratch tmp;      // every temporary of the call, freed on the way out
  int nchunk, schunk, *chunk_base;
  if (!edge_tables(a, points, labels, n, x_min, y_min, x_max, y_max, slab, slot_cap, tmp, st, &nchunk, &schunk, &chunk_base)) return NUHTC_E_HIP;
  if (n > 0) {
    ProfScope ps("cell_margin_bin", 0, 0, st);
    cellbin_launch(a.b, nchunk, st);
  }
  {
    ProfScope ps("cell_margin_edges", 0, 0, st);
    edge_launch(a, E, n, slot_cap, schunk, chunk_base, st);
  }
  {
    ProfScope ps("cell_margin_sweep", 0, 0, st);
    if (G > 0) {
      const int64_t cells = G * (2 * B + 1) * num_classes;                    // at most 2^16 * 65 * 14
      hipLaunchKernelGGL(mg_zero_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, a);
    }
    if (n > 0) hipLaunchKernelGGL(mg_sweep_kernel, dim3((unsigned)((n + REGION_STAGE - 1) / REGION_STAGE)), dim3(REGION_STAGE), 0, st, a);
  }
  return edge_finish(a, st, slots);
}
