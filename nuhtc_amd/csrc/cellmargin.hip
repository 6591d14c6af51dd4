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
//   edges      celledges.h with grow = R = e_{B-1}: an edge has one record per slab of the box that its y-range GROWN by R meets
//              (edge_slab_range), none when the grown range misses the box in y or the edge lies wholly left of x_min - R.  A point of a
//              slab therefore sees every edge that can straddle it and every edge within R of it.  M, slot_cap and *slots as in the census.
//   sweep      mg_sweep_kernel  rg_walk of celledges.h, the walk of the census -- one workgroup per 256 consecutive point records; the
//                               slab's edge records go through LDS 256 at a time in edge order, so the region changes are uniform over
//                               the workgroup -- around MgSweep, which stages the edge's bounding box beside the walk's edge and region
//                               (gathered once per workgroup).  Each lane carries (parity, best band) for the current region.
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
// Everything that decides a distance, an index or a limit -- margin_measure, margin_within, margin_box_near, edge_slab_range,
// margin_thresholds_ok, margin_call_ok (cellgrid_host.h) -- is plain C++, and tools/dev/cellmargin_host_check.cpp runs exactly those
// functions on the host under -fsanitize=address,undefined against __int128 arithmetic and direct loops.  The kernel code itself is not
// sanitized.
#include "celledges.h"

namespace {

struct CellMarginArgs : EdgeSlabs {   // grow == R = thr[B - 1]
  int B;                              // the thresholds
  int thr[MARGIN_MAX_BANDS];          // [B] strictly increasing
  unsigned long long* band_census;    // [G][2][B][C]
  unsigned long long* census;         // [G][C]
  int32_t* band;                      // [n]
  int32_t* band_region;               // [n]
  uint8_t* band_inside;               // [n]
};

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

// what a lane carries through rg_walk: (parity, best band) of the current region, and its minimum (band, region, side) over all of them.
// box and thr are the file's LDS beside the walk's: the bounding box of every staged edge, and the thresholds.
struct MgSweep {
  const CellMarginArgs& a;
  int4* box;
  int* thr;
  int parity, best, nb, nr, ni;
  // The four s_nop keep the loop over the staged edges (1.2 KiB of code) at the byte offset 0x3bc it had when the walk was written out in
  // this kernel.  Measured on gfx950 (profiles/cell_margin.json, slab_walk_vs_parent): with the same instructions at 0x308 or 0x38c the
  // sweep took 1.3 - 1.8 % longer, at 0x3bc it takes what it took.  They run once per workgroup; look at the offset again (llvm-objdump
  // -d) when the prologue of rg_walk or of this kernel changes.
  __device__ __forceinline__ void begin(int tid) {
    if (tid < a.B) thr[tid] = a.thr[tid];
    asm volatile("s_nop 0\n\ts_nop 0\n\ts_nop 0\n\ts_nop 0");
  }
  __device__ __forceinline__ void stage(int tid, const int4 ed) {
    box[tid] = make_int4(min(ed.x, ed.z), min(ed.y, ed.w), max(ed.x, ed.z), max(ed.y, ed.w));
  }
  __device__ __forceinline__ void reset() { parity = 0; best = a.B; }
  __device__ __forceinline__ void edge(int k, const int4 ed, const int4 me) {
    parity ^= (int)region_crossed(ed.x, ed.y, ed.z, ed.w, me.x, me.y);
    if (best > 0) {
      const int4 bx = box[k];
      if (margin_box_near(bx.x, bx.y, bx.z, bx.w, me.x, me.y, thr[best - 1])) {
        uint64_t q, l2;
        margin_measure(ed.x, ed.y, ed.z, ed.w, me.x, me.y, &q, &l2);
        while (best > 0 && margin_within(q, l2, thr[best - 1])) --best;
      }
    }
  }
  // the end of a region's run of edges
  __device__ __forceinline__ void flush(int cur, bool mine, int cls) {
    if (cur < 0) return;
    const bool near = mine && best < a.B;
    if (near && best < nb) { nb = best; nr = cur; ni = parity; }     // the regions come ascending: a tie keeps the smaller one
    mg_wave_add(a.band_census + (size_t)cur * 2 * a.B * a.C, near && cls >= 0 ? (parity * a.B + best) * a.C + cls : -1);
    mg_wave_add(a.census + (size_t)cur * a.C, mine && parity && cls >= 0 ? cls : -1);
  }
};

__global__ __launch_bounds__(REGION_STAGE) void mg_sweep_kernel(CellMarginArgs a) {
  __shared__ int4 st_box[REGION_STAGE];
  __shared__ int thr[MARGIN_MAX_BANDS];
  if (!rg_go(a)) return;                                 // uniform
  MgSweep w{a, st_box, thr, 0, a.B, a.B, -1, 0};
  const int4 me = rg_walk(a, w);
  if (me.w >= 0) { a.band[me.w] = w.nb; a.band_region[me.w] = w.nr; a.band_inside[me.w] = (uint8_t)w.ni; }
}

}  // namespace

extern "C" int nuhtc_cell_margin(int device, const int32_t* points, const int32_t* labels, int64_t n, int num_classes, const int32_t* edges,
                                 const int32_t* edge_region, int64_t E, int64_t G, const int32_t* thresholds, int B, int slab, int64_t slot_cap,
                                 int x_min, int y_min, int x_max, int y_max, int64_t* band_census, int64_t* census, int32_t* band,
                                 int32_t* band_region, uint8_t* band_inside, int64_t* slots, void* stream) {
  if (!cell_call_ok(n, MST_MAX_POINTS, num_classes, slab, x_min, y_min, x_max, y_max) || !margin_call_ok(E, G, slab, slot_cap, thresholds, B))
    return NUHTC_E_INVALID;
  if ((n > 0 && (!band || !band_region || !band_inside)) || (G > 0 && (!band_census || !census))) return NUHTC_E_INVALID;
  CellMarginArgs a{};
  EdgeCall h;
  const int rc = edge_front(a, h, device, points, labels, n, num_classes, edges, edge_region, E, G, thresholds[B - 1], slab, slot_cap, x_min, y_min,
                            x_max, y_max, slots, stream);
  if (rc) return rc;
  a.B = B;
  for (int k = 0; k < B; ++k) a.thr[k] = thresholds[k];
  a.band_census = reinterpret_cast<unsigned long long*>(band_census); a.census = reinterpret_cast<unsigned long long*>(census);
  a.band = band; a.band_region = band_region; a.band_inside = band_inside;
  const int64_t cells = G * (2 * B + 1) * num_classes;                        // at most 2^16 * 65 * 14
  return edge_run(a, h, EdgeTags{"cell_margin_bin", "cell_margin_edges", "cell_margin_sweep"},
                  [&] { hipLaunchKernelGGL(mg_zero_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, h.st, a); },
                  [&] { hipLaunchKernelGGL(mg_sweep_kernel, dim3((unsigned)((n + REGION_STAGE - 1) / REGION_STAGE)), dim3(REGION_STAGE), 0, h.st, a); });
}
