// Nucleus density maps of a slide (gfx950): class-wise kernel rasters of the nucleus centres on a lattice anchored at the slide's origin.
//
// Definition (nuhtc_amd/density.py holds it in full, with the int64 brute-force restatement `density_reference`): n points in HALF pixels
// (|p| < 2^27, n <= 2^24), one label each, C classes (1 .. 14), a bandwidth h (1 .. 16384) and a pitch s (1 .. 2^20) in half pixels, and a
// window gx0, gy0, W, H in lattice units (W * H <= 2^24, every site coordinate |g * s| < 2^28).  Site (u, v) lies at
// q = ((gx0 + u) * s, (gy0 + v) * s).  count[c][v][u] is the number of points of label c with d2(q, p) <= h * h (inclusive), weight[c][v][u]
// the sum of h * h - d2(q, p) over them: the un-normalised Epanechnikov kernel in exact integers.  A label outside 0 .. C - 1 is counted
// nowhere.  Integer adds only and one owner per site: a pure function of the input, bitwise the same on every call.
//
// Stages, all on the caller's stream:
//   geometry   on the HOST from the caller's bounding box (cell_grid_side of cellgrid_host.h): cells of side >= h, at most 2^22 of them.
//   binning    cellbin.h, reach h, ONE key per cell: the records of a row of neighbouring cells are one contiguous range, whatever
//              their labels.
//   sites      one workgroup per tile of 16 x 16 sites, one thread per site, no atomics: the lattice, a thread's site and the sweep are
//              cellsites.h's (site_sweep, with the barrier contract), shared with the territories; dens_take and dens_write are this
//              file's.  Two kernels, chosen on the host per call by site_route:
//                staged  (dens_tile_kernel)  the records of the tile's footprint grown by h through LDS, 256 at a time: a broadcast LDS
//                        read instead of 256 threads walking the same global ranges.
//                direct  (dens_site_kernel)  every thread walks the (at most 3 x 3) cells its own disc can touch, straight from global
//                        memory: fewer records per site as soon as the sites of a tile lie far apart (a pitch above about h / 5).
//              The per-class accumulators are LDS, slot-major (class c of thread tid at word c * 256 + tid: no bank conflicts), 12 bytes
//              per class and thread; C pairs of registers indexed by a label would go to scratch.  At the end every site writes all
//              C planes, zeros included.
//   outputs    both kernels test the binning's flag first, so a point outside the stated box leaves every output untouched
//              (NUHTC_E_INVALID).  With n == 0 the outputs are cleared by two memsets and nothing is launched.
//
// No counter can overflow for any accepted input (cellgrid_host.h has the argument): a term is at most 2^28 and a weight below 2^52.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, profiles/cell_density_resources.txt): no scratch in either kernel; LDS per
// workgroup is dynamic, dens_lds_bytes(C) = 4096 + 3072 C bytes: 19,456 B at the tool's C = 5, 47,104 B at C = 14; both kernels take 30
// VGPRs, 8 waves per SIMD.  Measured on 10^6 centres, 128 px bandwidth (profiles/cell_density.json, both kernels forced with
// -DNUHTC_SITE_ROUTE, two alternating rounds in one process), ms per call staged / direct: pitch 64 px 0.71 / 0.49 uniform and 1.89 / 1.02
// clustered, pitch 32 px 0.78 / 0.64, pitch 16 px 1.04 / 1.10 -- the rule of site_route_staged picks the faster one at each.
// The two s_nop in front of the staged sweep keep the loop over the staged records at the byte offset it had when the sweep was written
// out in dens_tile_kernel (the shared form drops a redundant compare and branch behind the second barrier: 8 bytes).  Measured
// (profiles/cell_density.json, site_sweep_vs_parent, unpadded_staged): the same instructions 8 bytes earlier took 1 - 4 % longer per call
// at every forced-staged shape; with the padding cell_density_tile takes what the parent's took (stage_rounds there: 0.608 - 0.609 ms
// beside 0.609 - 0.613).  They run once per workgroup; look at the offset again (llvm-objdump -d) when the prologue of site_sweep or of
// this kernel changes.  The territories' staged loop moved by 4 bytes and cell_territory_owner measured the same (profiles/cell_territory.json).
//
// Everything that decides an index or a limit -- the floor cell, the clamped cells of a footprint, the weight term, the window check and
// the route (cellgrid_host.h) -- is plain C++, and tools/dev/celldensity_host_check.cpp calls exactly those functions on the host under
// -fsanitize=address,undefined against counts over all points.  The kernel code itself is not sanitized.
#include <cstring>

#include "cellsites.h"

namespace {

constexpr int DENS_MAX_CELLS = 1 << 22;

struct CellDensityArgs {
  CellBin b;                          // the points, the grid and the records in cell order (cellbin.h, one key per cell)
  SiteLattice t;                      // reach = the bandwidth h
  int C;
  int32_t* count;                     // [C][H][W]
  unsigned long long* weight;         // [C][H][W]
};

inline int dens_lds_bytes(int C) { return SITE_STAGE_BYTES + C * SITE_NT * (int)(sizeof(unsigned long long) + sizeof(int)); }

// this thread's own accumulators behind the stage: slot-major, all zero
struct DensSlots { int* cnt; unsigned long long* wt; };
__device__ __forceinline__ DensSlots dens_slots(unsigned char* lds, int C) {
  const int tid = threadIdx.x;
  DensSlots m;
  m.wt = reinterpret_cast<unsigned long long*>(lds + SITE_STAGE_BYTES) + tid;
  m.cnt = reinterpret_cast<int*>(lds + SITE_STAGE_BYTES + C * SITE_NT * (int)sizeof(unsigned long long)) + tid;
  for (int c = 0; c < C; ++c) { m.cnt[c * SITE_NT] = 0; m.wt[c * SITE_NT] = 0; }
  return m;
}

__device__ __forceinline__ void dens_take(const CellDensityArgs& a, const int4 o, const Site& me, int h2, const DensSlots& m) {
  if ((unsigned)o.z >= (unsigned)a.C) return;            // a label outside 0 .. C - 1 is counted nowhere
  const int t = dens_term(o.x - me.qx, o.y - me.qy, a.t.reach, h2);
  if (t < 0) return;
  m.cnt[o.z * SITE_NT] += 1;
  m.wt[o.z * SITE_NT] += (unsigned long long)t;
}

__device__ __forceinline__ void dens_write(const CellDensityArgs& a, const Site& me, const DensSlots& m) {
  if (!me.active) return;
  const size_t plane = (size_t)a.t.H * a.t.W, at = (size_t)me.v * a.t.W + me.u;
  for (int c = 0; c < a.C; ++c) {
    a.count[c * plane + at] = m.cnt[c * SITE_NT];
    a.weight[c * plane + at] = m.wt[c * SITE_NT];
  }
}

// both kernels: the flag, the accumulators, the sweep of cellsites.h (staged through the front of the LDS, or direct), the write
template <bool STAGED>
__device__ __forceinline__ void dens_sites(const CellDensityArgs& a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dens_lds[];
  if (*a.b.flag) return;                                 // the binning met a point outside the box: nothing is written (uniform)
  const int h2 = a.t.reach * a.t.reach;
  const DensSlots m = dens_slots(dens_lds, a.C);
  const Site me = site_of(a.t);
  if (STAGED) asm volatile("s_nop 0\n\ts_nop 0");        // once per workgroup: the loop's byte offset, see the header
  site_sweep<STAGED>(a.b, a.t, me, reinterpret_cast<int4*>(dens_lds),[&](const int4& o) { dens_take(a, o, me, h2, m); });
  dens_write(a, me, m);
}
__global__ __launch_bounds__(SITE_NT) void dens_tile_kernel(CellDensityArgs a) { dens_sites<true>(a); }
__global__ __launch_bounds__(SITE_NT) void dens_site_kernel(CellDensityArgs a) { dens_sites<false>(a); }

}  // namespace

extern "C" int nuhtc_cell_density(int device, const int32_t* points, const int32_t* labels, int64_t n, int num_classes, int h, int s, int gx0,
                                  int gy0, int W, int H, int x_min, int y_min, int x_max, int y_max, int32_t* count, int64_t* weight, void* stream) {
  if (!cell_call_ok(n, MST_MAX_POINTS, num_classes, h, x_min, y_min, x_max, y_max) || !site_window_ok(s, gx0, gy0, W, H, DENS_MAX_SITES)) return NUHTC_E_INVALID;
  if (!count || !weight || (n > 0 && (!points || !labels))) return NUHTC_E_INVALID;
  if (hipSetDevice(device) != hipSuccess) return NUHTC_E_HIP;
  hipStream_t st = (hipStream_t)stream;
  const size_t sites = (size_t)num_classes * H * W;
  if (n == 0) {
    if (hipMemsetAsync(count, 0, sites * sizeof(int32_t), st) != hipSuccess || hipMemsetAsync(weight, 0, sites * sizeof(int64_t), st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
      return NUHTC_E_HIP;
    return 0;
  }
  CellDensityArgs a;
  memset(&a, 0, sizeof(a));
  a.t = site_lattice(h, s, gx0, gy0, W, H); a.C = num_classes;
  a.count = count; a.weight = reinterpret_cast<unsigned long long*>(weight);
  DevScratch tmp;      // every temporary of the call, freed on the way out
  const int nchunk = cellbin_setup(a.b, points, labels, (int)n, x_min, y_min, x_max, y_max, h, DENS_MAX_CELLS, 1, tmp, st);
  if (!nchunk) return NUHTC_E_HIP;
  const bool staged = site_route(s, h, a.b.side);
  {
    ProfScope ps("cell_density_bin", 0, 0, st);
    cellbin_launch(a.b, nchunk, st);
  }
  {
    ProfScope ps(staged ? "cell_density_tile" : "cell_density_site", 0, 0, st);
    site_launch(staged, dens_tile_kernel, dens_site_kernel, site_tiles(W, H), dens_lds_bytes(a.C), st, a);
  }
  return cellbin_finish(a.b, st);
}
