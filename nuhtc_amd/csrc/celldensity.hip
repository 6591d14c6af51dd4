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
//   sites      one workgroup per tile of 16 x 16 sites, one thread per site, no atomics.  The sites are the first queries of this family
//              that are not the points themselves: a site may lie outside the box on any side, so its cell is a FLOOR (site_cell) and
//              its cell range is clamped and may be empty (site_cell_range); cell_sweep of cellbin.h assumes a query inside the box and is
//              not used.  Two kernels, chosen on the host per call by dens_route_staged:
//                staged  (dens_tile_kernel)  the tile's footprint grown by h covers a small rectangle of cells.  Row by row of that
//                        rectangle the workgroup copies the records into LDS, 256 at a time (one 16-byte load per record and thread),
//                        and every thread then takes each staged record against its own site: a broadcast LDS read instead of 256
//                        threads walking the same global ranges.  The label of a staged record is uniform over the workgroup.
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
// -DNUHTC_DENSITY_ROUTE, two alternating rounds in one process), ms per call staged / direct: pitch 64 px 0.71 / 0.49 uniform and 1.89 / 1.02
// clustered, pitch 32 px 0.78 / 0.64, pitch 16 px 1.04 / 1.10 -- the rule of dens_route_staged picks the faster one at each.
//
// Everything that decides an index or a limit -- the floor cell, the clamped range, the weight term, the window check and the route
// (cellgrid_host.h) -- is plain C++, and tools/dev/celldensity_host_check.cpp runs exactly those functions on the host under
// -fsanitize=address,undefined against counts over all points.  The kernel code itself is not sanitized.
#include <cstring>

#include "cellbin.h"

namespace {

constexpr int DENS_MAX_CELLS = 1 << 22;
constexpr int DENS_NT = DENS_TILE * DENS_TILE;          // 256 sites, one thread each
constexpr int DENS_STAGE_BYTES = DENS_NT * (int)sizeof(int4);

struct CellDensityArgs {
  CellBin b;                          // the points, the grid and the records in cell order (cellbin.h, one key per cell)
  int C, h, s, gx0, gy0, W, H, tiles_x;
  int32_t* count;                     // [C][H][W]
  unsigned long long* weight;         // [C][H][W]
};

inline int dens_lds_bytes(int C) { return DENS_STAGE_BYTES + C * DENS_NT * (int)(sizeof(unsigned long long) + sizeof(int)); }

// the site of this thread: (u, v) in the window, whether it exists, and its position in half pixels.  A thread past the window's edge
// takes the last site of its row or column (a valid coordinate) and writes nothing.
struct DensSite { int u, v, qx, qy; bool active; };
__device__ __forceinline__ DensSite dens_site_of(const CellDensityArgs& a) {
  DensSite t;
  const int tid = threadIdx.x;
  const int u = (int)(blockIdx.x % a.tiles_x) * DENS_TILE + (tid & (DENS_TILE - 1)), v = (int)(blockIdx.x / a.tiles_x) * DENS_TILE + tid / DENS_TILE;
  t.active = u < a.W && v < a.H;
  t.u = min(u, a.W - 1); t.v = min(v, a.H - 1);
  t.qx = (a.gx0 + t.u) * a.s; t.qy = (a.gy0 + t.v) * a.s;
  return t;
}

__device__ __forceinline__ void dens_take(const CellDensityArgs& a, const int4 o, const DensSite& me, int h2, int* cnt, unsigned long long* wt) {
  if ((unsigned)o.z >= (unsigned)a.C) return;            // a label outside 0 .. C - 1 is counted nowhere
  const int t = dens_term(o.x - me.qx, o.y - me.qy, a.h, h2);
  if (t < 0) return;
  cnt[o.z * DENS_NT] += 1;
  wt[o.z * DENS_NT] += (unsigned long long)t;
}

__device__ __forceinline__ void dens_write(const CellDensityArgs& a, const DensSite& me, const int* cnt, const unsigned long long* wt) {
  if (!me.active) return;
  const size_t plane = (size_t)a.H * a.W, at = (size_t)me.v * a.W + me.u;
  for (int c = 0; c < a.C; ++c) {
    a.count[c * plane + at] = cnt[c * DENS_NT];
    a.weight[c * plane + at] = wt[c * DENS_NT];
  }
}

// staged: the records of the tile's footprint through LDS, 256 at a time.  Every loop bound is the tile's, uniform over the workgroup:
// every thread meets every barrier.
__global__ __launch_bounds__(DENS_NT) void dens_tile_kernel(CellDensityArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dens_lds[];
  const CellBin& g = a.b;
  if (*g.flag) return;                                   // the binning met a point outside the box: nothing is written (uniform)
  const int tid = threadIdx.x, C = a.C, h = a.h, h2 = h * h;
  int4* __restrict__ stage = reinterpret_cast<int4*>(dens_lds);
  unsigned long long* wt = reinterpret_cast<unsigned long long*>(dens_lds + DENS_STAGE_BYTES) + tid;
  int* cnt = reinterpret_cast<int*>(dens_lds + DENS_STAGE_BYTES + C * DENS_NT * (int)sizeof(unsigned long long)) + tid;
  for (int c = 0; c < C; ++c) { cnt[c * DENS_NT] = 0; wt[c * DENS_NT] = 0; }          // this thread's own slots
  const DensSite me = dens_site_of(a);
  const int u0 = (int)(blockIdx.x % a.tiles_x) * DENS_TILE, v0 = (int)(blockIdx.x / a.tiles_x) * DENS_TILE;
  const int u1 = min(u0 + DENS_TILE, a.W) - 1, v1 = min(v0 + DENS_TILE, a.H) - 1;
  int cx0, cx1, cy0, cy1;
  site_cell_range((a.gx0 + u0) * a.s - h, (a.gx0 + u1) * a.s + h, g.x_min, g.side, g.ncx, &cx0, &cx1);
  site_cell_range((a.gy0 + v0) * a.s - h, (a.gy0 + v1) * a.s + h, g.y_min, g.side, g.ncy, &cy0, &cy1);
  if (cx0 > cx1) cy1 = cy0 - 1;                          // beside the grid: no row
  for (int gy = cy0; gy <= cy1; ++gy) {
    const int j0 = g.cell_start[gy * g.ncx + cx0], j1 = g.cell_start[gy * g.ncx + cx1 + 1];
    for (int base = j0; base < j1; base += DENS_NT) {
      __syncthreads();                                   // the chunk before this one has been read by everyone
      if (base + tid < j1) stage[tid] = g.recs[base + tid];
      __syncthreads();
      const int m = min(DENS_NT, j1 - base);
      for (int k = 0; k < m; ++k) dens_take(a, stage[k], me, h2, cnt, wt);
    }
  }
  dens_write(a, me, cnt, wt);
}

// direct: every site walks the cells its own disc can touch
__global__ __launch_bounds__(DENS_NT) void dens_site_kernel(CellDensityArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dens_lds[];
  const CellBin& g = a.b;
  if (*g.flag) return;
  const int tid = threadIdx.x, C = a.C, h = a.h, h2 = h * h;
  unsigned long long* wt = reinterpret_cast<unsigned long long*>(dens_lds + DENS_STAGE_BYTES) + tid;
  int* cnt = reinterpret_cast<int*>(dens_lds + DENS_STAGE_BYTES + C * DENS_NT * (int)sizeof(unsigned long long)) + tid;
  for (int c = 0; c < C; ++c) { cnt[c * DENS_NT] = 0; wt[c * DENS_NT] = 0; }
  const DensSite me = dens_site_of(a);
  if (!me.active) return;                                // no barrier in this kernel
  int cx0, cx1, cy0, cy1;
  site_cell_range(me.qx - h, me.qx + h, g.x_min, g.side, g.ncx, &cx0, &cx1);
  site_cell_range(me.qy - h, me.qy + h, g.y_min, g.side, g.ncy, &cy0, &cy1);
  if (cx0 > cx1) cy1 = cy0 - 1;
  for (int gy = cy0; gy <= cy1; ++gy) {
    const int j0 = g.cell_start[gy * g.ncx + cx0], j1 = g.cell_start[gy * g.ncx + cx1 + 1];
    for (int j = j0; j < j1; ++j) dens_take(a, g.recs[j], me, h2, cnt, wt);
  }
  dens_write(a, me, cnt, wt);
}

}  // namespace

extern "C" int nuhtc_cell_density(int device, const int32_t* points, const int32_t* labels, int64_t n, int num_classes, int h, int s, int gx0,
                                  int gy0, int W, int H, int x_min, int y_min, int x_max, int y_max, int32_t* count, int64_t* weight, void* stream) {
  if (!cell_call_ok(n, MST_MAX_POINTS, num_classes, h, x_min, y_min, x_max, y_max) || !dens_window_ok(s, gx0, gy0, W, H)) return NUHTC_E_INVALID;
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
  a.C = num_classes; a.h = h; a.s = s; a.gx0 = gx0; a.gy0 = gy0; a.W = W; a.H = H;
  a.tiles_x = (W + DENS_TILE - 1) / DENS_TILE;
  a.count = count; a.weight = reinterpret_cast<unsigned long long*>(weight);
  DevScratch tmp;      // every temporary of the call, freed on the way out
  const int nchunk = cellbin_setup(a.b, points, labels, (int)n, x_min, y_min, x_max, y_max, h, DENS_MAX_CELLS, 1, tmp, st);
  if (!nchunk) return NUHTC_E_HIP;
  const unsigned tiles = (unsigned)a.tiles_x * (unsigned)((H + DENS_TILE - 1) / DENS_TILE);        // at most 2^24 (W * H <= 2^24)
#ifdef NUHTC_DENSITY_ROUTE                                // dev probe: -DNUHTC_DENSITY_ROUTE=1 staged, =2 direct, whatever the shape
  const bool staged = NUHTC_DENSITY_ROUTE == 1;
#else
  const bool staged = dens_route_staged(s, h, a.b.side);
#endif
  {
    ProfScope ps("cell_density_bin", 0, 0, st);
    cellbin_launch(a.b, nchunk, st);
  }
  {
    ProfScope ps(staged ? "cell_density_tile" : "cell_density_site", 0, 0, st);
    if (staged) hipLaunchKernelGGL(dens_tile_kernel, dim3(tiles), dim3(DENS_NT), dens_lds_bytes(a.C), st, a);
    else hipLaunchKernelGGL(dens_site_kernel, dim3(tiles), dim3(DENS_NT), dens_lds_bytes(a.C), st, a);
  }
  return cellbin_finish(a.b, st);
}
