// Nucleus territories of a slide (gfx950): the nearest-nucleus raster of the nucleus centres on the lattice of the density maps -- which
// nucleus, and so which cell class, each piece of the plane belongs to.  The Voronoi family in raster form: exact integers, no
// circumcentre and no tie rule beyond "the smaller row".
//
// Definition (nuhtc_amd/territory.py holds it in full, with the int64 brute-force restatement `territory_reference`): n points in HALF
// pixels (|p| < 2^27, n <= 2^24), one label each, C classes (1 .. 14), a reach R (1 .. 16384) and a pitch s (1 .. 2^20) in half pixels,
// and a window gx0, gy0, W, H in lattice units (W * H <= 2^28, every site coordinate |g * s| < 2^28).  Site (u, v) lies at
// q = ((gx0 + u) * s, (gy0 + v) * s).  The rows with a label in 0 .. C - 1 compete; owner[v][u] is the competitor that minimises
// (d2(q, p_i), i) among those with d2 <= R * R (inclusive; a tie goes to the smaller row), or -1; nearest_d2[v][u] is that d2, or -1.
// The tallies are over the window: area and border per row, open per row, contact by class pair, the census of the sites by class.
// A minimum of 64-bit keys and integer adds only: a pure function of the input, bitwise the same on every call.
//
// Stages, all on the caller's stream:
//   geometry   on the HOST from the caller's bounding box (cell_grid_side of cellgrid_host.h): cells of side >= R, at most 2^22 of them.
//   binning    cellbin.h, reach R, ONE key per cell, and the zeroing of the per-row arrays and the tables (terr_zero_kernel, AFTER the
//              binning and only if its flag is clear).
//   owner      one workgroup per tile of 16 x 16 sites, one thread per site, no atomics: the lattice, a thread's site and the sweep are
//              cellsites.h's (site_sweep, with the barrier contract), shared with the density maps; terr_take and terr_write are this
//              file's.  Every thread holds its best key (terr_key: d2 in the high word, the row in the low one) in two registers.  Two
//              kernels, chosen on the host per call by site_route:
//                staged  (terr_tile_kernel)  the records of the tile's footprint grown by R through LDS 256 at a time, every thread
//                        against every staged record.  LDS is the 4 KiB stage only.
//                direct  (terr_site_kernel)  every thread walks the (at most 3 x 3) cells its own disc can touch.
//   tally      one thread per site in row-major order (a grid-stride loop over blocks of 256 sites) once the owner map is complete:
//              its own owner and the four neighbours' inside the window.  area / border / open go to the per-row arrays by integer
//              atomics, ONE per run of equal owners among the lanes of a wave (ballots: the run's length and the border sites in it by
//              popcount); contact and the census of the sites go to the workgroup's 32-bit LDS table [(C + 1)][(C + 1)] (terr_table_at;
//              class C is "none") and from there, once at the end, to the int64 outputs by 64-bit atomics, non-zero entries only.
//   outputs    every kernel tests the binning's flag first, so a point outside the stated box leaves every output untouched
//              (NUHTC_E_INVALID).  With n == 0 the maps are filled with -1 and the tables cleared by memsets, free_sites = W * H, and
//              nothing is launched.
//
// No counter can overflow for any accepted input (cellgrid_host.h has the argument).
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, profiles/cell_territory_resources.txt): no scratch in any kernel;
// terr_tile_kernel 18 VGPRs and the 4,096 B stage, terr_site_kernel 22 VGPRs and no LDS, terr_tally_kernel 22 VGPRs and the 900 B table,
// terr_zero_kernel 9 VGPRs; registers allow 8 waves per SIMD in all of them.
//
// Measured on one MI355X (tools/bench_territory.py -> profiles/cell_territory.json; 500 000 centres on a 36 000-px square, reach 64 px,
// C = 5, medians of 10 calls, the variants forced with -DNUHTC_SITE_ROUTE / -DNUHTC_TERRITORY_PER_SITE in two alternating rounds in
// one process, every variant bitwise equal to the shipped call).  Pitch 4 px, 81.6 M sites: 2.05 ms per call uniform (binning 0.07,
// owner 0.85, tally 0.92) and 1.85 ms clustered.  Pitch 32 px, 1.27 M sites: 0.47 and 0.53 ms.
//   owner route, ms staged / direct: pitch 4 px 2.05 / 2.26 uniform and 1.83 / 2.08 clustered; pitch 32 px 0.53 / 0.45 and 0.78 / 0.55 --
//              both kernels are kept, and the rule of the density maps picks the faster one at each measured shape.
//   tally, ms one atomic per run of a wave / one per site: pitch 4 px 2.05 / 5.55 uniform and 1.85 / 3.55 clustered; pitch 32 px
//              0.47 / 0.49 and 0.54 / 0.56 -- the wave-level reduction pays wherever territories span many sites and costs nothing
//              where they do not.
//
// Everything that decides an index or a limit -- the floor cell, the clamped cells of a footprint, the key and its order, the offer of a
// record, the table index, the flush bound, the window check and the route (cellgrid_host.h) -- is plain C++, and
// tools/dev/cellterritory_host_check.cpp calls exactly those functions on the host under -fsanitize=address,undefined.  The kernel code
// itself is not sanitized.
#include <algorithm>
#include <cstring>

#include "cellsites.h"

namespace {

constexpr int TERR_MAX_CELLS = 1 << 22;
constexpr int TERR_TALLY_BLOCKS = 2048;                 // workgroups of the tally kernel at most: one table flush each

struct CellTerritoryArgs {
  CellBin b;                          // the points, the grid and the records in cell order (cellbin.h, one key per cell)
  SiteLattice t;                      // reach = R
  int C;
  int32_t* owner;                     // [H][W]
  int32_t* nearest_d2;                // [H][W]
  int32_t* area;                      // [n]
  int32_t* border;                    // [n]
  int32_t* open;                      // [n] 0 / 1
  unsigned long long* contact;        // [C][C]
  unsigned long long* class_sites;    // [C]
  unsigned long long* free_sites;     // [1]
};

__global__ __launch_bounds__(256) void terr_zero_kernel(CellTerritoryArgs a) {
  if (*a.b.flag) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < a.b.n) { a.area[i] = 0; a.border[i] = 0; a.open[i] = 0; }
  if (i < a.C * a.C) a.contact[i] = 0;
  if (i < a.C) a.class_sites[i] = 0;
  if (i == 0) *a.free_sites = 0;
}

__device__ __forceinline__ void terr_take(const CellTerritoryArgs& a, const int4 o, const Site& me, int R2, unsigned long long& best) {
  const unsigned long long key = terr_offer(o.x - me.qx, o.y - me.qy, o.z, o.w, a.C, a.t.reach, R2);
  best = key < best ? key : best;
}

__device__ __forceinline__ void terr_write(const CellTerritoryArgs& a, const Site& me, unsigned long long best) {
  if (!me.active) return;
  const size_t at = (size_t)me.v * a.t.W + me.u;
  a.owner[at] = terr_key_row(best);
  a.nearest_d2[at] = terr_key_d2(best);
}

// both kernels: the flag, the best key, the sweep of cellsites.h (staged or direct), the write
template <bool STAGED>
__device__ __forceinline__ void terr_owner(const CellTerritoryArgs& a, int4* stage) {
  if (*a.b.flag) return;                                 // the binning met a point outside the box: nothing is written (uniform)
  const int R2 = a.t.reach * a.t.reach;
  const Site me = site_of(a.t);
  unsigned long long best = TERR_NO_KEY;
  site_sweep<STAGED>(a.b, a.t, me, stage, [&](const int4& o) { terr_take(a, o, me, R2, best); });
  terr_write(a, me, best);
}
__global__ __launch_bounds__(SITE_NT) void terr_tile_kernel(CellTerritoryArgs a) {
  __shared__ int4 stage[SITE_NT];
  terr_owner<true>(a, stage);
}
__global__ __launch_bounds__(SITE_NT) void terr_site_kernel(CellTerritoryArgs a) { terr_owner<false>(a, nullptr); }

// the tallies of the finished owner map.  RUNS: one atomic per run of equal owners among the lanes of a wave; else one per site.
template <bool RUNS>
__global__ __launch_bounds__(SITE_NT) void terr_tally_kernel(CellTerritoryArgs a) {
  __shared__ unsigned table[TERR_TABLE_WORDS];
  if (*a.b.flag) return;                                 // uniform
  const int tid = threadIdx.x, lane = tid & 63, C = a.C, W = a.t.W, H = a.t.H, total = W * H;      // total <= 2^28
  for (int i = tid; i < TERR_TABLE_WORDS; i += SITE_NT) table[i] = 0;
  __syncthreads();
  const int32_t* __restrict__ owner = a.owner;
  for (int base = blockIdx.x * SITE_NT; base < total; base += gridDim.x * SITE_NT) {          // uniform over the workgroup; < 2^28 + 2^19
    const int k = base + tid;
    int me = -2;                                         // a lane past the last site: a run of its own, counted nowhere
    bool on_border = false, is_open = false;
    if (k < total) {
      me = owner[k];
      const int v = k / W, u = k - v * W;
      const int ca = me >= 0 ? cs_class(a.b.labels[me], C) : C;                               // an owner competes: ca < C
      atomicAdd(&table[terr_table_at(ca, C, C)], 1u);                                          // the census of the sites
      auto see = [&](int kk) {
        const int o = owner[kk];
        if (o == me) return;
        on_border = true;
        if (o < 0) is_open = true;
        else if (me >= 0) atomicAdd(&table[terr_table_at(ca, cs_class(a.b.labels[o], C), C)], 1u);
      };
      if (u > 0) see(k - 1);
      if (u < W - 1) see(k + 1);
      if (v > 0) see(k - W);
      if (v < H - 1) see(k + W);
      is_open = is_open || u == 0 || v == 0 || u == W - 1 || v == H - 1;
    }
    if (RUNS) {
      const int before = __shfl_up(me, 1);
      const bool head = lane == 0 || before != me;
      const unsigned long long heads = __ballot(head), borders = __ballot(on_border), opens = __ballot(is_open);
      if (head && me >= 0) {
        const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
        const int len = above ? __ffsll((long long)above) : 64 - lane;                         // lanes up to the next head
        const unsigned long long span = (len == 64 ? ~0ull : (1ull << len) - 1) << lane;
        atomicAdd(&a.area[me], len);
        const int nb = __popcll(borders & span);
        if (nb) atomicAdd(&a.border[me], nb);
        if (opens & span) atomicOr(&a.open[me], 1);
      }
    } else if (me >= 0) {
      atomicAdd(&a.area[me], 1);
      if (on_border) atomicAdd(&a.border[me], 1);
      if (is_open) atomicOr(&a.open[me], 1);
    }
  }
  __syncthreads();
  for (int i = tid; i < (C + 1) * (C + 1); i += SITE_NT) {                                     // the flush: once (terr_table_fits)
    const unsigned t = table[i];
    if (!t) continue;
    const int ca = i / (C + 1), cb = i - ca * (C + 1);
    if (cb == C) atomicAdd(ca == C ? a.free_sites : &a.class_sites[ca], (unsigned long long)t);
    else if (ca < C) atomicAdd(&a.contact[ca * C + cb], (unsigned long long)t);
  }
}

}  // namespace

extern "C" int nuhtc_cell_territory(int device, const int32_t* points, const int32_t* labels, int64_t n, int num_classes, int reach, int s, int gx0,
                                    int gy0, int W, int H, int x_min, int y_min, int x_max, int y_max, int32_t* owner, int32_t* nearest_d2,
                                    int32_t* area, int32_t* border, int32_t* open, int64_t* contact, int64_t* class_sites, int64_t* free_sites,
                                    void* stream) {
  if (!cell_call_ok(n, MST_MAX_POINTS, num_classes, reach, x_min, y_min, x_max, y_max) || !site_window_ok(s, gx0, gy0, W, H, TERR_MAX_SITES)) return NUHTC_E_INVALID;
  if (!owner || !nearest_d2 || !contact || !class_sites || !free_sites || (n > 0 && (!points || !labels || !area || !border || !open))) return NUHTC_E_INVALID;
  if (hipSetDevice(device) != hipSuccess) return NUHTC_E_HIP;
  hipStream_t st = (hipStream_t)stream;
  const size_t sites = (size_t)W * H;
  const int C = num_classes;
  if (n == 0) {
    const int64_t all = (int64_t)sites;
    if (hipMemsetAsync(owner, 0xff, sites * sizeof(int32_t), st) != hipSuccess || hipMemsetAsync(nearest_d2, 0xff, sites * sizeof(int32_t), st) != hipSuccess ||
        hipMemsetAsync(contact, 0, (size_t)C * C * sizeof(int64_t), st) != hipSuccess || hipMemsetAsync(class_sites, 0, C * sizeof(int64_t), st) != hipSuccess ||
        hipMemcpyAsync(free_sites, &all, sizeof(int64_t), hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
      return NUHTC_E_HIP;
    return 0;
  }
  CellTerritoryArgs a;
  memset(&a, 0, sizeof(a));
  a.t = site_lattice(reach, s, gx0, gy0, W, H); a.C = C;
  a.owner = owner; a.nearest_d2 = nearest_d2; a.area = area; a.border = border; a.open = open;
  a.contact = reinterpret_cast<unsigned long long*>(contact); a.class_sites = reinterpret_cast<unsigned long long*>(class_sites);
  a.free_sites = reinterpret_cast<unsigned long long*>(free_sites);
  DevScratch tmp;      // every temporary of the call, freed on the way out
  const int nchunk = cellbin_setup(a.b, points, labels, (int)n, x_min, y_min, x_max, y_max, reach, TERR_MAX_CELLS, 1, tmp, st);
  if (!nchunk) return NUHTC_E_HIP;
  {
    ProfScope ps("cell_territory_bin", 0, 0, st);
    cellbin_launch(a.b, nchunk, st);
    hipLaunchKernelGGL(terr_zero_kernel, dim3((unsigned)((std::max<int64_t>(n, C * C) + 255) / 256)), dim3(256), 0, st, a);
  }
  {
    ProfScope ps("cell_territory_owner", 0, 0, st);
    site_launch(site_route(s, reach, a.b.side), terr_tile_kernel, terr_site_kernel, site_tiles(W, H), 0, st, a);
  }
  {
    ProfScope ps("cell_territory_tally", 0, 0, st);
    const unsigned blocks = (unsigned)std::min<size_t>((sites + SITE_NT - 1) / SITE_NT, TERR_TALLY_BLOCKS);
#ifdef NUHTC_TERRITORY_PER_SITE                           // dev probe: one atomic per site instead of one per run of a wave
    hipLaunchKernelGGL(terr_tally_kernel<false>, dim3(blocks), dim3(SITE_NT), 0, st, a);
#else
    hipLaunchKernelGGL(terr_tally_kernel<true>, dim3(blocks), dim3(SITE_NT), 0, st, a);
#endif
  }
  return cellbin_finish(a.b, st);
}
