// Proximity graphs of a slide's nuclei (gfx950): the Gabriel graph and the relative neighbourhood graph (RNG) over the cell grid.
//
// Definition (nuhtc_amd/proximity.py holds it in full, with the int64 brute-force restatement `proximity_reference`): n points in HALF
// pixels (|p| < 2^27, n <= 2^24), one label each, a radius r in half pixels (1 .. 16384), by_class in {0, 1}.  A CANDIDATE is an unordered
// pair i < j with d2(i, j) <= r * r (inclusive) and, with by_class, labels[i] == labels[j] (plain equality).  A WITNESS is any other row k
// (with by_class: of the same label).  The candidate is a GABRIEL edge when no witness has d2(i, k) + d2(j, k) < d2(i, j) -- none strictly
// inside the disc with diameter ij -- and an RNG edge when none has max(d2(i, k), d2(j, k)) < d2(i, j).  Both strict, both decided by
// three int32 squared distances (cellgrid_host.h: prox_gabriel_blocked, prox_rng_blocked, with the overflow argument), both unique
// without a tie rule; RNG is a subgraph of Gabriel.  The result: the Gabriel edges (i, j) in ascending (i, j) order, their d2, one byte
// each that says whether the edge is an RNG edge too, and the two degrees of every row.  A pure function of the input, bitwise the same
// on every call.
//
// Why the grid suffices: a blocking witness has d2(i, k) < d2(i, j) <= r * r in either test, so it lies in the 3 x 3 cells around i on a
// grid of side >= r -- the cells the candidate itself was found in.
//
// Stages, all on the caller's stream, every one a launch of its own; no kernel waits on another workgroup, and every loop runs over a
// range of the binning's tables (celledgelist.h holds the frame -- the tables, the clear, the read-back, the order of the launches -- and
// this file the two sweeps and the body of the place kernel):
//   binning    cellbin.h, reach r, ONE key per cell; by_class is a compare in the sweep's predicate.
//   count      degree cleared; then one thread per record i in cell order sweeps its 3 x 3 cells (cell_sweep) for the candidates j with a
//              LARGER row -- every candidate is tested once, from the record of its smaller row -- and for each one sweeps the same
//              cells again for the witnesses k (prox_flags) -- of those cells only the window that can hold a blocker, the midpoint's row
//              first: k is skipped unless d2(i, k) < d2(i, j), and the loop is left once the Gabriel flag is cleared (the RNG flag went
//              before it).  The Gabriel edges of the record go to count[i], the degrees to
//              `degree` by integer atomics at both ends, and the totals m and m_rng to two 64-bit counters, one atomic per wave after a
//              shuffle reduction: the edge count is NOT bounded by a multiple of n (a clique of coincident points), and no int32 sees it
//              before it is known to be at most edge_cap <= 2^31 - 1.  The two flags of the first 64 candidates of a record are kept
//              in two 64-bit words (profiles/cell_proximity.json has this against testing twice).
//   (the host reads m, m_rng and the binning's flag back.  m > edge_cap: the call ends here, the three edge arrays untouched.)
//   scan       exscan_launch over the n counts (at most 1024 chunks: why n <= 2^24): the segment of every row.
//   emit       the sweep of the count stage again: a candidate among the first 64 of its record reads its kept flags, a later one is
//              tested again (the test is a pure function of the records, so the two passes agree).  The record writes i into `edges`
//              and (j, d2 | rng bit) into two temporaries, at its own segment in sweep order -- private to the thread, no atomics.
//   place      one thread per edge: its place in the segment is the number of edges there with a smaller j (cell_rank_in_segment of
//              cellgrid_host.h), where j, d2 and the RNG byte go.
//
// A point outside the stated box raises the binning's flag; every kernel tests it, nothing is written to the outputs, and the call
// returns NUHTC_E_INVALID.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, profiles/cell_proximity_resources.txt), VGPRs / SGPRs: prox_count_kernel 42 / 92,
// prox_emit_kernel 40 / 88, prox_place_kernel 14 / 22, el_clear_kernel 4 / 14; no LDS and no scratch in any of them, 8 waves per SIMD
// everywhere.  Measured on 500 000 centres at 64 px (profiles/cell_proximity.json, two alternating rounds in one process): the window of
// the witness loop against all nine cells (-DNUHTC_PROX_DIRECT) 1.63 against 1.63 ms per call on the uniform set and 5.4 - 5.6 against
// 11.3 ms on the clustered one; the kept flags against testing twice (-DNUHTC_PROX_RETEST) 1.63 against 1.75 and 5.4 - 5.6 against 6.4 - 6.5.
#include <climits>
#include <cstring>

#include "celledgelist.h"

namespace {

constexpr int PROX_MAX_CELLS = 1 << 22;
constexpr int PROX_NT = 256;
constexpr int PROX_KEPT = 64;         // candidates per record whose flags the count stage keeps for the emit stage

struct CellProxArgs {
  CellBin b;                          // the points, the grid and the records in cell order (cellbin.h, one key per cell)
  EdgeList e;                         // the Gabriel edges (celledgelist.h); totals: one pair, m and m_rng
  int r, by_class;
  unsigned long long* kept;           // [n][2] by POSITION in cell order: the Gabriel and the RNG flags of the record's first 64 candidates
  int* s_d2;                          // [m] beside e.s_hi: the edge's d2 | PROX_RNG_BIT
  int32_t* edge_d2; uint8_t* edge_rng;
};

#ifdef NUHTC_PROX_DIRECT
// dev probe (-DNUHTC_PROX_DIRECT), the direct form that was measured first: the witness loop over ALL of the 3 x 3 cells around the
// record, three rows that are each one contiguous range of records (cell_rows of cellbin.h, held in registers)
using ProxRows = CellRows;
__device__ __forceinline__ ProxRows prox_rows(const CellBin& g, const int4& me) { return cell_rows(g, me); }

__device__ __forceinline__ int prox_flags(const CellBin& g, const ProxRows& w, const int4& me, const int4& o, int dij, int r, int r2, int by_class) {
  bool gab = true, rng = true;
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    for (int k = w.j0[t]; k < w.j0[t] + w.n[t] && gab; ++k) {
      const int4 c = g.recs[k];
      if (by_class && c.z != me.z) continue;
      const int dik = cell_pair_d2(c.x - me.x, c.y - me.y, r, r2);
      if (dik < 0 || dik >= dij) continue;
      const int djk = cell_pair_d2(c.x - o.x, c.y - o.y, r, r2);
      if (prox_rng_blocked(dik, djk, dij)) { rng = false; gab = !prox_gabriel_blocked(dik, djk, dij); }
    }
  }
  return (int)gab | ((int)(gab && rng) << 1);
}
#else
struct ProxRows {};
__device__ __forceinline__ ProxRows prox_rows(const CellBin&, const int4&) { return ProxRows{}; }

// bit 0: (me, o) at d2 = dij is a Gabriel edge; bit 1: it is an RNG edge as well.  The ends are not told from the witnesses: an end, or a
// point coincident with one, never blocks (cellgrid_host.h).  dij == 0 skips every witness: coincident points are joined, rng = 1.
// The witness loop runs over the WINDOW of cells that can hold a blocker, near witnesses first: a blocker is nearer than sqrt(dij) to
// BOTH ends, so it lies in the overlap of the two boxes of half-width d >= sqrt(dij) around them (cell_pair_window of cellbin.h); the
// row of the pair's midpoint goes first.
__device__ __forceinline__ int prox_flags(const CellBin& g, const ProxRows&, const int4& me, const int4& o, int dij, int r, int r2, int by_class) {
  const CellWindow v = cell_pair_window(g, me, o, (int)sqrtf((float)dij) + 1);      // dij <= 2^28: the float root is off by far less than 1
  bool gab = true, rng = true;
  for (int t = 0; t < 3 && gab; ++t) {
    const int gy = t == 0 ? v.gm : t == 1 ? v.gm - 1 : v.gm + 1;
    if (gy < v.gy0 || gy > v.gy1) continue;
    const int k1 = g.cell_start[gy * g.ncx + v.gx1 + 1];
    for (int k = g.cell_start[gy * g.ncx + v.gx0]; k < k1 && gab; ++k) {
      const int4 c = g.recs[k];
      if (by_class && c.z != me.z) continue;
      const int dik = cell_pair_d2(c.x - me.x, c.y - me.y, r, r2);
      if (dik < 0 || dik >= dij) continue;
      const int djk = cell_pair_d2(c.x - o.x, c.y - o.y, r, r2);
      if (prox_rng_blocked(dik, djk, dij)) { rng = false; gab = !prox_gabriel_blocked(dik, djk, dij); }
    }
  }
  return (int)gab | ((int)(gab && rng) << 1);
}
#endif

__global__ __launch_bounds__(PROX_NT) void prox_count_kernel(CellProxArgs a) {
  const CellBin& g = a.b;
  if (*g.flag) return;                                   // uniform
  const int q = blockIdx.x * PROX_NT + threadIdx.x;
  int cnt = 0, cnt_rng = 0;                              // every lane of a wave takes part in the reduction: no early return
  if (q < a.e.n) {
    const int4 me = g.recs[q];
    const ProxRows w = prox_rows(g, me);
    const int by_class = a.by_class, r = a.r, r2 = a.r * a.r;
    unsigned long long keep_g = 0, keep_r = 0;
    int seen = 0;
    cell_sweep(g, me, r, [&](const int4& o) { return o.w > me.w && (!by_class || o.z == me.z); }, [&](int, const int4& o, int d2) {
      const int f = prox_flags(g, w, me, o, d2, r, r2, by_class);
      if (seen < PROX_KEPT) { keep_g |= (unsigned long long)(f & 1) << seen; keep_r |= (unsigned long long)(f >> 1) << seen; }
      ++seen;
      if (!(f & 1)) return;
      ++cnt;
      atomicAdd(a.e.degree + 2 * o.w, 1);
      if (f & 2) { ++cnt_rng; atomicAdd(a.e.degree + 2 * o.w + 1, 1); }
    });
    a.e.count[me.w] = cnt;
#ifndef NUHTC_PROX_RETEST
    a.kept[2 * (size_t)q] = keep_g; a.kept[2 * (size_t)q + 1] = keep_r;
#endif
    if (cnt) atomicAdd(a.e.degree + 2 * me.w, cnt);
    if (cnt_rng) atomicAdd(a.e.degree + 2 * me.w + 1, cnt_rng);
  }
  const long long m = wave_sum((long long)cnt), m_rng = wave_sum((long long)cnt_rng);
  if ((threadIdx.x & 63) == 0) {
    if (m) atomicAdd(a.e.totals, (unsigned long long)m);
    if (m_rng) atomicAdd(a.e.totals + 1, (unsigned long long)m_rng);
  }
}

__global__ __launch_bounds__(PROX_NT) void prox_emit_kernel(CellProxArgs a) {
  const CellBin& g = a.b;
  const int q = blockIdx.x * PROX_NT + threadIdx.x;
  if (q >= a.e.n) return;
  const int4 me = g.recs[q];
  const int room = a.e.count[me.w];
  if (!room) return;
  const ProxRows w = prox_rows(g, me);
  const int by_class = a.by_class, r = a.r, r2 = a.r * a.r;
  const long long base = a.e.start[me.w];
#ifndef NUHTC_PROX_RETEST
  const unsigned long long keep_g = a.kept[2 * (size_t)q], keep_r = a.kept[2 * (size_t)q + 1];
#endif
  int seen = 0, at = 0;
  cell_sweep(g, me, r, [&](const int4& o) { return o.w > me.w && (!by_class || o.z == me.z); }, [&](int, const int4& o, int d2) {
#ifdef NUHTC_PROX_RETEST                                 // dev probe (-DNUHTC_PROX_RETEST): the pair test twice, no kept flags
    const int f = prox_flags(g, w, me, o, d2, r, r2, by_class);
#else
    const int f = seen < PROX_KEPT ? (int)(keep_g >> seen & 1) | (int)(keep_r >> seen & 1) << 1 : prox_flags(g, w, me, o, d2, r, r2, by_class);
#endif
    ++seen;
    if (!(f & 1) || at >= room) return;                  // at < room always (the two passes agree): no index leaves the segment
    const long long p = base + at++;
    a.e.edges[2 * p] = me.w;
    a.e.s_hi[p] = o.w;
    a.s_d2[p] = d2 | (f & 2 ? PROX_RNG_BIT : 0);
  });
}

__global__ __launch_bounds__(PROX_NT) void prox_place_kernel(CellProxArgs a) {
  const long long p = (long long)blockIdx.x * PROX_NT + threadIdx.x;
  if (p >= a.e.m) return;
  const int lo = a.e.edges[2 * p], hi = a.e.s_hi[p];
  if ((unsigned)lo >= (unsigned)a.e.n) return;           // cannot happen (the emit stage filled every segment): no index leaves the tables
  const long long j0 = a.e.start[lo];
  const long long at = cell_rank_in_segment(a.e.s_hi, j0, j0 + a.e.count[lo], hi);
  const int d2 = a.s_d2[p];
  a.e.edges[2 * at + 1] = hi;                            // the even entries of the segment already hold lo, all the same
  a.edge_d2[at] = d2 & (PROX_RNG_BIT - 1);
  a.edge_rng[at] = (uint8_t)((d2 & PROX_RNG_BIT) != 0);
}

}  // namespace

extern "C" int nuhtc_cell_proximity(int device, const int32_t* points, const int32_t* labels, int64_t n, int num_classes, int r, int by_class,
                                    int64_t edge_cap, int x_min, int y_min, int x_max, int y_max, int32_t* edges, int32_t* edge_d2,
                                    uint8_t* edge_rng, int32_t* degree, int64_t* m, int64_t* m_rng, void* stream) {
  if (!cell_call_ok(n, MST_MAX_POINTS, num_classes, r, x_min, y_min, x_max, y_max) || (by_class != 0 && by_class != 1) || !m || !m_rng ||
      edge_cap < 0 || edge_cap > INT_MAX)
    return NUHTC_E_INVALID;
  if (n > 0 && (!points || !labels || !edges || !edge_d2 || !edge_rng || !degree)) return NUHTC_E_INVALID;
  if (n == 0) { *m = 0; *m_rng = 0; return 0; }
  if (hipSetDevice(device) != hipSuccess) return NUHTC_E_HIP;
  hipStream_t s = (hipStream_t)stream;
  CellProxArgs a;
  memset(&a, 0, sizeof(a));
  a.e.n = (int)n; a.r = r; a.by_class = by_class;
  a.e.edges = edges; a.edge_d2 = edge_d2; a.edge_rng = edge_rng; a.e.degree = degree;
  DevScratch tmp;      // every temporary of the call, freed on the way out
  const int nchunk = cellbin_setup(a.b, points, labels, (int)n, x_min, y_min, x_max, y_max, r, PROX_MAX_CELLS, 1, tmp, s);
  if (!nchunk) return NUHTC_E_HIP;
  EdgeListRun h;
  if (!edgelist_setup(a.e, h, {"cell_prox_bin", "cell_prox_count", "cell_prox_scan", "cell_prox_emit", "cell_prox_place"}, 1, tmp, s)) return NUHTC_E_HIP;
#ifndef NUHTC_PROX_RETEST
  a.kept = tmp.alloc<unsigned long long>((size_t)n * 2 * sizeof(unsigned long long));
  if (!tmp.ok()) return NUHTC_E_HIP;
#endif
  const unsigned nb = (unsigned)((n + PROX_NT - 1) / PROX_NT);
  long long rng = 0;
  int rc = edgelist_count(a.b, nchunk, a.e, h, [&] { hipLaunchKernelGGL(prox_count_kernel, dim3(nb), dim3(PROX_NT), 0, s, a); }, &rng, s);
  if (rc) return rc;
  if (a.e.m > 0 && a.e.m <= edge_cap) {
    a.e.s_hi = tmp.alloc<int>((size_t)a.e.m * sizeof(int)); a.s_d2 = tmp.alloc<int>((size_t)a.e.m * sizeof(int));
    if (!tmp.ok()) return NUHTC_E_HIP;
    rc = edgelist_finish(h, [&] { hipLaunchKernelGGL(prox_emit_kernel, dim3(nb), dim3(PROX_NT), 0, s, a); },
                         [&] { hipLaunchKernelGGL(prox_place_kernel, dim3((unsigned)((a.e.m + PROX_NT - 1) / PROX_NT)), dim3(PROX_NT), 0, s, a); }, s);
    if (rc) return rc;
  }
  *m = a.e.m; *m_rng = rng;
  return 0;
}
