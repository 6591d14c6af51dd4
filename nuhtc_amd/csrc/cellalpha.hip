// The alpha complex of a slide's nuclei (gfx950): the exact Delaunay edges within a radius, over the cell grid.
//
// Definition (nuhtc_amd/alphacomplex.py holds it in full, with the int64 brute-force restatement `alpha_reference`): n points in HALF
// pixels (|p| < 2^27, n <= 2^24), one label each, a radius r in half pixels (1 .. 512, D = 2 r the diameter), by_class in {0, 1}.  A
// CANDIDATE is an unordered pair i < j with d2(i, j) <= D * D (inclusive) and, with by_class, labels[i] == labels[j] (plain equality).  A
// WITNESS is any other row k (with by_class: of the same label).  The candidate is an EDGE when some disc of radius <= r has both ends on
// its boundary and no witness strictly inside.  With q = p_j - p_i the discs through both ends are numbered by a real t (centre
// (q + t q_perp) / 2), radius <= r is t^2 <= T^2 = (D^2 - d2) / d2, and a witness at rho = p_k - p_i with s = q x rho, m = rho . (rho - q)
// lies strictly inside disc t exactly when t s > m: it bounds t from above (s > 0), from below (s < 0), blocks the pair (s == 0, m < 0) or
// does not bind.  hi is the smallest upper bound, lo the largest lower one; the pair is an edge when it is not blocked, hi >= -T, lo <= T
// and lo <= hi.  apex[0] is the smallest row that attains hi when hi <= T (the third corner of an empty circumcircle of radius <= r on that
// side), apex[1] the same for lo when lo >= -T, else -1.  The edge is GABRIEL when no witness has m < 0 (proximity.py's rule).  Coincident
// points are joined, both sides open, Gabriel.  Every decision is a comparison of two rationals in int64 (cellgrid_host.h: alpha_witness,
// alpha_dead, alpha_verdict, with the overflow argument); no tie rule is needed.  The result: the edges (i, j) in ascending (i, j) order,
// their d2, the two apexes, one byte that says whether the edge is Gabriel, and the two degrees of every row.  A pure function of the
// input, bitwise the same on every call.
//
// Why the grid suffices: a witness that binds within [-T, T] or kills the pair lies on or inside a disc of radius <= r through both ends,
// so within D of i AND of j: on a grid of side >= D it is in the 3 x 3 cells around i, and more narrowly in the overlap of the two boxes
// of half-width D around the ends.  Unlike the Gabriel test a binding witness may lie farther from i than j does, so cellprox.hip's
// "d2(i, k) < d2(i, j)" window does not apply.
//
// Stages, all on the caller's stream, every one a launch of its own; no kernel waits on another workgroup, and every loop runs over a
// range of the binning's tables (celledgelist.h holds the frame -- the tables, the clear, the read-back, the order of the launches -- and
// this file the wave kernel and the body of the place kernel):
//   binning    cellbin.h, reach D, ONE key per cell; by_class is a compare in the sweep's predicate.
//   count      degree cleared; then ONE WAVE per record i in cell order (alpha_wave_kernel): the records of its 3 x 3 cells are staged in
//              LDS, the candidates j with a LARGER row sit across the lanes, 64 at a time -- every candidate is tested once, from the
//              record of its smaller row -- and every lane walks the staged witnesses for its own candidate.  Per candidate it carries
//              two fractions and two rows (AlphaState); a lane leaves the loop as soon as its pair is dead, and that is asked only when a
//              bound has moved.  The edges of the record go to count[i], the degrees to `degree` by integer atomics at both ends, and the
//              totals m and m_gabriel to 64 pairs of 64-bit counters (one pair per record, spread by its position, summed on the host):
//              the edge count is NOT bounded by a multiple of n (a clique of coincident points), and no int32 sees it before it is known
//              to be at most edge_cap <= 2^31 - 1.
//   (the host reads m, m_gabriel and the binning's flag back.  m > edge_cap: the call ends here, the four edge arrays untouched.)
//   scan       exscan_launch over the n counts (at most 1024 chunks: why n <= 2^24): the segment of every row.
//   emit       the count stage again (the test is a pure function of the records, so the two passes agree), now with the apexes: the
//              edges among 64 candidates are ranked by a ballot, and the record writes i into `edges` and (j, d2 | Gabriel bit, the
//              apexes) into temporaries at its own segment -- private to the wave, no atomics.
//   place      one thread per edge: its place in the segment is the number of edges there with a smaller j (cell_rank_in_segment of
//              cellgrid_host.h), where j, d2, the apexes and the byte go.
//
// A point outside the stated box raises the binning's flag; every kernel tests it, nothing is written to the outputs, and the call
// returns NUHTC_E_INVALID.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, profiles/cell_alpha_resources.txt): alpha_wave_kernel<false / true>, the shipped
// count and emit stage, 30 / 32 VGPRs and 8 KB of LDS (5 waves per SIMD); alpha_place_kernel 14 VGPRs, no LDS; no scratch anywhere.  The
// shipped library holds only these and the frame's clear kernel.  Two dev probes, both timed against the shipped route in
// profiles/cell_alpha.json: -DNUHTC_ALPHA_THREAD is the route that was built first, one THREAD per record with the witnesses read from
// global memory through the overlap window of the pair (alpha_test, alpha_count_kernel, alpha_emit_kernel and the kept verdicts, compiled
// only then); -DNUHTC_ALPHA_DIRECT, on top of it, walks all of the 3 x 3 cells around the record instead of the window.
#include <climits>
#include <cstring>

#include "celledgelist.h"

namespace {

constexpr int ALPHA_MAX_CELLS = 1 << 22;
constexpr int ALPHA_NT = 256;
constexpr int ALPHA_SLOTS = 64;       // pairs of 64-bit counters the totals are spread over (the wave route adds one pair per record)

struct CellAlphaArgs {
  CellBin b;                          // the points, the grid and the records in cell order (cellbin.h, one key per cell)
  EdgeList e;                         // the edges (celledgelist.h); totals: ALPHA_SLOTS pairs, m and m_gabriel
  int D, by_class;
#ifdef NUHTC_ALPHA_THREAD
  unsigned long long* kept;           // [n] by POSITION in cell order: which of the record's first 64 candidates are edges
#endif
  int* s_d2;                          // [m] beside e.s_hi: the edge's d2 | ALPHA_GABRIEL_BIT
  int2* s_apex;                       // [m] its apexes
  int32_t* edge_d2; int32_t* apex; uint8_t* edge_gabriel;
};

#ifndef NUHTC_ALPHA_THREAD
// The shipped route of the witness loop: ONE WAVE per record (a workgroup of 64 threads, so that its
// barrier is the wave's own).  The records of the 3 x 3 cells around the record are staged in LDS -- once when at most ALPHA_STAGE of them
// (8 KB), else chunk by chunk for every 64 candidates -- the candidates sit across the lanes, 64 at a time, and every lane walks ALL the
// staged witnesses for its own candidate (the same LDS address across the wave: a broadcast read); alpha_witness passes the far ones
// over.  The count form adds the degrees and the totals, the emit form ranks the edges of 64 candidates by a ballot and writes them to
// the record's segment.  Both test every candidate: no kept flags.  profiles/cell_alpha.json has it against the thread-per-record route
// (-DNUHTC_ALPHA_THREAD below).
constexpr int ALPHA_STAGE = 512;

// the position among the records of the c-th record of the three rows, 0 <= c < w.total
__device__ __forceinline__ int alpha_pos(const CellRows& w, int c) {
  if (c < w.n[0]) return w.j0[0] + c;
  c -= w.n[0];
  return c < w.n[1] ? w.j0[1] + c : w.j0[2] + c - w.n[1];
}

template <bool EMIT>
__global__ __launch_bounds__(64) void alpha_wave_kernel(CellAlphaArgs a) {
  __shared__ int4 lds[ALPHA_STAGE];
  const CellBin& g = a.b;
  if (*g.flag) return;                                   // uniform
  const int q = blockIdx.x, lane = threadIdx.x;          // one workgroup per record: q < n by the launch
  const int4 me = g.recs[q];
  int room = 0;
  long long base = 0;
  if (EMIT) {
    room = a.e.count[me.w];
    if (!room) return;                                   // uniform: before any barrier
    base = a.e.start[me.w];
  }
  const CellRows w = cell_rows(g, me);
  const int by_class = a.by_class, D = a.D, D2 = a.D * a.D;
  const bool all = w.total <= ALPHA_STAGE;
  if (all) {
    for (int c = lane; c < w.total; c += 64) lds[c] = g.recs[alpha_pos(w, c)];
    __syncthreads();
  }
  int cnt = 0, cnt_gab = 0, at = 0;
  for (int c0 = 0; c0 < w.total; c0 += 64) {             // every bound of the loops with a barrier inside is uniform
    const int c = c0 + lane;
    int4 o = make_int4(0, 0, 0, -1);
    int d2 = -1;
    if (c < w.total) {
      o = all ? lds[c] : g.recs[alpha_pos(w, c)];
      if (o.w > me.w && (!by_class || o.z == me.z)) d2 = cell_pair_d2(o.x - me.x, o.y - me.y, D, D2);
    }
    if (!__any(d2 >= 0)) continue;                       // uniform
    const bool live = d2 > 0;
    const int qx = o.x - me.x, qy = o.y - me.y;
    AlphaState st = alpha_open();
    bool dead = false;
    for (int k0 = 0; k0 < w.total; k0 += ALPHA_STAGE) {
      const int kn = min(ALPHA_STAGE, w.total - k0);
      if (!all) {
        __syncthreads();
        for (int k = lane; k < kn; k += 64) lds[k] = g.recs[alpha_pos(w, k0 + k)];
        __syncthreads();
      }
      if (live)
        for (int k = 0; k < kn && !dead; ++k) {
          const int4 cc = lds[k];
          if (by_class && cc.z != me.z) continue;
          if (alpha_witness(st, qx, qy, cc.x - me.x, cc.y - me.y, cc.w, D, D2)) dead = alpha_dead(st, d2, D2);
        }
    }
    int apex[2] = {-1, -1};
    const int f = d2 < 0 ? 0 : d2 == 0 ? 3 : dead ? 0 : alpha_verdict(st, d2, D2, apex);
    if (!EMIT) {
      if (f & 1) {
        ++cnt;
        atomicAdd(a.e.degree + 2 * o.w, 1);
        if (f & 2) { ++cnt_gab; atomicAdd(a.e.degree + 2 * o.w + 1, 1); }
      }
    } else {
      const unsigned long long edge = __ballot(f & 1);
      const int rank = at + __popcll(edge & ((1ull << lane) - 1));
      if ((f & 1) && rank < room) {                      // rank < room always (the two passes agree): no index leaves the segment
        const long long p = base + rank;
        a.e.edges[2 * p] = me.w;
        a.e.s_hi[p] = o.w;
        a.s_d2[p] = d2 | (f & 2 ? ALPHA_GABRIEL_BIT : 0);
        a.s_apex[p] = make_int2(apex[0], apex[1]);
      }
      at += __popcll(edge);
    }
  }
  if (!EMIT) {
    const unsigned long long m = (unsigned long long)wave_sum((long long)cnt), m_gab = (unsigned long long)wave_sum((long long)cnt_gab);
    if (lane == 0) {
      a.e.count[me.w] = (int)m;                          // at most the records of nine cells
      if (m) { atomicAdd(a.e.degree + 2 * me.w, (int)m); atomicAdd(a.e.totals + 2 * (q & (ALPHA_SLOTS - 1)), m); }
      if (m_gab) { atomicAdd(a.e.degree + 2 * me.w + 1, (int)m_gab); atomicAdd(a.e.totals + 2 * (q & (ALPHA_SLOTS - 1)) + 1, m_gab); }
    }
  }
}

#else
// dev probe (-DNUHTC_ALPHA_THREAD), the route that was built first: one THREAD per record, cell_sweep for the candidates and alpha_test
// for each of them; the count stage keeps the verdict of a record's first ALPHA_KEPT candidates for the emit stage.
constexpr int ALPHA_KEPT = 64;

// bit 0: (me, o) at d2 is an edge; bit 1: it is Gabriel as well; apex[0..1] written for an edge.  The ends are not told from the
// witnesses (cellgrid_host.h).  d2 == 0 consults no witness.  The witness loop runs over the WINDOW of cells that can hold a binding
// witness: the overlap of the two boxes of half-width D around the ends (cell_pair_window of cellbin.h); the row of the pair's midpoint
// goes first, where the witnesses that kill a pair are likeliest.
__device__ __forceinline__ int alpha_test(const CellBin& g, const int4& me, const int4& o, int d2, int D, int D2, int by_class, int* apex) {
  if (d2 == 0) { apex[0] = apex[1] = -1; return 3; }
  CellWindow v = cell_pair_window(g, me, o, D);
#ifdef NUHTC_ALPHA_DIRECT                               // all of the 3 x 3 cells around me, the midpoint's row still first
  const int cx = (me.x - g.x_min) / g.side, cy = (me.y - g.y_min) / g.side;
  v.gx0 = max(cx - 1, 0); v.gx1 = min(cx + 1, g.ncx - 1); v.gy0 = max(cy - 1, 0); v.gy1 = min(cy + 1, g.ncy - 1);
  v.gm = min(max(((me.y + o.y) / 2 - g.y_min) / g.side, v.gy0), v.gy1);
#endif
  const int qx = o.x - me.x, qy = o.y - me.y;
  AlphaState st = alpha_open();
  bool dead = false;
  for (int t = 0; t < 3 && !dead; ++t) {
    const int gy = t == 0 ? v.gm : t == 1 ? v.gm - 1 : v.gm + 1;
    if (gy < v.gy0 || gy > v.gy1) continue;
    const int k1 = g.cell_start[gy * g.ncx + v.gx1 + 1];
    for (int k = g.cell_start[gy * g.ncx + v.gx0]; k < k1 && !dead; ++k) {
      const int4 c = g.recs[k];
      if (by_class && c.z != me.z) continue;
      if (alpha_witness(st, qx, qy, c.x - me.x, c.y - me.y, c.w, D, D2)) dead = alpha_dead(st, d2, D2);
    }
  }
  return dead ? 0 : alpha_verdict(st, d2, D2, apex);
}

__global__ __launch_bounds__(ALPHA_NT) void alpha_count_kernel(CellAlphaArgs a) {
  const CellBin& g = a.b;
  if (*g.flag) return;                                   // uniform
  const int q = blockIdx.x * ALPHA_NT + threadIdx.x;
  int cnt = 0, cnt_gab = 0;                              // every lane of a wave takes part in the reduction: no early return
  if (q < a.e.n) {
    const int4 me = g.recs[q];
    const int by_class = a.by_class, D = a.D, D2 = a.D * a.D;
    unsigned long long keep = 0;
    int seen = 0;
    cell_sweep(g, me, D, [&](const int4& o) { return o.w > me.w && (!by_class || o.z == me.z); }, [&](int, const int4& o, int d2) {
      int apex[2];
      const int f = alpha_test(g, me, o, d2, D, D2, by_class, apex);
      if (seen < ALPHA_KEPT) keep |= (unsigned long long)(f & 1) << seen;
      ++seen;
      if (!(f & 1)) return;
      ++cnt;
      atomicAdd(a.e.degree + 2 * o.w, 1);
      if (f & 2) { ++cnt_gab; atomicAdd(a.e.degree + 2 * o.w + 1, 1); }
    });
    a.e.count[me.w] = cnt;
    a.kept[q] = keep;
    if (cnt) atomicAdd(a.e.degree + 2 * me.w, cnt);
    if (cnt_gab) atomicAdd(a.e.degree + 2 * me.w + 1, cnt_gab);
  }
  const long long m = wave_sum((long long)cnt), m_gab = wave_sum((long long)cnt_gab);
  if ((threadIdx.x & 63) == 0) {
    if (m) atomicAdd(a.e.totals, (unsigned long long)m);
    if (m_gab) atomicAdd(a.e.totals + 1, (unsigned long long)m_gab);
  }
}

__global__ __launch_bounds__(ALPHA_NT) void alpha_emit_kernel(CellAlphaArgs a) {
  const CellBin& g = a.b;
  const int q = blockIdx.x * ALPHA_NT + threadIdx.x;
  if (q >= a.e.n) return;
  const int4 me = g.recs[q];
  const int room = a.e.count[me.w];
  if (!room) return;
  const int by_class = a.by_class, D = a.D, D2 = a.D * a.D;
  const long long base = a.e.start[me.w];
  const unsigned long long keep = a.kept[q];
  int seen = 0, at = 0;
  cell_sweep(g, me, D, [&](const int4& o) { return o.w > me.w && (!by_class || o.z == me.z); }, [&](int, const int4& o, int d2) {
    const bool skip = seen < ALPHA_KEPT && !(keep >> seen & 1);
    ++seen;
    if (skip || at >= room) return;                      // at < room always (the two passes agree): no index leaves the segment
    int apex[2];
    const int f = alpha_test(g, me, o, d2, D, D2, by_class, apex);
    if (!(f & 1)) return;
    const long long p = base + at++;
    a.e.edges[2 * p] = me.w;
    a.e.s_hi[p] = o.w;
    a.s_d2[p] = d2 | (f & 2 ? ALPHA_GABRIEL_BIT : 0);
    a.s_apex[p] = make_int2(apex[0], apex[1]);
  });
}
#endif

__global__ __launch_bounds__(ALPHA_NT) void alpha_place_kernel(CellAlphaArgs a) {
  const long long p = (long long)blockIdx.x * ALPHA_NT + threadIdx.x;
  if (p >= a.e.m) return;
  const int lo = a.e.edges[2 * p], hi = a.e.s_hi[p];
  if ((unsigned)lo >= (unsigned)a.e.n) return;           // cannot happen (the emit stage filled every segment): no index leaves the tables
  const long long j0 = a.e.start[lo];
  const long long at = cell_rank_in_segment(a.e.s_hi, j0, j0 + a.e.count[lo], hi);
  const int d2 = a.s_d2[p];
  const int2 ap = a.s_apex[p];
  a.e.edges[2 * at + 1] = hi;                            // the even entries of the segment already hold lo, all the same
  a.edge_d2[at] = d2 & (ALPHA_GABRIEL_BIT - 1);
  a.apex[2 * at] = ap.x; a.apex[2 * at + 1] = ap.y;
  a.edge_gabriel[at] = (uint8_t)((d2 & ALPHA_GABRIEL_BIT) != 0);
}

}  // namespace

extern "C" int nuhtc_cell_alpha(int device, const int32_t* points, const int32_t* labels, int64_t n, int num_classes, int r, int by_class,
                                int64_t edge_cap, int x_min, int y_min, int x_max, int y_max, int32_t* edges, int32_t* edge_d2, int32_t* apex,
                                uint8_t* edge_gabriel, int32_t* degree, int64_t* m, int64_t* m_gabriel, void* stream) {
  if (!m || !m_gabriel || !alpha_call_ok(n, num_classes, r, by_class, edge_cap, x_min, y_min, x_max, y_max)) return NUHTC_E_INVALID;
  if (n > 0 && (!points || !labels || !edges || !edge_d2 || !apex || !edge_gabriel || !degree)) return NUHTC_E_INVALID;
  if (n == 0) { *m = 0; *m_gabriel = 0; return 0; }
  if (hipSetDevice(device) != hipSuccess) return NUHTC_E_HIP;
  hipStream_t s = (hipStream_t)stream;
  CellAlphaArgs a;
  memset(&a, 0, sizeof(a));
  a.e.n = (int)n; a.D = 2 * r; a.by_class = by_class;
  a.e.edges = edges; a.edge_d2 = edge_d2; a.apex = apex; a.edge_gabriel = edge_gabriel; a.e.degree = degree;
  DevScratch tmp;      // every temporary of the call, freed on the way out
  const int nchunk = cellbin_setup(a.b, points, labels, (int)n, x_min, y_min, x_max, y_max, a.D, ALPHA_MAX_CELLS, 1, tmp, s);
  if (!nchunk) return NUHTC_E_HIP;
  EdgeListRun h;
  if (!edgelist_setup(a.e, h, {"cell_alpha_bin", "cell_alpha_count", "cell_alpha_scan", "cell_alpha_emit", "cell_alpha_place"}, ALPHA_SLOTS, tmp, s))
    return NUHTC_E_HIP;
#ifndef NUHTC_ALPHA_THREAD
  auto count = [&] { hipLaunchKernelGGL(alpha_wave_kernel<false>, dim3((unsigned)n), dim3(64), 0, s, a); };
  auto emit = [&] { hipLaunchKernelGGL(alpha_wave_kernel<true>, dim3((unsigned)n), dim3(64), 0, s, a); };
#else
  a.kept = tmp.alloc<unsigned long long>((size_t)n * sizeof(unsigned long long));
  if (!tmp.ok()) return NUHTC_E_HIP;
  const unsigned nb = (unsigned)((n + ALPHA_NT - 1) / ALPHA_NT);
  auto count = [&] { hipLaunchKernelGGL(alpha_count_kernel, dim3(nb), dim3(ALPHA_NT), 0, s, a); };
  auto emit = [&] { hipLaunchKernelGGL(alpha_emit_kernel, dim3(nb), dim3(ALPHA_NT), 0, s, a); };
#endif
  long long gabriel = 0;
  int rc = edgelist_count(a.b, nchunk, a.e, h, count, &gabriel, s);
  if (rc) return rc;
  if (a.e.m > 0 && a.e.m <= edge_cap) {
    a.e.s_hi = tmp.alloc<int>((size_t)a.e.m * sizeof(int)); a.s_d2 = tmp.alloc<int>((size_t)a.e.m * sizeof(int));
    a.s_apex = tmp.alloc<int2>((size_t)a.e.m * sizeof(int2));
    if (!tmp.ok()) return NUHTC_E_HIP;
    rc = edgelist_finish(h, emit, [&] { hipLaunchKernelGGL(alpha_place_kernel, dim3((unsigned)((a.e.m + ALPHA_NT - 1) / ALPHA_NT)), dim3(ALPHA_NT), 0, s, a); }, s);
    if (rc) return rc;
  }
  *m = a.e.m; *m_gabriel = gabriel;
  return 0;
}
