// Minimum spanning forest of a slide's nuclei (gfx950): Boruvka rounds over the cell grid, with the lock-free union of cellunion.h.
//
// Definition (nuhtc_amd/mst.py holds it in full, with the int64 brute-force restatement `mst_reference`): n points in HALF pixels
// (|p| < 2^27, n <= 2^24), one label each, a radius r in half pixels (1 .. 16384), by_class in {0, 1}.  An EDGE is an unordered pair
// i < j with dx * dx + dy * dy <= r * r (inclusive; coincident points are joined with d2 = 0) and, with by_class, labels[i] == labels[j]
// (plain equality).  Edges are ordered by the key (d2, i, j), a strict total order, so the minimum spanning forest of the edge set is
// UNIQUE -- what Kruskal's algorithm returns on the edges in ascending key order -- and that forest is the result: its edges (i, j) in
// ascending (i, j) order, their d2, and the tree of every point, numbered 0 .. T - 1 by ascending smallest row.  Integer arithmetic only:
// the result is a pure function of the input and bitwise the same on every call.
//
// Why Boruvka gives Kruskal's forest: under a strict total order the smallest edge leaving ANY set of points belongs to the unique
// minimum forest (cut property), so every edge a round picks is an edge of the result, whatever the components look like.
//
// Stages, all on the caller's stream, every one a launch of its own; no kernel waits on another workgroup:
//   binning    cellbin.h, reach r, ONE key per cell; by_class is a compare in the sweep's predicate, as in cellcluster.hip.
//   init       comp[row] = parent[row] = row, the component of every record next to it in CELL order (pcomp), the picks cleared.
//   round      at most 25 of them, run from the host; after each, ONE int is read back (the edges so far) and the loop ends when a
//              round added none.  Every round at least halves the components that still have an edge out, and n <= 2^24: round 25 can
//              add nothing, and if it does the call returns NUHTC_E_HIP.
//     pick     one thread per record in cell order sweeps its 3 x 3 cells (cell_sweep) and keeps in registers the smallest
//              (d2, lo, hi) over the records o within reach with pcomp[o] != pcomp[me].  (d2, lo, hi) is 29 + 24 + 24 bits, more than
//              one 64-bit atomic holds (cellgrid_host.h: mst_key): the thread stores its own best by position (lkey = (d2, lo), lhi)
//              and does atomicMin(best1 + comp, lkey).  Then a streaming kernel with no sweep: every record whose lkey equals
//              best1[comp] does atomicMin(best2 + comp, lhi).  Exact: the component's smallest edge is also the smallest edge of its
//              inside end, so that end holds (d2, lo) AND the right hi; any other record with the same (d2, lo) holds an edge that is
//              no smaller, hence an hi that is no smaller.  Before the first atomic a wave whose picking lanes all sit in ONE
//              component reduces with shuffles and sends one atomic; a mixed wave first reads best1[comp] and sends only a smaller
//              key (in round one every lane is its own component, later most waves are uniform).  A record with no neighbour of
//              another component within reach never gets one again -- components only grow -- and is marked `done`: its sweep is
//              skipped in every later round.
//     emit     one thread per component root c with a pick e.  c' = the component at e's other end; when c' picked e as well and
//              c' < c the thread leaves the emission to c' (under a strict total order the picks form no cycle but such 2-cycles).
//              Otherwise (lo, hi, d2) goes to an unordered list through an atomic counter.  Either way unite(lo, hi).
//     relabel  comp[row] = pcomp[position] = the root above row (a read-only walk), parent[row] set to it (an ancestor: the invariant
//              of cellunion.h holds), best1 / best2 cleared.
//   order      the canonical edge order without a sort: count the edges per lo (atomics), scan the n counts (exscan_launch, at most
//              1024 chunks: why n <= 2^24), drop every edge into the segment of its lo in arrival order (the counts go back to zero),
//              then one thread per edge writes it at start[lo] + the edges of the segment with a smaller hi (cell_rank_in_segment of
//              cellgrid_host.h) -- hi is distinct within a segment.  The output is a pure function of the input; a star of coincident points stays parallel.
//   number     root flags where comp[row] == row, one scan, tree[i] = rank[comp[i]], T = rank[n - 1] + flag[n - 1].
//
// A point outside the stated box raises the binning's flag; every later kernel tests it, no edge is ever emitted, nothing is written to
// the outputs, and the call returns NUHTC_E_INVALID.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, profiles/cell_mst_resources.txt), VGPRs / SGPRs: the sweep mst_pick_kernel
// 30 / 50, mst_init_kernel 18 / 22, mst_place_kernel 14 / 18, mst_relabel_kernel 14 / 18, mst_emit_kernel 10 / 27, the others less; no
// scratch and no LDS in any of them.  Registers never limit the occupancy (8 waves per SIMD everywhere): the 32-wave cap of a CU does.
#include <algorithm>
#include <climits>
#include <cstring>

#include "cellbin.h"
#include "cellunion.h"

namespace {

constexpr int MST_MAX_CELLS = 1 << 22;
constexpr int MST_NT = 256;
constexpr int MST_MAX_ROUNDS = 25;

struct CellMstArgs {
  CellBin b;                      // the points, the grid and the records in cell order (cellbin.h, one key per cell)
  int n, r, by_class, m;          // m: the edges of the forest, known on the host once the rounds are over
  int* pcomp;                     // [n] by POSITION in cell order: the component of that record
  int* comp;                      // [n] by row: the component (its smallest row)
  int* parent;                    // [n] by row: the union-find forest (parent <= row)
  uint8_t* done;                  // [n] by position: every neighbour within reach shares the record's component
  unsigned long long* lkey;       // [n] by position: the (d2, lo) of the record's own smallest edge out, MST_NO_KEY for none
  int* lhi;                       // [n] by position: the hi of that edge
  unsigned long long* best1;      // [n] by component: the smallest (d2, lo) of an edge out
  int* best2;                     // [n] by component: the smallest hi among the edges with that (d2, lo)
  int* e_lo; int* e_hi; int* e_d2;      // [n] the edges in arrival order
  int* count;                     // the edges so far
  int* s_lo; int* s_hi; int* s_d2;      // [n] the edges segment by segment of lo, arrival order inside
  int* sin;                       // [fchunk * CB_CHUNK] scan input: edges per lo, later the root flags; zero past n
  int* sout;                      // [fchunk * CB_CHUNK] scan output
  int* t_dev;
  int32_t* edges; int32_t* edge_d2; int32_t* tree;
};

__device__ __forceinline__ unsigned long long mst_wave_min(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, (unsigned long long)__shfl_xor(v, o));
  return v;
}

__global__ __launch_bounds__(MST_NT) void mst_init_kernel(CellMstArgs a) {
  const CellBin& g = a.b;
  if (*g.flag) return;                                   // the binning met a point outside the box: nothing is written
  const int q = blockIdx.x * MST_NT + threadIdx.x;
  if (q >= a.n) return;
  const int row = g.recs[q].w;
  a.pcomp[q] = row; a.comp[row] = row; a.parent[row] = row; a.done[q] = 0;
  a.lkey[q] = MST_NO_KEY;
  a.best1[row] = MST_NO_KEY; a.best2[row] = INT_MAX;
}

__global__ __launch_bounds__(MST_NT) void mst_pick_kernel(CellMstArgs a) {
  const CellBin& g = a.b;
  if (*g.flag) return;                                   // uniform
  const int q = blockIdx.x * MST_NT + threadIdx.x;
  const int lane = threadIdx.x & 63;
  unsigned long long key = MST_NO_KEY;                   // every lane of a wave takes part in the reduction: no early return
  int mc = -1;
  if (q < a.n && !a.done[q]) {
    const int4 me = g.recs[q];
    mc = a.pcomp[q];
    int hi = INT_MAX;
    const int by_class = a.by_class;
    cell_sweep(g, me, a.r, [&](const int4& o) { return !by_class || o.z == me.z; }, [&](int j, const int4& o, int d2) {
      if (a.pcomp[j] == mc) return;                      // the record itself among them
      const unsigned long long k = mst_key(d2, min(me.w, o.w));
      const int h = max(me.w, o.w);
      if (mst_edge_less(k, h, key, hi)) { key = k; hi = h; }
    });
    a.lkey[q] = key;
    a.lhi[q] = hi;
#ifndef NUHTC_MST_NO_DONE                                // dev probe (-DNUHTC_MST_NO_DONE): what the mark saves
    if (key == MST_NO_KEY) a.done[q] = 1;
#endif
  }
  const unsigned long long has = __ballot(key != MST_NO_KEY);
  if (!has) return;                                      // uniform
  const int first = __ffsll(has) - 1;
  const int c0 = __shfl(mc, first);
  if (!__ballot(key != MST_NO_KEY && mc != c0)) {        // the picking lanes share one component: one atomic for the wave
    const unsigned long long least = mst_wave_min(key);
    if (lane == first && __hip_atomic_load(a.best1 + c0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > least) atomicMin(a.best1 + c0, least);
  } else if (key != MST_NO_KEY && __hip_atomic_load(a.best1 + mc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > key) {
    atomicMin(a.best1 + mc, key);                        // a stale read is a LARGER value: at worst one atomic too many
  }
}

__global__ __launch_bounds__(MST_NT) void mst_pick_hi_kernel(CellMstArgs a) {
  if (*a.b.flag) return;
  const int q = blockIdx.x * MST_NT + threadIdx.x;
  if (q >= a.n) return;
  const unsigned long long key = a.lkey[q];
  if (key == MST_NO_KEY) return;
  const int mc = a.pcomp[q];
  if (a.best1[mc] == key) atomicMin(a.best2 + mc, a.lhi[q]);
}

__global__ __launch_bounds__(MST_NT) void mst_emit_kernel(CellMstArgs a) {
  if (*a.b.flag) return;
  const int c = blockIdx.x * MST_NT + threadIdx.x;
  if (c >= a.n || a.comp[c] != c) return;
  const unsigned long long key = a.best1[c];
  if (key == MST_NO_KEY) return;
  const int lo = mst_key_lo(key), hi = a.best2[c], d2 = mst_key_d2(key);
  if ((unsigned)hi >= (unsigned)a.n || lo >= hi) return; // cannot happen (pick_hi gave every picked (d2, lo) its hi): no index leaves the tables
  const int c2 = a.comp[a.comp[lo] == c ? hi : lo];      // the component at the other end
  const bool theirs = c2 < c && a.best1[c2] == key && a.best2[c2] == hi;      // the mutual pick is emitted by the smaller component
  if (!theirs) {
    const int at = atomicAdd(a.count, 1);
    if (at < a.n) { a.e_lo[at] = lo; a.e_hi[at] = hi; a.e_d2[at] = d2; }       // a forest has at most n - 1 edges
  }
  cc_unite(a.parent, lo, hi);
}

__global__ __launch_bounds__(MST_NT) void mst_relabel_kernel(CellMstArgs a) {
  const CellBin& g = a.b;
  if (*g.flag) return;
  const int q = blockIdx.x * MST_NT + threadIdx.x;
  if (q >= a.n) return;
  const int row = g.recs[q].w;
  // No union runs in this launch: the root is final for the round.  The walk only READS the entries of others (relaxed loads) and then
  // writes its OWN entry, an ancestor in either state: the path halving of cc_find here sent one atomic per step to the entries next to the
  // root of a tree of 458 000 rows, and the stage took 2.6 ms of the uniform benchmark set's 3.5 ms of kernels.
  int root = row;
  for (int p = cc_load(a.parent + root); p != root; p = cc_load(a.parent + root)) root = p;
  if (root != row) __hip_atomic_store(a.parent + row, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);    // the next round finds it in one step
  a.comp[row] = root; a.pcomp[q] = root;
  a.best1[row] = MST_NO_KEY; a.best2[row] = INT_MAX;
}

__global__ __launch_bounds__(MST_NT) void mst_count_kernel(CellMstArgs a) {
  const int e = blockIdx.x * MST_NT + threadIdx.x;
  if (e < a.m) atomicAdd(a.sin + a.e_lo[e], 1);
}

__global__ __launch_bounds__(MST_NT) void mst_segment_kernel(CellMstArgs a) {
  const int e = blockIdx.x * MST_NT + threadIdx.x;
  if (e >= a.m) return;
  const int lo = a.e_lo[e];
  const int at = a.sout[lo] + atomicSub(a.sin + lo, 1) - 1;      // the segment fills from its end; the counts return to zero
  a.s_lo[at] = lo; a.s_hi[at] = a.e_hi[e]; a.s_d2[at] = a.e_d2[e];
}

__global__ __launch_bounds__(MST_NT) void mst_place_kernel(CellMstArgs a) {
  const int p = blockIdx.x * MST_NT + threadIdx.x;
  if (p >= a.m) return;
  const int lo = a.s_lo[p], hi = a.s_hi[p];
  const int j0 = a.sout[lo], j1 = a.sout[lo + 1];        // lo < hi <= n - 1: entry lo + 1 is inside the n counts
  const int at = (int)cell_rank_in_segment(a.s_hi, j0, j1, hi);
  a.edges[2 * (size_t)at] = lo; a.edges[2 * (size_t)at + 1] = hi;
  a.edge_d2[at] = a.s_d2[p];
}

__global__ __launch_bounds__(MST_NT) void mst_rootflag_kernel(CellMstArgs a) {
  if (*a.b.flag) return;
  const int i = blockIdx.x * MST_NT + threadIdx.x;
  if (i < a.n) a.sin[i] = a.comp[i] == i;
}

__global__ __launch_bounds__(MST_NT) void mst_number_kernel(CellMstArgs a) {
  if (*a.b.flag) return;
  const int i = blockIdx.x * MST_NT + threadIdx.x;
  if (i >= a.n) return;
  a.tree[i] = a.sout[a.comp[i]];
  if (i == a.n - 1) *a.t_dev = a.sout[i] + a.sin[i];
}

}  // namespace

extern "C" int nuhtc_cell_mst(int device, const int32_t* points, const int32_t* labels, int64_t n, int num_classes, int r, int by_class,
                              int x_min, int y_min, int x_max, int y_max, int32_t* edges, int32_t* edge_d2, int32_t* tree,
                              int64_t* m, int64_t* trees, int64_t* rounds, void* stream) {
  if (!cell_call_ok(n, MST_MAX_POINTS, num_classes, r, x_min, y_min, x_max, y_max) || (by_class != 0 && by_class != 1) || !m || !trees || !rounds)
    return NUHTC_E_INVALID;
  if (n > 0 && (!points || !labels || !edges || !edge_d2 || !tree)) return NUHTC_E_INVALID;
  if (n == 0) { *m = 0; *trees = 0; *rounds = 0; return 0; }
  if (hipSetDevice(device) != hipSuccess) return NUHTC_E_HIP;
  hipStream_t s = (hipStream_t)stream;
  CellMstArgs a;
  memset(&a, 0, sizeof(a));
  a.n = (int)n; a.r = r; a.by_class = by_class;
  a.edges = edges; a.edge_d2 = edge_d2; a.tree = tree;
  DevScratch tmp;      // every temporary of the call, freed on the way out
  const int nchunk = cellbin_setup(a.b, points, labels, (int)n, x_min, y_min, x_max, y_max, r, MST_MAX_CELLS, 1, tmp, s);
  if (!nchunk) return NUHTC_E_HIP;
  const int fchunk = (int)((n + CB_CHUNK - 1) / CB_CHUNK);                 // scan chunks of the n counts / root flags: at most 1024
  const size_t scan_bytes = (size_t)fchunk * CB_CHUNK * sizeof(int), row_bytes = (size_t)n * sizeof(int);
  // ONE allocation for the tables of this file, carved in 256-byte steps (each hipMalloc and hipFree of twenty cost more than a round)
  const size_t step = 256, rows_up = (row_bytes + step - 1) / step * step, done_up = ((size_t)n + step - 1) / step * step;
  const size_t total = 15 * rows_up + done_up + 2 * scan_bytes + 1024 * sizeof(int) + 2 * step;     // 11 int tables + 2 of 8 bytes = 15 rows
  char* base = tmp.alloc<char>(total);
  if (!tmp.ok()) return NUHTC_E_HIP;
  size_t at = 0;
  auto carve = [&](size_t bytes) { char* p = base + at; at += (bytes + step - 1) / step * step; return p; };
  auto ints = [&](size_t bytes) { return reinterpret_cast<int*>(carve(bytes)); };
  a.lkey = reinterpret_cast<unsigned long long*>(carve(2 * row_bytes)); a.best1 = reinterpret_cast<unsigned long long*>(carve(2 * row_bytes));
  a.pcomp = ints(row_bytes); a.comp = ints(row_bytes); a.parent = ints(row_bytes); a.lhi = ints(row_bytes); a.best2 = ints(row_bytes);
  a.e_lo = ints(row_bytes); a.e_hi = ints(row_bytes); a.e_d2 = ints(row_bytes);
  a.s_lo = ints(row_bytes); a.s_hi = ints(row_bytes); a.s_d2 = ints(row_bytes);
  a.done = reinterpret_cast<uint8_t*>(carve((size_t)n));
  a.sin = ints(scan_bytes); a.sout = ints(scan_bytes);
  const ExScan scan{a.sin, a.sout, ints(1024 * sizeof(int))};
  a.count = ints(sizeof(int)); a.t_dev = ints(sizeof(int));
  if (at > total) return NUHTC_E_HIP;
  if (hipMemsetAsync(a.sin, 0, scan_bytes, s) != hipSuccess || hipMemsetAsync(a.count, 0, sizeof(int), s) != hipSuccess ||
      hipMemsetAsync(a.t_dev, 0, sizeof(int), s) != hipSuccess)
    return NUHTC_E_HIP;
  const unsigned nb = (unsigned)((n + MST_NT - 1) / MST_NT);
  {
    ProfScope ps("cell_mst_bin", 0, 0, s);
    cellbin_launch(a.b, nchunk, s);
  }
  {
    ProfScope ps("cell_mst_init", 0, 0, s);
    hipLaunchKernelGGL(mst_init_kernel, dim3(nb), dim3(MST_NT), 0, s, a);
  }
  int h_count = 0, n_rounds = 0, round = 0;
  for (; round < MST_MAX_ROUNDS; ++round) {
    {
      ProfScope ps("cell_mst_pick", 0, 0, s);
      hipLaunchKernelGGL(mst_pick_kernel, dim3(nb), dim3(MST_NT), 0, s, a);
      hipLaunchKernelGGL(mst_pick_hi_kernel, dim3(nb), dim3(MST_NT), 0, s, a);
    }
    {
      ProfScope ps("cell_mst_emit", 0, 0, s);
      hipLaunchKernelGGL(mst_emit_kernel, dim3(nb), dim3(MST_NT), 0, s, a);
    }
    int now = 0;                                         // the one int a round sends back
    if (!launched() || hipMemcpyAsync(&now, a.count, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
      return NUHTC_E_HIP;
    if (now < h_count || now >= n) return NUHTC_E_HIP;   // a forest of n points has at most n - 1 edges
    if (now == h_count) break;
    h_count = now;
    ++n_rounds;
    ProfScope ps("cell_mst_relabel", 0, 0, s);
    hipLaunchKernelGGL(mst_relabel_kernel, dim3(nb), dim3(MST_NT), 0, s, a);
  }
  if (round == MST_MAX_ROUNDS) return NUHTC_E_HIP;       // round 25 still added edges: not this algorithm any more
  a.m = h_count;
  if (a.m > 0) {
    ProfScope ps("cell_mst_order", 0, 0, s);
    const unsigned eb = (unsigned)((a.m + MST_NT - 1) / MST_NT);
    hipLaunchKernelGGL(mst_count_kernel, dim3(eb), dim3(MST_NT), 0, s, a);
    exscan_launch(scan, fchunk, s);
    hipLaunchKernelGGL(mst_segment_kernel, dim3(eb), dim3(MST_NT), 0, s, a);
    hipLaunchKernelGGL(mst_place_kernel, dim3(eb), dim3(MST_NT), 0, s, a);
  }
  {
    ProfScope ps("cell_mst_number", 0, 0, s);
    hipLaunchKernelGGL(mst_rootflag_kernel, dim3(nb), dim3(MST_NT), 0, s, a);
    exscan_launch(scan, fchunk, s);
    hipLaunchKernelGGL(mst_number_kernel, dim3(nb), dim3(MST_NT), 0, s, a);
  }
  int h_t = 0;
  const int rc = cellbin_finish(a.b, s, a.t_dev, &h_t);
  if (rc == 0) { *m = a.m; *trees = h_t; *rounds = n_rounds; }
  return rc;
}
