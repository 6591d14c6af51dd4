// Nucleus clusters of a slide (gfx950): DBSCAN over the cell grid, with a lock-free union of the core points.
//
// Definition (nuhtc_amd/clusters.py holds it in full, with the int64 brute-force restatement `cluster_reference`): n points in HALF pixels
// (|p| < 2^27, n <= 2^24), one label each, a radius r in half pixels (1 .. 16384), min_pts >= 1, by_class in {0, 1}.  adj(i, j) holds when
// dx * dx + dy * dy <= r * r (inclusive; adj(i, i) holds) and, with by_class, labels[i] == labels[j] (plain equality).  degree[i] counts
// the j with adj(i, j), i itself among them; i is a core point when degree[i] >= min_pts.  Clusters are the connected components of adj
// among core points; the root of a cluster is its smallest core row.  A non-core point joins the cluster of the adjacent core point with
// the smallest key (d2, j) -- a border point -- or is noise (cluster -1).  Clusters are numbered 0 .. m - 1 by ascending root.  Integer
// arithmetic only: the result is a pure function of the input and bitwise the same on every call.
//
// Stages, all on the caller's stream, every one a launch of its own; no kernel waits on another workgroup:
//   binning    cellbin.h, reach r, ONE key per cell in both modes.  by_class compares the label in the sweep (`o.z != me.z`, cc_sweep) and
//              does not sort on (cell, class): those keys fold every label outside 0 .. C - 1 into one run, while adjacency here is plain
//              equality of labels, so the run of "the others" would need the compare anyway; one key per cell keeps the graph's 2^22-cell
//              grid and one set of kernels for both modes, and the compare costs one instruction on a record that is loaded in any case.
//   degree     one thread per record in cell order, the 3 x 3 sweep of cellbin.h (cell_sweep, the point itself included).  Writes
//              degree and core by original row, the degree again in CELL order (rdeg: the later sweeps read a candidate's core flag next
//              to its record, not through its row), and parent[row] = row for a core point.
//   hook       every core point sweeps once more and unites itself with each adjacent core point of a SMALLER row (every pair once).
//              unite(a, b): find both roots; link the larger root under the smaller with atomicCAS(parent + hi, hi, lo); when the CAS
//              fails, hi is no root any more and the value the CAS returned is its parent: go on from there.  After a failure the larger
//              of the two roots is strictly smaller than before, so a thread's loop is bounded by its own arithmetic: nothing spins on a
//              value another wave must produce, and there is no barrier across workgroups and no cooperative launch.  parent[x] <= x
//              always holds (a root is only ever linked under a smaller index; the path halving below writes an ancestor with atomicMin),
//              so the smallest row of a component is a root for ever and the final root IS that row: canonical with no further pass.
//              Reads of parent in this kernel are relaxed agent-scope atomic loads; a stale value is an earlier parent of the same entry,
//              hence a point of the same component at or above the current parent, and the CAS (which fails on a stale root) is what
//              decides.  The find halves the path it walks (atomicMin(parent + x, grandparent), no return value).
//   resolve    core points walk to their root (plain loads: the hooking is a finished launch).  A non-core point with degree > 1 sweeps
//              for the smallest (d2 << 32 | j) among its adjacent core points and takes that point's root; the others are noise (-1).
//              Writes root[row] and rootflag[row] = 1 where root == row.
//   numbering  exclusive scan of rootflag into rank by the scan of cellbin.h (exscan_launch) -- at most 1024 chunks of 16384 flags, which
//              is why n <= 2^24.  Then cluster[i] = rank[root[i]], the row rank[i] of every table is cleared where rootflag[i] (bbox to
//              its identity), and m = rank[n - 1] + rootflag[n - 1].
//   tables     one thread per record in cell order; 32-bit atomic adds for size, n_core and class_count, 64-bit adds for sum_xy, atomic
//              min / max for bbox.  Threads run in cell order, so a wave holds few clusters: the wave takes the cluster of its first
//              uncounted lane, reduces over the lanes of that cluster (ballot counts, wave_sum / wave_min / wave_max of block_prims.h
//              with the other lanes at the identity), that lane makes the 7 + C atomics, and the loop goes on with the lanes that are
//              left -- one round per distinct cluster in the wave, at most 64, each retiring at least its leader.  A wave in one cluster
//              is the one-round case.  The first version reduced only when all 64 lanes agreed and fell back to per-lane atomics; on
//              the clustered benchmark set (10 695 clusters, the largest 5870 nuclei) almost no wave agreed and the stage took 0.58 ms
//              of 1.06 ms of kernels, so the per-cluster rounds replaced it.  Integer sums: order does not matter.
//
// A point outside the stated box raises the binning's flag; every later kernel tests it and writes no output (the scan kernels run on
// temporaries only), and the call returns NUHTC_E_INVALID.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, profiles/cell_clusters_resources.txt), VGPRs / SGPRs: the three sweeps --
// cc_degree_kernel 22 / 38, cc_hook_kernel 22 / 44, cc_resolve_kernel 23 / 48 -- no scratch and no LDS in any of them; cc_number_kernel
// 14 / 28, cc_tables_kernel 36 / 32 (wave shuffles only), neither with scratch or LDS.  Registers and LDS never limit the occupancy (8
// waves per SIMD everywhere): the 32-wave cap of a CU does.
#include <algorithm>
#include <climits>
#include <cstring>

#include "cellbin.h"
#include "cellunion.h"

namespace {

constexpr int CC_MAX_CELLS = 1 << 22;
constexpr int64_t CC_MAX_POINTS = (int64_t)1 << 24;    // 1024 scan chunks of CB_CHUNK root flags
constexpr int CC_NT = 256;

struct CellClusterArgs {
  CellBin b;                // the points, the grid and the records in cell order (cellbin.h, one key per cell)
  int n, C, r, min_pts, by_class;
  int* rdeg;                // [n] the degree of the record at this position of the cell order
  int* parent;              // [n] by row: the union-find forest of the core points (parent <= row), -1 for a non-core point
  int* root;                // [n] by row: the root of the point's cluster, -1 for noise
  int* rootflag;            // [nchunk * CB_CHUNK] by row: 1 at a root, zero elsewhere and past n
  int* rank;                // [nchunk * CB_CHUNK]: roots in front of row i = the cluster number of a root
  int* m_dev;
  int32_t* cluster;         // [n]
  uint8_t* core;            // [n]
  int32_t* degree;          // [n]
  int32_t* size;            // [n rows of capacity] from here on; m rows are written
  int32_t* n_core;
  int32_t* class_count;     // [.][C]
  unsigned long long* sum_xy;   // [.][2]
  int32_t* bbox;            // [.][4] x_min, y_min, x_max, y_max
};

// f(j, o, d2) for every record o at position j with adj(me, o), the point itself included
template <typename F>
__device__ __forceinline__ void cc_sweep(const CellBin& g, const int4 me, int r, int by_class, F&& f) {
  cell_sweep(g, me, r, [&](const int4& o) { return !by_class || o.z == me.z; }, f);
}

__global__ __launch_bounds__(CC_NT) void cc_degree_kernel(CellClusterArgs a) {
  const CellBin& g = a.b;
  if (*g.flag) return;                                   // the binning met a point outside the box: nothing is written
  const int q = blockIdx.x * CC_NT + threadIdx.x;
  if (q >= a.n) return;
  const int4 me = g.recs[q];
  int deg = 0;
  cc_sweep(g, me, a.r, a.by_class, [&](int, const int4&, int) { ++deg; });
  const bool core = deg >= a.min_pts;
  a.rdeg[q] = deg;
  a.degree[me.w] = deg;
  a.core[me.w] = core ? 1 : 0;
  a.parent[me.w] = core ? me.w : -1;
}

// cc_load, cc_find, cc_unite and cc_root: cellunion.h, shared with cellmst.hip

__global__ __launch_bounds__(CC_NT) void cc_hook_kernel(CellClusterArgs a) {
  const CellBin& g = a.b;
  if (*g.flag) return;
  const int q = blockIdx.x * CC_NT + threadIdx.x;
  if (q >= a.n || a.rdeg[q] < a.min_pts) return;
  const int4 me = g.recs[q];
  const int min_pts = a.min_pts;
  cc_sweep(g, me, a.r, a.by_class, [&](int j, const int4& o, int) {
    if (o.w < me.w && a.rdeg[j] >= min_pts) cc_unite(a.parent, me.w, o.w);
  });
}

__global__ __launch_bounds__(CC_NT) void cc_resolve_kernel(CellClusterArgs a) {
  const CellBin& g = a.b;
  if (*g.flag) return;
  const int q = blockIdx.x * CC_NT + threadIdx.x;
  if (q >= a.n) return;
  const int4 me = g.recs[q];
  const int deg = a.rdeg[q], min_pts = a.min_pts;
  int root = -1;
  if (deg >= min_pts) {
    root = cc_root(a.parent, me.w);
  } else if (deg > 1) {                                  // a point alone in its disc has no core point to join
    unsigned long long best = ~0ull;
    cc_sweep(g, me, a.r, a.by_class, [&](int j, const int4& o, int dd) {
      if (a.rdeg[j] >= min_pts) best = min(best, ((unsigned long long)(unsigned)dd << 32) | (unsigned)o.w);
    });
    if (best != ~0ull) root = cc_root(a.parent, (int)(unsigned)best);
  }
  a.root[me.w] = root;
  if (root == me.w) a.rootflag[me.w] = 1;
}

__global__ __launch_bounds__(CC_NT) void cc_number_kernel(CellClusterArgs a) {
  if (*a.b.flag) return;
  const int i = blockIdx.x * CC_NT + threadIdx.x;
  if (i >= a.n) return;
  const int root = a.root[i], isroot = a.rootflag[i], mine = a.rank[i];
  a.cluster[i] = root < 0 ? -1 : a.rank[root];
  if (isroot) {                                          // row `mine` of the tables: cleared, the box to the identity of min / max
    a.size[mine] = 0;
    a.n_core[mine] = 0;
    for (int c = 0; c < a.C; ++c) a.class_count[(size_t)mine * a.C + c] = 0;
    a.sum_xy[2 * (size_t)mine] = 0; a.sum_xy[2 * (size_t)mine + 1] = 0;
    int32_t* bb = a.bbox + 4 * (size_t)mine;
    bb[0] = INT_MAX; bb[1] = INT_MAX; bb[2] = INT_MIN; bb[3] = INT_MIN;
  }
  if (i == a.n - 1) *a.m_dev = mine + isroot;
}

__device__ __forceinline__ void cc_table_add(const CellClusterArgs& a, int row, int cnt, int ncore, long long sx, long long sy, int x0, int y0, int x1, int y1) {
  atomicAdd(a.size + row, cnt);
  if (ncore) atomicAdd(a.n_core + row, ncore);
  atomicAdd(a.sum_xy + 2 * (size_t)row, (unsigned long long)sx);
  atomicAdd(a.sum_xy + 2 * (size_t)row + 1, (unsigned long long)sy);
  int32_t* bb = a.bbox + 4 * (size_t)row;
  atomicMin(bb, x0); atomicMin(bb + 1, y0); atomicMax(bb + 2, x1); atomicMax(bb + 3, y1);
}

__global__ __launch_bounds__(CC_NT) void cc_tables_kernel(CellClusterArgs a) {
  const CellBin& g = a.b;
  if (*g.flag) return;                                   // uniform
  const int q = blockIdx.x * CC_NT + threadIdx.x;
  const bool active = q < a.n;                           // every lane of a wave takes part in the reductions
  const int4 me = active ? g.recs[q] : make_int4(0, 0, -1, -1);
  const int row = active ? a.cluster[me.w] : -1;
  const int core = active && a.rdeg[q] >= a.min_pts;
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(row >= 0);          // the lanes not yet counted: the same value in every lane, so the loop is uniform
  while (todo) {
    const int leader = __ffsll(todo) - 1;
    const int crow = __shfl(row, leader);
    const bool in = row == crow;                         // the lanes of the leader's cluster (crow >= 0: no idle or noise lane)
    const unsigned long long mask = __ballot(in);
    const int ncore = __popcll(__ballot(in && core));
    const long long sx = wave_sum(in ? (long long)me.x : 0ll), sy = wave_sum(in ? (long long)me.y : 0ll);
    const int x0 = wave_min(in ? me.x : INT_MAX), y0 = wave_min(in ? me.y : INT_MAX);
    const int x1 = wave_max(in ? me.x : INT_MIN), y1 = wave_max(in ? me.y : INT_MIN);
    if (lane == leader) cc_table_add(a, crow, __popcll(mask), ncore, sx, sy, x0, y0, x1, y1);
    for (int c = 0; c < a.C; ++c) {
      const int k = __popcll(__ballot(in && me.z == c));
      if (lane == leader && k) atomicAdd(a.class_count + (size_t)crow * a.C + c, k);
    }
    todo &= ~mask;
  }
}

}  // namespace

extern "C" int nuhtc_cell_clusters(int device, const int32_t* points, const int32_t* labels, int64_t n, int num_classes, int r, int min_pts,
                                   int by_class, int x_min, int y_min, int x_max, int y_max, int32_t* cluster, uint8_t* core, int32_t* degree,
                                   int32_t* size, int32_t* n_core, int32_t* class_count, int64_t* sum_xy, int32_t* bbox, int64_t* m, void* stream) {
  if (!cell_call_ok(n, CC_MAX_POINTS, num_classes, r, x_min, y_min, x_max, y_max) || min_pts < 1 || (by_class != 0 && by_class != 1) || !m)
    return NUHTC_E_INVALID;
  if (n > 0 && (!points || !labels || !cluster || !core || !degree || !size || !n_core || !class_count || !sum_xy || !bbox)) return NUHTC_E_INVALID;
  if (n == 0) { *m = 0; return 0; }
  if (hipSetDevice(device) != hipSuccess) return NUHTC_E_HIP;
  hipStream_t s = (hipStream_t)stream;
  CellClusterArgs a;
  memset(&a, 0, sizeof(a));
  a.n = (int)n; a.C = num_classes; a.r = r; a.min_pts = min_pts; a.by_class = by_class;
  a.cluster = cluster; a.core = core; a.degree = degree; a.size = size; a.n_core = n_core; a.class_count = class_count;
  a.sum_xy = reinterpret_cast<unsigned long long*>(sum_xy); a.bbox = bbox;
  DevScratch tmp;      // every temporary of the call, freed on the way out
  const int nchunk = cellbin_setup(a.b, points, labels, (int)n, x_min, y_min, x_max, y_max, r, CC_MAX_CELLS, 1, tmp, s);
  if (!nchunk) return NUHTC_E_HIP;
  const int fchunk = (int)((n + CB_CHUNK - 1) / CB_CHUNK);                 // scan chunks of the root flags: at most 1024
  const size_t flag_bytes = (size_t)fchunk * CB_CHUNK * sizeof(int);
  a.rdeg = tmp.alloc<int>((size_t)n * sizeof(int)); a.parent = tmp.alloc<int>((size_t)n * sizeof(int)); a.root = tmp.alloc<int>((size_t)n * sizeof(int));
  a.rootflag = tmp.alloc<int>(flag_bytes); a.rank = tmp.alloc<int>(flag_bytes); a.m_dev = tmp.alloc<int>(sizeof(int));
  const ExScan scan{a.rootflag, a.rank, tmp.alloc<int>(1024 * sizeof(int))};
  if (!tmp.ok()) return NUHTC_E_HIP;
  if (hipMemsetAsync(a.rootflag, 0, flag_bytes, s) != hipSuccess || hipMemsetAsync(a.m_dev, 0, sizeof(int), s) != hipSuccess) return NUHTC_E_HIP;
  const unsigned nb = (unsigned)((n + CC_NT - 1) / CC_NT);
  {
    ProfScope ps("cell_clusters_bin", 0, 0, s);
    cellbin_launch(a.b, nchunk, s);
  }
  {
    ProfScope ps("cell_clusters_degree", 0, 0, s);
    hipLaunchKernelGGL(cc_degree_kernel, dim3(nb), dim3(CC_NT), 0, s, a);
  }
  {
    ProfScope ps("cell_clusters_hook", 0, 0, s);
    hipLaunchKernelGGL(cc_hook_kernel, dim3(nb), dim3(CC_NT), 0, s, a);
  }
  {
    ProfScope ps("cell_clusters_resolve", 0, 0, s);
    hipLaunchKernelGGL(cc_resolve_kernel, dim3(nb), dim3(CC_NT), 0, s, a);
  }
  {
    ProfScope ps("cell_clusters_number", 0, 0, s);
    exscan_launch(scan, fchunk, s);
    hipLaunchKernelGGL(cc_number_kernel, dim3(nb), dim3(CC_NT), 0, s, a);
  }
  {
    ProfScope ps("cell_clusters_tables", 0, 0, s);
    hipLaunchKernelGGL(cc_tables_kernel, dim3(nb), dim3(CC_NT), 0, s, a);
  }
  int h_m = 0;
  const int rc = cellbin_finish(a.b, s, a.m_dev, &h_m);
  if (rc == 0) *m = h_m;
  return rc;
}
