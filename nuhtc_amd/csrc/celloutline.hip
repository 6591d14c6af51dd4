// The alpha-shape outline of a slide's nuclei (gfx950): the rings and the components of the alpha complex, traced on the device.
//
// Definition (nuhtc_amd/outline.py holds it in full, with the plain walk `outline_reference`): the input is what nuhtc_cell_alpha left on
// the device -- the edges (i, j) in ascending order, their d2 and their two apexes -- with the points and the labels.  A row is a
// REPRESENTATIVE unless it is the larger end of an edge with d2 == 0; an edge between two representatives is KEPT.  A kept edge with
// exactly one apex is an OUTLINE edge and gives one half-edge, directed with the apex on its left, whose id is the edge's index.  The
// successor of u -> v is the out-half-edge v -> w met first when turning clockwise from v -> u (cellgrid_host.h: outline_better, exact in
// int64); the RINGS are the cycles of that map, led by their smallest id, written from the leader's tail onward and ordered by leader.
// ring_area2 is the shoelace sum relative to the leader's tail in wrap-around 64-bit adds.  Two kept edges with an apex are joined when
// they are sides of one triangle (i, j, apex); a COMPONENT is numbered by the rank of its smallest edge index.  A pure function of the
// input, bitwise the same on every call: atomics are used for integer minima, for counts that are scanned afterwards and for wrap-around
// sums, none of which depends on the order of arrival.
//
// Stages, all on the caller's stream, every one a launch of its own; no kernel waits on another workgroup:
//   mark        rep[row] = row, parent[e] = e; then one thread per edge checks its rows, its apexes and their sides, and that the list
//               ascends (the flag), and takes rep[j] = min(rep[j], i) over the edges with d2 == 0.
//   link        one thread per edge classifies it and counts the out-half-edges per tail; two scans (cellbin.h: exscan_launch) number
//               the outline edges in their order (the half-edge's working index x, so that the smallest x IS the smallest id) and lay the
//               CSR by tail.  (The host reads the flag and h back: a refused input ends here, the outputs untouched.)  The CSR is filled
//               -- the order inside a tail is arrival order, and nothing depends on it -- and one thread per half-edge folds
//               outline_better over the out-half-edges at its head: succ.
//   rank        pointer doubling, ceil(log2 h) rounds of one launch each, ping-pong between two buffers so that a round reads only the
//               previous round's values: (the minimum x over the next 2^k half-edges, the jump over them) until the minimum is the
//               cycle's; then every cycle is cut in front of its leader and (the half-edges up to the end, the jump) are doubled the
//               same way.  The host knows h, so no round is read back.
//   place       two scans over the leaders (the ring's number, the ring's first place); every half-edge writes its tail at (ring,
//               position); one thread per PLACE adds its shoelace term -- a wave whose places all lie in one ring adds them up first.
//   components  cellunion.h over the edge indices: every apexed kept edge finds the two other sides of its triangles by binary search in
//               the edge list and unites with them; the roots (the smallest edge of each component) are numbered by a scan; the rows take
//               the smallest component among their edges by atomicMin, and the rows that are no representatives their representative's.
//
// Every index that depends on the input is compared with its table before it is used: an edge list that is no alpha complex (the
// successor map no bijection) gives rings that mean nothing, but no access leaves a table.
#include <climits>
#include <cstring>

#include "cellbin.h"
#include "cellunion.h"

namespace {

constexpr int OL_NT = 256;
constexpr int OL_NONE = INT_MAX;      // a row no component has reached yet

struct OutlineArgs {
  const int32_t* points; const int32_t* labels;
  const int32_t* edges; const int32_t* edge_d2; const int32_t* apex;
  int n, m, by_class;
  int h, rounds;                      // the half-edges and the doubling rounds: known on the host after the link stage
  int* flag;                          // != 0: the input is refused
  int* totals;                        // [3] h, R, K
  int* rep;                           // [n] the smallest row on the same place (and of the same label, where the alpha complex was by class)
  int* out_flag; int* hid;            // [mpad] 1 for an outline edge, zero past m; the outline edges in front of it
  int* tail_count; int* tail_start;   // [npad] the out-half-edges at every row; those in front of its run in csr
  int* tail_fill;                     // [n]
  int* csr;                           // [h] the half-edges by tail
  int* he_edge; int2* he_ends;        // [h] the edge of a half-edge; its (tail, head)
  int* succ;                          // [h]
  int* mn[2]; int* jp[2];             // [h] ping-pong: the minimum over the next 2^k, the jump over them
  int* dist[2]; int* nx[2];           // [h] ping-pong: the half-edges up to the end of the cut ring (at most 2^k), the jump or -1
  int* lead_flag; int* ring_idx;      // [hpad] 1 for a leader; the leaders in front of it
  int* ring_len; int* ring_off;       // [hpad] the ring's length at its leader; the places in front of the ring
  int* place_ring;                    // [h] the ring of every place of ring_vertex, -1 for a place nobody wrote
  int* parent;                        // [m] the union-find over the edges
  int* root;                          // [m] the root of an apexed kept edge, else -1
  int* root_flag; int* comp_idx;      // [mpad] 1 for a root; the roots in front of it
  int32_t* ring_vertex; int32_t* ring_start; unsigned long long* ring_area2; int32_t* component_of_ring; int32_t* component; int32_t* component_label;
};

__device__ __forceinline__ bool ol_kept(const OutlineArgs& a, int i, int j) { return a.rep[i] == i && a.rep[j] == j; }

__global__ __launch_bounds__(OL_NT) void ol_init_kernel(OutlineArgs a) {
  const int t = blockIdx.x * OL_NT + threadIdx.x;
  if (t < a.n) a.rep[t] = t;
  if (t < a.m) a.parent[t] = t;
}

// one thread per edge: the checks of the entry point, and the representatives
__global__ __launch_bounds__(OL_NT) void ol_mark_kernel(OutlineArgs a) {
  const int e = blockIdx.x * OL_NT + threadIdx.x;
  if (e >= a.m) return;
  const int i = a.edges[2 * e], j = a.edges[2 * e + 1], a0 = a.apex[2 * e], a1 = a.apex[2 * e + 1];
  bool ok = (unsigned)i < (unsigned)a.n && (unsigned)j < (unsigned)a.n && i < j && a0 >= -1 && a0 < a.n && a1 >= -1 && a1 < a.n;
  if (ok && e > 0) {                                     // the list ascends: the binary search of the component stage relies on it
    const int pi = a.edges[2 * e - 2], pj = a.edges[2 * e - 1];
    ok = pi < i || (pi == i && pj < j);
  }
  if (ok) {
    const int ix = a.points[2 * i], iy = a.points[2 * i + 1], jx = a.points[2 * j], jy = a.points[2 * j + 1];
    ok = outline_coord_ok(ix, iy) && outline_coord_ok(jx, jy);
    const int64_t qx = (int64_t)jx - ix, qy = (int64_t)jy - iy;
    if (ok && a0 >= 0) {
      const int kx = a.points[2 * a0], ky = a.points[2 * a0 + 1];
      ok = outline_coord_ok(kx, ky) && outline_side(qx, qy, (int64_t)kx - ix, (int64_t)ky - iy) > 0;
    }
    if (ok && a1 >= 0) {
      const int kx = a.points[2 * a1], ky = a.points[2 * a1 + 1];
      ok = outline_coord_ok(kx, ky) && outline_side(qx, qy, (int64_t)kx - ix, (int64_t)ky - iy) < 0;
    }
  }
  if (!ok) { *a.flag = 1; return; }
  if (a.edge_d2[e] == 0) atomicMin(a.rep + j, i);
}

// 0: set aside or singular, 1: an outline edge, 2: an interior edge
__device__ __forceinline__ int ol_kind(const OutlineArgs& a, int e) {
  const int i = a.edges[2 * e], j = a.edges[2 * e + 1];
  if (!ol_kept(a, i, j)) return 0;
  return (int)(a.apex[2 * e] >= 0) + (int)(a.apex[2 * e + 1] >= 0);
}

// the (tail, head) of the half-edge of outline edge e: the apex on the left
__device__ __forceinline__ int2 ol_ends(const OutlineArgs& a, int e) {
  const int i = a.edges[2 * e], j = a.edges[2 * e + 1];
  return a.apex[2 * e] >= 0 ? make_int2(i, j) : make_int2(j, i);
}

__global__ __launch_bounds__(OL_NT) void ol_classify_kernel(OutlineArgs a) {
  if (*a.flag) return;                                   // a row outside the tables: nothing below may index with it
  const int e = blockIdx.x * OL_NT + threadIdx.x;
  if (e >= a.m) return;
  const bool outline = ol_kind(a, e) == 1;
  a.out_flag[e] = outline;
  if (outline) atomicAdd(a.tail_count + ol_ends(a, e).x, 1);
}

// totals[which] = the sum of `count` scanned values: the last prefix plus the last value
__global__ void ol_total_kernel(OutlineArgs a, const int* in, const int* out, int count, int which) {
  if (*a.flag) return;
  a.totals[which] = count > 0 ? out[count - 1] + in[count - 1] : 0;
}

__global__ __launch_bounds__(OL_NT) void ol_fill_kernel(OutlineArgs a) {
  const int e = blockIdx.x * OL_NT + threadIdx.x;
  if (e >= a.m || !a.out_flag[e]) return;
  const int x = a.hid[e];
  if ((unsigned)x >= (unsigned)a.h) return;              // cannot happen: x counts the outline edges in front of e
  const int2 ends = ol_ends(a, e);
  a.he_edge[x] = e;
  a.he_ends[x] = ends;
  const int at = a.tail_start[ends.x] + atomicAdd(a.tail_fill + ends.x, 1);
  if ((unsigned)at < (unsigned)a.h) a.csr[at] = x;       // always: the run holds tail_count places
}

__global__ __launch_bounds__(OL_NT) void ol_succ_kernel(OutlineArgs a) {
  const int x = blockIdx.x * OL_NT + threadIdx.x;
  if (x >= a.h) return;
  const int2 uv = a.he_ends[x];
  const int64_t vx = a.points[2 * uv.y], vy = a.points[2 * uv.y + 1];
  const int64_t ax = a.points[2 * uv.x] - vx, ay = a.points[2 * uv.x + 1] - vy;
  const int s0 = a.tail_start[uv.y], s1 = min(s0 + a.tail_count[uv.y], a.h);
  int best = -1;
  int64_t bx = 0, by = 0;
  for (int s = s0; s < s1; ++s) {
    const int y = a.csr[s];
    if ((unsigned)y >= (unsigned)a.h) continue;          // cannot happen: every place of the run was filled
    const int w = a.he_ends[y].y;
    const int64_t cx = a.points[2 * w] - vx, cy = a.points[2 * w + 1] - vy;
    if (outline_better(ax, ay, cx, cy, y, bx, by, best)) { best = y; bx = cx; by = cy; }
  }
  if (best < 0) best = x;                                // no out-half-edge at the head (no alpha complex): a ring of its own
  a.succ[x] = best;
  a.mn[0][x] = x;
  a.jp[0][x] = best;
}

__global__ __launch_bounds__(OL_NT) void ol_min_round_kernel(OutlineArgs a, int from) {
  const int x = blockIdx.x * OL_NT + threadIdx.x;
  if (x >= a.h) return;
  const int j = a.jp[from][x];
  a.mn[from ^ 1][x] = min(a.mn[from][x], a.mn[from][j]);
  a.jp[from ^ 1][x] = a.jp[from][j];
}

// the ring is cut in front of its leader: the half-edge whose successor is the leader is the last
__global__ __launch_bounds__(OL_NT) void ol_cut_kernel(OutlineArgs a, int fin) {
  const int x = blockIdx.x * OL_NT + threadIdx.x;
  if (x >= a.h) return;
  const int lead = a.mn[fin][x], nx = a.succ[x] == lead ? -1 : a.succ[x];
  a.nx[0][x] = nx;
  a.dist[0][x] = nx < 0 ? 0 : 1;
  a.lead_flag[x] = lead == x;
}

__global__ __launch_bounds__(OL_NT) void ol_rank_round_kernel(OutlineArgs a, int from) {
  const int x = blockIdx.x * OL_NT + threadIdx.x;
  if (x >= a.h) return;
  const int j = a.nx[from][x];
  int d = a.dist[from][x], nx = j;
  if (j >= 0) { d += a.dist[from][j]; nx = a.nx[from][j]; }
  a.dist[from ^ 1][x] = d;
  a.nx[from ^ 1][x] = nx;
}

__global__ __launch_bounds__(OL_NT) void ol_len_kernel(OutlineArgs a, int fin_min, int fin_rank) {
  const int x = blockIdx.x * OL_NT + threadIdx.x;
  if (x >= a.h) return;
  a.ring_len[x] = a.mn[fin_min][x] == x ? a.dist[fin_rank][x] + 1 : 0;
}

__global__ __launch_bounds__(OL_NT) void ol_place_kernel(OutlineArgs a, int fin_min, int fin_rank) {
  const int x = blockIdx.x * OL_NT + threadIdx.x;
  if (x >= a.h) return;
  const int lead = a.mn[fin_min][x], ring = a.ring_idx[lead], R = a.totals[1];
  const int at = a.ring_off[lead] + a.dist[fin_rank][lead] - a.dist[fin_rank][x];
  if ((unsigned)at < (unsigned)a.h && (unsigned)ring < (unsigned)R) {        // always, for the cycles of a bijection
    a.ring_vertex[at] = a.he_ends[x].x;
    a.place_ring[at] = ring;
  }
  if (lead == x && (unsigned)ring < (unsigned)R) { a.ring_start[ring] = a.ring_off[x]; a.ring_area2[ring] = 0; }
  if (x == 0) a.ring_start[R] = a.h;                     // R <= h <= m: ring_start has m + 1 places
}

// one thread per place: (v[t] - o) x (v[t + 1] - o) with o the ring's first vertex, in wrap-around 64-bit adds
__global__ __launch_bounds__(OL_NT) void ol_area_kernel(OutlineArgs a) {
  const int t = blockIdx.x * OL_NT + threadIdx.x;
  int ring = -1;
  unsigned long long term = 0;
  if (t < a.h) {
    ring = a.place_ring[t];
    if (ring >= 0) {
      const int s0 = a.ring_start[ring], s1 = a.ring_start[ring + 1];
      const int o = a.ring_vertex[s0], p = a.ring_vertex[t], q = a.ring_vertex[t + 1 < s1 ? t + 1 : s0];
      const int64_t ox = a.points[2 * o], oy = a.points[2 * o + 1];
      const int64_t px = a.points[2 * p] - ox, py = a.points[2 * p + 1] - oy, qx = a.points[2 * q] - ox, qy = a.points[2 * q + 1] - oy;
      term = (unsigned long long)(px * qy - py * qx);    // below 2^57 in magnitude
    }
  }
  const int first = __shfl(ring, 0);
  if (__all(ring == first || ring < 0)) {                // one ring in the wave (uniform: every lane takes part)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) term += (unsigned long long)__shfl_xor(term, o);
    if ((threadIdx.x & 63) == 0 && first >= 0 && term) atomicAdd(a.ring_area2 + first, term);
  } else if (ring >= 0 && term) {
    atomicAdd(a.ring_area2 + ring, term);
  }
}

// the index of the edge (lo, hi) in the ascending list, or -1
__device__ __forceinline__ int ol_find_edge(const OutlineArgs& a, int u, int v) {
  const int lo = min(u, v), hi = max(u, v);
  int b = 0, e = a.m;
  while (b < e) {
    const int mid = b + (e - b) / 2;
    const int i = a.edges[2 * mid], j = a.edges[2 * mid + 1];
    if (i < lo || (i == lo && j < hi)) b = mid + 1; else e = mid;
  }
  return b < a.m && a.edges[2 * b] == lo && a.edges[2 * b + 1] == hi ? b : -1;
}

__global__ __launch_bounds__(OL_NT) void ol_unite_kernel(OutlineArgs a) {
  const int e = blockIdx.x * OL_NT + threadIdx.x;
  if (e >= a.m || ol_kind(a, e) == 0) return;
  const int i = a.edges[2 * e], j = a.edges[2 * e + 1];
  for (int c = 0; c < 2; ++c) {
    const int k = a.apex[2 * e + c];
    if (k < 0) continue;
    for (int end = 0; end < 2; ++end) {
      const int f = ol_find_edge(a, end ? j : i, k);
      if (f >= 0 && f != e && ol_kind(a, f) > 0) cc_unite(a.parent, e, f);
    }
  }
}

__global__ __launch_bounds__(OL_NT) void ol_root_kernel(OutlineArgs a) {
  const int e = blockIdx.x * OL_NT + threadIdx.x;
  if (e >= a.m) return;
  const int r = ol_kind(a, e) > 0 ? cc_root(a.parent, e) : -1;
  a.root[e] = r;
  a.root_flag[e] = r == e;
}

__global__ __launch_bounds__(OL_NT) void ol_rows_init_kernel(OutlineArgs a) {
  const int v = blockIdx.x * OL_NT + threadIdx.x;
  if (v < a.n) a.component[v] = OL_NONE;
}

__global__ __launch_bounds__(OL_NT) void ol_rows_min_kernel(OutlineArgs a) {
  const int e = blockIdx.x * OL_NT + threadIdx.x;
  if (e >= a.m) return;
  const int r = a.root[e];
  if (r < 0) return;
  const int c = a.comp_idx[r], i = a.edges[2 * e], j = a.edges[2 * e + 1];
  atomicMin(a.component + i, c);
  atomicMin(a.component + j, c);
  if (r == e) a.component_label[c] = a.by_class ? a.labels[i] : -1;          // c < K <= m
}

// a representative turns "no component" into -1; any other row takes its representative's value (which that row's own thread may or may
// not have turned yet: both readings mean -1)
__global__ __launch_bounds__(OL_NT) void ol_rows_final_kernel(OutlineArgs a) {
  const int v = blockIdx.x * OL_NT + threadIdx.x;
  if (v >= a.n) return;
  const int r = a.rep[v];
  const int c = __hip_atomic_load(a.component + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(a.component + v, c == OL_NONE ? -1 : c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(OL_NT) void ol_ring_component_kernel(OutlineArgs a) {
  const int x = blockIdx.x * OL_NT + threadIdx.x;
  if (x >= a.h || !a.lead_flag[x]) return;
  const int ring = a.ring_idx[x], r = a.root[a.he_edge[x]];
  if ((unsigned)ring < (unsigned)a.totals[1]) a.component_of_ring[ring] = r >= 0 ? a.comp_idx[r] : -1;
}

inline unsigned ol_blocks(int64_t count) { return (unsigned)((count + OL_NT - 1) / OL_NT); }

// a zeroed scan input of `count` values padded to whole chunks, and its output
inline bool ol_scan_pair(DevScratch& tmp, int64_t count, int** in, int** out, int* nchunk, hipStream_t s) {
  *nchunk = (int)((count + CB_CHUNK - 1) / CB_CHUNK);
  if (*nchunk < 1) *nchunk = 1;
  const size_t bytes = (size_t)*nchunk * CB_CHUNK * sizeof(int);
  *in = tmp.alloc<int>(bytes); *out = tmp.alloc<int>(bytes);
  return tmp.ok() && hipMemsetAsync(*in, 0, bytes, s) == hipSuccess;
}

}  // namespace

extern "C" int nuhtc_alpha_outline(int device, const int32_t* points, const int32_t* labels, int64_t n, int by_class, const int32_t* edges,
                                   const int32_t* edge_d2, const int32_t* apex, int64_t m, int32_t* ring_vertex, int32_t* ring_start,
                                   int64_t* ring_area2, int32_t* component_of_ring, int32_t* component, int32_t* component_label,
                                   int64_t* counts, void* stream) {
  if (!counts || !ring_start || !outline_call_ok(n, m, by_class)) return NUHTC_E_INVALID;
  if (n > 0 && (!points || !labels || !component)) return NUHTC_E_INVALID;
  if (m > 0 && (n == 0 || !edges || !edge_d2 || !apex || !ring_vertex || !ring_area2 || !component_of_ring || !component_label)) return NUHTC_E_INVALID;
  if (hipSetDevice(device) != hipSuccess) return NUHTC_E_HIP;
  hipStream_t s = (hipStream_t)stream;
  OutlineArgs a;
  memset(&a, 0, sizeof(a));
  a.points = points; a.labels = labels; a.edges = edges; a.edge_d2 = edge_d2; a.apex = apex;
  a.n = (int)n; a.m = (int)m; a.by_class = by_class;
  a.ring_vertex = ring_vertex; a.ring_start = ring_start; a.ring_area2 = reinterpret_cast<unsigned long long*>(ring_area2);
  a.component_of_ring = component_of_ring; a.component = component; a.component_label = component_label;
  if (m == 0) {                                          // no edge: no ring and no component; every row is in no triangle
    if (hipMemsetAsync(ring_start, 0, sizeof(int32_t), s) != hipSuccess) return NUHTC_E_HIP;
    if (n > 0 && hipMemsetAsync(component, 0xff, (size_t)n * sizeof(int32_t), s) != hipSuccess) return NUHTC_E_HIP;
    if (hipStreamSynchronize(s) != hipSuccess) return NUHTC_E_HIP;
    counts[0] = counts[1] = counts[2] = 0;
    return 0;
  }
  DevScratch tmp;      // every temporary of the call, freed on the way out
  int mchunk = 0, nchunk = 0, hchunk = 0, unused = 0;
  a.flag = tmp.alloc<int>(sizeof(int)); a.totals = tmp.alloc<int>(3 * sizeof(int));
  a.rep = tmp.alloc<int>((size_t)n * sizeof(int)); a.tail_fill = tmp.alloc<int>((size_t)n * sizeof(int));
  a.parent = tmp.alloc<int>((size_t)m * sizeof(int)); a.root = tmp.alloc<int>((size_t)m * sizeof(int));
  if (!tmp.ok() || !ol_scan_pair(tmp, m, &a.out_flag, &a.hid, &mchunk, s) || !ol_scan_pair(tmp, n, &a.tail_count, &a.tail_start, &nchunk, s) ||
      !ol_scan_pair(tmp, m, &a.root_flag, &a.comp_idx, &unused, s))
    return NUHTC_E_HIP;
  int* chunk_base = tmp.alloc<int>(1024 * sizeof(int));
  if (!tmp.ok() || hipMemsetAsync(a.flag, 0, sizeof(int), s) != hipSuccess || hipMemsetAsync(a.totals, 0, 3 * sizeof(int), s) != hipSuccess ||
      hipMemsetAsync(a.tail_fill, 0, (size_t)n * sizeof(int), s) != hipSuccess)
    return NUHTC_E_HIP;
  {
    ProfScope ps("cell_outline_mark", 0, 0, s);
    hipLaunchKernelGGL(ol_init_kernel, dim3(ol_blocks(n > m ? n : m)), dim3(OL_NT), 0, s, a);
    hipLaunchKernelGGL(ol_mark_kernel, dim3(ol_blocks(m)), dim3(OL_NT), 0, s, a);
  }
  {
    ProfScope ps("cell_outline_link", 0, 0, s);
    hipLaunchKernelGGL(ol_classify_kernel, dim3(ol_blocks(m)), dim3(OL_NT), 0, s, a);
    exscan_launch(ExScan{a.out_flag, a.hid, chunk_base}, mchunk, s);
    exscan_launch(ExScan{a.tail_count, a.tail_start, chunk_base}, nchunk, s);
    hipLaunchKernelGGL(ol_total_kernel, dim3(1), dim3(1), 0, s, a, (const int*)a.out_flag, (const int*)a.hid, (int)m, 0);
  }
  int h_flag = 0, h_tot[3] = {0, 0, 0};
  if (!launched() || hipMemcpyAsync(&h_flag, a.flag, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipMemcpyAsync(h_tot, a.totals, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
    return NUHTC_E_HIP;
  if (h_flag) return NUHTC_E_INVALID;
  a.h = h_tot[0];
  if (a.h < 0 || a.h > a.m) return NUHTC_E_HIP;
  a.rounds = outline_rounds(a.h);
  if (a.h > 0) {
    const size_t hb = (size_t)a.h * sizeof(int);
    a.csr = tmp.alloc<int>(hb); a.he_edge = tmp.alloc<int>(hb); a.he_ends = tmp.alloc<int2>((size_t)a.h * sizeof(int2));
    a.succ = tmp.alloc<int>(hb); a.place_ring = tmp.alloc<int>(hb);
    for (int k = 0; k < 2; ++k) { a.mn[k] = tmp.alloc<int>(hb); a.jp[k] = tmp.alloc<int>(hb); a.dist[k] = tmp.alloc<int>(hb); a.nx[k] = tmp.alloc<int>(hb); }
    if (!tmp.ok() || !ol_scan_pair(tmp, a.h, &a.lead_flag, &a.ring_idx, &hchunk, s) || !ol_scan_pair(tmp, a.h, &a.ring_len, &a.ring_off, &unused, s))
      return NUHTC_E_HIP;
    if (hipMemsetAsync(a.csr, 0xff, hb, s) != hipSuccess || hipMemsetAsync(a.place_ring, 0xff, hb, s) != hipSuccess) return NUHTC_E_HIP;
    const unsigned hbk = ol_blocks(a.h);
    {
      ProfScope ps("cell_outline_link", 0, 0, s);
      hipLaunchKernelGGL(ol_fill_kernel, dim3(ol_blocks(m)), dim3(OL_NT), 0, s, a);
      hipLaunchKernelGGL(ol_succ_kernel, dim3(hbk), dim3(OL_NT), 0, s, a);
    }
    int fin_min = 0, fin_rank = 0;
    {
      ProfScope ps("cell_outline_rank", 0, 0, s);
      for (int k = 0; k < a.rounds; ++k, fin_min ^= 1) hipLaunchKernelGGL(ol_min_round_kernel, dim3(hbk), dim3(OL_NT), 0, s, a, fin_min);
      hipLaunchKernelGGL(ol_cut_kernel, dim3(hbk), dim3(OL_NT), 0, s, a, fin_min);
      for (int k = 0; k < a.rounds; ++k, fin_rank ^= 1) hipLaunchKernelGGL(ol_rank_round_kernel, dim3(hbk), dim3(OL_NT), 0, s, a, fin_rank);
    }
    {
      ProfScope ps("cell_outline_place", 0, 0, s);
      hipLaunchKernelGGL(ol_len_kernel, dim3(hbk), dim3(OL_NT), 0, s, a, fin_min, fin_rank);
      exscan_launch(ExScan{a.lead_flag, a.ring_idx, chunk_base}, hchunk, s);
      exscan_launch(ExScan{a.ring_len, a.ring_off, chunk_base}, hchunk, s);
      hipLaunchKernelGGL(ol_total_kernel, dim3(1), dim3(1), 0, s, a, (const int*)a.lead_flag, (const int*)a.ring_idx, a.h, 1);
      hipLaunchKernelGGL(ol_place_kernel, dim3(hbk), dim3(OL_NT), 0, s, a, fin_min, fin_rank);
      hipLaunchKernelGGL(ol_area_kernel, dim3(hbk), dim3(OL_NT), 0, s, a);
    }
  } else if (hipMemsetAsync(ring_start, 0, sizeof(int32_t), s) != hipSuccess) {
    return NUHTC_E_HIP;
  }
  {
    ProfScope ps("cell_outline_components", 0, 0, s);
    hipLaunchKernelGGL(ol_unite_kernel, dim3(ol_blocks(m)), dim3(OL_NT), 0, s, a);
    hipLaunchKernelGGL(ol_root_kernel, dim3(ol_blocks(m)), dim3(OL_NT), 0, s, a);
    exscan_launch(ExScan{a.root_flag, a.comp_idx, chunk_base}, mchunk, s);
    hipLaunchKernelGGL(ol_total_kernel, dim3(1), dim3(1), 0, s, a, (const int*)a.root_flag, (const int*)a.comp_idx, (int)m, 2);
    hipLaunchKernelGGL(ol_rows_init_kernel, dim3(ol_blocks(n)), dim3(OL_NT), 0, s, a);
    hipLaunchKernelGGL(ol_rows_min_kernel, dim3(ol_blocks(m)), dim3(OL_NT), 0, s, a);
    hipLaunchKernelGGL(ol_rows_final_kernel, dim3(ol_blocks(n)), dim3(OL_NT), 0, s, a);
    if (a.h > 0) hipLaunchKernelGGL(ol_ring_component_kernel, dim3(ol_blocks(a.h)), dim3(OL_NT), 0, s, a);
  }
  if (!launched() || hipMemcpyAsync(h_tot, a.totals, 3 * sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
    return NUHTC_E_HIP;
  counts[0] = a.h; counts[1] = h_tot[1]; counts[2] = h_tot[2];
  return 0;
}
