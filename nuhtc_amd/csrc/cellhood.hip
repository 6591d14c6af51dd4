// Cellular neighbourhoods of a slide (gfx950): the class composition of every nucleus's window -- itself and the k nearest neighbours
// nuhtc_cell_graph listed -- clustered by k-means into K neighbourhood types, in integers throughout.
//
// Definition (nuhtc_amd/neighbourhoods.py holds it in full, with the numpy restatement `neighbourhoods_reference`): w[i][c] counts the
// rows of label c among row i and its listed neighbours (sum <= 33).  Seeding is k-means++ with exact picks: row_0 = u_0 mod n, then for
// every further centre g_i = the smallest squared distance of w[i] to a chosen window, T = sum g_i, t = u_j mod T and the smallest row
// whose inclusive prefix of g exceeds t (row_0 again when T == 0).  Lloyd runs on centres in fixed point (10 fractional bits):
// a_t[i] = argmin_j sum_c (1024 w[i][c] - q[j][c])^2 with ties to the smaller j; it stops at the first t with a_t == a_{t-1} (converged)
// or at max_iter; otherwise q[j][c] = floor((2048 s_j[c] + m_j) / (2 m_j)) for every type with members.  With given centres: one
// assignment.  Integer adds only: no result depends on the arrival order of an atomic, and the call is bitwise repeatable.
//
// Stages, all on the caller's stream:
//   window   one thread per row gathers the labels of the row's neighbours and counts by class into 16 bytes (C <= 14 counts of at most
//            33), the copy every later pass reads with ONE 128-bit load per row; an index outside -1 .. n - 1 raises the flag and is not
//            followed.  A second kernel, like every kernel from here on a no-op under the flag, writes the int32 `window` output (one
//            thread per entry, coalesced), sets hood to -1 and zeroes the small outputs: a refused call leaves every output untouched.
//   seeding  per further centre two launches: an elementwise min-update of g against the window of the row chosen last (read from
//            seed_rows on the device: nothing comes back to the host per centre) with the sum of each block of 256 rows, and ONE workgroup
//            of 1024 threads that adds the block sums in chunks, scans the chunk sums in int64, finds the chunk, the block and, with an
//            int scan over the block's 256 values of g, the row that the pick rule names, and writes the row and its centre.
//   Lloyd    per iteration two launches.  Assign: the centres (K x 16 int32, zero from C on) sit in LDS; a thread takes its rows in a
//            grid-stride loop, 14 multiply-adds per centre with broadcast LDS reads, writes hood and counts the rows that changed; the
//            members and window sums of a workgroup's rows go into uint32 LDS counters (the non-zero entries of a window only) and are
//            flushed with 64-bit integer atomics.  Update: one workgroup, one thread per centre entry, does the rounding division, records
//            the first iteration without a change and clears the sums.  An iteration after convergence changes nothing, so the host
//            launches HOOD_BATCH iterations at a time and reads the flag and the recorded iteration once per batch; n_iter is what the
//            device recorded.  At t == max_iter the update is withheld, so centre_q is what the last assignment was made against.
//   final    one more assign pass against centre_q that writes hood, centre_sum, centre_n, centre_q and the inertia.
//
// Measured on one MI355X (tools/bench_neighbourhoods.py -> profiles/cell_neighbourhoods.json; 500 000 centres on a 36 000-px square,
// k = 10, 64 px, K = 8, C = 5, medians of 10 calls): 1.41 ms per call on the uniform set (converged at iteration 22, 24 launched: window
// 0.04, seeding 0.07, iterations 0.77, final 0.11) and 1.12 ms on the clustered set (iteration 10, 16 launched), 3.1 x and 1.7 x
// nuhtc_cell_graph at the same k and radius; an assign + update inside a batch takes 0.032 ms.  scikit-learn's Lloyd from the same seeding
// rows on 16 host threads: 101 and 73 ms.
//
// Everything that decides a value, an index or a limit -- the generator, the pick rule, both distances, the rounding, the packing and
// the limits -- is plain C++ in cellhood_host.h, and tools/dev/cellhood_host_check.cpp runs exactly those functions on the host under
// -fsanitize=address,undefined.  The kernel code itself is not sanitized.  Resources: profiles/cell_neighbourhoods_resources.txt.
#include <algorithm>
#include <cstring>

#include "block_prims.h"
#include "cellhood_host.h"
#include "common.h"

namespace {

enum { HOOD_Q_WORDS = HOOD_MAX_TYPES * HOOD_LANES, HOOD_ST_CHANGED = 0, HOOD_ST_CONVERGED = 1 };

struct HoodArgs {
  const int* neighbors;               // [n][k]
  const int* labels;                  // [n]
  int n, k, C, K, nblk;
  int* flag;                          // a neighbour index out of range
  HoodWin* win;                       // [n] the packed windows
  int* g;                             // [n] the seeding distance to the nearest chosen window
  long long* bsum;                    // [nblk] the sum of g over each block of HOOD_NT rows
  int* q16;                           // [HOOD_MAX_TYPES][HOOD_LANES] the centres, zero from C on
  int* state;                         // HOOD_ST_*: the rows that changed in this iteration, the first iteration without a change
  unsigned long long* acc;            // [HOOD_Q_WORDS] window sums + [HOOD_MAX_TYPES] members of the iteration; then the inertia
  int* window; int* hood; int* centre_q; unsigned long long* centre_sum; unsigned long long* centre_n; int* seed_rows;
};

__global__ __launch_bounds__(HOOD_NT) void hood_window_kernel(HoodArgs a) {
  const int i = blockIdx.x * HOOD_NT + threadIdx.x;
  if (i >= a.n) return;
  HoodWin w{0, 0};
  hood_win_add(w, a.labels[i], a.C);
  bool bad = false;
  const int* mine = a.neighbors + (size_t)i * a.k;
  for (int t = 0; t < a.k; ++t) {
    const int j = mine[t];
    if (!hood_neighbour_ok(j, a.n)) bad = true;           // not followed
    else if (j >= 0) hood_win_add(w, a.labels[j], a.C);
  }
  if (bad) atomicOr(a.flag, 1);
  a.win[i] = w;
}

// the int32 windows, hood = -1, the small outputs cleared (seed_rows = -1: what stands with given centres)
__global__ __launch_bounds__(HOOD_NT) void hood_expand_kernel(HoodArgs a) {
  if (*a.flag) return;
  const int C = a.C;
  const long long at = (long long)blockIdx.x * HOOD_NT + threadIdx.x;
  if (at < (long long)a.n * C) {
    const int i = (int)(at / C), c = (int)(at - (long long)i * C);
    a.window[at] = hood_win_at(a.win[i], c);
    if (c == 0) a.hood[i] = -1;
  }
  if (blockIdx.x == 0)
    for (int e = threadIdx.x; e < a.K * C; e += HOOD_NT) {
      a.centre_sum[e] = 0;
      if (e < a.K) { a.centre_n[e] = 0; a.seed_rows[e] = -1; }
    }
}

// the centre of a chosen row: 1024 * its window (the bytes 14 and 15 of a window are zero)
__device__ __forceinline__ void hood_place_centre(const HoodArgs& a, int j, int row, int lane) {
  if (lane < HOOD_LANES) a.q16[j * HOOD_LANES + lane] = lane < CELL_MAX_CLASSES ? HOOD_ONE * hood_win_at(a.win[row], lane) : 0;
  if (lane == 0) a.seed_rows[j] = row;
}

__global__ __launch_bounds__(64) void hood_seed_first_kernel(HoodArgs a, int row0) {
  if (*a.flag) return;
  hood_place_centre(a, 0, row0, threadIdx.x);             // row0 = u_0 mod n < n, taken on the host
}

// g against the window of the centre chosen last, and the sum of each block
__global__ __launch_bounds__(HOOD_NT) void hood_seed_update_kernel(HoodArgs a, int j) {
  __shared__ int wave_total[HOOD_NT / 64];
  if (*a.flag) return;
  const int i = blockIdx.x * HOOD_NT + threadIdx.x;
  const HoodWin last = a.win[a.seed_rows[j - 1]];         // a row: hood_seed_first_kernel / hood_seed_pick_kernel wrote it
  int v = 0;
  if (i < a.n) {
    v = hood_win_d2(a.win[i], last);
    if (j > 1) v = min(v, a.g[i]);
    a.g[i] = v;
  }
  v = wave_sum(v);                                        // <= 64 * 2178
  if ((threadIdx.x & 63) == 0) wave_total[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long s = 0;
    for (int k = 0; k < HOOD_NT / 64; ++k) s += wave_total[k];
    a.bsum[blockIdx.x] = s;
  }
}

// block-wide exclusive scan of one int64 per thread of HOOD_PICK_NT threads (block_exscan of block_prims.h in 64 bits); lds: 17 words
__device__ __forceinline__ long long hood_exscan64(long long v, long long* lds, long long* total) {
  constexpr int NW = HOOD_PICK_NT / 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { long long t = __shfl_up(incl, o); if (lane >= o) incl += t; }
  if (lane == 63) lds[wave] = incl;
  __syncthreads();
  if (wave == 0) {
    long long w = lane < NW ? lds[lane] : 0;
    long long wi = w;
#pragma unroll
    for (int o = 1; o < NW; o <<= 1) { long long t = __shfl_up(wi, o); if (lane >= o) wi += t; }
    if (lane < NW) lds[lane] = wi - w;
    if (lane == NW - 1) lds[NW] = wi;
  }
  __syncthreads();
  const long long res = lds[wave] + incl - v;
  *total = lds[NW];
  __syncthreads();
  return res;
}

// centre j: the row the pick rule names under the draw u
__global__ __launch_bounds__(HOOD_PICK_NT) void hood_seed_pick_kernel(HoodArgs a, int j, unsigned long long u) {
  __shared__ long long lds64[HOOD_PICK_NT / 64 + 1];
  __shared__ int lds32[HOOD_PICK_NT / 64 + 1];
  __shared__ int found_block, found_row;
  __shared__ long long found_rest;
  if (*a.flag) return;
  const int tid = threadIdx.x, chunk = hood_pick_chunk(a.nblk);
  const int b0 = min(tid * chunk, a.nblk), b1 = min(b0 + chunk, a.nblk);
  long long mine = 0;
  for (int b = b0; b < b1; ++b) mine += a.bsum[b];
  long long T;
  const long long before = hood_exscan64(mine, lds64, &T);
  if (tid == 0) { found_block = -1; found_rest = 0; found_row = a.seed_rows[0]; }          // T == 0: row_0 again
  __syncthreads();
  if (T > 0) {                                            // uniform
    const long long t = (long long)(u % (unsigned long long)T);
    if (hood_picks(before, mine, t)) {                    // one thread: the chunks tile the prefix
      long long run = before;
      for (int b = b0; b < b1; ++b) {
        const long long v = a.bsum[b];
        if (hood_picks(run, v, t)) { found_block = b; found_rest = t - run; }
        run += v;
      }
    }
    __syncthreads();
    const int i = found_block * HOOD_NT + tid;            // found_block >= 0: T > 0 and the chunks tile the prefix
    const int v = (found_block >= 0 && tid < HOOD_NT && i < a.n) ? a.g[i] : 0;
    int total;
    const int ex = block_exscan<HOOD_PICK_NT>(v, lds32, &total);
    if (hood_picks(ex, v, found_rest)) found_row = i;     // one thread: found_rest < the block's sum
    __syncthreads();
  }
  hood_place_centre(a, j, found_row, tid);
}

// one assignment of every row against the centres; FINAL: into the outputs, with the inertia
template <bool FINAL>
__global__ __launch_bounds__(HOOD_NT) void hood_assign_kernel(HoodArgs a) {
  __shared__ int q[HOOD_Q_WORDS];
  __shared__ unsigned s[HOOD_Q_WORDS];
  __shared__ unsigned m[HOOD_MAX_TYPES];
  __shared__ unsigned changed;
  if (*a.flag) return;
  const int tid = threadIdx.x, K = a.K;
  for (int e = tid; e < K * HOOD_LANES; e += HOOD_NT) { q[e] = a.q16[e]; s[e] = 0; }
  if (tid < HOOD_MAX_TYPES) m[tid] = 0;
  if (tid == 0) changed = 0;
  __syncthreads();
  int moved = 0;
  long long inertia = 0;
  for (int blk = blockIdx.x; blk < a.nblk; blk += gridDim.x) {
    const int i = blk * HOOD_NT + tid;
    if (i >= a.n) continue;
    const HoodWin w = a.win[i];
    unsigned long long best = hood_distance(w, q);
    int at = 0;
    for (int j = 1; j < K; ++j) {
      const unsigned long long D = hood_distance(w, q + j * HOOD_LANES);
      if (D < best) { best = D; at = j; }                 // strictly: a tie stays with the smaller j
    }
    if (a.hood[i] != at) { ++moved; a.hood[i] = at; }
    if (FINAL) inertia += (long long)best;
    atomicAdd(&m[at], 1u);
#pragma unroll
    for (int c = 0; c < CELL_MAX_CLASSES; ++c) {
      const unsigned v = (unsigned)hood_win_at(w, c);
      if (v) atomicAdd(&s[at * HOOD_LANES + c], v);
    }
  }
  if (!FINAL) {
    moved = wave_sum(moved);
    if ((tid & 63) == 0 && moved) atomicAdd(&changed, (unsigned)moved);
  } else {
    inertia = wave_sum(inertia);
    if ((tid & 63) == 0 && inertia) atomicAdd(&a.acc[HOOD_Q_WORDS + HOOD_MAX_TYPES], (unsigned long long)inertia);
  }
  __syncthreads();
  for (int e = tid; e < K * HOOD_LANES; e += HOOD_NT) {
    const unsigned v = s[e];
    const int j = e / HOOD_LANES, c = e % HOOD_LANES;
    if (FINAL) {
      if (v && c < a.C) atomicAdd(&a.centre_sum[j * a.C + c], (unsigned long long)v);
      if (blockIdx.x == 0 && c < a.C) a.centre_q[j * a.C + c] = q[e];
    } else if (v) {
      atomicAdd(&a.acc[e], (unsigned long long)v);
    }
  }
  if (tid < K && m[tid]) atomicAdd(FINAL ? &a.centre_n[tid] : &a.acc[HOOD_Q_WORDS + tid], (unsigned long long)m[tid]);
  if (!FINAL && tid == 0 && changed) atomicAdd((unsigned*)&a.state[HOOD_ST_CHANGED], changed);
}

// after the assignment of iteration t: the first iteration without a change is recorded; before that, and unless t is the last
// iteration, every type with members gets its rounded mean; the sums are cleared for the next assignment
__global__ __launch_bounds__(HOOD_Q_WORDS) void hood_update_kernel(HoodArgs a, int t, int last) {
  if (*a.flag) return;
  const int e = threadIdx.x, j = e / HOOD_LANES;
  const int changed = a.state[HOOD_ST_CHANGED], converged = a.state[HOOD_ST_CONVERGED];
  const long long sum = (long long)a.acc[e], members = (long long)a.acc[HOOD_Q_WORDS + j];
  __syncthreads();
  if (!converged && changed && !last && j < a.K) a.q16[e] = hood_round(sum, members, a.q16[e]);
  a.acc[e] = 0;
  if (e < HOOD_MAX_TYPES) a.acc[HOOD_Q_WORDS + e] = 0;
  if (e == 0) {
    if (!converged && !changed) a.state[HOOD_ST_CONVERGED] = t;
    a.state[HOOD_ST_CHANGED] = 0;
  }
}

unsigned hood_grid(int64_t items) { return (unsigned)((items + HOOD_NT - 1) / HOOD_NT); }

}  // namespace

extern "C" int nuhtc_neighbourhood_draws(uint32_t seed, int num_types, uint64_t* out) {
  if (num_types < 1 || num_types > HOOD_MAX_TYPES || !out) return NUHTC_E_INVALID;
  for (int j = 0; j < num_types; ++j) out[j] = hood_draw(seed, j);
  return 0;
}

extern "C" int nuhtc_neighbourhood_rule(int what, const int64_t* a, const int64_t* b, int64_t x, int64_t y, int64_t z, int64_t* out) {
  if (!out) return NUHTC_E_INVALID;
  if (what == 0) {                                        // the pick on an inclusive prefix a[0 .. x) at t = y
    if (!a || x < 1 || y < 0 || y >= a[x - 1]) return NUHTC_E_INVALID;
    *out = hood_pick_row(a, x, y);
    return 0;
  }
  if (what == 1) {                                        // the rounding of s = x over m = y, q = z for an empty type
    if (x < 0 || x > HOOD_MAX_POINTS * 33 || y < 0 || y > HOOD_MAX_POINTS || z < 0 || z > HOOD_MAX_CENTRE) return NUHTC_E_INVALID;
    *out = hood_round(x, y, (int)z);
    return 0;
  }
  if (what == 2) {                                        // D of the window a[0 .. x) to the centre b[0 .. y), x == y <= 14
    if (!a || !b || x != y || x < 1 || x > CELL_MAX_CLASSES) return NUHTC_E_INVALID;
    HoodWin w{0, 0};
    int q[HOOD_LANES] = {0};
    for (int c = 0; c < x; ++c) {
      if (a[c] < 0 || a[c] > 33 || !hood_centre_ok((int)b[c]) || b[c] != (int)b[c]) return NUHTC_E_INVALID;
      for (int64_t r = 0; r < a[c]; ++r) hood_win_add(w, c, (int)x);
      q[c] = (int)b[c];
    }
    *out = (int64_t)hood_distance(w, q);
    return 0;
  }
  return NUHTC_E_INVALID;
}

extern "C" int nuhtc_cell_neighbourhoods(int device, const int32_t* neighbors, const int32_t* labels, int64_t n, int k, int num_classes, int num_types,
                                         uint32_t seed, int max_iter, int centres_given, int32_t* centre_q, int32_t* window, int32_t* hood,
                                         int64_t* centre_sum, int64_t* centre_n, int32_t* seed_rows, int64_t* counts, void* stream) {
  if (!counts || !hood_call_ok(n, k, num_classes, num_types, max_iter) || (centres_given != 0 && centres_given != 1)) return NUHTC_E_INVALID;
  if (!centre_q || !centre_sum || !centre_n || !seed_rows || (n > 0 && (!neighbors || !labels || !window || !hood))) return NUHTC_E_INVALID;
  if (hipSetDevice(device) != hipSuccess) return NUHTC_E_HIP;
  hipStream_t s = (hipStream_t)stream;
  const int C = num_classes, K = num_types;
  int q16[HOOD_Q_WORDS];
  memset(q16, 0, sizeof(q16));
  if (centres_given) {                                    // K x C entries: read back, checked here
    int given[HOOD_MAX_TYPES * CELL_MAX_CLASSES];
    if (hipMemcpyAsync(given, centre_q, (size_t)K * C * sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
      return NUHTC_E_HIP;
    for (int e = 0; e < K * C; ++e) {
      if (!hood_centre_ok(given[e])) return NUHTC_E_INVALID;
      q16[(e / C) * HOOD_LANES + e % C] = given[e];
    }
  }
  if (n == 0) {                                           // no row: the centres are the given ones or zeros
    int none[HOOD_MAX_TYPES];
    for (int j = 0; j < K; ++j) none[j] = -1;
    if ((!centres_given && hipMemsetAsync(centre_q, 0, (size_t)K * C * sizeof(int32_t), s) != hipSuccess) ||
        hipMemsetAsync(centre_sum, 0, (size_t)K * C * sizeof(int64_t), s) != hipSuccess || hipMemsetAsync(centre_n, 0, K * sizeof(int64_t), s) != hipSuccess ||
        hipMemcpyAsync(seed_rows, none, K * sizeof(int32_t), hipMemcpyHostToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
      return NUHTC_E_HIP;
    counts[0] = 0; counts[1] = 1; counts[2] = 0;
    return 0;
  }
  HoodArgs a;
  memset(&a, 0, sizeof(a));
  a.neighbors = neighbors; a.labels = labels; a.n = (int)n; a.k = k; a.C = C; a.K = K; a.nblk = hood_blocks(n);
  a.window = window; a.hood = hood; a.centre_q = centre_q; a.seed_rows = seed_rows;
  a.centre_sum = reinterpret_cast<unsigned long long*>(centre_sum); a.centre_n = reinterpret_cast<unsigned long long*>(centre_n);
  DevScratch tmp;      // every temporary of the call, freed on the way out
  const size_t acc_bytes = (HOOD_Q_WORDS + HOOD_MAX_TYPES + 1) * sizeof(unsigned long long);
  a.flag = tmp.alloc<int>(sizeof(int)); a.state = tmp.alloc<int>(2 * sizeof(int));
  a.win = tmp.alloc<HoodWin>((size_t)n * sizeof(HoodWin)); a.g = tmp.alloc<int>((size_t)n * sizeof(int));
  a.bsum = tmp.alloc<long long>((size_t)a.nblk * sizeof(long long)); a.q16 = tmp.alloc<int>(sizeof(q16));
  a.acc = tmp.alloc<unsigned long long>(acc_bytes);
  if (!tmp.ok() || hipMemsetAsync(a.flag, 0, sizeof(int), s) != hipSuccess || hipMemsetAsync(a.state, 0, 2 * sizeof(int), s) != hipSuccess ||
      hipMemsetAsync(a.acc, 0, acc_bytes, s) != hipSuccess || hipMemcpyAsync(a.q16, q16, sizeof(q16), hipMemcpyHostToDevice, s) != hipSuccess)
    return NUHTC_E_HIP;
  {
    ProfScope ps("cell_hood_window", 0, 0, s);
    hipLaunchKernelGGL(hood_window_kernel, dim3(hood_grid(n)), dim3(HOOD_NT), 0, s, a);
    hipLaunchKernelGGL(hood_expand_kernel, dim3(hood_grid(n * C)), dim3(HOOD_NT), 0, s, a);
  }
  const unsigned grid = (unsigned)std::min(a.nblk, 2048);
  int h_state[2] = {0, 0}, h_flag = 0;
  int n_iter = 0;
  if (!centres_given) {
    {
      ProfScope ps("cell_hood_seed", 0, 0, s);
      hipLaunchKernelGGL(hood_seed_first_kernel, dim3(1), dim3(64), 0, s, a, (int)(hood_draw(seed, 0) % (unsigned long long)n));
      for (int j = 1; j < K; ++j) {
        hipLaunchKernelGGL(hood_seed_update_kernel, dim3((unsigned)a.nblk), dim3(HOOD_NT), 0, s, a, j);
        hipLaunchKernelGGL(hood_seed_pick_kernel, dim3(1), dim3(HOOD_PICK_NT), 0, s, a, j, hood_draw(seed, j));
      }
    }
    for (int t = 1; t <= max_iter && !h_state[HOOD_ST_CONVERGED];) {
      {
        ProfScope ps("cell_hood_iterate", 0, 0, s);
        for (int b = 0; b < HOOD_BATCH && t <= max_iter; ++b, ++t) {
          hipLaunchKernelGGL(hood_assign_kernel<false>, dim3(grid), dim3(HOOD_NT), 0, s, a);
          hipLaunchKernelGGL(hood_update_kernel, dim3(1), dim3(HOOD_Q_WORDS), 0, s, a, t, (int)(t == max_iter));
        }
      }
      if (!launched() || hipMemcpyAsync(&h_flag, a.flag, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess ||
          hipMemcpyAsync(h_state, a.state, sizeof(h_state), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return NUHTC_E_HIP;
      if (h_flag) return NUHTC_E_INVALID;
    }
    n_iter = h_state[HOOD_ST_CONVERGED] ? h_state[HOOD_ST_CONVERGED] : max_iter;
  }
  {
    ProfScope ps("cell_hood_final", 0, 0, s);
    hipLaunchKernelGGL(hood_assign_kernel<true>, dim3(grid), dim3(HOOD_NT), 0, s, a);
  }
  unsigned long long inertia = 0;
  if (!launched() || hipMemcpyAsync(&h_flag, a.flag, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipMemcpyAsync(&inertia, a.acc + HOOD_Q_WORDS + HOOD_MAX_TYPES, sizeof(inertia), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return NUHTC_E_HIP;
  if (h_flag) return NUHTC_E_INVALID;
  counts[0] = n_iter; counts[1] = centres_given || h_state[HOOD_ST_CONVERGED] ? 1 : 0; counts[2] = (int64_t)inertia;
  return 0;
}
