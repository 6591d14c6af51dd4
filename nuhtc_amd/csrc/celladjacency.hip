// Territory adjacency of a slide (gfx950): the discrete Delaunay graph of the nucleus centres, read off the owner map of the nucleus
// territories (cellterritory.hip) -- which nuclei are neighbours, and how long their common border is.
//
// Definition (nuhtc_amd/adjacency.py holds it in full, with the numpy restatement `adjacency_reference`): an owner map int32 (H, W) with
// entries in -1 .. n - 1 (W * H <= 2^28, n <= 2^24).  A SITE PAIR is an unordered pair of 4-adjacent sites inside the window, counted once.
// {i, j}, i < j, is an EDGE when some site pair has the owners i and j, both >= 0; shared[i, j] is the number of such site pairs; degree[i]
// is the number of distinct neighbours of row i.  The edges come out in ascending (i, j) order.  Integer adds and a rank only: a pure
// function of the map, bitwise the same on every call.  4-adjacency, as in the territories' `contact`: two territories that meet only
// diagonally are not adjacent.  The entry point takes the map, not the points: it needs nothing else, and cellterritory.hip stays as it is.
//
// Stages, all on the caller's stream, every one a launch of its own; no kernel waits on another workgroup, and every loop runs over a
// range of a table (a probe is bounded by the table's slot count and ends far earlier: both tables are at most half full):
//   count      adj_tile_kernel<false>: one workgroup per tile of 16 x 16 sites, one thread per site.  The thread checks its own owner
//              (adj_owner_ok: -1 .. n - 1, else the call's `bad` flag) and takes its right and its lower site pair inside the window
//              (adj_site_pairs: the tile reads a one-site halo on those two sides, straight from the map).  The key of a pair that is an
//              edge (adj_key) goes into the tile's LDS table of 1024 slots by a 64-bit compare-and-swap; every thread that finds its slot
//              empty has met a key new to the tile: one RECORD.  The records of the call, M, are summed in 64 bits: one atomic per workgroup,
//              spread over 256 words that the host adds up.
//              No owner is an index here: the keys index the table through their hash.
//   (the host reads M and the flag back -- the only synchronisation inside the call.  A bad owner: NUHTC_E_INVALID, nothing written.
//    Every table below is sized from M and allocated from the call's DevScratch BEFORE an output is touched.)
//   insert     degree and the tables cleared; adj_tile_kernel<true>: the same tile pass with a 32-bit count beside every LDS key, then
//              every occupied LDS slot goes into the call's open-addressing table of next_pow2(2 M) slots (adj_table_insert: a 64-bit
//              compare-and-swap on the key, a 32-bit add of the tile's count).  The thread that fills a slot has met the edge for the
//              first time: one more at up[i] (the edges whose SMALLER row is i) and at degree[i] and degree[j].
//   scan       exscan_launch over up: the segment of every row.  m = start[n - 1] + up[n - 1], read on the DEVICE by the place stage and
//              on the host at the end of the call.
//   place      only when m <= edge_cap (tested by every thread).  adj_gather_kernel: one thread per slot of the table; an occupied slot
//              takes the next free place of its row's segment (an atomic on fill[i]: arrival order), where i goes into `edges` and (j,
//              shared) into two temporaries.  adj_place_kernel: one thread per edge; its place in the segment is the number of edges
//              there with a smaller j (cell_rank_in_segment of cellgrid_host.h, shared with cellprox.hip, cellalpha.hip and
//              cellmst.hip), where j and shared go.  Nothing of the arrival order or of the hash survives.
//
// The rank costs (up-degree)^2 loads per row.  The up-degree is at most min(n - 1, 4 A) with A the sites a row owns; on a map of the
// territories a row owns sites within the reach R of its point only, so A <= (floor(2 R / s) + 1)^2 whatever the points do; a territory
// between Voronoi neighbours has a handful.  A designed map may have a long row (tests/test_hip_adjacency.py: 300 neighbours): it costs
// time, not correctness.
//
// Capacity protocol (cellprox.hip's): degree and m are always written; with m > edge_cap `edges` and `shared` stay untouched and one more
// call with edge_cap >= m succeeds with the same m.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, profiles/cell_adjacency_resources.txt): no scratch in any kernel;
// adj_tile_kernel<false> 14 VGPRs and 8,448 B of LDS, adj_tile_kernel<true> 19 and 12,544 B, adj_gather_kernel 12 and adj_place_kernel 14 VGPRs, no LDS;
// registers allow 8 waves per SIMD in all of them.
//
// Everything that decides an index or a limit -- the key and its halves, the slot hash, the slot count from M, the argument check, the
// owner check, the site of a thread (site_uv) and the pairs of a site at the window's edge (cellgrid_host.h) -- is plain C++, and tools/dev/celladjacency_host_check.cpp
// runs exactly those functions on the host under -fsanitize=address,undefined.  The kernel code itself is not sanitized.
//
// MEASURED on one MI355X (tools/bench_adjacency.py -> profiles/cell_adjacency.json; 500 000 centres on a 36 000-px square, reach 64 px,
// C = 5, medians of 10 calls on the resident owner map, every call bitwise equal to the first; the territory call that writes the map, timed
// the same way, beside it).  Pitch 4 px, 81.6 M sites: 2.50 ms per call uniform for 1.46 M edges (count 0.48, insert 0.88, place 0.16; the
// rest is the call's allocations, memsets and two synchronisations) beside 2.11 ms for the territories, and 2.14 ms clustered for 1.42 M
// edges (0.36 / 0.68 / 0.13) beside 1.85.  Pitch 32 px, 1.27 M sites: 1.21 ms for 1.21 M edges (0.02 / 0.26 / 0.09) beside 0.46, and 1.06 ms
// for 0.68 M edges (0.02 / 0.16 / 0.06) beside 0.46.  adjacency.build numpy to numpy, the territory call included: 8.0 / 5.7 ms at 4 px,
// 3.3 / 3.1 ms at 32 px.  The variants in two alternating rounds in one process, all bitwise equal to the shipped call:
//   LDS tile table / every site pair straight into the call's table (-DNUHTC_ADJ_PER_PAIR), ms: 2.50 / 2.68 uniform and 2.14 / 2.30
//              clustered at 4 px, 1.21 / 1.21 and 1.07 / 1.07 at 32 px -- the tile table pays where a border runs through many sites of a tile
//              and costs nothing where it does not: kept.
//   rank / one thread per row sorting its segment by insertion (-DNUHTC_ADJ_ROW_SORT), ms: 2.50 / 2.51 and 2.14 / 2.16 at 4 px,
//              1.21 / 1.22 and 1.07 / 1.08 at 32 px -- no difference beyond the spread at any measured shape, where no row has more
//              than 19 neighbours.  The rank is kept for the rows these shapes do not have: it is one thread per EDGE with work linear in
//              the segment, where the sort is one thread per ROW with quadratic work; a long row was NOT timed.
//   one counter for the records of every workgroup / 256 spread counters, one atomic per workgroup instead of one per wave: the count
//              stage 11.2 / 0.48 ms uniform and 5.3 / 0.36 ms clustered at 4 px (1.3 M adds to one address); the first form is gone.
#include <climits>
#include <cstring>
#include <vector>

#include "cellsites.h"

namespace {

constexpr int ADJ_NT = SITE_NT;                         // 256 sites, one thread each
constexpr int ADJ_COUNTERS = 256;                       // words the workgroups spread their record counts over; the host sums them
constexpr int ADJ_COUNTER_STRIDE = 16;                  // in 64-bit words: 128 B apart

struct AdjArgs {
  const int32_t* owner;               // [H][W]
  int W, H, n, tiles_x;
  long long cap;                      // edge_cap
  unsigned long long slots;           // of the call's table: a power of two, at least 2 M
  unsigned long long* tkey;           // [slots] ADJ_NO_KEY or adj_key
  unsigned* tcnt;                     // [slots] the site pairs of the key
  int* up;                            // [fchunk * CB_CHUNK] by row: the edges whose smaller row it is; zero past n
  int* start;                         // [fchunk * CB_CHUNK] by row: the edges in front of its segment
  int* fill;                          // [n] the places of the segment the gather has handed out
  unsigned long long* records;        // [ADJ_COUNTERS * ADJ_COUNTER_STRIDE] M, spread over ADJ_COUNTERS words
  int* bad;                           // [1] != 0: an owner outside -1 .. n - 1
  int* s_hi;                          // [min(M, cap)] the larger row of every edge, segment by segment, arrival order inside
  int* s_cnt;                         // [min(M, cap)] its shared
  int32_t* edges; int32_t* shared; int32_t* degree;
};

// the sum over the workgroup of v, 0 .. 2 at every thread (two barriers that count; every thread of the workgroup must arrive)
__device__ __forceinline__ int adj_block_sum(int v) { return __syncthreads_count(v >= 1) + __syncthreads_count(v == 2); }

// where a workgroup adds its records: one of ADJ_COUNTERS words, each on a cache line of its own.  (One word for every wave of every workgroup
// was measured first: with 1.3 M adds to one address the count stage took 11.2 ms at 81.6 M sites, and 0.48 ms in this form.)
__device__ __forceinline__ unsigned long long* adj_counter(const AdjArgs& a) { return a.records + (size_t)(blockIdx.x & (ADJ_COUNTERS - 1)) * ADJ_COUNTER_STRIDE; }

// the edges of the call, once the scan has run (n >= 1)
__device__ __forceinline__ long long adj_edges(const AdjArgs& a) { return (long long)a.start[a.n - 1] + a.up[a.n - 1]; }

// a key into the tile's table (at most half full: the probe meets the key or an empty slot) -> 1 when the key is new to the tile
template <bool COUNTED>
__device__ __forceinline__ int adj_tile_insert(unsigned long long* keys, unsigned* cnt, unsigned long long key) {
  unsigned s = (unsigned)adj_slot_of(key, ADJ_TILE_SLOTS);
  for (int t = 0; t < ADJ_TILE_SLOTS; ++t, s = (s + 1) & (ADJ_TILE_SLOTS - 1)) {
    const unsigned long long prev = atomicCAS(&keys[s], ADJ_NO_KEY, key);
    if (prev != ADJ_NO_KEY && prev != key) continue;
    if (COUNTED) atomicAdd(&cnt[s], 1u);
    return prev == ADJ_NO_KEY;
  }
  return 0;                                              // cannot happen: 512 keys at most in 1024 slots
}

// `pairs` site pairs of one edge into the call's table (at most half full).  A slot goes from empty to a key once and keeps it, so the
// plain load in front of the compare-and-swap can only err towards "empty", which the swap then settles.
__device__ __forceinline__ void adj_table_insert(const AdjArgs& a, unsigned long long key, unsigned pairs) {
  unsigned long long g = adj_slot_of(key, a.slots);
  for (unsigned long long t = 0; t < a.slots; ++t, g = (g + 1) & (a.slots - 1)) {
    unsigned long long prev = a.tkey[g];
    if (prev != key) {
      if (prev != ADJ_NO_KEY) continue;
      prev = atomicCAS(&a.tkey[g], ADJ_NO_KEY, key);
      if (prev != ADJ_NO_KEY && prev != key) continue;
    }
    if (prev == ADJ_NO_KEY) {                            // the first insert of the edge
      const int i = adj_key_lo(key), j = adj_key_hi(key);
      atomicAdd(&a.up[i], 1);
      atomicAdd(&a.degree[i], 1);
      atomicAdd(&a.degree[j], 1);
    }
    atomicAdd(&a.tcnt[g], pairs);
    return;
  }
}

// INSERT false: the owner check and the records of the tile.  INSERT true: the tile's keys with their counts into the call's table.
template <bool INSERT>
__global__ __launch_bounds__(ADJ_NT) void adj_tile_kernel(AdjArgs a) {
#ifndef NUHTC_ADJ_PER_PAIR
  __shared__ unsigned long long keys[ADJ_TILE_SLOTS];
  __shared__ unsigned cnt[INSERT ? ADJ_TILE_SLOTS : 1];
#endif
  const int tid = threadIdx.x, W = a.W, H = a.H, n = a.n;
  int u, v;
  site_uv(blockIdx.x, a.tiles_x, tid, &u, &v);
  const bool in = u < W && v < H;
  int me = -1, right = -1, lower = -1;                   // a pair that does not exist: (-1, -1), no edge
  if (in) {
    const size_t at = (size_t)v * W + u;                 // < 2^28
    const int pairs = adj_site_pairs(u, v, W, H);
    me = a.owner[at];
    right = pairs & 1 ? a.owner[at + 1] : me;
    lower = pairs & 2 ? a.owner[at + W] : me;
    if (!INSERT && !adj_owner_ok(me, n)) *a.bad = 1;     // every site of the window is some thread's own
  }
  const bool e_right = adj_is_edge(me, right, n), e_lower = adj_is_edge(me, lower, n);
#ifdef NUHTC_ADJ_PER_PAIR                                 // dev probe: every site pair that is an edge is a record of its own, no LDS table
  if (INSERT) {
    if (e_right) adj_table_insert(a, adj_key(me, right), 1u);
    if (e_lower) adj_table_insert(a, adj_key(me, lower), 1u);
  } else {
    const int fresh = adj_block_sum((int)e_right + (int)e_lower);
    if (tid == 0 && fresh) atomicAdd(adj_counter(a), (unsigned long long)fresh);
  }
#else
  if (!__syncthreads_or(e_right || e_lower)) return;     // a tile inside one territory, or nobody's: no key (uniform)
  for (int i = tid; i < ADJ_TILE_SLOTS; i += ADJ_NT) { keys[i] = ADJ_NO_KEY; if (INSERT) cnt[i] = 0; }
  __syncthreads();
  int fresh = 0;
  if (e_right) fresh += adj_tile_insert<INSERT>(keys, cnt, adj_key(me, right));
  if (e_lower) fresh += adj_tile_insert<INSERT>(keys, cnt, adj_key(me, lower));
  if (INSERT) {
    __syncthreads();
    for (int i = tid; i < ADJ_TILE_SLOTS; i += ADJ_NT)
      if (keys[i] != ADJ_NO_KEY) adj_table_insert(a, keys[i], cnt[i]);
  } else {
    fresh = adj_block_sum(fresh);
    if (tid == 0 && fresh) atomicAdd(adj_counter(a), (unsigned long long)fresh);
  }
#endif
}

__global__ __launch_bounds__(ADJ_NT) void adj_gather_kernel(AdjArgs a) {
  const unsigned long long g = (unsigned long long)blockIdx.x * ADJ_NT + threadIdx.x;
  if (g >= a.slots || adj_edges(a) > a.cap) return;
  const unsigned long long key = a.tkey[g];
  if (key == ADJ_NO_KEY) return;
  const int i = adj_key_lo(key);
  const long long p = (long long)a.start[i] + atomicAdd(&a.fill[i], 1);
  if (p >= a.cap) return;                                // cannot happen (p < m <= cap): no index leaves the arrays
  a.edges[2 * p] = i;
  a.s_hi[p] = adj_key_hi(key);
  a.s_cnt[p] = (int)a.tcnt[g];
}

__global__ __launch_bounds__(ADJ_NT) void adj_place_kernel(AdjArgs a) {
  const long long p = (long long)blockIdx.x * ADJ_NT + threadIdx.x, m = adj_edges(a);
  if (m > a.cap || p >= m) return;
  const int lo = a.edges[2 * p], hi = a.s_hi[p];
  if ((unsigned)lo >= (unsigned)a.n) return;             // cannot happen (the gather filled every segment): no index leaves the tables
  const long long j0 = a.start[lo];
  const long long at = cell_rank_in_segment(a.s_hi, j0, j0 + a.up[lo], hi);
  a.edges[2 * at + 1] = hi;                              // the even entries of the segment already hold lo, all the same
  a.shared[at] = a.s_cnt[p];
}

#ifdef NUHTC_ADJ_ROW_SORT
// dev probe (-DNUHTC_ADJ_ROW_SORT), the plain alternative to the rank: one thread per ROW sorts its segment by insertion, then writes it
__global__ __launch_bounds__(ADJ_NT) void adj_rowsort_kernel(AdjArgs a) {
  const int i = blockIdx.x * ADJ_NT + threadIdx.x;
  if (i >= a.n || adj_edges(a) > a.cap) return;
  const long long j0 = a.start[i], j1 = j0 + a.up[i];
  for (long long j = j0 + 1; j < j1; ++j) {
    const int hi = a.s_hi[j], c = a.s_cnt[j];
    long long k = j;
    for (; k > j0 && a.s_hi[k - 1] > hi; --k) { a.s_hi[k] = a.s_hi[k - 1]; a.s_cnt[k] = a.s_cnt[k - 1]; }
    a.s_hi[k] = hi; a.s_cnt[k] = c;
  }
  for (long long j = j0; j < j1; ++j) { a.edges[2 * j + 1] = a.s_hi[j]; a.shared[j] = a.s_cnt[j]; }
}
#endif

}  // namespace

extern "C" int nuhtc_territory_adjacency(int device, const int32_t* owner, int W, int H, int64_t n, int64_t edge_cap, int32_t* edges,
                                         int32_t* edge_shared, int32_t* degree, int64_t* m, void* stream) {
  if (!adj_call_ok(W, H, n, edge_cap) || !owner || !m || (n > 0 && !degree) || (edge_cap > 0 && (!edges || !edge_shared))) return NUHTC_E_INVALID;
  if (hipSetDevice(device) != hipSuccess) return NUHTC_E_HIP;
  hipStream_t s = (hipStream_t)stream;
  AdjArgs a;
  memset(&a, 0, sizeof(a));
  a.owner = owner; a.W = W; a.H = H; a.n = (int)n; a.cap = edge_cap;
  a.tiles_x = (W + SITE_TILE - 1) / SITE_TILE;
  a.edges = edges; a.shared = edge_shared; a.degree = degree;
  const unsigned tiles = site_tiles(W, H);
  DevScratch tmp;      // every temporary of the call, freed on the way out
  constexpr size_t counter_words = (size_t)ADJ_COUNTERS * ADJ_COUNTER_STRIDE;
  a.records = tmp.alloc<unsigned long long>(counter_words * sizeof(unsigned long long)); a.bad = tmp.alloc<int>(sizeof(int));
  if (!tmp.ok()) return NUHTC_E_HIP;
  if (hipMemsetAsync(a.records, 0, counter_words * sizeof(unsigned long long), s) != hipSuccess || hipMemsetAsync(a.bad, 0, sizeof(int), s) != hipSuccess) return NUHTC_E_HIP;
  {
    ProfScope ps("cell_adjacency_count", 0, 0, s);
    hipLaunchKernelGGL(adj_tile_kernel<false>, dim3(tiles), dim3(ADJ_NT), 0, s, a);
  }
  std::vector<unsigned long long> h_counters(counter_words, 0);
  int h_bad = 0;
  if (!launched() || hipMemcpyAsync(h_counters.data(), a.records, counter_words * sizeof(unsigned long long), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipMemcpyAsync(&h_bad, a.bad, sizeof(h_bad), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
    return NUHTC_E_HIP;
  if (h_bad) return NUHTC_E_INVALID;                     // an owner outside -1 .. n - 1: every output untouched
  if (n == 0) { *m = 0; return 0; }                      // every owner is -1
  int64_t M = 0;                                         // <= 2^29
  for (int c = 0; c < ADJ_COUNTERS; ++c) M += (int64_t)h_counters[(size_t)c * ADJ_COUNTER_STRIDE];
  if (M == 0) {
    if (hipMemsetAsync(degree, 0, (size_t)n * sizeof(int32_t), s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return NUHTC_E_HIP;
    *m = 0;
    return 0;
  }
  const int fchunk = (int)((n + CB_CHUNK - 1) / CB_CHUNK);                 // scan chunks of the n counts: at most 1024
  const size_t scan_bytes = (size_t)fchunk * CB_CHUNK * sizeof(int);
  const size_t rows = (size_t)std::min<int64_t>(M, edge_cap);               // m <= M, and the place stage runs with m <= edge_cap only
  a.slots = (unsigned long long)adj_table_slots(M);
  a.up = tmp.alloc<int>(scan_bytes); a.start = tmp.alloc<int>(scan_bytes);
  const ExScan scan{a.up, a.start, tmp.alloc<int>(1024 * sizeof(int))};
  a.fill = tmp.alloc<int>((size_t)n * sizeof(int));
  a.tkey = tmp.alloc<unsigned long long>((size_t)a.slots * sizeof(unsigned long long)); a.tcnt = tmp.alloc<unsigned>((size_t)a.slots * sizeof(unsigned));
  if (rows) { a.s_hi = tmp.alloc<int>(rows * sizeof(int)); a.s_cnt = tmp.alloc<int>(rows * sizeof(int)); }
  if (!tmp.ok()) return NUHTC_E_HIP;                     // before any output is written
  if (hipMemsetAsync(a.up, 0, scan_bytes, s) != hipSuccess || hipMemsetAsync(a.fill, 0, (size_t)n * sizeof(int), s) != hipSuccess ||
      hipMemsetAsync(a.tkey, 0xff, (size_t)a.slots * sizeof(unsigned long long), s) != hipSuccess ||
      hipMemsetAsync(a.tcnt, 0, (size_t)a.slots * sizeof(unsigned), s) != hipSuccess || hipMemsetAsync(degree, 0, (size_t)n * sizeof(int32_t), s) != hipSuccess)
    return NUHTC_E_HIP;
  {
    ProfScope ps("cell_adjacency_insert", 0, 0, s);
    hipLaunchKernelGGL(adj_tile_kernel<true>, dim3(tiles), dim3(ADJ_NT), 0, s, a);
    exscan_launch(scan, fchunk, s);
  }
  if (rows) {
    ProfScope ps("cell_adjacency_place", 0, 0, s);
    hipLaunchKernelGGL(adj_gather_kernel, dim3((unsigned)((a.slots + ADJ_NT - 1) / ADJ_NT)), dim3(ADJ_NT), 0, s, a);       // at most 2^22 workgroups
#ifdef NUHTC_ADJ_ROW_SORT
    hipLaunchKernelGGL(adj_rowsort_kernel, dim3((unsigned)((n + ADJ_NT - 1) / ADJ_NT)), dim3(ADJ_NT), 0, s, a);
#else
    hipLaunchKernelGGL(adj_place_kernel, dim3((unsigned)((rows + ADJ_NT - 1) / ADJ_NT)), dim3(ADJ_NT), 0, s, a);
#endif
  }
  int h_last[2] = {0, 0};                                // start[n - 1], up[n - 1]
  if (!launched() || hipMemcpyAsync(&h_last[0], a.start + (n - 1), sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipMemcpyAsync(&h_last[1], a.up + (n - 1), sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
    return NUHTC_E_HIP;
  *m = (int64_t)h_last[0] + h_last[1];
  return 0;
}
