// The count / scan / emit / place frame of the per-slide analyses that return an edge list in ascending (i, j) order from two sweeps of
// the cell grid (gfx950): the proximity graphs (cellprox.hip) and the alpha complex (cellalpha.hip) use all of it.  The other two edge
// lists take their segments from elsewhere -- celladjacency.hip from a hash table, cellmst.hip from the picks of its rounds -- and share
// only the last step, cell_rank_in_segment of cellgrid_host.h, which all four place kernels call.
//   count      degree cleared (el_clear_kernel); the caller's sweep counts the edges of every record into count[i], adds the degrees at
//              both ends and the two totals (m and one more: the RNG or the Gabriel edges) into `slots` pairs of 64-bit counters.
//   (the host reads the totals and the binning's flag back: edgelist_count.  m > edge_cap: the call ends here, the edge arrays untouched.)
//   scan       exscan_launch over the n counts (at most 1024 chunks: why n <= 2^24): the segment of every row.
//   emit       the caller's sweep again: i into `edges`, (j, payload) into temporaries at the record's own segment, in sweep order.
//   place      the caller's kernel, one thread per edge, around cell_rank_in_segment.
// Each analysis keeps its sweep kernels, its payload arrays, the body of its place kernel and its argument check; the launches come in
// as lambdas, the profile tags as literals.
#pragma once
#include "cellbin.h"

namespace {

constexpr int EL_NT = 256;
constexpr int EL_MAX_SLOTS = 64;

struct EdgeList {
  int n;
  long long m;                        // the edges, known on the host after the count stage
  int* count;                         // [fchunk * CB_CHUNK] by row: the edges whose smaller row it is; zero past n
  int* start;                         // [fchunk * CB_CHUNK] by row: the edges in front of its segment
  unsigned long long* totals;         // [slots][2] m and the second total, summed on the host
  int* s_hi;                          // [m] the larger row of every edge, segment by segment, sweep order inside
  int32_t* edges; int32_t* degree;
};

// the profile tags of the five stages (string literals), and the host side of a call: the scan's tables and the number of counter pairs
struct EdgeListTags { const char *bin, *count, *scan, *emit, *place; };
struct EdgeListRun { EdgeListTags tags; ExScan scan; int fchunk, slots; };

__global__ __launch_bounds__(EL_NT) void el_clear_kernel(const int* flag, int32_t* degree, int n) {
  if (*flag) return;                                     // the binning met a point outside the box: nothing is written
  const int i = blockIdx.x * EL_NT + threadIdx.x;
  if (i < 2 * n) degree[i] = 0;                          // 2 n <= 2^25
}

// Set-up: count / start / the scan's chunk table / `slots` pairs of counters from `tmp`, the counts and the counters cleared on s.
// e.n set by the caller.  false when an allocation or a memset failed.
inline bool edgelist_setup(EdgeList& e, EdgeListRun& h, const EdgeListTags& tags, int slots, DevScratch& tmp, hipStream_t s) {
  h.tags = tags;
  h.fchunk = (e.n + CB_CHUNK - 1) / CB_CHUNK;            // scan chunks of the n counts: at most 1024
  h.slots = slots;
  const size_t scan_bytes = (size_t)h.fchunk * CB_CHUNK * sizeof(int), totals_bytes = 2 * (size_t)slots * sizeof(unsigned long long);
  e.count = tmp.alloc<int>(scan_bytes); e.start = tmp.alloc<int>(scan_bytes);
  h.scan = ExScan{e.count, e.start, tmp.alloc<int>(1024 * sizeof(int))};
  e.totals = tmp.alloc<unsigned long long>(totals_bytes);
  return slots <= EL_MAX_SLOTS && tmp.ok() && hipMemsetAsync(e.count, 0, scan_bytes, s) == hipSuccess &&
         hipMemsetAsync(e.totals, 0, totals_bytes, s) == hipSuccess;
}

// The first half: the binning and the count stage (the clear, then the caller's launch) under their tags, then the read-back: the
// totals copied back through cellbin_finish (the flag, and the stream synchronised) and summed over the slots -> 0 with e.m and *second
// set, NUHTC_E_INVALID when a point lay outside the box, NUHTC_E_HIP.
template <typename Count>
inline int edgelist_count(const CellBin& b, int nchunk, EdgeList& e, const EdgeListRun& h, Count&& count, long long* second, hipStream_t s) {
  {
    ProfScope ps(h.tags.bin, 0, 0, s);
    cellbin_launch(b, nchunk, s);
  }
  {
    ProfScope ps(h.tags.count, 0, 0, s);
    hipLaunchKernelGGL(el_clear_kernel, dim3((unsigned)((2 * (long long)e.n + EL_NT - 1) / EL_NT)), dim3(EL_NT), 0, s, b.flag, e.degree, e.n);
    count();
  }
  unsigned long long h_slots[2 * EL_MAX_SLOTS], h_tot[2] = {0, 0};
  if (hipMemcpyAsync(h_slots, e.totals, 2 * (size_t)h.slots * sizeof(unsigned long long), hipMemcpyDeviceToHost, s) != hipSuccess) return NUHTC_E_HIP;
  const int rc = cellbin_finish(b, s);                   // the flag, and the stream synchronised: the totals are here
  if (rc) return rc;
  for (int k = 0; k < h.slots; ++k) { h_tot[0] += h_slots[2 * k]; h_tot[1] += h_slots[2 * k + 1]; }
  e.m = (long long)h_tot[0];
  *second = (long long)h_tot[1];
  return 0;
}

// The second half, for 0 < e.m <= edge_cap (so e.m <= INT_MAX: the int32 scan is safe) and s_hi and the payloads allocated: scan, emit
// and place under their tags, the stream synchronised -> 0 or NUHTC_E_HIP.
template <typename Emit, typename Place>
inline int edgelist_finish(const EdgeListRun& h, Emit&& emit, Place&& place, hipStream_t s) {
  {
    ProfScope ps(h.tags.scan, 0, 0, s);
    exscan_launch(h.scan, h.fchunk, s);
  }
  {
    ProfScope ps(h.tags.emit, 0, 0, s);
    emit();
  }
  {
    ProfScope ps(h.tags.place, 0, 0, s);
    place();
  }
  return launched() && hipStreamSynchronize(s) == hipSuccess ? 0 : NUHTC_E_HIP;
}

}  // namespace
