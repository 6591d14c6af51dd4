// What the analyses of points against polygon EDGES share on the device (gfx950) -- the region census (cellregion.hip) and the margin
// bands (cellmargin.hip): the edges binned by the slab (row of the points' grid, cellbin.h with one key per cell) they meet, so that a
// workgroup of point records can stage its slab's edges through LDS in edge order.  One copy of the five kernels and of the table
// carving; the two files differ in ONE thing, the slabs an edge gets a record in (rg_range: region_slab_range, or margin_slab_range with
// the y-range grown by the largest threshold), and in their sweep over the records.
//
// A is the file's argument block.  It holds, under these names: b (CellBin), edges, edge_region, E, G, have_grid, slot_cap, total,
// slab_count, slab_start, emitted, slots -- see CellRegionArgs -- and the file declares, in front of the launches,
//   __device__ bool rg_range(const A&, int4 edge, int* s0, int* s1)    the slabs s0 .. s1 the edge has a record in, false for none.
//
//   rg_check_kernel  every edge against the limits (a vertex outside +-2^27, a region outside 0 .. G - 1 or below the one in front of it
//                    raise the binning's flag) and the number of slabs it has a record in, summed in 64 bits: M, the (edge, slab) records
//                    the call needs.  Every later kernel first compares M with the caller's slot_cap (rg_go): no int32 sees M, or a sum
//                    of slab counts, before that.
//   rg_count_kernel  the edges per slab (atomics), then exscan_launch of cellbin.h over the slabs.
//   rg_emit_kernel   the records (edge, slab) into their slab's segment, in atomic arrival order.
//   rg_place_kernel  every record to its final place: the segment's start plus the NUMBER of records of the segment with a smaller edge
//                    index.  No sort and nothing left of the arrival order: a segment is in edge order, hence grouped by region, ascending.
// No kernel waits on another workgroup; every loop runs over a range of a table.
#pragma once
#include "cellbin.h"

namespace {

// may this call write?  No edge or point was refused, and the records fit the caller's cap.  Uniform over the grid.
template <class A>
__device__ __forceinline__ bool rg_go(const A& a) { return *a.b.flag == 0 && *a.total <= a.slot_cap; }

template <class A>
__global__ __launch_bounds__(256) void rg_check_kernel(A a) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  int nslab = 0;
  if (e < a.E) {
    const int4 ed = a.edges[e];
    if (!region_edge_ok(ed.x, ed.y, ed.z, ed.w, a.edge_region[e], e ? a.edge_region[e - 1] : 0, a.G)) {
      *a.b.flag = 1;
    } else if (a.have_grid) {
      int s0, s1;
      if (rg_range(a, ed, &s0, &s1)) nslab = s1 - s0 + 1;        // at most 2^22 rows: 64 lanes of them stay below 2^31
    }
  }
  const int sum = wave_sum(nslab);
  if ((threadIdx.x & 63) == 0 && sum) atomicAdd(a.total, (unsigned long long)sum);
}

template <class A>
__global__ __launch_bounds__(256) void rg_count_kernel(A a) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= a.E || !rg_go(a)) return;
  int s0, s1;
  if (!rg_range(a, a.edges[e], &s0, &s1)) return;
  for (int s = s0; s <= s1; ++s) atomicAdd(&a.slab_count[s], 1);
}

template <class A>
__global__ __launch_bounds__(256) void rg_emit_kernel(A a) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= a.E || !rg_go(a)) return;
  int s0, s1;
  if (!rg_range(a, a.edges[e], &s0, &s1)) return;
  for (int s = s0; s <= s1; ++s) a.emitted[a.slab_start[s] + atomicSub(&a.slab_count[s], 1) - 1] = make_int2(e, s);
}

template <class A>
__global__ __launch_bounds__(256) void rg_place_kernel(A a) {
  const unsigned long long j = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
  if (!rg_go(a) || j >= *a.total) return;
  const int2 me = a.emitted[j];
  const int k0 = a.slab_start[me.y], k1 = a.slab_start[me.y + 1];
  int rank = 0;
  for (int k = k0; k < k1; ++k) rank += a.emitted[k].x < me.x;     // an edge is in a segment once: the ranks are a permutation
  a.slots[k0 + rank] = me.x;
}

// The points' grid and the tables of the edge records for one call, on s.  With n > 0 the points are set up for binning (cellbin_setup,
// reach slab, one key per cell); with n == 0 only the flag exists.  Then ONE allocation for the tables of this header, carved in 256-byte
// steps: the slab counts with M behind them (one memset), the slab starts, the scan's chunk bases and the two record tables.
// -> false when an allocation or a memset failed.  *nchunk, *schunk: the scan chunks of the cells and of the slabs.
template <class A>
inline bool edge_tables(A& a, const int32_t* points, const int32_t* labels, int64_t n, int x_min, int y_min, int x_max, int y_max, int slab,
                        int64_t slot_cap, DevScratch& tmp, hipStream_t st, int* nchunk, int* schunk, int** chunk_base) {
  *nchunk = 0; *schunk = 1;
  if (n > 0) {
    *nchunk = cellbin_setup(a.b, points, labels, (int)n, x_min, y_min, x_max, y_max, slab, REGION_MAX_CELLS, 1, tmp, st);
    if (!*nchunk) return false;
    a.have_grid = 1;
    *schunk = (a.b.ncy + 1 + CB_CHUNK - 1) / CB_CHUNK;           // + 1: the entry behind the last slab holds the total; at most 257
  } else {
    a.b.flag = tmp.alloc<int>(sizeof(int));
    if (!tmp.ok() || hipMemsetAsync(a.b.flag, 0, sizeof(int), st) != hipSuccess) return false;
  }
  const size_t step = 256, slab_bytes = (size_t)*schunk * CB_CHUNK * sizeof(int), cap = (size_t)(slot_cap > 0 ? slot_cap : 1);
  const size_t emit_up = (cap * sizeof(int2) + step - 1) / step * step, slot_up = (cap * sizeof(int) + step - 1) / step * step;
  const size_t bytes = 2 * slab_bytes + 2 * step + 1024 * sizeof(int) + emit_up + slot_up;
  char* base = tmp.alloc<char>(bytes);
  if (!tmp.ok()) return false;
  size_t at = 0;
  auto carve = [&](size_t b) { char* p = base + at; at += (b + step - 1) / step * step; return p; };
  a.slab_count = reinterpret_cast<int*>(carve(slab_bytes));
  a.total = reinterpret_cast<unsigned long long*>(carve(sizeof(unsigned long long)));
  a.slab_start = reinterpret_cast<int*>(carve(slab_bytes));
  *chunk_base = reinterpret_cast<int*>(carve(1024 * sizeof(int)));
  a.emitted = reinterpret_cast<int2*>(carve(cap * sizeof(int2)));
  a.slots = reinterpret_cast<int*>(carve(cap * sizeof(int)));
  if (at > bytes) return false;
  return hipMemsetAsync(a.slab_count, 0, slab_bytes + step, st) == hipSuccess;
}

// the launches that bin the edges: check, and with points count, scan, emit and place
template <class A>
inline void edge_launch(const A& a, int64_t E, int64_t n, int64_t slot_cap, int schunk, int* chunk_base, hipStream_t st) {
  const unsigned eb = (unsigned)((E + 255) / 256);
  if (eb) hipLaunchKernelGGL(rg_check_kernel<A>, dim3(eb), dim3(256), 0, st, a);
  if (n > 0) {
    if (eb) hipLaunchKernelGGL(rg_count_kernel<A>, dim3(eb), dim3(256), 0, st, a);
    exscan_launch(ExScan{a.slab_count, a.slab_start, chunk_base}, schunk, st);
    if (eb) hipLaunchKernelGGL(rg_emit_kernel<A>, dim3(eb), dim3(256), 0, st, a);
    if (eb && slot_cap > 0) hipLaunchKernelGGL(rg_place_kernel<A>, dim3((unsigned)((slot_cap + 255) / 256)), dim3(256), 0, st, a);
  }
}

// the end of a call: M read back behind the binning's flag.  -> the return code; *slots = M on success
template <class A>
inline int edge_finish(const A& a, hipStream_t st, int64_t* slots) {
  unsigned long long h_total = 0;
  if (hipMemcpyAsync(&h_total, a.total, sizeof(h_total), hipMemcpyDeviceToHost, st) != hipSuccess) return NUHTC_E_HIP;
  const int rc = cellbin_finish(a.b, st);                // synchronises: h_total has arrived
  if (rc == 0) *slots = (int64_t)h_total;
  return rc;
}

}  // namespace
