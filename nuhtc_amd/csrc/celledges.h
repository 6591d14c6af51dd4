// What the analyses of points against polygon EDGES share (gfx950) -- the region census (cellregion.hip) and the margin bands
// (cellmargin.hip): the edges binned by the slab (row of the points' grid, cellbin.h with one key per cell) they meet, the walk of a
// workgroup of point records through its slabs' edges, and the frame of the entry point.  One copy of each; a file keeps its own
// fields, what a lane does per edge and at the end of a region, its zero kernel and its entry point's own checks.
//
// EdgeSlabs is the part of the argument block both files have; their blocks derive from it.  `grow` is the ONE thing the binning of the
// two differs in: the R by which an edge's y-range is grown before its slabs are taken (edge_slab_range of cellgrid_host.h), 0 for the
// census, the largest threshold for the bands.
//
//   rg_check_kernel  every edge against the limits (a vertex outside +-2^27, a region outside 0 .. G - 1 or below the one in front of it
//                    raise the binning's flag) and the number of slabs it has a record in, summed in 64 bits: M, the (edge, slab) records
//                    the call needs.  Every later kernel first compares M with the caller's slot_cap (rg_go): no int32 sees M, or a sum
//                    of slab counts, before that.
//   rg_count_kernel  the edges per slab (atomics), then exscan_launch of cellbin.h over the slabs.
//   rg_emit_kernel   the records (edge, slab) into their slab's segment, in atomic arrival order.
//   rg_place_kernel  every record to its final place: the segment's start plus the NUMBER of records of the segment with a smaller edge
//                    index.  No sort and nothing left of the arrival order: a segment is in edge order, hence grouped by region, ascending.
//   rg_walk          the body of the sweep kernels (rg_cross_kernel, mg_sweep_kernel): one workgroup per 256 consecutive point records,
//                    see there.
// No kernel waits on another workgroup; every loop runs over a range of a table.
//
// The host frame, in the manner of celledgelist.h: edge_front (the checks of the shared arguments, the device, the shared fields, the
// tables) and edge_run (the binning of the points and of the edges and the sweep under their tags, M read back).  The zero launch and
// the sweep launch come in as lambdas, the profile tags as literals.
#pragma once
#include <climits>

#include "cellbin.h"

namespace {

struct EdgeSlabs {
  CellBin b;                          // the points, the grid and the records in cell order (cellbin.h, one key per cell)
  const int4* edges;                  // [E] (ax, ay, bx, by) half pixels
  const int32_t* edge_region;         // [E] non-decreasing
  int E, G, C;
  int have_grid;                      // 0 with n == 0: the edges are checked, no slab is counted
  int grow;                           // R: an edge has a record in every slab its y-range grown by R meets
  unsigned long long slot_cap;        // the (edge, slab) records the caller left room for
  unsigned long long* total;          // M: the records the call needs
  int* slab_count;                    // [schunk * CB_CHUNK] per slab, zero past them; counted up, and down again by the emit
  int* slab_start;                    // [schunk * CB_CHUNK] entry k = records in front of slab k (entry ncy: all of them)
  int2* emitted;                      // [slot_cap] (edge, slab) in arrival order inside a slab's segment
  int* slots;                         // [slot_cap] the edge of every record, slab by slab, in edge order
};

// may this call write?  No edge or point was refused, and the records fit the caller's cap.  Uniform over the grid.
__device__ __forceinline__ bool rg_go(const EdgeSlabs& a) { return *a.b.flag == 0 && *a.total <= a.slot_cap; }

// the slabs s0 .. s1 the edge has a record in, false for none
__device__ __forceinline__ bool rg_slabs_of(const EdgeSlabs& a, const int4 e, int* s0, int* s1) {
  return edge_slab_range(e.x, e.y, e.z, e.w, a.grow, a.b.x_min, a.b.y_min, a.b.y_max, a.b.side, s0, s1);
}

__global__ __launch_bounds__(256) void rg_check_kernel(EdgeSlabs a) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  int nslab = 0;
  if (e < a.E) {
    const int4 ed = a.edges[e];
    if (!region_edge_ok(ed.x, ed.y, ed.z, ed.w, a.edge_region[e], e ? a.edge_region[e - 1] : 0, a.G)) {
      *a.b.flag = 1;
    } else if (a.have_grid) {
      int s0, s1;
      if (rg_slabs_of(a, ed, &s0, &s1)) nslab = s1 - s0 + 1;     // at most 2^22 rows: 64 lanes of them stay below 2^31
    }
  }
  const int sum = wave_sum(nslab);
  if ((threadIdx.x & 63) == 0 && sum) atomicAdd(a.total, (unsigned long long)sum);
}

__global__ __launch_bounds__(256) void rg_count_kernel(EdgeSlabs a) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= a.E || !rg_go(a)) return;
  int s0, s1;
  if (!rg_slabs_of(a, a.edges[e], &s0, &s1)) return;
  for (int s = s0; s <= s1; ++s) atomicAdd(&a.slab_count[s], 1);
}

__global__ __launch_bounds__(256) void rg_emit_kernel(EdgeSlabs a) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= a.E || !rg_go(a)) return;
  int s0, s1;
  if (!rg_slabs_of(a, a.edges[e], &s0, &s1)) return;
  for (int s = s0; s <= s1; ++s) a.emitted[a.slab_start[s] + atomicSub(&a.slab_count[s], 1) - 1] = make_int2(e, s);
}

__global__ __launch_bounds__(256) void rg_place_kernel(EdgeSlabs a) {
  const unsigned long long j = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
  if (!rg_go(a) || j >= *a.total) return;
  const int2 me = a.emitted[j];
  const int k0 = a.slab_start[me.y], k1 = a.slab_start[me.y + 1];
  int rank = 0;
  for (int k = k0; k < k1; ++k) rank += a.emitted[k].x < me.x;     // an edge is in a segment once: the ranks are a permutation
  a.slots[k0 + rank] = me.x;
}

// The sweep of one workgroup of REGION_STAGE consecutive point records, the grid being ceil(n / REGION_STAGE) workgroups of that many
// threads and rg_go(a) tested by the kernel.  For each slab that holds some of the records (they are in row order, so these are few)
// the slab's edge records go through LDS REGION_STAGE at a time -- coordinates and region gathered once per workgroup -- and every
// thread of that slab takes each staged edge by a broadcast LDS read.  The edge sequence, and with it the region changes, are the same
// for every thread of the workgroup.  What a file does with it is `w`, whose members are inlined here:
//   w.begin(tid)              once, in front of the first barrier: what the file puts into LDS of its own for the whole walk
//   w.stage(tid, ed)          between the two barriers of a pass: thread tid has loaded edge ed and stages what else the file keeps of it
//   w.reset()                 in front of a region's run of edges
//   w.edge(k, ed, me)         staged edge k = ed against the lane's record me; only lanes whose record lies in the slab
//   w.flush(cur, mine, cls)   the end of region cur's run (cur < 0: there was none).  EVERY thread of the workgroup calls it at once, so
//                             ballots inside see whole waves; mine: the lane's record lies in the slab; cls: its class, -1 for none
// -> the lane's record (x, y, label, index), index -1 for a lane past the last record.
template <class Walk>
__device__ __forceinline__ int4 rg_walk(const EdgeSlabs& a, Walk& w) {
  __shared__ int4 st_edge[REGION_STAGE];
  __shared__ int st_region[REGION_STAGE];
  __shared__ int next_row;
  const CellBin& g = a.b;
  const int tid = threadIdx.x, j = blockIdx.x * REGION_STAGE + tid;
  const bool have = j < g.n;
  const int4 me = have ? g.recs[j] : make_int4(0, 0, -1, -1);
  const int my_row = have ? (me.y - g.y_min) / g.side : INT_MAX;
  const int cls = have && (unsigned)me.z < (unsigned)a.C ? me.z : -1;
  w.begin(tid);
  if (tid == 0) next_row = my_row;                       // thread 0 has a record: the grid is ceil(n / 256) workgroups
  __syncthreads();
  int row = next_row;
  while (row != INT_MAX) {                               // the slabs that hold records of this workgroup, ascending
    const bool mine = my_row == row;
    const int k0 = a.slab_start[row], k1 = a.slab_start[row + 1];
    int cur = -1;
    w.reset();
    for (int base = k0; base < k1; base += REGION_STAGE) {
      __syncthreads();                                   // the chunk before this one has been read by everyone
      if (base + tid < k1) {
        const int e = a.slots[base + tid];
        const int4 ed = a.edges[e];
        st_edge[tid] = ed;
        w.stage(tid, ed);
        st_region[tid] = a.edge_region[e];
      }
      __syncthreads();
      const int m = min(REGION_STAGE, k1 - base);
      for (int k = 0; k < m; ++k) {
        const int r = __builtin_amdgcn_readfirstlane(st_region[k]);
        if (r != cur) {                                  // the same for every thread of the workgroup
          w.flush(cur, mine, cls);
          cur = r;
          w.reset();
        }
        if (mine) w.edge(k, st_edge[k], me);
      }
    }
    w.flush(cur, mine, cls);
    __syncthreads();                                     // everyone has read next_row
    if (tid == 0) next_row = INT_MAX;
    __syncthreads();
    if (have && my_row > row) atomicMin(&next_row, my_row);
    __syncthreads();
    row = next_row;
  }
  return me;
}

// the profile tags of the three stages (string literals), and the host side of one call
struct EdgeTags { const char *bin, *edges, *sweep; };
struct EdgeCall {
  DevScratch tmp;                     // every temporary of the call, freed on the way out
  hipStream_t st;
  int64_t n;
  int64_t* slots;                     // the caller's M
  int nchunk, schunk, *chunk_base;    // the scan chunks of the cells and of the slabs, and the slab scan's chunk table
};

// The points' grid and the tables of the edge records for one call, on h.st.  With n > 0 the points are set up for binning
// (cellbin_setup, reach slab, one key per cell); with n == 0 only the flag exists.  Then ONE allocation for the tables of this header,
// carved in 256-byte steps: the slab counts with M behind them (one memset), the slab starts, the scan's chunk bases and the two record
// tables.  -> false when an allocation or a memset failed.
inline bool edge_tables(EdgeSlabs& a, EdgeCall& h, const int32_t* points, const int32_t* labels, int x_min, int y_min, int x_max, int y_max, int slab) {
  h.nchunk = 0; h.schunk = 1;
  if (h.n > 0) {
    h.nchunk = cellbin_setup(a.b, points, labels, (int)h.n, x_min, y_min, x_max, y_max, slab, REGION_MAX_CELLS, 1, h.tmp, h.st);
    if (!h.nchunk) return false;
    a.have_grid = 1;
    h.schunk = (a.b.ncy + 1 + CB_CHUNK - 1) / CB_CHUNK;          // + 1: the entry behind the last slab holds the total; at most 257
  } else {
    a.b.flag = h.tmp.alloc<int>(sizeof(int));
    if (!h.tmp.ok() || hipMemsetAsync(a.b.flag, 0, sizeof(int), h.st) != hipSuccess) return false;
  }
  const size_t step = 256, slab_bytes = (size_t)h.schunk * CB_CHUNK * sizeof(int), cap = (size_t)(a.slot_cap > 0 ? a.slot_cap : 1);
  const size_t emit_up = (cap * sizeof(int2) + step - 1) / step * step, slot_up = (cap * sizeof(int) + step - 1) / step * step;
  const size_t bytes = 2 * slab_bytes + 2 * step + 1024 * sizeof(int) + emit_up + slot_up;
  char* base = h.tmp.alloc<char>(bytes);
  if (!h.tmp.ok()) return false;
  size_t at = 0;
  auto carve = [&](size_t b) { char* p = base + at; at += (b + step - 1) / step * step; return p; };
  a.slab_count = reinterpret_cast<int*>(carve(slab_bytes));
  a.total = reinterpret_cast<unsigned long long*>(carve(sizeof(unsigned long long)));
  a.slab_start = reinterpret_cast<int*>(carve(slab_bytes));
  h.chunk_base = reinterpret_cast<int*>(carve(1024 * sizeof(int)));
  a.emitted = reinterpret_cast<int2*>(carve(cap * sizeof(int2)));
  a.slots = reinterpret_cast<int*>(carve(cap * sizeof(int)));
  if (at > bytes) return false;
  return hipMemsetAsync(a.slab_count, 0, slab_bytes + step, h.st) == hipSuccess;
}

// The front of an entry point, behind its own *_call_ok and output pointer checks and before anything is launched: the pointers of
// the shared arguments and the 16-byte alignment of the edges (-> NUHTC_E_INVALID), the device, the shared fields of the caller's
// zeroed block and the tables (-> NUHTC_E_HIP).  -> 0: the file fills in its own fields and calls edge_run.
inline int edge_front(EdgeSlabs& a, EdgeCall& h, int device, const int32_t* points, const int32_t* labels, int64_t n, int num_classes,
                      const int32_t* edges, const int32_t* edge_region, int64_t E, int64_t G, int grow, int slab, int64_t slot_cap, int x_min,
                      int y_min, int x_max, int y_max, int64_t* slots, void* stream) {
  if (!slots || (n > 0 && (!points || !labels)) || (E > 0 && (!edges || !edge_region))) return NUHTC_E_INVALID;
  if (reinterpret_cast<uintptr_t>(edges) & 15) return NUHTC_E_INVALID;        // an edge is one 16-byte load
  if (hipSetDevice(device) != hipSuccess) return NUHTC_E_HIP;
  h.st = (hipStream_t)stream; h.n = n; h.slots = slots;
  a.edges = reinterpret_cast<const int4*>(edges); a.edge_region = edge_region;
  a.E = (int)E; a.G = (int)G; a.C = num_classes; a.grow = grow; a.slot_cap = (unsigned long long)slot_cap;
  return edge_tables(a, h, points, labels, x_min, y_min, x_max, y_max, slab) ? 0 : NUHTC_E_HIP;
}

// The run of a call whose block is filled: the points binned, the edges binned (check, and with points count, scan, emit and place)
// and the file's sweep -- zero() with regions, sweep() with points -- each under its tag; then M read back behind the binning's flag.
// -> the return code; *h.slots = M on success
template <class Zero, class Sweep>
inline int edge_run(const EdgeSlabs& a, const EdgeCall& h, const EdgeTags& tags, Zero&& zero, Sweep&& sweep) {
  hipStream_t st = h.st;
  if (h.n > 0) {
    ProfScope ps(tags.bin, 0, 0, st);
    cellbin_launch(a.b, h.nchunk, st);
  }
  {
    ProfScope ps(tags.edges, 0, 0, st);
    const unsigned eb = (unsigned)((a.E + 255) / 256);
    if (eb) hipLaunchKernelGGL(rg_check_kernel, dim3(eb), dim3(256), 0, st, a);
    if (h.n > 0) {
      if (eb) hipLaunchKernelGGL(rg_count_kernel, dim3(eb), dim3(256), 0, st, a);
      exscan_launch(ExScan{a.slab_count, a.slab_start, h.chunk_base}, h.schunk, st);
      if (eb) hipLaunchKernelGGL(rg_emit_kernel, dim3(eb), dim3(256), 0, st, a);
      if (eb && a.slot_cap > 0) hipLaunchKernelGGL(rg_place_kernel, dim3((unsigned)((a.slot_cap + 255) / 256)), dim3(256), 0, st, a);
    }
  }
  {
    ProfScope ps(tags.sweep, 0, 0, st);
    if (a.G > 0) zero();
    if (h.n > 0) sweep();
  }
  unsigned long long h_total = 0;
  if (hipMemcpyAsync(&h_total, a.total, sizeof(h_total), hipMemcpyDeviceToHost, st) != hipSuccess) return NUHTC_E_HIP;
  const int rc = cellbin_finish(a.b, st);                // synchronises: h_total has arrived
  if (rc == 0) *h.slots = (int64_t)h_total;
  return rc;
}

}  // namespace
