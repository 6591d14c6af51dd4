// Spatial statistics of a slide (gfx950): pair-distance histograms by class pair, and the nearest nucleus of every class for every nucleus.
//
// Definition (nuhtc_amd/spatial.py holds it in full, with the int64 brute-force restatement `spatial_reference`): n points in HALF pixels
// (|p| < 2^27, n <= 2^28), one label each, C classes (1 .. 14), B bin edges e_1 < .. < e_B in half pixels (1 <= B <= 32, e_1 >= 1,
// e_B <= 16384).  The bin of an ordered pair (i, j), i != j, d2 = dx * dx + dy * dy, is the smallest t with d2 <= e_t^2 (inclusive edges;
// none beyond e_B; coincident points: bin 0).  pair_hist[a][b][t] counts the ordered pairs with label_i = a, label_j = b and bin t (not
// cumulative; a label outside 0 .. C - 1 is in no row and no column), nn_d2[i][c] is the least d2 from i to a j != i of class c within
// e_B (-1: none; for every i, whatever its label), class_n[c] the points of class c.  Integer adds only: the result does not depend on
// the arrival order of any atomic and is bitwise the same on every call.
//
// Stages, all on the caller's stream:
//   geometry   on the HOST from the caller's bounding box (cell_grid_side of cellgrid_host.h): the cell side is the smallest multiple of
//              e_B whose grid has at most 2^18 cells -- 2^18 and not the graph's 2^22, because every cell has C + 1 keys.
//   binning    cellbin.h on the key cell * (C + 1) + class (class C: a label out of range): the
//              records come out sorted by (cell, class).
//   search     one thread per record in that order, 256 per workgroup, a grid-stride loop over the blocks of 256 records.  The class loop
//              is OUTSIDE the cell loop: for each candidate class b a thread walks the (at most nine) runs of class-b records of its
//              3 x 3 cells -- nine contiguous ranges, the same or neighbouring ones across the wave, one 16-byte load per record.  That
//              differs from the shape the issue sketched (a flush at the end of every run): a thread flushes once per class instead of
//              once per (cell, class) run, nine times fewer adds into the shared table, for 18 reads of the start table per class.
//              Per pair: cell_pair_d2 of cellgrid_host.h (the box test against e_B, then d2 <= 2^29), cs_bin_of (five exact
//              integer compares against the table of e_t^2 <= 2^28 in LDS), one add to the thread's PRIVATE counter of that bin, and the
//              running minimum in a register.  The private counters are LDS, slot-major (counter t of thread tid at word t * 256 + tid):
//              no atomics and no bank conflicts.  At the end of a class the thread writes nn_d2[i][b]; then the workgroup meets at a
//              barrier and lane t < B of every wave sums counter t over the 64 columns of ITS wave (cs_rotated_column: the 32 lanes of
//              a half wave read 32 banks), breaking the sum where the query class changes, and adds each piece into the workgroup's
//              uint64 table [a][b][t] with one 64-bit LDS atomic: lanes of a wave hit B different addresses, so nothing serialises on
//              the few class pairs.  When its blocks are done the workgroup adds the non-zero entries of its table into the global
//              int64 pair_hist (64-bit vector atomics) and its class census into class_n.
//   outputs    pair_hist and class_n are zeroed by a kernel of this call AFTER the binning and only if the flag is clear, so a point
//              outside the stated box leaves every output untouched (NUHTC_E_INVALID).
//
// No 32-bit counter can overflow for any accepted input.  A private counter is cleared for every (query, class) and counts candidates of
// one query: at most n - 1 < 2^28.  The census of a workgroup counts its own queries: at most n <= 2^28.  Every sum of more than one
// thread's counts is 64-bit from the first add on: the row sums of a wave (<= 64 * 2^28), the workgroup's table and pair_hist
// (<= n^2 <= 2^56).  Record positions and the start table are int32 and n <= 2^28.  So the accepted n stays 2^28 and no early flush is
// needed.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage): cs_search_kernel takes 30 VGPRs, 78 SGPRs and no scratch; cs_zero_kernel 6 and 14;
// the binning kernels at most 31 and 26, none with scratch (profiles/cell_spatial_resources.txt).  LDS per workgroup is dynamic,
// cs_lds_bytes(C, B) = 8 C^2 B + 1024 B + 1216 bytes: 40,384 B at the tool's C = 5, B = 32 (3 workgroups = 12 waves per CU), 84,160 B at
// C = 14, B = 32 (1 workgroup).
//
// Everything that decides an index or a limit -- the grid geometry, the (cell, class) key and the pair distance (cellgrid_host.h), the bin
// lookup, the LDS carve and the rotated column (cellspatial_host.h) -- is plain C++, and tools/dev/cellspatial_host_check.cpp runs exactly those functions on the host under
// -fsanitize=address,undefined against counts over all pairs of small point sets.  The kernel code itself is not sanitized.
#include <algorithm>
#include <cstring>

#include "cellbin.h"
#include "cellspatial_host.h"

namespace {

struct CellSpatialArgs {
  CellBin b;                       // the points, the grid and the records in (cell, class) order
  int n, C, B, nblk;
  int reach;                       // e_B
  int e2[CS_MAX_BINS];             // e_t^2, CS_NO_EDGE from B on
  unsigned long long* pair_hist;   // [C][C][B]
  int32_t* nn_d2;                  // [n][C]
  unsigned long long* class_n;     // [C]
};

__global__ __launch_bounds__(256) void cs_zero_kernel(CellSpatialArgs a) {
  if (*a.b.flag) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < a.C * a.C * a.B) a.pair_hist[i] = 0;
  if (i < a.C) a.class_n[i] = 0;
}

// as compiled: 30 VGPRs, 78 SGPRs, no scratch, no static LDS (the dynamic carve above); registers allow 8 waves per SIMD, so LDS sets the occupancy
__global__ __launch_bounds__(CS_NT) void cs_search_kernel(CellSpatialArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char cs_lds[];
  const CellBin& g = a.b;
  if (*g.flag) return;                                   // the binning met a point outside the box: nothing is written (uniform)
  const int tid = threadIdx.x, lane = tid & 63, wbase = tid & ~63;
  const int C = a.C, B = a.B, sub = C + 1;
  unsigned long long* __restrict__ table = reinterpret_cast<unsigned long long*>(cs_lds);
  unsigned* __restrict__ priv = reinterpret_cast<unsigned*>(cs_lds + cs_lds_priv_off(C, B));
  int* __restrict__ e2 = reinterpret_cast<int*>(cs_lds + cs_lds_e2_off(C, B));
  int* __restrict__ cls = reinterpret_cast<int*>(cs_lds + cs_lds_cls_off(C, B));
  unsigned* __restrict__ cn = reinterpret_cast<unsigned*>(cs_lds + cs_lds_cn_off(C, B));
  for (int i = tid; i < C * C * B; i += CS_NT) table[i] = 0;
  if (tid < CS_MAX_BINS) e2[tid] = a.e2[tid];
  if (tid < 16) cn[tid] = 0;
  __syncthreads();
  const int reach = a.reach, reach2 = reach * reach;     // e_B and e_B^2 <= 2^28
  for (int blk = blockIdx.x; blk < a.nblk; blk += gridDim.x) {          // uniform over the workgroup: every thread meets every barrier
    const int q = blk * CS_NT + tid;
    const bool active = q < a.n;
    const int4 me = active ? g.recs[q] : make_int4(g.x_min, g.y_min, -1, -1);
    const int my_class = active ? cs_class(me.z, C) : C;
    cls[tid] = my_class;
    if (my_class < C) atomicAdd(&cn[my_class], 1u);
    const int cx = (me.x - g.x_min) / g.side, cy = (me.y - g.y_min) / g.side;
    const int cx0 = max(cx - 1, 0), cx1 = active ? min(cx + 1, g.ncx - 1) : -1;      // an idle thread walks no cell
    const int cy0 = max(cy - 1, 0), cy1 = min(cy + 1, g.ncy - 1);
    for (int b = 0; b < C; ++b) {
      for (int t = 0; t < B; ++t) priv[cs_priv_at(t, tid)] = 0;
      int best = CS_NO_EDGE;
      for (int gy = cy0; gy <= cy1; ++gy)
        for (int gx = cx0; gx <= cx1; ++gx) {
          const int key = cell_key(gy * g.ncx + gx, b, sub);
          const int j0 = g.cell_start[key], j1 = g.cell_start[key + 1];
          for (int j = j0; j < j1; ++j) {
            const int4 o = g.recs[j];
            const int dd = cell_pair_d2(o.x - me.x, o.y - me.y, reach, reach2);
            if (dd < 0 || o.w == me.w) continue;
            best = min(best, dd);
            priv[cs_priv_at(cs_bin_of(e2, dd), tid)] += 1;
          }
        }
      if (active) a.nn_d2[(size_t)me.w * C + b] = best == CS_NO_EDGE ? -1 : best;
      __syncthreads();
      if (lane < B) {                                    // row `lane` of this wave's 64 columns, in pieces of one query class
        int cur = C;
        unsigned long long acc = 0;
        for (int jj = 0; jj < 64; ++jj) {
          const int col = wbase + cs_rotated_column(jj, lane);
          const int aj = cls[col];
          if (aj != cur) {
            if (acc && cur < C) atomicAdd(&table[cs_table_at(cur, b, lane, C, B)], acc);
            cur = aj; acc = 0;
          }
          acc += priv[cs_priv_at(lane, col)];
        }
        if (acc && cur < C) atomicAdd(&table[cs_table_at(cur, b, lane, C, B)], acc);
      }
      __syncthreads();
    }
  }
  for (int i = tid; i < C * C * B; i += CS_NT)
    if (table[i]) atomicAdd(&a.pair_hist[i], table[i]);
  if (tid < C && cn[tid]) atomicAdd(&a.class_n[tid], (unsigned long long)cn[tid]);
}

}  // namespace

extern "C" int nuhtc_cell_spatial(int device, const int32_t* points, const int32_t* labels, int64_t n, int num_classes, const int32_t* edges,
                                  int num_bins, int x_min, int y_min, int x_max, int y_max, int64_t* pair_hist, int32_t* nn_d2, int64_t* class_n,
                                  void* stream) {
  CellSpatialArgs a;
  memset(&a, 0, sizeof(a));
  if (!cs_edges_ok(edges, num_bins, a.e2) || !cell_call_ok(n, CELL_MAX_POINTS, num_classes, edges[num_bins - 1], x_min, y_min, x_max, y_max))
    return NUHTC_E_INVALID;
  if (!pair_hist || !class_n || (n > 0 && (!points || !labels || !nn_d2))) return NUHTC_E_INVALID;
  if (hipSetDevice(device) != hipSuccess) return NUHTC_E_HIP;
  hipStream_t s = (hipStream_t)stream;
  const int C = num_classes, B = num_bins;
  if (n == 0) {
    if (hipMemsetAsync(pair_hist, 0, (size_t)C * C * B * sizeof(int64_t), s) != hipSuccess || hipMemsetAsync(class_n, 0, C * sizeof(int64_t), s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
      return NUHTC_E_HIP;
    return 0;
  }
  a.n = (int)n; a.C = C; a.B = B; a.reach = edges[B - 1]; a.nblk = (int)((n + CS_NT - 1) / CS_NT);
  a.pair_hist = reinterpret_cast<unsigned long long*>(pair_hist); a.nn_d2 = nn_d2; a.class_n = reinterpret_cast<unsigned long long*>(class_n);
  DevScratch tmp;      // every temporary of the call, freed on the way out
  const int nchunk = cellbin_setup(a.b, points, labels, (int)n, x_min, y_min, x_max, y_max, edges[B - 1], CS_MAX_CELLS, C + 1, tmp, s);
  if (!nchunk) return NUHTC_E_HIP;
  const int lds = cs_lds_bytes(C, B);
  if (hipFuncSetAttribute((const void*)cs_search_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) return NUHTC_E_HIP;
  {
    ProfScope ps("cell_spatial_bin", 0, 0, s);
    cellbin_launch(a.b, nchunk, s);
    hipLaunchKernelGGL(cs_zero_kernel, dim3((C * C * B + 255) / 256), dim3(256), 0, s, a);
  }
  {
    ProfScope ps("cell_spatial_search", 0, 0, s);
    hipLaunchKernelGGL(cs_search_kernel, dim3(std::min(a.nblk, 2048)), dim3(CS_NT), lds, s, a);
  }
  return cellbin_finish(a.b, s);
}
