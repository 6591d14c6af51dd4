// Cell graph of a slide (gfx950): for every nucleus its k nearest nuclei within a radius and the class census of that disc.
//
// Definition (nuhtc_amd/cellgraph.py holds it in full, with the int64 brute-force restatement `graph_reference`): n points in HALF pixels
// (px = rint(x0 + x1), py = rint(y0 + y1) of the record's box, int32, |p| < 2^27), a radius r in half pixels (1 .. 16384), 1 <= k <= 32.
// The neighbours of i are the j != i with d2 = dx * dx + dy * dy <= r * r (inclusive; coincident points are neighbours), ordered by
// (d2, j) ascending and cut to k; class_count[i][c] counts ALL j != i within the radius with label c, not only the first k.  Everything is
// integer arithmetic, so the result is a pure function of the input.
//
// Stages, all on the caller's stream:
//   geometry   on the HOST, from the bounding box the caller passes in (numpy min / max over the points, O(n), the way nuhtc_merge_overlap
//              gets its extent): the cell side is the smallest multiple of r whose grid over the box has at most 2^22 cells, so side >= r
//              and the 3 x 3 cells around a point always hold its disc.  No reduction kernel, no read-back before the first launch; a
//              point outside the stated box is caught by the binning kernels (flag -> NUHTC_E_INVALID, outputs untouched).
//   binning    histogram of the points per cell (atomics), exclusive scan of the cells (block_exscan_1024 of block_prims.h on 16 cells
//              per thread: per-chunk totals, a scan of the totals, the chunks again with their base), scatter of (x, y, label, index)
//              records into cell order.  The order of the records INSIDE a cell is atomic arrival order.
//   search     one thread per record in cell order, so the lanes of a wave sit in the same or adjacent cells and read the same records
//              (one 16-byte load per record, the same address across most of the wave).  Per grid row the three cells are one contiguous
//              range of records.  A candidate's key is (d2 << 32) | index: one 64-bit total order, so neither the cut at k nor the order
//              of ties can see the arrival order of the scatter.
//
// Where the candidate list lives.  A list is at most 32 keys of 8 bytes and is indexed by a run-time position (sorted insertion), which
// in registers would turn into private scratch memory; it is kept in LDS instead, slot-major (key s of thread t at word s * 256 + t), so
// the 64 lanes of a wave read and write 64 consecutive 8-byte words: conflict-free.  The class census sits behind it the same way
// (counter c of thread t at c * 256 + t).  No per-query global scratch exists.  LDS per 256-thread workgroup = 256 * (8 k + 4 C) bytes,
// sized by the call's k and C: 21,504 B at the tool's k = 8, C = 5 -> 7 workgroups = 28 of a CU's 32 waves by LDS (160 KiB per CU);
// 79,872 B at k = 32, C = 14 -> 2 workgroups = 8 waves per CU, 2 per SIMD.  As compiled the search kernel takes 28 VGPRs and 52 SGPRs
// and no scratch (hipcc -Rpass-analysis=kernel-resource-usage), so registers never limit it: LDS does, and the 32-wave cap.
#include <algorithm>
#include <cstring>

#include "block_prims.h"
#include "common.h"

namespace {

constexpr int CG_MAX_CELLS = 1 << 22;
constexpr int CG_SCAN_PER = 16;                       // cells per thread of the scan
constexpr int CG_CHUNK = 1024 * CG_SCAN_PER;          // cells per workgroup of the scan
constexpr int CG_NT = 256;                            // threads of the search workgroup

struct CellGraphArgs {
  const int32_t* points;    // [n][2] half pixels
  const int32_t* labels;    // [n]
  int n, C, r, k;
  int x_min, y_min, x_max, y_max, side, ncx, ncy;
  int* cell_count;          // [nchunk * CG_CHUNK], zero past the grid; counted up by the histogram, down again by the scatter
  int* cell_start;          // [nchunk * CG_CHUNK]: entry c = records in front of cell c (entry ncx * ncy: all of them)
  int* chunk_base;          // [1024]: records in front of each scan chunk
  int4* recs;               // [n] (x, y, label, index) in cell order
  int* flag;                // != 0: a point lies outside the stated bounding box
  int32_t* neighbors;       // [n][k]
  int32_t* d2;              // [n][k]
  int32_t* class_count;     // [n][C]
};

// the cell of point i, or -1 (and the flag) when it lies outside the box the grid was laid over
__device__ __forceinline__ int cell_of(const CellGraphArgs& a, int x, int y) {
  if (x < a.x_min || x > a.x_max || y < a.y_min || y > a.y_max) { *a.flag = 1; return -1; }
  return ((y - a.y_min) / a.side) * a.ncx + (x - a.x_min) / a.side;
}

__global__ __launch_bounds__(256) void cg_count_kernel(CellGraphArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const int c = cell_of(a, a.points[2 * i], a.points[2 * i + 1]);
  if (c >= 0) atomicAdd(&a.cell_count[c], 1);
}

// sum of the 16 cells of this thread (two 32-byte halves: 16-byte vector loads)
__device__ __forceinline__ int load16(const int* __restrict__ src, int v[CG_SCAN_PER]) {
  int s = 0;
#pragma unroll
  for (int q = 0; q < CG_SCAN_PER / 4; ++q) {
    const int4 w = reinterpret_cast<const int4*>(src)[q];
    v[4 * q] = w.x; v[4 * q + 1] = w.y; v[4 * q + 2] = w.z; v[4 * q + 3] = w.w;
    s += w.x + w.y + w.z + w.w;
  }
  return s;
}

__global__ __launch_bounds__(1024) void cg_chunk_total_kernel(CellGraphArgs a) {
  __shared__ int lds16[17];
  int v[CG_SCAN_PER], total;
  const int s = load16(a.cell_count + (size_t)blockIdx.x * CG_CHUNK + threadIdx.x * CG_SCAN_PER, v);
  block_exscan_1024(s, lds16, &total);
  if (threadIdx.x == 0) a.chunk_base[blockIdx.x] = total;
}

__global__ __launch_bounds__(1024) void cg_chunk_scan_kernel(CellGraphArgs a, int nchunk) {
  __shared__ int lds16[17];
  int total;
  const int v = (int)threadIdx.x < nchunk ? a.chunk_base[threadIdx.x] : 0;
  const int ex = block_exscan_1024(v, lds16, &total);
  if ((int)threadIdx.x < nchunk) a.chunk_base[threadIdx.x] = ex;
}

__global__ __launch_bounds__(1024) void cg_cell_scan_kernel(CellGraphArgs a) {
  __shared__ int lds16[17];
  int v[CG_SCAN_PER], total;
  const size_t at = (size_t)blockIdx.x * CG_CHUNK + threadIdx.x * CG_SCAN_PER;
  const int s = load16(a.cell_count + at, v);
  int acc = a.chunk_base[blockIdx.x] + block_exscan_1024(s, lds16, &total);
#pragma unroll
  for (int q = 0; q < CG_SCAN_PER / 4; ++q) {
    int4 w;
    w.x = acc; acc += v[4 * q];
    w.y = acc; acc += v[4 * q + 1];
    w.z = acc; acc += v[4 * q + 2];
    w.w = acc; acc += v[4 * q + 3];
    reinterpret_cast<int4*>(a.cell_start + at)[q] = w;
  }
}

__global__ __launch_bounds__(256) void cg_scatter_kernel(CellGraphArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const int x = a.points[2 * i], y = a.points[2 * i + 1];
  const int c = cell_of(a, x, y);
  if (c < 0) return;
  const int pos = a.cell_start[c] + atomicSub(&a.cell_count[c], 1) - 1;       // the cell fills from its end; the counts return to zero
  a.recs[pos] = make_int4(x, y, a.labels[i], i);
}

__global__ __launch_bounds__(CG_NT) void cg_search_kernel(CellGraphArgs a) {
  extern __shared__ unsigned long long cg_lds[];
  if (*a.flag) return;                                   // the binning met a point outside the box: nothing is written
  const int tid = threadIdx.x, q = blockIdx.x * CG_NT + tid;
  if (q >= a.n) return;
  unsigned long long* __restrict__ list = cg_lds + tid;                          // key s at list[s * CG_NT]
  int* __restrict__ census = reinterpret_cast<int*>(cg_lds + a.k * CG_NT) + tid;    // counter c at census[c * CG_NT]
  for (int c = 0; c < a.C; ++c) census[c * CG_NT] = 0;
  const int4 me = a.recs[q];
  const int cx = (me.x - a.x_min) / a.side, cy = (me.y - a.y_min) / a.side;
  const int r = a.r, r2 = r * r, k = a.k;
  const int cx0 = max(cx - 1, 0), cx1 = min(cx + 1, a.ncx - 1);
  int cnt = 0;
  unsigned long long worst = ~0ull;                      // the k-th key once the list is full: nothing at or above it enters
  for (int gy = max(cy - 1, 0); gy <= min(cy + 1, a.ncy - 1); ++gy) {
    const int j0 = a.cell_start[gy * a.ncx + cx0], j1 = a.cell_start[gy * a.ncx + cx1 + 1];
    for (int j = j0; j < j1; ++j) {
      const int4 o = a.recs[j];
      const int dx = o.x - me.x, dy = o.y - me.y;        // |p| < 2^27: no overflow
      if (o.w == me.w || dx > r || dx < -r || dy > r || dy < -r) continue;
      const int dd = dx * dx + dy * dy;                  // <= 2 * 16384^2 = 2^29
      if (dd > r2) continue;
      if ((unsigned)o.z < (unsigned)a.C) census[o.z * CG_NT] += 1;
      const unsigned long long key = ((unsigned long long)(unsigned)dd << 32) | (unsigned)o.w;
      if (key >= worst) continue;
      int p = cnt < k ? cnt : k - 1;                     // sorted insertion from the end; a full list drops its last key
      while (p > 0) {
        const unsigned long long prev = list[(p - 1) * CG_NT];
        if (prev < key) break;
        list[p * CG_NT] = prev;
        --p;
      }
      list[p * CG_NT] = key;
      if (cnt < k) ++cnt;
      if (cnt == k) worst = list[(k - 1) * CG_NT];
    }
  }
  int32_t* __restrict__ nb = a.neighbors + (size_t)me.w * k;
  int32_t* __restrict__ dd = a.d2 + (size_t)me.w * k;
  for (int s = 0; s < k; ++s) {
    const unsigned long long key = s < cnt ? list[s * CG_NT] : ~0ull;          // ~0: both halves are -1
    nb[s] = (int32_t)(unsigned)key;
    dd[s] = (int32_t)(unsigned)(key >> 32);
  }
  int32_t* __restrict__ cc = a.class_count + (size_t)me.w * a.C;
  for (int c = 0; c < a.C; ++c) cc[c] = census[c * CG_NT];
}

// cells of the grid of side `side` over [lo, hi]
inline long long cells_along(int lo, int hi, long long side) { return ((long long)hi - lo) / side + 1; }

}  // namespace

extern "C" int nuhtc_cell_graph(int device, const int32_t* points, const int32_t* labels, int64_t n, int num_classes, int r, int k, int x_min,
                                int y_min, int x_max, int y_max, int32_t* neighbors, int32_t* d2, int32_t* class_count, void* stream) {
  constexpr int LIM = 1 << 27;
  if (n < 0 || n > (1 << 28) || k < 1 || k > 32 || r < 1 || r > 16384 || num_classes < 1 || num_classes > 14) return NUHTC_E_INVALID;
  if (n > 0 && (!points || !labels || !neighbors || !d2 || !class_count)) return NUHTC_E_INVALID;
  if (n > 0 && (x_min > x_max || y_min > y_max || x_min <= -LIM || y_min <= -LIM || x_max >= LIM || y_max >= LIM)) return NUHTC_E_INVALID;
  if (n == 0) return 0;
  if (hipSetDevice(device) != hipSuccess) return NUHTC_E_HIP;
  hipStream_t s = (hipStream_t)stream;
  CellGraphArgs a;
  memset(&a, 0, sizeof(a));
  a.points = points; a.labels = labels; a.n = (int)n; a.C = num_classes; a.r = r; a.k = k;
  a.x_min = x_min; a.y_min = y_min; a.x_max = x_max; a.y_max = y_max;
  a.neighbors = neighbors; a.d2 = d2; a.class_count = class_count;
  // the smallest multiple m * r with at most 2^22 cells (the cell count does not grow with m): bisection on m
  long long lo = 1, hi = (1LL << 29) / r + 1;             // at hi the grid is one cell
  while (lo < hi) {
    const long long m = (lo + hi) / 2;
    if (cells_along(x_min, x_max, m * r) * cells_along(y_min, y_max, m * r) <= CG_MAX_CELLS) hi = m; else lo = m + 1;
  }
  a.side = (int)(lo * r);
  a.ncx = (int)cells_along(x_min, x_max, a.side); a.ncy = (int)cells_along(y_min, y_max, a.side);
  const int ncell = a.ncx * a.ncy;
  const int nchunk = (ncell + 1 + CG_CHUNK - 1) / CG_CHUNK;      // + 1: the entry behind the last cell holds the total; at most 257
  const size_t cells_bytes = (size_t)nchunk * CG_CHUNK * sizeof(int);
  DevScratch tmp;      // every temporary of the call, freed on the way out
  a.cell_count = tmp.alloc<int>(cells_bytes); a.cell_start = tmp.alloc<int>(cells_bytes);
  a.chunk_base = tmp.alloc<int>(1024 * sizeof(int)); a.flag = tmp.alloc<int>(sizeof(int));
  a.recs = tmp.alloc<int4>((size_t)n * sizeof(int4));
  if (!tmp.ok()) return NUHTC_E_HIP;
  if (hipMemsetAsync(a.cell_count, 0, cells_bytes, s) != hipSuccess || hipMemsetAsync(a.flag, 0, sizeof(int), s) != hipSuccess) return NUHTC_E_HIP;
  const size_t lds = (size_t)CG_NT * (8 * k + 4 * num_classes);
  if (hipFuncSetAttribute((const void*)cg_search_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return NUHTC_E_HIP;
  const unsigned nb = (unsigned)((n + 255) / 256);
  {
    ProfScope ps("cell_graph_bin", 0, 0, s);
    hipLaunchKernelGGL(cg_count_kernel, dim3(nb), dim3(256), 0, s, a);
    hipLaunchKernelGGL(cg_chunk_total_kernel, dim3(nchunk), dim3(1024), 0, s, a);
    hipLaunchKernelGGL(cg_chunk_scan_kernel, dim3(1), dim3(1024), 0, s, a, nchunk);
    hipLaunchKernelGGL(cg_cell_scan_kernel, dim3(nchunk), dim3(1024), 0, s, a);
    hipLaunchKernelGGL(cg_scatter_kernel, dim3(nb), dim3(256), 0, s, a);
  }
  {
    ProfScope ps("cell_graph_search", 0, 0, s);
    hipLaunchKernelGGL(cg_search_kernel, dim3(nb), dim3(CG_NT), lds, s, a);
  }
  int h_flag = 0;
  if (!launched() || hipMemcpyAsync(&h_flag, a.flag, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
    return NUHTC_E_HIP;
  return h_flag ? NUHTC_E_INVALID : 0;
}
