// Cell graph of a slide (gfx950): for every nucleus its k nearest nuclei within a radius and the class census of that disc.
//
// Definition (nuhtc_amd/cellgraph.py holds it in full, with the int64 brute-force restatement `graph_reference`): n points in HALF pixels
// (px = rint(x0 + x1), py = rint(y0 + y1) of the record's box, int32, |p| < 2^27: cellgrid_host.h), a radius r in half pixels (1 .. 16384), 1 <= k <= 32.
// The neighbours of i are the j != i with d2 = dx * dx + dy * dy <= r * r (inclusive; coincident points are neighbours), ordered by
// (d2, j) ascending and cut to k; class_count[i][c] counts ALL j != i within the radius with label c, not only the first k.  Everything is
// integer arithmetic, so the result is a pure function of the input.
//
// Stages, all on the caller's stream:
//   geometry   on the HOST, from the bounding box the caller passes in (numpy min / max over the points, O(n), the way nuhtc_merge_overlap
//              gets its extent): the cell side is the smallest multiple of r whose grid over the box has at most 2^22 cells, so side >= r
//              and the 3 x 3 cells around a point always hold its disc.  No reduction kernel, no read-back before the first launch; a
//              point outside the stated box is caught by the binning kernels (flag -> NUHTC_E_INVALID, outputs untouched).
//   binning    cellbin.h, one key per cell: (x, y, label, index) records in cell order, in atomic arrival order INSIDE a cell.
//   search     one thread per record in cell order, the 3 x 3 sweep of cellbin.h (cell_sweep) without the point itself.  A candidate's
//              key is (d2 << 32) | index: one 64-bit total order, so neither the cut at k nor the order of ties can see the arrival
//              order of the scatter.
//
// Where the candidate list lives.  A list is at most 32 keys of 8 bytes and is indexed by a run-time position (sorted insertion), which
// in registers would turn into private scratch memory; it is kept in LDS instead, slot-major (key s of thread t at word s * 256 + t), so
// the 64 lanes of a wave read and write 64 consecutive 8-byte words: conflict-free.  The class census sits behind it the same way
// (counter c of thread t at c * 256 + t).  No per-query global scratch exists.  LDS per 256-thread workgroup = 256 * (8 k + 4 C) bytes,
// sized by the call's k and C: 21,504 B at the tool's k = 8, C = 5 -> 7 workgroups = 28 of a CU's 32 waves by LDS (160 KiB per CU);
// 79,872 B at k = 32, C = 14 -> 2 workgroups = 8 waves per CU, 2 per SIMD.  As compiled the search kernel takes 28 VGPRs and 49 SGPRs
// and no scratch (hipcc -Rpass-analysis=kernel-resource-usage, profiles/cell_graph_resources.txt), so registers never limit it: LDS does, and the 32-wave cap.
#include <algorithm>
#include <cstring>

#include "cellbin.h"

namespace {

constexpr int CG_MAX_CELLS = 1 << 22;
constexpr int CG_NT = 256;                            // threads of the search workgroup

struct CellGraphArgs {
  CellBin b;                // the points, the grid and the records in cell order (cellbin.h, one key per cell)
  int n, C, r, k;
  int32_t* neighbors;       // [n][k]
  int32_t* d2;              // [n][k]
  int32_t* class_count;     // [n][C]
};

__global__ __launch_bounds__(CG_NT) void cg_search_kernel(CellGraphArgs a) {
  extern __shared__ unsigned long long cg_lds[];
  const CellBin& g = a.b;
  if (*g.flag) return;                                   // the binning met a point outside the box: nothing is written
  const int tid = threadIdx.x, q = blockIdx.x * CG_NT + tid;
  if (q >= a.n) return;
  unsigned long long* __restrict__ list = cg_lds + tid;                          // key s at list[s * CG_NT]
  int* __restrict__ census = reinterpret_cast<int*>(cg_lds + a.k * CG_NT) + tid;    // counter c at census[c * CG_NT]
  for (int c = 0; c < a.C; ++c) census[c * CG_NT] = 0;
  const int4 me = g.recs[q];
  const int k = a.k, C = a.C;
  int cnt = 0;
  unsigned long long worst = ~0ull;                      // the k-th key once the list is full: nothing at or above it enters
  cell_sweep(g, me, a.r, [&](const int4& o) { return o.w != me.w; }, [&](int, const int4& o, int dd) {
    if ((unsigned)o.z < (unsigned)C) census[o.z * CG_NT] += 1;
    const unsigned long long key = ((unsigned long long)(unsigned)dd << 32) | (unsigned)o.w;
    if (key >= worst) return;
    int p = cnt < k ? cnt : k - 1;                       // sorted insertion from the end; a full list drops its last key
    while (p > 0) {
      const unsigned long long prev = list[(p - 1) * CG_NT];
      if (prev < key) break;
      list[p * CG_NT] = prev;
      --p;
    }
    list[p * CG_NT] = key;
    if (cnt < k) ++cnt;
    if (cnt == k) worst = list[(k - 1) * CG_NT];
  });
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

}  // namespace

extern "C" int nuhtc_cell_graph(int device, const int32_t* points, const int32_t* labels, int64_t n, int num_classes, int r, int k, int x_min,
                                int y_min, int x_max, int y_max, int32_t* neighbors, int32_t* d2, int32_t* class_count, void* stream) {
  if (!cell_call_ok(n, CELL_MAX_POINTS, num_classes, r, x_min, y_min, x_max, y_max) || k < 1 || k > 32) return NUHTC_E_INVALID;
  if (n > 0 && (!points || !labels || !neighbors || !d2 || !class_count)) return NUHTC_E_INVALID;
  if (n == 0) return 0;
  if (hipSetDevice(device) != hipSuccess) return NUHTC_E_HIP;
  hipStream_t s = (hipStream_t)stream;
  CellGraphArgs a;
  memset(&a, 0, sizeof(a));
  a.n = (int)n; a.C = num_classes; a.r = r; a.k = k;
  a.neighbors = neighbors; a.d2 = d2; a.class_count = class_count;
  DevScratch tmp;      // every temporary of the call, freed on the way out
  const int nchunk = cellbin_setup(a.b, points, labels, (int)n, x_min, y_min, x_max, y_max, r, CG_MAX_CELLS, 1, tmp, s);
  if (!nchunk) return NUHTC_E_HIP;
  const size_t lds = (size_t)CG_NT * (8 * k + 4 * num_classes);
  if (hipFuncSetAttribute((const void*)cg_search_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return NUHTC_E_HIP;
  const unsigned nb = (unsigned)((n + 255) / 256);
  {
    ProfScope ps("cell_graph_bin", 0, 0, s);
    cellbin_launch(a.b, nchunk, s);
  }
  {
    ProfScope ps("cell_graph_search", 0, 0, s);
    hipLaunchKernelGGL(cg_search_kernel, dim3(nb), dim3(CG_NT), lds, s, a);
  }
  return cellbin_finish(a.b, s);
}
