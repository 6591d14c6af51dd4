// Per-nucleus shape integers (gfx950): a pure function of the mask of one list entry, INTEGERS ONLY -- the pixel count A, the bounding
// rectangle x0 y0 x1 y1 (x1, y1 exclusive), the nine coordinate sums up to the third order (Sx Sy Sxx Sxy Syy Sxxx Sxxy Sxyy Syyy, x the
// column and y the row in frame pixels) and the ten box counts N_1 .. N_10: N_j counts the squares of side 2^j anchored at the
// rectangle's corner that hold a set pixel and an unset position (a position outside the rectangle is unset): int64 [24] a nucleus.
// nuhtc_amd/nucshape.py defines them, restates them in numpy (shape_reference: the device equals it bit for bit) and derives the seven
// Shape.HuMoments* and Shape.FractalDimension from them on the host in float64.
//
// One workgroup of 256 threads per nucleus, the shape of nucleus_gradient_kernel (nucgrad.hip); it reads mask words only:
//   1. all threads scan the mask for its rectangle and area (block_mask_rect_256, maskbits.h);
//   2. the sums: one thread per mask word of the rectangle, the padding bits of a row's last word masked off on every read; the set-bit
//      loop takes the word's own sums of x, x^2, x^3, the row's y multiplies them once a word; nine per-thread int64, integer wave
//      reductions (block_prims.h), then across the four waves;
//   3. the box counts from a pyramid of two bit planes, "any set" and "all set" (nucshape_host.h).  The front: one thread per word of
//      level 2 takes four mask rows of 128 pixels, aligned to x0 by a funnel shift across adjacent words (rows below the rectangle and
//      words behind it read as zero and are never addressed), builds levels 1 and 2 IN REGISTERS, counts N_1 and N_2 and keeps the
//      level-2 word in LDS -- level 1 of a 1024-px rectangle (2 x 32 KB) is never stored.  Each further level comes from four children
//      in LDS, any = OR, all = AND, a child outside the level empty; N_j = the population count of any & ~all over the level; one
//      barrier a level;
//   4. the row leaves with ordinary vector stores.
// Integer adds in any grouping give the same bits: a row is bitwise repeatable across runs and batch splits.
// LDS: the two planes of the levels 2 .. 10 sized for the 1024-px frame, 2 x 2751 words = 22 008 B; 4 x 9 int64 and 4 x 10 ints of the
// reductions, the rectangle scan's 20 ints: 22 544 B a workgroup with alignment (7 workgroups a CU).
#include "maskbits.h"
#include "nucleus_list.h"
#include "nucshape_host.h"

namespace {

struct NucShapeParams {
  NucleusList list;
  NucleusMasks m;
  int64_t* shape;          // [n_max][24]
};

__global__ __launch_bounds__(256) void nucleus_shape_kernel(NucShapeParams p) {
  __shared__ uint32_t any_pl[NUCSHAPE_PLANE];
  __shared__ uint32_t all_pl[NUCSHAPE_PLANE];
  __shared__ long long reds[4][NUCSHAPE_NSUMS];
  __shared__ int redn[4][NUCSHAPE_LEVELS];
  __shared__ int red[4][5];
  const int d = blockIdx.x, H = p.m.H, wpr = p.m.wpr;
  long long b, r;
  const NucleusEntry at = nucleus_entry(p.list, d, b, r);
  if (at == NUCLEUS_PAST) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int64_t* __restrict__ out = p.shape + (long long)d * NUCSHAPE_ROW;
  const auto zero_row = [&] {
    if (tid < NUCSHAPE_ROW) out[tid] = 0;
  };
  if (at == NUCLEUS_OUTSIDE) { zero_row(); return; }
  const uint32_t* __restrict__ m = nucleus_mask(p.m, p.list.K, b, r);
  const unsigned last = nucleus_last_word(p.m);

  const MaskRect rc = block_mask_rect_256(m, H, wpr, last, red);
  if (rc.area < 1) { zero_row(); return; }
  const int x0 = rc.x0, y0 = rc.y0, w = rc.x1 - rc.x0 + 1, h = rc.y1 - rc.y0 + 1;      // 1 <= w, h <= 1024; y0 + h <= H
  const int wx0 = x0 >> 5, wx1 = rc.x1 >> 5, nw = wx1 - wx0 + 1;                       // wx1 <= wpr - 1

  // ---- the sums
  long long s[NUCSHAPE_NSUMS] = {0, 0, 0, 0, 0, 0, 0, 0, 0};                           // Sx Sy Sxx Sxy Syy Sxxx Sxxy Sxyy Syyy
  for (int i = tid; i < h * nw; i += 256) {
    const int rr = i / nw, cw = wx0 + i - rr * nw;
    unsigned v = nucshape_mask_word(m + (long long)(y0 + rr) * wpr, cw, wx1, wpr, last);
    if (!v) continue;
    const long long y = y0 + rr, cnt = __popc(v);
    long long sx = 0, sxx = 0, sxxx = 0;
    for (; v; v &= v - 1) {
      const long long x = cw * 32 + __ffs(v) - 1;
      sx += x; sxx += x * x; sxxx += x * x * x;
    }
    s[0] += sx; s[1] += y * cnt; s[2] += sxx; s[3] += y * sx; s[4] += y * y * cnt;
    s[5] += sxxx; s[6] += y * sxx; s[7] += y * y * sx; s[8] += y * y * y * cnt;
  }
#pragma unroll
  for (int k = 0; k < NUCSHAPE_NSUMS; ++k) {
    const long long v = wave_sum(s[k]);
    if (lane == 0) reds[wave][k] = v;
  }

  // ---- the front: levels 1 and 2 from the mask rows, level 2 into LDS
  int n[NUCSHAPE_LEVELS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  {
    const int R = nucshape_rows(h, 2), P = nucshape_words(w, 2);                       // R <= 256, P <= 8: R * P <= 2048 words
    for (int i = tid; i < R * P; i += 256) {
      const int r2 = i / P, k2 = i - r2 * P;
      uint32_t px[4][4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int v = 4 * r2 + t;                                                      // the aligned row: inside the rectangle or zero
#pragma unroll
        for (int a = 0; a < 4; ++a)
          px[t][a] = v < h ? nucshape_aligned_word(m + (long long)(y0 + v) * wpr, x0, 4 * k2 + a, wx1, wpr, last) : 0u;
      }
      uint32_t any2, all2;
      int n1, n2;
      nucshape_front(px, any2, all2, n1, n2);
      n[0] += n1; n[1] += n2;
      any_pl[i] = any2; all_pl[i] = all2;                                              // nucshape_base(2) == 0, pitch P
    }
  }
  __syncthreads();

  // ---- the levels 3 .. 10, each from its four children
#pragma unroll
  for (int L = 3; L <= NUCSHAPE_LEVELS; ++L) {
    const int Rc = nucshape_rows(h, L - 1), Pc = nucshape_words(w, L - 1), R = nucshape_rows(h, L), P = nucshape_words(w, L);
    const uint32_t* ca = any_pl + nucshape_base(L - 1);
    const uint32_t* cl = all_pl + nucshape_base(L - 1);
    for (int i = tid; i < R * P; i += 256) {                                           // R * P <= nucshape_level_words(L)
      const int rr = i / P, k = i - rr * P;
      const int r0 = 2 * rr, r1 = r0 + 1, k0 = 2 * k, k1 = k0 + 1;                     // r0 < Rc and k0 < Pc always
      const bool hr = r1 < Rc, hk = k1 < Pc;
      uint32_t any, all;
      nucshape_parent(ca[r0 * Pc + k0], hk ? ca[r0 * Pc + k1] : 0u, hr ? ca[r1 * Pc + k0] : 0u, hr && hk ? ca[r1 * Pc + k1] : 0u,
                      cl[r0 * Pc + k0], hk ? cl[r0 * Pc + k1] : 0u, hr ? cl[r1 * Pc + k0] : 0u, hr && hk ? cl[r1 * Pc + k1] : 0u, any, all);
      n[L - 1] += nucshape_mixed(any, all);
      any_pl[nucshape_base(L) + i] = any; all_pl[nucshape_base(L) + i] = all;
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < NUCSHAPE_LEVELS; ++k) {
    const int v = wave_sum(n[k]);
    if (lane == 0) redn[wave][k] = v;
  }
  __syncthreads();
  if (tid < NUCSHAPE_ROW) {                               // A, x0 y0 x1 y1, the nine sums, N_1 .. N_10
    long long v;
    if (tid == 0) v = rc.area;
    else if (tid < NUCSHAPE_SUMS) v = tid == 1 ? x0 : tid == 2 ? y0 : tid == 3 ? x0 + w : y0 + h;
    else if (tid < NUCSHAPE_BOXES) { const int k = tid - NUCSHAPE_SUMS; v = reds[0][k] + reds[1][k] + reds[2][k] + reds[3][k]; }
    else { const int k = tid - NUCSHAPE_BOXES; v = (long long)redn[0][k] + redn[1][k] + redn[2][k] + redn[3][k]; }
    out[tid] = v;
  }
}

int launch_nucleus_shape(const NucShapeParams& p, hipStream_t s) {
  // the bytes of a batch depend on its masks: the profile records the time alone
  ProfScope ps("nucleus_shape", 0, 0, s);
  hipLaunchKernelGGL(nucleus_shape_kernel, dim3((unsigned)p.list.n_max), dim3(256), 0, s, p);
  return launched() ? 0 : NUHTC_E_HIP;
}

}  // namespace

extern "C" {

int nuhtc_op_nucleus_shape(nuhtc_engine* e, int B, const uint32_t* masks, int K, int H, int W, const int32_t* pairs_dev, const int32_t* n_dev,
                           int n_max, int64_t* shape, void* stream) {
  if (!e || !masks || !pairs_dev || !shape) return NUHTC_E_INVALID;
  const std::string why = nucshape_args_error(B, K, H, W, n_max);
  if (!why.empty()) FAIL(e, NUHTC_E_INVALID, why);
  NucShapeParams p{};
  nucleus_op_route(B, masks, K, H, W, pairs_dev, n_dev, n_max, p.list, p.m);
  p.shape = shape;
  HIP_CHECK(e, hipSetDevice(e->device));
  hipStream_t s = (hipStream_t)stream;
  return op_finish(e, launch_nucleus_shape(p, s), s, "nucleus_shape launch failed", "nucleus_shape kernel failed");
}

}  // extern "C"
