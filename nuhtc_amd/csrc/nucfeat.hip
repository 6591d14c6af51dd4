// Per-nucleus embeddings (gfx950): the FPN maps of a tile averaged under the final mask of one kept detection.
//
// For a mask M (H x W bits, A = set pixels) and level l (map x_l [H_l][W_l][64], stride s_l in mask pixels):
//   w_l(i, j) = set pixels (y, x) with y / s_l == i and x / s_l == j          (an integer, 0 .. s_l * s_l)
//   e_l[c]    = (sum over cells of w_l(i, j) * x_l[i][j][c]) / A              -> out[l * 64 + c], 256 floats, level 0 first
// i.e. the mean over the nucleus's pixels of each map upsampled piecewise-constant (nuhtc_amd/nucfeat.py pool_reference is the float64
// restatement).  The layout of the row is that of nuhtc_features (csrc/pool.hip), which is the same mean under a mask of the whole image.
//
// One workgroup per nucleus, 256 threads: all of them scan the mask once for its bounding rectangle and area (H * W / 32 words, 8 KB for
// a 256-px tile), then wave l takes level l with lane = channel, so a cell is one coalesced 256-byte row.  Only the cells the rectangle
// touches are visited: per cell row the lanes count the weights of 64 cells (popcounts of the mask words under the cell, split at word
// boundaries, so any stride works), the weights are read lane by lane into scalars and the non-zero ones enter ONE fused multiply-add chain
// per (level, channel), cells in row-major order.  That order is a function of the mask alone: no atomics, no partial sums whose
// grouping depends on the launch, so a nucleus gives the same bits in any batch, on any call.  Error against exact arithmetic: n
// roundings of the chain (n = non-zero cells; w converts exactly, the product is not rounded) and one of the division:
// |got - exact| <= ((1 + u)^(n + 1) - 1) * sum(w |x|) / A with u = 2^-24, below (n + 3) u sum(w |x|) / A for every n a mask can have
// here (n^2 u < 4).
//
// Bytes per nucleus: the mask scan (H * W / 8) plus 256 bytes per visited cell; a 20 x 20 px nucleus at strides 2 / 4 / 8 / 16 touches
// about 100 + 36 + 9 + 4 cells = 37 KB of map rows, all L2 hits behind the inference that wrote them.
#include <climits>

#include "maskbits.h"
#include "nucleus_list.h"

namespace {

struct NucPoolParams {
  const float* x[4];       // level maps [B][Hl][Wl][64]
  int Hl[4], Wl[4], stride[4];
  NucleusList list;
  NucleusMasks m;          // the padding bits of a row's last word are zero: W is not read
  float* out;              // [n_max][256]
};

// set bits of row words `row` in the columns [cx0, cx1), which may span several words
__device__ __forceinline__ int row_popc(const uint32_t* __restrict__ row, int cx0, int cx1) {
  int cnt = 0;
  for (int wv = cx0 >> 5; wv <= (cx1 - 1) >> 5; ++wv) {
    const int lo = max(cx0 - wv * 32, 0), hi = min(cx1 - wv * 32, 32);
    const unsigned bits = (hi - lo == 32 ? 0xffffffffu : ((1u << (hi - lo)) - 1u)) << lo;
    cnt += __popc(row[wv] & bits);
  }
  return cnt;
}

__global__ __launch_bounds__(256) void nucleus_pool_kernel(NucPoolParams p) {
  __shared__ int red[4][5];
  const int d = blockIdx.x, H = p.m.H, wpr = p.m.wpr;
  long long b, r;
  const NucleusEntry at = nucleus_entry(p.list, d, b, r);
  if (at == NUCLEUS_PAST) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* __restrict__ dst = p.out + (long long)d * 256 + tid;
  const auto zero_row = [&] { *dst = 0.f; };
  if (at == NUCLEUS_OUTSIDE) { zero_row(); return; }
  const uint32_t* __restrict__ m = nucleus_mask(p.m, p.list.K, b, r);

  // ---- bounding rectangle and area of the mask (maskbits.h)
  const MaskRect rc = block_mask_rect_256(m, H, wpr, ~0u, red);
  const int y0 = rc.y0, y1 = rc.y1, x0 = rc.x0, x1 = rc.x1, area = rc.area;
  if (area == 0) { zero_row(); return; }

  // ---- wave = level, lane = channel
  const int s = p.stride[wave], Hl = p.Hl[wave], Wl = p.Wl[wave];
  const float* __restrict__ xl = p.x[wave] + b * (long long)Hl * Wl * 64 + lane;
  const int i0 = y0 / s, i1 = min(y1 / s, Hl - 1), j0 = x0 / s, j1 = min(x1 / s, Wl - 1);
  float acc = 0.f;
  for (int i = i0; i <= i1; ++i) {
    const int ry0 = i * s, ry1 = min(ry0 + s, H);
    for (int jb = j0; jb <= j1; jb += 64) {
      int wgt = 0;                                       // lane t: the weight of cell (i, jb + t)
      if (jb + lane <= j1) {
        const int cx0 = (jb + lane) * s, cx1 = min(cx0 + s, wpr * 32);
        for (int y = ry0; y < ry1; ++y) wgt += row_popc(m + (long long)y * wpr, cx0, cx1);
      }
      const int cnt = min(64, j1 - jb + 1);
      const float* __restrict__ row = xl + ((long long)i * Wl + jb) * 64;
      for (int t = 0; t < cnt; t += 4) {                // four loads in flight; the chain itself stays in cell order
        float v[4];
        int w[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int tt = min(t + u, cnt - 1);
          v[u] = row[tt * 64];
          w[u] = t + u < cnt ? __builtin_amdgcn_readlane(wgt, tt) : 0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (w[u]) acc = fmaf((float)w[u], v[u], acc);
      }
    }
  }
  *dst = __fdiv_rn(acc, (float)area);
}

int launch_nucleus_pool(const NucPoolParams& p, hipStream_t s) {
  if (p.list.n_max < 1) return 0;
  // the bytes of a batch depend on its masks: the profile records the time alone
  ProfScope ps("nucleus_pool", 0, 0, s);
  hipLaunchKernelGGL(nucleus_pool_kernel, dim3((unsigned)p.list.n_max), dim3(256), 0, s, p);
  return launched() ? 0 : NUHTC_E_HIP;
}

}  // namespace

extern "C" {

int nuhtc_nucleus_features(nuhtc_engine* e, const nuhtc_dets* dets, int B, const int64_t* idx_dev, const int32_t* n_dev, int cap, float* feat_dev,
                           void* stream) {
  NucPoolParams p{};
  if (const int rc = nucleus_engine_route(e, "nuhtc_nucleus_features", "pool under", dets, B, idx_dev, n_dev, cap, feat_dev && B >= 1 && cap >= 1, p.list, p.m)) return rc;
  const nuhtc_config& c = e->cfg;
  const int sf = (int)c.scale_factor;
  for (int l = 0; l < 4; ++l) {
    // a map cell of stride 4 << l in network pixels covers (4 << l) / scale_factor mask pixels: whole pixels for scale factors 1, 2 and 4
    if ((float)sf != c.scale_factor || sf < 1 || (4 << l) % sf) FAIL(e, NUHTC_E_INVALID, "nuhtc_nucleus_features: scale_factor must be 1, 2 or 4 (whole mask pixels per map cell)");
    p.x[l] = e->x[l]; p.Hl[l] = e->st[l].H; p.Wl[l] = e->st[l].W; p.stride[l] = (4 << l) / sf;
  }
  p.out = feat_dev;
  HIP_CHECK(e, hipSetDevice(e->device));
  const int rc = launch_nucleus_pool(p, (hipStream_t)stream);
  if (rc) FAIL(e, rc, "nucleus_pool launch failed");
  return 0;
}

int nuhtc_op_nucleus_pool(nuhtc_engine* e, const float* const maps[4], const int32_t h[4], const int32_t w[4], const int32_t strides[4], int B,
                          const uint32_t* masks, int K, int H, int W, const int32_t* pairs_dev, const int32_t* n_dev, int n_max, float* out, void* stream) {
  if (!e || !maps || !h || !w || !strides || !masks || !pairs_dev || !out) return NUHTC_E_INVALID;
  if (B < 1 || B > 4096 || K < 1 || K > 65536 || H < 1 || W < 1 || (long long)H * W > (1ll << 26) || n_max < 1 || n_max > (1 << 24))
    FAIL(e, NUHTC_E_INVALID, "nucleus_pool op: size out of range (B 1..4096, K 1..65536, H x W at most 2^26, n_max 1..2^24)");
  NucPoolParams p{};
  for (int l = 0; l < 4; ++l) {
    if (!maps[l] || h[l] < 1 || w[l] < 1 || strides[l] < 1 || (H - 1) / strides[l] >= h[l] || (W - 1) / strides[l] >= w[l] || (long long)h[l] * w[l] > (1ll << 26))
      FAIL(e, NUHTC_E_INVALID, "nucleus_pool op: a level map is missing or does not cover the H x W image at its stride");
    p.x[l] = maps[l]; p.Hl[l] = h[l]; p.Wl[l] = w[l]; p.stride[l] = strides[l];
  }
  nucleus_op_route(B, masks, K, H, W, pairs_dev, n_dev, n_max, p.list, p.m);
  p.out = out;
  HIP_CHECK(e, hipSetDevice(e->device));
  hipStream_t s = (hipStream_t)stream;
  return op_finish(e, launch_nucleus_pool(p, s), s, "nucleus_pool launch failed", "nucleus_pool kernel failed");
}

}  // extern "C"
