// Per-nucleus gradient integers (gfx950): under the mask of one list entry, INTEGERS ONLY -- with h the haematoxylin value of a frame
// pixel, (gx2, gy2) twice numpy's np.gradient of h over the H x W frame, q = gx2^2 + gy2^2 and m = isqrt(4 q) (the magnitude in quarter
// grey levels, 0..1442): the pixel count A, the sums S1..S4 of m, m^2, m^3, m^4, the least and greatest m, the number of edge pixels (m
// >= T and q a local maximum along the quantised gradient direction) and the ten-bin histogram of m over [mn, mx]: int64 [18] a nucleus.
// nuhtc_amd/nucgrad.py defines them, restates them in numpy (grad_reference: the device equals it bit for bit) and derives the eight
// Nucleus.Gradient.* columns from them on the host in float64.
//
// One workgroup of 256 threads per nucleus, the shape of nucleus_texture_kernel (nuctex.hip):
//   1. all threads scan the mask for its rectangle and area (block_mask_rect_256, maskbits.h);
//   2. pass 1, one thread per mask word of the rectangle and a set-bit loop over its pixels, the padding bits of a row's last word masked
//      off on every read so that no pixel at x >= W is ever addressed: h is COMPUTED WHERE IT IS NEEDED (haematoxylin_value of
//      haematoxylin.h: three bytes of the tile, the table in LDS), nothing staged, so a rectangle of any size is one pass without bands.
//      q of a pixel reads its four neighbours, each address clamped to the frame (nucgrad_lo / nucgrad_hi of nucgrad_host.h); the edge
//      test reads q of two more pixels, and only where m >= T; a neighbour outside the frame has q = 0 and is not read.  S1..S4 and the
//      edge count go into per-thread int64, the extremes into ints; integer wave reductions (block_prims.h), then across the four waves;
//   3. pass 2 recomputes m of every mask pixel and adds into the wave's OWN copy of the ten bins in LDS (nucgrad_bin);
//   4. the copies are summed and the row leaves with ordinary vector stores.
// Integer adds in any grouping give the same bits: a row is bitwise repeatable across runs and batch splits.
// LDS: the table, 4 x 10 bins, 4 x 5 int64 and 4 x 2 ints of the reductions, the rectangle scan's 20 ints: 1.5 KB a workgroup.
#include "maskbits.h"
#include "nucleus_list.h"
#include "nucgrad_host.h"

namespace {

struct NucGradParams {
  NucleusList list;
  NucleusMasks m;
  NucleusTiles t;
  int64_t* grad;           // [n_max][18]
  int thr;                 // T, quarter grey levels
};

// the frame of one nucleus: h and q of a pixel inside it
struct GradFrame {
  const uint8_t* __restrict__ tile;
  const int* lut;
  long long kb0, kb1, kb2;
  int H, W, pitch;
  // 0 <= x < W, 0 <= y < H
  __device__ __forceinline__ int h(int x, int y) const {
    return haematoxylin_value(tile + ((long long)y * pitch + x) * 3, lut, kb0, kb1, kb2);
  }
  // 0 <= x < W, 0 <= y < H: every read is clamped to the frame
  __device__ __forceinline__ int q(int x, int y, int& gx2, int& gy2) const {
    gx2 = (h(nucgrad_hi(x, W), y) - h(nucgrad_lo(x), y)) * nucgrad_weight(x, W);
    gy2 = (h(x, nucgrad_hi(y, H)) - h(x, nucgrad_lo(y))) * nucgrad_weight(y, H);
    return gx2 * gx2 + gy2 * gy2;
  }
  // any x, y: 0 outside the frame, and nothing read
  __device__ __forceinline__ int q_or_zero(int x, int y) const {
    if (x < 0 || x >= W || y < 0 || y >= H) return 0;
    int gx2, gy2;
    return q(x, y, gx2, gy2);
  }
};

__global__ __launch_bounds__(256) void nucleus_gradient_kernel(NucGradParams p) {
  __shared__ int lut[256];
  __shared__ int bins[4][NUCGRAD_BINS];
  __shared__ long long reds[4][5];
  __shared__ int redm[4][2];
  __shared__ int red[4][5];
  const int d = blockIdx.x, H = p.m.H, wpr = p.m.wpr;
  long long b, r;
  const NucleusEntry at = nucleus_entry(p.list, d, b, r);
  if (at == NUCLEUS_PAST) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int64_t* __restrict__ out = p.grad + (long long)d * NUCGRAD_ROW;
  const auto zero_row = [&] {
    if (tid < NUCGRAD_ROW) out[tid] = 0;
  };
  if (at == NUCLEUS_OUTSIDE) { zero_row(); return; }
  const uint32_t* __restrict__ m = nucleus_mask(p.m, p.list.K, b, r);
  const unsigned last = nucleus_last_word(p.m);

  const MaskRect rc = block_mask_rect_256(m, H, wpr, last, red);
  if (rc.area < 1) { zero_row(); return; }
  lut[tid] = p.t.lut[tid];
  if (tid < 4 * NUCGRAD_BINS) (&bins[0][0])[tid] = 0;
  __syncthreads();
  const GradFrame F{nucleus_tile(p.t, H, b), lut, p.t.kb[0], p.t.kb[1], p.t.kb[2], H, p.m.W, p.t.pitch};
  const int wx0 = rc.x0 >> 5, nw = (rc.x1 >> 5) - wx0 + 1, rows = rc.y1 - rc.y0 + 1;
  const int thr = p.thr;

  // ---- pass 1: the sums, the extremes, the edge pixels
  long long s1 = 0, s2 = 0, s3 = 0, s4 = 0, ne = 0;
  int mn = NUCGRAD_M_MAX, mx = 0;
  for (int i = tid; i < rows * nw; i += 256) {
    const int rr = i / nw, w = wx0 + i - rr * nw, y = rc.y0 + rr;
    unsigned v = m[y * wpr + w];
    if (w == wpr - 1) v &= last;
    for (; v; v &= v - 1) {
      const int x = w * 32 + __ffs(v) - 1;
      int gx2, gy2;
      const int q = F.q(x, y, gx2, gy2);
      const int mag = nucgrad_mag(q);
      const long long m1 = mag, m2 = m1 * m1;
      s1 += m1; s2 += m2; s3 += m2 * m1; s4 += m2 * m2;
      mn = min(mn, mag); mx = max(mx, mag);
      if (mag >= thr) {                                   // thr >= 1: q > 0, the gradient has a direction
        int dx, dy;
        nucgrad_step(nucgrad_sector(gx2, gy2), dx, dy);
        if (q > F.q_or_zero(x + dx, y + dy) && q >= F.q_or_zero(x - dx, y - dy)) ++ne;
      }
    }
  }
  s1 = wave_sum(s1); s2 = wave_sum(s2); s3 = wave_sum(s3); s4 = wave_sum(s4); ne = wave_sum(ne);
  mn = wave_min(mn); mx = wave_max(mx);
  if (lane == 0) {
    reds[wave][0] = s1; reds[wave][1] = s2; reds[wave][2] = s3; reds[wave][3] = s4; reds[wave][4] = ne;
    redm[wave][0] = mn; redm[wave][1] = mx;
  }
  __syncthreads();
  mn = min(min(redm[0][0], redm[1][0]), min(redm[2][0], redm[3][0]));
  mx = max(max(redm[0][1], redm[1][1]), max(redm[2][1], redm[3][1]));

  // ---- pass 2: the histogram over [mn, mx]
  int* __restrict__ mine = bins[wave];
  for (int i = tid; i < rows * nw; i += 256) {
    const int rr = i / nw, w = wx0 + i - rr * nw, y = rc.y0 + rr;
    unsigned v = m[y * wpr + w];
    if (w == wpr - 1) v &= last;
    for (; v; v &= v - 1) {
      const int x = w * 32 + __ffs(v) - 1;
      int gx2, gy2;
      atomicAdd(&mine[nucgrad_bin(nucgrad_mag(F.q(x, y, gx2, gy2)), mn, mx)], 1);
    }
  }
  __syncthreads();
  if (tid < NUCGRAD_ROW) {                              // A, S1..S4, mn, mx, n_edge, hist[10]
    const int k = tid >= NUCGRAD_HIST ? tid - NUCGRAD_HIST : 0, s = tid == 7 ? 4 : (tid >= 1 && tid <= 4 ? tid - 1 : 0);
    long long v;
    if (tid == 0) v = rc.area;
    else if (tid == 5) v = mn;
    else if (tid == 6) v = mx;
    else if (tid < NUCGRAD_HIST) v = reds[0][s] + reds[1][s] + reds[2][s] + reds[3][s];
    else v = (long long)bins[0][k] + bins[1][k] + bins[2][k] + bins[3][k];
    out[tid] = v;
  }
}

int launch_nucleus_gradient(const NucGradParams& p, hipStream_t s) {
  // the bytes of a batch depend on its masks: the profile records the time alone
  ProfScope ps("nucleus_gradient", 0, 0, s);
  hipLaunchKernelGGL(nucleus_gradient_kernel, dim3((unsigned)p.list.n_max), dim3(256), 0, s, p);
  return launched() ? 0 : NUHTC_E_HIP;
}

}  // namespace

extern "C" {

int nuhtc_op_nucleus_gradient(nuhtc_engine* e, const uint8_t* tiles, int channel_mode, const int32_t* lut_dev, const int32_t k[3], int B,
                              const uint32_t* masks, int K, int H, int W, const int32_t* pairs_dev, const int32_t* n_dev, int n_max,
                              int edge_thr, int64_t* grad, void* stream) {
  if (!e || !tiles || !lut_dev || !k || !masks || !pairs_dev || !grad) return NUHTC_E_INVALID;
  const std::string why = nucgrad_args_error(B, K, H, W, W, n_max, channel_mode, edge_thr);
  if (!why.empty()) FAIL(e, NUHTC_E_INVALID, why);
  NucGradParams p{};
  nucleus_op_route(B, masks, K, H, W, pairs_dev, n_dev, n_max, p.list, p.m);
  if (const int rc = nucleus_tiles_args(e, "nucleus_gradient", p.list, p.m, tiles, channel_mode, lut_dev, k, p.t)) return rc;
  p.grad = grad;
  p.thr = edge_thr;
  HIP_CHECK(e, hipSetDevice(e->device));
  hipStream_t s = (hipStream_t)stream;
  return op_finish(e, launch_nucleus_gradient(p, s), s, "nucleus_gradient launch failed", "nucleus_gradient kernel failed");
}

}  // extern "C"
