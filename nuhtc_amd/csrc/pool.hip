// Tile embeddings (gfx950): the per-channel mean of the four FPN maps over their whole padded grid
// (tools/extract_features_nuhtc.py:81-85 of the reference: `features_lvl[l].mean(dim=(2, 3))`, concatenated over l = 0..3).
//
// Deterministic by construction -- no float atomics: the same tile gives the same bits whatever batch it sits in and whichever
// call computed it.  Pass 1 (fpn_mean_pool_kernel, ONE launch for the four levels): a workgroup sums POOL_CHUNK pixels of one
// (tile, level) in fp64 and writes its 64 partial sums to a fixed slot of the slab; pass 2 (fpn_mean_pool_final_kernel) adds a
// (tile, level)'s partials in chunk order and divides by H*W once.  fp64 accumulation makes the result the correctly rounded mean
// up to one fp32 rounding, so it also equals a float64 mean of the same map to ~1e-7 relative.
#include "common.h"

__global__ __launch_bounds__(256) void fpn_mean_pool_kernel(PoolLevels p, double* __restrict__ slab) {
  const int nc = p.choff[4];
  const int b = blockIdx.y, k = blockIdx.x;
  int l = 0;
  while (l < 3 && k >= p.choff[l + 1]) ++l;
  const int hw = p.hw[l];
  const int p0 = (k - p.choff[l]) * POOL_CHUNK;
  const float4* __restrict__ src = reinterpret_cast<const float4*>(p.x[l]) + (long long)b * hw * 16;
  // 16 lanes per pixel (one float4 of the 64 channels each), 16 pixels per pass of the workgroup: a wave reads 1 KB contiguous
  const int t = threadIdx.x, c4 = t & 15;
  double ax = 0.0, ay = 0.0, az = 0.0, aw = 0.0;
#pragma unroll 4
  for (int i = t >> 4; i < POOL_CHUNK; i += 16) {
    const int pix = p0 + i;
    if (pix < hw) {
      const float4 v = src[(long long)pix * 16 + c4];
      ax += v.x; ay += v.y; az += v.z; aw += v.w;
    }
  }
  // lanes L, L^16, L^32, L^48 of a wave hold the same four channels
#pragma unroll
  for (int m = 16; m <= 32; m <<= 1) {
    ax += __shfl_xor(ax, m); ay += __shfl_xor(ay, m); az += __shfl_xor(az, m); aw += __shfl_xor(aw, m);
  }
  __shared__ double red[4][64];
  const int wave = t >> 6, lane = t & 63;
  if (lane < 16) {
    red[wave][4 * c4 + 0] = ax; red[wave][4 * c4 + 1] = ay; red[wave][4 * c4 + 2] = az; red[wave][4 * c4 + 3] = aw;
  }
  __syncthreads();
  if (t < 64) slab[((long long)b * nc + k) * 64 + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
}

__global__ __launch_bounds__(256) void fpn_mean_pool_final_kernel(PoolLevels p, const double* __restrict__ slab, float* __restrict__ feat) {
  const int nc = p.choff[4];
  const int b = blockIdx.x, l = threadIdx.x >> 6, c = threadIdx.x & 63;
  double s = 0.0;
  for (int k = p.choff[l]; k < p.choff[l + 1]; ++k) s += slab[((long long)b * nc + k) * 64 + c];
  feat[(long long)b * 256 + threadIdx.x] = (float)(s / (double)p.hw[l]);
}

int pool_chunks(const int hw[4], int choff[5]) {
  choff[0] = 0;
  for (int l = 0; l < 4; ++l) {
    if (hw[l] < 1) return NUHTC_E_INVALID;
    choff[l + 1] = choff[l] + cdiv(hw[l], POOL_CHUNK);
  }
  return 0;
}

int launch_fpn_mean_pool(const PoolLevels& p, int B, double* slab, float* feat, hipStream_t s) {
  if (B < 1 || p.choff[4] < 4) return NUHTC_E_INVALID;
  long long px = 0;
  for (int l = 0; l < 4; ++l) px += p.hw[l];
  {
    ProfScope ps("fpn_mean_pool", (double)B * px * 64, (double)B * px * 64 * 4 + (double)B * p.choff[4] * 64 * 8, s);
    hipLaunchKernelGGL(fpn_mean_pool_kernel, dim3((unsigned)p.choff[4], (unsigned)B), dim3(256), 0, s, p, slab);
    if (!launched()) return NUHTC_E_HIP;
  }
  ProfScope ps("fpn_mean_pool_final", (double)B * p.choff[4] * 64, (double)B * p.choff[4] * 64 * 8 + (double)B * 256 * 4, s);
  hipLaunchKernelGGL(fpn_mean_pool_final_kernel, dim3((unsigned)B), dim3(256), 0, s, p, (const double*)slab, feat);
  return launched() ? 0 : NUHTC_E_HIP;
}
