// Device helpers on bit-packed instance masks and LDS sort keys, shared by the per-tile mask-NMS of the slide path (roi.hip
// tile_post_kernel) and the evaluation kernels (eval.hip).
#pragma once
#include <hip/hip_runtime.h>

// popcount of a & b over the words [w0, w1), by one wave: every lane returns the sum
__device__ __forceinline__ int wave_and_popc(const unsigned* a, const unsigned* b, int w0, int w1, int lane) {
  int cnt = 0;
  for (int wv = w0 + lane; wv < w1; wv += 64) cnt += __popc(a[wv] & b[wv]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  return cnt;
}

// ascending bitonic sort of key[0 .. npad) in LDS (npad a power of two >= 2) by the NT threads of a workgroup; the keys must have
// been written before a barrier, and the sort ends with one
template <int NT>
__device__ __forceinline__ void bitonic_sort_u64(unsigned long long* key, int npad, int tid) {
  for (int k = 2; k <= npad; k <<= 1)
    for (int jj = k >> 1; jj > 0; jj >>= 1) {
      for (int t = tid; t < (npad >> 1); t += NT) {
        int lo = ((t / jj) * (jj << 1)) + (t % jj), hi = lo + jj;
        bool asc = ((lo & k) == 0);
        unsigned long long a = key[lo], c = key[hi];
        if ((a > c) == asc) { key[lo] = c; key[hi] = a; }
      }
      __syncthreads();
    }
}
