// Device building blocks shared by the kernels of several translation units (gfx950, wave64), one copy of each: full-wave reductions,
// the descending-score sort keys, the LDS bitonic sort, next_pow2 and the block-wide exclusive scan.  Header-only; every function is
// __forceinline__ and keeps one fixed operation order, so a kernel computes the same bits whichever file it lives in.
#pragma once
#include <hip/hip_runtime.h>

// ---- reductions over all 64 lanes of a wave: every lane returns the result.  The butterfly runs over xor offsets 32, 16, .. 1 in that
// order (part of the result of a float sum).  Reductions over part of a wave stay with the register layout they belong to.
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// ---- the high word of a sort key whose ASCENDING order visits the best score first.  A call site picks one by the scores it can see:
// desc_key_nonneg: the inverted raw bits.  Only for scores >= +0 (probabilities: sigmoid / softmax outputs), where the unsigned order
//                  of the bits is the float order; a negative score (or -0) would sort in front of every positive one.
// desc_key_total : the inverted order-preserving map of all floats (negative ones have their bits flipped, the others get the sign
//                  bit), for scores a caller hands in unchecked.
// The two give different keys for the same score: moving a site from one to the other changes what it computes.
__device__ __forceinline__ unsigned desc_key_nonneg(float s) { return ~__float_as_uint(s); }
__device__ __forceinline__ unsigned desc_key_total(float s) {
  const unsigned u = __float_as_uint(s);
  return ~((u & 0x80000000u) ? ~u : (u | 0x80000000u));
}

__host__ __device__ __forceinline__ int next_pow2(int v) { int p = 1; while (p < v) p <<= 1; return p; }

// ascending bitonic sort of key[0 .. npad) in LDS (npad a power of two >= 2) by the NT threads of a workgroup; the keys must have
// been written before a barrier, and the sort ends with one
template <int NT>
__device__ __forceinline__ void bitonic_sort_u64(unsigned long long* key, int npad, int tid) {
  for (int k = 2; k <= npad; k <<= 1)
    for (int jj = k >> 1; jj > 0; jj >>= 1) {
      for (int t = tid; t < (npad >> 1); t += NT) {
        int lo = ((t / jj) * (jj << 1)) + (t % jj), hi = lo + jj;   // t -> pair (lo, lo + jj)
        bool asc = ((lo & k) == 0);
        unsigned long long a = key[lo], c = key[hi];
        if ((a > c) == asc) { key[lo] = c; key[hi] = a; }
      }
      __syncthreads();
    }
}

// block-wide exclusive scan of one int per thread (blockDim.x == NT, a multiple of 64 up to 1024), returns exclusive prefix, *total gets
// the sum; lds: NT / 64 + 1 ints
template <int NT>
__device__ __forceinline__ int block_exscan(int v, int* lds, int* total) {
  constexpr int NW = NT / 64;
  static_assert(NT % 64 == 0 && NW >= 1 && NW <= 16, "whole waves, and their sums scanned by one");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { int t = __shfl_up(incl, o); if (lane >= o) incl += t; }
  if (lane == 63) lds[wave] = incl;
  __syncthreads();
  if (wave == 0) {
    int w = lane < NW ? lds[lane] : 0;
    int wi = w;
#pragma unroll
    for (int o = 1; o < NW; o <<= 1) { int t = __shfl_up(wi, o); if (lane >= o) wi += t; }
    if (lane < NW) lds[lane] = wi - w;
    if (lane == NW - 1) lds[NW] = wi;
  }
  __syncthreads();
  int res = lds[wave] + incl - v;
  *total = lds[NW];
  __syncthreads();
  return res;
}
// blockDim.x == 1024; lds16: 17 ints
__device__ __forceinline__ int block_exscan_1024(int v, int* lds16, int* total) { return block_exscan<1024>(v, lds16, total); }
