// Device helpers on bit-packed instance masks, shared by the per-tile mask-NMS of the slide path (roi.hip tile_post_kernel) and the
// evaluation kernels (eval.hip): the popcount of an AND, the IoU verdict on a pair and the greedy pass over sorted candidates.  The
// sort and the wave reductions they build on are in block_prims.h.
#pragma once
#include "block_prims.h"

// popcount of a & b over the words [w0, w1), by one wave: every lane returns the sum
__device__ __forceinline__ int wave_and_popc(const unsigned* a, const unsigned* b, int w0, int w1, int lane) {
  int cnt = 0;
  for (int wv = w0 + lane; wv < w1; wv += 64) cnt += __popc(a[wv] & b[wv]);
  return wave_sum(cnt);
}

// does a pair of masks with `inter` common pixels overlap by more than thr?  IoU in float64 on the integer counts, as numpy decides it.
// The two callers treat an empty union differently and each keeps its form: UNION_CLAMPED divides by max(union, 1) (stats_utils.py
// mask_nms, eval_select_kernel), the other form never suppresses on an empty union (tile_post_kernel).  They differ only for a
// negative threshold on two empty masks.
template <bool UNION_CLAMPED>
__device__ __forceinline__ bool mask_inter_over(int inter, int area_a, int area_c, double thr) {
  const int uni = area_a + area_c - inter;
  if (UNION_CLAMPED) return (double)inter / (double)max(uni, 1) > thr;
  return uni > 0 && (double)inter / (double)uni > thr;
}
// the same from the masks, ANDed over the words [w0, w1) by one wave (all its lanes call, all get the verdict)
template <bool UNION_CLAMPED>
__device__ __forceinline__ bool mask_pair_over(const unsigned* mi, const unsigned* mj, int w0, int w1, int area_a, int area_c, double thr, int lane) {
  return mask_inter_over<UNION_CLAMPED>(wave_and_popc(mi, mj, w0, w1, lane), area_a, area_c, thr);
}

// Greedy suppression over m candidates in visiting order by the NT threads of a workgroup: sup[c] != 0 = removed.  For a kept candidate
// a the pairs (a, c > a) are independent of each other, so every wave takes its own c and there is one barrier per kept candidate.
// on_keep(a) runs in every thread and returns what the pair tests of a share; over(kept, c) is called by whole waves and returns
// whether a suppresses c (its cheap pre-test on hulls or bounding boxes included).  over() is the whole verdict and not a word range
// for the pass to AND because the two callers treat a failed pre-test differently: tile_post_kernel skips the pair, eval_select_kernel
// still judges it on 0 common pixels (which suppresses under a negative threshold, as numpy does).  In tile_post_kernel this form costs
// 2 VGPRs (60 -> 62) against the loop written in place; its 4 waves per SIMD are set by 1024 threads and 94 KiB of LDS, so it stays.
template <int NT, typename OnKeep, typename Over>
__device__ __forceinline__ void greedy_mask_pass(int m, unsigned char* sup, OnKeep on_keep, Over over) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int a = 0; a < m; ++a) {
    if (sup[a]) continue;   // uniform: sup[] only changes between barriers
    const auto kept = on_keep(a);
    for (int c = a + 1 + wave; c < m; c += NT / 64) {
      if (sup[c]) continue;
      const bool hit = over(kept, c);
      if (lane == 0 && hit) sup[c] = 1;
    }
    __syncthreads();
  }
}
