// Device helpers on bit-packed instance masks, shared by the per-tile mask-NMS of the slide path (roi.hip tile_post_kernel) and the
// evaluation kernels (eval.hip): the popcount of an AND, the IoU verdict on a pair and the greedy pass over sorted candidates; and by
// the per-nucleus kernels (nucfeat.hip, nucmorph.hip): the bounding rectangle of a mask.  The sort and the wave reductions they build
// on are in block_prims.h.
#pragma once
#include "block_prims.h"

// popcount of a & b over the words [w0, w1), by one wave: every lane returns the sum
__device__ __forceinline__ int wave_and_popc(const unsigned* a, const unsigned* b, int w0, int w1, int lane) {
  int cnt = 0;
  for (int wv = w0 + lane; wv < w1; wv += 64) cnt += __popc(a[wv] & b[wv]);
  return wave_sum(cnt);
}

// Bounding rectangle (x0..x1 and y0..y1, both ends inclusive) and area of one bit-packed mask m [H][wpr] by the 256 threads of a
// workgroup (nucfeat.hip, nucmorph.hip): every thread returns the same values, in scalar registers.  `last`: the bits of a row's last
// word that count (~0u where the padding bits are known to be zero).  An empty mask gives area 0, x0 = y0 = INT_MAX, x1 = y1 = -1.
// red: 4 x 5 ints of LDS; one barrier.
struct MaskRect { int x0, y0, x1, y1, area; };
__device__ __forceinline__ MaskRect block_mask_rect_256(const unsigned* __restrict__ m, int H, int wpr, unsigned last, int (*red)[5]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int y0 = 0x7fffffff, y1 = -1, x0 = 0x7fffffff, x1 = -1, area = 0;
  for (int w = tid; w < H * wpr; w += 256) {
    const int y = w / wpr, cw = w - y * wpr;
    const unsigned v = cw == wpr - 1 ? m[w] & last : m[w];
    if (v) {
      y0 = min(y0, y); y1 = max(y1, y);
      x0 = min(x0, cw * 32 + __ffs(v) - 1); x1 = max(x1, cw * 32 + 31 - __clz(v));
      area += __popc(v);
    }
  }
  y0 = wave_min(y0); y1 = wave_max(y1); x0 = wave_min(x0); x1 = wave_max(x1); area = wave_sum(area);
  if (lane == 0) { red[wave][0] = y0; red[wave][1] = y1; red[wave][2] = x0; red[wave][3] = x1; red[wave][4] = area; }
  __syncthreads();
  MaskRect r;
  r.y0 = min(min(red[0][0], red[1][0]), min(red[2][0], red[3][0]));
  r.y1 = max(max(red[0][1], red[1][1]), max(red[2][1], red[3][1]));
  r.x0 = min(min(red[0][2], red[1][2]), min(red[2][2], red[3][2]));
  r.x1 = max(max(red[0][3], red[1][3]), max(red[2][3], red[3][3]));
  r.area = red[0][4] + red[1][4] + red[2][4] + red[3][4];
  // the same in every lane: in scalar registers, so loops over the rectangle are scalar too
  r.y0 = __builtin_amdgcn_readfirstlane(r.y0); r.y1 = __builtin_amdgcn_readfirstlane(r.y1); r.x0 = __builtin_amdgcn_readfirstlane(r.x0);
  r.x1 = __builtin_amdgcn_readfirstlane(r.x1); r.area = __builtin_amdgcn_readfirstlane(r.area);
  return r;
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
