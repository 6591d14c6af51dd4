// COCO run-length masks on the device (gfx950, wave64): the compressed `counts` string of cocoapi common/maskApi.c rleEncode + rleToString and
// the box of rleToBbox, for n bit-packed H x W masks -- what nuhtc_amd/cocomask.py encode / to_bbox give, byte for byte (integer arithmetic
// only).  Engine-free entry point in the manner of nuhtc_merge_overlap / nuhtc_tissue_mask.
//
// One 1024-thread workgroup per mask, three launches per call:
//   rle_mask_kernel<false>  the string's length and the box of every mask
//   rle_offsets_kernel      exclusive scan of the lengths in mask order -> byte offset of every string in the pool (no atomics: placement
//                           is a function of the lengths alone)
//   rle_mask_kernel<true>   the same walk again, now writing the characters at the mask's offset
// The walk is cheap enough to run twice: a mask costs its occupied rectangle, not its frame.  Steps of a workgroup:
//   1. every thread looks at its share of the frame's words once: the occupied column range [c0, c1] and row range [r0, r1] (most of a
//      frame is empty and costs nothing after this);
//   2. a thread per column c0 .. c1 + 1 walks the rows r0 .. r1 + 1 of its column and finds the transitions against the previous pixel in
//      column-major order (index p = x * H + y; for row 0 that is the previous column's last row), counts them, and after a block scan of
//      the per-column counts writes their positions p into LDS, in order;
//   3. a thread per count forms the count (difference of neighbouring positions), its delta against the count two places back (from the
//      fourth on), the number of characters of that value and -- first pass -- its share of rleToBbox; a second block scan gives the
//      character's place in the string.
#include "block_prims.h"
#include "common.h"

#define RLE_NT 1024
#define RLE_LDS_RUNS 15360          // positions that fit the 64 KB of LDS a workgroup may take beside the reduction scratch

// min / max of four values over the workgroup: v[0], v[1] minima, v[2], v[3] maxima; every thread gets the results
__device__ __forceinline__ void rle_block_minmax(int* v, int (*red)[16]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  v[0] = wave_min(v[0]); v[1] = wave_min(v[1]); v[2] = wave_max(v[2]); v[3] = wave_max(v[3]);
  if (lane == 0) for (int k = 0; k < 4; ++k) red[k][wave] = v[k];
  __syncthreads();
  for (int w = 0; w < RLE_NT / 64; ++w) {
    v[0] = min(v[0], red[0][w]); v[1] = min(v[1], red[1][w]); v[2] = max(v[2], red[2][w]); v[3] = max(v[3], red[3][w]);
  }
  __syncthreads();
}

__device__ __forceinline__ int rle_pixel(const uint32_t* m, int wpr, int y, int x) { return (m[(size_t)y * wpr + (x >> 5)] >> (x & 31)) & 1; }

// transitions of column x over the rows r0 .. re (every row outside r0 .. r1 is clear; re = r1 + 1 where that row exists), in order; EMIT: their positions go to
// pos[k], k counting on from `k` (dropped past `cap`).  Returns the number of transitions.
template <bool EMIT>
__device__ __forceinline__ int rle_walk_column(const uint32_t* m, int wpr, int H, int x, int r0, int re, bool bottom_row_used, int* pos, int k, int cap) {
  int cnt = 0;
  // the pixel before (0, x) in column-major order is (H - 1, x - 1); before (0, 0) the run of zeros starts
  int prev = (x > 0 && bottom_row_used) ? rle_pixel(m, wpr, H - 1, x - 1) : 0;
  if (r0 > 0) {                       // row 0 is clear: a 1-run that came down the previous column ends at the top of this one
    if (prev) {
      if (EMIT && k + cnt < cap) pos[k + cnt] = x * H;
      ++cnt;
    }
    prev = 0;                         // row r0 - 1 is clear as well
  }
  for (int y = r0; y <= re; ++y) {
    const int cur = rle_pixel(m, wpr, y, x);
    if (cur != prev) {
      if (EMIT && k + cnt < cap) pos[k + cnt] = x * H + y;
      ++cnt;
    }
    prev = cur;
  }
  return cnt;
}

template <bool WRITE>
__global__ __launch_bounds__(RLE_NT) void rle_mask_kernel(const uint32_t* __restrict__ words, const int32_t* __restrict__ n_dev, int n_max, int H, int W,
                                                          int run_cap, int32_t* __restrict__ len, const int32_t* __restrict__ off,
                                                          uint8_t* __restrict__ bytes, long long pool_cap, int32_t* __restrict__ bbox) {
  extern __shared__ int pos[];        // [run_cap] positions of the transitions, ascending
  __shared__ int red[4][16];
  __shared__ int scan_lds[17];
  const int i = blockIdx.x, tid = threadIdx.x;
  const int n = n_dev ? min(max(*n_dev, 0), n_max) : n_max;
  if (i >= n) return;
  long long o = 0;
  if (WRITE) {                        // (uniform over the workgroup) nothing to write: given up on, or past the pool
    const int L = len[i];
    o = off[i];
    if (L < 0 || o + L > pool_cap) return;
  }
  const int wpr = W >> 5, nw = H * wpr, N = H * W;
  const uint32_t* m = words + (size_t)i * nw;

  // ---- 1. occupied rectangle
  int v[4] = {W, H, -1, -1};          // c0, r0, c1, r1
  for (int w = tid; w < nw; w += RLE_NT) {
    const uint32_t bits = m[w];
    if (bits) {
      const int y = w / wpr, xb = (w - y * wpr) << 5;
      v[0] = min(v[0], xb + __ffs(bits) - 1);
      v[2] = max(v[2], xb + 31 - __clz((int)bits));
      v[1] = min(v[1], y);
      v[3] = max(v[3], y);
    }
  }
  rle_block_minmax(v, red);
  const int c0 = v[0], r0 = v[1], c1 = v[2], r1 = v[3];

  // ---- 2. transitions, a thread per column; the column after the last occupied one closes a run that reaches the bottom of c1
  int T = 0;
  if (c1 >= 0) {
    const int ce = min(c1 + 1, W - 1), re = min(r1 + 1, H - 1), ncols = ce - c0 + 1;
    const bool bottom = r1 == H - 1;
    for (int cb = 0; cb < ncols; cb += RLE_NT) {
      const bool active = cb + tid < ncols;
      const int x = c0 + cb + tid;
      const int cnt = active ? rle_walk_column<false>(m, wpr, H, x, r0, re, bottom, pos, 0, 0) : 0;
      int total;
      const int ex = block_exscan_1024(cnt, scan_lds, &total);
      if (active && cnt && T + ex < run_cap) rle_walk_column<true>(m, wpr, H, x, r0, re, bottom, pos, T + ex, run_cap);
      T += total;
    }
  }
  __syncthreads();
  const int ncounts = T + 1;          // T transitions cut the frame into T + 1 runs (the first one, of zeros, may be empty)
  if (ncounts > run_cap) {            // more runs than positions: the caller encodes this one (only the first pass gets here)
    if (!WRITE && tid == 0) {
      len[i] = -1;
      for (int k = 0; k < 4; ++k) bbox[4 * i + k] = 0;
    }
    return;
  }

  // ---- 3. counts -> deltas -> characters.  e(k): end of run k = start of run k + 1
  auto e = [&](int k) { return k < 0 ? 0 : k < T ? pos[k] : N; };
  const int mb = ncounts & ~1;        // rleToBbox looks at whole (0-run, 1-run) pairs
  int bb[4] = {W, H, 0, 0};           // xs, ys, xe, ye
  int slen = 0;
  for (int kb = 0; kb < ncounts; kb += RLE_NT) {
    const int k = kb + tid;
    const bool active = k < ncounts;
    int val = 0, nch = 0;
    if (active) {
      const int e1 = e(k - 1), e0 = e(k);
      val = e0 - e1;
      if (k > 2) val -= e(k - 2) - e(k - 3);
      int x = val;
      bool more;
      do {                            // rleToString: 5 bits per character, sign-aware stop
        const int c = x & 0x1f;
        x >>= 5;
        more = (c & 0x10) ? x != -1 : x != 0;
        ++nch;
      } while (more);
      if (!WRITE && k < mb) {
        const int t = e0 - (k & 1);   // even k: first pixel of a 1-run; odd k: its last pixel
        const int bx = t / H, by = t - bx * H;
        bb[0] = min(bb[0], bx); bb[2] = max(bb[2], bx); bb[1] = min(bb[1], by); bb[3] = max(bb[3], by);
        if ((k & 1) && e1 / H < bx) { bb[1] = 0; bb[3] = H - 1; }      // a 1-run that ends in a later column than it began in
      }
    }
    int total;
    const int ex = block_exscan_1024(nch, scan_lds, &total);
    if (WRITE && active) {
      uint8_t* dst = bytes + o + slen + ex;
      int x = val;
      bool more;
      do {
        int c = x & 0x1f;
        x >>= 5;
        more = (c & 0x10) ? x != -1 : x != 0;
        if (more) c |= 0x20;
        *dst++ = (uint8_t)(c + 48);
      } while (more);
    }
    slen += total;
  }
  if (!WRITE) {
    rle_block_minmax(bb, red);
    if (tid == 0) {
      len[i] = slen;
      const bool any = mb > 0;
      bbox[4 * i + 0] = any ? bb[0] : 0;
      bbox[4 * i + 1] = any ? bb[1] : 0;
      bbox[4 * i + 2] = any ? bb[2] - bb[0] + 1 : 0;
      bbox[4 * i + 3] = any ? bb[3] - bb[1] + 1 : 0;
    }
  }
}

// off[k] = sum of max(len[j], 0) over j < k, k = 0 .. n
__global__ __launch_bounds__(RLE_NT) void rle_offsets_kernel(const int32_t* __restrict__ len, const int32_t* __restrict__ n_dev, int n_max,
                                                             int32_t* __restrict__ off) {
  __shared__ int scan_lds[17];
  const int tid = threadIdx.x;
  const int n = n_dev ? min(max(*n_dev, 0), n_max) : n_max;
  int base = 0;
  for (int b = 0; b < n; b += RLE_NT) {
    const int k = b + tid;
    const int v = k < n ? max(len[k], 0) : 0;
    int total;
    const int ex = block_exscan_1024(v, scan_lds, &total);
    if (k < n) off[k] = base + ex;
    base += total;
  }
  if (tid == 0) off[n] = base;
}

extern "C" int nuhtc_rle_encode(int device, const uint32_t* words_dev, const int32_t* n_dev, int n_max, int H, int W, int run_cap,
                                int32_t* len_dev, int32_t* off_dev, uint8_t* bytes_dev, int64_t pool_cap, int32_t* bbox_dev, void* stream) {
  if (H < 1 || W < 1 || (W & 31) || (long long)H * W > (1LL << 20) || run_cap < 1 || n_max < 0 || pool_cap < 0 || !off_dev ||
      (n_max > 0 && (!words_dev || !len_dev || !bbox_dev)) || (pool_cap > 0 && !bytes_dev))
    return NUHTC_E_INVALID;
  const int cap = min(min(run_cap, H * W + 1), RLE_LDS_RUNS);          // a frame has at most H * W + 1 counts
  if ((long long)n_max * cap * 5 > 2147483647LL) return NUHTC_E_INVALID;      // the offsets are int32 (a count is at most 5 characters)
  if (hipSetDevice(device) != hipSuccess) return NUHTC_E_HIP;
  hipStream_t s = (hipStream_t)stream;
  const size_t lds = (size_t)cap * sizeof(int);
  if (n_max > 0)
    hipLaunchKernelGGL(rle_mask_kernel<false>, dim3(n_max), dim3(RLE_NT), lds, s, words_dev, n_dev, n_max, H, W, cap, len_dev, (const int32_t*)off_dev,
                       bytes_dev, (long long)pool_cap, bbox_dev);
  hipLaunchKernelGGL(rle_offsets_kernel, dim3(1), dim3(RLE_NT), 0, s, (const int32_t*)len_dev, n_dev, n_max, off_dev);
  if (n_max > 0)
    hipLaunchKernelGGL(rle_mask_kernel<true>, dim3(n_max), dim3(RLE_NT), lds, s, words_dev, n_dev, n_max, H, W, cap, len_dev, (const int32_t*)off_dev,
                       bytes_dev, (long long)pool_cap, bbox_dev);
  return launched() ? 0 : NUHTC_E_HIP;
}
