// Tissue mask and tile selection of the whole-slide path (nuhtc_amd/tissue.py on the device): `segmentTissue` up to the binary image that
// contours are found on, and `process_contour`'s grid of point-in-polygon tests.  Everything here is integer arithmetic on bytes and int32
// coordinates, so each step equals its host counterpart byte for byte.  Engine-free entry points in the manner of nuhtc_merge_overlap.
#include <cstring>

#include "common.h"

// ----------------------------------------------------------------------------- mask: saturation -> median -> histogram | threshold -> close
#define TM_TW 64            // output tile of one 256-thread workgroup (8 pixels per thread)
#define TM_TH 32
#define TM_MAXR 7           // mthresh <= 15
#define TM_MAXCLOSE 16

// S of OpenCV's 8-bit RGB2HSV: (v - min) * sdiv[v] + 2^11 >> 12 with sdiv[v] = round(255 * 2^12 / v), sdiv[0] = 0.  The quotient is never
// a tie (2^13 * 255 / v is odd for no v <= 255), so round-half-up in integers is the host's np.rint.
__device__ __forceinline__ int tm_sdiv(int v) { return v ? (2 * (255 << 12) + v) / (2 * v) : 0; }

// One launch: the RGB tile with its halo becomes a saturation tile in LDS (replicated borders = clamped source coordinates), then every
// thread finds the rank k*k/2 value of its windows by a bitwise binary search on the value: eight counting passes, no sort.
__global__ __launch_bounds__(256) void tissue_median_kernel(const uint8_t* __restrict__ img, int H, int W, long long row_stride, int pix_stride, int k,
                                                            uint8_t* __restrict__ sat, uint8_t* __restrict__ med, unsigned long long* __restrict__ hist) {
  __shared__ uint8_t tile[(TM_TH + 2 * TM_MAXR) * (TM_TW + 2 * TM_MAXR)];
  __shared__ int sdiv[256];
  __shared__ int lhist[256];
  const int tid = threadIdx.x, R = k >> 1, pw = TM_TW + 2 * R, ph = TM_TH + 2 * R;
  const int tx0 = blockIdx.x * TM_TW, ty0 = blockIdx.y * TM_TH;
  sdiv[tid] = tm_sdiv(tid);
  lhist[tid] = 0;
  __syncthreads();
  for (int i = tid; i < pw * ph; i += 256) {
    const int ly = i / pw, lx = i - ly * pw;
    const int gy = min(max(ty0 + ly - R, 0), H - 1), gx = min(max(tx0 + lx - R, 0), W - 1);
    const uint8_t* p = img + (long long)gy * row_stride + (long long)gx * pix_stride;
    const int r = p[0], g = p[1], b = p[2];
    const int v = max(r, max(g, b)), lo = min(r, min(g, b));
    tile[i] = (uint8_t)(((v - lo) * sdiv[v] + (1 << 11)) >> 12);
  }
  __syncthreads();
  const int rank = (k * k) >> 1;
  for (int j = 0; j < TM_TW * TM_TH / 256; ++j) {
    const int p = tid + j * 256, oy = p / TM_TW, ox = p - oy * TM_TW;
    const int gy = ty0 + oy, gx = tx0 + ox;
    if (gy >= H || gx >= W) continue;
    const uint8_t* win = tile + oy * pw + ox;
    int m = 0;
    for (int bit = 128; bit; bit >>= 1) {           // the largest t with fewer than rank + 1 window values below it is the median
      const int t = m | bit;
      int below = 0;
      for (int wy = 0; wy < k; ++wy)
        for (int wx = 0; wx < k; ++wx) below += win[wy * pw + wx] < t;
      if (below <= rank) m = t;
    }
    const long long o = (long long)gy * W + gx;
    if (sat) sat[o] = win[R * pw + R];
    med[o] = (uint8_t)m;
    atomicAdd(&lhist[m], 1);
  }
  __syncthreads();
  if (lhist[tid]) atomicAdd(&hist[tid], (unsigned long long)lhist[tid]);
}

// Threshold + rectangular close of side k in one launch.  With a = k / 2 and b = k - k / 2 - 1 the dilation takes the offsets -b .. a and
// the erosion -a .. b, so in tile coordinates both are windows [i, i + k - 1]: the binary tile starts k - 1 before the output tile, the
// dilated one a before it.  Outside the image the binary image reads 0 and the dilated one 255: the border never wins.
__global__ __launch_bounds__(256) void tissue_close_kernel(const uint8_t* __restrict__ med, int H, int W, int thr, int up, int k, uint8_t* __restrict__ out) {
  __shared__ uint8_t bin[(TM_TH + 2 * (TM_MAXCLOSE - 1)) * (TM_TW + 2 * (TM_MAXCLOSE - 1))];
  __shared__ uint8_t dil[(TM_TH + TM_MAXCLOSE - 1) * (TM_TW + TM_MAXCLOSE - 1)];
  const int tid = threadIdx.x, h = k - 1, a = k >> 1;
  const int bw = TM_TW + 2 * h, bh = TM_TH + 2 * h, dw = TM_TW + h, dh = TM_TH + h;
  const int tx0 = blockIdx.x * TM_TW, ty0 = blockIdx.y * TM_TH;
  for (int i = tid; i < bw * bh; i += 256) {
    const int ly = i / bw, lx = i - ly * bw;
    const int gy = ty0 - h + ly, gx = tx0 - h + lx;
    const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
    bin[i] = in && med[(long long)gy * W + gx] > thr ? (uint8_t)up : (uint8_t)0;
  }
  __syncthreads();
  for (int i = tid; i < dw * dh; i += 256) {
    const int ly = i / dw, lx = i - ly * dw;
    const int gy = ty0 - a + ly, gx = tx0 - a + lx;
    int m = 255;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
      m = 0;
      for (int wy = 0; wy < k; ++wy)
        for (int wx = 0; wx < k; ++wx) m = max(m, (int)bin[(ly + wy) * bw + lx + wx]);
    }
    dil[i] = (uint8_t)m;
  }
  __syncthreads();
  for (int j = 0; j < TM_TW * TM_TH / 256; ++j) {
    const int p = tid + j * 256, oy = p / TM_TW, ox = p - oy * TM_TW;
    const int gy = ty0 + oy, gx = tx0 + ox;
    if (gy >= H || gx >= W) continue;
    int m = 255;
    for (int wy = 0; wy < k; ++wy)
      for (int wx = 0; wx < k; ++wx) m = min(m, (int)dil[(oy + wy) * dw + ox + wx]);
    out[(long long)gy * W + gx] = (uint8_t)m;
  }
}

extern "C" int nuhtc_tissue_mask(int device, const uint8_t* img, int H, int W, int64_t row_stride, int pix_stride, int stage, int mthresh, int sthresh,
                                 int sthresh_up, int close, uint8_t* binary, uint8_t* sat, uint8_t* med, int64_t* hist, void* stream) {
  if (stage != NUHTC_TISSUE_ALL && stage != NUHTC_TISSUE_MEDIAN && stage != NUHTC_TISSUE_THRESHOLD) return NUHTC_E_INVALID;
  const bool front = stage != NUHTC_TISSUE_THRESHOLD, back = stage != NUHTC_TISSUE_MEDIAN;
  if (H < 1 || W < 1 || (long long)H * W > 2147483647LL || cdiv(H, TM_TH) > 65535) return NUHTC_E_INVALID;
  if (front && (!img || !hist || pix_stride < 3 || row_stride < (int64_t)W * pix_stride || mthresh < 1 || mthresh > 2 * TM_MAXR + 1 || !(mthresh & 1))) return NUHTC_E_INVALID;
  if (back && (!binary || close < 0 || close > TM_MAXCLOSE || sthresh_up < 0)) return NUHTC_E_INVALID;
  if (stage != NUHTC_TISSUE_ALL && !med) return NUHTC_E_INVALID;
  if (hipSetDevice(device) != hipSuccess) return NUHTC_E_HIP;
  hipStream_t s = (hipStream_t)stream;
  DevScratch tmp;
  if (!med && !(med = tmp.alloc<uint8_t>((size_t)H * W))) return NUHTC_E_HIP;
  const dim3 grid(cdiv(W, TM_TW), cdiv(H, TM_TH));
  if (front) {
    if (hipMemsetAsync(hist, 0, 256 * sizeof(int64_t), s) != hipSuccess) return NUHTC_E_HIP;
    hipLaunchKernelGGL(tissue_median_kernel, grid, dim3(256), 0, s, img, H, W, (long long)row_stride, pix_stride, mthresh, sat, med,
                       reinterpret_cast<unsigned long long*>(hist));
  }
  if (back)
    hipLaunchKernelGGL(tissue_close_kernel, grid, dim3(256), 0, s, med, H, W, sthresh, sthresh_up > 255 ? 255 : sthresh_up, close > 0 ? close : 1, binary);
  if (!launched() || hipStreamSynchronize(s) != hipSuccess) return NUHTC_E_HIP;
  return 0;
}

// ----------------------------------------------------------------------------- point in polygon
#define PIP_CHUNK 1024      // vertices staged through LDS at a time (+ the one that closes the chunk's last edge)

// cv2.pointPolygonTest(..., False) of the calling thread's point against a closed contour, vertices staged through `lds` by the whole
// workgroup (every thread of it must call, `active` or not).  Per edge (x1, y1) -> (x2, y2) one 64-bit cross product decides both
// questions: zero inside the edge's box = on the edge; for an edge with exactly one end at y <= py its sign against the sign of
// dy = y2 - y1 is the host's float test px < x1 + (py - y1) * (x2 - x1) / dy, exactly.  Returns +1 / 0 / -1.
__device__ int pip_test(const int32_t* __restrict__ verts, long long n, int px, int py, int2* lds) {
  bool on = false;
  int cross_n = 0;
  for (long long c0 = 0; c0 < n; c0 += PIP_CHUNK) {
    const int ne = (int)min((long long)PIP_CHUNK, n - c0);          // edges of this chunk; its vertices are ne + 1
    __syncthreads();
    for (int i = threadIdx.x; i <= ne; i += blockDim.x) {
      long long v = c0 + i;
      if (v >= n) v -= n;
      lds[i] = make_int2(verts[2 * v], verts[2 * v + 1]);
    }
    __syncthreads();
    int2 p1 = lds[0];
    for (int i = 1; i <= ne; ++i) {
      const int2 p2 = lds[i];
      const int dx = p2.x - p1.x, dy = p2.y - p1.y;
      const long long cross = (long long)dx * (py - p1.y) - (long long)dy * (px - p1.x);
      on |= cross == 0 && min(p1.x, p2.x) <= px && px <= max(p1.x, p2.x) && min(p1.y, p2.y) <= py && py <= max(p1.y, p2.y);
      cross_n += ((p1.y <= py) != (p2.y <= py)) && (dy > 0 ? cross > 0 : cross < 0);
      p1 = p2;
    }
  }
  return on ? 0 : (cross_n & 1) ? 1 : -1;
}

__global__ __launch_bounds__(256) void pip_points_kernel(const int32_t* __restrict__ verts, long long n_vert, const int32_t* __restrict__ pts, long long n,
                                                         int8_t* __restrict__ out) {
  __shared__ int2 lds[PIP_CHUNK + 1];
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = i < n;
  const int r = pip_test(verts, n_vert, active ? pts[2 * i] : 0, active ? pts[2 * i + 1] : 0, lds);
  if (active) out[i] = (int8_t)r;
}

struct GridArgs {
  int start_x, start_y, ny, step;
  long long ncand;
  int off[8];               // (dx, dy) of the slots of this launch
  int n_off, group;         // slots used / threads per candidate (1, 2 or 4: n_off rounded up)
  int mode;                 // 0: keep = any slot >= 0; 1: keep = all slots >= 0; 2 (one slot, a hole): keep = 0 where the slot is > 0
};

// One thread per (candidate, slot); the slots of a candidate are neighbouring lanes and vote across them.
__global__ __launch_bounds__(256) void pip_grid_kernel(GridArgs g, const int32_t* __restrict__ verts, long long n_vert, uint8_t* __restrict__ keep) {
  __shared__ int2 lds[PIP_CHUNK + 1];
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long cand = t / g.group;
  const int slot = (int)(t - cand * g.group);
  const bool active = cand < g.ncand && slot < g.n_off;
  int px = 0, py = 0;
  if (active) {
    const long long ix = cand / g.ny, iy = cand - ix * g.ny;
    px = (int)(g.start_x + ix * g.step + g.off[2 * slot]);
    py = (int)(g.start_y + iy * g.step + g.off[2 * slot + 1]);
  }
  const int r = pip_test(verts, n_vert, px, py, lds);
  if (g.mode == 2) {
    if (active && r > 0) keep[cand] = 0;
    return;
  }
  // a slot past n_off is neutral: it fails an 'any' vote and passes an 'all' vote
  int vote = active ? r >= 0 : g.mode == 1;
  for (int d = 1; d < g.group; d <<= 1) {
    const int other = __shfl_xor(vote, d);
    vote = g.mode == 1 ? (vote & other) : (vote | other);
  }
  if (active && slot == 0) keep[cand] = (uint8_t)vote;
}

extern "C" int nuhtc_points_polygon_test(int device, const int32_t* contour, int64_t n_vert, const int32_t* pts, int64_t n, int8_t* out, void* stream) {
  if (n_vert < 1 || n_vert > (1LL << 40) || n < 0 || n > (1LL << 38) || !contour || (n > 0 && (!pts || !out))) return NUHTC_E_INVALID;
  if (n == 0) return 0;
  if (hipSetDevice(device) != hipSuccess) return NUHTC_E_HIP;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(pip_points_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, contour, (long long)n_vert, pts, (long long)n, out);
  if (!launched() || hipStreamSynchronize(s) != hipSuccess) return NUHTC_E_HIP;
  return 0;
}

extern "C" int nuhtc_grid_in_contour(int device, int start_x, int start_y, int nx, int ny, int step, const int32_t* offsets, int n_off, int require_all,
                                     const int32_t* contour, int64_t n_vert, const int32_t* holes, int64_t n_pool, const int64_t* hole_off, int n_holes,
                                     int hole_dx, int hole_dy, uint8_t* keep, void* stream) {
  const long long LIM = 1LL << 30;
  if (nx < 0 || ny < 0 || step < 1 || n_off < 1 || n_off > 4 || !offsets || n_vert < 0 || n_vert > (1LL << 40) || (n_vert > 0 && !contour) ||
      (n_vert == 0 && contour) || n_holes < 0 || n_pool < 0 || (n_holes > 0 && (!holes || !hole_off)))
    return NUHTC_E_INVALID;
  const long long ncand = (long long)nx * ny;
  if (ncand > 2147483647LL || (ncand > 0 && !keep)) return NUHTC_E_INVALID;
  // every point a kernel forms stays within +-2^30: the grid's corners moved by every offset
  const long long x_hi = start_x + (long long)(nx > 0 ? nx - 1 : 0) * step, y_hi = start_y + (long long)(ny > 0 ? ny - 1 : 0) * step;
  for (int j = 0; j <= n_off; ++j) {
    const long long dx = j < n_off ? offsets[2 * j] : hole_dx, dy = j < n_off ? offsets[2 * j + 1] : hole_dy;
    if (start_x + dx < -LIM || x_hi + dx > LIM || start_y + dy < -LIM || y_hi + dy > LIM) return NUHTC_E_INVALID;
  }
  for (int h = 0; h < n_holes; ++h)
    if ((h == 0 && hole_off[0] != 0) || hole_off[h + 1] <= hole_off[h] || hole_off[h + 1] > n_pool) return NUHTC_E_INVALID;
  if (ncand == 0) return 0;
  if (hipSetDevice(device) != hipSuccess) return NUHTC_E_HIP;
  hipStream_t s = (hipStream_t)stream;
  GridArgs g;
  memset(&g, 0, sizeof(g));
  g.start_x = start_x; g.start_y = start_y; g.ny = ny; g.step = step; g.ncand = ncand;
  if (n_vert == 0) {
    if (hipMemsetAsync(keep, 1, (size_t)ncand, s) != hipSuccess) return NUHTC_E_HIP;
  } else {
    for (int j = 0; j < 2 * n_off; ++j) g.off[j] = offsets[j];
    g.n_off = n_off; g.group = n_off == 1 ? 1 : n_off == 2 ? 2 : 4; g.mode = require_all ? 1 : 0;
    hipLaunchKernelGGL(pip_grid_kernel, dim3((unsigned)((ncand * g.group + 255) / 256)), dim3(256), 0, s, g, contour, (long long)n_vert, keep);
  }
  g.off[0] = hole_dx; g.off[1] = hole_dy; g.n_off = 1; g.group = 1; g.mode = 2;
  for (int h = 0; h < n_holes; ++h)            // in stream order after the contour's launch: a hole only clears
    hipLaunchKernelGGL(pip_grid_kernel, dim3((unsigned)((ncand + 255) / 256)), dim3(256), 0, s, g, holes + 2 * hole_off[h],
                       (long long)(hole_off[h + 1] - hole_off[h]), keep);
  if (!launched() || hipStreamSynchronize(s) != hipSuccess) return NUHTC_E_HIP;
  return 0;
}
