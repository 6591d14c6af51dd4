// Per-nucleus morphometry and haematoxylin intensity (gfx950): under the final mask of one kept detection, INTEGERS ONLY -- the area,
// the bounding rectangle, the sums of x, y, x^2, y^2 and xy, the crack length, the three perimeter classes of
// skimage.measure.perimeter(neighbourhood=4), twice the area of the convex hull of the pixel corners and the 256-bin histogram of a
// fixed-point haematoxylin value of the tile's pixels.  nuhtc_amd/nucmorph.py defines every one of them, restates them in numpy
// (morph_reference: the device equals it bit for bit) and derives every named floating-point feature from them on the host in float64.
//
// One workgroup of 256 threads per nucleus, the shape of nucleus_pool_kernel (nucfeat.hip):
//   1. all threads scan the mask for its rectangle and area (block_mask_rect_256, maskbits.h);
//   2. the rectangle's rows are staged in LDS in bands: the mask words of the rows [yb - 2, ye + 2) with one zero word on either side
//      (a band holds MW words: of a rectangle 8 words wide 204 staged rows, i.e. up to 200 rows of the rectangle, and anything taller
//      takes a further band -- a nucleus is one band, the full 256-px frame two; a full 1024-px frame takes 19 bands of 56 rows), a
//      pixel outside the frame reading as 0;
//   3. one thread per mask word: the border word B = M & ~(up & down & left & right) of the rows [yb - 1, ye + 1), the neighbours'
//      bits carried across the word boundaries from the margin words, into a second LDS band; for the rows [yb, ye) also the crack
//      edges (popcounts of M & ~neighbour), the moments (a set-bit loop: int32 sums of x and x^2 per word, int64 per thread) and the
//      histogram (haematoxylin_value of haematoxylin.h: three bytes of the tile per set pixel, the table in LDS; one LDS integer add per pixel);
//   4. one thread per row: its leftmost and rightmost set pixel, for the hull; one thread per border word: the 3 x 3 code of every
//      border pixel from three 34-bit windows of B, classified by three 64-bit membership masks;
//   5. integer wave and block sums (any grouping gives the same bits), then one thread per side of the hull runs its monotone chain over
//      the row extents (hull_chain2, nucmorph_host.h; the stacks reuse the two bands);
//   6. 16 int64 and 256 int32 per nucleus leave with ordinary vector stores.
// LDS: 2 x 8 KB bands, 4 KB row extents, 2 KB histogram and table: 22.3 KB a workgroup.  The padding bits of a row's last word are
// masked off on every read, so no tile pixel at x >= W is ever addressed.
#include "maskbits.h"
#include "nucleus_list.h"
#include "nucmorph_host.h"

namespace {

constexpr int MW = 2048;          // words of one LDS band (mask, and border): at least 5 rows of the widest rectangle (34 words a row)
constexpr unsigned long long CODES_1 = (1ull << 5) | (1ull << 7) | (1ull << 15) | (1ull << 17) | (1ull << 25) | (1ull << 27);
constexpr unsigned long long CODES_2 = (1ull << 21) | (1ull << 33);
constexpr unsigned long long CODES_3 = (1ull << 13) | (1ull << 23);
static_assert(MW >= NUCMORPH_MAX_SIDE + 1 && MW / (NUCMORPH_MAX_SIDE / 32 + 2) >= 5, "a band holds a hull stack and five rows of any rectangle");

struct NucMorphParams {
  NucleusList list;
  NucleusMasks m;
  NucleusTiles t;
  int64_t* raw;            // [n_max][16]
  int32_t* hist;           // [n_max][256]
};

__global__ __launch_bounds__(256) void nucleus_morph_kernel(NucMorphParams p) {
  __shared__ uint32_t Ms[MW], Bs[MW], ext[NUCMORPH_MAX_SIDE];
  __shared__ int hist[NUCMORPH_BINS], lut[NUCMORPH_BINS];
  __shared__ int red[4][5];
  __shared__ long long redl[4][5];
  __shared__ int redi[4][4];
  __shared__ long long side[2];
  const int d = blockIdx.x, H = p.m.H, wpr = p.m.wpr;
  long long b, r;
  const NucleusEntry at = nucleus_entry(p.list, d, b, r);
  if (at == NUCLEUS_PAST) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int64_t* __restrict__ raw = p.raw + (long long)d * NUCMORPH_RAW;
  int32_t* __restrict__ hout = p.hist + (long long)d * NUCMORPH_BINS;
  const auto zero_row = [&] {
    if (tid < NUCMORPH_RAW) raw[tid] = 0;
    hout[tid] = 0;
  };
  if (at == NUCLEUS_OUTSIDE) { zero_row(); return; }
  const uint32_t* __restrict__ m = nucleus_mask(p.m, p.list.K, b, r);
  const uint8_t* __restrict__ tile = nucleus_tile(p.t, H, b);
  const unsigned last = nucleus_last_word(p.m);

  const MaskRect rc = block_mask_rect_256(m, H, wpr, last, red);
  if (rc.area == 0) { zero_row(); return; }
  hist[tid] = 0;
  lut[tid] = p.t.lut[tid];
  const int x0 = rc.x0, y0 = rc.y0, x1 = rc.x1, y1 = rc.y1;                 // inclusive
  const int wx0 = x0 >> 5, nw = (x1 >> 5) - wx0 + 1, pitch = nw + 2;       // staged words of a row: one margin word on either side
  const int band = MW / pitch - 4;                                          // rows of codes per band
  const long long kb0 = p.t.kb[0], kb1 = p.t.kb[1], kb2 = p.t.kb[2];
  long long sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
  int E = 0, n1 = 0, n2 = 0, n3 = 0;
  for (int yb = y0; yb <= y1; yb += band) {
    const int ye = min(yb + band, y1 + 1), rows = ye - yb + 4;             // staged rows [yb - 2, ye + 2); rows * pitch <= MW
    __syncthreads();                                                        // the readers of the band before (and hist / lut above)
    for (int i = tid; i < rows * pitch; i += 256) {
      const int rr = i / pitch, c = i - rr * pitch, y = yb - 2 + rr, w = wx0 - 1 + c;
      unsigned v = 0;
      if (y >= 0 && y < H && c >= 1 && c <= nw) {
        v = m[y * wpr + w];
        if (w == wpr - 1) v &= last;
      }
      Ms[i] = v;
      Bs[i] = 0;
    }
    __syncthreads();
    // ---- border words of the rows [yb - 1, ye + 1); edges, moments and histogram of the rows [yb, ye)
    for (int i = tid; i < (rows - 2) * nw; i += 256) {
      const int rr = i / nw + 1, c = i - (rr - 1) * nw + 1;
      const uint32_t* q = Ms + rr * pitch + c;
      const unsigned v = q[0];
      if (!v) continue;
      const unsigned up = q[-pitch], dn = q[pitch], lf = (v << 1) | (q[-1] >> 31), rt = (v >> 1) | (q[1] << 31);
      Bs[rr * pitch + c] = v & ~(up & dn & lf & rt);
      if (rr < 2 || rr >= rows - 2) continue;
      const int y = yb - 2 + rr, xb = (wx0 + c - 1) * 32;
      E += __popc(v & ~up) + __popc(v & ~dn) + __popc(v & ~lf) + __popc(v & ~rt);
      const uint8_t* __restrict__ px = tile + ((long long)y * p.t.pitch + xb) * 3;
      int s1 = 0, s2 = 0;
      for (unsigned bits = v; bits; bits &= bits - 1) {
        const int bit = __ffs(bits) - 1, x = xb + bit;
        s1 += x; s2 += x * x;
        atomicAdd(&hist[haematoxylin_value(px + bit * 3, lut, kb0, kb1, kb2)], 1);
      }
      const int cnt = __popc(v);
      sx += s1; sy += (long long)y * cnt; sxx += s2; syy += (long long)y * y * cnt; sxy += (long long)y * s1;
    }
    __syncthreads();
    // ---- per row of [yb, ye): leftmost and rightmost set pixel
    for (int rr = 2 + tid; rr < rows - 2; rr += 256) {
      const uint32_t* q = Ms + rr * pitch + 1;
      int lo = 0, hi = nw - 1;
      while (lo < nw && !q[lo]) ++lo;
      while (hi > lo && !q[hi]) --hi;
      ext[yb - 2 + rr - y0] = lo == nw ? NUCMORPH_EMPTY_ROW
                                       : (unsigned)((wx0 + lo) * 32 + __ffs(q[lo]) - 1) | ((unsigned)((wx0 + hi) * 32 + 31 - __clz(q[hi])) << 16);
    }
    // ---- 3 x 3 codes of the border pixels of the rows [yb, ye)
    for (int i = tid; i < (rows - 4) * nw; i += 256) {
      const int rr = i / nw + 2, c = i - (rr - 2) * nw + 1;
      const uint32_t* q = Bs + rr * pitch + c;
      const unsigned bw = q[0];
      if (!bw) continue;
      unsigned long long win[3];                       // bit j + 1 of a window = pixel j of the word; bits 0 and 33 = the neighbours' ends
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const uint32_t* t = q + (k - 1) * pitch;
        win[k] = ((unsigned long long)t[0] << 1) | (t[-1] >> 31) | ((unsigned long long)(t[1] & 1u) << 33);
      }
      for (unsigned bits = bw; bits; bits &= bits - 1) {
        const int bit = __ffs(bits) - 1;
        const unsigned a = (unsigned)(win[0] >> bit) & 7u, c3 = (unsigned)(win[1] >> bit) & 7u, e = (unsigned)(win[2] >> bit) & 7u;
        const int code = 1 + 2 * (int)(((a >> 1) & 1u) + ((e >> 1) & 1u) + (c3 & 1u) + (c3 >> 2))
                           + 10 * (int)((a & 1u) + (a >> 2) + (e & 1u) + (e >> 2));
        n1 += (int)((CODES_1 >> code) & 1ull); n2 += (int)((CODES_2 >> code) & 1ull); n3 += (int)((CODES_3 >> code) & 1ull);
      }
    }
  }
  // ---- integer sums over the workgroup
  sx = wave_sum(sx); sy = wave_sum(sy); sxx = wave_sum(sxx); syy = wave_sum(syy); sxy = wave_sum(sxy);
  E = wave_sum(E); n1 = wave_sum(n1); n2 = wave_sum(n2); n3 = wave_sum(n3);
  if (lane == 0) {
    redl[wave][0] = sx; redl[wave][1] = sy; redl[wave][2] = sxx; redl[wave][3] = syy; redl[wave][4] = sxy;
    redi[wave][0] = E; redi[wave][1] = n1; redi[wave][2] = n2; redi[wave][3] = n3;
  }
  __syncthreads();                                      // also: ext[] complete, the bands free for the hull stacks
  if (tid == 0) side[0] = hull_chain2<false>(ext, y1 - y0 + 1, Ms);
  if (tid == 64) side[1] = hull_chain2<true>(ext, y1 - y0 + 1, Bs);
  __syncthreads();
  if (tid < NUCMORPH_RAW) {
    long long v = 0;
    if (tid == 0) v = rc.area;
    else if (tid == 1) v = x0;
    else if (tid == 2) v = y0;
    else if (tid == 3) v = x1 + 1;
    else if (tid == 4) v = y1 + 1;
    else if (tid < 10) v = redl[0][tid - 5] + redl[1][tid - 5] + redl[2][tid - 5] + redl[3][tid - 5];
    else if (tid < 14) v = (long long)redi[0][tid - 10] + redi[1][tid - 10] + redi[2][tid - 10] + redi[3][tid - 10];
    else if (tid == 14) v = side[1] - side[0];
    raw[tid] = v;
  }
  hout[tid] = hist[tid];
}

int launch_nucleus_morph(const NucMorphParams& p, hipStream_t s) {
  // the bytes of a batch depend on its masks: the profile records the time alone
  ProfScope ps("nucleus_morph", 0, 0, s);
  hipLaunchKernelGGL(nucleus_morph_kernel, dim3((unsigned)p.list.n_max), dim3(256), 0, s, p);
  return launched() ? 0 : NUHTC_E_HIP;
}

}  // namespace

extern "C" {

int nuhtc_nucleus_morph(nuhtc_engine* e, const nuhtc_dets* dets, int B, const uint8_t* tiles_dev, int channel_mode, const int32_t* lut_dev,
                        const int32_t k[3], const int64_t* idx_dev, const int32_t* n_dev, int cap, int64_t* raw_dev, int32_t* hist_dev, void* stream) {
  NucMorphParams p{};
  if (const int rc = nucleus_engine_route(e, "nuhtc_nucleus_morph", "measure", dets, B, idx_dev, n_dev, cap, tiles_dev && lut_dev && k && raw_dev && hist_dev, p.list, p.m)) return rc;
  if (const int rc = nucleus_tiles_args(e, "nucleus_morph", p.list, p.m, tiles_dev, channel_mode, lut_dev, k, p.t)) return rc;
  p.raw = raw_dev; p.hist = hist_dev;
  HIP_CHECK(e, hipSetDevice(e->device));
  const int rc = launch_nucleus_morph(p, (hipStream_t)stream);
  if (rc) FAIL(e, rc, "nucleus_morph launch failed");
  return 0;
}

int nuhtc_op_nucleus_morph(nuhtc_engine* e, const uint8_t* tiles, int channel_mode, const int32_t* lut_dev, const int32_t k[3], int B,
                           const uint32_t* masks, int K, int H, int W, const int32_t* pairs_dev, const int32_t* n_dev, int n_max,
                           int64_t* raw, int32_t* hist, void* stream) {
  if (!e || !tiles || !lut_dev || !k || !masks || !pairs_dev || !raw || !hist) return NUHTC_E_INVALID;
  NucMorphParams p{};
  nucleus_op_route(B, masks, K, H, W, pairs_dev, n_dev, n_max, p.list, p.m);
  if (const int rc = nucleus_tiles_args(e, "nucleus_morph", p.list, p.m, tiles, channel_mode, lut_dev, k, p.t)) return rc;
  p.raw = raw; p.hist = hist;
  HIP_CHECK(e, hipSetDevice(e->device));
  hipStream_t s = (hipStream_t)stream;
  return op_finish(e, launch_nucleus_morph(p, s), s, "nucleus_morph launch failed", "nucleus_morph kernel failed");
}

}  // extern "C"
