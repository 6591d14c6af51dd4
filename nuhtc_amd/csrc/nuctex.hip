// Per-nucleus grey-level co-occurrence counts (gfx950): under the final mask of one kept detection, INTEGERS ONLY -- for the offsets
// (dy, dx) = (0, 1) and (1, 0) the number of unordered pixel pairs {p, p + o}, both in the mask and in the frame, per unordered pair of
// their grey levels q = haematoxylin value >> 4 (16 levels), stored as the upper triangle: int32 [2][136] per nucleus.
// nuhtc_amd/nuctex.py defines them, restates them in numpy (glcm_reference: the device equals it bit for bit) and derives the 26
// Haralick features from them on the host in float64.
//
// One workgroup of 256 threads per nucleus, the shape of nucleus_morph_kernel (nucmorph.hip):
//   1. all threads scan the mask for its rectangle and area (block_mask_rect_256, maskbits.h);
//   2. one thread per mask word v of the rectangle: the pair words are bit operations on v, the word to its right and the word below --
//      R = v & ((v >> 1) | (next << 31)) (bit x: the pixels x and x + 1 are both set), D = v & below -- the padding bits of a row's last
//      word masked off on every read and a word outside the frame read as 0, so no pixel at x >= W or y >= H is ever addressed;
//   3. a set-bit loop over the pixels of the word that are in a pair: the level of a pixel is COMPUTED WHERE IT IS NEEDED
//      (haematoxylin_value of haematoxylin.h: three bytes of the tile, the table in LDS), once for the pixel itself, which serves its
//      pair to the left and the one to the right, and once more for the pixel below it -- twice per pixel of a solid mask, nothing staged,
//      so a rectangle of any size is one pass without bands;
//   4. one LDS integer add per run of pairs that fall into the same cell (a thread holds one pending cell per offset: under a constant
//      colour a word costs two adds, not 63), into the wave's OWN copy of the 272 counters -- the four waves never share an address;
//   5. the four copies are summed and leave with ordinary vector stores.
// Integer adds in any grouping give the same bits: a row is bitwise repeatable across runs and batch splits.
// LDS: 4 x 272 counters, the table, the rectangle scan's 20 ints: 5.4 KB a workgroup.
#include "maskbits.h"
#include "nucleus_list.h"
#include "nuctex_host.h"

namespace {

struct NucTexParams {
  NucleusList list;
  NucleusMasks m;
  NucleusTiles t;
  int32_t* tex;            // [n_max][2][136]
};

// one pending (cell, count) per offset: a run of pairs of the same cell is one LDS add
struct PendingCell {
  int cell, n;
  __device__ __forceinline__ void add(int* cnt, int c) {
    if (c == cell) { ++n; return; }
    if (n) atomicAdd(&cnt[cell], n);
    cell = c; n = 1;
  }
  __device__ __forceinline__ void flush(int* cnt) {
    if (n) atomicAdd(&cnt[cell], n);
    n = 0;
  }
};

__global__ __launch_bounds__(256) void nucleus_texture_kernel(NucTexParams p) {
  __shared__ int cnt[4][NUCTEX_ROW];
  __shared__ int lut[256];
  __shared__ int red[4][5];
  const int d = blockIdx.x, H = p.m.H, wpr = p.m.wpr;
  long long b, r;
  const NucleusEntry at = nucleus_entry(p.list, d, b, r);
  if (at == NUCLEUS_PAST) return;
  const int tid = threadIdx.x, wave = tid >> 6;
  int32_t* __restrict__ out = p.tex + (long long)d * NUCTEX_ROW;
  const auto zero_row = [&] {
    for (int i = tid; i < NUCTEX_ROW; i += 256) out[i] = 0;
  };
  if (at == NUCLEUS_OUTSIDE) { zero_row(); return; }
  const uint32_t* __restrict__ m = nucleus_mask(p.m, p.list.K, b, r);
  const uint8_t* __restrict__ tile = nucleus_tile(p.t, H, b);
  const unsigned last = nucleus_last_word(p.m);

  const MaskRect rc = block_mask_rect_256(m, H, wpr, last, red);
  if (rc.area < 2) { zero_row(); return; }              // no pixel, or one: no pair
  for (int i = tid; i < 4 * NUCTEX_ROW; i += 256) (&cnt[0][0])[i] = 0;
  lut[tid] = p.t.lut[tid];
  __syncthreads();
  int* __restrict__ mine = cnt[wave];
  const int wx0 = rc.x0 >> 5, nw = (rc.x1 >> 5) - wx0 + 1, rows = rc.y1 - rc.y0 + 1;
  const long long kb0 = p.t.kb[0], kb1 = p.t.kb[1], kb2 = p.t.kb[2];
  const long long below = (long long)p.t.pitch * 3;
  PendingCell right{0, 0}, down{0, 0};
  for (int i = tid; i < rows * nw; i += 256) {
    const int rr = i / nw, w = wx0 + i - rr * nw, y = rc.y0 + rr;
    const uint32_t* q = m + y * wpr + w;
    unsigned v = q[0];
    if (w == wpr - 1) v &= last;
    if (!v) continue;
    unsigned nx = 0, dn = 0;
    if (w + 1 < wpr) { nx = q[1]; if (w + 1 == wpr - 1) nx &= last; }
    if (y + 1 < H) { dn = q[wpr]; if (w == wpr - 1) dn &= last; }
    const unsigned R = v & ((v >> 1) | (nx << 31)), D = v & dn;
    const uint8_t* __restrict__ px = tile + ((long long)y * p.t.pitch + w * 32) * 3;
    int prev = 0;                                       // the level of pixel bit - 1 whenever that pixel is in R
    for (unsigned bits = R | (R << 1) | D; bits; bits &= bits - 1) {        // every pixel of this word that is in a pair of this word
      const int bit = __ffs(bits) - 1;
      const int lv = haematoxylin_value(px + bit * 3, lut, kb0, kb1, kb2) >> NUCTEX_SHIFT;
      if (bit > 0 && ((R >> (bit - 1)) & 1u)) right.add(mine, nuctex_cell(prev, lv));
      if ((D >> bit) & 1u) down.add(mine, NUCTEX_CELLS + nuctex_cell(lv, haematoxylin_value(px + below + bit * 3, lut, kb0, kb1, kb2) >> NUCTEX_SHIFT));
      prev = lv;
    }
    // the pair across the word boundary: bit 31 of v (prev is its level) and bit 0 of the next word, a set pixel at x = 32 (w + 1) < W
    if (R >> 31) right.add(mine, nuctex_cell(prev, haematoxylin_value(px + 32 * 3, lut, kb0, kb1, kb2) >> NUCTEX_SHIFT));
  }
  right.flush(mine);
  down.flush(mine);
  __syncthreads();
  for (int i = tid; i < NUCTEX_ROW; i += 256) out[i] = cnt[0][i] + cnt[1][i] + cnt[2][i] + cnt[3][i];
}

int launch_nucleus_texture(const NucTexParams& p, hipStream_t s) {
  // the bytes of a batch depend on its masks: the profile records the time alone
  ProfScope ps("nucleus_texture", 0, 0, s);
  hipLaunchKernelGGL(nucleus_texture_kernel, dim3((unsigned)p.list.n_max), dim3(256), 0, s, p);
  return launched() ? 0 : NUHTC_E_HIP;
}

}  // namespace

extern "C" {

int nuhtc_nucleus_texture(nuhtc_engine* e, const nuhtc_dets* dets, int B, const uint8_t* tiles_dev, int channel_mode, const int32_t* lut_dev,
                          const int32_t k[3], const int64_t* idx_dev, const int32_t* n_dev, int cap, int32_t* tex_dev, void* stream) {
  NucTexParams p{};
  if (const int rc = nucleus_engine_route(e, "nuhtc_nucleus_texture", "measure", dets, B, idx_dev, n_dev, cap, tiles_dev && lut_dev && k && tex_dev, p.list, p.m)) return rc;
  if (const int rc = nucleus_tiles_args(e, "nucleus_texture", p.list, p.m, tiles_dev, channel_mode, lut_dev, k, p.t)) return rc;
  p.tex = tex_dev;
  HIP_CHECK(e, hipSetDevice(e->device));
  const int rc = launch_nucleus_texture(p, (hipStream_t)stream);
  if (rc) FAIL(e, rc, "nucleus_texture launch failed");
  return 0;
}

int nuhtc_op_nucleus_texture(nuhtc_engine* e, const uint8_t* tiles, int channel_mode, const int32_t* lut_dev, const int32_t k[3], int B,
                             const uint32_t* masks, int K, int H, int W, const int32_t* pairs_dev, const int32_t* n_dev, int n_max,
                             int32_t* tex, void* stream) {
  if (!e || !tiles || !lut_dev || !k || !masks || !pairs_dev || !tex) return NUHTC_E_INVALID;
  NucTexParams p{};
  nucleus_op_route(B, masks, K, H, W, pairs_dev, n_dev, n_max, p.list, p.m);
  if (const int rc = nucleus_tiles_args(e, "nucleus_texture", p.list, p.m, tiles, channel_mode, lut_dev, k, p.t)) return rc;
  p.tex = tex;
  HIP_CHECK(e, hipSetDevice(e->device));
  hipStream_t s = (hipStream_t)stream;
  return op_finish(e, launch_nucleus_texture(p, s), s, "nucleus_texture launch failed", "nucleus_texture kernel failed");
}

}  // extern "C"
