// Scoring images that are larger than a tile (nuhtc_stitch_*, nuhtc_op_stitch_*): what tools/eval_consep.py needs from the masks of the
// tiles an image was cut into, as integer tables -- the protocol of `CoNSePCocoDataset.evaluate` (nuhtc/datasets/WSI_coco_CoNSeP.py:117-426).
//
//   gather : after nuhtc_infer, per tile of the batch: every detection with score >= fg_thr whose float box keeps `discard_offset` pixels
//            from each INNER tile edge (:198-211) becomes a candidate of its image: the tight box of its mask in image pixels, area, score,
//            label, an order key and the mask cropped to that box in the nuhtc_merge_overlap layout, appended to the image's pool.  Three
//            kernels -- measure (one wave per slot), scan (one workgroup per image: exclusive scan over the slots in (tile, slot) order),
//            fill (one wave per slot) -- so a candidate's number depends on the order of the tiles alone, never on the order atomics land.
//            A crop starts at any bit of a tile row (tiles overlap at a stride that is no multiple of 32): every crop word is funnelled out
//            of two tile words.
//   (the image-level mask-NMS is nuhtc_merge_overlap(NUHTC_OVERLAP_MASK) on these records; Engine.stitch_nms feeds it)
//   pairs  : one wave per kept prediction walks the set pixels of its crop over the image's ground-truth map (int32 [H][W], row + 1),
//            counts its partners in a 64-slot table of its own in LDS and emits (row, position, pixels); area_t by a histogram pass.
//   render : `convert_format` 'conic' (WSI_coco.py:863-906) in the image frame: inst_map = max position + 1, type_map = max label + 1 over
//            the masks covering a pixel, two independent maxima, by atomicMax.
//
// Every index read from device memory (counts, labels, tile records, kept lists, candidate boxes and offsets, map values) is range-checked
// before it is used as an address; lists are written below their capacity only and the needed size is counted past it.  Wave reductions and
// the block scan: block_prims.h.
#include <climits>

#include "engine.h"
#include "maskbits.h"

namespace {

constexpr int SW = 8;                // ints of scratch per detection slot: pass, x0, y0, x1, y1, area, candidate number, word offset
constexpr int SP_SLOTS = 64;         // partners one prediction may have: one table slot per lane
constexpr int ST_MAX_TCAP = 8192;    // ground-truth rows the LDS histogram of area_t holds
constexpr int ST_MAX_OFF = 1 << 20;  // largest tile offset / image side

#define ST_WAVE_SYNC()                                     \
  do {                                                     \
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); \
    __builtin_amdgcn_wave_barrier();                       \
  } while (0)

struct GatherParams {
  const float* boxes; const int* labels; const int* counts; const unsigned* masks; const int* meta;
  int B, K, T, C;
  float fg_thr, lo, hi;
  nuhtc_stitch_store st;
};

__device__ __forceinline__ int crop_words(const int* w) { return (w[4] - w[2]) * ((w[3] - w[1] + 31) >> 5); }

// one wave per detection slot: the candidate rules, then area and tight box of the mask (tile pixels)
__global__ __launch_bounds__(256) void stitch_measure_kernel(GatherParams p) {
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= p.B * p.K) return;
  const int b = s / p.K, r = s - b * p.K;
  int* w = p.st.work + (long long)s * SW;
  const int* m = p.meta + b * 8;
  const int img = m[0];
  bool ok = r < min(max(p.counts[b], 0), p.K);
  if (ok && (img < 0 || img >= p.st.n_img || m[1] < 0 || m[1] > ST_MAX_OFF || m[2] < 0 || m[2] > ST_MAX_OFF)) {
    if (lane == 0) atomicOr(&p.st.counters[3], 2);      // a tile record that names no image: flagged on image 0
    ok = false;
  }
  if (ok) {
    const float* bx = p.boxes + (long long)s * 5;
    ok = bx[4] >= p.fg_thr;                              // (false for NaN)
    if (!m[3] && bx[0] < p.lo) ok = false;
    if (!m[4] && bx[2] > p.hi) ok = false;
    if (!m[5] && bx[1] < p.lo) ok = false;
    if (!m[6] && bx[3] > p.hi) ok = false;               // the reference compares y2 with the tile WIDTH (:211); tiles are square here
    const int lab = p.labels[s];
    if (ok && (lab < 0 || lab >= p.C)) {
      if (lane == 0) atomicOr(&p.st.counters[img * 4 + 3], 1);
      ok = false;
    }
  }
  if (!ok) {
    if (lane == 0) w[0] = 0;
    return;
  }
  const int wpr = p.T >> 5, words = p.T * wpr;
  const unsigned* mi = p.masks + (long long)s * words;
  int cnt = 0, y0 = p.T, y1 = 0, x0 = p.T, x1 = 0;
  for (int wv = lane; wv < words; wv += 64) {
    const unsigned v = mi[wv];
    if (v) {
      const int y = wv / wpr, xw = (wv - y * wpr) << 5;
      cnt += __popc(v);
      y0 = min(y0, y); y1 = max(y1, y + 1);
      x0 = min(x0, xw + __ffs((int)v) - 1); x1 = max(x1, xw + 32 - __clz((int)v));
    }
  }
  cnt = wave_sum(cnt);
  y0 = wave_min(y0); y1 = wave_max(y1); x0 = wave_min(x0); x1 = wave_max(x1);
  if (lane == 0) {
    w[0] = 1;
    if (cnt) { w[1] = x0; w[2] = y0; w[3] = x1; w[4] = y1; }
    else { w[1] = 0; w[2] = 0; w[3] = 0; w[4] = 0; }      // an empty mask stays a candidate, with an empty crop
    w[5] = cnt;
  }
}

// one workgroup per image: numbers the passing slots of its tiles in (tile, slot) order behind what the image already holds
__global__ __launch_bounds__(1024) void stitch_scan_kernel(GatherParams p) {
  __shared__ int lds16[17];
  const int img = blockIdx.x, tid = threadIdx.x;
  const int S = p.B * p.K, per = (S + 1023) / 1024;
  const int lo = min(tid * per, S), hi = min(lo + per, S);
  int* cn = p.st.counters + img * 4;
  const long long base_c = cn[0], base_w = cn[1];
  int c = 0, ww = 0;
  for (int s = lo; s < hi; ++s) {
    const int* w = p.st.work + (long long)s * SW;
    if (w[0] && p.meta[(s / p.K) * 8] == img) { ++c; ww += crop_words(w); }
  }
  int tot_c, tot_w;
  const int ex_c = block_exscan_1024(c, lds16, &tot_c);
  const int ex_w = block_exscan_1024(ww, lds16, &tot_w);
  long long idx = base_c + ex_c, off = base_w + ex_w;
  int flag = 0;
  for (int s = lo; s < hi; ++s) {
    int* w = p.st.work + (long long)s * SW;
    if (!(w[0] && p.meta[(s / p.K) * 8] == img)) continue;
    const int nw = crop_words(w);
    const bool fits_c = idx < p.st.cand_cap, fits_w = off + nw <= p.st.pool_cap;
    w[6] = fits_c ? (int)idx : -1;
    w[7] = fits_w ? (int)off : -1;
    flag |= (fits_c ? 0 : 1) | (fits_w ? 0 : 2);
    ++idx;
    off += nw;
  }
  if (flag) atomicOr(&cn[2], flag);
  if (tid == 0) {          // the sizes the image needs, counted past the capacities (every thread read them before the scans' barriers)
    cn[0] = (int)min(base_c + tot_c, (long long)INT_MAX);
    cn[1] = (int)min(base_w + tot_w, (long long)INT_MAX);
  }
}

// one wave per detection slot: the candidate record, and its crop funnelled out of the tile's rows
__global__ __launch_bounds__(256) void stitch_fill_kernel(GatherParams p) {
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= p.B * p.K) return;
  const int* w = p.st.work + (long long)s * SW;
  if (!w[0]) return;
  const int idx = w[6], off = w[7];
  if (idx < 0 || idx >= p.st.cand_cap) return;
  const int b = s / p.K, r = s - b * p.K;
  const int* m = p.meta + b * 8;
  const int img = m[0];
  if (img < 0 || img >= p.st.n_img) return;
  const int x0 = w[1], y0 = w[2], x1 = w[3], y1 = w[4];
  if (x0 < 0 || y0 < 0 || x1 > p.T || y1 > p.T || x1 < x0 || y1 < y0) return;
  const long long rec = (long long)img * p.st.cand_cap + idx;
  const int cw = x1 - x0, ch = y1 - y0, cwpr = (cw + 31) >> 5, nw = ch * cwpr;
  const bool crop = off >= 0 && (long long)off + nw <= p.st.pool_cap;
  if (lane == 0) {
    int* bo = p.st.box + rec * 4;
    const bool any = w[5] > 0;
    bo[0] = any ? x0 + m[1] : 0; bo[1] = any ? y0 + m[2] : 0; bo[2] = any ? x1 + m[1] : 0; bo[3] = any ? y1 + m[2] : 0;
    p.st.area[rec] = w[5];
    p.st.score[rec] = p.boxes[(long long)s * 5 + 4];
    const int lab = p.labels[s];
    p.st.label[rec] = lab;
    p.st.key[rec] = ((long long)m[7] * p.C + lab) * p.K + r;      // tile location, class, slot: the np.concatenate of bbox2result
    p.st.off[rec] = crop ? off : -1;
  }
  if (!crop) return;
  const int wpr = p.T >> 5;
  const unsigned* mi = p.masks + (long long)s * p.T * wpr;
  unsigned* dst = p.st.pool + (long long)img * p.st.pool_cap + off;
  for (int t = lane; t < nw; t += 64) {
    const int y = t / cwpr, j = t - y * cwpr;
    const int xs = x0 + (j << 5), wi = xs >> 5, sh = xs & 31;
    const unsigned* row = mi + (long long)(y0 + y) * wpr;
    unsigned v = row[wi] >> sh;
    if (sh && wi + 1 < wpr) v |= row[wi + 1] << (32 - sh);
    const int rem = cw - (j << 5);
    if (rem < 32) v &= (1u << rem) - 1u;
    dst[t] = v;
  }
}

struct ScoreParams {
  nuhtc_stitch_store st;
  int image; const int* kept; int n_kept; const int* gt;
  int H, W, t_cap, cap;
  int* area_t; int* trips; int* inst_map; int* type_map; int* counters;
};

// the crop of kept prediction q, checked: false (and counters[2] flagged) when a value read from memory would lead outside a buffer
struct Crop { int x0, y0, w, h, wpr, label; const unsigned* bits; };
__device__ __forceinline__ bool load_crop(const ScoreParams& p, int q, int lane, Crop& c) {
  const int cand = p.kept[q];
  const int n_cand = min(max(p.st.counters[p.image * 4], 0), p.st.cand_cap);
  bool ok = cand >= 0 && cand < n_cand;
  if (ok) {
    const long long rec = (long long)p.image * p.st.cand_cap + cand;
    const int* bo = p.st.box + rec * 4;
    const long long off = p.st.off[rec];
    c.x0 = bo[0]; c.y0 = bo[1]; c.w = bo[2] - bo[0]; c.h = bo[3] - bo[1]; c.wpr = (c.w + 31) >> 5;
    c.label = p.st.label[rec];
    ok = c.x0 >= 0 && c.y0 >= 0 && c.w >= 0 && c.h >= 0 && bo[2] <= p.W && bo[3] <= p.H && off >= 0 &&
         off + (long long)c.h * c.wpr <= p.st.pool_cap;
    c.bits = p.st.pool + (long long)p.image * p.st.pool_cap + (ok ? off : 0);
  }
  if (!ok && lane == 0) atomicOr(&p.counters[2], 1);
  return ok;
}
// word t of a crop, its bits past the crop's width cleared
__device__ __forceinline__ unsigned crop_word(const Crop& c, int t, int& y, int& xs) {
  y = t / c.wpr;
  const int j = t - y * c.wpr, rem = c.w - (j << 5);
  xs = c.x0 + (j << 5);
  const unsigned v = c.bits[t];
  return rem < 32 ? v & ((1u << rem) - 1u) : v;
}

// area_t[t] += pixels with value t + 1 (zeroed by the launcher)
__global__ __launch_bounds__(256) void stitch_area_t_kernel(ScoreParams p) {
  extern __shared__ int hist[];
  const int tid = threadIdx.x;
  for (int t = tid; t < p.t_cap; t += 256) hist[t] = 0;
  __syncthreads();
  const int total = p.H * p.W;
  bool bad = false;
  for (int i = blockIdx.x * 256 + tid; i < total; i += gridDim.x * 256) {
    const int t = p.gt[i];
    if (t > 0 && t <= p.t_cap) atomicAdd(&hist[t - 1], 1);
    else if (t != 0) bad = true;
  }
  if (bad) atomicOr(&p.counters[2], 1);
  __syncthreads();
  for (int t = tid; t < p.t_cap; t += 256)
    if (hist[t]) atomicAdd(&p.area_t[t], hist[t]);
}

// one wave per kept prediction
__global__ __launch_bounds__(256) void stitch_pairs_kernel(ScoreParams p) {
  __shared__ int skey[4][SP_SLOTS];      // ground-truth value (row + 1) of a partner, 0 = free
  __shared__ int scnt[4][SP_SLOTS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = blockIdx.x * 4 + wave;
  if (q >= p.n_kept) return;
  Crop c;
  if (!load_crop(p, q, lane, c)) return;
  int* key = skey[wave];
  int* cnt = scnt[wave];
  key[lane] = 0;
  cnt[lane] = 0;
  ST_WAVE_SYNC();
  bool bad = false, full = false;
  for (int t = lane; t < c.h * c.wpr; t += 64) {
    int y, xs;
    unsigned v = crop_word(c, t, y, xs);
    while (v) {
      const int bit = __ffs((int)v) - 1;
      v &= v - 1;
      const int g = p.gt[(long long)(c.y0 + y) * p.W + xs + bit];
      if (g > 0 && g <= p.t_cap) {
        unsigned h = ((unsigned)g * 0x9E3779B1u) >> 26;
        bool done = false;
        for (int probe = 0; probe < SP_SLOTS && !done; ++probe) {
          const int prev = atomicCAS(&key[h], 0, g);
          if (prev == 0 || prev == g) { atomicAdd(&cnt[h], 1); done = true; }
          h = (h + 1) & (SP_SLOTS - 1);
        }
        if (!done) full = true;
      } else if (g != 0) {
        bad = true;
      }
    }
  }
  ST_WAVE_SYNC();
  if (__any(bad) && lane == 0) atomicOr(&p.counters[2], 1);
  if (__any(full) && lane == 0) atomicOr(&p.counters[3], 1);     // more distinct partners than the table holds
  const bool mine = key[lane] != 0;
  const unsigned long long bal = __ballot(mine);
  const int n = __popcll(bal);
  if (!n) return;
  int base = 0;
  if (lane == 0) base = atomicAdd(&p.counters[0], n);
  base = __shfl(base, 0);
  if (mine) {
    const int pos = base + __popcll(bal & ((1ull << lane) - 1ull));
    if (pos >= 0 && pos < p.cap) {
      int* o = p.trips + (long long)pos * 3;
      o[0] = key[lane] - 1; o[1] = q; o[2] = cnt[lane];
    } else {
      atomicOr(&p.counters[1], 1);
    }
  }
}

// one wave per kept prediction (maps zeroed by the launcher)
__global__ __launch_bounds__(256) void stitch_render_kernel(ScoreParams p) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= p.n_kept) return;
  Crop c;
  if (!load_crop(p, q, lane, c)) return;
  for (int t = lane; t < c.h * c.wpr; t += 64) {
    int y, xs;
    unsigned v = crop_word(c, t, y, xs);
    while (v) {
      const int bit = __ffs((int)v) - 1;
      v &= v - 1;
      const long long pix = (long long)(c.y0 + y) * p.W + xs + bit;
      atomicMax(&p.inst_map[pix], q + 1);
      atomicMax(&p.type_map[pix], c.label + 1);
    }
  }
}

const char* bad_store(const nuhtc_stitch_store* st) {
  if (!st || !st->box || !st->area || !st->score || !st->label || !st->key || !st->off || !st->pool || !st->counters || !st->work)
    return "stitch: null store buffer";
  if (st->n_img < 1 || st->n_img > 4096 || st->cand_cap < 1 || st->pool_cap < 1) return "stitch: store sizes out of range (n_img 1..4096, capacities >= 1)";
  return nullptr;
}

int launch_gather(const GatherParams& p, hipStream_t s) {
  ProfScope ps("stitch_gather", 0, 0, s);
  const int S = p.B * p.K;
  hipLaunchKernelGGL(stitch_measure_kernel, dim3(cdiv(S, 4)), dim3(256), 0, s, p);
  hipLaunchKernelGGL(stitch_scan_kernel, dim3(p.st.n_img), dim3(1024), 0, s, p);
  hipLaunchKernelGGL(stitch_fill_kernel, dim3(cdiv(S, 4)), dim3(256), 0, s, p);
  return launched() ? 0 : NUHTC_E_HIP;
}

const char* bad_gather(const nuhtc_stitch_store* st, int B, int K, int T, int C) {
  if (const char* m = bad_store(st)) return m;
  if (B < 1 || B > 256 || K < 1 || K > 2048 || C < 1 || C > 14) return "stitch_gather: B (1..256), K (1..2048) or C (1..14) out of range";
  if (T < 32 || T % 32 || T > 1024) return "stitch_gather: tiles are square with a side that is a multiple of 32, at most 1024";
  if ((long long)B * K * T * (T >> 5) >= (1ll << 31)) return "stitch_gather: the masks of a batch must stay below 2^31 words";
  if ((long long)B * K * SW > st->work_cap) return "stitch_gather: the store's work buffer holds fewer than 8 ints per detection slot";
  return nullptr;
}

// counters [4]: [0] trip entries needed, [1] entries dropped (capacity), [2] a value or index out of range, [3] partner table overflow
const char* bad_score(const nuhtc_stitch_store* st, int image, int n_kept, int H, int W) {
  if (const char* m = bad_store(st)) return m;
  if (image < 0 || image >= st->n_img || n_kept < 0 || n_kept > st->cand_cap) return "stitch: image or n_kept out of range";
  if (H < 1 || W < 1 || H > ST_MAX_OFF || W > ST_MAX_OFF || (long long)H * W > (1ll << 28)) return "stitch: image size out of range (H x W at most 2^28)";
  return nullptr;
}

int launch_pairs(const ScoreParams& p, hipStream_t s) {
  ProfScope ps("stitch_pairs", 0, 0, s);
  if (hipMemsetAsync(p.counters, 0, 4 * sizeof(int), s) != hipSuccess || hipMemsetAsync(p.area_t, 0, (size_t)p.t_cap * sizeof(int), s) != hipSuccess)
    return NUHTC_E_HIP;
  const int chunks = std::max(1, std::min(256, cdiv(p.H * p.W, 256 * 16)));
  hipLaunchKernelGGL(stitch_area_t_kernel, dim3(chunks), dim3(256), (size_t)p.t_cap * sizeof(int), s, p);
  if (p.n_kept) hipLaunchKernelGGL(stitch_pairs_kernel, dim3(cdiv(p.n_kept, 4)), dim3(256), 0, s, p);
  return launched() ? 0 : NUHTC_E_HIP;
}

int launch_render(const ScoreParams& p, hipStream_t s) {
  ProfScope ps("stitch_render", 0, 0, s);
  const size_t bytes = (size_t)p.H * p.W * sizeof(int);
  if (hipMemsetAsync(p.inst_map, 0, bytes, s) != hipSuccess || hipMemsetAsync(p.type_map, 0, bytes, s) != hipSuccess) return NUHTC_E_HIP;
  if (p.n_kept) hipLaunchKernelGGL(stitch_render_kernel, dim3(cdiv(p.n_kept, 4)), dim3(256), 0, s, p);
  return launched() ? 0 : NUHTC_E_HIP;
}

int pairs_args(nuhtc_engine* e, const nuhtc_stitch_store* st, int image, const int32_t* kept, int n_kept, const int32_t* gt_map, int H, int W, int t_cap,
               int trip_cap, int32_t* area_t, int32_t* trips, int32_t* counters, ScoreParams* p) {
  if (!kept || !gt_map || !area_t || !trips || !counters) FAIL(e, NUHTC_E_INVALID, "stitch_pairs: null argument");
  if (const char* m = bad_score(st, image, n_kept, H, W)) FAIL(e, NUHTC_E_INVALID, m);
  if (t_cap < 1 || t_cap > ST_MAX_TCAP || trip_cap < 1) FAIL(e, NUHTC_E_INVALID, "stitch_pairs: t_cap (1..8192) / trip_cap out of range");
  *p = ScoreParams{*st, image, kept, n_kept, gt_map, H, W, t_cap, trip_cap, area_t, trips, nullptr, nullptr, counters};
  return 0;
}

int render_args(nuhtc_engine* e, const nuhtc_stitch_store* st, int image, const int32_t* kept, int n_kept, int H, int W, int32_t* inst_map,
                int32_t* type_map, int32_t* counters, ScoreParams* p) {
  if (!kept || !inst_map || !type_map || !counters) FAIL(e, NUHTC_E_INVALID, "stitch_render: null argument");
  if (const char* m = bad_score(st, image, n_kept, H, W)) FAIL(e, NUHTC_E_INVALID, m);
  *p = ScoreParams{*st, image, kept, n_kept, nullptr, H, W, 0, 0, nullptr, nullptr, inst_map, type_map, counters};
  return 0;
}

}  // namespace

extern "C" {

int nuhtc_stitch_gather(nuhtc_engine* e, const nuhtc_dets* dets, int B, const int32_t* tile_meta, float fg_thr, float discard_offset,
                        const nuhtc_stitch_store* st, void* stream) {
  if (!e) return NUHTC_E_INVALID;
  if (!dets || !dets->boxes || !dets->labels || !dets->counts || !dets->masks || !tile_meta) FAIL(e, NUHTC_E_INVALID, "bad nuhtc_stitch_gather arguments");
  const nuhtc_config& c = e->cfg;
  if (B > c.max_batch || c.tile_h != c.tile_w) FAIL(e, NUHTC_E_INVALID, "nuhtc_stitch_gather: B beyond max_batch, or tiles that are not square");
  if (const char* m = bad_gather(st, B, c.max_per_img, c.tile_w, c.num_classes)) FAIL(e, NUHTC_E_INVALID, m);
  HIP_CHECK(e, hipSetDevice(e->device));
  GatherParams p{dets->boxes, dets->labels, dets->counts, dets->masks, tile_meta, B, c.max_per_img, c.tile_w, c.num_classes,
                 fg_thr, discard_offset, (float)c.tile_w - discard_offset, *st};
  RUN(launch_gather(p, (hipStream_t)stream));
  return 0;
}

int nuhtc_op_stitch_gather(nuhtc_engine* e, const float* boxes, const int32_t* labels, const int32_t* counts, const uint32_t* masks,
                           const int32_t* tile_meta, int B, int K, int tile, int C, float fg_thr, float discard_offset, const nuhtc_stitch_store* st,
                           void* stream) {
  if (!e || !boxes || !labels || !counts || !masks || !tile_meta) return NUHTC_E_INVALID;
  if (const char* m = bad_gather(st, B, K, tile, C)) FAIL(e, NUHTC_E_INVALID, m);
  HIP_CHECK(e, hipSetDevice(e->device));
  hipStream_t s = (hipStream_t)stream;
  GatherParams p{boxes, labels, counts, masks, tile_meta, B, K, tile, C, fg_thr, discard_offset, (float)tile - discard_offset, *st};
  return op_finish(e, launch_gather(p, s), s, "stitch_gather launch failed", "stitch_gather kernel failed");
}

int nuhtc_stitch_pairs(nuhtc_engine* e, const nuhtc_stitch_store* st, int image, const int32_t* kept, int n_kept, const int32_t* gt_map, int H, int W,
                       int t_cap, int trip_cap, int32_t* area_t, int32_t* trips, int32_t* counters, void* stream) {
  if (!e) return NUHTC_E_INVALID;
  ScoreParams p;
  if (int rc = pairs_args(e, st, image, kept, n_kept, gt_map, H, W, t_cap, trip_cap, area_t, trips, counters, &p)) return rc;
  HIP_CHECK(e, hipSetDevice(e->device));
  RUN(launch_pairs(p, (hipStream_t)stream));
  return 0;
}

int nuhtc_op_stitch_pairs(nuhtc_engine* e, const nuhtc_stitch_store* st, int image, const int32_t* kept, int n_kept, const int32_t* gt_map, int H,
                          int W, int t_cap, int trip_cap, int32_t* area_t, int32_t* trips, int32_t* counters, void* stream) {
  if (!e) return NUHTC_E_INVALID;
  ScoreParams p;
  if (int rc = pairs_args(e, st, image, kept, n_kept, gt_map, H, W, t_cap, trip_cap, area_t, trips, counters, &p)) return rc;
  HIP_CHECK(e, hipSetDevice(e->device));
  hipStream_t s = (hipStream_t)stream;
  return op_finish(e, launch_pairs(p, s), s, "stitch_pairs launch failed", "stitch_pairs kernel failed");
}

int nuhtc_stitch_render(nuhtc_engine* e, const nuhtc_stitch_store* st, int image, const int32_t* kept, int n_kept, int H, int W, int32_t* inst_map,
                        int32_t* type_map, int32_t* counters, void* stream) {
  if (!e) return NUHTC_E_INVALID;
  ScoreParams p;
  if (int rc = render_args(e, st, image, kept, n_kept, H, W, inst_map, type_map, counters, &p)) return rc;
  HIP_CHECK(e, hipSetDevice(e->device));
  RUN(launch_render(p, (hipStream_t)stream));
  return 0;
}

int nuhtc_op_stitch_render(nuhtc_engine* e, const nuhtc_stitch_store* st, int image, const int32_t* kept, int n_kept, int H, int W, int32_t* inst_map,
                           int32_t* type_map, int32_t* counters, void* stream) {
  if (!e) return NUHTC_E_INVALID;
  ScoreParams p;
  if (int rc = render_args(e, st, image, kept, n_kept, H, W, inst_map, type_map, counters, &p)) return rc;
  HIP_CHECK(e, hipSetDevice(e->device));
  hipStream_t s = (hipStream_t)stream;
  return op_finish(e, launch_render(p, s), s, "stitch_render launch failed", "stitch_render kernel failed");
}

}  // extern "C"
