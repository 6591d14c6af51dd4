// Scoring a batch of tiles on the device (nuhtc_eval_batch, nuhtc_op_eval_*): what tools/test_pannuke.py needs from the masks of a finished
// nuhtc_infer, as integer tables -- the host never sees a mask.
//
//   eval_select_kernel : `WSIDataset.evaluate` of the reference (nuhtc/datasets/WSI_coco.py:278-545): score >= fg_thr, then `mask_nms`
//                        (stats_utils.py:10-32): visit in descending score, a kept mask removes every later one with
//                        inter / max(union, 1) > thr, decided in float64 on the integer popcounts exactly as numpy decides it.
//                        Equal scores are visited in descending slot order (what a stable ascending argsort, reversed, gives).
//   eval_area_t_kernel,
//   eval_pairs_kernel  : intersections of every (ground-truth instance, selected prediction) pair and both areas (`get_mask_inter_union`,
//                        stats_utils.py:438-455).  The ground truth comes as per-class instance maps whose values are row numbers + 1
//                        (evaluation.gt_rows), so one walk over the set pixels of a prediction counts all its partners in an LDS histogram;
//                        only the non-zero (tile, t, p, inter) entries leave the kernel.
//   eval_render_kernel : `convert_format` (WSI_coco.py:863-906), 'pannuke' (H, W, C + 1) and 'conic' (H, W, 2) label maps.
//   eval_joint_kernel  : the joint histograms `get_fast_pq_map` builds (tools/analysis_tools/pannuke/utils.py:7-104) between the true and the
//                        predicted map of each class, and between the two maps `binarize` (utils.py:141-162) makes of all classes: an LDS hash
//                        table of (true id, pred id) -> pixels per (tile, table), emitted as non-zero entries.
//
// Every index a kernel reads from device memory (counts, selections, map values) is range-checked before it is used as an address;
// output lists are written below their capacity only and the needed size is counted past it (emit_nonempty).  The sort, its total-order
// score key and the wave reductions come from block_prims.h, the mask-pair verdict and the greedy pass from maskbits.h.
#include "engine.h"
#include "maskbits.h"

namespace {

constexpr int EV_MAXK = 2048;       // detections per tile the LDS tables hold
constexpr int EV_MAX_TCAP = 8192;   // ground-truth rows per tile the LDS histograms hold
constexpr int ES_NT = 1024;
constexpr int EJ_NT = 1024;
constexpr int EJ_SLOTS = 4096;      // hash slots of one joint table: distinct (true id, pred id) pairs of one tile and class
constexpr int EJ_CLASS_SHIFT = 27;  // binarised id = class << 27 | id: ordered class-major like `binarize` numbers them

struct SelectParams {
  const float* scores; int score_stride;
  const int* counts; const unsigned* masks; const int* labels;
  int K, H, W; float fg_thr; double thr;
  int* sel; int* nsel; int* sel_labels;
};

__global__ __launch_bounds__(ES_NT) void eval_select_kernel(SelectParams p) {
  __shared__ unsigned long long okey[EV_MAXK];
  __shared__ short4 sbb[EV_MAXK];            // rows [x, y) and word columns [z, w) that hold the set bits of the candidate
  __shared__ int sarea[EV_MAXK];
  __shared__ short sidx[EV_MAXK];
  __shared__ short skept[EV_MAXK];
  __shared__ unsigned char sup[EV_MAXK];
  __shared__ int s_m;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int NWV = ES_NT / 64;
  const int K = p.K;
  const int n = min(max(p.counts[b], 0), K);
  const int wpr = p.W >> 5, words = p.H * wpr;
  const float* scores = p.scores + (long long)b * K * p.score_stride;
  const unsigned* masks = p.masks + (long long)b * K * words;
  if (tid == 0) s_m = 0;
  __syncthreads();
  const int npad = next_pow2(max(n, 2));
  for (int j = tid; j < npad; j += ES_NT) {
    unsigned long long key = ~0ull;
    if (j < n) {
      const float sc = scores[(long long)j * p.score_stride];
      if (sc >= p.fg_thr) {          // (false for NaN)
        key = ((unsigned long long)desc_key_total(sc) << 32) | (unsigned)(0xFFFF - j);      // (scores come in unchecked: any sign)
        atomicAdd(&s_m, 1);
      }
    }
    okey[j] = key;
    sup[j] = 0;
  }
  __syncthreads();
  bitonic_sort_u64<ES_NT>(okey, npad, tid);
  const int m = s_m;                 // the candidates that passed the filter sort first
  // area and extent of every candidate, one wave each
  for (int a = wave; a < m; a += NWV) {
    const int i = 0xFFFF - (int)(okey[a] & 0xFFFF);
    const unsigned* mi = masks + (long long)i * words;
    int cnt = 0, y0 = p.H, y1 = 0, x0 = wpr, x1 = 0;
    for (int wv = lane; wv < words; wv += 64) {
      const unsigned v = mi[wv];
      if (v) {
        const int y = wv / wpr, x = wv - y * wpr;
        cnt += __popc(v);
        y0 = min(y0, y); y1 = max(y1, y + 1); x0 = min(x0, x); x1 = max(x1, x + 1);
      }
    }
    cnt = wave_sum(cnt);
    y0 = wave_min(y0); y1 = wave_max(y1); x0 = wave_min(x0); x1 = wave_max(x1);
    if (lane == 0) {
      sidx[a] = (short)i;
      sarea[a] = cnt;
      sbb[a] = make_short4((short)y0, (short)y1, (short)x0, (short)x1);
    }
  }
  __syncthreads();
  // greedy pass; pre-test: the bounding rows and word columns of the two candidates (disjoint ones still get the verdict on 0 pixels)
  struct Kept { short4 bb; const unsigned* mi; int area; };
  int nout = 0;                      // (tid 0)
  greedy_mask_pass<ES_NT>(
      m, sup,
      [&](int a) {
        if (tid == 0) skept[nout++] = sidx[a];
        return Kept{sbb[a], masks + (long long)sidx[a] * words, sarea[a]};
      },
      [&](const Kept& k, int c) {
        const short4 bc = sbb[c];
        const int y0 = max(k.bb.x, bc.x), y1 = min(k.bb.y, bc.y);
        if (y0 < y1 && max(k.bb.z, bc.z) < min(k.bb.w, bc.w))
          return mask_pair_over<true>(k.mi, masks + (long long)sidx[c] * words, y0 * wpr, y1 * wpr, k.area, sarea[c], p.thr, lane);
        return mask_inter_over<true>(0, k.area, sarea[c], p.thr);
      });
  if (tid == 0) { s_m = nout; p.nsel[b] = nout; }
  __syncthreads();
  const int kept = s_m;
  for (int j = tid; j < K; j += ES_NT) {
    const int slot = j < kept ? skept[j] : -1;
    p.sel[(long long)b * K + j] = slot;
    if (p.sel_labels) p.sel_labels[(long long)b * K + j] = (slot >= 0 && p.labels) ? p.labels[(long long)b * K + slot] : -1;
  }
}

// The tail of a kernel that leaves the non-empty ones of its workgroup's `nslots` LDS slots as entries of a global list of `cap`
// entries: counts them, reserves a range with one atomic on counters[0] (the size the list needs, counted past cap too), writes the
// entries that lie below cap -- ascending slot index per thread stride -- and flags counters[1] when one did not.  *s_cnt must be 0
// since a barrier; NT threads; a thread returns from its kernel after this.
template <int NT, typename NonEmpty, typename Write>
__device__ __forceinline__ void emit_nonempty(int nslots, int cap, int* counters, int* s_cnt, int* s_base, NonEmpty nonempty, Write write) {
  const int tid = threadIdx.x;
  int mine = 0;
  for (int i = tid; i < nslots; i += NT) mine += nonempty(i);
  int off = mine ? atomicAdd(s_cnt, mine) : 0;
  __syncthreads();
  if (tid == 0) *s_base = *s_cnt ? atomicAdd(&counters[0], *s_cnt) : 0;
  __syncthreads();
  if (!mine) return;
  off += *s_base;
  for (int i = tid; i < nslots; i += NT)
    if (nonempty(i)) {
      if (off < cap) write(i, off);
      else atomicOr(&counters[1], 1);
      ++off;
    }
}

struct PairsParams {
  const unsigned* masks; const int* sel; const int* nsel; const int* gt;
  int K, H, W, C, t_cap, cap;
  int* area_t; int* area_p; int* trips; int* counters;
};

// counts of the ground-truth rows of a tile: area_t[b][t] += pixels with value t + 1 in any channel (zeroed by the launcher)
__global__ __launch_bounds__(256) void eval_area_t_kernel(PairsParams p) {
  extern __shared__ int hist[];
  const int b = blockIdx.y, tid = threadIdx.x;
  for (int t = tid; t < p.t_cap; t += 256) hist[t] = 0;
  __syncthreads();
  const long long total = (long long)p.H * p.W * p.C;
  const int* g = p.gt + (long long)b * total;
  bool bad = false;
  for (long long i = (long long)blockIdx.x * 256 + tid; i < total; i += (long long)gridDim.x * 256) {
    const int t = g[i];
    if (t > 0 && t <= p.t_cap) atomicAdd(&hist[t - 1], 1);
    else if (t != 0) bad = true;
  }
  if (bad) atomicOr(&p.counters[2], 1);
  __syncthreads();
  for (int t = tid; t < p.t_cap; t += 256)
    if (hist[t]) atomicAdd(&p.area_t[(long long)b * p.t_cap + t], hist[t]);
}

// one workgroup per (selected prediction q, tile b)
__global__ __launch_bounds__(256) void eval_pairs_kernel(PairsParams p) {
  extern __shared__ int hist[];
  __shared__ int s_area, s_cnt, s_base;
  const int b = blockIdx.y, q = blockIdx.x, tid = threadIdx.x;
  const int n = min(max(p.nsel[b], 0), p.K);
  if (q >= n) return;
  const int slot = p.sel[(long long)b * p.K + q];
  if (slot < 0 || slot >= p.K) {
    if (tid == 0) atomicOr(&p.counters[2], 1);
    return;
  }
  for (int t = tid; t < p.t_cap; t += 256) hist[t] = 0;
  if (tid == 0) { s_area = 0; s_cnt = 0; }
  __syncthreads();
  const int wpr = p.W >> 5, words = p.H * wpr;
  const unsigned* m = p.masks + ((long long)b * p.K + slot) * words;
  const int* g = p.gt + (long long)b * p.H * p.W * p.C;
  int area = 0;
  bool bad = false;
  for (int wv = tid; wv < words; wv += 256) {
    unsigned v = m[wv];
    if (!v) continue;
    area += __popc(v);
    const int y = wv / wpr, x0 = (wv - y * wpr) << 5;
    while (v) {
      const int bit = __ffs((int)v) - 1;
      v &= v - 1;
      const int* gp = g + ((long long)y * p.W + x0 + bit) * p.C;
      for (int c = 0; c < p.C; ++c) {
        const int t = gp[c];
        if (t > 0 && t <= p.t_cap) atomicAdd(&hist[t - 1], 1);
        else if (t != 0) bad = true;
      }
    }
  }
  if (area) atomicAdd(&s_area, area);
  if (bad) atomicOr(&p.counters[2], 1);
  __syncthreads();
  if (tid == 0) p.area_p[(long long)b * p.K + q] = s_area;
  emit_nonempty<256>(p.t_cap, p.cap, p.counters, &s_cnt, &s_base, [&](int t) { return hist[t] != 0; },
                     [&](int t, int off) {
                       int* o = p.trips + (long long)off * 4;
                       o[0] = b; o[1] = t; o[2] = q; o[3] = hist[t];
                     });
}

struct RenderParams {
  const unsigned* masks; const int* sel; const int* nsel; const int* labels;
  int K, H, W, C, format;
  int* out;
};

__global__ __launch_bounds__(256) void eval_render_kernel(RenderParams p) {
  __shared__ short s_slot[EV_MAXK];
  __shared__ short s_val[EV_MAXK];
  __shared__ int s_lab[EV_MAXK];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int n = min(max(p.nsel[b], 0), p.K);
  for (int i = tid; i < n; i += 256) {
    const int slot = p.sel[(long long)b * p.K + i];
    const bool ok = slot >= 0 && slot < p.K;
    s_slot[i] = ok ? (short)slot : (short)-1;      // (a slot outside the tile paints nothing)
    s_lab[i] = ok ? p.labels[(long long)b * p.K + slot] : -1;
    s_val[i] = (short)(i + 1);
  }
  __syncthreads();
  if (p.format == NUHTC_EVAL_PANNUKE) {
    // 1-based position of a prediction among those of its class; labels outside [0, C) get no channel
    if (tid < p.C) {
      int cnt = 0;
      for (int i = 0; i < n; ++i)
        if (s_lab[i] == tid) s_val[i] = (short)++cnt;
    }
    __syncthreads();
  }
  const int pix = blockIdx.x * 256 + tid;
  if (pix >= p.H * p.W) return;
  const int y = pix / p.W, x = pix - y * p.W;
  const int wpr = p.W >> 5, CO = p.format == NUHTC_EVAL_PANNUKE ? p.C + 1 : 2;
  int* o = p.out + ((long long)b * p.H * p.W + pix) * CO;
  for (int c = 0; c < CO; ++c) o[c] = 0;
  const unsigned* mw = p.masks + (long long)b * p.K * p.H * wpr + (long long)y * wpr + (x >> 5);
  int any = 0, last = 0, mx = 0;
  for (int i = 0; i < n; ++i) {
    const int slot = s_slot[i];
    if (slot < 0) continue;
    if (!((mw[(long long)slot * p.H * wpr] >> (x & 31)) & 1u)) continue;
    any = 1;
    const int lab = s_lab[i];
    if (p.format == NUHTC_EVAL_PANNUKE) {
      if (lab >= 0 && lab < p.C) o[lab] = s_val[i];      // later instances win: their index within the class is larger
    } else {
      last = i + 1;
      mx = max(mx, lab + 1);
    }
  }
  if (p.format == NUHTC_EVAL_PANNUKE) o[p.C] = n > 0 ? 1 - any : 0;   // (`convert_format` returns all zeros for an image without predictions)
  else { o[0] = last; o[1] = mx; }
}

struct JointParams {
  const int* tmap; const int* pmap;
  int Ct, Cp, H, W, C, cap;
  int* joint; int* counters;
};

__device__ __forceinline__ bool joint_insert(unsigned long long* keys, int* cnt, unsigned long long key, int add) {
  unsigned h = (unsigned)((key * 0x9E3779B97F4A7C15ull) >> 52) & (EJ_SLOTS - 1);
  for (int probe = 0; probe < EJ_SLOTS; ++probe) {
    const unsigned long long prev = atomicCAS(&keys[h], ~0ull, key);
    if (prev == ~0ull || prev == key) { atomicAdd(&cnt[h], add); return true; }
    h = (h + 1) & (EJ_SLOTS - 1);
  }
  return false;
}

// id of a pixel in the map `binarize` makes of C channels: the last non-zero channel wins; 0 = background
__device__ __forceinline__ int bin_id(const int* v, int C, bool& bad) {
  for (int c = C - 1; c >= 0; --c) {
    const int x = v[c];
    if (x > 0 && x < (1 << EJ_CLASS_SHIFT)) return (c << EJ_CLASS_SHIFT) | x;
    if (x != 0) bad = true;
  }
  return 0;
}

// one workgroup per (table k, tile b): k < C the maps of class k, k == C the binarised maps
__global__ __launch_bounds__(EJ_NT) void eval_joint_kernel(JointParams p) {
  __shared__ unsigned long long keys[EJ_SLOTS];
  __shared__ int cnt[EJ_SLOTS];
  __shared__ int s_cnt, s_base, s_full;
  const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  for (int i = tid; i < EJ_SLOTS; i += EJ_NT) { keys[i] = ~0ull; cnt[i] = 0; }
  if (tid == 0) { s_cnt = 0; s_full = 0; }
  __syncthreads();
  const int HW = p.H * p.W;
  const int* tm = p.tmap + (long long)b * HW * p.Ct;
  const int* pm = p.pmap + (long long)b * HW * p.Cp;
  int zz = 0;
  bool bad = false, full = false;
  for (int pix = tid; pix < HW; pix += EJ_NT) {
    if (*(volatile int*)&s_full) break;      // the table is full and the batch flagged: no further pixel walks all its slots
    int t, q;
    if (k < p.C) {
      t = tm[(long long)pix * p.Ct + k];
      q = pm[(long long)pix * p.Cp + k];
      if (t < 0) { bad = true; t = 0; }
      if (q < 0) { bad = true; q = 0; }
    } else {
      t = bin_id(tm + (long long)pix * p.Ct, p.C, bad);
      q = bin_id(pm + (long long)pix * p.Cp, p.C, bad);
    }
    if (!(t | q)) { ++zz; continue; }
    if (!joint_insert(keys, cnt, ((unsigned long long)(unsigned)t << 32) | (unsigned)q, 1)) { full = true; s_full = 1; }
  }
  if (zz && !*(volatile int*)&s_full && !joint_insert(keys, cnt, 0ull, zz)) full = true;
  if (bad) atomicOr(&p.counters[2], 1);
  if (full) atomicOr(&p.counters[1], 1);
  __syncthreads();
  emit_nonempty<EJ_NT>(EJ_SLOTS, p.cap, p.counters, &s_cnt, &s_base, [&](int i) { return keys[i] != ~0ull; },
                       [&](int i, int off) {
                         int* o = p.joint + (long long)off * 5;
                         o[0] = b; o[1] = k; o[2] = (int)(keys[i] >> 32); o[3] = (int)(keys[i] & 0xFFFFFFFFull); o[4] = cnt[i];
                       });
}

int launch_select(const SelectParams& p, int B, hipStream_t s) {
  ProfScope ps("eval_select", 0, 0, s);
  hipLaunchKernelGGL(eval_select_kernel, dim3(B), dim3(ES_NT), 0, s, p);
  return launched() ? 0 : NUHTC_E_HIP;
}

// `counters` [4]: [0] entries the list needs, [1] entries were dropped (capacity), [2] a map value or slot was out of range
int launch_pairs(const PairsParams& p, int B, hipStream_t s) {
  ProfScope ps("eval_pairs", 0, 0, s);
  if (hipMemsetAsync(p.counters, 0, 4 * sizeof(int), s) != hipSuccess ||
      hipMemsetAsync(p.area_t, 0, (size_t)B * p.t_cap * sizeof(int), s) != hipSuccess ||
      hipMemsetAsync(p.area_p, 0, (size_t)B * p.K * sizeof(int), s) != hipSuccess)
    return NUHTC_E_HIP;
  const size_t lds = (size_t)p.t_cap * sizeof(int);
  const int chunks = std::max(1, std::min(64, cdiv(p.H * p.W * p.C, 256 * 16)));
  hipLaunchKernelGGL(eval_area_t_kernel, dim3(chunks, B), dim3(256), lds, s, p);
  hipLaunchKernelGGL(eval_pairs_kernel, dim3(p.K, B), dim3(256), lds, s, p);
  return launched() ? 0 : NUHTC_E_HIP;
}

int launch_render(const RenderParams& p, int B, hipStream_t s) {
  ProfScope ps("eval_render", 0, 0, s);
  hipLaunchKernelGGL(eval_render_kernel, dim3(cdiv(p.H * p.W, 256), B), dim3(256), 0, s, p);
  return launched() ? 0 : NUHTC_E_HIP;
}

int launch_joint(const JointParams& p, int B, hipStream_t s) {
  ProfScope ps("eval_joint", 0, 0, s);
  if (hipMemsetAsync(p.counters, 0, 4 * sizeof(int), s) != hipSuccess) return NUHTC_E_HIP;
  hipLaunchKernelGGL(eval_joint_kernel, dim3(p.C + 1, B), dim3(EJ_NT), 0, s, p);
  return launched() ? 0 : NUHTC_E_HIP;
}

// the geometry every entry point shares; nullptr when it is fine
const char* bad_geometry(int B, int K, int H, int W, int C) {
  if (B < 1 || B > 4096) return "eval: B out of range (1..4096)";
  if (K < 1 || K > EV_MAXK) return "eval: K out of range (1..2048)";
  if (H < 1 || W < 32 || W % 32 || H > 32767 || W > 32767 * 32 || (long long)H * W > (1ll << 26)) return "eval: W must be a multiple of 32 and H x W at most 2^26";
  if (C < 1 || C > 14) return "eval: C out of range (1..14)";
  return nullptr;
}

}  // namespace

extern "C" {

int nuhtc_op_eval_select(nuhtc_engine* e, const float* scores, int score_stride, const int32_t* counts, const uint32_t* masks, const int32_t* labels,
                         int B, int K, int H, int W, float fg_thr, double thr, int32_t* sel, int32_t* nsel, int32_t* sel_labels, void* stream) {
  if (!e || !scores || !counts || !masks || !sel || !nsel) return NUHTC_E_INVALID;
  if (const char* m = bad_geometry(B, K, H, W, 1)) FAIL(e, NUHTC_E_INVALID, m);
  if (score_stride < 1) FAIL(e, NUHTC_E_INVALID, "eval_select op: score_stride must be positive");
  HIP_CHECK(e, hipSetDevice(e->device));
  hipStream_t s = (hipStream_t)stream;
  SelectParams p{scores, score_stride, counts, masks, labels, K, H, W, fg_thr, thr, sel, nsel, sel_labels};
  return op_finish(e, launch_select(p, B, s), s, "eval_select launch failed", "eval_select kernel failed");
}

int nuhtc_op_eval_pairs(nuhtc_engine* e, const uint32_t* masks, const int32_t* sel, const int32_t* nsel, const int32_t* gt_maps, int B, int K, int H,
                        int W, int C, int t_cap, int cap, int32_t* area_t, int32_t* area_p, int32_t* trips, int32_t* counters, void* stream) {
  if (!e || !masks || !sel || !nsel || !gt_maps || !area_t || !area_p || !trips || !counters) return NUHTC_E_INVALID;
  if (const char* m = bad_geometry(B, K, H, W, C)) FAIL(e, NUHTC_E_INVALID, m);
  if (t_cap < 1 || t_cap > EV_MAX_TCAP || cap < 1) FAIL(e, NUHTC_E_INVALID, "eval_pairs op: t_cap (1..8192) / cap out of range");
  HIP_CHECK(e, hipSetDevice(e->device));
  hipStream_t s = (hipStream_t)stream;
  PairsParams p{masks, sel, nsel, gt_maps, K, H, W, C, t_cap, cap, area_t, area_p, trips, counters};
  return op_finish(e, launch_pairs(p, B, s), s, "eval_pairs launch failed", "eval_pairs kernel failed");
}

int nuhtc_op_eval_render(nuhtc_engine* e, const uint32_t* masks, const int32_t* sel, const int32_t* nsel, const int32_t* labels, int B, int K, int H,
                         int W, int C, int format, int32_t* out, void* stream) {
  if (!e || !masks || !sel || !nsel || !labels || !out) return NUHTC_E_INVALID;
  if (const char* m = bad_geometry(B, K, H, W, C)) FAIL(e, NUHTC_E_INVALID, m);
  if (format != NUHTC_EVAL_PANNUKE && format != NUHTC_EVAL_CONIC) FAIL(e, NUHTC_E_INVALID, "eval_render op: unknown format");
  HIP_CHECK(e, hipSetDevice(e->device));
  hipStream_t s = (hipStream_t)stream;
  RenderParams p{masks, sel, nsel, labels, K, H, W, C, format, out};
  return op_finish(e, launch_render(p, B, s), s, "eval_render launch failed", "eval_render kernel failed");
}

int nuhtc_op_eval_joint(nuhtc_engine* e, const int32_t* true_maps, int Ct, const int32_t* pred_maps, int Cp, int B, int H, int W, int C, int cap,
                        int32_t* joint, int32_t* counters, void* stream) {
  if (!e || !true_maps || !pred_maps || !joint || !counters) return NUHTC_E_INVALID;
  if (B < 1 || B > 4096 || H < 1 || W < 1 || (long long)H * W > (1ll << 26) || C < 1 || C > 14 || Ct < C || Cp < C || cap < 1)
    FAIL(e, NUHTC_E_INVALID, "eval_joint op: size out of range (C 1..14 <= Ct, Cp; H x W at most 2^26)");
  HIP_CHECK(e, hipSetDevice(e->device));
  hipStream_t s = (hipStream_t)stream;
  JointParams p{true_maps, pred_maps, Ct, Cp, H, W, C, cap, joint, counters};
  return op_finish(e, launch_joint(p, B, s), s, "eval_joint launch failed", "eval_joint kernel failed");
}

int nuhtc_eval_batch(nuhtc_engine* e, const nuhtc_dets* dets, int B, const nuhtc_eval_args* a, void* stream) {
  if (!e) return NUHTC_E_INVALID;
  if (!dets || !dets->boxes || !dets->labels || !dets->counts || !dets->masks || !a || !a->sel || !a->nsel || !a->sel_labels || !a->counters)
    FAIL(e, NUHTC_E_INVALID, "bad nuhtc_eval_batch arguments");
  const nuhtc_config& c = e->cfg;
  if (B < 1 || B > c.max_batch) FAIL(e, NUHTC_E_INVALID, "nuhtc_eval_batch: B out of range");
  if (const char* m = bad_geometry(B, c.max_per_img, c.tile_h, c.tile_w, c.num_classes)) FAIL(e, NUHTC_E_INVALID, m);
  if (a->format != NUHTC_EVAL_PANNUKE && a->format != NUHTC_EVAL_CONIC) FAIL(e, NUHTC_E_INVALID, "nuhtc_eval_batch: unknown format");
  const bool joint = a->gt_maps && a->pred_maps && a->joint && a->format == NUHTC_EVAL_PANNUKE;
  if (a->gt_maps && (!a->area_t || !a->area_p || !a->trips || a->t_cap < 1 || a->t_cap > EV_MAX_TCAP || a->trip_cap < 1 || (joint && a->joint_cap < 1)))
    FAIL(e, NUHTC_E_INVALID, "nuhtc_eval_batch: ground truth given without its output tables (t_cap 1..8192)");
  HIP_CHECK(e, hipSetDevice(e->device));
  hipStream_t s = (hipStream_t)stream;
  const int K = c.max_per_img, H = c.tile_h, W = c.tile_w, C = c.num_classes;
  HIP_CHECK(e, hipMemsetAsync(a->counters, 0, 8 * sizeof(int32_t), s));
  SelectParams sp{dets->boxes + 4, 5, dets->counts, dets->masks, dets->labels, K, H, W, a->fg_thr, a->mask_nms_thr, a->sel, a->nsel, a->sel_labels};
  RUN(launch_select(sp, B, s));
  if (a->gt_maps) {
    PairsParams pp{dets->masks, a->sel, a->nsel, a->gt_maps, K, H, W, C, a->t_cap, a->trip_cap, a->area_t, a->area_p, a->trips, a->counters};
    RUN(launch_pairs(pp, B, s));
  }
  if (a->pred_maps) {
    RenderParams rp{dets->masks, a->sel, a->nsel, dets->labels, K, H, W, C, a->format, a->pred_maps};
    RUN(launch_render(rp, B, s));
  }
  if (joint) {
    JointParams jp{a->gt_maps, a->pred_maps, C, C + 1, H, W, C, a->joint_cap, a->joint, a->counters + 4};
    RUN(launch_joint(jp, B, s));
  }
  return 0;
}

}  // extern "C"
