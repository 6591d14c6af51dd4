// libnuhtc_hip.so — C ABI (include/nuhtc_hip.h), weight packing, workspace and the launch sequence of the
// htc_lite_swin tile-inference path (reference call stack: SURVEY §3.3; nuhtc/models/htc_cus.py:110-121,
// nuhtc/models/htc_roi_head_cus.py:2184-2372).  Host code only enqueues kernels; there is no CPU fallback.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "common.h"
#include "engine.h"

// =============================================================================== small helpers
static const int DEPTHS[4] = {2, 2, 6, 2};
static const int NHEADS[4] = {3, 6, 12, 24};

static thread_local std::string g_create_error;

void nuhtc_default_config(nuhtc_config* c) {
  memset(c, 0, sizeof(*c));
  c->abi_version = NUHTC_ABI_VERSION;
  c->num_classes = 5;
  c->tile_h = c->tile_w = 256;
  c->max_batch = 16;
  c->scale_factor = 2.0f;
  const float mean[3] = {123.675f, 116.28f, 103.53f}, std[3] = {58.395f, 57.12f, 57.375f};
  for (int i = 0; i < 3; ++i) { c->mean[i] = mean[i]; c->std[i] = std[i]; }
  c->rpn_nms_pre = 3000; c->rpn_max_per_img = 1000; c->rpn_nms_iou = 0.7f; c->rpn_min_bbox_size = 10.f;
  c->score_thr = 0.35f; c->nms_iou = 0.5f; c->max_per_img = 500; c->mask_thr_binary = 0.5f;
  c->att_thres = 0.965926f;
  c->watershed_proposal = 1;
  c->max_cc_proposals = 512;
  const float st[3][4] = {{0.1f, 0.1f, 0.2f, 0.2f}, {0.05f, 0.05f, 0.1f, 0.1f}, {0.033f, 0.033f, 0.067f, 0.067f}};
  memcpy(c->stage_stds, st, sizeof(st));
  c->margin = 2; c->min_area = 10; c->mask_nms_thr = 0.05f;
  c->matrix_pipe = NUHTC_PIPE_BF16_SPLIT;
  c->schedule = NUHTC_SCHED_LATENCY;
  c->att_pool_fp16 = 0;
  c->features_only = 0;
}

// ---- the front of the path, host side: what nuhtc_create / nuhtc_finalize / run_backbone and nuhtc_op_patch_embed share
// the per-axis factors new / old (mmdet Resize: w_scale, h_scale) must both equal scale_factor, i.e. scale * size is an integer
static bool resize_ok(int vh, int vw, float scale) {
  const double sh = (double)vh * scale, sw = (double)vw * scale;
  return scale >= 1.0f && scale <= 8.0f && sh == floor(sh) && sw == floor(sw);
}
// img_shape (Hv, Wv) = mmcv.rescale_size of the valid image, pad_shape (Hn, Wn) = Pad(size_divisor=32) of it, and cv2's per-axis tables
struct ResizeGeom {
  int Hv, Wv, Hn, Wn;
  std::vector<int> tx, ty;
};
static ResizeGeom resize_geom(int vh, int vw, float scale) {
  ResizeGeom r;
  r.Hv = (int)(vh * (double)scale + 0.5); r.Wv = (int)(vw * (double)scale + 0.5);
  r.Hn = (r.Hv + 31) / 32 * 32; r.Wn = (r.Wv + 31) / 32 * 32;
  cv_linear_tables(vw, r.Wv, true, r.tx);
  cv_linear_tables(vh, r.Hv, false, r.ty);
  return r;
}
// Normalize's constants as the kernels take them: mean[3], then 1 / std[3] (mmcv.imnormalize multiplies by the float64 reciprocal)
static void norm_consts(const float mean[3], const float std[3], float mi[6]) {
  for (int i = 0; i < 3; ++i) { mi[i] = mean[i]; mi[3 + i] = (float)(1.0 / (double)std[i]); }
}
// patch embedding weight [96][3][4][4] -> [48][96], k = (kh*4+kw)*3 + c
static std::vector<float> pack_patch_embed(const float* w) {
  std::vector<float> p(48 * 96);
  for (int o = 0; o < 96; ++o)
    for (int ch = 0; ch < 3; ++ch)
      for (int kh = 0; kh < 4; ++kh)
        for (int kw = 0; kw < 4; ++kw) p[((kh * 4 + kw) * 3 + ch) * 96 + o] = w[((o * 3 + ch) * 4 + kh) * 4 + kw];
  return p;
}

const char* nuhtc_last_error(const nuhtc_engine* e) { return e ? e->err.c_str() : g_create_error.c_str(); }

int nuhtc_create(const nuhtc_config* cfg, int device, nuhtc_engine** out) {
  if (!cfg || !out) { g_create_error = "null argument"; return NUHTC_E_INVALID; }
  if (cfg->abi_version != NUHTC_ABI_VERSION) { g_create_error = "abi_version mismatch"; return NUHTC_E_INVALID; }
  if (cfg->tile_h <= 0 || cfg->tile_w <= 0 || cfg->tile_w % 32) { g_create_error = "tile_h / tile_w must be positive and tile_w a multiple of 32 (bit-packed mask rows)"; return NUHTC_E_INVALID; }
  if (cfg->valid_h < 0 || cfg->valid_w < 0 || cfg->valid_h > cfg->tile_h || cfg->valid_w > cfg->tile_w) { g_create_error = "valid_h / valid_w must lie in [0, tile] (0 = the whole tile)"; return NUHTC_E_INVALID; }
  {
    // resized image = mmcv.rescale_size: int(size*scale + 0.5); the per-axis factors new/old (mmdet Resize: w_scale, h_scale) must
    // both equal scale_factor, i.e. scale*size is an integer.  Pad(size_divisor=32) then rounds the network input up.
    const int vh = cfg->valid_h ? cfg->valid_h : cfg->tile_h, vw = cfg->valid_w ? cfg->valid_w : cfg->tile_w;
    if (!resize_ok(vh, vw, cfg->scale_factor)) {
      g_create_error = "scale_factor (80/mag) must be in [1,8] and scale_factor * image size must be integers";
      return NUHTC_E_INVALID;
    }
    if ((double)vh * cfg->scale_factor < 32 || (double)vw * cfg->scale_factor < 32) { g_create_error = "the resized image must be at least 32 x 32"; return NUHTC_E_INVALID; }
  }
  // class logits live in rows of 16 floats: num_classes + 2 (objectness pair) values per RoI, see bbox_tail_kernel
  if (cfg->num_classes < 1 || cfg->num_classes > 14) { g_create_error = "num_classes out of range (1..14)"; return NUHTC_E_INVALID; }
  if (cfg->max_batch < 1 || cfg->max_batch > 256) { g_create_error = "max_batch out of range"; return NUHTC_E_INVALID; }
  if (cfg->rpn_nms_pre < 1 || cfg->rpn_nms_pre > 4096 || cfg->rpn_max_per_img < 1 || cfg->rpn_max_per_img > 4096) { g_create_error = "rpn_nms_pre / rpn_max_per_img out of range (<=4096)"; return NUHTC_E_INVALID; }
  if (cfg->max_per_img < 1 || cfg->max_per_img > 2048) { g_create_error = "max_per_img out of range"; return NUHTC_E_INVALID; }
  if (cfg->max_cc_proposals < 0 || cfg->max_cc_proposals > 4096) { g_create_error = "max_cc_proposals out of range"; return NUHTC_E_INVALID; }
  if (cfg->schedule != NUHTC_SCHED_LATENCY && cfg->schedule != NUHTC_SCHED_THROUGHPUT) { g_create_error = "schedule must be NUHTC_SCHED_LATENCY or NUHTC_SCHED_THROUGHPUT"; return NUHTC_E_INVALID; }
  if (cfg->att_pool_fp16 != 0 && cfg->att_pool_fp16 != 1) { g_create_error = "att_pool_fp16 must be 0 or 1"; return NUHTC_E_INVALID; }
  if (cfg->features_only != 0 && cfg->features_only != 1) { g_create_error = "features_only must be 0 or 1"; return NUHTC_E_INVALID; }
  if (cfg->matrix_pipe != NUHTC_PIPE_BF16_SPLIT && cfg->matrix_pipe != NUHTC_PIPE_FP32) { g_create_error = "matrix_pipe must be NUHTC_PIPE_BF16_SPLIT or NUHTC_PIPE_FP32"; return NUHTC_E_INVALID; }
  {
    const char* probes[4] = {nuhtc_tu_probe_conv(), nuhtc_tu_probe_gemm(), nuhtc_tu_probe_mlp(), nuhtc_tu_probe_swin()};
    const char* dev = getenv("NUHTC_DEV");
    for (const char* pr : probes)
      if (pr && !(dev && dev[0] == '1')) {
        g_create_error = std::string("this library was compiled with the result-altering dev probe ") + pr + " (wrong results by design); rebuild without it, or set NUHTC_DEV=1 for a timing experiment";
        return NUHTC_E_STATE;
      }
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { g_create_error = "no such HIP device"; return NUHTC_E_HIP; }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) { g_create_error = "hipGetDeviceProperties failed"; return NUHTC_E_HIP; }
  if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos) { g_create_error = std::string("this library is built for gfx950 only, device is ") + prop.gcnArchName; return NUHTC_E_INVALID; }
  nuhtc_engine* e = new nuhtc_engine();
  e->cfg = *cfg;
  e->device = device;
  *out = e;
  return 0;
}

// The three streams of an engine (the one handed out by nuhtc_stream + two side streams) live for the whole process: a closed
// engine returns them to a per-device pool and the next engine takes them over.  The stream handed out may be in use by the
// caller's allocator after the engine is gone (PyTorch's caching allocator records events on the stream a block was allocated
// on when the block is freed: a destroyed stream there is a segmentation fault), and a pooled triple keeps the placement it was
// created with (see nuhtc_finalize).
struct StreamTriple { hipStream_t own, side, side2; };
static std::mutex g_stream_mu;
static std::map<int, std::vector<StreamTriple>> g_stream_pool;

void nuhtc_destroy(nuhtc_engine* e) {
  if (!e) return;
  hipSetDevice(e->device);
  hipDeviceSynchronize();
  if (e->own && e->side && e->side2) {
    std::lock_guard<std::mutex> lock(g_stream_mu);
    g_stream_pool[e->device].push_back(StreamTriple{e->own, e->side, e->side2});
  } else {
    if (e->side) hipStreamDestroy(e->side);
    if (e->side2) hipStreamDestroy(e->side2);
  }
  if (e->ev_side2) hipEventDestroy(e->ev_side2);
  if (e->ev_rpn) hipEventDestroy(e->ev_rpn);
  if (e->ev_side) hipEventDestroy(e->ev_side);
  if (e->ev_fpn) hipEventDestroy(e->ev_fpn);
  if (e->overflow_host) hipHostFree(e->overflow_host);
  for (void* p : e->allocs) hipFree(p);
  delete e;
}

void* nuhtc_stream(nuhtc_engine* e) { return e ? (void*)e->own : nullptr; }

// Names and shapes of the state_dict entries the path reads (the same table as nuhtc_amd/weights.py:schema).
static std::map<std::string, std::vector<int64_t>> weight_schema(int nc) {
  std::map<std::string, std::vector<int64_t>> s;
  auto wb = [&](const std::string& p, std::vector<int64_t> w) { s[p + ".weight"] = w; s[p + ".bias"] = {w[0]}; };
  wb("backbone.patch_embed.projection", {96, 3, 4, 4});
  s["backbone.patch_embed.norm.weight"] = {96}; s["backbone.patch_embed.norm.bias"] = {96};
  for (int st = 0; st < 4; ++st) {
    const int64_t C = 96 << st;
    for (int b = 0; b < DEPTHS[st]; ++b) {
      const std::string p = "backbone.stages." + std::to_string(st) + ".blocks." + std::to_string(b) + ".";
      s[p + "norm1.weight"] = {C}; s[p + "norm1.bias"] = {C}; s[p + "norm2.weight"] = {C}; s[p + "norm2.bias"] = {C};
      s[p + "attn.w_msa.relative_position_bias_table"] = {169, NHEADS[st]};
      wb(p + "attn.w_msa.qkv", {3 * C, C}); wb(p + "attn.w_msa.proj", {C, C});
      wb(p + "ffn.layers.0.0", {4 * C, C}); wb(p + "ffn.layers.1", {C, 4 * C});
    }
    if (st < 3) {
      const std::string p = "backbone.stages." + std::to_string(st) + ".downsample.";
      s[p + "norm.weight"] = {4 * C}; s[p + "norm.bias"] = {4 * C}; s[p + "reduction.weight"] = {2 * C, 4 * C};
    }
    s["backbone.norm" + std::to_string(st) + ".weight"] = {C}; s["backbone.norm" + std::to_string(st) + ".bias"] = {C};
    wb("neck.lateral_convs." + std::to_string(st) + ".conv", {64, C, 1, 1});
    wb("neck.fpn_convs." + std::to_string(st) + ".conv", {64, 64, 3, 3});
    wb("roi_head.semantic_head.lateral_convs." + std::to_string(st) + ".conv", {64, 64, 1, 1});
    wb("roi_head.semantic_head.convs." + std::to_string(st) + ".conv", {64, 64, 3, 3});
    wb("roi_head.mask_head.0.convs." + std::to_string(st) + ".conv", {64, 64, 3, 3});
  }
  wb("rpn_head.rpn_conv", {64, 64, 3, 3}); wb("rpn_head.rpn_cls", {3, 64, 1, 1}); wb("rpn_head.rpn_reg", {12, 64, 1, 1});
  for (int k = 0; k < 3; ++k) {
    const std::string p = "roi_head.bbox_head." + std::to_string(k) + ".";
    wb(p + "shared_fcs.0", {256, 3136}); wb(p + "shared_fcs.1", {256, 256}); wb(p + "fc_cls", {nc + 2, 256}); wb(p + "fc_reg", {4, 256});
  }
  wb("roi_head.mask_head.0.upsample", {64, 64, 2, 2}); wb("roi_head.mask_head.0.conv_logits", {1, 64, 1, 1});
  wb("roi_head.mask_head.0.conv_res.conv", {64, 64, 1, 1});   // unused at test time (res_feat is None), accepted
  wb("roi_head.semantic_head.conv_embedding.conv", {64, 64, 1, 1}); wb("roi_head.semantic_head.conv_logits", {1, 64, 1, 1});
  return s;
}

int nuhtc_load_weight(nuhtc_engine* e, const char* name, const float* host, const int64_t* shape, int ndim) {
  if (!e) return NUHTC_E_INVALID;
  if (!name || !host || !shape) FAIL(e, NUHTC_E_INVALID, "nuhtc_load_weight: null argument");
  if (ndim < 1 || ndim > 4) FAIL(e, NUHTC_E_INVALID, std::string("nuhtc_load_weight: ") + name + ": ndim must be 1..4");
  if (e->finalized) FAIL(e, NUHTC_E_STATE, "load_weight after finalize");
  if (e->schema.empty()) e->schema = weight_schema(e->cfg.num_classes);
  auto it = e->schema.find(name);
  if (it == e->schema.end()) FAIL(e, NUHTC_E_NOTFOUND, std::string("nuhtc_load_weight: unknown weight name: ") + name);
  HostTensor t;
  size_t n = 1;
  for (int i = 0; i < ndim; ++i) { t.shape.push_back(shape[i]); n *= (size_t)shape[i]; }
  if (t.shape != it->second) FAIL(e, NUHTC_E_INVALID, std::string("nuhtc_load_weight: bad shape for ") + name);
  // a features-only engine keeps the backbone and the neck: the heads' tensors of a full checkpoint are accepted and dropped
  if (e->cfg.features_only && strncmp(name, "backbone.", 9) != 0 && strncmp(name, "neck.", 5) != 0) return 0;
  t.data.assign(host, host + n);
  e->raw[name] = std::move(t);
  return 0;
}

// =============================================================================== device allocation
int dev_alloc(nuhtc_engine* e, void** p, size_t bytes) {
  bytes = (bytes + 255) & ~(size_t)255;
  if (bytes == 0) bytes = 256;
  HIP_CHECK(e, hipMalloc(p, bytes));
  e->allocs.push_back(*p);
  return 0;
}

int upload_bytes(nuhtc_engine* e, void** dst, const void* host, size_t bytes) {
  int rc = dev_alloc(e, dst, bytes);
  if (rc) return rc;
  HIP_CHECK(e, hipMemcpy(*dst, host, bytes, hipMemcpyHostToDevice));
  return 0;
}

int upload_gemm_weight(nuhtc_engine* e, float** dst, const std::vector<float>& v, int N, int K) {
  int rc = upload(e, dst, v);
  if (rc) return rc;
  if (e->cfg.matrix_pipe == NUHTC_PIPE_FP32) return 0;
  if ((size_t)N * K != v.size()) FAIL(e, NUHTC_E_INVALID, "upload_gemm_weight: shape mismatch");
  std::vector<unsigned short> split;
  rc = gemm_make_split(v.data(), N, K, split);
  if (rc) FAIL(e, rc, "gemm_make_split failed");
  void* sp = nullptr;
  if ((rc = upload_bytes(e, &sp, split.data(), split.size() * 2))) return rc;
  e->wsplit[*dst] = {sp, N, K};
  return 0;
}

int egemm(nuhtc_engine* e, GemmParams p, hipStream_t s) {
  // products of depth < 96 stay on the fp32 MFMA kernel (4 k-tiles: prologue and epilogue dominate and the fp32 kernel keeps 4
  // workgroups per CU; measured 0.28 vs 0.32-0.40 ms per step for the 64x64 pointwise layers), batched products too
  if (!p.Wsplit && p.batch <= 1 && p.K >= 96) {
    auto it = e->wsplit.find(p.W);
    if (it != e->wsplit.end()) {
      // a split of another geometry under this pointer would be read out of bounds by the kernel, silently: refuse it (the first
      // rows of a weight with the same K are a valid product: the split is row-major in n)
      if (it->second.K != p.K || p.N > it->second.N) FAIL(e, NUHTC_E_STATE, "egemm: the weight's bf16 split was made for another [N][K]");
      p.Wsplit = it->second.planes;
    }
  }
  {   // dev: ablation of the step (tools/dev/r04_ablate.py): 4 = 3x3 convolutions, 8 = 96-column split GEMMs, 64 = every other product
    static const int& skip_ = dev_knob_ref("SKIP", 0);
    if (skip_ && (p.amode == A_CONV3 ? (skip_ & 4) : (p.Wsplit && p.N % 96 == 0) ? (skip_ & 8) : (skip_ & 64))) return 0;
  }
  return launch_gemm(p, s);
}

static int upload_fuse(nuhtc_engine* e, void** dst, const std::vector<float>& w, int N2) {
  *dst = nullptr;
  if (e->cfg.matrix_pipe != NUHTC_PIPE_BF16_SPLIT) return 0;
  if (w.size() != (size_t)N2 * 64) FAIL(e, NUHTC_E_INVALID, "upload_fuse: shape mismatch");
  std::vector<unsigned short> img;
  const int rc = conv3_pack_fuse(w.data(), N2, img);
  if (rc) FAIL(e, rc, "conv3_pack_fuse failed");
  return upload_bytes(e, dst, img.data(), img.size() * 2);
}

const HostTensor* raw(nuhtc_engine* e, const std::string& name, std::initializer_list<int64_t> shape) {
  auto it = e->raw.find(name);
  if (it == e->raw.end()) { e->err = "missing weight: " + name; return nullptr; }
  std::vector<int64_t> s(shape);
  if (it->second.shape != s) { e->err = "bad shape for weight: " + name; return nullptr; }
  return &it->second;
}

std::vector<float> pack_conv3(const HostTensor& w, int O, int I) {
  std::vector<float> p((size_t)O * 9 * I);
  for (int o = 0; o < O; ++o)
    for (int i = 0; i < I; ++i)
      for (int t = 0; t < 9; ++t) p[((size_t)o * 9 + t) * I + i] = w.data[((size_t)o * I + i) * 9 + t];
  return p;
}

// =============================================================================== finalize
// window_attn_mfma_kernel reads the additive score terms (relative-position bias, shift mask) per lane: the lane of query i = 32 ti + l32
// in half-wave `half` needs, for key tile tj, the 16 accumulator registers r <-> key 32 tj + (r & 3) + 8 (r >> 2) + 4 half.  Packed
// as [ti][q][lane = 32 half + l32][4] with q = (16 tj + r) / 4 (4096 floats per 49 x 49 table): the q-th 16-byte load of a wave covers 1 KB of
// contiguous memory (round 4: with a lane's 32 floats contiguous, [ti][lane][32], every load instruction touched 64 different cache lines; the
// loads of a table that is the same for every window cost 0.08 of the launches' 0.66 ms per step, tools/dev/r04_attn_probe.sh).
static void pack_attn_terms(const float* qk /* [49][49] query-major */, float* out /* 4096 */) {
  for (int ti = 0; ti < 2; ++ti)
    for (int half = 0; half < 2; ++half)
      for (int l = 0; l < 32; ++l)
        for (int tj = 0; tj < 2; ++tj)
          for (int r = 0; r < 16; ++r) {
            const int i = ti * 32 + l, j = tj * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            const int f = tj * 16 + r, lane = half * 32 + l;
            out[ti * 2048 + ((f >> 2) * 64 + lane) * 4 + (f & 3)] = (i < WS2 && j < WS2) ? qk[i * WS2 + j] : 0.f;
          }
}

// The window geometry of a stage for B images of H x W tokens (mmdet/models/backbones/swin.py:182-226,254-283), host side: what
// build_stage_maps uploads for the engine and nuhtc_op_window_msa for one call.  g: H, W, Hp, Wp, nW set (stage_dims).
struct StageMaps {
  std::vector<int> map[2], cidx[2], ctok[2], vrow[2];   // see StageGeom, per shift state
  std::vector<int> padbits[2];        // 2 words per window of the image
  std::vector<float> mask;            // shift mask, packed per lane [nW][4096]
  std::vector<int> mask_any;          // [nW]
};

static void stage_dims(StageGeom& g, int H, int W, int C) {
  g.H = H; g.W = W; g.C = C; g.nH = C / 32;
  g.Hp = cdiv(H, WS) * WS; g.Wp = cdiv(W, WS) * WS;
  g.nW = (g.Hp / WS) * (g.Wp / WS);
}

static StageMaps stage_maps(const StageGeom& g, int B) {
  StageMaps o;
  // window-row -> token maps (un-shifted and shifted), (mmdet/models/backbones/swin.py:182-226,254-283)
  for (int sh = 0; sh < 2; ++sh) {
    std::vector<int>& m = o.map[sh];
    m.resize((size_t)B * g.nW * WS2);
    for (int b = 0; b < B; ++b)
      for (int wy = 0; wy < g.Hp / WS; ++wy)
        for (int wx = 0; wx < g.Wp / WS; ++wx)
          for (int py = 0; py < WS; ++py)
            for (int px = 0; px < WS; ++px) {
              int ys = wy * WS + py, xs = wx * WS + px;                        // coordinates in the rolled frame
              int y = sh ? (ys + 3) % g.Hp : ys, x = sh ? (xs + 3) % g.Wp : xs;  // roll(-3): rolled[ys] = padded[(ys+3) % Hp]
              size_t row = ((size_t)b * g.nW + (size_t)wy * (g.Wp / WS) + wx) * WS2 + py * WS + px;
              m[row] = (y < g.H && x < g.W) ? (b * g.H * g.W + y * g.W + x) : -1;
            }
    // the non-padding window rows in window order: the QKV / proj GEMMs run on these only (padding rows of the window
    // image hold the QKV bias, see launch_layernorm_windows)
    std::vector<int>&ci = o.cidx[sh], &ct = o.ctok[sh], &vr = o.vrow[sh];
    ci.resize(m.size());
    ct.reserve((size_t)B * g.H * g.W);
    vr.reserve((size_t)B * g.H * g.W);
    for (size_t r = 0; r < m.size(); ++r) {
      ci[r] = m[r] >= 0 ? (int)ct.size() : -1;
      if (m[r] >= 0) { ct.push_back(m[r]); vr.push_back((int)r); }
    }
    std::vector<int>& pb = o.padbits[sh];    // 49 bits per window of the image (tile 0's windows; every tile has the same)
    pb.assign((size_t)g.nW * 2, 0);
    for (int w = 0; w < g.nW; ++w)
      for (int j = 0; j < WS2; ++j)
        if (m[(size_t)w * WS2 + j] < 0) pb[(size_t)2 * w + (j >> 5)] |= 1 << (j & 31);
  }
  // shift mask on the padded grid (swin.py:197-218)
  std::vector<int> ids((size_t)g.Hp * g.Wp);
  auto region = [](int v, int n) { return v < n - WS ? 0 : (v < n - 3 ? 1 : 2); };
  for (int y = 0; y < g.Hp; ++y)
    for (int x = 0; x < g.Wp; ++x) ids[(size_t)y * g.Wp + x] = region(y, g.Hp) * 3 + region(x, g.Wp);
  std::vector<float> mask((size_t)g.nW * WS2 * WS2);
  for (int wy = 0; wy < g.Hp / WS; ++wy)
    for (int wx = 0; wx < g.Wp / WS; ++wx) {
      int w = wy * (g.Wp / WS) + wx;
      for (int p = 0; p < WS2; ++p)
        for (int q = 0; q < WS2; ++q) {
          int ip = ids[(size_t)(wy * WS + p / WS) * g.Wp + wx * WS + p % WS];
          int iq = ids[(size_t)(wy * WS + q / WS) * g.Wp + wx * WS + q % WS];
          mask[((size_t)w * WS2 + p) * WS2 + q] = ip == iq ? 0.f : -100.f;
        }
    }
  o.mask.resize((size_t)g.nW * 4096);
  o.mask_any.assign(g.nW, 0);
  for (int w = 0; w < g.nW; ++w) {
    pack_attn_terms(mask.data() + (size_t)w * WS2 * WS2, o.mask.data() + (size_t)w * 4096);
    for (int i = 0; i < WS2 * WS2; ++i)
      if (mask[(size_t)w * WS2 * WS2 + i] != 0.f) { o.mask_any[w] = 1; break; }
  }
  return o;
}

// StageMaps -> the device pointers of g through `up` (a host vector -> device copy, null on failure); the bias row sits behind the window
// image of B images
template <typename Up>
static bool upload_stage_maps(StageGeom& g, const StageMaps& m, int B, Up up) {
  bool ok = true;
  for (int sh = 0; sh < 2; ++sh) {
    ok &= (g.map[sh] = up(m.map[sh])) != nullptr;
    ok &= (g.cidx[sh] = up(m.cidx[sh])) != nullptr;
    ok &= (g.ctok[sh] = up(m.ctok[sh])) != nullptr;
    ok &= (g.vrow[sh] = up(m.vrow[sh])) != nullptr;
    ok &= (g.padbits[sh] = reinterpret_cast<unsigned long long*>(up(m.padbits[sh]))) != nullptr;
  }
  g.bias_row = B * g.nW * WS2;
  ok &= (g.brow = up(std::vector<int>(1, g.bias_row))) != nullptr;
  ok &= (g.mask = up(m.mask)) != nullptr;
  ok &= (g.mask_any = up(m.mask_any)) != nullptr;
  return ok;
}

static int build_stage_maps(nuhtc_engine* e, int s) {
  StageGeom& g = e->st[s];
  const int B = e->cfg.max_batch;
  int rc = 0;
  auto up = [&](const auto& v) {
    typename std::remove_const<typename std::remove_reference<decltype(v[0])>::type>::type* p = nullptr;
    if (!rc) rc = upload(e, &p, v);
    return rc ? nullptr : p;
  };
  upload_stage_maps(g, stage_maps(g, B), B, up);
  return rc;
}

// the relative-position bias table [169][nH] -> the per-lane packed terms of the attention kernel, [nH][4096] (pack_attn_terms)
static std::vector<float> pack_rel_bias(const float* tab, int nH) {
  std::vector<float> rb((size_t)nH * WS2 * WS2), rbT((size_t)nH * 4096);
  for (int a = 0; a < WS2; ++a)
    for (int b = 0; b < WS2; ++b) {
      const int rel = (a / WS - b / WS + WS - 1) * (2 * WS - 1) + (a % WS - b % WS + WS - 1);
      for (int h = 0; h < nH; ++h) rb[(size_t)h * WS2 * WS2 + a * WS2 + b] = tab[(size_t)rel * nH + h];
    }
  for (int h = 0; h < nH; ++h) pack_attn_terms(rb.data() + (size_t)h * WS2 * WS2, rbT.data() + (size_t)h * 4096);
  return rbT;
}

// a LayerNorm in the A path of the linear behind it (gemm.hip A_LN): y = ((x - mean) rstd g + b) W^T + bias = rstd ((x - mean) (W diag g)^T) + (bias + W b);
// W' = W diag(g) is rounded once to fp32 (its split is exact from there), bias' summed in fp64 (bias_host null: 0)
static void fold_ln(const float* W_host, const float* bias_host, const float* g, const float* b, int N, int K, std::vector<float>& w2, std::vector<float>& b2) {
  w2.resize((size_t)N * K); b2.resize(N);
  for (int n = 0; n < N; ++n) {
    double acc = bias_host ? bias_host[n] : 0.0;
    for (int k = 0; k < K; ++k) {
      w2[(size_t)n * K + k] = W_host[(size_t)n * K + k] * g[k];
      acc += (double)W_host[(size_t)n * K + k] * (double)b[k];
    }
    b2[n] = (float)acc;
  }
}

// PatchMerging of a [B][H][W][C] token tensor: norm (g, b [4C]) and reduction weight (w [2C][4C]) from nn.Unfold order k = c*4 + q
// (q = kh*2+kw) to gather order k' = q*C + c (transformer.py:363-385), and the merged row -> its top-left token (b, 2 y2, 2 x2)
struct MergePack {
  std::vector<float> g, b, w;
  std::vector<int> src;
};
static MergePack pack_merge(const float* g, const float* b, const float* w, int C, int B, int H, int W) {
  MergePack m;
  m.g.resize(4 * C); m.b.resize(4 * C); m.w.resize((size_t)2 * C * 4 * C);
  for (int q = 0; q < 4; ++q)
    for (int ch = 0; ch < C; ++ch) {
      m.g[q * C + ch] = g[ch * 4 + q];
      m.b[q * C + ch] = b[ch * 4 + q];
      for (int n = 0; n < 2 * C; ++n) m.w[(size_t)n * 4 * C + q * C + ch] = w[(size_t)n * 4 * C + ch * 4 + q];
    }
  m.src.resize((size_t)B * (H / 2) * (W / 2));
  for (int bi = 0; bi < B; ++bi)
    for (int y2 = 0; y2 < H / 2; ++y2)
      for (int x2 = 0; x2 < W / 2; ++x2) m.src[((size_t)bi * (H / 2) + y2) * (W / 2) + x2] = (bi * H + 2 * y2) * W + 2 * x2;
  return m;
}

// nuhtc_features' pooling (csrc/pool.hip): the chunk layout of four maps of hw[l] pixels, and the bytes of the slab of partial sums for B tiles
static int pool_layout(const int hw[4], PoolLevels& p) {
  const int rc = pool_chunks(hw, p.choff);
  for (int l = 0; l < 4; ++l) p.hw[l] = hw[l];
  return rc;
}
static size_t pool_slab_bytes(const PoolLevels& p, int B) { return (size_t)B * p.choff[4] * 64 * sizeof(double); }

// The route of a Swin block, from what is known at finalize.  The fp32 pipe has the plain kernels only; on the split pipe the block runs through the
// fused kernels of mlp.hip where they exist for its channel count (stage 1), else with its two norms in the A path of the QKV / fc1 linears.
static BlockRoute block_route(int matrix_pipe, int C) {
  if (matrix_pipe != NUHTC_PIPE_BF16_SPLIT) return ROUTE_PLAIN;
  return lnqkv_supported(C) && mlp_supported(C) ? ROUTE_FUSED : ROUTE_A_LN;
}

int nuhtc_finalize(nuhtc_engine* e) {
  if (!e) return NUHTC_E_INVALID;
  if (e->finalized) FAIL(e, NUHTC_E_STATE, "finalize called twice");
  HIP_CHECK(e, hipSetDevice(e->device));
  const nuhtc_config& c = e->cfg;
  const int B = c.max_batch;
  e->vh = c.valid_h ? c.valid_h : c.tile_h; e->vw = c.valid_w ? c.valid_w : c.tile_w;
  const ResizeGeom rg = resize_geom(e->vh, e->vw, c.scale_factor);
  e->Hv = rg.Hv; e->Wv = rg.Wv;             // img_shape
  const int Hn = rg.Hn, Wn = rg.Wn;         // pad_shape
  e->Hn = Hn; e->Wn = Wn;
  int rc;
  std::vector<float> on_g_host[4], on_b_host[4];      // the stages' output norms, for the fold into the FPN laterals
  if ((rc = upload(e, &e->rs_xtab, rg.tx)) || (rc = upload(e, &e->rs_ytab, rg.ty))) return rc;
  // ---- geometry
  for (int s = 0; s < 4; ++s) {
    stage_dims(e->st[s], Hn >> (2 + s), Wn >> (2 + s), 96 << s);
    if ((rc = build_stage_maps(e, s))) return rc;
  }
  // ---- patch embed: [96][3][4][4] -> [48][96], k = (kh*4+kw)*3 + c
  {
    RAW(w, "backbone.patch_embed.projection.weight", 96, 3, 4, 4);
    RAW(b, "backbone.patch_embed.projection.bias", 96);
    RAW(g, "backbone.patch_embed.norm.weight", 96);
    RAW(be, "backbone.patch_embed.norm.bias", 96);
    if ((rc = upload(e, &e->pe_w, pack_patch_embed(w->data.data()))) || (rc = upload(e, &e->pe_b, b->data)) || (rc = upload(e, &e->pe_g, g->data)) ||
        (rc = upload(e, &e->pe_beta, be->data)))
      return rc;
  }
  // ---- Swin blocks
  for (int s = 0; s < 4; ++s) {
    const int C = 96 << s, nH = NHEADS[s];
    for (int b = 0; b < DEPTHS[s]; ++b) {
      BlockW bw{};
      bw.route = block_route(c.matrix_pipe, C);
      std::string p = "backbone.stages." + std::to_string(s) + ".blocks." + std::to_string(b) + ".";
      RAW(n1w, p + "norm1.weight", C); RAW(n1b, p + "norm1.bias", C);
      RAW(tab, p + "attn.w_msa.relative_position_bias_table", 169, nH);
      RAW(qw, p + "attn.w_msa.qkv.weight", 3 * C, C); RAW(qb, p + "attn.w_msa.qkv.bias", 3 * C);
      RAW(pw, p + "attn.w_msa.proj.weight", C, C); RAW(pb, p + "attn.w_msa.proj.bias", C);
      RAW(n2w, p + "norm2.weight", C); RAW(n2b, p + "norm2.bias", C);
      RAW(f1w, p + "ffn.layers.0.0.weight", 4 * C, C); RAW(f1b, p + "ffn.layers.0.0.bias", 4 * C);
      RAW(f2w, p + "ffn.layers.1.weight", C, 4 * C); RAW(f2b, p + "ffn.layers.1.bias", C);
      if ((rc = upload(e, &bw.relbT, pack_rel_bias(tab->data.data(), nH)))) return rc;
      if ((rc = upload(e, &bw.n1g, n1w->data)) || (rc = upload(e, &bw.n1b, n1b->data)) ||           (rc = upload_gemm_weight(e, &bw.qkv_w, qw->data, 3 * C, C)) || (rc = upload(e, &bw.qkv_b, qb->data)) || (rc = upload_gemm_weight(e, &bw.proj_w, pw->data, C, C)) ||
          (rc = upload(e, &bw.proj_b, pb->data)) || (rc = upload(e, &bw.n2g, n2w->data)) || (rc = upload(e, &bw.n2b, n2b->data)) ||
          (rc = upload_gemm_weight(e, &bw.f1_w, f1w->data, 4 * C, C)) || (rc = upload(e, &bw.f1_b, f1b->data)) || (rc = upload_gemm_weight(e, &bw.f2_w, f2w->data, C, 4 * C)) ||
          (rc = upload(e, &bw.f2_b, f2b->data)))
        return rc;
      if (bw.route == ROUTE_A_LN) {
        // the two norms of the block ride in the A path of the linear behind them (gemm.hip A_LN, fold_ln)
        auto fold = [&](const std::vector<float>& W, const std::vector<float>& bias, const std::vector<float>& gam, const std::vector<float>& bet, int N,
                        float** wdev, float** bdev) -> int {
          std::vector<float> w2, b2;
          fold_ln(W.data(), bias.data(), gam.data(), bet.data(), N, C, w2, b2);
          int r = upload_gemm_weight(e, wdev, w2, N, C);
          return r ? r : upload(e, bdev, b2);
        };
        if ((rc = fold(qw->data, qb->data, n1w->data, n1b->data, 3 * C, &bw.qkv_wln, &bw.qkv_bln)) ||
            (rc = fold(f1w->data, f1b->data, n2w->data, n2b->data, 4 * C, &bw.f1_wln, &bw.f1_bln)))
          return rc;
      }
      if (bw.route == ROUTE_FUSED) {
        std::vector<unsigned short> st;
        lnqkv_pack_stream(qw->data.data(), C, st);
        if ((rc = upload_bytes(e, &bw.qkv_stream, st.data(), st.size() * 2))) return rc;
        mlp_pack_stream(f1w->data.data(), f2w->data.data(), C, st);
        if ((rc = upload_bytes(e, &bw.mlp_stream, st.data(), st.size() * 2))) return rc;
        proj_pack_stream(pw->data.data(), C, st);
        if ((rc = upload_bytes(e, &bw.proj_stream, st.data(), st.size() * 2))) return rc;
      }
      e->blocks[s].push_back(bw);
    }
    {
      std::string p = "backbone.norm" + std::to_string(s) + ".";
      RAW(w, p + "weight", C); RAW(b, p + "bias", C);
      if ((rc = upload(e, &e->on_g[s], w->data)) || (rc = upload(e, &e->on_b[s], b->data))) return rc;
      on_g_host[s] = w->data; on_b_host[s] = b->data;
    }
    if (s < 3) {
      // PatchMerging: norm and reduction weight in gather order (pack_merge)
      std::string p = "backbone.stages." + std::to_string(s) + ".downsample.";
      RAW(nw, p + "norm.weight", 4 * C); RAW(nb, p + "norm.bias", 4 * C); RAW(rw, p + "reduction.weight", 2 * C, 4 * C);
      const StageGeom& g = e->st[s];
      const MergePack m = pack_merge(nw->data.data(), nb->data.data(), rw->data.data(), C, B, g.H, g.W);
      if ((rc = upload(e, &e->mg_g[s], m.g)) || (rc = upload(e, &e->mg_b[s], m.b)) || (rc = upload_gemm_weight(e, &e->mg_w[s], m.w, 2 * C, 4 * C))) return rc;
      e->merge_one_launch[s] = c.matrix_pipe == NUHTC_PIPE_BF16_SPLIT && g.H % 2 == 0 && g.W % 2 == 0;
      if (e->merge_one_launch[s]) {
        // the merging norm in the A path of the reduction linear (gemm.hip A_LN, two segments per row): W' = W diag(gamma), b' = W beta
        std::vector<float> wl, bl;
        fold_ln(m.w.data(), nullptr, m.g.data(), m.b.data(), 2 * C, 4 * C, wl, bl);
        if ((rc = upload_gemm_weight(e, &e->mg_wln[s], wl, 2 * C, 4 * C)) || (rc = upload(e, &e->mg_bln[s], bl)) || (rc = upload(e, &e->mg_src[s], m.src))) return rc;
      }
    }
  }
  // ---- FPN
  e->out_ln_folded = c.matrix_pipe == NUHTC_PIPE_BF16_SPLIT;
  for (int i = 0; i < 4; ++i) {
    const int C = 96 << i;
    RAW(lw, "neck.lateral_convs." + std::to_string(i) + ".conv.weight", 64, C, 1, 1);
    RAW(lb, "neck.lateral_convs." + std::to_string(i) + ".conv.bias", 64);
    RAW(fw, "neck.fpn_convs." + std::to_string(i) + ".conv.weight", 64, 64, 3, 3);
    RAW(fb, "neck.fpn_convs." + std::to_string(i) + ".conv.bias", 64);
    if ((rc = upload_gemm_weight(e, &e->lat_w[i], lw->data, 64, C)) || (rc = upload(e, &e->lat_b[i], lb->data)) ||
        (rc = upload_gemm_weight(e, &e->fpn_w[i], pack_conv3(*fw, 64, 64), 64, 576)) || (rc = upload(e, &e->fpn_b[i], fb->data)))
      return rc;
    if (e->out_ln_folded) {      // the stage's output norm folded into its lateral (gemm.hip A_LN, N = 64)
      std::vector<float> wl, bl;
      fold_ln(lw->data.data(), lb->data.data(), on_g_host[i].data(), on_b_host[i].data(), 64, C, wl, bl);
      if ((rc = upload_gemm_weight(e, &e->lat_wln[i], wl, 64, C)) || (rc = upload(e, &e->lat_bln[i], bl))) return rc;
    }
  }
  {      // ---- nuhtc_features: chunk layout of the four maps and the slab of the pooling's partial sums (csrc/pool.hip)
    int hw[4];
    for (int l = 0; l < 4; ++l) hw[l] = e->st[l].H * e->st[l].W;
    if ((rc = pool_layout(hw, e->pool))) FAIL(e, rc, "pool_chunks: empty FPN level");
    if ((rc = dev_alloc(e, (void**)&e->pool_slab, pool_slab_bytes(e->pool, B)))) return rc;
  }
  const bool heads = !c.features_only;      // a features-only engine packs and allocates nothing behind the FPN
  // ---- RPN: 3x3 conv, then cls(3)+reg(12) fused into one N=32 pointwise layer (cols 0-2 cls, 3-14 reg, rest 0)
  if (heads) {
    RAW(cw, "rpn_head.rpn_conv.weight", 64, 64, 3, 3); RAW(cb, "rpn_head.rpn_conv.bias", 64);
    RAW(kw, "rpn_head.rpn_cls.weight", 3, 64, 1, 1); RAW(kb, "rpn_head.rpn_cls.bias", 3);
    RAW(rw, "rpn_head.rpn_reg.weight", 12, 64, 1, 1); RAW(rb, "rpn_head.rpn_reg.bias", 12);
    std::vector<float> w(32 * 64, 0.f), b(32, 0.f);
    for (int n = 0; n < 3; ++n) { b[n] = kb->data[n]; for (int k = 0; k < 64; ++k) w[n * 64 + k] = kw->data[n * 64 + k]; }
    for (int n = 0; n < 12; ++n) { b[3 + n] = rb->data[n]; for (int k = 0; k < 64; ++k) w[(3 + n) * 64 + k] = rw->data[n * 64 + k]; }
    if ((rc = upload_gemm_weight(e, &e->rpn_w, pack_conv3(*cw, 64, 64), 64, 576)) || (rc = upload(e, &e->rpn_b, cb->data)) ||
        (rc = upload_gemm_weight(e, &e->rpn_hw, w, 32, 64)) || (rc = upload(e, &e->rpn_hb, b)) || (rc = upload_fuse(e, &e->rpn_hf, w, 32)))
      return rc;
    e->conv_fuse = e->rpn_hf != nullptr;
  }
  // ---- semantic head
  if (heads) {
    const std::string p = "roi_head.semantic_head.";
    for (int i = 0; i < 4; ++i) {
      RAW(lw, p + "lateral_convs." + std::to_string(i) + ".conv.weight", 64, 64, 1, 1);
      RAW(lb, p + "lateral_convs." + std::to_string(i) + ".conv.bias", 64);
      RAW(cw, p + "convs." + std::to_string(i) + ".conv.weight", 64, 64, 3, 3);
      RAW(cb, p + "convs." + std::to_string(i) + ".conv.bias", 64);
      if ((rc = upload_gemm_weight(e, &e->sem_lw[i], lw->data, 64, 64)) || (rc = upload(e, &e->sem_lb[i], lb->data)) || (rc = upload_fuse(e, &e->sem_lf[i], lw->data, 64)) ||
          (rc = upload_gemm_weight(e, &e->sem_cw[i], pack_conv3(*cw, 64, 64), 64, 576)) || (rc = upload(e, &e->sem_cb[i], cb->data)))
        return rc;
    }
    RAW(ew, p + "conv_embedding.conv.weight", 64, 64, 1, 1); RAW(eb, p + "conv_embedding.conv.bias", 64);
    RAW(gw, p + "conv_logits.weight", 1, 64, 1, 1); RAW(gb, p + "conv_logits.bias", 1);
    if ((rc = upload_gemm_weight(e, &e->sem_ew, ew->data, 64, 64)) || (rc = upload(e, &e->sem_eb, eb->data)) || (rc = upload_fuse(e, &e->sem_ef, ew->data, 64)) || (rc = upload(e, &e->sem_gw, gw->data)) ||
        (rc = upload(e, &e->sem_gb, gb->data)))
      return rc;
  }
  if (heads && (rc = finalize_roi(e))) return rc;

  // ---- workspace (sized for max_batch)
  const StageGeom& g0 = e->st[0];
  if ((rc = ws(e, &e->img, "img", {B, Hn, Wn, 3}, 0))) return rc;
  size_t max_tok = 0, max_win = 0, max_qkv = 0, max_hid = 0;
  const int max_c = e->st[3].C;      // + one row of 3 max_c behind the window image: the bias row of StageGeom::bias_row
  for (int s = 0; s < 4; ++s) {
    const StageGeom& g = e->st[s];
    max_tok = std::max(max_tok, (size_t)g.H * g.W * g.C);
    max_win = std::max(max_win, (size_t)g.nW * WS2 * g.C);
    max_qkv = std::max(max_qkv, (size_t)g.nW * WS2 * 3 * g.C);
    max_hid = std::max(max_hid, (size_t)g.H * g.W * 4 * g.C);
  }
  if ((rc = ws(e, &e->tokA, "tokens", {B, (int64_t)max_tok}, 0)) || (rc = ws(e, &e->tokB, nullptr, {B, (int64_t)max_tok}, 0)) ||
      (rc = ws(e, &e->xw, nullptr, {B, (int64_t)max_win}, 0)) || (rc = ws(e, &e->qkv, nullptr, {(int64_t)B * (int64_t)max_qkv + 3 * (int64_t)max_c}, 0)) ||
      (rc = ws(e, &e->att, nullptr, {B, (int64_t)max_win}, 0)) || (rc = ws(e, &e->hid, nullptr, {B, (int64_t)std::max(max_hid, max_qkv)}, 0)))
    return rc;
  e->tok[0] = e->tokA; e->tok[1] = e->tokB;
  for (int s = 2; s < 4; ++s)
    if ((rc = ws(e, &e->tok[s], nullptr, {B, (int64_t)e->st[s].H * e->st[s].W * e->st[s].C}, 0))) return rc;
  for (int s = 0; s < 4; ++s)
    if ((rc = ws(e, &e->ln_out[s], nullptr, {B, (int64_t)e->st[1].H * e->st[1].W, 8}, 0))) return rc;
  if ((rc = ws(e, &e->ln_part, nullptr, {B, (int64_t)e->st[1].H * e->st[1].W, 8}, 0)) ||     // (stage 1, one partial per token: the same again)
      (rc = ws(e, &e->ln_part2, nullptr, {B, (int64_t)e->st[1].H * e->st[1].W, 8}, 0)))
    return rc;     // rows x (C / 96) x 2 is the same in stages 2-4
  for (int s = 0; s < 4; ++s) {
    const StageGeom& g = e->st[s];
    std::string n = std::to_string(s);
    if ((rc = ws(e, &e->c[s], ("c" + n).c_str(), {B, g.H, g.W, g.C}, 0)) || (rc = ws(e, &e->lat[s], ("lat" + n).c_str(), {B, g.H, g.W, 64}, 0)) ||
        (rc = ws(e, &e->x[s], ("x" + n).c_str(), {B, g.H, g.W, 64}, 0)))
      return rc;
    e->pool.x[s] = e->x[s];
    if (heads && ((rc = ws(e, &e->rpn[s], ("rpn" + n).c_str(), {B, g.H, g.W, 32}, 0)) || (rc = ws(e, &e->semg[s], nullptr, {B, g.H, g.W, 64}, 0))))
      return rc;
  }
  if (heads && ((rc = ws(e, &e->tmpA, nullptr, {B, g0.H, g0.W, 64}, 0)) || (rc = ws(e, &e->tmpB, nullptr, {B, g0.H, g0.W, 64}, 0)) ||
                (rc = ws(e, &e->tmpR, nullptr, {B, g0.H, g0.W, 64}, 0)) ||
                (rc = ws(e, &e->sem_feat, "sem_feat", {B, g0.H, g0.W, 64}, 0)) || (rc = ws(e, &e->x0sem, "x0sem", {B, g0.H, g0.W, 64}, 0)) ||
                (rc = ws(e, &e->sem_pred, "sem_pred", {B, g0.H, g0.W}, 0))))
    return rc;
  if (heads && (rc = alloc_roi_workspace(e))) return rc;
  {
    // The side stream carries the RPN branch (and the mid-size RoI class) beside the main stream's semantic branch.  Its NMS
    // launches are large grids of one-wave workgroups that slow a co-running main-stream kernel tenfold while they last (a 20 us
    // kernel of the component-proposal chain takes 200 us beside nms_mask_levels_kernel).  Running the branch at the lowest
    // stream priority (NUHTC_SIDE_PRIO=1, dev) frees the main stream but stretches the RPN chain by the same amount, and the
    // join then waits for it: measured 11.48-11.52 against 11.41-11.46 ms per step, so the default stays equal priority.
    // The stream handed out by nuhtc_stream() and the two side streams are created back to back: the runtime deals its hardware
    // queues to streams in creation order and the queues go round the command processor's four pipes, so the three end up on
    // three different pipes whatever GPU_MAX_HW_QUEUES is.  (Two queues of one pipe that wait on each other's events stall each
    // other: with 8-24 queues an engine whose side stream shared the pipe of the caller's stream ran 30 % slower.)
    bool pooled = false;
    {
      std::lock_guard<std::mutex> lock(g_stream_mu);
      auto& pool = g_stream_pool[e->device];
      if (!pool.empty()) { e->own = pool.back().own; e->side = pool.back().side; e->side2 = pool.back().side2; pool.pop_back(); pooled = true; }
    }
    if (!pooled) {
      HIP_CHECK(e, hipStreamCreateWithFlags(&e->own, hipStreamNonBlocking));
      int least = 0, greatest = 0;
      HIP_CHECK(e, hipDeviceGetStreamPriorityRange(&least, &greatest));
      HIP_CHECK(e, hipStreamCreateWithPriority(&e->side, hipStreamNonBlocking, dev_knob("SIDE_PRIO", 0) ? least : 0));
      HIP_CHECK(e, hipStreamCreateWithFlags(&e->side2, hipStreamNonBlocking));
    }
  }
  HIP_CHECK(e, hipEventCreateWithFlags(&e->ev_rpn, hipEventDisableTiming));
  HIP_CHECK(e, hipEventCreateWithFlags(&e->ev_side, hipEventDisableTiming));
  HIP_CHECK(e, hipEventCreateWithFlags(&e->ev_fpn, hipEventDisableTiming));
  HIP_CHECK(e, hipEventCreateWithFlags(&e->ev_side2, hipEventDisableTiming));
  HIP_CHECK(e, hipDeviceSynchronize());
  e->raw.clear();
  e->finalized = true;
  return 0;
}

// =============================================================================== dense part of the path
GemmParams gp(const float* A, const float* W, const float* bias, float* C, int M, int N, int K) {
  GemmParams p;
  memset(&p, 0, sizeof(p));
  p.A = A; p.W = W; p.bias = bias; p.C = C; p.M = M; p.N = N; p.K = K; p.lda = K; p.ldc = N; p.alpha = 1.f; p.m_mul = 1;
  return p;
}

static int conv3x3(nuhtc_engine* e, const float* in, const float* w, const float* b, float* out, int nimg, int H, int W, int act,
                   const int* m_dev, int m_mul, hipStream_t s, const Conv3Fuse* fuse = nullptr) {
  GemmParams p = gp(in, w, b, out, nimg * H * W, 64, 576);
  p.amode = A_CONV3; p.cH = H; p.cW = W; p.cC = 64; p.act = act; p.m_dev = m_dev; p.m_mul = m_mul; p.fuse = fuse;
  return egemm(e, p, s);
}
static Conv3Fuse pointwise(int N2, const void* w2f, const float* bias2, float* out2, int act2, int store_out) {
  Conv3Fuse f;
  memset(&f, 0, sizeof(f));
  f.N2 = N2; f.w2f = w2f; f.bias2 = bias2; f.out2 = out2; f.act2 = act2; f.store_out = store_out;
  return f;
}

// The attention half of a block up to the attention output (swin.py:356-363 up to proj): the QKV front writes the window image `qkv` of B
// images (geometry g, shift state sh), the window attention writes its rows to att[out_map[window row]] (g.map: token order, g.cidx: compact
// window order).  Only the T real tokens go through the QKV linear, which scatters its rows into the window image; a padding row of the image is
// the QKV bias (LN of a zero-padded token is 0 after swin.py:341-343's F.pad, so its qkv is the bias).  By the block's route:
//   ROUTE_FUSED    one kernel: LN1, window gather, QKV linear (mlp.hip)
//   ROUTE_A_LN     the norm in the linear's A path: statistics ln_epi (C / 96 partials per row, left by the producer's epilogue) or, with ln_epi
//                  null, computed here into ln_scratch; qkv_split: the bf16 split of the folded weight (null: the engine's table)
//   ROUTE_PLAIN    layernorm_windows writes the tokens in window order without the padding rows (xw, T rows) and the padding rows, then the linear
// On the first two the attention kernel never reads a padding row (StageGeom::padbits): the launch that writes the window image writes ONE bias row
// instead of the padding rows (stage 4: 72 % of the image's rows, stages 2-3: 20 %; profiles/r05_padbits_merge_ln.txt).
static int run_attn_front(nuhtc_engine* e, const StageGeom& g, const BlockW& w, int B, int sh, const float* x, float* xw, float* qkv, float* att,
                          const int* out_map, const float* ln_epi, float* ln_scratch, const void* qkv_split, hipStream_t s) {
  const int T = B * g.H * g.W, Mw = B * g.nW * WS2, C = g.C;
  // the Swin linears take the block-tile form of the engine's schedule (nuhtc_config.schedule, gemm.hip)
  auto linear = [&](GemmParams p) { p.throughput = e->cfg.schedule == NUHTC_SCHED_THROUGHPUT; return egemm(e, p, s); };
  switch (w.route) {
    case ROUTE_FUSED:
      RUN(launch_swin_lnqkv(x, qkv, g.ctok[sh], g.vrow[sh], g.brow, 1, w.n1g, w.n1b, w.qkv_stream, w.qkv_b, T, C, s));
      break;
    case ROUTE_A_LN: {      // the launch's extra workgroups write the bias row
      if (!ln_epi) RUN(launch_ln_stats(x, ln_scratch, T, C, s));
      GemmParams p = gp(x, w.qkv_wln, w.qkv_bln, qkv, T, 3 * C, C);
      p.amode = A_LN; p.ln_part = ln_epi ? ln_epi : ln_scratch; p.ln_nparts = ln_epi ? C / 96 : 1; p.a_rows = g.ctok[sh]; p.Wsplit = qkv_split;
      p.pad_rows = g.brow; p.n_pad = 1; p.pad_val = w.qkv_b;
      p.store = ST_ROWMAP; p.row_map = g.vrow[sh];
      RUN(linear(p));
      break;
    }
    case ROUTE_PLAIN: {
      RUN(launch_layernorm_windows(x, g.map[sh], g.cidx[sh], w.n1g, w.n1b, xw, qkv, w.qkv_b, Mw, C, s));
      GemmParams p = gp(xw, w.qkv_w, w.qkv_b, qkv, T, 3 * C, C);
      p.store = ST_ROWMAP; p.row_map = g.vrow[sh];
      RUN(linear(p));
      break;
    }
  }
  const bool split = w.route != ROUTE_PLAIN;
  RUN(launch_window_attn(qkv, w.relbT, sh ? g.mask : nullptr, sh ? g.mask_any : nullptr, out_map, att, B * g.nW, g.nW, C, g.nH, split, s,
                         split ? g.padbits[sh] : nullptr, g.bias_row));
  return 0;
}

int run_backbone(nuhtc_engine* e, int B, hipStream_t s) {
  const int Hn = e->Hn, Wn = e->Wn;
  // the Swin linears take the block-tile form of the engine's schedule (nuhtc_config.schedule, gemm.hip)
  auto linear = [&](GemmParams p) { p.throughput = e->cfg.schedule == NUHTC_SCHED_THROUGHPUT; return egemm(e, p, s); };
  {      // resize + Normalize + Pad inside the patch embedding: one launch, no `img` tensor (profiles/r05_preproc_fused.txt)
    float mi[6];
    norm_consts(e->cfg.mean, e->cfg.std, mi);
    RUN(launch_patch_embed_tiles(e->in_tiles, B, e->cfg.tile_h, e->cfg.tile_w, Hn, Wn, e->Hv, e->Wv, e->rs_xtab, e->rs_ytab, e->in_swap, mi, e->pe_w, e->pe_b, e->pe_g, e->pe_beta,
                                 e->tokA, s));
  }
  float* x = e->tok[0];
  // On ROUTE_A_LN the statistics of a norm are left by the epilogue of the GEMM that produced the tensor (profiles/r05_ln_in_a.txt), in ln_part.
  const float* first_part = e->ln_part;      // where the first block of the stage finds its LN1 partials: ln_part2 behind a merging linear in A_LN form
  e->last_batch = B;
  for (int st = 0; st < 4; ++st) {
    const StageGeom& g = e->st[st];
    const int T = B * g.H * g.W, C = g.C;
    const size_t nb = e->blocks[st].size();
    const bool merge_a = st < 3 && e->merge_one_launch[st];
    // the last block's FFN leaves the partials of the stage's final tensor in ln_out[st]: for the merging norm in the reduction linear, the output norm in the FPN lateral
    const bool final_stats = merge_a || e->out_ln_folded;
    float* xalt = st < 3 ? e->tok[st + 1] : nullptr;
    for (size_t b = 0; b < nb; ++b) {
      const BlockW& w = e->blocks[st][b];
      const int sh = (int)(b & 1);
      float* last_stats = final_stats && b + 1 == nb ? e->ln_out[st] : nullptr;
      // x += proj(attn(LN1(x)))      (mmdet swin.py:356-363)
      // ROUTE_FUSED: the projection rides in front of the fused FFN kernel, and the attention kernel writes its rows in TOKEN order (window
      // row -> token map) instead of the compact window order the projection GEMM scatters from
      RUN(run_attn_front(e, g, w, B, sh, x, e->xw, e->qkv, e->att, w.route == ROUTE_FUSED ? g.map[sh] : g.cidx[sh], b == 0 ? first_part : e->ln_part, nullptr, nullptr, s));
      if (e->debug_tokens) {
        auto it = e->bufs.find("att_s" + std::to_string(st) + "b" + std::to_string(b));
        if (it != e->bufs.end()) hipMemcpyAsync(it->second.ptr, e->att, (size_t)T * C * sizeof(float), hipMemcpyDeviceToDevice, s);
      }
      // x += W2·gelu(W1·LN2(x))      (swin.py:365-367, mmcv FFN)
      if (w.route == ROUTE_FUSED) {      // one kernel: attention projection + residual, LN2, both linears, GELU and the residual (mlp.hip)
        RUN(launch_swin_mlp(x, x, w.n2g, w.n2b, w.mlp_stream, w.f1_b, w.f2_b, T, C, s, e->att, w.proj_stream, w.proj_b, last_stats));
      } else {
        const bool ln_a = w.route == ROUTE_A_LN;
        GemmParams p = gp(e->att, w.proj_w, w.proj_b, x, T, C, C);
        p.store = ST_ROWMAP; p.row_map = g.ctok[sh]; p.res = x; p.ldr = C;
        if (ln_a) p.stats_out = e->ln_part;      // LN2 rides in fc1: its statistics leave with the rows
        RUN(linear(p));
        if (ln_a) {
          p = gp(x, w.f1_wln, w.f1_bln, e->hid, T, 4 * C, C);
          p.amode = A_LN; p.ln_part = e->ln_part; p.ln_nparts = C / 96;
        } else {
          RUN(launch_layernorm(x, nullptr, w.n2g, w.n2b, e->xw, T, C, s));
          p = gp(e->xw, w.f1_w, w.f1_b, e->hid, T, 4 * C, C);
        }
        p.act = ACT_GELU;
        RUN(linear(p));
        p = gp(e->hid, w.f2_w, w.f2_b, x, T, C, 4 * C);
        p.res = x; p.ldr = C;
        p.stats_out = b + 1 < nb ? (ln_a ? e->ln_part : nullptr) : last_stats;      // LN1 of the next block rides in its QKV linear
        RUN(linear(p));
      }
      if (e->debug_tokens) {
        auto it = e->bufs.find("tok_s" + std::to_string(st) + "b" + std::to_string(b));
        if (it != e->bufs.end()) hipMemcpyAsync(it->second.ptr, x, (size_t)T * C * sizeof(float), hipMemcpyDeviceToDevice, s);
      }
    }
    // swin.py:756-762 (tokens == NHWC) on the fp32 pipe; else the output norm runs in the lateral's A path (run_fpn, profiles/r05_out_ln.txt)
    if (!e->out_ln_folded) RUN(launch_layernorm(x, nullptr, e->on_g[st], e->on_b[st], e->c[st], T, C, s));
    if (st < 3) {
      const bool next_ln = e->blocks[st + 1][0].route == ROUTE_A_LN;   // LN1 of the next stage's first block rides in its QKV linear
      if (merge_a) {     // transformer.py:363-385 in one launch: row m = LayerNorm of the 2 x 2 tokens at mg_src[m] (two runs of 2 C floats, W tokens apart)
        GemmParams p = gp(x, e->mg_wln[st], e->mg_bln[st], xalt, T / 4, 2 * C, 4 * C);
        p.lda = C; p.amode = A_LN; p.ln_part = e->ln_out[st]; p.ln_nparts = 4 * (C / 96); p.a_rows = e->mg_src[st]; p.seg_k = 2 * C; p.seg_rows = g.W;
        if (next_ln) p.stats_out = e->ln_part2;      // not ln_part: other workgroups of this launch are still reading it
        RUN(linear(p));
        first_part = e->ln_part2;
      } else {           // fp32 pipe, or a map with an odd side: merge_ln_kernel + the plain reduction linear
        RUN(launch_merge_ln(x, e->mg_g[st], e->mg_b[st], e->xw, B, g.H, g.W, C, s));
        GemmParams p = gp(e->xw, e->mg_w[st], nullptr, xalt, T / 4, 2 * C, 4 * C);
        if (next_ln) p.stats_out = e->ln_part;
        RUN(linear(p));
        first_part = e->ln_part;
      }
      x = xalt;
    }
  }
  return 0;
}

// An FPN lateral (fpn.py:152-179) of B maps of H x W tokens of C channels: out = A W^T + bias, + the nearest-upsampled coarser lateral
// `parent` [B][H/2][W/2][64] in the epilogue (null: the top level).  ln_part: the rows are LayerNorm'ed in the product's A path (gemm.hip A_LN;
// W, bias with the norm folded in) from C / 96 partials per row.
static GemmParams lateral_params(const float* A, const float* W, const float* bias, float* out, int B, int H, int Wd, int C, const float* ln_part,
                                 const float* parent) {
  GemmParams p = gp(A, W, bias, out, B * H * Wd, 64, C);
  if (ln_part) { p.amode = A_LN; p.ln_part = ln_part; p.ln_nparts = C / 96; }
  if (parent) { p.up = parent; p.upH = H; p.upW = Wd; }
  return p;
}

int run_fpn(nuhtc_engine* e, int B, hipStream_t s, bool sem_lateral) {
  // FPN (mmdet/models/necks/fpn.py:152-179): laterals coarse->fine with the nearest-upsampled coarser lateral added in the epilogue
  for (int i = 3; i >= 0; --i) {
    const StageGeom& g = e->st[i];
    const float* parent = i < 3 ? e->lat[i + 1] : nullptr;
    // with the output norm folded, c[i] = LayerNorm(tok[i]) is never written: the lateral takes the stage's raw tokens and its partials
    const GemmParams p = e->out_ln_folded ? lateral_params(e->tok[i], e->lat_wln[i], e->lat_bln[i], e->lat[i], B, g.H, g.W, g.C, e->ln_out[i], parent)
                                          : lateral_params(e->c[i], e->lat_w[i], e->lat_b[i], e->lat[i], B, g.H, g.W, g.C, nullptr, parent);
    RUN(egemm(e, p, s));
  }
  for (int i = 0; i < 4; ++i) {
    const StageGeom& g = e->st[i];
    if (sem_lateral) {
      const Conv3Fuse f = pointwise(64, e->sem_lf[i], e->sem_lb[i], e->semg[i], ACT_NONE, 1);
      RUN(conv3x3(e, e->lat[i], e->fpn_w[i], e->fpn_b[i], e->x[i], B, g.H, g.W, ACT_NONE, nullptr, 1, s, &f));
    } else {
      RUN(conv3x3(e, e->lat[i], e->fpn_w[i], e->fpn_b[i], e->x[i], B, g.H, g.W, ACT_NONE, nullptr, 1, s));
    }
  }
  return 0;
}

int run_neck_heads(nuhtc_engine* e, int B, hipStream_t s) {
  // Pointwise layers that follow a 3x3 convolution are computed in that convolution's epilogue on the split pipe (conv.hip,
  // Conv3Fuse): the semantic head's lateral 1x1 rides on the FPN output conv of its level, the RPN's cls + reg layer on the RPN
  // conv (whose output is then never stored), conv_logits + conv_embedding (+ x0 + sem) on the semantic head's last conv.
  const bool fuse = e->conv_fuse;
  RUN(run_fpn(e, B, s, fuse));
  // RPN head (mmdet/models/dense_heads/rpn_head.py:62-68).  The RPN branch (conv + 1x1 heads here, proposal selection and
  // NMS in run_roi_path) and the semantic branch below both depend only on the FPN maps: the RPN branch runs on the side
  // stream from here on, so the tails of either branch's launches are filled by the other's blocks; joined before build_rois.
  // (throughput schedule: the branch stays on the caller's stream, the fork below is then a no-op between a stream and itself)
  hipStream_t s2 = e->cfg.schedule == NUHTC_SCHED_THROUGHPUT ? s : e->side;
  if (s2 != s && (hipEventRecord(e->ev_fpn, s) != hipSuccess || hipStreamWaitEvent(s2, e->ev_fpn, 0) != hipSuccess))
    FAIL(e, NUHTC_E_HIP, "side-stream fork failed");
  // the RPN head shares its weights across the levels (rpn_head.py:62-68 runs forward_single per level with the same modules): the four
  // maps go through ONE launch of the fused conv + cls/reg kernel -- the tiles of levels 1-3 (a third of level 0's) fill the tail of
  // level 0's persistent grid instead of three launches of 32-512 tiles on 256 CUs (profiles/r06_rpn_one_launch_ab.txt)
  if (fuse) {
    Conv3Fuse f = pointwise(32, e->rpn_hf, e->rpn_hb, e->rpn[0], ACT_NONE, 0);
    f.n_more = 3;
    for (int i = 1; i < 4; ++i) { f.more_in[i - 1] = e->x[i]; f.more_out2[i - 1] = e->rpn[i]; f.more_H[i - 1] = e->st[i].H; f.more_W[i - 1] = e->st[i].W; }
    RUN(conv3x3(e, e->x[0], e->rpn_w, e->rpn_b, e->tmpR, B, e->st[0].H, e->st[0].W, ACT_RELU, nullptr, 1, s2, &f));
  }
  for (int i = 0; i < 4 && !fuse; ++i) {      // fp32 pipe: conv, then the pointwise layer, per level
    const StageGeom& g = e->st[i];
    RUN(conv3x3(e, e->x[i], e->rpn_w, e->rpn_b, e->tmpR, B, g.H, g.W, ACT_RELU, nullptr, 1, s2));
    RUN(egemm(e, gp(e->tmpR, e->rpn_hw, e->rpn_hb, e->rpn[i], B * g.H * g.W, 32, 64), s2));
  }
  if (s2 != s && hipEventRecord(e->ev_rpn, s2) != hipSuccess) FAIL(e, NUHTC_E_HIP, "hipEventRecord failed");   // RPN maps ready (side stream)
  // FusedSemanticHead (fused_semantic_head.py:97-111)
  if (!fuse)
    for (int i = 0; i < 4; ++i) {
      const StageGeom& g = e->st[i];
      RUN(egemm(e, gp(e->x[i], e->sem_lw[i], e->sem_lb[i], e->semg[i], B * g.H * g.W, 64, 64), s));
    }
  const StageGeom& g0 = e->st[0];
  RUN(launch_sem_fuse(e->semg[0], e->semg[1], e->semg[2], e->semg[3], e->tmpA, B, g0.H, g0.W, s));
  float* a = e->tmpA;
  float* b = e->tmpB;
  for (int j = 0; j < 4; ++j) {
    if (fuse && j == 3) {
      // conv_logits (64 -> 1), conv_embedding (+ ReLU) and x0 + sem for the 7x7 RoI features, all from the tile in registers
      Conv3Fuse f = pointwise(64, e->sem_ef, e->sem_eb, e->sem_feat, ACT_RELU, 0);
      f.res2 = e->x[0]; f.out3 = e->x0sem;
      f.wn1 = e->sem_gw; f.bn1 = e->sem_gb; f.outn1 = e->sem_pred;
      RUN(conv3x3(e, a, e->sem_cw[j], e->sem_cb[j], b, B, g0.H, g0.W, ACT_RELU, nullptr, 1, s, &f));
      return 0;
    }
    RUN(conv3x3(e, a, e->sem_cw[j], e->sem_cb[j], b, B, g0.H, g0.W, ACT_RELU, nullptr, 1, s));
    std::swap(a, b);
  }
  RUN(launch_conv1x1_n1(a, e->sem_gw, e->sem_gb, e->sem_pred, B * g0.H * g0.W, 64, s));
  {
    GemmParams p = gp(a, e->sem_ew, e->sem_eb, e->sem_feat, B * g0.H * g0.W, 64, 64);
    p.act = ACT_RELU;
    RUN(egemm(e, p, s));
    // x0 + sem for the 7x7 RoI features (roi.hip: one interpolation serves the FPN level-0 and the semantic term)
    p.C = e->x0sem; p.res = e->x[0]; p.ldr = 64;
    RUN(egemm(e, p, s));
  }
  return 0;
}

// =============================================================================== public entry points
static int check_infer_args(nuhtc_engine* e, const uint8_t* tiles, int B) {
  if (!e) return NUHTC_E_INVALID;
  if (!e->finalized) FAIL(e, NUHTC_E_STATE, "nuhtc_infer before nuhtc_finalize");
  if (!tiles || B < 1 || B > e->cfg.max_batch) FAIL(e, NUHTC_E_INVALID, "bad tiles pointer or batch size (1..max_batch)");
  return 0;
}

static int check_detect_engine(nuhtc_engine* e) {
  if (e->cfg.features_only) FAIL(e, NUHTC_E_STATE, "this engine was created with features_only = 1: it serves nuhtc_features only");
  return 0;
}

// one step; a step that fails forgets the caller's tile pointer (nuhtc_get_buffer("img") reads it again: include/nuhtc_hip.h)
static int run_step(nuhtc_engine* e, int B, const float* rois, int n_rois, int n_dets, hipStream_t s, const nuhtc_dets* out) {
  int rc = run_backbone(e, B, s);
  if (!rc) rc = run_neck_heads(e, B, s);
  if (!rc) rc = run_roi_path(e, B, rois, n_rois, n_dets, s, out);
  if (rc) e->in_tiles = nullptr;
  return rc;
}

int nuhtc_infer(nuhtc_engine* e, const uint8_t* tiles, int B, int channel_mode, void* stream, const nuhtc_dets* out) {
  int rc = check_infer_args(e, tiles, B);
  if (rc || (rc = check_detect_engine(e))) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIP_CHECK(e, hipSetDevice(e->device));
  e->lastB = B;
  e->in_tiles = tiles; e->in_swap = channel_mode == NUHTC_CH_SWAP;      // the backbone's first launch reads the tiles (swin.hip patch_embed_tiles_kernel)
  return run_step(e, B, nullptr, 0, 0, s, out);
}

int nuhtc_infer_fixed_load(nuhtc_engine* e, const uint8_t* tiles, int B, int channel_mode, const float* rois, int n_rois, int n_dets,
                           void* stream, const nuhtc_dets* out) {
  int rc = check_infer_args(e, tiles, B);
  if (rc || (rc = check_detect_engine(e))) return rc;
  if (!rois || n_rois < 1 || n_rois > e->roi_cap || n_dets < 1 || n_dets > e->cfg.max_per_img) FAIL(e, NUHTC_E_INVALID, "bad fixed-load arguments");
  hipStream_t s = (hipStream_t)stream;
  HIP_CHECK(e, hipSetDevice(e->device));
  e->lastB = B;
  e->in_tiles = tiles; e->in_swap = channel_mode == NUHTC_CH_SWAP;      // the backbone's first launch reads the tiles (swin.hip patch_embed_tiles_kernel)
  return run_step(e, B, rois, n_rois, n_dets, s, out);
}

int nuhtc_features(nuhtc_engine* e, const uint8_t* tiles, int B, int channel_mode, void* stream, float* feat) {
  int rc = check_infer_args(e, tiles, B);
  if (rc) return rc;
  if (!feat) FAIL(e, NUHTC_E_INVALID, "nuhtc_features: null feature buffer");
  hipStream_t s = (hipStream_t)stream;
  HIP_CHECK(e, hipSetDevice(e->device));
  e->lastB = B;
  e->in_tiles = tiles; e->in_swap = channel_mode == NUHTC_CH_SWAP;      // the backbone's first launch reads the tiles (swin.hip patch_embed_tiles_kernel)
  // Swin-T + FPN (model.extract_feat), every launch on the caller's stream, then the means of x[0..3] (csrc/pool.hip)
  rc = run_backbone(e, B, s);
  if (!rc) rc = run_fpn(e, B, s, false);
  if (!rc && (rc = launch_fpn_mean_pool(e->pool, B, e->pool_slab, feat, s))) e->err = "fpn_mean_pool launch failed";
  if (rc) e->in_tiles = nullptr;
  return rc;
}

int nuhtc_mask_contours(nuhtc_engine* e, const nuhtc_dets* dets, int B, int cap, int16_t* xy, int32_t* n, void* stream) {
  if (!e) return NUHTC_E_INVALID;
  if (!dets || !dets->masks || !dets->counts || !xy || !n || B < 1 || B > e->cfg.max_batch || cap < 1)
    FAIL(e, NUHTC_E_INVALID, "bad nuhtc_mask_contours arguments");
  HIP_CHECK(e, hipSetDevice(e->device));
  int rc = launch_contours(dets->masks, dets->keep, dets->counts, B, e->cfg.max_per_img, e->cfg.tile_h, e->cfg.tile_w, cap, xy, n,
                           (hipStream_t)stream);
  if (rc) FAIL(e, rc, "contour launch failed (tile width must be a multiple of 32)");
  return 0;
}


int nuhtc_export_kept(nuhtc_engine* e, const nuhtc_dets* dets, int B, const int32_t* contour_n, const int16_t* contour_xy, int contour_cap, int cap,
                      int32_t* n_dev, int64_t* idx_dev, float* boxes_dev, int32_t* labels_dev, int32_t* cn_dev, int16_t* xy_dev, uint32_t* words_dev,
                      void* stream) {
  if (!e) return NUHTC_E_INVALID;
  if (!dets || !dets->boxes || !dets->labels || !dets->counts || !dets->keep || !dets->masks || B < 1 || B > e->cfg.max_batch || cap < 1 ||
      !n_dev || !idx_dev || !boxes_dev || !labels_dev || !cn_dev || !words_dev || (contour_xy && (!xy_dev || contour_cap < 1)))
    FAIL(e, NUHTC_E_INVALID, "bad nuhtc_export_kept arguments");
  HIP_CHECK(e, hipSetDevice(e->device));
  if (!e->export_pos) {
    int rc = dev_alloc(e, (void**)&e->export_pos, (size_t)e->cfg.max_batch * e->cfg.max_per_img * sizeof(int32_t));
    if (rc) return rc;
  }
  ExportParams p{dets->boxes, dets->labels, dets->counts, dets->keep, dets->masks, contour_n, contour_xy, B, e->cfg.max_per_img,
                 e->cfg.tile_h * (e->cfg.tile_w / 32), contour_cap, cap, n_dev, idx_dev, boxes_dev, labels_dev, cn_dev, xy_dev, words_dev};
  int rc = launch_export_kept(p, e->export_pos, (hipStream_t)stream);
  if (rc) FAIL(e, rc, "export launch failed");
  // n_dev[1]: the capacity flag nuhtc_check reports, so that a caller that fetches results through this export needs no second
  // round trip (and may have the engine's next batch enqueued already, which resets the flag)
  if (e->overflow) HIP_CHECK(e, hipMemcpyAsync(n_dev + 1, e->overflow, sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  else HIP_CHECK(e, hipMemsetAsync(n_dev + 1, 0, sizeof(int32_t), (hipStream_t)stream));
  return 0;
}

int nuhtc_export_crops(nuhtc_engine* e, const uint32_t* words_dev, const int32_t* n_dev, int cap, int32_t* crop_box_dev, int32_t* crop_area_dev,
                       int32_t* crop_off_dev, uint32_t* crop_words_dev, int pool_cap, void* stream) {
  if (!e) return NUHTC_E_INVALID;
  if (!words_dev || !n_dev || cap < 1 || !crop_box_dev || !crop_area_dev || !crop_off_dev || !crop_words_dev || pool_cap < 1)
    FAIL(e, NUHTC_E_INVALID, "bad nuhtc_export_crops arguments");
  HIP_CHECK(e, hipSetDevice(e->device));
  const int max_cap = e->cfg.max_batch * e->cfg.max_per_img;
  if (cap > max_cap) FAIL(e, NUHTC_E_INVALID, "nuhtc_export_crops: cap exceeds max_batch * max_per_img");
  if (!e->crop_size) {
    int rc = dev_alloc(e, (void**)&e->crop_size, (size_t)max_cap * sizeof(int32_t));
    if (rc) return rc;
  }
  int rc = launch_export_crops(words_dev, n_dev, cap, e->cfg.tile_h, e->cfg.tile_w / 32, crop_box_dev, crop_area_dev, crop_off_dev, e->crop_size, crop_words_dev,
                               pool_cap, (hipStream_t)stream);
  if (rc) FAIL(e, rc, "crop export launch failed");
  return 0;
}

int nuhtc_check(nuhtc_engine* e, void* stream) {
  if (!e) return NUHTC_E_INVALID;
  HIP_CHECK(e, hipSetDevice(e->device));
  if (e->overflow && !e->overflow_host) HIP_CHECK(e, hipHostMalloc((void**)&e->overflow_host, 4 * sizeof(int), hipHostMallocDefault));
  if (e->overflow) HIP_CHECK(e, hipMemcpyAsync(e->overflow_host, e->overflow, 4 * sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_CHECK(e, hipStreamSynchronize((hipStream_t)stream));
  if (e->overflow && e->overflow_host[0]) FAIL(e, NUHTC_E_CAPACITY, "connected-component proposals exceeded max_cc_proposals on at least one tile");
  return 0;
}

int nuhtc_get_buffer(nuhtc_engine* e, const char* name, void** ptr, int64_t* shape, int* ndim, int* dtype) {
  if (!e || !name || !ptr) return NUHTC_E_INVALID;
  if (strcmp(name, "__enable_token_dump") == 0) {
    // allocate per-block token and attention-output snapshots (parity tests only)
    if (!e->debug_tokens) {
      for (int s = 0; s < 4; ++s)
        for (int b = 0; b < DEPTHS[s]; ++b) {
          float* p;
          const StageGeom& g = e->st[s];
          int rc = ws(e, &p, ("tok_s" + std::to_string(s) + "b" + std::to_string(b)).c_str(), {e->cfg.max_batch, g.H * g.W, g.C}, 0);
          if (rc) return rc;
          // the block's attention output as the kernel wrote it: token order where proj is fused into the FFN kernel, else compact window order
          rc = ws(e, &p, ("att_s" + std::to_string(s) + "b" + std::to_string(b)).c_str(), {e->cfg.max_batch, g.H * g.W, g.C}, 0);
          if (rc) return rc;
        }
      e->debug_tokens = true;
    }
    *ptr = nullptr;
    if (ndim) *ndim = 0;
    return 0;
  }
  auto it = e->bufs.find(name);
  if (it == e->bufs.end()) FAIL(e, NUHTC_E_NOTFOUND, std::string("unknown buffer: ") + name);
  if (e->out_ln_folded && e->last_batch && name[0] == 'c' && name[1] >= '0' && name[1] <= '3' && name[2] == 0) {
    // the stage's output norm ran inside the FPN lateral: the tensor is computed now, from the stage's tokens, by the kernel that writes it on the
    // other path (parity tests read c0..c3)
    const int st = name[1] - '0';
    const StageGeom& g = e->st[st];
    HIP_CHECK(e, hipSetDevice(e->device));
    HIP_CHECK(e, hipDeviceSynchronize());
    const int rc = launch_layernorm(e->tok[st], nullptr, e->on_g[st], e->on_b[st], e->c[st], e->last_batch * g.H * g.W, g.C, nullptr);
    if (rc) FAIL(e, rc, "layernorm for a requested c buffer failed");
    HIP_CHECK(e, hipDeviceSynchronize());
  }
  if (strcmp(name, "img") == 0 && e->in_tiles) {
    // the pre-processing runs inside the patch embedding: the normalised image is computed now, by preproc_kernel, from the tiles of the last call
    // (which must still be what they were: parity tests read `img` right after the call)
    float mi[6];
    norm_consts(e->cfg.mean, e->cfg.std, mi);
    HIP_CHECK(e, hipSetDevice(e->device));
    HIP_CHECK(e, hipDeviceSynchronize());
    const int rc = launch_preproc(e->in_tiles, e->img, e->last_batch, e->cfg.tile_h, e->cfg.tile_w, e->Hn, e->Wn, e->Hv, e->Wv, e->rs_xtab, e->rs_ytab, e->in_swap, mi, nullptr);
    if (rc) FAIL(e, rc, "preproc for the requested img buffer failed");
    HIP_CHECK(e, hipDeviceSynchronize());
  }
  *ptr = it->second.ptr;
  if (ndim) *ndim = (int)it->second.shape.size();
  if (shape)
    for (size_t i = 0; i < it->second.shape.size() && i < 6; ++i) shape[i] = it->second.shape[i];
  if (dtype) *dtype = it->second.dtype;
  return 0;
}

int nuhtc_op_gemm(nuhtc_engine* e, const float* A, const float* W, const float* bias, float* C, int M, int N, int K, int act, void* stream) {
  if (!e || !A || !W || !C) return NUHTC_E_INVALID;
  HIP_CHECK(e, hipSetDevice(e->device));
  GemmParams p = gp(A, W, bias, C, M, N, K);
  p.act = act;
  int rc = launch_gemm(p, (hipStream_t)stream);
  if (rc) FAIL(e, rc, "gemm launch failed (K%32, N%32 required)");
  return 0;
}

int nuhtc_op_gemm_split(nuhtc_engine* e, const float* A, const float* W_dev, const float* W_host, const float* bias, float* C, int M, int N,
                        int K, int act, void* stream) {
  if (!e || !A || !W_dev || !W_host || !C) return NUHTC_E_INVALID;
  HIP_CHECK(e, hipSetDevice(e->device));
  hipStream_t s = (hipStream_t)stream;
  std::vector<unsigned short> split;      // a private split of this call's weight: the registry of the engines' weights is not touched
  int rc = gemm_make_split(W_host, N, K, split);
  if (rc) FAIL(e, rc, "gemm_make_split failed (K % 8)");
  DevScratch sc;
  GemmParams p = gp(A, W_dev, bias, C, M, N, K);
  p.act = act;
  p.Wsplit = sc.upload(split);
  if (!sc.ok()) FAIL(e, NUHTC_E_HIP, "gemm_split op: scratch upload failed");
  rc = launch_gemm(p, s);
  return op_finish(e, rc, s, "gemm launch failed (K%32, N%32 required)", "gemm kernel failed");
}

int nuhtc_op_conv3(nuhtc_engine* e, const nuhtc_conv3_args* a, void* stream) {
  if (!e || !a) return NUHTC_E_INVALID;
  if (!a->in || !a->w) FAIL(e, NUHTC_E_INVALID, "conv3 op: null input or weight");
  if (a->nimg < 1 || a->H < 1 || a->W < 1 || (long long)a->nimg * a->H * a->W * 64 >= (1ll << 31)) FAIL(e, NUHTC_E_INVALID, "conv3 op: size out of range");
  if (a->pipe != NUHTC_PIPE_BF16_SPLIT && a->pipe != NUHTC_PIPE_FP32) FAIL(e, NUHTC_E_INVALID, "conv3 op: unknown pipe");
  if (a->n_more < 0 || a->n_more > 3) FAIL(e, NUHTC_E_INVALID, "conv3 op: n_more out of range");
  if (!a->N2 && (a->n_more || a->out2 || a->out3 || a->outn1 || !a->out)) FAIL(e, NUHTC_E_INVALID, "conv3 op: fused options need N2, a plain conv needs out");
  for (int k = 0; k < a->n_more; ++k)
    if ((long long)a->nimg * a->more_H[k] * a->more_W[k] * 64 >= (1ll << 31)) FAIL(e, NUHTC_E_INVALID, "conv3 op: further map out of range");
  HIP_CHECK(e, hipSetDevice(e->device));
  hipStream_t s = (hipStream_t)stream;
  // private device copies of the packed weights (the engine's registry is not touched), freed after the launch
  DevScratch sc;
  int rc = 0;
  HostTensor wt;
  wt.shape = {64, 64, 3, 3};
  wt.data.assign(a->w, a->w + 64 * 64 * 9);
  const std::vector<float> wp = pack_conv3(wt, 64, 64);
  GemmParams p = gp(a->in, sc.upload(wp), a->bias ? sc.upload(a->bias, 64) : nullptr, a->out, a->nimg * a->H * a->W, 64, 576);
  p.amode = A_CONV3; p.cH = a->H; p.cW = a->W; p.cC = 64; p.act = a->act; p.m_dev = a->nimg_dev; p.m_mul = a->H * a->W;
  if (a->pipe == NUHTC_PIPE_BF16_SPLIT) {
    std::vector<unsigned short> split;
    if (!(rc = gemm_make_split(wp.data(), 64, 576, split))) p.Wsplit = sc.upload(split);
  }
  Conv3Fuse f;
  memset(&f, 0, sizeof(f));
  if (!rc && a->N2) {
    std::vector<unsigned short> img;
    rc = a->w2 ? conv3_pack_fuse(a->w2, a->N2, img) : NUHTC_E_INVALID;
    if (!rc) {
      f = pointwise(a->N2, sc.upload(img), a->b2 ? sc.upload(a->b2, a->N2) : nullptr, a->out2, a->act2, a->store_out);
      f.res2 = a->res2; f.out3 = a->out3; f.outn1 = a->outn1;
      f.wn1 = a->wn1 ? sc.upload(a->wn1, 64) : nullptr;
      f.bn1 = a->bn1 ? sc.upload(a->bn1, 1) : nullptr;
      f.n_more = a->n_more;
      for (int k = 0; k < a->n_more; ++k) { f.more_in[k] = a->more_in[k]; f.more_out2[k] = a->more_out2[k]; f.more_H[k] = a->more_H[k]; f.more_W[k] = a->more_W[k]; }
      p.fuse = &f;
    }
  }
  if (!sc.ok()) FAIL(e, NUHTC_E_HIP, "conv3 op: scratch upload failed");
  if (!rc) rc = launch_gemm(p, s);
  return op_finish(e, rc, s, "conv3 launch refused or failed (fused options: split pipe, N2 32 / 64, out3 with N2 64 and res2, n_more without store_out / out3 / outn1 / nimg_dev)",
                   "conv3 kernel failed");
}

int nuhtc_op_ln_gemm(nuhtc_engine* e, const float* X_dev, int T, const int* rows_dev, const float* W_host, const float* bias_host, const float* ln_g_host,
                     const float* ln_b_host, float* C_dev, int M, int N, int K, int act, void* stream) {
  if (!e || !X_dev || !W_host || !ln_g_host || !ln_b_host || !C_dev || M < 1 || N < 1 || K < 1 || T < 1) return NUHTC_E_INVALID;
  HIP_CHECK(e, hipSetDevice(e->device));
  hipStream_t s = (hipStream_t)stream;
  std::vector<float> w2, b2;
  fold_ln(W_host, bias_host, ln_g_host, ln_b_host, N, K, w2, b2);
  std::vector<unsigned short> split;
  int rc = gemm_make_split(w2.data(), N, K, split);
  if (rc) FAIL(e, rc, "gemm_make_split failed (K % 8)");
  DevScratch sc;
  float* st = sc.alloc<float>((size_t)T * 8);
  GemmParams p = gp(X_dev, sc.upload(w2), sc.upload(b2), C_dev, M, N, K);
  p.act = act; p.Wsplit = sc.upload(split); p.amode = A_LN; p.ln_part = st; p.ln_nparts = 1; p.a_rows = rows_dev;
  if (!sc.ok()) FAIL(e, NUHTC_E_HIP, "ln_gemm op: scratch upload failed");
  rc = launch_ln_stats(X_dev, st, T, K, s);
  if (!rc) rc = launch_gemm(p, s);
  return op_finish(e, rc, s, "ln_gemm launch failed (N % 96, K % 32 required)", "ln_gemm failed");
}

int nuhtc_op_gemm_ln_gemm(nuhtc_engine* e, const float* A_dev, const float* Wp_host, const float* bp_host, const float* res_dev, const int* row_map_dev,
                          const float* W_host, const float* bias_host, const float* ln_g_host, const float* ln_b_host, float* Y_dev, float* C_dev, int M,
                          int Kp, int K, int N, int act, void* stream) {
  if (!e || !A_dev || !Wp_host || !W_host || !ln_g_host || !ln_b_host || !Y_dev || !C_dev || M < 1 || N < 1 || K < 1 || Kp < 1 || K % 96) return NUHTC_E_INVALID;
  HIP_CHECK(e, hipSetDevice(e->device));
  hipStream_t s = (hipStream_t)stream;
  std::vector<float> w2, b2;
  fold_ln(W_host, bias_host, ln_g_host, ln_b_host, N, K, w2, b2);
  std::vector<unsigned short> split, split_p;
  int rc = gemm_make_split(w2.data(), N, K, split);
  if (!rc) rc = gemm_make_split(Wp_host, K, Kp, split_p);
  if (rc) FAIL(e, rc, "gemm_make_split failed (K % 8)");
  DevScratch sc;
  float* st = sc.alloc<float>((size_t)M * (K / 96) * 8);
  GemmParams q = gp(A_dev, sc.upload(Wp_host, (size_t)K * Kp), bp_host ? sc.upload(bp_host, K) : nullptr, Y_dev, M, K, Kp);   // the producer: Y[row_map(m)] = A Wp^T + bp (+ res), statistics on the way out
  q.Wsplit = sc.upload(split_p); q.stats_out = st;
  if (res_dev) { q.res = res_dev; q.ldr = K; }
  if (row_map_dev) { q.store = ST_ROWMAP; q.row_map = row_map_dev; }
  GemmParams p = gp(Y_dev, sc.upload(w2), sc.upload(b2), C_dev, M, N, K);
  p.act = act; p.Wsplit = sc.upload(split); p.amode = A_LN; p.ln_part = st; p.ln_nparts = K / 96;
  if (!sc.ok()) FAIL(e, NUHTC_E_HIP, "gemm_ln_gemm op: scratch upload failed");
  rc = launch_gemm(q, s);
  if (!rc) rc = launch_gemm(p, s);
  return op_finish(e, rc, s, "gemm_ln_gemm launch failed", "gemm_ln_gemm failed");
}

int nuhtc_op_merge_ln_gemm(nuhtc_engine* e, const float* X_dev, int B, int H, int W, int C, const float* W_host, const float* ln_g_host, const float* ln_b_host,
                           float* Y_dev, void* stream) {
  if (!e || !X_dev || !W_host || !ln_g_host || !ln_b_host || !Y_dev || B < 1 || H < 2 || W < 2 || (H & 1) || (W & 1) || C < 96 || C % 96) return NUHTC_E_INVALID;
  HIP_CHECK(e, hipSetDevice(e->device));
  hipStream_t s = (hipStream_t)stream;
  const int T = B * H * W, M = T / 4;
  const MergePack m = pack_merge(ln_g_host, ln_b_host, W_host, C, B, H, W);      // the packing of nuhtc_finalize
  std::vector<float> wl, bl;
  fold_ln(m.w.data(), nullptr, m.g.data(), m.b.data(), 2 * C, 4 * C, wl, bl);
  std::vector<unsigned short> split;
  int rc = gemm_make_split(wl.data(), 2 * C, 4 * C, split);
  if (rc) FAIL(e, rc, "gemm_make_split failed");
  DevScratch sc;
  float* st = sc.alloc<float>((size_t)T * (C / 96) * 8);
  GemmParams p = gp(X_dev, sc.upload(wl), sc.upload(bl), Y_dev, M, 2 * C, 4 * C);
  p.Wsplit = sc.upload(split); p.lda = C; p.amode = A_LN; p.ln_part = st; p.ln_nparts = 4 * (C / 96); p.a_rows = sc.upload(m.src); p.seg_k = 2 * C; p.seg_rows = W;
  if (!sc.ok()) FAIL(e, NUHTC_E_HIP, "merge_ln_gemm op: scratch upload failed");
  rc = launch_ln_stats(X_dev, st, T * (C / 96), 96, s);       // a partial per token and 96 channels: what the producers' epilogues leave
  if (!rc) rc = launch_gemm(p, s);
  return op_finish(e, rc, s, "merge_ln_gemm launch failed", "merge_ln_gemm failed");
}

int nuhtc_op_swin_mlp(nuhtc_engine* e, const float* x_dev, const float* ln_g_dev, const float* ln_b_dev, const float* w1_host, const float* b1_dev,
                      const float* w2_host, const float* b2_dev, float* out_dev, int T, int C, void* stream) {
  if (!e || !x_dev || !ln_g_dev || !ln_b_dev || !w1_host || !b1_dev || !w2_host || !b2_dev || !out_dev || T < 1) return NUHTC_E_INVALID;
  if (!mlp_supported(C)) FAIL(e, NUHTC_E_INVALID, "nuhtc_op_swin_mlp: unsupported channel count");
  HIP_CHECK(e, hipSetDevice(e->device));
  hipStream_t s = (hipStream_t)stream;
  std::vector<unsigned short> st;
  mlp_pack_stream(w1_host, w2_host, C, st);
  DevScratch sc;
  const void* d = sc.upload(st);
  if (!sc.ok()) FAIL(e, NUHTC_E_HIP, "weight stream upload failed");
  const int rc = launch_swin_mlp(x_dev, out_dev, ln_g_dev, ln_b_dev, d, b1_dev, b2_dev, T, C, s);
  return op_finish(e, rc, s, "swin_mlp launch failed", "swin_mlp kernel failed");
}

int nuhtc_op_swin_proj_mlp(nuhtc_engine* e, const float* x_dev, const float* att_dev, const float* wp_host, const float* bp_dev, const float* ln_g_dev,
                           const float* ln_b_dev, const float* w1_host, const float* b1_dev, const float* w2_host, const float* b2_dev, float* out_dev,
                           int T, int C, void* stream) {
  if (!e || !x_dev || !att_dev || !wp_host || !bp_dev || !ln_g_dev || !ln_b_dev || !w1_host || !b1_dev || !w2_host || !b2_dev || !out_dev || T < 1) return NUHTC_E_INVALID;
  if (!mlp_supported(C)) FAIL(e, NUHTC_E_INVALID, "nuhtc_op_swin_proj_mlp: unsupported channel count");
  HIP_CHECK(e, hipSetDevice(e->device));
  hipStream_t s = (hipStream_t)stream;
  std::vector<unsigned short> st, sp;
  mlp_pack_stream(w1_host, w2_host, C, st);
  proj_pack_stream(wp_host, C, sp);
  DevScratch sc;
  const void *d = sc.upload(st), *dp = sc.upload(sp);
  if (!sc.ok()) FAIL(e, NUHTC_E_HIP, "weight stream upload failed");
  // the kernel works in place (its FFN residual re-reads x' where the projection stored it): out <- x first
  int rc = 0;
  if (out_dev != x_dev && hipMemcpyAsync(out_dev, x_dev, (size_t)T * C * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) rc = NUHTC_E_HIP;
  if (!rc) rc = launch_swin_mlp(out_dev, out_dev, ln_g_dev, ln_b_dev, d, b1_dev, b2_dev, T, C, s, att_dev, dp, bp_dev);
  return op_finish(e, rc, s, "swin_proj_mlp launch failed", "swin_proj_mlp kernel failed");
}

int nuhtc_op_window_msa(nuhtc_engine* e, const nuhtc_wmsa_args* a, void* stream) {
  if (!e || !a) return NUHTC_E_INVALID;
  if (!a->x || !a->out || !a->ln_g || !a->ln_b || !a->qkv_w || !a->qkv_b || !a->rel_table) FAIL(e, NUHTC_E_INVALID, "window_msa op: null argument");
  const int C = a->C, B = a->B, H = a->H, W = a->W;
  if (C != 96 && C != 192 && C != 384 && C != 768) FAIL(e, NUHTC_E_INVALID, "window_msa op: C must be 96, 192, 384 or 768");
  if (a->pipe != NUHTC_PIPE_BF16_SPLIT && a->pipe != NUHTC_PIPE_FP32) FAIL(e, NUHTC_E_INVALID, "window_msa op: unknown pipe");
  if (a->out_order != NUHTC_ORDER_TOKEN && a->out_order != NUHTC_ORDER_COMPACT) FAIL(e, NUHTC_E_INVALID, "window_msa op: unknown out_order");
  if (a->shifted != 0 && a->shifted != 1) FAIL(e, NUHTC_E_INVALID, "window_msa op: shifted must be 0 or 1");
  if (B < 1 || H < 1 || W < 1) FAIL(e, NUHTC_E_INVALID, "window_msa op: B, H, W must be >= 1");
  // the window image (B images of Hp x Wp rows of 3C floats, + the bias row) must stay below 2^31 elements: row counts and element
  // offsets of the launches are 32-bit
  if (((long long)B * (cdiv(H, WS) * (long long)WS) * (cdiv(W, WS) * (long long)WS) + 1) * 3 * C >= (1ll << 31))
    FAIL(e, NUHTC_E_INVALID, "window_msa op: size out of range (window image >= 2^31 elements)");
  HIP_CHECK(e, hipSetDevice(e->device));
  hipStream_t s = (hipStream_t)stream;
  StageGeom g{};
  stage_dims(g, H, W, C);
  const int T = B * H * W, sh = a->shifted;
  // the geometry of the engine's stages for B images and the weights packed as nuhtc_finalize packs them, in private scratch
  DevScratch sc;
  bool ok = upload_stage_maps(g, stage_maps(g, B), B, [&](const auto& v) { return sc.upload(v); });
  BlockW w{};
  w.n1g = sc.upload(a->ln_g, C); w.n1b = sc.upload(a->ln_b, C);
  w.qkv_w = sc.upload(a->qkv_w, (size_t)3 * C * C); w.qkv_b = sc.upload(a->qkv_b, (size_t)3 * C);
  w.relbT = sc.upload(pack_rel_bias(a->rel_table, g.nH));
  w.route = block_route(a->pipe, C);
  const void* qkv_split = nullptr;
  int rc = 0;
  if (w.route == ROUTE_FUSED) {
    std::vector<unsigned short> st;
    lnqkv_pack_stream(a->qkv_w, C, st);
    w.qkv_stream = sc.upload(st);
  } else if (w.route == ROUTE_A_LN) {
    std::vector<float> w2, b2;
    fold_ln(a->qkv_w, a->qkv_b, a->ln_g, a->ln_b, 3 * C, C, w2, b2);
    std::vector<unsigned short> sp;
    if ((rc = gemm_make_split(w2.data(), 3 * C, C, sp))) FAIL(e, rc, "window_msa op: gemm_make_split failed");
    w.qkv_wln = sc.upload(w2); w.qkv_bln = sc.upload(b2);
    qkv_split = sc.upload(sp);
  }
  float* qkv = sc.alloc<float>(((size_t)B * g.nW * WS2 + 1) * 3 * C * sizeof(float));
  float* xw = sc.alloc<float>((size_t)T * C * sizeof(float));
  float* st = sc.alloc<float>((size_t)T * 2 * sizeof(float));
  if (!ok || !sc.ok()) FAIL(e, NUHTC_E_HIP, "window_msa op: scratch upload failed");
  rc = run_attn_front(e, g, w, B, sh, a->x, xw, qkv, a->out, a->out_order == NUHTC_ORDER_TOKEN ? g.map[sh] : g.cidx[sh], nullptr, st, qkv_split, s);
  return op_finish(e, rc, s, "window_msa launch failed", "window_msa kernels failed");
}

// ---- the front of the path and the small dense kernels, op by op (tests/test_hip_front.py): each entry goes through the host code the engine
// uses for the same launch (resize_geom, norm_consts, pack_patch_embed, lateral_params + fold_ln, pool_layout)
int nuhtc_op_patch_embed(nuhtc_engine* e, const uint8_t* tiles_dev, int B, int th, int tw, int valid_h, int valid_w, float scale_factor, int channel_mode,
                         const float* mean, const float* std, const float* w_host, const float* b_host, const float* ln_g_host, const float* ln_b_host,
                         float* tok_dev, float* img_dev, void* stream) {
  if (!e || !tiles_dev || !mean || !std || !w_host || !b_host || !ln_g_host || !ln_b_host || !tok_dev) return NUHTC_E_INVALID;
  if (B < 1 || th < 1 || tw < 1 || valid_h < 1 || valid_w < 1 || valid_h > th || valid_w > tw) FAIL(e, NUHTC_E_INVALID, "patch_embed op: valid_h / valid_w must lie in [1, tile]");
  if (channel_mode != NUHTC_CH_AS_IS && channel_mode != NUHTC_CH_SWAP) FAIL(e, NUHTC_E_INVALID, "patch_embed op: unknown channel mode");
  if (!resize_ok(valid_h, valid_w, scale_factor)) FAIL(e, NUHTC_E_INVALID, "patch_embed op: scale_factor must be in [1,8] and scale_factor * image size must be integers");
  const ResizeGeom rg = resize_geom(valid_h, valid_w, scale_factor);
  if ((long long)B * rg.Hn * rg.Wn * 6 >= (1ll << 31)) FAIL(e, NUHTC_E_INVALID, "patch_embed op: size out of range");
  HIP_CHECK(e, hipSetDevice(e->device));
  hipStream_t s = (hipStream_t)stream;
  float mi[6];
  norm_consts(mean, std, mi);
  DevScratch sc;
  const int *xtab = sc.upload(rg.tx), *ytab = sc.upload(rg.ty);
  const float *w = sc.upload(pack_patch_embed(w_host)), *b = sc.upload(b_host, 96), *g = sc.upload(ln_g_host, 96), *beta = sc.upload(ln_b_host, 96);
  if (!sc.ok()) FAIL(e, NUHTC_E_HIP, "patch_embed op: scratch upload failed");
  const int swap = channel_mode == NUHTC_CH_SWAP;
  int rc = launch_patch_embed_tiles(tiles_dev, B, th, tw, rg.Hn, rg.Wn, rg.Hv, rg.Wv, xtab, ytab, swap, mi, w, b, g, beta, tok_dev, s);
  if (!rc && img_dev) rc = launch_preproc(tiles_dev, img_dev, B, th, tw, rg.Hn, rg.Wn, rg.Hv, rg.Wv, xtab, ytab, swap, mi, s);
  return op_finish(e, rc, s, "patch_embed launch failed", "patch_embed kernels failed");
}

int nuhtc_op_layernorm(nuhtc_engine* e, const float* x_dev, const float* g_dev, const float* b_dev, float* y_dev, int rows, int C, void* stream) {
  if (!e || !x_dev || !g_dev || !b_dev || !y_dev) return NUHTC_E_INVALID;
  if (rows < 1 || (C != 96 && C != 192 && C != 384 && C != 768) || (long long)rows * C >= (1ll << 31)) FAIL(e, NUHTC_E_INVALID, "layernorm op: rows >= 1, C in {96, 192, 384, 768}");
  HIP_CHECK(e, hipSetDevice(e->device));
  hipStream_t s = (hipStream_t)stream;
  const int rc = launch_layernorm(x_dev, nullptr, g_dev, b_dev, y_dev, rows, C, s);
  return op_finish(e, rc, s, "layernorm launch failed", "layernorm kernel failed");
}

int nuhtc_op_merge_ln(nuhtc_engine* e, const float* x_dev, const float* g_dev, const float* b_dev, float* y_dev, int B, int H, int W, int C, void* stream) {
  if (!e || !x_dev || !g_dev || !b_dev || !y_dev) return NUHTC_E_INVALID;
  if (B < 1 || H < 2 || W < 2 || (H & 1) || (W & 1)) FAIL(e, NUHTC_E_INVALID, "merge_ln op: H and W must be even (the network input is a multiple of 32)");
  if ((C != 96 && C != 192 && C != 384) || (long long)B * H * W * C >= (1ll << 31)) FAIL(e, NUHTC_E_INVALID, "merge_ln op: C in {96, 192, 384}");
  HIP_CHECK(e, hipSetDevice(e->device));
  hipStream_t s = (hipStream_t)stream;
  const int rc = launch_merge_ln(x_dev, g_dev, b_dev, y_dev, B, H, W, C, s);
  return op_finish(e, rc, s, "merge_ln launch failed", "merge_ln kernel failed");
}

int nuhtc_op_fpn_lateral(nuhtc_engine* e, const float* X_dev, int B, int H, int W, int C, const float* W_host, const float* bias_host, const float* ln_g_host,
                         const float* ln_b_host, const float* parent_dev, float* out_dev, void* stream) {
  if (!e || !X_dev || !W_host || !bias_host || !out_dev || (ln_g_host == nullptr) != (ln_b_host == nullptr)) return NUHTC_E_INVALID;
  if (B < 1 || H < 1 || W < 1 || (C != 96 && C != 192 && C != 384 && C != 768) || (long long)B * H * W * C >= (1ll << 31)) FAIL(e, NUHTC_E_INVALID, "fpn_lateral op: size out of range");
  if (parent_dev && ((H & 1) || (W & 1))) FAIL(e, NUHTC_E_INVALID, "fpn_lateral op: a map with a parent has even sides");
  HIP_CHECK(e, hipSetDevice(e->device));
  hipStream_t s = (hipStream_t)stream;
  const int T = B * H * W;
  DevScratch sc;
  GemmParams p;
  int rc = 0;
  if (ln_g_host) {      // the split pipe's form: the stage's output norm folded into the lateral, statistics as the producers' epilogues leave them
    std::vector<float> wl, bl;
    fold_ln(W_host, bias_host, ln_g_host, ln_b_host, 64, C, wl, bl);
    std::vector<unsigned short> split;
    if ((rc = gemm_make_split(wl.data(), 64, C, split))) FAIL(e, rc, "gemm_make_split failed");
    float* st = sc.alloc<float>((size_t)T * (C / 96) * 2 * sizeof(float));
    p = lateral_params(X_dev, sc.upload(wl), sc.upload(bl), out_dev, B, H, W, C, st, parent_dev);
    p.Wsplit = sc.upload(split);
    if (!sc.ok()) FAIL(e, NUHTC_E_HIP, "fpn_lateral op: scratch upload failed");
    rc = launch_ln_stats(X_dev, st, T * (C / 96), 96, s);
  } else {              // the fp32 pipe's form: the norm ran before (layernorm_kernel), the weight has no split
    p = lateral_params(X_dev, sc.upload(W_host, (size_t)64 * C), sc.upload(bias_host, 64), out_dev, B, H, W, C, nullptr, parent_dev);
    if (!sc.ok()) FAIL(e, NUHTC_E_HIP, "fpn_lateral op: scratch upload failed");
  }
  if (!rc) rc = launch_gemm(p, s);
  return op_finish(e, rc, s, "fpn_lateral launch failed", "fpn_lateral kernels failed");
}

int nuhtc_op_sem_fuse(nuhtc_engine* e, const float* g0, const float* g1, const float* g2, const float* g3, float* out, int B, int H, int W, void* stream) {
  if (!e || !g0 || !g1 || !g2 || !g3 || !out) return NUHTC_E_INVALID;
  if (B < 1 || H < 8 || W < 8 || H % 8 || W % 8 || (long long)B * H * W * 64 >= (1ll << 31)) FAIL(e, NUHTC_E_INVALID, "sem_fuse op: H and W must be multiples of 8 (level 0 of a network input that is a multiple of 32)");
  HIP_CHECK(e, hipSetDevice(e->device));
  hipStream_t s = (hipStream_t)stream;
  const int rc = launch_sem_fuse(g0, g1, g2, g3, out, B, H, W, s);
  return op_finish(e, rc, s, "sem_fuse launch failed", "sem_fuse kernel failed");
}

int nuhtc_op_pointwise64(nuhtc_engine* e, const float* x_dev, const float* w_dev, const float* b_dev, float* y_dev, int rows, const int32_t* rows_dev,
                         int rows_mul, int sigmoid, void* stream) {
  if (!e || !x_dev || !w_dev || !b_dev || !y_dev) return NUHTC_E_INVALID;
  if (rows < 1 || (long long)rows * 64 >= (1ll << 31)) FAIL(e, NUHTC_E_INVALID, "pointwise64 op: rows out of range");
  if (!rows_dev && sigmoid) FAIL(e, NUHTC_E_INVALID, "pointwise64 op: the fixed-row form has no sigmoid");
  if (rows_dev && rows_mul < 1) FAIL(e, NUHTC_E_INVALID, "pointwise64 op: rows_mul must be >= 1");
  HIP_CHECK(e, hipSetDevice(e->device));
  hipStream_t s = (hipStream_t)stream;
  const int rc = rows_dev ? launch_conv1x1_n1_dev(x_dev, w_dev, b_dev, y_dev, rows, rows_dev, rows_mul, sigmoid ? 1 : 0, s)
                          : launch_conv1x1_n1(x_dev, w_dev, b_dev, y_dev, rows, 64, s);
  return op_finish(e, rc, s, "pointwise64 launch failed", "pointwise64 kernel failed");
}

int nuhtc_op_fpn_mean_pool(nuhtc_engine* e, const float* const maps[4], const int32_t hw[4], int B, float* feat_dev, void* stream) {
  if (!e || !maps || !hw || !feat_dev || B < 1) return NUHTC_E_INVALID;
  PoolLevels p{};
  int hwi[4];
  for (int l = 0; l < 4; ++l) {
    if (!maps[l] || hw[l] < 1 || (long long)B * hw[l] * 64 >= (1ll << 31)) FAIL(e, NUHTC_E_INVALID, "fpn_mean_pool op: null or empty level");
    hwi[l] = hw[l];
    p.x[l] = maps[l];
  }
  int rc = pool_layout(hwi, p);
  if (rc) FAIL(e, rc, "pool_chunks: empty FPN level");
  HIP_CHECK(e, hipSetDevice(e->device));
  hipStream_t s = (hipStream_t)stream;
  DevScratch sc;
  double* slab = sc.alloc<double>(pool_slab_bytes(p, B));
  if (!sc.ok()) FAIL(e, NUHTC_E_HIP, "fpn_mean_pool op: scratch allocation failed");
  rc = launch_fpn_mean_pool(p, B, slab, feat_dev, s);
  return op_finish(e, rc, s, "fpn_mean_pool launch failed", "fpn_mean_pool kernels failed");
}

#ifdef NUHTC_DEV
// dev (tools/dev/r04_state_buffers.py): gives one of the Swin activation buffers new memory (the old allocation stays until nuhtc_destroy, so the
// new one lands elsewhere).  which: 0 tokA, 1 tokB, 2 xw, 3 qkv, 4 att, 5 hid; returns the new device address through *addr
extern "C" int nuhtc_dev_realloc(nuhtc_engine* e, int which, unsigned long long* addr) {
  if (!e || which < 0 || which > 5) return NUHTC_E_INVALID;
  HIP_CHECK(e, hipSetDevice(e->device));
  HIP_CHECK(e, hipDeviceSynchronize());
  float** slots[6] = {&e->tokA, &e->tokB, &e->xw, &e->qkv, &e->att, &e->hid};
  void* base = nullptr;
  size_t bytes = 0;
  HIP_CHECK(e, hipMemGetAddressRange((hipDeviceptr_t*)&base, &bytes, (hipDeviceptr_t)*slots[which]));
  void* p = nullptr;
  HIP_CHECK(e, hipMalloc(&p, bytes));
  HIP_CHECK(e, hipMemset(p, 0, bytes));
  e->allocs.push_back(p);
  *slots[which] = (float*)p;
  if (which == 0) e->bufs["tokens"].ptr = p;
  e->tok[0] = e->tokA; e->tok[1] = e->tokB;
  if (addr) *addr = (unsigned long long)p;
  return 0;
}
#endif
