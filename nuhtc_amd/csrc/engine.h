// Engine state of libnuhtc_hip.so (host side).
#pragma once
#include <unordered_map>

#include "common.h"

struct StageGeom {
  int H, W, C, nH;     // token grid, channels, heads
  int Hp, Wp, nW;      // padded grid (multiple of 7) and windows per image
  int* map[2];         // dev: window-row -> token index (-1 = padding), [max_batch*nW*49], un-shifted / shifted
  int* cidx[2];        // dev: window-row -> index among the non-padding window rows (-1 = padding); tile b's rows are [b*H*W, (b+1)*H*W)
  int* ctok[2];        // dev: that compact index -> token index, [max_batch*H*W]
  int* vrow[2];        // dev: that compact index -> window row
  // the attention kernel of the split pipe never reads a padding row: bit j of padbits[shift][window of the image] says row j of the window
  // is one, and the kernel reads row `bias_row` (one row behind the window image of the largest batch, holding the block's QKV bias) instead
  unsigned long long* padbits[2];
  int* brow;           // dev: {bias_row}, the one-entry "padding row list" of the launches that write it
  int bias_row;
  float* mask;         // dev: shift mask, packed per lane [nW][4096] (engine.hip pack_attn_terms)
  int* mask_any;       // dev: [nW] 1 where the window's mask has a non-zero entry
};

// Which kernels a Swin block runs through (engine.hip block_route): layernorm kernels + plain linears | the norms in the A path of the QKV / fc1
// linears | the fused LN1 + QKV kernel and the fused projection + FFN kernel (mlp.hip)
enum BlockRoute { ROUTE_PLAIN, ROUTE_A_LN, ROUTE_FUSED };

struct BlockW {
  BlockRoute route;
  float *n1g, *n1b, *relbT /* relative-position bias packed per lane [nH][4096] */, *qkv_w, *qkv_b, *proj_w, *proj_b, *n2g, *n2b, *f1_w, *f1_b, *f2_w, *f2_b;
  // ROUTE_A_LN (gemm.hip A_LN): the norm's affine part folded into the linear behind it -- W' = W diag(gamma), b' = b + W beta (fp64 on the
  // host, rounded once); null on the other routes
  float *qkv_wln, *qkv_bln, *f1_wln, *f1_bln;
  // ROUTE_FUSED (mlp.hip), null on the other routes:
  void* qkv_stream;    // fused LN1 + QKV: k-permuted split planes of qkv_w
  void* mlp_stream;    // fused FFN half: chunk-major split planes of f1_w / f2_w
  void* proj_stream;   // attention projection in front of the fused FFN half: k-permuted split planes of proj_w
};

struct nuhtc_engine {
  nuhtc_config cfg;
  int device = 0;
  std::string err;
  std::map<std::string, HostTensor> raw;
  std::map<std::string, std::vector<int64_t>> schema;   // names / shapes nuhtc_load_weight accepts
  std::map<std::string, BufInfo> bufs;
  std::vector<void*> allocs;
  // fp32 weight pointer -> its exact bf16 split (gemm_make_split), filled by upload_gemm_weight at finalize and read by egemm for every
  // launch: the engine's own table (a handle is not thread-safe by contract, so no lock); the buffers are in `allocs`
  // the entry records the [N][K] geometry the split was made for: egemm hands it out only to a launch of exactly that geometry
  struct WSplit { const void* planes; int N, K; };
  std::unordered_map<const float*, WSplit> wsplit;
  bool finalized = false;
  bool debug_tokens = false;
  int lastB = 0;
  int Hn = 0, Wn = 0;     // network input = pad_shape: img_shape rounded up to a multiple of 32
  int Hv = 0, Wv = 0;     // img_shape = scale_factor * valid image size (boxes are clipped to it)
  int vh = 0, vw = 0;     // ori_shape = the image inside the tile buffer
  int *rs_xtab = nullptr, *rs_ytab = nullptr;   // cv2 linear-resize tables (swin.hip preproc)

  StageGeom st[4];
  // backbone weights
  float *pe_w = nullptr, *pe_b = nullptr, *pe_g = nullptr, *pe_beta = nullptr;
  std::vector<BlockW> blocks[4];
  // decided at finalize from what was packed: PatchMerging of stage st in one launch (mg_wln[st]: split pipe and even H, W), the output norms in the
  // FPN laterals (lat_wln: split pipe), the pointwise layers in the 3x3 convolutions' epilogues (rpn_hf: split pipe and detection heads)
  bool merge_one_launch[3] = {}, out_ln_folded = false, conv_fuse = false;
  float *on_g[4], *on_b[4], *mg_g[3], *mg_b[3], *mg_w[3];
  float *mg_wln[3] = {}, *mg_bln[3] = {};   // PatchMerging norm folded into its reduction linear (gemm.hip A_LN, two segments): W diag(gamma), W beta
  int* mg_src[3] = {};                     // dev: merged row -> its top-left token (b, 2 y2, 2 x2) of the stage's token tensor, [max_batch * H/2 * W/2]
  // neck / dense heads
  float *lat_w[4], *lat_b[4], *fpn_w[4], *fpn_b[4];
  float *rpn_w, *rpn_b, *rpn_hw, *rpn_hb;
  void *rpn_hf, *sem_lf[4], *sem_ef;   // pointwise layers as conv3_pack_fuse images (split pipe): computed in the epilogue of the 3x3 convolution before them
  float *sem_lw[4], *sem_lb[4], *sem_cw[4], *sem_cb[4], *sem_ew, *sem_eb, *sem_gw, *sem_gb;
  // roi heads
  float *fc1_w[3], *fc1_b[3], *fc2_w[3], *fc2_b[3], *head_w[3], *head_b[3];   // head_w: [16][256] rows 0..nc+1 normed cls, then 4 reg
  float *mk_w[4], *mk_b[4], *mk_up_w, *mk_up_b, *mk_lw, *mk_lb;

  // workspace
  float *img, *tokA, *tokB, *xw, *qkv, *att, *hid;
  // Output norms of the stages (swin.py:756-762) in the A path of the FPN lateral that consumes them (split pipe): every stage keeps its own token
  // buffer and the partials of its final tensor until the neck has run; c[st] then exists only on request (nuhtc_get_buffer computes it)
  float* tok[4] = {};           // tok[0] = tokA, tok[1] = tokB, two more
  float* ln_out[4] = {};        // partials of the stage's final tensor, left by its last block's FFN
  float *lat_wln[4] = {}, *lat_bln[4] = {};   // lateral 1x1 with the output norm folded in: W diag(gamma), b + W beta
  // pre-processing inside the patch embedding: the tiles of the running call; `img` is computed only on request (nuhtc_get_buffer)
  const uint8_t* in_tiles = nullptr;
  int in_swap = 0;
  int last_batch = 0;
  float* ln_part2 = nullptr;   // the partials the patch-merging GEMM leaves for the next stage's first block (it READS ln_part in the same launch)
  float* ln_part = nullptr;    // LayerNorm partials of the current token tensor, [token][C / 96][2] = {mean, sum of squared deviations} per 96 channels:
                               // written by the epilogue of the GEMM that produced the tensor (proj, fc2, patch merging), read by the next A_LN linear
  float *c[4], *lat[4], *x[4], *rpn[4], *semg[4];
  float *tmpA, *tmpB, *tmpR, *sem_feat, *sem_pred, *x0sem;   // tmpR: RPN conv output (side stream)
  // nuhtc_features (pool.hip): the four maps x[l], their chunk layout and the fp64 partials of the mean
  PoolLevels pool{};
  double* pool_slab = nullptr;
  // proposals / roi path
  int roi_cap = 0;          // rois per tile: max_cc_proposals + rpn_max_per_img
  int cand_cap = 0;         // rpn candidates per tile (<= 4 * nms_pre), det candidates per tile
  int* overflow = nullptr;  // dev int[4]
  int* overflow_host = nullptr;   // pinned int[4]: nuhtc_check copies the flags on the caller's stream (a synchronous hipMemcpy goes through the null stream and waited ~6 ms per call in a loop that keeps four batches in flight)
  int32_t* export_pos = nullptr;   // nuhtc_export_kept scratch [max_batch * max_per_img]
  int32_t* crop_size = nullptr;    // nuhtc_export_crops scratch [max_batch * max_per_img]
  hipStream_t own = nullptr;        // a stream for the caller to run this engine on (nuhtc_stream): created right before the two side streams
  hipStream_t side = nullptr;       // proposal selection / NMS run here, concurrently with the semantic head on the caller's stream
  hipEvent_t ev_rpn = nullptr, ev_side = nullptr, ev_fpn = nullptr;
  hipStream_t side2 = nullptr;      // the big-box RoI kernel runs here, beside the stream kernel (side) and the LDS-tile kernels (caller's stream)
  hipEvent_t ev_side2 = nullptr;
  struct RoiWs* rw = nullptr;
};

// ---- engine construction (engine.hip): device memory that lives until nuhtc_destroy, weights from the checkpoint
// a device allocation of the engine, rounded up to 256 bytes
int dev_alloc(nuhtc_engine* e, void** p, size_t bytes);
// a host image -> new engine memory (the split and stream images of the matrix pipe, see upload for typed vectors)
int upload_bytes(nuhtc_engine* e, void** dst, const void* host, size_t bytes);
template <typename T>
int upload(nuhtc_engine* e, T** dst, const std::vector<T>& v) {
  return upload_bytes(e, (void**)dst, v.data(), v.size() * sizeof(T));
}
// workspace of `shape` elements of T; with a name it is listed for nuhtc_get_buffer
template <typename T>
int ws(nuhtc_engine* e, T** p, const char* name, std::vector<int64_t> shape, int dtype) {
  size_t n = 1;
  for (auto d : shape) n *= (size_t)d;
  int rc = dev_alloc(e, (void**)p, n * sizeof(T));
  if (rc) return rc;
  if (name) e->bufs[name] = BufInfo{(void*)*p, shape, dtype};
  return 0;
}
// the checkpoint tensor `name`, which must have `shape` (null and e->err set otherwise)
const HostTensor* raw(nuhtc_engine* e, const std::string& name, std::initializer_list<int64_t> shape);
#define RAW(var, name, ...)                                 \
  const HostTensor* var = raw(e, (name), {__VA_ARGS__});    \
  if (!var) return NUHTC_E_STATE;
// [O][I][3][3] -> [O][(ky*3+kx)*I + i]
std::vector<float> pack_conv3(const HostTensor& w, int O, int I);
// uploads a GEMM weight [N][K] and, unless cfg.matrix_pipe == NUHTC_PIPE_FP32, its exact bf16 split (gemm.hip) into e->wsplit
int upload_gemm_weight(nuhtc_engine* e, float** dst, const std::vector<float>& v, int N, int K);

// ---- launch sequence
// a plain product: lda = K, ldc = N, alpha 1, everything else off
GemmParams gp(const float* A, const float* W, const float* bias, float* C, int M, int N, int K);
// runs a launch_* call inside a function of the engine that returns an error code; a failure is returned with e->err naming the call
#define RUN(expr)                                                                                        \
  do {                                                                                                   \
    int _rc = (expr);                                                                                    \
    if (_rc) { e->err = std::string(#expr) + " failed (" + std::to_string(_rc) + ")"; return _rc; }     \
  } while (0)
// the end of an op entry point (a test hook) that launched work on `s`: waits for it, then reports a refused launch (rc != 0) or a failed kernel
inline int op_finish(nuhtc_engine* e, int rc, hipStream_t s, const char* launch_err, const char* kernel_err) {
  const hipError_t he = hipStreamSynchronize(s);
  if (rc) FAIL(e, rc, launch_err);
  if (he != hipSuccess) FAIL(e, NUHTC_E_HIP, kernel_err);
  return 0;
}
// launch_gemm with the split of p.W taken from the engine's table (bf16 matrix pipe) when the engine has one
int egemm(nuhtc_engine* e, GemmParams p, hipStream_t s);
int finalize_roi(nuhtc_engine* e);
int alloc_roi_workspace(nuhtc_engine* e);
// rois_fixed != null -> fixed-load mode
int run_roi_path(nuhtc_engine* e, int B, const float* rois_fixed, int n_rois, int n_dets, hipStream_t s, const nuhtc_dets* out);
int run_backbone(nuhtc_engine* e, int B, hipStream_t s);
int run_neck_heads(nuhtc_engine* e, int B, hipStream_t s);
// the FPN half of run_neck_heads (laterals + fpn_convs -> x[0..3]); sem_lateral: the semantic head's lateral 1x1 rides in the
// fpn_convs' epilogue (Conv3Fuse, detection path) -- off for nuhtc_features
int run_fpn(nuhtc_engine* e, int B, hipStream_t s, bool sem_lateral);
int launch_conv1x1_n1_dev(const float* x, const float* w, const float* b, float* y, int rows_cap, const int* rows_dev, int rows_mul,
                          int sigmoid, hipStream_t s);
