// Host orchestration of the proposal + RoI cascade + mask part of the path
// (nuhtc/models/htc_roi_head_cus.py:2184-2372, mmdet/models/dense_heads/rpn_head.py:103-236, tools/infer_wsi.py:486-531).
// Everything stays on the device: variable RoI / detection counts are device-side integers consumed by the kernels.
#include <cmath>
#include <cstring>

#include "engine.h"
#include "proposals.h"
#include "roi.h"

#define BIG_SPLIT_MAX 512      // big boxes per batch up to which each of a box's maps gets a workgroup of its own (roi_feat7_big_kernel)
struct RoiWs {
  // RPN proposals
  float *cand_boxes, *cand_scores;
  unsigned* rpn_keys;   // [B][4][key_stride]
  int rpn_key_stride;
  int* cand_count;
  float *nms_sboxes;
  int *nms_src, *nms_ntotal, *nms_seg_start, *nms_seg_n, *nms_pos;
  unsigned long long* nms_keepbits;
  unsigned long long* nms_mask;
  float* rpn_dets;
  int *rpn_src, *rpn_counts;
  int rpn_slot, rpn_cap, rpn_pow2;
  // connected-component proposals
  unsigned char *cc_a, *cc_b, *cc_touch;
  int *cc_labels, *cc_stats, *cc_counts, *cc_list, *cc_nlist;
  float* cc_boxes;
  // rois + cascade
  float* rois;
  int *roi_off, *roi_cnt, *roi_total;
  float *G2, *G3, *ap_inv, *ap_S, *ap_Ft;
  float *feats, *h1, *h2;
  int *fb_count, *fb_list, *mid_list;
  float* big_part;      // per-map partial features of the big boxes while they are few (roi_feat7_big_kernel)
  unsigned char* fb_flag;
  float *cls[3], *reg[3];
  int total_cap;
  // detections
  float *dc_boxes, *dc_scores;
  int *dc_ids, *dc_count;
  int det_cap, det_pow2;
  float* det_dets;      // used when the caller passes no output struct
  int *det_src, *det_counts, *det_labels;
  // mask branch
  float* mask_rois;
  int *det_off, *det_total;
  float *mfeat, *mtmpA, *mtmpB, *mup, *mprob;
  int mask_cap;
  unsigned* masks_own;
  int* areas_own;
  unsigned char* keep_own;
};

// fc_cls [nc+2][256] / fc_reg [4][256] of one bbox head -> the [nc+6][256] weight and [nc+6] bias bbox_tail_kernel reads (also nuhtc_op_bbox_tail)
static void pack_bbox_head(const float* wc, const float* bc, const float* wr, const float* br, int nc, std::vector<float>& hw, std::vector<float>& hb) {
  // NormedLinear: weight_ = W / (||W||_row + 1e-6)   (normed_predictor.py:34-35)
  hw.assign((size_t)(nc + 6) * 256, 0.f);
  hb.assign(nc + 6, 0.f);
  for (int n = 0; n < nc + 2; ++n) {
    float ss = 0.f;
    for (int k2 = 0; k2 < 256; ++k2) ss += wc[n * 256 + k2] * wc[n * 256 + k2];
    float den = sqrtf(ss) + 1e-6f;
    for (int k2 = 0; k2 < 256; ++k2) hw[n * 256 + k2] = wc[n * 256 + k2] / den;
    hb[n] = bc[n];
  }
  for (int n = 0; n < 4; ++n) {
    for (int k2 = 0; k2 < 256; ++k2) hw[(nc + 2 + n) * 256 + k2] = wr[n * 256 + k2];
    hb[nc + 2 + n] = br[n];
  }
}
// the reference compares the mask IoU against the Python double 0.05 (tools/infer_wsi.py:60-84), not against its float image
static double mask_nms_thr(float thr) { return std::round((double)thr * 1e6) / 1e6; }

int finalize_roi(nuhtc_engine* e) {
  const int nc = e->cfg.num_classes;
  int rc;
  for (int k = 0; k < 3; ++k) {
    const std::string p = "roi_head.bbox_head." + std::to_string(k) + ".";
    RAW(w1, p + "shared_fcs.0.weight", 256, 3136); RAW(b1, p + "shared_fcs.0.bias", 256);
    RAW(w2, p + "shared_fcs.1.weight", 256, 256); RAW(b2, p + "shared_fcs.1.bias", 256);
    RAW(wc, p + "fc_cls.weight", nc + 2, 256); RAW(bc, p + "fc_cls.bias", nc + 2);
    RAW(wr, p + "fc_reg.weight", 4, 256); RAW(br, p + "fc_reg.bias", 4);
    // flatten order of the reference is (c, ph, pw); the RoI kernel emits (ph, pw, c)
    std::vector<float> w1p((size_t)256 * 3136);
    for (int n = 0; n < 256; ++n)
      for (int c = 0; c < 64; ++c)
        for (int bin = 0; bin < 49; ++bin) w1p[(size_t)n * 3136 + bin * 64 + c] = w1->data[(size_t)n * 3136 + c * 49 + bin];
    std::vector<float> hw, hb;
    pack_bbox_head(wc->data.data(), bc->data.data(), wr->data.data(), br->data.data(), nc, hw, hb);
    if ((rc = upload_gemm_weight(e, &e->fc1_w[k], w1p, 256, 3136)) || (rc = upload(e, &e->fc1_b[k], b1->data)) || (rc = upload_gemm_weight(e, &e->fc2_w[k], w2->data, 256, 256)) ||
        (rc = upload(e, &e->fc2_b[k], b2->data)) || (rc = upload(e, &e->head_w[k], hw)) || (rc = upload(e, &e->head_b[k], hb)))
      return rc;
  }
  {
    const std::string p = "roi_head.mask_head.0.";
    for (int j = 0; j < 4; ++j) {
      RAW(w, p + "convs." + std::to_string(j) + ".conv.weight", 64, 64, 3, 3);
      RAW(b, p + "convs." + std::to_string(j) + ".conv.bias", 64);
      if ((rc = upload_gemm_weight(e, &e->mk_w[j], pack_conv3(*w, 64, 64), 64, 576)) || (rc = upload(e, &e->mk_b[j], b->data))) return rc;
    }
    RAW(uw, p + "upsample.weight", 64, 64, 2, 2); RAW(ub, p + "upsample.bias", 64);
    RAW(lw, p + "conv_logits.weight", 1, 64, 1, 1); RAW(lb, p + "conv_logits.bias", 1);
    // ConvTranspose2d(k=2,s=2) weight [in][out][kh][kw] -> GEMM weight [(kh*2+kw)*64 + oc][ic]
    std::vector<float> w((size_t)256 * 64), b(256);
    for (int ic = 0; ic < 64; ++ic)
      for (int oc = 0; oc < 64; ++oc)
        for (int t = 0; t < 4; ++t) w[((size_t)t * 64 + oc) * 64 + ic] = uw->data[((size_t)ic * 64 + oc) * 4 + t];
    for (int t = 0; t < 4; ++t)
      for (int oc = 0; oc < 64; ++oc) b[t * 64 + oc] = ub->data[oc];
    if ((rc = upload_gemm_weight(e, &e->mk_up_w, w, 256, 64)) || (rc = upload(e, &e->mk_up_b, b)) || (rc = upload(e, &e->mk_lw, lw->data)) || (rc = upload(e, &e->mk_lb, lb->data))) return rc;
  }
  return 0;
}

static int round_up(int v, int m) { return (v + m - 1) / m * m; }
static int pow2_ge(int v) { int p = 2; while (p < v) p <<= 1; return p; }

int alloc_roi_workspace(nuhtc_engine* e) {
  const nuhtc_config& c = e->cfg;
  const int B = c.max_batch;
  const int Hn = e->Hn, Wn = e->Wn;
  RoiWs* w = new RoiWs();
  memset(w, 0, sizeof(*w));
  e->rw = w;
  int rc;
  if ((rc = nms_set_attributes())) { e->err = "hipFuncSetAttribute(nms_prepare) failed"; return rc; }
  // RPN candidates: per level min(nms_pre, anchors)
  w->rpn_slot = c.rpn_nms_pre;
  int maxc = 0;
  for (int l = 0; l < 4; ++l) maxc += std::min(c.rpn_nms_pre, e->st[l].H * e->st[l].W * 3);
  w->rpn_cap = round_up(std::max(maxc, 64), 64) + 64 * 3;   // each level's segment of the sorted list is 64-aligned (launch_nms_levels)
  w->rpn_pow2 = pow2_ge(maxc);
  e->roi_cap = c.max_cc_proposals + c.rpn_max_per_img;
  w->det_cap = round_up(e->roi_cap * c.num_classes, 64);
  w->det_pow2 = pow2_ge(e->roi_cap * c.num_classes);
  if (maxc > NMS_MAX_CAP || w->det_cap > NMS_MAX_CAP) { e->err = "candidate capacity exceeds NMS_MAX_CAP (reduce rpn_nms_pre / max_cc_proposals)"; return NUHTC_E_INVALID; }
  const int nmscap = std::max(w->rpn_cap, w->det_cap);
  w->rpn_key_stride = round_up(e->st[0].H * e->st[0].W * 3, 64);
  if ((rc = ws(e, &w->rpn_keys, nullptr, {B, 4, w->rpn_key_stride}, 1)) ||
      (rc = ws(e, &w->cand_boxes, "rpn_cand_boxes", {B, 4, w->rpn_slot, 4}, 0)) || (rc = ws(e, &w->cand_scores, "rpn_cand_scores", {B, 4, w->rpn_slot}, 0)) ||
      (rc = ws(e, &w->cand_count, "rpn_cand_count", {B, 4}, 1)) || (rc = ws(e, &w->nms_sboxes, nullptr, {B, nmscap, 4}, 0)) ||
      (rc = ws(e, &w->nms_src, nullptr, {B, nmscap}, 1)) || (rc = ws(e, &w->nms_ntotal, nullptr, {B}, 1)) ||
      (rc = ws(e, &w->nms_seg_start, nullptr, {B, 4}, 1)) || (rc = ws(e, &w->nms_seg_n, nullptr, {B, 4}, 1)) ||
      (rc = ws(e, &w->nms_pos, nullptr, {B, nmscap}, 1)) || (rc = ws(e, &w->nms_keepbits, nullptr, {B, nmscap / 64}, 3)) ||
      (rc = ws(e, &w->nms_mask, nullptr, {B, nmscap, nmscap / 64}, 3)) || (rc = ws(e, &w->rpn_dets, "rpn_props", {B, c.rpn_max_per_img, 5}, 0)) ||
      (rc = ws(e, &w->rpn_src, nullptr, {B, c.rpn_max_per_img}, 1)) || (rc = ws(e, &w->rpn_counts, "rpn_counts", {B}, 1)))
    return rc;
  const int64_t HW = (int64_t)Hn * Wn;
  const int ccc = std::max(c.max_cc_proposals, 1);
  if ((rc = ws(e, &w->cc_a, nullptr, {B, HW}, 2)) || (rc = ws(e, &w->cc_b, "cc_mask", {B, Hn, Wn}, 2)) || (rc = ws(e, &w->cc_touch, nullptr, {B, HW}, 2)) ||
      (rc = ws(e, &w->cc_labels, "cc_labels", {B, Hn, Wn}, 1)) || (rc = ws(e, &w->cc_stats, nullptr, {B, HW, 5}, 1)) ||
      (rc = ws(e, &w->cc_list, nullptr, {B, CC_LIST_CAP}, 1)) || (rc = ws(e, &w->cc_nlist, nullptr, {B}, 1)) ||
      (rc = ws(e, &w->cc_boxes, "cc_props", {B, ccc, 4}, 0)) || (rc = ws(e, &w->cc_counts, "cc_counts", {B}, 1)) ||
      (rc = ws(e, &e->overflow, nullptr, {4}, 1)))
    return rc;
  w->total_cap = B * e->roi_cap;
  const int T = w->total_cap;
  if ((rc = ws(e, &w->rois, "rois", {T, 5}, 0)) || (rc = ws(e, &w->roi_off, "roi_off", {B}, 1)) || (rc = ws(e, &w->roi_cnt, "roi_counts", {B}, 1)) ||
      (rc = ws(e, &w->roi_total, "roi_total", {1}, 1)) || (rc = ws(e, &w->G2, "G2", {B, e->st[2].H * e->st[2].W, 64}, 0)) ||
      (rc = ws(e, &w->G3, "G3", {B, e->st[3].H * e->st[3].W, 64}, 0)) || (rc = ws(e, &w->feats, "bbox_feats", {T, 49, 64}, 0)) ||
      (rc = ws(e, &w->h1, nullptr, {T, 256}, 0)) || (rc = ws(e, &w->h2, "h2", {T, 256}, 0)) ||
      (rc = ws(e, &w->ap_inv, nullptr, {B, e->st[2].H * e->st[2].W}, 0)) ||
      (rc = ws(e, &w->ap_S, nullptr, {B, (int64_t)e->st[2].H * e->st[2].W, (int64_t)e->st[2].H * e->st[2].W}, 0)) ||
      (rc = ws(e, &w->ap_Ft, nullptr, {B, 64, e->st[2].H * e->st[2].W}, 0)) ||
      (rc = ws(e, &w->fb_count, "roi_fallback_count", {8}, 1)) || (rc = ws(e, &w->mid_list, nullptr, {T}, 1)) || (rc = ws(e, &w->fb_list, nullptr, {T}, 1)) || (rc = ws(e, &w->fb_flag, nullptr, {T}, 2)))
    return rc;
  if ((rc = ws(e, &w->big_part, nullptr, {BIG_SPLIT_MAX, 3, 49, 64}, 0))) return rc;
  for (int k = 0; k < 3; ++k) {
    std::string n = std::to_string(k);
    if ((rc = ws(e, &w->cls[k], ("cls" + n).c_str(), {T, 16}, 0)) || (rc = ws(e, &w->reg[k], ("reg" + n).c_str(), {T, 4}, 0))) return rc;
    std::string rn = "rois_stage" + n;
    float* snap;
    if ((rc = ws(e, &snap, rn.c_str(), {T, 5}, 0))) return rc;
  }
  if ((rc = ws(e, &w->dc_boxes, nullptr, {B, w->det_cap, 4}, 0)) || (rc = ws(e, &w->dc_scores, nullptr, {B, w->det_cap}, 0)) ||
      (rc = ws(e, &w->dc_ids, nullptr, {B, w->det_cap}, 1)) || (rc = ws(e, &w->dc_count, "det_cand_count", {B}, 1)) ||
      (rc = ws(e, &w->det_src, nullptr, {B, c.max_per_img}, 1)) || (rc = ws(e, &w->det_counts, nullptr, {B}, 1)))
    return rc;
  w->mask_cap = B * c.max_per_img;
  const int D = w->mask_cap;
  if ((rc = ws(e, &w->mask_rois, "mask_rois", {D, 5}, 0)) || (rc = ws(e, &w->det_off, "det_off", {B}, 1)) || (rc = ws(e, &w->det_total, "det_total", {1}, 1)) ||
      (rc = ws(e, &w->mfeat, "mask_feats", {D, 196, 64}, 0)) || (rc = ws(e, &w->mtmpA, nullptr, {D, 196, 64}, 0)) || (rc = ws(e, &w->mtmpB, nullptr, {D, 196, 64}, 0)) ||
      (rc = ws(e, &w->mup, nullptr, {D, 784, 64}, 0)) || (rc = ws(e, &w->mprob, "mask_prob", {D, 28, 28}, 0)))
    return rc;
  if (hipMemset(e->overflow, 0, 16) != hipSuccess) { e->err = "hipMemset failed"; return NUHTC_E_HIP; }
  return 0;
}

// the route NUHTC_AP_AUTO stands for: the reference-on-CUDA fp16 arithmetic with the switch, else the GEMM pair where HW % 32 == 0, else attn_pool_kernel
static int attn_pool_route(const nuhtc_engine* e, int HW, int route) {
  return route != NUHTC_AP_AUTO ? route : e->cfg.att_pool_fp16 ? NUHTC_AP_FP16 : HW % 32 == 0 ? NUHTC_AP_GEMM : NUHTC_AP_KERNEL;
}
// One attention-pool table G [B][HW][64] of a level map F [B][HW][64] (roi_extractors_cus.py:220-238), by `route` (NUHTC_AP_*; AUTO: the reference-on-CUDA
// fp16 arithmetic with the switch, else the GEMM pair where HW % 32 == 0 and attn_pool_kernel otherwise).  inv [B][HW], S [B][HW][HW], Ft [B][64][HW]:
// scratch of the GEMM route.  Also nuhtc_op_attn_pool.
static int attn_pool_table(nuhtc_engine* e, const float* F, float* G, int B, int HW, float tau, int route, float* inv, float* S, float* Ft, hipStream_t s) {
  route = attn_pool_route(e, HW, route);
  if (route == NUHTC_AP_FP16) {
    RUN(launch_attn_pool_fp16(F, G, B, HW, tau, s));      // the reference-on-CUDA rounding (roi_extractors_cus.py:203,231)
  } else if (route == NUHTC_AP_GEMM) {
    if (HW % 32 != 0) FAIL(e, NUHTC_E_INVALID, "attention pool: the GEMM route needs HW % 32 == 0");
    // S = relu(cos(F_q, F_p) - tau) + tau as one batched GEMM F·Fᵀ with the cosine epilogue, then G = S·F / HW
    RUN(launch_rownorm_inv(F, inv, B * HW, 64, s));
    GemmParams p1 = gp(F, F, nullptr, S, HW, HW, 64);
    p1.act = ACT_COS; p1.cos_ri = inv; p1.cos_rj = inv; p1.cos_tau = tau;
    p1.batch = B; p1.sA = (long long)HW * 64; p1.sW = (long long)HW * 64; p1.sC = (long long)HW * HW; p1.sRi = HW; p1.sRj = HW;
    RUN(egemm(e, p1, s));
    RUN(launch_transpose(F, Ft, B, HW, 64, s));
    GemmParams p2 = gp(S, Ft, nullptr, G, HW, 64, HW);
    p2.alpha = 1.0f / (float)HW;
    p2.batch = B; p2.sA = (long long)HW * HW; p2.sW = (long long)HW * 64; p2.sC = (long long)HW * 64;
    RUN(egemm(e, p2, s));
  } else if (route == NUHTC_AP_KERNEL) {
    RUN(launch_attn_pool(F, G, B, HW, tau, s));
  } else FAIL(e, NUHTC_E_INVALID, "attention pool: unknown route");
  return 0;
}

// the list forms of the P = 7 RoI features as the engine sets them (also nuhtc_op_roi_feats); big_part: [BIG_SPLIT_MAX][3][49][64]
static void roi_feat_modes(RoiFeatParams& fp, float* big_part) {
  static const int& stream_few = dev_knob_ref("STREAM_FEW", 1);
  static const int& big_split = dev_knob_ref("BIG_SPLIT", 1);
  fp.stream_few = stream_few;
  fp.big_part = big_split ? big_part : nullptr; fp.big_split_max = BIG_SPLIT_MAX;
}

int run_roi_path(nuhtc_engine* e, int B, const float* rois_fixed, int n_rois, int n_dets, hipStream_t s, const nuhtc_dets* out) {
  const nuhtc_config& c = e->cfg;
  RoiWs* w = e->rw;
  const int Hn = e->Hn, Wn = e->Wn;
  const bool fixed = rois_fixed != nullptr;
  if (!out || !out->boxes || !out->labels || !out->counts) FAIL(e, NUHTC_E_INVALID, "nuhtc_dets.boxes/labels/counts are required");
  if (hipMemsetAsync(e->overflow, 0, 16, s) != hipSuccess) FAIL(e, NUHTC_E_HIP, "hipMemsetAsync failed");

  // ---- RPN proposals (rpn_head.py:103-236)
  if (!fixed) {
    RpnLevels lv;
    for (int l = 0; l < 4; ++l) { lv.out[l] = e->rpn[l]; lv.h[l] = e->st[l].H; lv.w[l] = e->st[l].W; lv.stride[l] = 4 << l; }
    RpnSelParams sp;
    sp.nms_pre = c.rpn_nms_pre; sp.slot = w->rpn_slot; sp.cand_boxes = w->cand_boxes; sp.cand_scores = w->cand_scores; sp.cand_count = w->cand_count; sp.keys = w->rpn_keys; sp.key_stride = w->rpn_key_stride;
    sp.img_h = e->Hv; sp.img_w = e->Wv; sp.min_size = c.rpn_min_bbox_size;      // max_shape = img_shape (rpn_head.py:141,219)
    // RPN selection + NMS depend only on the RPN maps: they run on the side stream, overlapping the semantic head /
    // connected-component kernels the caller's stream is still working through (fork at ev_rpn, join before build_rois)
    hipStream_t s2 = e->cfg.schedule == NUHTC_SCHED_THROUGHPUT ? s : e->side;
    if (s2 != s && hipStreamWaitEvent(s2, e->ev_rpn, 0) != hipSuccess) FAIL(e, NUHTC_E_HIP, "hipStreamWaitEvent failed");
    RUN(launch_rpn_select(lv, sp, B, s2));
    NmsParams np;
    memset(&np, 0, sizeof(np));
    np.boxes = w->cand_boxes; np.scores = w->cand_scores; np.ids = nullptr; np.group_count = w->cand_count; np.n_groups = 4; np.slot = w->rpn_slot;
    np.cap = w->rpn_cap; np.cap_pow2 = w->rpn_pow2; np.iou_thr = c.rpn_nms_iou; np.max_keep = c.rpn_max_per_img;
    np.sorted_boxes = w->nms_sboxes; np.sorted_src = w->nms_src; np.n_total = w->nms_ntotal; np.mask = w->nms_mask;
    np.out_dets = w->rpn_dets; np.out_src = w->rpn_src; np.out_counts = w->rpn_counts;
    np.seg_start = w->nms_seg_start; np.seg_n = w->nms_seg_n; np.sorted_pos = w->nms_pos; np.keepbits = w->nms_keepbits;
    RUN(launch_nms_levels(np, B, s2));
    if (s2 != s && hipEventRecord(e->ev_side, s2) != hipSuccess) FAIL(e, NUHTC_E_HIP, "hipEventRecord failed");
    // ---- connected-component ("watershed") proposals (htc_roi_head_cus.py:283-342)
    if (c.watershed_proposal && c.max_cc_proposals > 0) {
      CcParams cp;
      cp.sem_pred = e->sem_pred; cp.h = e->st[0].H; cp.w = e->st[0].W; cp.img_h = e->Hv; cp.img_w = e->Wv; cp.min_area = 10;   /* interpolated to img_shape (htc_roi_head_cus.py:285,397) */ cp.cap = c.max_cc_proposals;
      cp.mask_a = w->cc_a; cp.mask_b = w->cc_b; cp.touch = w->cc_touch; cp.labels = w->cc_labels; cp.stats = w->cc_stats; cp.boxes = w->cc_boxes;
      cp.counts = w->cc_counts; cp.overflow = e->overflow; cp.list = w->cc_list; cp.nlist = w->cc_nlist;
      RUN(launch_cc_proposals(cp, B, s));
    }
  }
  const bool use_cc = !fixed && c.watershed_proposal && c.max_cc_proposals > 0;
  // ---- attention-pool tables for levels 2, 3 (roi_extractors_cus.py:220-238): independent of the proposals
  for (int l = 2; l < 4; ++l)
    RUN(attn_pool_table(e, e->x[l], l == 2 ? w->G2 : w->G3, B, e->st[l].H * e->st[l].W, c.att_thres, NUHTC_AP_AUTO, w->ap_inv, w->ap_S, w->ap_Ft, s));
  // join: the side stream carries the RPN branch (convs + heads from run_neck_heads, selection + NMS above)
  if (e->cfg.schedule != NUHTC_SCHED_THROUGHPUT && hipStreamWaitEvent(s, fixed ? e->ev_rpn : e->ev_side, 0) != hipSuccess) FAIL(e, NUHTC_E_HIP, "hipStreamWaitEvent failed");
  RUN(launch_build_rois(use_cc ? w->cc_boxes : nullptr, w->cc_counts, std::max(c.max_cc_proposals, 1), w->rpn_dets, w->rpn_counts, c.rpn_max_per_img,
                        rois_fixed, n_rois, w->rois, w->roi_off, w->roi_cnt, w->roi_total, B, s));
  const int Rcap = fixed ? B * n_rois : B * e->roi_cap;

  RoiFeatParams fp;
  fp.rois = w->rois; fp.r_dev = w->roi_total; fp.x0 = e->x[0]; fp.x1 = e->x[1]; fp.G2 = w->G2; fp.G3 = w->G3; fp.sem = e->sem_feat; fp.x0sem = e->x0sem;
  fp.H0 = e->st[0].H; fp.W0 = e->st[0].W; fp.H1 = e->st[1].H; fp.W1 = e->st[1].W; fp.H2 = e->st[2].H; fp.W2 = e->st[2].W; fp.H3 = e->st[3].H; fp.W3 = e->st[3].W;
  fp.out = w->feats; fp.fb_count = w->fb_count; fp.fb_list = w->fb_list; fp.list_cap = w->total_cap; fp.mid_list = w->mid_list; fp.fb_flag = w->fb_flag;
  roi_feat_modes(fp, w->big_part);
  // ---- 3-stage cascade (htc_roi_head_cus.py:2255-2280)
  for (int k = 0; k < 3; ++k) {
    auto it = e->bufs.find("rois_stage" + std::to_string(k));
    if (it != e->bufs.end() && e->debug_tokens)
      if (hipMemcpyAsync(it->second.ptr, w->rois, (size_t)Rcap * 5 * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) FAIL(e, NUHTC_E_HIP, "memcpy failed");
    RUN(launch_roi_feat(fp, 7, Rcap, s, e->cfg.schedule == NUHTC_SCHED_THROUGHPUT ? nullptr : e->side, e->ev_fpn, e->ev_side, e->side2, e->ev_side2));   // (both events are free again after the RPN join)
    {
      GemmParams p = gp(w->feats, e->fc1_w[k], e->fc1_b[k], w->h1, Rcap, 256, 3136);
      p.act = ACT_RELU; p.m_dev = w->roi_total;
      RUN(egemm(e, p, s));
    }
    {
      GemmParams p = gp(w->h1, e->fc2_w[k], e->fc2_b[k], w->h2, Rcap, 256, 256);
      p.act = ACT_RELU; p.m_dev = w->roi_total;
      RUN(egemm(e, p, s));
    }
    BboxTailParams tp;
    tp.h = w->h2; tp.w = e->head_w[k]; tp.b = e->head_b[k]; tp.nc = c.num_classes; tp.r_dev = w->roi_total; tp.cls = w->cls[k]; tp.reg = w->reg[k];
    tp.refine = k < 2; tp.rois = w->rois;
    for (int j = 0; j < 4; ++j) tp.stds[j] = c.stage_stds[k][j];
    tp.img_w = (float)e->Wv; tp.img_h = (float)e->Hv;
    RUN(launch_bbox_tail(tp, Rcap, s));
  }
  // ---- ensemble + Seesaw activation + multiclass NMS (htc_roi_head_cus.py:2283-2303)
  DetCandParams dp;
  dp.rois = w->rois; dp.cls0 = w->cls[0]; dp.cls1 = w->cls[1]; dp.cls2 = w->cls[2]; dp.reg2 = w->reg[2]; dp.roi_off = w->roi_off; dp.roi_cnt = w->roi_cnt;
  dp.nc = c.num_classes;
  for (int j = 0; j < 4; ++j) dp.stds[j] = c.stage_stds[2][j];
  dp.img_w = (float)e->Wv; dp.img_h = (float)e->Hv; dp.scale = c.scale_factor; dp.score_thr = fixed ? -1.0f : c.score_thr;
  dp.cand_boxes = w->dc_boxes; dp.cand_scores = w->dc_scores; dp.cand_ids = w->dc_ids; dp.cand_count = w->dc_count; dp.cap = w->det_cap;
  RUN(launch_det_candidates(dp, B, s));
  {
    NmsParams np;
    memset(&np, 0, sizeof(np));
    np.boxes = w->dc_boxes; np.scores = w->dc_scores; np.ids = w->dc_ids; np.group_count = w->dc_count; np.n_groups = 1; np.slot = w->det_cap;
    np.cap = w->det_cap; np.cap_pow2 = w->det_pow2; np.iou_thr = fixed ? 2.0f : c.nms_iou; np.max_keep = c.max_per_img;
    np.sorted_boxes = w->nms_sboxes; np.sorted_src = w->nms_src; np.n_total = w->nms_ntotal; np.mask = w->nms_mask;
    np.out_dets = out->boxes; np.out_src = w->det_src; np.out_counts = out->counts;
    // fixed-load mode: IoU threshold 2.0 suppresses nothing, so the first n_dets rows are the top-n_dets (roi,class)
    // pairs by score; det_finish clamps the per-tile count to n_dets (row stride stays max_per_img)
    RUN(launch_nms(np, B, s));
  }
  DetFinishParams df;
  df.B = B; df.max_keep = c.max_per_img; df.dets = out->boxes; df.keep_src = w->det_src; df.cand_ids = w->dc_ids; df.det_counts = out->counts;
  df.labels = out->labels; df.mask_rois = w->mask_rois; df.det_off = w->det_off; df.det_total = w->det_total; df.scale = c.scale_factor;
  df.limit = fixed ? n_dets : c.max_per_img;
  RUN(launch_det_finish(df, s));
  if (!out->masks) return 0;

  // ---- mask branch (htc_roi_head_cus.py:2310-2367)
  const int Dcap = B * c.max_per_img;
  RoiFeatParams mp = fp;
  mp.rois = w->mask_rois; mp.r_dev = w->det_total; mp.out = w->mfeat;
  RUN(launch_roi_feat(mp, 14, Dcap, s));
  float* a = w->mfeat;
  float* b = w->mtmpA;
  for (int j = 0; j < 4; ++j) {
    GemmParams p = gp(a, e->mk_w[j], e->mk_b[j], b, Dcap * 196, 64, 576);
    p.amode = A_CONV3; p.cH = 14; p.cW = 14; p.cC = 64; p.act = ACT_RELU; p.m_dev = w->det_total; p.m_mul = 196;
    RUN(egemm(e, p, s));
    a = b;
    b = (b == w->mtmpA) ? w->mtmpB : w->mtmpA;
  }
  {
    GemmParams p = gp(a, e->mk_up_w, e->mk_up_b, w->mup, Dcap * 196, 256, 64);
    p.act = ACT_RELU; p.store = ST_DECONV2; p.cH = 14; p.cW = 14; p.ldc = 64; p.m_dev = w->det_total; p.m_mul = 196;
    RUN(egemm(e, p, s));
  }
  RUN(launch_conv1x1_n1_dev(w->mup, e->mk_lw, e->mk_lb, w->mprob, Dcap * 784, w->det_total, 784, 1, s));
  PasteParams pp;
  pp.prob = w->mprob; pp.mask_rois = w->mask_rois; pp.det_off = w->det_off; pp.det_counts = out->counts; pp.max_keep = c.max_per_img;
  pp.H = c.tile_h; pp.W = c.tile_w; pp.vH = e->vh; pp.vW = e->vw; pp.scale = c.scale_factor; pp.thr = c.mask_thr_binary; pp.masks = out->masks; pp.areas = out->areas;
  RUN(launch_paste(pp, B, s));
  if (out->keep && out->areas) {
    TilePostParams tp;
    tp.dets = out->boxes; tp.labels = out->labels; tp.areas = out->areas; tp.det_counts = out->counts; tp.masks = out->masks; tp.keep = out->keep;
    tp.max_keep = c.max_per_img; tp.H = c.tile_h; tp.W = c.tile_w; tp.vH = e->vh; tp.vW = e->vw; tp.margin = c.margin; tp.min_area = c.min_area;
    tp.thr = mask_nms_thr(c.mask_nms_thr);
    RUN(launch_tile_post(tp, B, s));
  }
  return 0;
}

// =============================================================================== stand-alone ops
int nuhtc_op_roi_align(nuhtc_engine* e, const float* feat, int N, int H, int W, const float* rois, int R, int P, float scale, int sr, float* out,
                       void* stream) {
  if (!e || !feat || !rois || !out) return NUHTC_E_INVALID;
  HIP_CHECK(e, hipSetDevice(e->device));
  int rc = launch_roi_align(feat, N, H, W, 64, rois, R, nullptr, P, scale, sr, out, 0, (hipStream_t)stream);
  if (rc) FAIL(e, rc, "roi_align launch failed");
  return 0;
}

int nuhtc_op_nms(nuhtc_engine* e, const float* boxes, const float* scores, int n, float iou_thr, int32_t* keep_idx, int32_t* count_dev, void* stream) {
  if (!e || !boxes || !scores || !keep_idx || !count_dev) return NUHTC_E_INVALID;
  if (!e->finalized) FAIL(e, NUHTC_E_STATE, "nuhtc_op_nms before finalize");
  if (n < 0 || n > NMS_MAX_CAP) FAIL(e, NUHTC_E_INVALID, "nms op: n out of range");
  HIP_CHECK(e, hipSetDevice(e->device));
  hipStream_t s = (hipStream_t)stream;
  // scratch sized for this call (test entry point: allocation cost is irrelevant)
  const int cap = std::max(round_up(n, 64), 64);
  DevScratch sc;
  NmsParams np;
  memset(&np, 0, sizeof(np));
  np.boxes = boxes; np.scores = scores; np.ids = nullptr; np.group_count = sc.upload(&n, 1); np.n_groups = 1; np.slot = cap; np.cap = cap; np.cap_pow2 = pow2_ge(std::max(n, 2));
  np.iou_thr = iou_thr; np.max_keep = cap; np.sorted_boxes = sc.alloc<float>((size_t)cap * 16); np.sorted_src = sc.alloc<int>((size_t)cap * 4);
  np.n_total = sc.alloc<int>(4); np.mask = sc.alloc<unsigned long long>((size_t)cap * (cap / 64) * 8); np.out_dets = sc.alloc<float>((size_t)cap * 20);
  np.out_src = keep_idx; np.out_counts = count_dev;
  if (!sc.ok()) FAIL(e, NUHTC_E_HIP, "nms op: scratch allocation failed");
  const int rc = launch_nms(np, 1, s);
  return op_finish(e, rc, s, "nms launch failed", "nms kernel failed");
}

int nuhtc_op_cc_mask(nuhtc_engine* e, const float* sem_pred, int B, int h, int w, int H, int W, uint8_t* mask_out, void* stream) {
  if (!e || !sem_pred || !mask_out) return NUHTC_E_INVALID;
  if (B < 1 || h < 1 || w < 1 || H < 2 || W < 2 || (long long)H * W > (1ll << 26)) FAIL(e, NUHTC_E_INVALID, "cc_mask op: size out of range");
  HIP_CHECK(e, hipSetDevice(e->device));
  CcParams cp;
  memset(&cp, 0, sizeof(cp));
  cp.sem_pred = sem_pred; cp.h = h; cp.w = w; cp.img_h = H; cp.img_w = W; cp.mask_a = mask_out;
  int rc = launch_cc_mask(cp, B, (hipStream_t)stream);
  if (rc) FAIL(e, rc, "cc_mask launch failed");
  return 0;
}

int nuhtc_op_cc_proposals(nuhtc_engine* e, const uint8_t* mask, int B, int H, int W, int open, int min_area, int cap, uint8_t* opened_out,
                          uint8_t* filled_out, int32_t* labels_out, int32_t* stats_out, float* boxes_out, int32_t* counts_out,
                          int32_t* overflow_out, void* stream) {
  if (!e || !mask || !opened_out || !filled_out || !labels_out || !stats_out || !boxes_out || !counts_out || !overflow_out) return NUHTC_E_INVALID;
  if (B < 1 || H < 1 || W < 1 || (long long)H * W > (1ll << 26) || cap < 1 || cap > CC_LIST_CAP)
    FAIL(e, NUHTC_E_INVALID, "cc_proposals op: size out of range");
  HIP_CHECK(e, hipSetDevice(e->device));
  hipStream_t s = (hipStream_t)stream;
  const size_t total = (size_t)B * H * W;
  // scratch sized for this call (test entry point: allocation cost is irrelevant)
  DevScratch sc;
  CcParams cp;
  memset(&cp, 0, sizeof(cp));
  cp.img_h = H; cp.img_w = W; cp.min_area = min_area; cp.cap = cap;
  cp.mask_a = opened_out; cp.mask_b = filled_out; cp.touch = sc.alloc<unsigned char>(total); cp.labels = labels_out; cp.stats = stats_out;
  cp.list = sc.alloc<int>((size_t)B * CC_LIST_CAP * sizeof(int)); cp.nlist = sc.alloc<int>((size_t)B * sizeof(int));
  cp.boxes = boxes_out; cp.counts = counts_out; cp.overflow = overflow_out;
  if (!sc.ok()) FAIL(e, NUHTC_E_HIP, "cc_proposals op: scratch allocation failed");
  int rc = 0;
  if (hipMemcpyAsync(opened_out, mask, total, hipMemcpyDeviceToDevice, s) != hipSuccess || hipMemsetAsync(overflow_out, 0, sizeof(int32_t), s) != hipSuccess)
    rc = NUHTC_E_HIP;
  if (!rc) rc = launch_cc_from_mask(cp, B, open != 0, s);
  return op_finish(e, rc, s, "cc_proposals launch failed", "cc_proposals kernel failed");
}

// ---- the detection tail, op by op: each fills the parameter block run_roi_path fills and calls the same launch_* function
// small device int arrays the ops check on the host before a kernel indexes with them (after the stream's earlier work)
static bool read_ints(const int32_t* dev, int n, std::vector<int>& out, hipStream_t s) {
  out.resize(n);
  return hipStreamSynchronize(s) == hipSuccess && hipMemcpy(out.data(), dev, (size_t)n * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess;
}

int nuhtc_op_bbox_tail(nuhtc_engine* e, const nuhtc_bbox_tail_args* a, void* stream) {
  if (!e || !a || !a->h || !a->cls_w || !a->cls_b || !a->reg_w || !a->reg_b || !a->r_dev || !a->rois || !a->cls || !a->reg) return NUHTC_E_INVALID;
  if (a->nc < 1 || a->nc + 6 > 64 || a->nc + 2 > 16) FAIL(e, NUHTC_E_INVALID, "bbox_tail op: nc out of range (nc + 2 <= 16 columns of cls)");
  if (a->cap < 1) FAIL(e, NUHTC_E_INVALID, "bbox_tail op: cap out of range");
  HIP_CHECK(e, hipSetDevice(e->device));
  hipStream_t s = (hipStream_t)stream;
  std::vector<int> r;
  if (!read_ints(a->r_dev, 1, r, s)) FAIL(e, NUHTC_E_HIP, "bbox_tail op: reading r_dev failed");
  if (r[0] < 0 || r[0] > a->cap) FAIL(e, NUHTC_E_INVALID, "bbox_tail op: *r_dev exceeds cap");
  std::vector<float> hw, hb;
  pack_bbox_head(a->cls_w, a->cls_b, a->reg_w, a->reg_b, a->nc, hw, hb);
  DevScratch sc;
  BboxTailParams tp;
  tp.h = a->h; tp.w = sc.upload(hw); tp.b = sc.upload(hb); tp.nc = a->nc; tp.r_dev = a->r_dev; tp.cls = a->cls; tp.reg = a->reg;
  tp.refine = a->refine != 0; tp.rois = a->rois;
  for (int j = 0; j < 4; ++j) tp.stds[j] = a->stds[j];
  tp.img_w = a->img_w; tp.img_h = a->img_h;
  if (!sc.ok()) FAIL(e, NUHTC_E_HIP, "bbox_tail op: scratch allocation failed");
  const int rc = launch_bbox_tail(tp, a->cap, s);
  return op_finish(e, rc, s, "bbox_tail launch failed", "bbox_tail kernel failed");
}

int nuhtc_op_det_post(nuhtc_engine* e, const nuhtc_det_post_args* a, void* stream) {
  if (!e || !a || !a->rois || !a->cls0 || !a->cls1 || !a->cls2 || !a->reg2 || !a->roi_off || !a->roi_cnt || !a->dets || !a->labels || !a->counts ||
      !a->mask_rois || !a->det_off || !a->det_total || !a->cand_count || !a->cand_scores || !a->cand_ids || !a->cand_boxes)
    return NUHTC_E_INVALID;
  if (!e->finalized) FAIL(e, NUHTC_E_STATE, "nuhtc_op_det_post before finalize");
  if (a->nc < 1 || a->nc + 2 > 16) FAIL(e, NUHTC_E_INVALID, "det_post op: nc out of range (nc + 2 <= 16)");
  if (a->B < 1 || a->B > 256) FAIL(e, NUHTC_E_INVALID, "det_post op: B out of range (1..256)");
  if (a->cap < 64 || a->cap % 64 || a->cap > NMS_MAX_CAP) FAIL(e, NUHTC_E_INVALID, "det_post op: cap must be a multiple of 64 up to NMS_MAX_CAP");
  if (a->max_per_img < 1 || a->max_per_img > 2048 || a->limit < 0 || a->total < 0) FAIL(e, NUHTC_E_INVALID, "det_post op: max_per_img / limit / total out of range");
  HIP_CHECK(e, hipSetDevice(e->device));
  hipStream_t s = (hipStream_t)stream;
  const int B = a->B;
  std::vector<int> off, cnt;
  if (!read_ints(a->roi_off, B, off, s) || !read_ints(a->roi_cnt, B, cnt, s)) FAIL(e, NUHTC_E_HIP, "det_post op: reading roi_off / roi_cnt failed");
  for (int b = 0; b < B; ++b)
    if (off[b] < 0 || cnt[b] < 0 || (long long)off[b] + cnt[b] > a->total) FAIL(e, NUHTC_E_INVALID, "det_post op: roi_off + roi_cnt exceeds total");
  DevScratch sc;
  DetCandParams dp;
  dp.rois = a->rois; dp.cls0 = a->cls0; dp.cls1 = a->cls1; dp.cls2 = a->cls2; dp.reg2 = a->reg2; dp.roi_off = a->roi_off; dp.roi_cnt = a->roi_cnt;
  dp.nc = a->nc;
  for (int j = 0; j < 4; ++j) dp.stds[j] = a->stds[j];
  dp.img_w = a->img_w; dp.img_h = a->img_h; dp.scale = a->scale; dp.score_thr = a->score_thr;
  dp.cand_boxes = a->cand_boxes; dp.cand_scores = a->cand_scores; dp.cand_ids = a->cand_ids; dp.cand_count = a->cand_count; dp.cap = a->cap;
  NmsParams np;
  memset(&np, 0, sizeof(np));
  np.boxes = a->cand_boxes; np.scores = a->cand_scores; np.ids = a->cand_ids; np.group_count = a->cand_count; np.n_groups = 1; np.slot = a->cap;
  np.cap = a->cap; np.cap_pow2 = pow2_ge(a->cap); np.iou_thr = a->nms_iou; np.max_keep = a->max_per_img;
  np.sorted_boxes = sc.alloc<float>((size_t)B * a->cap * 16); np.sorted_src = sc.alloc<int>((size_t)B * a->cap * 4); np.n_total = sc.alloc<int>((size_t)B * 4);
  np.mask = sc.alloc<unsigned long long>((size_t)B * a->cap * (a->cap / 64) * 8);
  np.out_dets = a->dets; np.out_src = sc.alloc<int>((size_t)B * a->max_per_img * 4); np.out_counts = a->counts;
  DetFinishParams df;
  df.B = B; df.max_keep = a->max_per_img; df.dets = a->dets; df.keep_src = np.out_src; df.cand_ids = a->cand_ids; df.det_counts = a->counts;
  df.labels = a->labels; df.mask_rois = a->mask_rois; df.det_off = a->det_off; df.det_total = a->det_total; df.scale = a->scale;
  df.limit = a->limit;
  if (!sc.ok()) FAIL(e, NUHTC_E_HIP, "det_post op: scratch allocation failed");
  int rc = launch_det_candidates(dp, B, s);
  if (!rc) rc = launch_nms(np, B, s);
  if (!rc) rc = launch_det_finish(df, s);
  return op_finish(e, rc, s, "det_post launch failed", "det_post kernel failed");
}

int nuhtc_op_paste(nuhtc_engine* e, const nuhtc_paste_args* a, void* stream) {
  if (!e || !a || !a->prob || !a->mask_rois || !a->det_off || !a->det_counts || !a->masks || !a->areas) return NUHTC_E_INVALID;
  if (a->B < 1 || a->B > 256) FAIL(e, NUHTC_E_INVALID, "paste op: B out of range (1..256)");
  if (a->max_keep < 1 || a->max_keep > 2048) FAIL(e, NUHTC_E_INVALID, "paste op: max_keep out of range (1..2048)");
  if (a->H < 1 || a->W < 32 || a->W % 32 || a->vH < 0 || a->vH > a->H || a->vW < 0 || a->vW > a->W || a->D < 0)
    FAIL(e, NUHTC_E_INVALID, "paste op: W must be a multiple of 32 and the valid canvas inside H x W");
  HIP_CHECK(e, hipSetDevice(e->device));
  hipStream_t s = (hipStream_t)stream;
  std::vector<int> off, cnt;
  if (!read_ints(a->det_off, a->B, off, s) || !read_ints(a->det_counts, a->B, cnt, s)) FAIL(e, NUHTC_E_HIP, "paste op: reading det_off / det_counts failed");
  for (int b = 0; b < a->B; ++b)
    if (off[b] < 0 || cnt[b] < 0 || cnt[b] > a->max_keep || (long long)off[b] + cnt[b] > a->D) FAIL(e, NUHTC_E_INVALID, "paste op: det_off / det_counts exceed D or max_keep");
  PasteParams pp;
  pp.prob = a->prob; pp.mask_rois = a->mask_rois; pp.det_off = a->det_off; pp.det_counts = a->det_counts; pp.max_keep = a->max_keep;
  pp.H = a->H; pp.W = a->W; pp.vH = a->vH; pp.vW = a->vW; pp.scale = a->scale; pp.thr = a->thr; pp.masks = a->masks; pp.areas = a->areas;
  const int rc = launch_paste(pp, a->B, s);
  return op_finish(e, rc, s, "paste launch failed", "paste kernel failed");
}

int nuhtc_op_tile_post(nuhtc_engine* e, const nuhtc_tile_post_args* a, void* stream) {
  if (!e || !a || !a->dets || !a->labels || !a->areas || !a->det_counts || !a->masks || !a->keep) return NUHTC_E_INVALID;
  if (a->B < 1 || a->B > 256) FAIL(e, NUHTC_E_INVALID, "tile_post op: B out of range (1..256)");
  if (a->max_keep < 1 || a->max_keep > 2048) FAIL(e, NUHTC_E_INVALID, "tile_post op: max_keep out of range (1..2048)");
  if (a->H < 1 || a->W < 32 || a->W % 32 || a->vH < 0 || a->vH > a->H || a->vW < 0 || a->vW > a->W)
    FAIL(e, NUHTC_E_INVALID, "tile_post op: W must be a multiple of 32 and the valid canvas inside H x W");
  HIP_CHECK(e, hipSetDevice(e->device));
  hipStream_t s = (hipStream_t)stream;
  std::vector<int> cnt;
  if (!read_ints(a->det_counts, a->B, cnt, s)) FAIL(e, NUHTC_E_HIP, "tile_post op: reading det_counts failed");
  for (int b = 0; b < a->B; ++b)
    if (cnt[b] < 0 || cnt[b] > a->max_keep) FAIL(e, NUHTC_E_INVALID, "tile_post op: det_counts exceed max_keep");
  TilePostParams tp;
  tp.dets = a->dets; tp.labels = a->labels; tp.areas = a->areas; tp.det_counts = a->det_counts; tp.masks = a->masks; tp.keep = a->keep;
  tp.max_keep = a->max_keep; tp.H = a->H; tp.W = a->W; tp.vH = a->vH; tp.vW = a->vW; tp.margin = a->margin; tp.min_area = a->min_area;
  tp.thr = mask_nms_thr(a->thr);
  const int rc = launch_tile_post(tp, a->B, s);
  return op_finish(e, rc, s, "tile_post launch failed", "tile_post kernel failed");
}

// ---- the RPN half of the proposals, op by op: the same parameter blocks and launch_* functions as run_roi_path
int nuhtc_op_rpn_select(nuhtc_engine* e, const float* const out[4], const int32_t h[4], const int32_t w[4], int B, int nms_pre, int img_h, int img_w,
                        float min_size, float* cand_boxes, float* cand_scores, int32_t* cand_count, void* stream) {
  if (!e || !out || !h || !w || !cand_boxes || !cand_scores || !cand_count) return NUHTC_E_INVALID;
  for (int l = 0; l < 4; ++l)
    if (!out[l]) return NUHTC_E_INVALID;
  if (!e->finalized) FAIL(e, NUHTC_E_STATE, "nuhtc_op_rpn_select before finalize");
  if (B < 1 || B > 256) FAIL(e, NUHTC_E_INVALID, "rpn_select op: B out of range (1..256)");
  if (nms_pre < 1 || nms_pre > 4096) FAIL(e, NUHTC_E_INVALID, "rpn_select op: nms_pre out of range (1..4096)");
  int maxn = 0;
  for (int l = 0; l < 4; ++l) {
    if (h[l] < 1 || w[l] < 1 || (long long)h[l] * w[l] * 3 > (1ll << 24)) FAIL(e, NUHTC_E_INVALID, "rpn_select op: level size out of range");
    maxn = std::max(maxn, h[l] * w[l] * 3);
  }
  HIP_CHECK(e, hipSetDevice(e->device));
  hipStream_t s = (hipStream_t)stream;
  RpnLevels lv;
  for (int l = 0; l < 4; ++l) { lv.out[l] = out[l]; lv.h[l] = h[l]; lv.w[l] = w[l]; lv.stride[l] = 4 << l; }
  DevScratch sc;
  RpnSelParams sp;
  sp.nms_pre = nms_pre; sp.slot = nms_pre; sp.cand_boxes = cand_boxes; sp.cand_scores = cand_scores; sp.cand_count = cand_count;
  sp.key_stride = round_up(maxn, 64);
  sp.keys = sc.alloc<unsigned>((size_t)B * 4 * sp.key_stride * sizeof(unsigned));
  sp.img_h = img_h; sp.img_w = img_w; sp.min_size = min_size;
  if (!sc.ok()) FAIL(e, NUHTC_E_HIP, "rpn_select op: scratch allocation failed");
  const int rc = launch_rpn_select(lv, sp, B, s);
  return op_finish(e, rc, s, "rpn_select launch refused or failed", "rpn_select kernel failed");
}

int nuhtc_op_nms_levels(nuhtc_engine* e, const float* boxes, const float* scores, const int32_t* group_count, int B, int G, int slot, float iou_thr,
                        int max_keep, int route, float* dets, int32_t* src, int32_t* counts, void* stream) {
  if (!e || !boxes || !scores || !group_count || !dets || !src || !counts) return NUHTC_E_INVALID;
  if (!e->finalized) FAIL(e, NUHTC_E_STATE, "nuhtc_op_nms_levels before finalize");
  if (B < 1 || B > 256) FAIL(e, NUHTC_E_INVALID, "nms_levels op: B out of range (1..256)");
  if (G < 1 || G > NMS_MAX_GROUPS || slot < 1 || slot > NMS_MAX_CAP || max_keep < 1 || (route != 0 && route != 1))
    FAIL(e, NUHTC_E_INVALID, "nms_levels op: G (1..16), slot (1..16384), max_keep (>= 1) or route (0, 1) out of range");
  HIP_CHECK(e, hipSetDevice(e->device));
  hipStream_t s = (hipStream_t)stream;
  std::vector<int> cnt;
  if (!read_ints(group_count, B * G, cnt, s)) FAIL(e, NUHTC_E_HIP, "nms_levels op: reading group_count failed");
  for (int c : cnt)
    if (c < 0 || c > slot) FAIL(e, NUHTC_E_INVALID, "nms_levels op: a group count exceeds slot");
  // capacities as alloc_roi_workspace derives rpn_cap / rpn_pow2 from G levels of `slot` candidates
  const int maxc = G * slot;
  const int cap = round_up(std::max(maxc, 64), 64) + 64 * (G - 1);
  const size_t nw = (size_t)cap / 64;
  if ((unsigned long long)B * cap * nw * 8 > (1ull << 32)) FAIL(e, NUHTC_E_INVALID, "nms_levels op: the mask matrix of this call would exceed 4 GiB");
  DevScratch sc;
  NmsParams np;
  memset(&np, 0, sizeof(np));
  np.boxes = boxes; np.scores = scores; np.ids = nullptr; np.group_count = group_count; np.n_groups = G; np.slot = slot;
  np.cap = cap; np.cap_pow2 = pow2_ge(maxc); np.iou_thr = iou_thr; np.max_keep = max_keep;
  np.out_dets = dets; np.out_src = src; np.out_counts = counts;
  // every scratch array starts as 0xFF bytes: nothing may lean on zeroed or left-over memory
  struct { void** p; size_t bytes; } parts[] = {
      {(void**)&np.sorted_boxes, (size_t)B * cap * 16}, {(void**)&np.sorted_src, (size_t)B * cap * 4}, {(void**)&np.n_total, (size_t)B * 4},
      {(void**)&np.seg_start, (size_t)B * G * 4},       {(void**)&np.seg_n, (size_t)B * G * 4},        {(void**)&np.sorted_pos, (size_t)B * cap * 4},
      {(void**)&np.keepbits, (size_t)B * nw * 8},       {(void**)&np.mask, (size_t)B * cap * nw * 8}};
  int rc = 0;
  for (auto& part : parts) {
    *part.p = sc.alloc<void>(part.bytes);
    if (!sc.ok()) FAIL(e, NUHTC_E_HIP, "nms_levels op: scratch allocation failed");
    if (hipMemsetAsync(*part.p, 0xFF, part.bytes, s) != hipSuccess) rc = NUHTC_E_HIP;
  }
  if (!rc) rc = route == 0 ? launch_nms_levels(np, B, s) : launch_nms(np, B, s);
  return op_finish(e, rc, s, "nms_levels launch refused or failed (route 0: G * max_keep <= 8192; sorted-list capacity within the route's limit)",
                   "nms_levels kernel failed");
}

int nuhtc_op_build_rois(nuhtc_engine* e, const float* cc_boxes, const int32_t* cc_counts, int cc_cap, const float* rpn_dets, const int32_t* rpn_counts,
                        int rpn_cap, const float* fixed, int n_fixed, int B, int cap, float* rois, int32_t* roi_off, int32_t* roi_cnt, int32_t* total,
                        void* stream) {
  if (!e || !rois || !roi_off || !roi_cnt || !total) return NUHTC_E_INVALID;
  if (!fixed && (!rpn_dets || !rpn_counts || (cc_boxes && !cc_counts))) return NUHTC_E_INVALID;
  if (B < 1 || B > 256) FAIL(e, NUHTC_E_INVALID, "build_rois op: B out of range (1..256)");
  if (cap < 0 || cc_cap < 0 || rpn_cap < 0 || n_fixed < 0) FAIL(e, NUHTC_E_INVALID, "build_rois op: negative capacity");
  HIP_CHECK(e, hipSetDevice(e->device));
  hipStream_t s = (hipStream_t)stream;
  long long rows = (long long)B * n_fixed;
  if (!fixed) {
    std::vector<int> nr, ncc(B, 0);
    if (!read_ints(rpn_counts, B, nr, s) || (cc_boxes && !read_ints(cc_counts, B, ncc, s))) FAIL(e, NUHTC_E_HIP, "build_rois op: reading the counts failed");
    rows = 0;
    for (int b = 0; b < B; ++b) {
      if (nr[b] < 0 || nr[b] > rpn_cap || ncc[b] < 0 || ncc[b] > cc_cap) FAIL(e, NUHTC_E_INVALID, "build_rois op: a count exceeds its capacity");
      rows += nr[b] + ncc[b];
    }
  }
  if (rows > cap) FAIL(e, NUHTC_E_INVALID, "build_rois op: more rows than cap");
  const int rc = launch_build_rois(cc_boxes, cc_counts, cc_cap, rpn_dets, rpn_counts, rpn_cap, fixed, n_fixed, rois, roi_off, roi_cnt, total, B, s);
  return op_finish(e, rc, s, "build_rois launch failed", "build_rois kernel failed");
}

// ---- the RoI feature block, op by op: the attention-pool tables and the fused RoI features of run_roi_path on the caller's maps and boxes
int nuhtc_op_attn_pool(nuhtc_engine* e, const float* F, int B, int HW, float tau, int route, float* G, void* stream) {
  if (!e || !F || !G) return NUHTC_E_INVALID;
  if (!e->finalized) FAIL(e, NUHTC_E_STATE, "nuhtc_op_attn_pool before finalize");
  if (B < 1 || B > 256) FAIL(e, NUHTC_E_INVALID, "attn_pool op: B out of range (1..256)");
  if (HW < 1 || HW > 16384 || (long long)B * HW * HW > (1ll << 28)) FAIL(e, NUHTC_E_INVALID, "attn_pool op: HW out of range (1..16384, B * HW * HW <= 2^28)");
  if (route < NUHTC_AP_AUTO || route > NUHTC_AP_FP16) FAIL(e, NUHTC_E_INVALID, "attn_pool op: unknown route");
  if (route == NUHTC_AP_GEMM && HW % 32 != 0) FAIL(e, NUHTC_E_INVALID, "attn_pool op: the GEMM route needs HW % 32 == 0");
  HIP_CHECK(e, hipSetDevice(e->device));
  hipStream_t s = (hipStream_t)stream;
  route = attn_pool_route(e, HW, route);
  DevScratch sc;
  float *inv = nullptr, *S = nullptr, *Ft = nullptr;      // scratch of the GEMM route alone
  if (route == NUHTC_AP_GEMM) {
    inv = sc.alloc<float>((size_t)B * HW * sizeof(float));
    S = sc.alloc<float>((size_t)B * HW * HW * sizeof(float));
    Ft = sc.alloc<float>((size_t)B * HW * 64 * sizeof(float));
  }
  if (!sc.ok()) FAIL(e, NUHTC_E_HIP, "attn_pool op: scratch allocation failed");
  const int rc = attn_pool_table(e, F, G, B, HW, tau, route, inv, S, Ft, s);
  const hipError_t he = hipStreamSynchronize(s);
  if (rc) return rc;                                      // (attn_pool_table named the launch that failed)
  if (he != hipSuccess) FAIL(e, NUHTC_E_HIP, "attn_pool kernel failed");
  return 0;
}

int nuhtc_op_roi_feats(nuhtc_engine* e, const nuhtc_roi_feats_args* a, void* stream) {
  if (!e || !a || !a->x0 || !a->x1 || !a->sem || !a->x0sem || !a->G2 || !a->G3 || !a->rois || !a->r_dev || !a->out) return NUHTC_E_INVALID;
  if (a->P == 7 && (!a->fb_flag || !a->counts)) return NUHTC_E_INVALID;
  if (!e->finalized) FAIL(e, NUHTC_E_STATE, "nuhtc_op_roi_feats before finalize");
  if (a->P != 7 && a->P != 14) FAIL(e, NUHTC_E_INVALID, "roi_feats op: P must be 7 or 14");
  if (a->B < 1 || a->B > 256) FAIL(e, NUHTC_E_INVALID, "roi_feats op: B out of range (1..256)");
  if (a->cap < 1 || a->cap > (1 << 20)) FAIL(e, NUHTC_E_INVALID, "roi_feats op: cap out of range (1..2^20)");
  for (int l = 0; l < 4; ++l)
    if (a->H[l] < 1 || a->W[l] < 1 || a->H[l] > 4096 || a->W[l] > 4096) FAIL(e, NUHTC_E_INVALID, "roi_feats op: level size out of range (1..4096)");
  HIP_CHECK(e, hipSetDevice(e->device));
  hipStream_t s = (hipStream_t)stream;
  std::vector<int> r;
  if (!read_ints(a->r_dev, 1, r, s)) FAIL(e, NUHTC_E_HIP, "roi_feats op: reading r_dev failed");
  if (r[0] < 0 || r[0] > a->cap) FAIL(e, NUHTC_E_INVALID, "roi_feats op: *r_dev exceeds cap");
  {   // column 0 of a live row is the image the kernels index the maps with; the coordinates go through float -> int conversions
    std::vector<float> rows((size_t)r[0] * 5);
    if (r[0] && hipMemcpy(rows.data(), a->rois, rows.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) FAIL(e, NUHTC_E_HIP, "roi_feats op: reading rois failed");
    for (int i = 0; i < r[0]; ++i) {
      const float* q = &rows[(size_t)i * 5];
      if (!(q[0] >= 0.f && q[0] < (float)a->B) || q[0] != floorf(q[0])) FAIL(e, NUHTC_E_INVALID, "roi_feats op: a RoI's image index is outside 0..B-1");
      for (int j = 1; j < 5; ++j)
        if (!(fabsf(q[j]) <= 1.0e6f)) FAIL(e, NUHTC_E_INVALID, "roi_feats op: a RoI coordinate is not finite (|v| <= 1e6)");
    }
  }
  DevScratch sc;
  RoiFeatParams fp;
  fp.rois = a->rois; fp.r_dev = a->r_dev; fp.x0 = a->x0; fp.x1 = a->x1; fp.G2 = a->G2; fp.G3 = a->G3; fp.sem = a->sem; fp.x0sem = a->x0sem;
  fp.H0 = a->H[0]; fp.W0 = a->W[0]; fp.H1 = a->H[1]; fp.W1 = a->W[1]; fp.H2 = a->H[2]; fp.W2 = a->W[2]; fp.H3 = a->H[3]; fp.W3 = a->W[3];
  fp.out = a->out; fp.fb_count = sc.alloc<int>(8 * sizeof(int)); fp.fb_list = sc.alloc<int>((size_t)a->cap * sizeof(int)); fp.list_cap = a->cap;
  fp.mid_list = sc.alloc<int>((size_t)a->cap * sizeof(int)); fp.fb_flag = a->fb_flag;
  roi_feat_modes(fp, sc.alloc<float>((size_t)BIG_SPLIT_MAX * 3 * 49 * 64 * sizeof(float)));
  if (!sc.ok()) FAIL(e, NUHTC_E_HIP, "roi_feats op: scratch allocation failed");
  int rc;
  if (a->P == 7) {
    rc = launch_roi_feat(fp, 7, a->cap, s, e->cfg.schedule == NUHTC_SCHED_THROUGHPUT ? nullptr : e->side, e->ev_fpn, e->ev_side, e->side2, e->ev_side2);
    if (!rc && hipMemcpyAsync(a->counts, fp.fb_count, 3 * sizeof(int), hipMemcpyDeviceToDevice, s) != hipSuccess) rc = NUHTC_E_HIP;
  } else rc = launch_roi_feat(fp, 14, a->cap, s);
  return op_finish(e, rc, s, "roi_feats launch failed", "roi_feats kernel failed");
}
