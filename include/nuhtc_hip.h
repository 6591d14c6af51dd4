/* nuhtc_hip.h — C ABI of libnuhtc_hip.so, the MI355X (gfx950) engine for NuHTC's htc_lite_swin
 * tile-inference path.
 *
 * What it replaces in the reference (paths relative to the boyden/NuHTC tree, `mmdet/` =
 * thirdparty/mmdetection/mmdet/): the reference has no native code of its own; its native seam is
 * mmcv's pybind extension (`mmcv._ext`: roi_align_forward, nms; call sites
 * mmdet/models/roi_heads/roi_extractors/base_roi_extractor.py:53-58, mmdet/models/dense_heads/rpn_head.py:232,
 * nuhtc/models/bbox_head.py:93) plus torch ATen.  This library replaces the whole device side of
 * `inference_detector(model, imgs)` (mmdet/apis/inference.py:90-153 ->
 * nuhtc/models/htc_cus.py:110-121 `simple_test`), i.e. everything between "uint8 tiles" and
 * "(bbox_results, segm_results)", and additionally the per-tile filter + mask-NMS of
 * tools/infer_wsi.py:510-531,60-84.
 *
 * Conventions
 *   - every function returns 0 on success or a negative NUHTC_E_* code; nothing throws across the ABI;
 *     nuhtc_last_error() gives the message of the last failure on that engine (or of a failed create).
 *   - plain pointers and sizes only.  `dev` pointers are HIP device pointers owned by the caller
 *     (e.g. torch tensors); `host` pointers are host memory.  The engine owns weights + workspace.
 *   - all work is enqueued on the `stream` passed in (a hipStream_t cast to void*, NULL = default
 *     stream); functions that return counts to the host synchronise that stream, others do not.
 *   - one engine per (device, stream user); an engine is not thread-safe; engines are independent.
 */
#ifndef NUHTC_HIP_H
#define NUHTC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NUHTC_ABI_VERSION 12

enum {
  NUHTC_OK = 0,
  NUHTC_E_INVALID = -1,   /* bad argument / unsupported configuration */
  NUHTC_E_HIP = -2,       /* a HIP runtime call failed */
  NUHTC_E_STATE = -3,     /* call order violated (e.g. infer before finalize, missing weight) */
  NUHTC_E_CAPACITY = -4,  /* a per-tile capacity (proposals) overflowed; results would be truncated */
  NUHTC_E_NOTFOUND = -5   /* unknown weight / buffer name */
};

/* channel handling of the two reference entry points:
 *   0: tools/infer.py      (file -> BGR -> to_rgb): tile channels are used as given (RGB vs RGB means)
 *   1: tools/infer_wsi.py  (RGB ndarray run through the BGR pipeline): channels are reversed first     */
enum { NUHTC_CH_AS_IS = 0, NUHTC_CH_SWAP = 1 };

/* How the fp32 matrix products of the path (Swin linears, convolutions, FCs and -- since ABI v6 -- the two products of window attention)
 * are executed.  Both are fp32 arithmetic: fp32
 * operands and results, exact products, fp32 accumulation.
 *   NUHTC_PIPE_BF16_SPLIT (default): every fp32 operand is split exactly into three bf16 numbers (8 + 8 + 8 significand bits)
 *       and the product runs as six v_mfma_f32_32x32x16_bf16 per 16-deep step.  The six products are exact; the three cross terms
 *       a2*b3, a3*b2 (each <= 2^-24 |a*b|: round-to-nearest splits give |a2| <= 2^-8 |a|, |a3| <= 2^-16 |a|) and a3*b3 (<= 2^-32)
 *       are dropped, i.e. at worst 2^-23 |a*b| per product, one fp32 rounding unit -- not bit-identical to an fp32 fma chain.
 *       Measured error against fp64 is at or below that of the fp32 MFMA chain (csrc/gemm.hip, DESIGN.md 4,
 *       tests/test_hip_dense.py), and parity with the reference is instance-exact with every disagreement explained by a
 *       threshold (tests/parity_util.py), not bitwise.
 *   NUHTC_PIPE_FP32: v_mfma_f32_32x32x2_f32, bitwise an fp32 fma chain (1/16 of the bf16 MFMA rate on gfx950). */
enum { NUHTC_PIPE_BF16_SPLIT = 0, NUHTC_PIPE_FP32 = 1 };

/* What an engine's launch schedule is tuned for (same arithmetic, same results bit for bit):
 *   NUHTC_SCHED_LATENCY (default): one batch at a time as fast as possible -- 128-row block tiles for the Swin linears (the launch
 *       fills the chip soonest), the RPN branch and the big / mid-size RoI classes on the engine's two side streams beside the
 *       caller's stream.
 *   NUHTC_SCHED_THROUGHPUT: for engines that run beside others (nuhtc_amd.pipeline.EnginePipeline sets it) -- 256-row block
 *       tiles (fewer LDS bytes and operand splits per MFMA; another batch's kernels fill the under-filled tail of a launch) and
 *       every kernel of the batch on the caller's stream (the other batches are the concurrency; forks and joins inside a batch
 *       only add cross-stream waits and kernels that compete with their own batch).  Measured with four batches in flight:
 *       +1.5 % for the tiles, +4 % for the single stream; a batch alone is 3-5 % slower this way. */
enum { NUHTC_SCHED_LATENCY = 0, NUHTC_SCHED_THROUGHPUT = 1 };

typedef struct nuhtc_engine nuhtc_engine;

/* Mirrors the `model` / `test_cfg` / `test_pipeline` keys of
 * configs/nuhtc/htc_lite_swin_pytorch_fpn_{PanNuke,CoNSeP,...}_seasaw_CAS.py that the path reads. */
typedef struct nuhtc_config {
  int32_t abi_version;       /* = NUHTC_ABI_VERSION */
  int32_t num_classes;       /* 5 (PanNuke) / 4 (CoNSeP) ... ; 1..14              config:5   */
  int32_t tile_h, tile_w;    /* size of the uint8 input buffers and of the output masks in pixels (256); tile_w % 32 == 0 */
  int32_t valid_h, valid_w;  /* the image inside the buffer (top-left corner); 0 = the whole tile.  Like the reference's test
                              * pipeline the image is resized (img_shape = scale * valid), normalised and zero-padded to the next
                              * multiple of 32 (pad_shape, Pad(size_divisor=32), transforms.py:570-); boxes are clipped to img_shape,
                              * the component proposals are computed at img_shape, masks are pasted into valid_h x valid_w
                              * (ori_shape) and are zero outside it.  scale * valid must be integers. */
  int32_t max_batch;         /* workspace is sized for this many tiles per nuhtc_infer call  */
  float   scale_factor;      /* 2.0 : MultiScaleFlipAug(scale_factor) = 80/mag (tools/infer_wsi.py:416-419); 1..8 */
  float   mean[3], std[3];   /* img_norm_cfg                                     config:8   */
  /* test_cfg.rpn                                                                config:256-261 */
  int32_t rpn_nms_pre;       /* 3000 */
  int32_t rpn_max_per_img;   /* 1000 */
  float   rpn_nms_iou;       /* 0.7  */
  float   rpn_min_bbox_size; /* 10   */
  /* test_cfg.rcnn                                                               config:262-266 */
  float   score_thr;         /* 0.35 */
  float   nms_iou;           /* 0.5  */
  int32_t max_per_img;       /* 500  */
  float   mask_thr_binary;   /* 0.5  */
  /* roi_head                                                                    config:72-160 */
  float   att_thres;         /* 0.965926 : AttentionRoIExtractor thres */
  int32_t watershed_proposal;/* 1 : prepend connected-component proposals (htc_roi_head_cus.py:2217-2221) */
  int32_t max_cc_proposals;  /* capacity for those per tile (the reference has no cap; overflow -> NUHTC_E_CAPACITY) */
  float   stage_stds[3][4];  /* bbox_coder.target_stds of the 3 cascade stages  config:97,115,133 */
  /* tools/infer_wsi.py post-processing (args.margin, args.min_area, mask_nms thr)  infer_wsi.py:510-526 */
  int32_t margin;            /* 2    */
  int32_t min_area;          /* 10   */
  float   mask_nms_thr;      /* 0.05 */
  int32_t matrix_pipe;       /* NUHTC_PIPE_BF16_SPLIT (default) or NUHTC_PIPE_FP32 */
  int32_t schedule;          /* NUHTC_SCHED_LATENCY (default) or NUHTC_SCHED_THROUGHPUT (v5) */
  int32_t att_pool_fp16;     /* 0 (default): the attention-pool branch of AttentionRoIExtractor in fp32, as the reference computes it on a CPU
                              * device (the north star's "fp32 tolerance").  1 (v10): as the reference computes it when its
                              * feature maps are on a CUDA device -- it casts that branch to fp16 there (nuhtc/models/roi_extractors_cus.py:203,231):
                              * every tensor operation of :231-237 rounds to fp16 (reductions accumulate in fp32), the fp16 result is added
                              * into the fp32 RoI features.  Only the level-2 / level-3 tables change; see INTEGRATION.md section 6. */
  int32_t features_only;     /* 0 (default): the detection engine.  1 (v11): an engine for nuhtc_features only -- nuhtc_finalize requires and
                              * packs the backbone.* / neck.* tensors alone (nuhtc_load_weight accepts the checkpoint's other tensors of the
                              * schema and drops them), no workspace is allocated for the heads or the RoI path (max_batch can then be large),
                              * nuhtc_infer / nuhtc_infer_fixed_load return NUHTC_E_STATE. */
} nuhtc_config;

/* Fills `cfg` with the PanNuke defaults listed above. */
void nuhtc_default_config(nuhtc_config* cfg);

/* Creates an engine on HIP device `device`.  Replaces `build_detector(cfg.model)` +
 * `.to(device)` of nuhtc/apis/inference.py:11-57. */
int nuhtc_create(const nuhtc_config* cfg, int device, nuhtc_engine** out);
void nuhtc_destroy(nuhtc_engine* e);
const char* nuhtc_last_error(const nuhtc_engine* e);

/* Uploads one tensor of the mmdet state_dict (SURVEY Appendix B naming, fp32, host memory, C order).
 * Replaces `load_checkpoint(model, ckpt)` (nuhtc/apis/inference.py:44).  Names outside the path's schema are rejected with
 * NUHTC_E_NOTFOUND (buffers such as relative_position_index, loss_cls.cum_samples, roi_head.kernel, EMA / optimizer entries
 * are the caller's to drop), a wrong shape or ndim > 4 with NUHTC_E_INVALID; nuhtc_last_error() names the tensor. */
int nuhtc_load_weight(nuhtc_engine* e, const char* name, const float* host_data, const int64_t* shape, int ndim);

/* Checks that every tensor of the path was loaded and pre-packs weights (NHWC / k-major layouts,
 * NormedLinear row normalisation, relative-position bias (nH,49,49), shift masks, window maps). */
int nuhtc_finalize(nuhtc_engine* e);

/* Per-tile results in device memory, capacity `max_per_img` rows per tile (caller-allocated).
 * Row r of tile b lives at index b*max_per_img + r.  Rows are in the reference's NMS order
 * (score descending); `bbox2result` class grouping is done by the host mirror. */
typedef struct nuhtc_dets {
  float*    boxes;      /* dev [B*max_per_img*5]  x1,y1,x2,y2,score in original-tile pixels */
  int32_t*  labels;     /* dev [B*max_per_img] */
  int32_t*  counts;     /* dev [B]  detections per tile */
  uint32_t* masks;      /* dev [B*max_per_img * tile_h * (tile_w/32)] bit-packed rows, bit (x&31) of word x>>5; may be NULL */
  int32_t*  areas;      /* dev [B*max_per_img] mask pixel counts; may be NULL */
  uint8_t*  keep;       /* dev [B*max_per_img] 1 = survives the infer_wsi.py margin/min_area filter + mask-NMS; may be NULL */
} nuhtc_dets;

/* The hot path: B tiles (B <= max_batch) of tile_h x tile_w x 3 uint8 HWC in device memory ->
 * detections.  Replaces `inference_detector(model, [ndarray]*B)` (mmdet/apis/inference.py:90) and,
 * when out->keep != NULL, tools/infer_wsi.py:510-531.  Enqueues on `stream`; does not synchronise. */
int nuhtc_infer(nuhtc_engine* e, const uint8_t* tiles_dev, int B, int channel_mode, void* stream, const nuhtc_dets* out);

/* Tile embeddings (v11): B tiles (B <= max_batch) as for nuhtc_infer -> feat_dev [B][256] float32 = the per-channel mean of the four FPN
 * maps over their whole padded grid (pad_shape / 4 .. / 32), levels 0..3 of 64 channels each.  Replaces `model_feat` of the reference's
 * tools/extract_features_nuhtc.py:37-91 (`model.extract_feat` = Swin-T + FPN, then `features_lvl[l].mean(dim=(2, 3))`, concatenated).
 * Runs the backbone and the FPN (laterals + fpn_convs, without the semantic head's lateral in their epilogue), nothing of the heads, then
 * the pooling (csrc/pool.hip: fp64 partials in a fixed layout, no float atomics -- bitwise the same features for a tile in any batch, on
 * any call).  nuhtc_get_buffer("x0".."x3") returns the maps afterwards.  Enqueues on `stream`; does not synchronise. */
int nuhtc_features(nuhtc_engine* e, const uint8_t* tiles_dev, int B, int channel_mode, void* stream, float* feat_dev);

/* Fixed-load variant for benchmarking with synthetic weights: the proposal stage is
 * computed but replaced by `rois_dev` (dev [B*n_rois*4] x1,y1,x2,y2 in network pixels), and exactly
 * `n_dets` highest-scoring (roi,class) pairs per tile are carried into the mask branch. */
int nuhtc_infer_fixed_load(nuhtc_engine* e, const uint8_t* tiles_dev, int B, int channel_mode, const float* rois_dev,
                           int n_rois, int n_dets, void* stream, const nuhtc_dets* out);

/* Outer contours of the instance masks of a finished nuhtc_infer, traced on the device so that only vertex lists leave it.
 * Replaces `mask2inst` (tools/infer_wsi.py:51-54: cv2.findContours(mask, RETR_TREE, CHAIN_APPROX_SIMPLE)[0][0]) applied
 * to every detection that survived the per-tile filter + mask-NMS (:533-539).  For detection slot s = b*max_per_img + r
 * with r < dets->counts[b] and (dets->keep == NULL or dets->keep[s]):  n_dev[s] = number of vertices written to
 * xy_dev[s*cap*2 ..] as (x, y) int16 pairs in tile pixels, open ring (the caller repeats the first point and adds the
 * tile origin); n_dev[s] = -1 if the contour has more than `cap` vertices (trace that one on the host; the length of the
 * border itself is not limited); n_dev[s] = 0 for slots that are not traced.  dets->masks and dets->counts must be non-NULL.
 * Enqueues on `stream`; does not synchronise. */
int nuhtc_mask_contours(nuhtc_engine* e, const nuhtc_dets* dets, int B, int cap, int16_t* xy_dev, int32_t* n_dev, void* stream);

/* Compacts the kept detections of a finished nuhtc_infer (slots r < counts[b] with keep set), in (tile, slot) order, into
 * dense device buffers of capacity `cap` rows, so that a slide loop fetches a batch's results with a few fixed-size
 * asynchronous copies instead of one copy per detection (the fields tools/infer_wsi.py:486-539 reads out of `result`):
 * n_dev [2]: [0] = number of kept detections (may exceed cap: then only the first cap rows were written and the caller falls
 * back to reading the detection buffers directly), [1] = the capacity flag of that inference (non-zero: nuhtc_check would return
 * NUHTC_E_CAPACITY; v5); idx_dev [cap] = b * max_per_img + r; boxes_dev [cap][5]; labels_dev
 * [cap]; cn_dev [cap] / xy_dev [cap][contour_cap][2] = contour length / vertices from nuhtc_mask_contours (contour_n /
 * contour_xy may be NULL: cn = 0, no vertices); words_dev [cap][tile_h * tile_w / 32] = the bit-packed masks.
 * Enqueues on `stream`; does not synchronise. */
int nuhtc_export_kept(nuhtc_engine* e, const nuhtc_dets* dets, int B, const int32_t* contour_n, const int16_t* contour_xy, int contour_cap,
                      int cap, int32_t* n_dev, int64_t* idx_dev, float* boxes_dev, int32_t* labels_dev, int32_t* cn_dev, int16_t* xy_dev,
                      uint32_t* words_dev, void* stream);

/* Crops the masks nuhtc_export_kept compacted (words_dev [n][tile_h * tile_w / 32], n = min(*n_dev, cap)) to their bounding
 * rectangles, on the device: crop_box_dev [cap][4] = x0, y0, x1, y1 in tile pixels (x1 / y1 exclusive; zeros for an empty mask),
 * crop_area_dev [cap] = set pixels, crop_off_dev [cap + 1] = word offset of each crop in crop_words_dev (entry cap = total words the
 * crops need: when it exceeds pool_cap the crops past the pool were not written and the caller cuts those from words_dev),
 * crop_words_dev = rows of (w + 31) / 32 words with crop column x in bit x & 31 of word x >> 5 -- the layout nuhtc_merge_overlap
 * takes.  Replaces the per-detection numpy slicing of the slide loop (tools/infer_wsi.py:533-566 works on such crops).
 * Enqueues on `stream`; does not synchronise. */
int nuhtc_export_crops(nuhtc_engine* e, const uint32_t* words_dev, const int32_t* n_dev, int cap, int32_t* crop_box_dev, int32_t* crop_area_dev,
                       int32_t* crop_off_dev, uint32_t* crop_words_dev, int pool_cap, void* stream);

/* Overlap measure of nuhtc_merge_overlap. */
enum {
  NUHTC_OVERLAP_MASK = 0,     /* IoU of the instance masks (pixel sets) */
  NUHTC_OVERLAP_POLYGON = 1   /* the reference's: IoU of the shapely polygons of the rings tools/infer_wsi.py writes (first contour of
                                 cv2.findContours through the border-pixel centres; buffer(0) + largest part when the ring touches
                                 itself, tools/nuclei_merge.py:37-59), computed exactly from the mask crops (csrc/merge.hip) */
};

/* Cross-tile duplicate removal over all detections of a slide: tools/nuclei_merge.py:62-174 `merge_overlap`, strategy
 * 'probability' (visit in descending score, ties by lower index; an alive detection removes every later one whose overlap
 * with it exceeds `thr`, compared as a double division like the reference's `inter.area / (a.area + b.area - inter.area)`).
 * All pointers are device memory of `device`:  boxes [n][4] int32 = x0,y0,x1,y1 (x1,y1 exclusive) of each mask crop in
 * slide pixels (the bounding box of the mask's set pixels); scores [n]; areas [n] = set pixels (NUHTC_OVERLAP_MASK only, may
 * be NULL otherwise); bits = the crops, bit-packed row by row, (x1-x0+31)/32 uint32 words per row, pixel x of a row in bit
 * (x&31) of word x>>5; bit_off [n] = word offset of each crop in `bits`; n_words = total words of `bits`.
 * x_min..y_max bound all boxes (the slide extent).  keep_dev [n] receives 1 for kept detections.  Allocates its own scratch
 * (about 120 bytes per detection, plus a copy of `bits` in polygon mode), runs on `stream` and synchronises it before
 * returning.  A detection may have any number of higher-scored overlapping neighbours (24 are kept inline, the rest in a
 * spill pool that is grown and the pass repeated when it runs out); NUHTC_E_CAPACITY only if 2^30 spill entries do not
 * suffice.  The decision rounds run until nothing changes, however long a chain of overlapping neighbours is (one level per
 * launch); every detection is decided after at most n launches, and NUHTC_E_CAPACITY is returned, never a keep set, should
 * that bound be passed.  NUHTC_E_INVALID in polygon mode if a crop exceeds about 430x430 pixels. */
int nuhtc_merge_overlap(int device, const int32_t* boxes, const float* scores, const int32_t* areas, const uint32_t* bits,
                        const int64_t* bit_off, int64_t n, int64_t n_words, int overlap, double thr, int x_min, int y_min,
                        int x_max, int y_max, uint8_t* keep_dev, void* stream);

/* Synchronises `stream` and reports whether the last nuhtc_infer overflowed max_cc_proposals on some tile (returns
 * NUHTC_E_CAPACITY) — call before trusting the results.  That is the only capacity of the path that is not the reference's
 * own cap: RPN candidates, RoIs and detection candidates are sized for their worst case (nms_pre per level,
 * max_cc_proposals + rpn_max_per_img, RoIs x classes), detections are cut at max_per_img as the reference cuts them. */
int nuhtc_check(nuhtc_engine* e, void* stream);

/* Parity-test access to intermediate tensors of the last nuhtc_infer call (device pointers into the
 * engine workspace; valid until the next call).  Names: "img", "c0".."c3", "x0".."x3", "rpn0".."rpn3",
 * "sem_pred", "sem_feat", "rpn_props", "rpn_counts", "cc_mask", "cc_props", "cc_counts", "rois", "roi_counts",
 * "cls0".."cls2", "reg0".."reg2", "bbox_feats", "mask_prob", "tokens<stage><block>" ...
 * shape receives up to 6 dims; *dtype: 0=f32, 1=i32, 2=u8, 3=u32.
 * Two of them are not written by the step any more (either matrix pipe) and are computed by this call, synchronising the device: "img" (the
 * pre-processing runs inside the patch embedding) and "c0".."c3" (the stages' output norms run inside the FPN laterals; computed from the
 * stages' token buffers).  LIFETIME of "img": the engine keeps only the POINTER of the last nuhtc_infer's `tiles` and reads it again here --
 * the caller must keep that device buffer alive and unchanged until it has fetched "img" (or never ask for it); a step that fails drops
 * the pointer ("img" then returns whatever the buffer held). */
int nuhtc_get_buffer(nuhtc_engine* e, const char* name, void** dev_ptr, int64_t* shape, int* ndim, int* dtype);

/* Stand-alone ops for kernel-level parity tests (all pointers device memory, fp32). */
/* C[M,N] = act(A[M,K] * W[N,K]^T + bias[N]);  act: 0 none, 1 relu, 2 gelu(erf).  K%32==0, N%32==0. */
int nuhtc_op_gemm(nuhtc_engine* e, const float* A, const float* W, const float* bias, float* C, int M, int N, int K,
                  int act, void* stream);
/* The same product on the bf16 matrix pipe with exactly split operands (NUHTC_PIPE_BF16_SPLIT); W_host = host copy of W_dev (the
 * split of a constant weight is made on the host, as at nuhtc_finalize).  Synchronises `stream`. */
int nuhtc_op_gemm_split(nuhtc_engine* e, const float* A, const float* W_dev, const float* W_host, const float* bias, float* C, int M,
                        int N, int K, int act, void* stream);
/* ABI v8 (round 5).  A linear behind a LayerNorm with the norm in the product's A path (csrc/gemm.hip A_LN; what the QKV and fc1 linears of
 * Swin stages 2-4 run: mmdet swin.py:358,365): C[M,N] = act(LN(X[rows[m]])[M,K] * W[N,K]^T + bias[N]) with LN = LayerNorm(K, eps 1e-5,
 * ln_g, ln_b).  W, bias, ln_g, ln_b are HOST arrays (the norm's affine part is folded into the linear on the host exactly as nuhtc_finalize
 * folds it: W' = W diag(ln_g) rounded once to fp32 and split exactly, bias' = bias + W ln_b in fp64); X [T][K] and `rows` (device int32 [M]
 * indices into X, or NULL for the identity with M <= T) are device memory.  The row statistics come from ln_stats_kernel (csrc/swin.hip).
 * N % 96 == 0, K % 32 == 0.  Synchronises `stream`. */
int nuhtc_op_ln_gemm(nuhtc_engine* e, const float* X_dev, int T, const int* rows_dev, const float* W_host, const float* bias_host, const float* ln_g_host,
                     const float* ln_b_host, float* C_dev, int M, int N, int K, int act, void* stream);
/* The same linear fed the way the engine feeds it: a producer product Y[row_map(m)] = A[M,Kp] * Wp[K,Kp]^T + bp (+ res[row_map(m)]) whose
 * epilogue leaves, per row and 96 columns, {mean, sum of squared deviations} of what it stored (GemmParams.stats_out), and the A_LN linear
 * C = act(LN(Y) * W^T + bias) that merges those partials -- no pass over Y computes statistics.  Y_dev [M][K] and C_dev [M][N] are outputs;
 * row_map_dev (device int32 [M], a permutation of 0..M-1) and res_dev ([M][K]) may be NULL.  K % 96 == 0, N % 96 == 0.  Synchronises `stream`. */
int nuhtc_op_gemm_ln_gemm(nuhtc_engine* e, const float* A_dev, const float* Wp_host, const float* bp_host, const float* res_dev, const int* row_map_dev,
                          const float* W_host, const float* bias_host, const float* ln_g_host, const float* ln_b_host, float* Y_dev, float* C_dev, int M,
                          int Kp, int K, int N, int act, void* stream);
/* ABI v9 (round 5).  PatchMerging (mmdet/models/utils/transformer.py:363-385: nn.Unfold(2, stride 2), LayerNorm(4C), Linear(4C -> 2C, no bias)) as
 * the engine runs it on the split pipe: ONE product whose A rows are gathered from the token tensor as two runs of 2C floats (the 2 x 2 tokens of
 * a merged row), the norm in the A path (csrc/gemm.hip A_LN with seg_k) and the row statistics merged from per-token partials over 96 channels.
 * X_dev [B*H*W][C] tokens; W_host [2C][4C], ln_g_host / ln_b_host [4C] in the REFERENCE's column order k = c*4 + kh*2 + kw (re-ordered here exactly as
 * nuhtc_finalize re-orders them); Y_dev [B*(H/2)*(W/2)][2C].  H, W even, C % 96 == 0.  Synchronises `stream`. */
int nuhtc_op_merge_ln_gemm(nuhtc_engine* e, const float* X_dev, int B, int H, int W, int C, const float* W_host, const float* ln_g_host,
                           const float* ln_b_host, float* Y_dev, void* stream);
/* The fused FFN half of a Swin block (csrc/mlp.hip; mmdet swin.py:365-367): out[T,C] = x + W2 gelu(W1 LN(x) + b1) + b2 with
 * LN = LayerNorm(C, eps 1e-5, ln_g, ln_b), W1 [4C][C], W2 [C][4C] given as HOST arrays (packed like nuhtc_finalize packs them),
 * everything else device memory.  C must be a width the fused kernel serves (96).  Synchronises `stream`. */
int nuhtc_op_swin_mlp(nuhtc_engine* e, const float* x_dev, const float* ln_g_dev, const float* ln_b_dev, const float* w1_host,
                      const float* b1_dev, const float* w2_host, const float* b2_dev, float* out_dev, int T, int C, void* stream);
/* ABI v6 (round 4).  The same kernel with the attention projection in front (mmdet swin.py:360-367, the second half of a Swin block from the
 * attention output on):  x' = x + Wp att + bp;  out = x' + W2 gelu(W1 LN(x') + b1) + b2.  att [T,C] in token order, Wp [C][C] given as a HOST
 * array, everything else as in nuhtc_op_swin_mlp.  Synchronises `stream`. */
int nuhtc_op_swin_proj_mlp(nuhtc_engine* e, const float* x_dev, const float* att_dev, const float* wp_host, const float* bp_dev,
                           const float* ln_g_dev, const float* ln_b_dev, const float* w1_host, const float* b1_dev, const float* w2_host,
                           const float* b2_dev, float* out_dev, int T, int C, void* stream);
/* mmcv RoIAlign(avg, aligned=True) on an NHWC map: feat [N,H,W,C=64], rois [R,5] -> out [R,P,P,C]. */
int nuhtc_op_roi_align(nuhtc_engine* e, const float* feat_nhwc, int N, int H, int W, const float* rois, int R, int P,
                       float spatial_scale, int sampling_ratio, float* out, void* stream);
/* mmcv nms on n boxes (n <= 16384): keep_idx[0..*count) in descending-score order (ties: lower index). */
int nuhtc_op_nms(nuhtc_engine* e, const float* boxes, const float* scores, int n, float iou_thr, int32_t* keep_idx,
                 int32_t* count_dev, void* stream);
/* The two halves of the connected-component ("watershed") proposals of nuhtc_infer (htc_roi_head_cus.py:283-342), as test entry points.
 * nuhtc_op_cc_mask: semantic logits sem_pred [B,h,w] -> bilinear (align_corners) to [H,W], 5x5 Gaussian (sigma 1.1, reflect pad), > 0
 * -> mask_out [B,H,W] uint8 (0/1).  H, W >= 2.
 * nuhtc_op_cc_proposals: binary mask [B,H,W] -> opened_out (the mask after open(5x5, 2) when `open`, else a copy) -> filled_out
 * (binary_fill_holes, 4-connected background) -> labels_out [B,H,W] (4-connected components of the filled mask; label = raster index
 * of the component's first pixel within its image, -1 for background) -> stats_out [B,H*W,5] (area, xmin, ymin, xmax, ymax at the
 * root's index; area 0 elsewhere) -> boxes_out [B,cap,4] / counts_out [B] (components with min_area < area < H*W/4 in raster order,
 * [xmin, ymin, xmax+1, ymax+1]); *overflow_out = number of images with more than `cap` such components (cap <= 4096).
 * Scratch is allocated per call.  Synchronises `stream`. */
int nuhtc_op_cc_mask(nuhtc_engine* e, const float* sem_pred_dev, int B, int h, int w, int H, int W, uint8_t* mask_out_dev, void* stream);
int nuhtc_op_cc_proposals(nuhtc_engine* e, const uint8_t* mask_dev, int B, int H, int W, int open, int min_area, int cap, uint8_t* opened_out,
                          uint8_t* filled_out, int32_t* labels_out, int32_t* stats_out, float* boxes_out, int32_t* counts_out,
                          int32_t* overflow_out, void* stream);
/* A 3x3 convolution 64 -> 64 (zero padding 1) with the options the engine uses, as a test entry point: the weights are packed as
 * nuhtc_finalize packs them (private copies, freed before the call returns) and the launch goes through the engine's GEMM dispatch,
 * so the halo kernel (csrc/conv.hip) serves pipe NUHTC_PIPE_BF16_SPLIT and the implicit-GEMM kernel (csrc/gemm.hip) NUHTC_PIPE_FP32.
 * in / out: device NHWC [nimg][H][W][64]; w: HOST [64][64][3][3] (OIHW); bias: HOST [64] or NULL; act: 0 none, 1 relu.
 * nimg_dev: optional device int32 image count (images >= *nimg_dev are not written).
 * N2 = 32 / 64 fuses a pointwise layer 64 -> N2 on the activated output (split pipe only): out2 [..][N2] = act2(w2 . out + b2) with
 * w2 / b2 HOST [N2][64] / [N2]; store_out = 0 drops `out`; out3 = res2 + out2 (N2 = 64, device [..][64]); outn1 [..] = wn1 . out + bn1
 * (HOST [64] / [1]).  n_more <= 3 further maps (device more_in / more_out2, more_H x more_W, nimg images each) go through the same layers
 * in the same launch (only without store_out, out3, outn1 and nimg_dev).  An option the path does not serve returns NUHTC_E_INVALID.
 * Synchronises `stream`. */
typedef struct nuhtc_conv3_args {
  const float* in;
  float* out;
  const float* w;
  const float* bias;
  int32_t nimg, H, W, act;
  const int32_t* nimg_dev;
  int32_t pipe;
  int32_t N2;
  const float* w2;
  const float* b2;
  int32_t act2, store_out;
  float* out2;
  const float* res2;
  float* out3;
  const float* wn1;
  const float* bn1;
  float* outn1;
  int32_t n_more;
  const float* more_in[3];
  float* more_out2[3];
  int32_t more_H[3], more_W[3];
} nuhtc_conv3_args;
int nuhtc_op_conv3(nuhtc_engine* e, const nuhtc_conv3_args* a, void* stream);
/* The attention half of a Swin block up to the attention output (mmdet swin.py:356-363 -> ShiftWindowMSA -> WindowMSA up to, not including,
 * `proj`), as a test entry point: LN1, pad to a multiple of 7, roll(-3, -3) when `shifted`, window partition, QKV, softmax(scale q k^T +
 * relative-position bias [+ shift mask]) v, reverse partition, roll back, crop.  x: device [B][H][W][C] tokens before LN1; out: device
 * [B*H*W][C], rows in token order (out_order NUHTC_ORDER_TOKEN: b*H*W + y*W + x) or in the compact window order of the (shift state's)
 * window image (NUHTC_ORDER_COMPACT: the non-padding window rows in window order).  ln_g / ln_b [C], qkv_w [3C][C], qkv_b [3C], rel_table
 * [169][C/32] are HOST arrays, packed as nuhtc_finalize packs them.  The geometry (window maps, padding rows, shift mask) is built by the
 * code the engine builds its own with, for this (B, H, W), and the launches are the engine's route for (pipe, C): on the split pipe the
 * fused LN1 + QKV kernel (C = 96) or ln_stats + the A_LN linear (C > 96), one bias row behind the window image and the attention kernel that
 * reads it for every padding row; on the fp32 pipe layernorm_windows + the linear + the fp32 attention kernel.  Private scratch, freed
 * before the call returns.  C in {96, 192, 384, 768}; B, H, W >= 1.  Synchronises `stream`. */
enum { NUHTC_ORDER_TOKEN = 0, NUHTC_ORDER_COMPACT = 1 };
typedef struct nuhtc_wmsa_args {
  const float* x;
  float* out;
  const float* ln_g;
  const float* ln_b;
  const float* qkv_w;
  const float* qkv_b;
  const float* rel_table;
  int32_t B, H, W, C;
  int32_t shifted, pipe, out_order;
} nuhtc_wmsa_args;
int nuhtc_op_window_msa(nuhtc_engine* e, const nuhtc_wmsa_args* a, void* stream);
/* The front of the path and the small dense kernels, op by op, as test entry points.  Each goes through the host code nuhtc_finalize and the step
 * use for the same launch (resize tables, weight repacking, the lateral's GEMM parameters, the pooling's chunk layout), with private scratch that
 * is freed before the call returns.  Pointers are device memory unless named *_host.  Each synchronises `stream`.
 * nuhtc_op_patch_embed: tiles [B][th][tw][3] uint8 with the image in the top-left valid_h x valid_w -> cv2's 8-bit linear resize by scale_factor,
 *   channel swap (channel_mode), Normalize (mean[3], std[3]: HOST), zero Pad to a multiple of 32 (Hn x Wn), the 4x4 stride-4 convolution (w_host
 *   [96][3][4][4], b_host [96]) and LayerNorm(96) (ln_g_host, ln_b_host) -> tok [B * Hn/4 * Wn/4][96] by patch_embed_tiles_kernel; img (may be NULL)
 *   [B][Hn][Wn][3], the normalised padded image by preproc_kernel from the same tables.  Refuses what nuhtc_create refuses of a scale: outside
 *   [1, 8], or scale_factor * valid size not an integer (any resized size >= 1 is served here).
 * nuhtc_op_layernorm: y [rows][C] = LayerNorm(x [rows][C]) (eps 1e-5) by the kernels launch_layernorm picks without a row map: C in {96, 192, 384, 768}.
 * nuhtc_op_merge_ln: PatchMerging's gather + LayerNorm(4C) of the fp32 pipe: x [B][H][W][C] -> y [B * H/2 * W/2][4C], column k = (kh*2+kw)*C + c;
 *   g, b [4C] in THAT order (nuhtc_finalize permutes the checkpoint's nn.Unfold order c*4 + kh*2+kw into it).  H, W even, C in {96, 192, 384}.
 * nuhtc_op_fpn_lateral: out [B][H][W][64] = X W^T + bias (+ parent [B][H/2][W/2][64] at (y / 2, x / 2), NULL: the top level), parameters as run_fpn
 *   fills them.  X [B*H*W][C]; W_host [64][C], bias_host [64].  With ln_g_host / ln_b_host [C] the rows are LayerNorm'ed in the product's A path
 *   (split pipe: the norm folded into W and bias as nuhtc_finalize folds it, statistics by ln_stats_kernel as one partial per 96 columns -- what the
 *   producers' epilogues leave); with both NULL X is used as it is and the product runs on the fp32 MFMA kernel (the fp32 pipe's form).
 * nuhtc_op_sem_fuse: out [B][H][W][64] = relu(g0) + sum_i relu(bilinear_align_corners(g_i [B][H >> i][W >> i][64] -> H x W)), i = 1..3; H, W % 8 == 0.
 * nuhtc_op_pointwise64: y [row] = w [64] . x [row][64] + b [1].  rows_dev NULL: the fixed-row launch over `rows` rows (sigmoid must be 0); else the
 *   grid-strided launch sized by the capacity `rows`, limited on the device to min(rows, *rows_dev * rows_mul) rows, y = sigmoid(.) when `sigmoid`.
 * nuhtc_op_fpn_mean_pool: maps[l] [B][hw[l]][64] -> feat [B][256] = the per-channel means, level-major (the pooling of nuhtc_features). */
int nuhtc_op_patch_embed(nuhtc_engine* e, const uint8_t* tiles_dev, int B, int th, int tw, int valid_h, int valid_w, float scale_factor, int channel_mode,
                         const float* mean, const float* std, const float* w_host, const float* b_host, const float* ln_g_host, const float* ln_b_host,
                         float* tok_dev, float* img_dev, void* stream);
int nuhtc_op_layernorm(nuhtc_engine* e, const float* x_dev, const float* g_dev, const float* b_dev, float* y_dev, int rows, int C, void* stream);
int nuhtc_op_merge_ln(nuhtc_engine* e, const float* x_dev, const float* g_dev, const float* b_dev, float* y_dev, int B, int H, int W, int C, void* stream);
int nuhtc_op_fpn_lateral(nuhtc_engine* e, const float* X_dev, int B, int H, int W, int C, const float* W_host, const float* bias_host, const float* ln_g_host,
                         const float* ln_b_host, const float* parent_dev, float* out_dev, void* stream);
int nuhtc_op_sem_fuse(nuhtc_engine* e, const float* g0, const float* g1, const float* g2, const float* g3, float* out, int B, int H, int W, void* stream);
int nuhtc_op_pointwise64(nuhtc_engine* e, const float* x_dev, const float* w_dev, const float* b_dev, float* y_dev, int rows, const int32_t* rows_dev,
                         int rows_mul, int sigmoid, void* stream);
int nuhtc_op_fpn_mean_pool(nuhtc_engine* e, const float* const maps[4], const int32_t hw[4], int B, float* feat_dev, void* stream);
/* The detection tail of nuhtc_infer, op by op, as test entry points (csrc/roi.hip: everything behind the RoI features that turns numbers into
 * decisions).  Each fills the parameter block nuhtc_infer fills and calls the same launch function; integer arrays a kernel indexes with
 * (*r_dev, roi_off / roi_cnt, det_off / det_counts) are read back and checked against the stated capacities first.  All pointers are device
 * memory unless marked HOST.  Each synchronises `stream`.  NUHTC_E_INVALID: a null pointer, nc + 6 > 64 or nc + 2 > 16, max_keep /
 * max_per_img > 2048, W % 32 != 0, a valid canvas outside H x W, B > 256, counts beyond the capacities.
 * nuhtc_op_bbox_tail: h [cap][256] (the output of the two shared FCs) -> cls [cap][16] (nc + 2 used: NormedLinear, 20 * h / (|h| + 1e-6) against
 *   the row-normalised fc_cls), reg [cap][4] (fc_reg) and, with `refine`, rois [cap][5] regressed in place (delta2bbox, stds, clipped to img_w x
 *   img_h) for the rows below *r_dev; rows from *r_dev on are not written.  cls_w [nc+2][256], cls_b [nc+2], reg_w [4][256], reg_b [4] are HOST
 *   arrays in the checkpoint's layout, packed as nuhtc_finalize packs them. */
typedef struct nuhtc_bbox_tail_args {
  const float* h;
  const float* cls_w;
  const float* cls_b;
  const float* reg_w;
  const float* reg_b;
  int32_t nc, cap, refine;
  float stds[4];
  float img_w, img_h;
  const int32_t* r_dev;
  float* rois;
  float* cls;
  float* reg;
} nuhtc_bbox_tail_args;
int nuhtc_op_bbox_tail(nuhtc_engine* e, const nuhtc_bbox_tail_args* a, void* stream);
/* nuhtc_op_det_post: mean of the three stages' logits, Seesaw activation, delta2bbox / scale, score > score_thr -> the candidates of tile b
 *   (RoIs roi_off[b] .. + roi_cnt[b] of rois [total][5], cls0..2 [total][16], reg2 [total][4]) in (roi, class) order: cand_count [B],
 *   cand_scores / cand_ids [B][cap], cand_boxes [B][cap][4] (cap: a multiple of 64 up to 16384; candidates beyond it are dropped) -> multiclass
 *   NMS (mmcv batched_nms: class offset max(boxes of the tile) + 1, IoU > nms_iou) -> dets [B][max_per_img][5], labels [B][max_per_img],
 *   counts [B] (clamped to `limit`), mask_rois [sum counts][5] (tile, box * scale; room for B * max_per_img rows), det_off [B], det_total [1].
 *   Needs a finalized engine. */
typedef struct nuhtc_det_post_args {
  const float* rois;
  const float* cls0;
  const float* cls1;
  const float* cls2;
  const float* reg2;
  const int32_t* roi_off;
  const int32_t* roi_cnt;
  int32_t B, nc, total, cap;
  float stds[4];
  float img_w, img_h, scale, score_thr, nms_iou;
  int32_t max_per_img, limit;
  float* dets;
  int32_t* labels;
  int32_t* counts;
  float* mask_rois;
  int32_t* det_off;
  int32_t* det_total;
  int32_t* cand_count;
  float* cand_scores;
  int32_t* cand_ids;
  float* cand_boxes;
} nuhtc_det_post_args;
int nuhtc_op_det_post(nuhtc_engine* e, const nuhtc_det_post_args* a, void* stream);
/* nuhtc_op_paste: prob [D][28][28] and mask_rois [D][5] (network pixels; detection j of tile b is row det_off[b] + j, j < det_counts[b]) ->
 *   masks [B][max_keep][H][W/32] (bit x & 31 of word x >> 5: bilinear sample of the box's probability map >= thr, inside the box's integer hull
 *   and the valid canvas vH x vW) and areas [B][max_keep] (set bits).  Slots from det_counts[b] on are not written. */
typedef struct nuhtc_paste_args {
  const float* prob;
  const float* mask_rois;
  const int32_t* det_off;
  const int32_t* det_counts;
  int32_t B, D, max_keep, H, W, vH, vW;
  float scale, thr;
  uint32_t* masks;
  int32_t* areas;
} nuhtc_paste_args;
int nuhtc_op_paste(nuhtc_engine* e, const nuhtc_paste_args* a, void* stream);
/* nuhtc_op_tile_post: dets [B][max_keep][5], labels, areas [B][max_keep], masks as above (each inside the integer hull of its box: the pair test
 *   skips masks whose hulls do not meet) -> keep [B][max_keep] uint8 for the slots below det_counts[b]: margin / min_area filter, then greedy
 *   mask-NMS at IoU > thr (rounded to the double the reference compares with) in the order score descending, ties by class-major position
 *   descending.  Slots from det_counts[b] on are not written. */
typedef struct nuhtc_tile_post_args {
  const float* dets;
  const int32_t* labels;
  const int32_t* areas;
  const int32_t* det_counts;
  const uint32_t* masks;
  uint8_t* keep;
  int32_t B, max_keep, H, W, vH, vW, margin, min_area;
  float thr;
} nuhtc_tile_post_args;
int nuhtc_op_tile_post(nuhtc_engine* e, const nuhtc_tile_post_args* a, void* stream);
/* The RPN half of the proposals of nuhtc_infer, op by op, as test entry points (csrc/proposals.hip, build_rois_kernel of csrc/roi.hip).  Each
 * fills the parameter block nuhtc_infer fills and calls the same launch function; scratch is allocated per call; counts a kernel indexes with are
 * read back and checked against the capacities first.  All pointers are device memory.  Each synchronises `stream` and needs a finalized engine.
 * nuhtc_op_rpn_select: the four level maps out[l] [B][h[l] * w[l]][32] (columns 0-2 objectness logits, 3 + 4 a + j the deltas of anchor a; stride
 *   4 << l) -> per (image, level) the nms_pre best anchors by (score descending, index ascending) -- all of them in index order when the level has
 *   no more than nms_pre -- decoded (delta2bbox, stds 1), clipped to img_w x img_h and kept where width and height > min_size:
 *   cand_boxes [B][4][nms_pre][4], cand_scores [B][4][nms_pre], cand_count [B][4]; slots from the count on are not written.  The key scratch row
 *   holds the largest level rounded up to 64 (level 0 in the engine).  NUHTC_E_INVALID: nms_pre outside 1..4096, B outside 1..256, h or w < 1.
 * nuhtc_op_nms_levels: candidates boxes [B][G][slot][4], scores [B][G][slot], group_count [B][G] -> mmcv batched_nms with id = group, the first
 *   max_keep survivors: dets [B][max_keep][5], src [B][max_keep] (flat index into scores), counts [B].  route 0: launch_nms_levels (the engine's RPN
 *   route), route 1: launch_nms with ids == null.  The capacity of the sorted list is that of the engine's workspace for G levels of `slot`
 *   candidates: G * slot rounded up to 64 (at least 64) plus 64 (G - 1).  All scratch of the call (sorted boxes, sources, positions, segment tables,
 *   survivor words, the mask matrix) is filled with 0xFF bytes before the launch.  NUHTC_E_INVALID: G outside 1..16, slot outside 1..16384, max_keep
 *   < 1, a count outside 0..slot, and what the launch functions refuse (G * max_keep > 8192 on route 0, a capacity beyond their limits).
 * nuhtc_op_build_rois: per image cat(cc_boxes [B][cc_cap][4] below cc_counts [B], rpn_dets [B][rpn_cap][5] below rpn_counts [B]) (cc_boxes NULL:
 *   RPN rows alone), or with `fixed` [B][n_fixed][4] those rows -> rois [cap][5] (image index, box) flattened over the batch, roi_off / roi_cnt [B],
 *   total [1]; rows from *total on are not written.  NUHTC_E_INVALID: B outside 1..256, counts beyond the capacities, more rows than `cap`. */
int nuhtc_op_rpn_select(nuhtc_engine* e, const float* const out[4], const int32_t h[4], const int32_t w[4], int B, int nms_pre, int img_h, int img_w,
                        float min_size, float* cand_boxes, float* cand_scores, int32_t* cand_count, void* stream);
int nuhtc_op_nms_levels(nuhtc_engine* e, const float* boxes, const float* scores, const int32_t* group_count, int B, int G, int slot, float iou_thr,
                        int max_keep, int route, float* dets, int32_t* src, int32_t* counts, void* stream);
int nuhtc_op_build_rois(nuhtc_engine* e, const float* cc_boxes, const int32_t* cc_counts, int cc_cap, const float* rpn_dets, const int32_t* rpn_counts,
                        int rpn_cap, const float* fixed, int n_fixed, int B, int cap, float* rois, int32_t* roi_off, int32_t* roi_cnt, int32_t* total,
                        void* stream);

/* The block of nuhtc_infer that turns RoIs into head features, op by op, as test entry points (csrc/roi.hip: the attention-pool tables, roi_classify_kernel,
 * the LDS-tile, stream, big-box and giant kernels of the 7 x 7 features and roi_feat14_kernel).  Each fills the parameter block nuhtc_infer fills and
 * calls the same function; scratch is allocated per call; *r_dev and the image index of every live RoI are read back and checked first.  All pointers are
 * device memory.  Each synchronises `stream` and needs a finalized engine.
 * nuhtc_op_attn_pool: level map F [B][HW][64] -> G [B][HW][64], G[b][q] = mean_p F[b][p] * (relu(cos(F[b][q], F[b][p]) - tau) + tau), by `route`:
 *   NUHTC_AP_AUTO what nuhtc_infer picks (attn_pool_fp16_kernel with nuhtc_config.att_pool_fp16, else the cosine-epilogue GEMM pair where HW % 32 == 0
 *   and attn_pool_kernel otherwise), or one of them by name.  NUHTC_E_INVALID: a null pointer, B outside 1..256, HW outside 1..16384 or B * HW * HW >
 *   2^28, an unknown route, NUHTC_AP_GEMM with HW % 32 != 0.
 * nuhtc_op_roi_feats: rois [cap][5] (image, x1, y1, x2, y2 in network pixels; rows below *r_dev are live) on x0 [B][H[0]][W[0]][64] (stride 4),
 *   x1 (stride 8, H[1] x W[1]), sem and x0sem = fp32 x0 + sem (both H[0] x W[0]) and the tables G2 [B][H[2] * W[2]][64], G3 -> out [cap][P * P][64]:
 *   RoIAlign(x0) + RoIAlign(x1) + G2[centre] + G3[centre] + the semantic RoIAlign(14, adaptive), average-pooled 2 x 2 for P = 7.  P = 7 also gives
 *   fb_flag [cap] (the kernel form of each RoI: 0 / 3 LDS tiles small / large, 1 stream, 2 big-box, 4 giant) and counts [3] (the lengths of the big,
 *   mid-size and giant lists); it runs with the side streams and events of the latency schedule and with the list forms (stream_few, the big-box
 *   split) as nuhtc_infer sets them.  Rows from *r_dev on are not written.  NUHTC_E_INVALID: a null pointer, P not 7 or 14, B outside 1..256, cap
 *   outside 1..2^20, a level size outside 1..4096, *r_dev outside 0..cap, a live RoI whose image index is not an integer in 0..B-1 or with a
 *   coordinate that is not finite. */
#define NUHTC_AP_AUTO 0
#define NUHTC_AP_GEMM 1
#define NUHTC_AP_KERNEL 2
#define NUHTC_AP_FP16 3
int nuhtc_op_attn_pool(nuhtc_engine* e, const float* F, int B, int HW, float tau, int route, float* G, void* stream);
typedef struct nuhtc_roi_feats_args {
  const float* x0;
  const float* x1;
  const float* sem;
  const float* x0sem;
  const float* G2;
  const float* G3;
  const float* rois;
  const int32_t* r_dev;
  int32_t B, cap, P;
  int32_t H[4], W[4];
  float* out;
  uint8_t* fb_flag;
  int32_t* counts;
} nuhtc_roi_feats_args;
int nuhtc_op_roi_feats(nuhtc_engine* e, const nuhtc_roi_feats_args* a, void* stream);

/* Scoring a batch on the device (csrc/eval.hip).  Replaces what the reference's `WSIDataset.evaluate` (nuhtc/datasets/WSI_coco.py:278-545) and
 * tools/analysis_tools/pannuke/compute_stats.py compute from decoded masks, up to the integer tables the metrics are functions of: the host
 * finishes with nuhtc_amd.evaluation.*_tables.  nuhtc_config is unchanged (no ABI bump).
 * nuhtc_eval_batch runs after nuhtc_infer on the same `dets`, enqueues on `stream` and does not synchronise:
 *   select : per tile, the detections with score >= fg_thr in descending score (equal scores: descending slot -- a stable ascending argsort,
 *            reversed), greedily suppressed where inter / max(union, 1) > mask_nms_thr, the comparison made in double on the popcounts like
 *            numpy's (`mask_nms`, nuhtc/utils/stats_utils.py:10-32).  sel [B][max_per_img] = kept slots in that order (-1 behind them),
 *            nsel [B], sel_labels [B][max_per_img] = their labels.  Unlike the slide path's keep flags there is no margin / min-area filter.
 *   pairs  : (gt_maps != NULL) gt_maps [B][tile_h][tile_w][num_classes] holds, per class channel, the ROW NUMBER + 1 of the ground-truth
 *            instance covering a pixel (0 = none; rows in class-major, ascending-id order, below t_cap <= 8192).  area_t [B][t_cap] = pixels of
 *            each row, area_p [B][max_per_img] = pixels of each selected prediction (in sel order), trips [trip_cap][4] = the non-zero
 *            intersections as (tile, row, position in sel, pixels), in no particular order.  counters[0] = entries the list needs (beyond
 *            trip_cap they were not written), counters[1] != 0: entries were dropped, counters[2] != 0: a map value outside [0, t_cap].
 *   render : (pred_maps != NULL) `convert_format` (WSI_coco.py:863-906) of the selected predictions: NUHTC_EVAL_PANNUKE -> pred_maps
 *            [B][tile_h][tile_w][num_classes + 1] (channel c = 1-based index within class c, later instances win; last channel 1 - any, all
 *            zero for a tile without predictions), NUHTC_EVAL_CONIC -> [B][tile_h][tile_w][2] = (1-based index, max class + 1).
 *   joint  : (gt_maps, pred_maps and joint != NULL, NUHTC_EVAL_PANNUKE) the joint histograms of `get_fast_pq_map` (pannuke/utils.py:7-104)
 *            between gt_maps and pred_maps, table k < num_classes for class k and table num_classes for the maps `binarize` makes of all
 *            classes (last non-zero channel wins; ids there are class << 27 | id, which keeps `binarize`'s class-major order):
 *            joint [joint_cap][5] = (tile, table, true id, pred id, pixels) for every pair that occurs, (0, 0) included;
 *            counters[4..6] as counters[0..2] (also set when a table holds more than 4096 distinct pairs).
 * All pointers are device memory; counters is int32 [8]. */
enum { NUHTC_EVAL_PANNUKE = 0, NUHTC_EVAL_CONIC = 1 };
typedef struct nuhtc_eval_args {
  const int32_t* gt_maps;
  int32_t t_cap, trip_cap, joint_cap, format;
  float fg_thr;
  double mask_nms_thr;
  int32_t* sel;
  int32_t* nsel;
  int32_t* sel_labels;
  int32_t* area_t;
  int32_t* area_p;
  int32_t* trips;
  int32_t* joint;
  int32_t* counters;
  int32_t* pred_maps;
} nuhtc_eval_args;
int nuhtc_eval_batch(nuhtc_engine* e, const nuhtc_dets* dets, int B, const nuhtc_eval_args* a, void* stream);
/* The four steps as test entry points on raw device arrays: masks [B][K][H][W/32] (bit x & 31 of word x >> 5), K <= 2048, W % 32 == 0,
 * C <= 14.  Every index read from device memory is range-checked by the kernels.  Each synchronises `stream`.
 * nuhtc_op_eval_select: scores[(b * K + j) * score_stride], counts [B]; labels / sel_labels may be NULL.
 * nuhtc_op_eval_pairs : counters int32 [4].   nuhtc_op_eval_render: out as pred_maps above.
 * nuhtc_op_eval_joint : true_maps [B][H][W][Ct], pred_maps [B][H][W][Cp] (any non-negative ids, Ct, Cp >= C; W any), counters int32 [4]. */
int nuhtc_op_eval_select(nuhtc_engine* e, const float* scores, int score_stride, const int32_t* counts, const uint32_t* masks, const int32_t* labels,
                         int B, int K, int H, int W, float fg_thr, double thr, int32_t* sel, int32_t* nsel, int32_t* sel_labels, void* stream);
int nuhtc_op_eval_pairs(nuhtc_engine* e, const uint32_t* masks, const int32_t* sel, const int32_t* nsel, const int32_t* gt_maps, int B, int K, int H,
                        int W, int C, int t_cap, int cap, int32_t* area_t, int32_t* area_p, int32_t* trips, int32_t* counters, void* stream);
int nuhtc_op_eval_render(nuhtc_engine* e, const uint32_t* masks, const int32_t* sel, const int32_t* nsel, const int32_t* labels, int B, int K, int H,
                         int W, int C, int format, int32_t* out, void* stream);
int nuhtc_op_eval_joint(nuhtc_engine* e, const int32_t* true_maps, int Ct, const int32_t* pred_maps, int Cp, int B, int H, int W, int C, int cap,
                        int32_t* joint, int32_t* counters, void* stream);

/* Scoring images larger than a tile on the device (csrc/stitch.hip): the protocol of `CoNSePCocoDataset.evaluate`
 * (nuhtc/datasets/WSI_coco_CoNSeP.py:117-426) -- overlapping tiles, detections near an inner tile edge dropped, the rest shifted into the image
 * frame, one mask-NMS per image, statistics against the image's instance map -- up to the integer tables nuhtc_amd.evaluation.*_tables finish.
 * nuhtc_config is unchanged (no ABI bump).
 * A store holds the candidates of n_img images, all device memory: per image cand_cap records -- box [n_img][cand_cap][4] = x0, y0, x1, y1 (exclusive)
 * of the mask's set pixels in image pixels (zeros for an empty mask), area, score, label, key (int64: (tile location * C + label) * K + slot, the
 * candidate order of the reference within an image), off (int64 word offset of the crop in the image's pool, -1: it did not fit) -- and
 * pool [n_img][pool_cap] words of crops in the nuhtc_merge_overlap layout.  counters [n_img][4]: [0] candidates and [1] pool words the image needs so
 * far (counted past the capacities; the caller zeroes them to start an image), [2] bit 0: candidates, bit 1: crops were dropped, [3] != 0: a label
 * outside [0, C) or a tile record out of range.  work: scratch of work_cap >= 8 * B * K int32.
 *   gather : tile_meta [B][8] = image, x offset, y offset, first column, last column, first row, last row (flags), tile location.  Slots
 *            r < counts[b] with score >= fg_thr (false for NaN) become candidates unless x1 < discard_offset on a tile that is not in the first
 *            column, x2 > tile - discard_offset on one not in the last, and the same for y1 / y2 and rows (float boxes).  Candidates are numbered
 *            behind those the image holds, in (tile of the batch, slot) order.  Tiles are square, side % 32 == 0.
 *            nuhtc_stitch_gather runs after nuhtc_infer on the same `dets`, enqueues on `stream` and does not synchronise.
 *   pairs  : kept [n_kept] = candidate numbers of one image (the survivors of its mask-NMS in visiting order); gt_map [H][W] = row + 1 of the
 *            ground-truth instance of a pixel, 0 = none, at most t_cap <= 8192.  area_t [t_cap] = pixels per row, trips [trip_cap][3] = (row,
 *            position in kept, pixels) of the non-zero intersections, in no particular order.  counters [4]: [0] entries needed, [1] entries
 *            dropped, [2] a map value, candidate number, box or offset out of range, [3] a prediction met more than 64 rows (its entries are
 *            incomplete).  The call zeroes counters and area_t.
 *   render : inst_map, type_map [H][W] = max over the kept masks covering a pixel of position + 1, of label + 1 (`convert_format` 'conic',
 *            WSI_coco.py:863-906); counters[2] is ORed as above and not cleared.
 * nuhtc_stitch_* enqueue and return; the nuhtc_op_stitch_* twins are the test entry points on raw arrays (boxes [B][K][5], labels [B][K],
 * counts [B], masks [B][K][tile][tile / 32]) and synchronise `stream`. */
typedef struct nuhtc_stitch_store {
  int32_t n_img, cand_cap, pool_cap, work_cap;
  int32_t* box;
  int32_t* area;
  float* score;
  int32_t* label;
  int64_t* key;
  int64_t* off;
  uint32_t* pool;
  int32_t* counters;
  int32_t* work;
} nuhtc_stitch_store;
int nuhtc_stitch_gather(nuhtc_engine* e, const nuhtc_dets* dets, int B, const int32_t* tile_meta, float fg_thr, float discard_offset,
                        const nuhtc_stitch_store* st, void* stream);
int nuhtc_stitch_pairs(nuhtc_engine* e, const nuhtc_stitch_store* st, int image, const int32_t* kept, int n_kept, const int32_t* gt_map, int H, int W,
                       int t_cap, int trip_cap, int32_t* area_t, int32_t* trips, int32_t* counters, void* stream);
int nuhtc_stitch_render(nuhtc_engine* e, const nuhtc_stitch_store* st, int image, const int32_t* kept, int n_kept, int H, int W, int32_t* inst_map,
                        int32_t* type_map, int32_t* counters, void* stream);
int nuhtc_op_stitch_gather(nuhtc_engine* e, const float* boxes, const int32_t* labels, const int32_t* counts, const uint32_t* masks,
                           const int32_t* tile_meta, int B, int K, int tile, int C, float fg_thr, float discard_offset, const nuhtc_stitch_store* st,
                           void* stream);
int nuhtc_op_stitch_pairs(nuhtc_engine* e, const nuhtc_stitch_store* st, int image, const int32_t* kept, int n_kept, const int32_t* gt_map, int H,
                          int W, int t_cap, int trip_cap, int32_t* area_t, int32_t* trips, int32_t* counters, void* stream);
int nuhtc_op_stitch_render(nuhtc_engine* e, const nuhtc_stitch_store* st, int image, const int32_t* kept, int n_kept, int H, int W, int32_t* inst_map,
                           int32_t* type_map, int32_t* counters, void* stream);

/* A HIP stream owned by the engine (valid after nuhtc_finalize) that a caller MAY run this engine on,
 * and should when it keeps several engines busy at once or raises GPU_MAX_HW_QUEUES above the runtime's default of 4: the stream
 * is created next to the engine's two internal side streams, which puts the three on different pipes of the command processor
 * (batches in flight).  Any other stream remains valid for every entry point.
 * LIFETIME: the engine's streams are POOLED for the life of the process, not destroyed: nuhtc_destroy hands the (own, side, side2)
 * triple back to a per-device pool and the next engine created on that device reuses the same handles (PyTorch's allocator touches a
 * block's allocation stream when it frees the block, long after the engine is gone).  A caller must therefore NOT use, wait on or
 * record into the handle after nuhtc_destroy: it may already belong to an unrelated engine. */
void* nuhtc_stream(nuhtc_engine* e);

/* Host-thread placement (v7; v8: original-mask bookkeeping, restore, explicit-root test entry).  Restricts the CALLING thread (threads
 * it creates later inherit the mask) to the CPUs of the NUMA node the device is attached to (/sys/bus/pci/devices/<bdf>/local_cpulist),
 * intersected with the mask the thread had BEFORE its first placement (kept per thread: a thread placed for a GPU of one socket can be
 * placed again for a GPU of the other).  The thread that submits an engine's work should run there: the command processor reads every
 * dispatch packet from host memory last written by the submitter, and from the other socket of a two-socket host that costs 1.4-2.9 us
 * per packet -- 0.3-0.4 ms per step of the back-to-back dense launches.  Returns 0 (bound, or already inside the
 * node), NUHTC_E_NOTFOUND when the host exposes no NUMA node for the device (nothing changed), NUHTC_E_STATE when the caller's own mask
 * has no CPU of that node (nothing changed: the caller chose otherwise), NUHTC_E_INVALID for a string that is not a PCI address (hex
 * digits, ':' and '.'), NUHTC_E_HIP for a bad device.  nuhtc_restore_host_thread gives the calling thread the mask it had before its first
 * placement (0 also when it was never placed).  No counterpart in the reference: its launcher (tools/test.py:100-103,179-183 -> mmcv
 * init_dist) leaves the placement of a rank to the operating system.  NEVER called implicitly by the library, and since v8 not by the
 * Python host either unless asked (`init_detector(..., bind_host=True)`, NUHTC_HOST_AFFINITY=1, or the entry points that own their
 * process: bench.py, tools/infer_wsi.py, tools/bench_wsi.py).  _pci takes the PCI address ("0000:75:00.0") instead of a device index;
 * _at is the test entry point: the same code against a sysfs tree under `sysfs_root` (the NUHTC_SYSFS_ROOT variable of v7 is gone). */
int nuhtc_bind_host_thread(int device);
int nuhtc_bind_host_thread_pci(const char* pci_bdf);
int nuhtc_bind_host_thread_at(const char* sysfs_root, const char* pci_bdf);
int nuhtc_restore_host_thread(void);

/* Text of the QuPath documents of a slide (v10).  The reference builds one dict per nucleus (tools/infer_wsi.py:550-585) and json.dump()s
 * the lists (:659-664); these write the same bytes from arrays.  Host memory only, no device work, callable from any thread.
 * head / mid / tail are NUL-terminated pieces of the feature template per class (the host cuts them out of json.dumps of one template
 * feature, so key order, separators and the classification block are json's own); numbers are written the way json.dumps writes a Python
 * int / float (float.__repr__: shortest round-trip digits, exponent form below 1e-4 and from 1e16 on).  Records are separated by ", ";
 * the enclosing brackets are the caller's.
 *   nuhtc_write_ring_features : record i = head | "[x, y], [x, y], ..." of ring i (verts[ring_off[i] .. ring_off[i+1]), int32 pairs) |
 *       mid[label[i]] | repr(score[i]) | tail[label[i]].  Fills feat_start[0..n]: record i is out[feat_start[i] .. feat_start[i+1] - 2).
 *       `threads` host threads share the records (0: the hardware's, at most 16).
 *   nuhtc_write_point_features: record i = head | repr(xy[2i]) ", " repr(xy[2i+1]) | mid[label[i]] | repr(score[i]) | tail[label[i]].
 *   nuhtc_join_features       : the records pick[0..n_pick) of a text written by nuhtc_write_ring_features (same feat_start convention),
 *       joined by ", " (the merged document: the records the cross-tile merge kept).
 * Each returns the number of bytes written.  When `out` is NULL or `cap` is below what the text needs, nothing is written and the
 * needed size is returned (exact for the ring and join writers, an upper bound for the point writer): call once to size.
 * Negative: NUHTC_E_INVALID (null argument, label outside [0, n_labels), n_labels > 64, decreasing offsets). */
int64_t nuhtc_write_ring_features(const int32_t* verts, const int64_t* ring_off, const int32_t* label, const double* score, int64_t n,
                                  const char* head, const char* const* mid, const char* const* tail, int32_t n_labels,
                                  char* out, int64_t cap, int64_t* feat_start, int32_t threads);
int64_t nuhtc_write_point_features(const double* xy, const int32_t* label, const double* score, int64_t n,
                                   const char* head, const char* const* mid, const char* const* tail, int32_t n_labels,
                                   char* out, int64_t cap);
int64_t nuhtc_join_features(const char* text, const int64_t* feat_start, const int64_t* pick, int64_t n_pick, char* out, int64_t cap,
                            int32_t threads);

/* Rings of a written GeoJSON back into mask crops (v10; tools/nuclei_merge.py on the GPU).  A ring tools/infer_wsi.py writes is the traced outer
 * border of one 8-connected pixel component (`cv2.findContours(...)[0][0]`, :51-58): vertices on pixel centres, edges along the 8 chain directions.
 * The pixels inside or on it are that component with its holes filled -- what nuhtc_merge_overlap derives from a detection's mask crop before it
 * measures polygons -- so the filled rings are a valid input of nuhtc_merge_overlap.  verts: int32 pairs, ring i = verts[ring_off[i] .. ring_off[i+1])
 * WITHOUT the repeated closing vertex.  Fills boxes[n][4] (x0, y0, x1, y1 exclusive), areas[n] (set pixels), word_off[n] and the bit-packed crops
 * (rows of (w + 31) / 32 words, pixel x in bit x & 31 of word x >> 5).  Returns the number of words; with `bits` NULL or `cap_words` too small only
 * boxes and word_off are filled and the needed size is returned.  NUHTC_E_INVALID: an empty ring, an edge that is not horizontal, vertical or diagonal
 * (not a traced ring: use the polygon path of the host), a ring wider or taller than 65535 pixels.  Host memory, any thread. */
int64_t nuhtc_fill_rings(const int32_t* verts, const int64_t* ring_off, int64_t n, int32_t* boxes, int32_t* areas, int64_t* word_off,
                         uint32_t* bits, int64_t cap_words, int32_t threads);

/* Tissue mask and tile selection of the whole-slide path on the device (csrc/tissue.hip; the host code they equal byte for byte is
 * nuhtc_amd/tissue.py).  Engine-free like nuhtc_merge_overlap: pointers are device memory of `device` unless marked HOST, each call allocates
 * and frees its own scratch, runs on `stream` and synchronises it before returning.  Integer arithmetic only. */
enum {
  NUHTC_TISSUE_ALL = 0,        /* image -> saturation -> median -> histogram -> threshold -> close */
  NUHTC_TISSUE_MEDIAN = 1,     /* image -> saturation -> median -> histogram (the first launch of an Otsu run; `med` is an output) */
  NUHTC_TISSUE_THRESHOLD = 2   /* `med` (an input) -> threshold -> close (the second launch, after the host's Otsu loop over `hist`) */
};
/* `segmentTissue` up to the binary image contours are found on.  img: uint8 pixels of >= 3 channels, pixel (y, x) channel c at
 * img[y * row_stride + x * pix_stride + c] (R, G, B first; pix_stride >= 3, row_stride >= W * pix_stride).  Steps: S of OpenCV's 8-bit RGB2HSV
 * (12-bit fixed point, 0 where v = 0); mthresh x mthresh median with replicated borders (mthresh odd, 1..15); binary = med > sthresh ?
 * min(sthresh_up, 255) : 0; close x close rectangular close anchored at close / 2 (0..16; 0 and 1 leave the image as it is; the border never wins).
 * Outputs [H][W] uint8: `binary` (not in stage MEDIAN), `sat` (nullable), `med` (nullable in stage ALL, required otherwise) and
 * hist[256] int64 = histogram of the median plane (stages ALL and MEDIAN; ignored in stage THRESHOLD).
 * NUHTC_E_INVALID (nothing written): a null required pointer, H or W < 1, H * W > 2^31 - 1, bad strides, mthresh even or outside 1..15,
 * close outside 0..16, sthresh_up < 0, an unknown stage. */
int nuhtc_tissue_mask(int device, const uint8_t* img, int H, int W, int64_t row_stride, int pix_stride, int stage, int mthresh, int sthresh,
                      int sthresh_up, int close, uint8_t* binary, uint8_t* sat, uint8_t* med, int64_t* hist, void* stream);
/* cv2.pointPolygonTest(contour, pt, False) of n integer points against one closed integer contour: out[i] = +1 inside, 0 on an edge or
 * vertex, -1 outside (on an edge wins, otherwise the parity of the edges a ray towards +x crosses, an edge counting when exactly one of its
 * ends has y <= py).  contour [n_vert][2], pts [n][2] int32 (x, y); exact for |coordinate| <= 2^30 (differences in 32 bits, products in
 * 64).  NUHTC_E_INVALID (nothing written): n_vert < 1, n < 0, a null pointer with n > 0. */
int nuhtc_points_polygon_test(int device, const int32_t* contour, int64_t n_vert, const int32_t* pts, int64_t n, int8_t* out, void* stream);
/* The grid of one tissue contour (`process_contour`): candidate (ix, iy) = (start_x + ix * step, start_y + iy * step), keep[ix * ny + iy] = 1
 * when the contour test passes and the point candidate + (hole_dx, hole_dy) is not strictly inside any hole.  The contour test takes
 * the n_off (1..4) points candidate + offsets[j]: with require_all = 0 one of them inside or on the contour passes ('four_pt'), with 1
 * all must ('four_pt_hard'); 'basic' / 'center' are n_off = 1.  contour NULL with n_vert = 0: no contour test (every candidate passes it).
 * holes: the vertices of all holes in one pool [n_pool][2], hole h = rows hole_off[h] .. hole_off[h + 1]; n_holes may be 0 (holes NULL).
 * HOST: offsets [n_off][2] int32, hole_off [n_holes + 1] int64.  Half-integer patch centres: the caller doubles every coordinate.
 * NUHTC_E_INVALID (nothing written): nx or ny < 0, nx * ny > 2^31 - 1, step < 1, a grid or tested point beyond +-2^30, n_off outside 1..4,
 * n_vert < 0, hole offsets that do not start at 0, decrease, leave a hole empty or run past n_pool, a null required pointer. */
int nuhtc_grid_in_contour(int device, int start_x, int start_y, int nx, int ny, int step, const int32_t* offsets, int n_off, int require_all,
                          const int32_t* contour, int64_t n_vert, const int32_t* holes, int64_t n_pool, const int64_t* hole_off, int n_holes,
                          int hole_dx, int hole_dy, uint8_t* keep, void* stream);

/* COCO RLE (pycocotools mask.encode / toBbox; tools/infer_wsi.py:600-627) of n bit-packed H x W masks, on the device (v12; csrc/rle.hip): what
 * cocoapi common/maskApi.c rleEncode + rleToString and rleToBbox compute, byte for byte (nuhtc_amd/cocomask.py encode / to_bbox are the host
 * twins).  Engine-free like nuhtc_merge_overlap; all pointers are device memory of `device`.  words_dev [n][H * W / 32]: rows of W / 32 words,
 * pixel x of a row in bit x & 31 of word x >> 5 -- the layout of nuhtc_dets.masks and of words_dev from nuhtc_export_kept.  n = n_max when
 * n_dev is NULL, else min(*n_dev, n_max) read on the device (n_dev[0] of nuhtc_export_kept chains without a host synchronisation); rows
 * past n are not touched.  Per mask i < n:
 *   len_dev [i]     = bytes of the compressed `counts` string (runs in column-major order over the whole frame, the first count the leading
 *                     run of zeros, from the fourth count on the difference from the count two places back, 5 bits per character + 48 with
 *                     continuation bit 0x20 and the sign-aware stop rule), or -1 when the mask has more than `run_cap` runs: that one writes
 *                     no bytes and a zero box, and the caller encodes it on the host (the convention of nuhtc_mask_contours).  run_cap costs
 *                     4 bytes of LDS per run and is taken as at most 15360;
 *   off_dev [i]     = byte offset of the string in bytes_dev = sum of max(len, 0) of the masks before it (placement is in mask order and a
 *                     function of the lengths alone); off_dev [n] = the total: when it exceeds pool_cap, the strings that would end past the
 *                     pool were not written (nuhtc_export_crops does the same with crop_off_dev) and no byte at or past pool_cap is touched;
 *   bbox_dev [i][4] = x, y, w, h of rleToBbox, including its quirk (a 1-run that ends in a later column than it began in spans the full
 *                     height: y = 0, h = H); zeros for an empty mask.
 * off_dev has n_max + 1 entries, bytes_dev pool_cap bytes (may be NULL with pool_cap = 0: lengths, offsets and boxes only).
 * NUHTC_E_INVALID (nothing enqueued): W % 32 != 0, H * W > 2^20, run_cap < 1, H or W < 1, n_max or pool_cap < 0, a null required pointer,
 * n_max * min(run_cap, H * W + 1) * 5 > 2^31 - 1 (the offsets are int32).  Enqueues three launches on `stream`; does not synchronise. */
int nuhtc_rle_encode(int device, const uint32_t* words_dev, const int32_t* n_dev, int n_max, int H, int W, int run_cap,
                     int32_t* len_dev, int32_t* off_dev, uint8_t* bytes_dev, int64_t pool_cap, int32_t* bbox_dev, void* stream);

/* Per-nucleus embeddings (csrc/nucfeat.hip): the FPN maps of a tile averaged under the final mask of a detection.  For a mask M (H x W bits,
 * A = set pixels) and level l (map x_l [H_l][W_l][64], stride s_l in mask pixels): w_l(i, j) = set pixels (y, x) with y / s_l == i and
 * x / s_l == j, e_l[c] = (sum over cells of w_l(i, j) * x_l[i][j][c]) / A, row = e_0 | e_1 | e_2 | e_3 (256 float32, the layout of
 * nuhtc_features, which is this mean under a mask of the whole image when the image fills the padded grid).  A == 0 gives a zero row.  The
 * sum of a (level, channel) is one fp32 fused multiply-add chain over the non-zero cells in row-major order, then one division: a function
 * of the mask and the maps alone, bitwise the same in any batch and on any call, and within (n + 3) 2^-24 sum(w |x|) / A of the exact value
 * (n = non-zero cells of the level).  nuhtc_config is unchanged (no ABI bump).  The reference has no counterpart on the device: its
 * tools/wsi_feat_extract.py / tools/nuclei_feat_extract.py build a per-nucleus table keyed by nuclei_id on the host.
 * nuhtc_nucleus_features runs after nuhtc_infer and nuhtc_export_kept of the same batch: idx_dev / n_dev are that export's (entry d = b *
 * max_per_img + r; n_dev[0] = kept detections), the masks are dets->masks, the maps the engine's x0..x3 at strides (4 << l) / scale_factor
 * mask pixels (NUHTC_E_INVALID unless scale_factor is 1, 2 or 4).  feat_dev [cap][256]: row d for d < min(n_dev[0], cap), in the export's
 * (tile, slot) order; later rows are not touched.  Enqueues one launch on `stream`; does not synchronise.
 * nuhtc_op_nucleus_pool is the test entry point on raw arrays: maps[l] device [B][h[l]][w[l]][64], strides[l] >= 1 with (H - 1) / strides[l] <
 * h[l] and (W - 1) / strides[l] < w[l] (h, w, strides and the pointer table are HOST arrays); masks device [B][K][H][(W + 31) / 32] (bit x & 31
 * of word x >> 5, bits from W on zero); pairs_dev device int32 [n_max][2] = (tile, slot), an entry outside [0, B) x [0, K) gives a zero row;
 * n = n_max when n_dev is NULL, else min(*n_dev, n_max); out device [n_max][256], rows from n on are not written.  Synchronises `stream`. */
int nuhtc_nucleus_features(nuhtc_engine* e, const nuhtc_dets* dets, int B, const int64_t* idx_dev, const int32_t* n_dev, int cap, float* feat_dev,
                           void* stream);
int nuhtc_op_nucleus_pool(nuhtc_engine* e, const float* const maps[4], const int32_t h[4], const int32_t w[4], const int32_t strides[4], int B,
                          const uint32_t* masks, int K, int H, int W, const int32_t* pairs_dev, const int32_t* n_dev, int n_max, float* out,
                          void* stream);

/* Per-nucleus morphometry and haematoxylin intensity (csrc/nucmorph.hip): INTEGERS ONLY, under the final mask M of a detection in its H x W
 * frame (a pixel outside the frame counts as 0).  raw row, 16 int64: A (set pixels); x0, y0, x1, y1 (bounding rectangle, x1 / y1 exclusive,
 * zeros when A == 0); Sx, Sy, Sxx, Syy, Sxy (sums of x, y, x^2, y^2, x y over the set pixels, tile pixels); E (pixel edges between a set
 * pixel and an unset or out-of-frame 4-neighbour); n1, n2, n3 (the perimeter classes of skimage.measure.perimeter(neighbourhood=4): on
 * the border image B = M & ~erode4(M), code = sum of B over the 3 x 3 neighbourhood weighted [[10,2,10],[2,1,2],[10,2,10]]; n1 counts
 * codes 5, 7, 15, 17, 25, 27, n2 counts 21, 33, n3 counts 13, 23); hull2 (twice the area of the convex hull of the corners of the set
 * pixels); 0 (reserved).  hist row, 256 int32: the histogram under M of h = clamp((k[0] L[R] + k[1] L[G] + k[2] L[B] + 2^27) >> 28, 0,
 * 255) in int64 with a floor shift, L = lut_dev (DEVICE int32 [256]), k (HOST int32 [3]) the red, green and blue coefficients, |k| < 2^20
 * and 0 <= L < 2^20 (nuhtc_amd/nucmorph.py stain_constants builds both).  Red is byte 0 of a pixel with NUHTC_CH_AS_IS and byte 2 with
 * NUHTC_CH_SWAP, as in nuhtc_infer.  Nothing is floating point: a nucleus gives the same bits in any batch and on any call, and
 * nuhtc_amd/nucmorph.py (morph_reference) restates every value in numpy and derives the named features from them on the host.
 * A == 0, or an entry outside the batch, gives a zero row in both outputs.  nuhtc_config is unchanged (no ABI bump).
 * nuhtc_nucleus_morph runs after nuhtc_infer and nuhtc_export_kept of the same batch: idx_dev / n_dev are that export's (entry d = b *
 * max_per_img + r; n_dev[0] = kept detections), the masks are dets->masks, tiles_dev [B][tile_h][tile_w][3] uint8 is the batch nuhtc_infer
 * was given (channel_mode too).  raw_dev [cap][16], hist_dev [cap][256]: row d for d < min(n_dev[0], cap), in the export's (tile, slot)
 * order; later rows are not touched.  NUHTC_E_INVALID: a null pointer, B outside 1 .. max_batch, cap outside 1 .. 2^24, a tile side above
 * 1024, an unknown channel_mode.  Enqueues one launch on `stream`; does not synchronise.
 * nuhtc_op_nucleus_morph is the test entry point on raw arrays: tiles device [B][H][W][3] uint8; masks device [B][K][H][(W + 31) / 32] (bit
 * x & 31 of word x >> 5; bits from W on are ignored); pairs_dev device int32 [n_max][2] = (tile, slot), an entry outside [0, B) x [0, K)
 * gives a zero row; n = n_max when n_dev is NULL, else min(*n_dev, n_max); raw [n_max][16], hist [n_max][256], rows from n on are not
 * written.  NUHTC_E_INVALID: a null pointer (n_dev excepted), B outside 1 .. 4096, K outside 1 .. 65536, H or W outside 1 .. 1024 (W need not
 * be a multiple of 32), n_max outside 1 .. 2^24, an unknown channel_mode.  Synchronises `stream`. */
int nuhtc_nucleus_morph(nuhtc_engine* e, const nuhtc_dets* dets, int B, const uint8_t* tiles_dev, int channel_mode, const int32_t* lut_dev,
                        const int32_t k[3], const int64_t* idx_dev, const int32_t* n_dev, int cap, int64_t* raw_dev, int32_t* hist_dev, void* stream);
int nuhtc_op_nucleus_morph(nuhtc_engine* e, const uint8_t* tiles, int channel_mode, const int32_t* lut_dev, const int32_t k[3], int B,
                           const uint32_t* masks, int K, int H, int W, const int32_t* pairs_dev, const int32_t* n_dev, int n_max,
                           int64_t* raw, int32_t* hist, void* stream);

/* Per-nucleus grey-level co-occurrence counts for the Haralick texture features (csrc/nuctex.hip): INTEGERS ONLY, under the final mask M
 * of a detection in its H x W frame.  The grey level of a pixel is q = h >> 4, h the haematoxylin value of nuhtc_nucleus_morph (the same
 * lut_dev, k and channel_mode): 16 levels.  tex row, int32 [2][136]: for the offsets (dy, dx) = (0, 1) and (1, 0), cell t(a, b) = 16 a -
 * a (a - 1) / 2 + (b - a) (the upper triangle in row-major order, a <= b) counts the unordered pixel pairs {p, p + offset} with both
 * pixels set in M and inside the frame whose levels are {a, b}.  The symmetric matrix of Haralick is G[a][b] = G[b][a] = the cell for a < b
 * and twice the cell on the diagonal.  Nothing is floating point: a nucleus gives the same bits in any batch and on any call, and
 * nuhtc_amd/nuctex.py (glcm_reference) restates the counts in numpy and derives the 26 named features from them on the host.  A mask
 * without a pair (empty, one pixel, a checkerboard), or an entry outside the batch, gives a zero row.  nuhtc_config is unchanged (no
 * ABI bump).
 * nuhtc_nucleus_texture runs after nuhtc_infer and nuhtc_export_kept of the same batch, with the arguments of nuhtc_nucleus_morph and
 * one output: tex_dev [cap][2][136], row d for d < min(n_dev[0], cap), in the export's (tile, slot) order; later rows are not touched.
 * NUHTC_E_INVALID: a null pointer, B outside 1 .. max_batch, cap outside 1 .. 2^24, a tile side above 1024, an unknown channel_mode.
 * Enqueues one launch on `stream`; does not synchronise.
 * nuhtc_op_nucleus_texture is the test entry point on raw arrays, with the arguments of nuhtc_op_nucleus_morph: tex [n_max][2][136], rows
 * from n = (n_dev ? min(*n_dev, n_max) : n_max) on are not written; a (tile, slot) outside [0, B) x [0, K) gives a zero row.
 * NUHTC_E_INVALID: a null pointer (n_dev excepted), B outside 1 .. 4096, K outside 1 .. 65536, H or W outside 1 .. 1024 (W need not be a
 * multiple of 32; a full 1024-px frame holds 1 047 552 pairs an offset, the largest count), n_max outside 1 .. 2^24, an unknown
 * channel_mode.  Synchronises `stream`. */
int nuhtc_nucleus_texture(nuhtc_engine* e, const nuhtc_dets* dets, int B, const uint8_t* tiles_dev, int channel_mode, const int32_t* lut_dev,
                          const int32_t k[3], const int64_t* idx_dev, const int32_t* n_dev, int cap, int32_t* tex_dev, void* stream);
int nuhtc_op_nucleus_texture(nuhtc_engine* e, const uint8_t* tiles, int channel_mode, const int32_t* lut_dev, const int32_t k[3], int B,
                             const uint32_t* masks, int K, int H, int W, const int32_t* pairs_dev, const int32_t* n_dev, int n_max,
                             int32_t* tex, void* stream);

/* Per-nucleus gradient integers for the Nucleus.Gradient.* features (csrc/nucgrad.hip): INTEGERS ONLY, under the mask M of a list entry in
 * its H x W frame.  h is the haematoxylin value of nuhtc_op_nucleus_morph (the same lut_dev, k and channel_mode); (gx2, gy2) is twice
 * numpy's np.gradient of h over the frame (central differences inside, twice the one-sided difference at the frame's edges, 0 along an
 * axis of one pixel; a neighbour outside M but inside the frame counts with its pixel); q = gx2^2 + gy2^2; m = isqrt(4 q), the magnitude
 * in quarter grey levels, 0 .. 1442.  grad row, 18 int64: A (set pixels); S1, S2, S3, S4 (the sums over M of m, m^2, m^3, m^4); mn, mx (the
 * least and greatest m); n_edge (the pixels of M with m >= edge_thr whose q is greater than q of the first and not less than q of the
 * second neighbour along the gradient's sector -- OpenCV's integer rule on |gx2|, |gy2| with tan 22.5 = 13573 / 2^15; a neighbour
 * outside the frame has q = 0); hist[10] (np.histogram(m, bins=10) in integers: bin min((m - mn) * 10 / (mx - mn), 9), bin 5 for all
 * when mx == mn).  nuhtc_amd/nucgrad.py (grad_reference) restates the row in numpy and derives the eight named features on the host.
 * An empty mask, or an entry outside the batch, gives a zero row.  nuhtc_config is unchanged (no ABI bump).
 * nuhtc_op_nucleus_gradient works on raw arrays, with the arguments, limits and error codes of nuhtc_op_nucleus_texture and a handle
 * that need not be finalized; in addition edge_thr (quarter grey levels) outside 1 .. 1442 gives NUHTC_E_INVALID.  grad [n_max][18], rows
 * from n = (n_dev ? min(*n_dev, n_max) : n_max) on are not written.  Synchronises `stream`.  There is no engine-route entry point: the
 * columns are produced from a written GeoJSON (nuhtc_amd/ringfeat.py). */
int nuhtc_op_nucleus_gradient(nuhtc_engine* e, const uint8_t* tiles, int channel_mode, const int32_t* lut_dev, const int32_t k[3], int B,
                              const uint32_t* masks, int K, int H, int W, const int32_t* pairs_dev, const int32_t* n_dev, int n_max,
                              int edge_thr, int64_t* grad, void* stream);

/* Per-nucleus shape integers for the Shape.HuMoments1..7 and Shape.FractalDimension features (csrc/nucshape.hip): INTEGERS ONLY, a pure
 * function of the mask M of a list entry in its H x W frame; no tile is read.  x is the column, y the row, both frame pixels.  shape row,
 * 24 int64: A (set pixels); x0, y0, x1, y1 (the bounding rectangle, x1 and y1 exclusive; all 0 when A == 0); Sx, Sy, Sxx, Sxy, Syy, Sxxx,
 * Sxxy, Sxyy, Syyy (the sums over M of x, y, x^2, x y, y^2, x^3, x^2 y, x y^2, y^3); N_1 .. N_10 (the box counts: with s = 2^j, the s x s
 * squares anchored at (x0, y0) -- box (i, k) covers x0 + i s <= x < x0 + (i + 1) s, y0 + k s <= y < y0 + (k + 1) s -- that hold at least
 * one set pixel and at least one unset position among their s^2 positions, a position outside the rectangle being unset whether or not
 * it lies inside the frame; all ten are written, sizes larger than the rectangle included).  nuhtc_amd/nucshape.py (shape_reference)
 * restates the row in numpy and derives the eight named features on the host.  An empty mask, or an entry outside the batch, gives a
 * zero row.  nuhtc_config is unchanged (no ABI bump).
 * nuhtc_op_nucleus_shape works on raw arrays, with the masks, the list, the limits and the error codes of nuhtc_op_nucleus_texture (B 1 ..
 * 4096, K 1 .. 65536, H and W 1 .. 1024, W need not be a multiple of 32 and bits from W on are ignored, n_max 1 .. 2^24; a null pointer
 * other than n_dev is NUHTC_E_INVALID) and a handle that need not be finalized.  shape [n_max][24], rows from n = (n_dev ? min(*n_dev,
 * n_max) : n_max) on are not written.  Synchronises `stream`.  There is no engine-route entry point: the op takes the engine's masks as
 * they are, and the columns are produced from a written GeoJSON (nuhtc_amd/ringfeat.py). */
int nuhtc_op_nucleus_shape(nuhtc_engine* e, int B, const uint32_t* masks, int K, int H, int W, const int32_t* pairs_dev, const int32_t* n_dev,
                           int n_max, int64_t* shape, void* stream);

/* Nuclei of a WRITTEN GeoJSON in front of the two measurement ops above (csrc/ringfeat.hip; nuhtc_amd/ringfeat.py, tools/wsi_feat_extract.py):
 * every nucleus gets a square frame of side S (32, 64, 128 or 256) whose pixel (0, 0) is the slide pixel origin[i] = (x, y); the masks and
 * frames below are what nuhtc_op_nucleus_morph / nuhtc_op_nucleus_texture read with B = n, K = 1, H = W = S and the pairs (i, 0).
 * Engine-free: every pointer is device memory of `device`; each call enqueues ONE launch on `stream` and does not synchronise.
 * nuhtc_config is unchanged (no ABI bump).
 * nuhtc_op_ring_fill: verts [nv][2] int32 slide pixels, ring i = the vertices [ring_off[i], ring_off[i + 1]) (ring_off int64 [n + 1]), the
 *   closing vertex NOT repeated; origin int32 [n][2].  masks [n][S][S / 32] uint32, bit x & 31 of word x >> 5: the pixels inside or on the
 *   ring, the set nuhtc_fill_rings defines (the border drawn by integer steps along every edge; outside = everything 4-reachable from
 *   beyond the frame without stepping on the border; the mask is everything else -- holes filled, a region a ring winds round twice
 *   inside), bit for bit.  status int32 [n]: 0 = filled; 1 = a vertex lies outside the frame; 2 = an edge is off the eight chain
 *   directions (not a traced ring), or the ring has no vertex or leaves [0, nv).  With a status other than 0 the mask is all zeros.
 *   A call writes the masks and statuses of its n rings and nothing else; the same input gives the same bits on every call.
 * nuhtc_op_frame_gather: block [bh][bw][3] uint8, a part of the slide whose pixel (0, 0) is the slide pixel (bx, by); the same origin
 *   array.  frames [n][S][S][3] uint8 (4-byte aligned): the frame at origin[i], 0 where it leaves the block.
 * NUHTC_E_INVALID, before anything is launched: a null pointer, S not one of the four sides, n outside 1 .. 4096 (the measurement ops'
 * limit on B), nv < 1, bh or bw outside 1 .. 32768. */
int nuhtc_op_ring_fill(int device, const int32_t* verts, int64_t nv, const int64_t* ring_off, const int32_t* origin, int n, int S,
                       uint32_t* masks, int32_t* status, void* stream);
int nuhtc_op_frame_gather(int device, const uint8_t* block, int bh, int bw, int bx, int by, const int32_t* origin, int n, int S,
                          uint8_t* frames, void* stream);

/* Per-nucleus Fourier-descriptor integers for the Shape.FSD1..6 features (csrc/nucfsd.hip): INTEGERS ONLY, a pure function of the ORDERED
 * RING of a nucleus -- the verts / ring_off of nuhtc_op_ring_fill above, read the same way; no mask, no frame, no tile.  Engine-free like
 * nuhtc_op_ring_fill: every pointer is device memory of `device`; the call enqueues ONE launch on `stream` and does not synchronise.
 * Edge e of a ring of n vertices runs from vertex e to vertex (e + 1) mod n; it is on the chain when dx == 0, dy == 0 or |dx| == |dy|
 * (max(|dx|, |dy|) axial unit steps of length 1, or diagonal ones of length sqrt 2; a zero-length edge contributes nothing).  a_e and b_e
 * are the axial and diagonal steps on the edges before e, A and B the totals: the perimeter is A + B sqrt 2.
 * rows [n][644] int32: status, A, B, n, then for each sample k = 0 .. 127 the five numbers x_e, y_e, d_e, a_e, b_e of the edge e(k) that
 *   holds the point at k / 128 of the perimeter: its start vertex, its Freeman code (0 = east, counter-clockwise on the screen, as
 *   nuhtc_mask_contours numbers them; 0 for a zero-length edge) and its start length.  e(k) is the largest e with a_e + b_e sqrt 2 <=
 *   (k / 128) (A + B sqrt 2), decided exactly in integers as the sign of p + q sqrt 2 with p = 128 a_e - k A, q = 128 b_e - k B (that of
 *   p and q where they agree, otherwise p^2 against 2 q^2 in int64): a sample on a vertex belongs to the edge that leaves it.
 * status [n] int32, also word 0 of the row: 0 = measured; 1 = degenerate (no vertex, or A + B == 0); 2 = not a traced ring (an edge off
 *   the chain, or ring_off leaves [0, nv] or decreases: nuhtc_op_ring_fill's 2); 3 = A + B > 2^24 steps (beyond it the int64 squares are
 *   not safe).  With a status other than 0 the other 643 words of the row are 0.  A ring may have any number of vertices.
 * nuhtc_amd/nucfsd.py (fsd_reference) restates the row in numpy and derives the six named features on the host.  A call writes the rows
 * and statuses of its n rings and nothing else; the same input gives the same bits on every call.  nuhtc_config is unchanged (no ABI
 * bump).  NUHTC_E_INVALID, before anything is launched: a null pointer, n outside 1 .. 4096, nv outside 1 .. 2^30. */
int nuhtc_op_ring_fsd(int device, const int32_t* verts, int64_t nv, const int64_t* ring_off, int n, int32_t* rows, int32_t* status, void* stream);

/* Cell graph of a slide (csrc/cellgraph.hip; nuhtc_amd/cellgraph.py has the definition and its brute-force int64 restatement `graph_reference`):
 * for every nucleus its k nearest nuclei within a radius, and the class census of that disc.  Not in the reference.  Engine-free like
 * nuhtc_merge_overlap: every pointer is device memory of `device`, the call allocates and frees its own scratch, runs on `stream` and
 * synchronises it before returning.  nuhtc_config is unchanged (no ABI bump).
 *   points [n][2] int32: node positions in HALF pixels, px = rint(x0 + x1), py = rint(y0 + y1) of the record's box (half to even): twice the
 *     centre <id>_point.geojson writes.  |p| < 2^27.  labels [n] int32.  0 <= n <= 2^28.
 *   r: the radius in half pixels (2 x the radius in pixels), 1 .. 16384.  k: 1 .. 32.  num_classes C: 1 .. 14.
 *   x_min, y_min, x_max, y_max: the bounding box of the points (inclusive), computed by the caller on the host (the grid geometry is derived
 *     from it on the host: cell side = the smallest multiple of r whose grid over the box has at most 2^22 cells; ignored when n == 0).
 * All arithmetic is integer.  The neighbours of i are the j != i with d2(i, j) = dx * dx + dy * dy <= r * r (the radius is inclusive;
 * coincident points, d2 == 0, are neighbours of each other), ordered by (d2, j) ascending and cut to the first k:
 *   neighbors   [n][k] int32: the row index j of each neighbour, -1 past the end of the list
 *   d2          [n][k] int32: its squared distance in half pixels^2, -1 past the end of the list
 *   class_count [n][C] int32: how many j != i within the radius have label c -- all of them, not only the first k; a label outside
 *                             [0, C) is a neighbour like any other and is counted in no class.
 * The result is a pure function of the input: bitwise the same on every call.  n == 0 returns NUHTC_OK and touches nothing; n == 1 gives
 * -1 in every slot and zero counts.  NUHTC_E_INVALID, before anything is launched and with the outputs untouched: k, r, num_classes or n
 * out of range, a null pointer with n > 0, a bounding box that is empty or reaches +-2^27 (so: any coordinate out of range).
 * NUHTC_E_INVALID after the binning, the outputs still untouched: a point lies outside the stated bounding box. */
int nuhtc_cell_graph(int device, const int32_t* points, const int32_t* labels, int64_t n, int num_classes, int r, int k, int x_min, int y_min,
                     int x_max, int y_max, int32_t* neighbors, int32_t* d2, int32_t* class_count, void* stream);

/* Spatial statistics of a slide (csrc/cellspatial.hip; nuhtc_amd/spatial.py has the definition and its brute-force int64 restatement
 * `spatial_reference`): pair-distance histograms by class pair and the nearest nucleus of every class for every nucleus.  Not in the
 * reference.  Engine-free like nuhtc_cell_graph: points, labels and the three outputs are device memory of `device`, the call allocates and
 * frees its own scratch, runs on `stream` and synchronises it before returning.  nuhtc_config is unchanged (no ABI bump).
 *   points [n][2] int32: node positions in HALF pixels (as for nuhtc_cell_graph), |p| < 2^27.  labels [n] int32.  0 <= n <= 2^28.
 *   num_classes C: 1 .. 14.  edges [num_bins] int32 in HOST memory: the bin edges e_1 < .. < e_B in half pixels, strictly increasing,
 *     1 <= B <= 32, e_1 >= 1, e_B <= 16384.
 *   x_min, y_min, x_max, y_max: the bounding box of the points (inclusive), computed by the caller on the host (cell side = the smallest
 *     multiple of e_B whose grid over the box has at most 2^18 cells; ignored when n == 0).
 * All arithmetic is integer.  The bin of an ordered pair (i, j), i != j, d2 = dx * dx + dy * dy, is the smallest t with d2 <= e_t^2 (edges
 * inclusive; no bin beyond e_B; coincident points fall in bin 0):
 *   pair_hist [C][C][B] int64: the ordered pairs with label_i = a, label_j = b in bin t, not cumulative; a label outside [0, C) is counted in
 *                              no row and no column.
 *   nn_d2     [n][C] int32:    the least d2 from i to a j != i of class c with d2 <= e_B^2, -1 for none; written for every i.
 *   class_n   [C] int64:       the points of each class.
 * The call zeroes pair_hist and class_n itself.  The result is a pure function of the input: bitwise the same on every call.  n == 0
 * zeroes pair_hist and class_n and returns NUHTC_OK; n == 1 gives nn_d2 = -1.  NUHTC_E_INVALID, before anything is launched and with the
 * outputs untouched: B, the edges, num_classes or n out of range, a null pointer, a bounding box that is empty or reaches +-2^27 (so: any
 * coordinate out of range).  NUHTC_E_INVALID after the binning, the outputs still untouched: a point lies outside the stated bounding box. */
int nuhtc_cell_spatial(int device, const int32_t* points, const int32_t* labels, int64_t n, int num_classes, const int32_t* edges, int num_bins,
                       int x_min, int y_min, int x_max, int y_max, int64_t* pair_hist, int32_t* nn_d2, int64_t* class_n, void* stream);

/* Nucleus clusters of a slide (csrc/cellcluster.hip; nuhtc_amd/clusters.py has the definition and its brute-force int64 restatement
 * `cluster_reference`): DBSCAN with a deterministic choice for border points.  Not in the reference.  Engine-free like the cell graph's
 * call: points, labels and the eight outputs are device memory of `device`, the call allocates and frees its own scratch, runs on `stream`
 * and synchronises it before returning.  nuhtc_config is unchanged (no ABI bump).
 *   points [n][2] int32: node positions in HALF pixels (as for the cell graph), |p| < 2^27.  labels [n] int32.  0 <= n <= 2^24: the dense
 *     numbering scans one flag per point in at most 1024 chunks of 16384, and no slide has that many nuclei.
 *   num_classes C: 1 .. 14.  r: the radius in half pixels, 1 .. 16384.  min_pts >= 1.  by_class: 0 or 1.
 *   x_min, y_min, x_max, y_max: the bounding box of the points (inclusive), computed by the caller on the host (cell side = the smallest
 *     multiple of r whose grid over the box has at most 2^22 cells; ignored when n == 0).
 * All arithmetic is integer.  adj(i, j): dx * dx + dy * dy <= r * r (inclusive; adj(i, i) holds; coincident points are adjacent) and, with
 * by_class, labels[i] == labels[j] (plain equality, also for labels outside [0, C)).  degree[i] = the number of j with adj(i, j), i among
 * them; i is a core point when degree[i] >= min_pts.  Clusters are the connected components of adj among core points, the root of a
 * cluster is its smallest core row, and clusters are numbered 0 .. m - 1 by ascending root.  A non-core point with an adjacent core point
 * (a border point) joins the cluster of the adjacent core point with the smallest (d2, j); every other point is noise.
 *   cluster [n] int32: the cluster of every point, -1 for noise.  core [n] uint8: 1 for a core point.  degree [n] int32.
 *   Per cluster, n rows of capacity each, the first m written and the rest untouched:
 *   size [.] int32, n_core [.] int32, class_count [.][C] int32 (a label outside [0, C) is counted in no class),
 *   sum_xy [.][2] int64 (half pixels), bbox [.][4] int32 (x_min, y_min, x_max, y_max, half pixels).
 *   m: HOST memory, the number of clusters, written on success only.
 * The result is a pure function of the input: bitwise the same on every call.  n == 0 sets m = 0, launches nothing and returns NUHTC_OK.
 * NUHTC_E_INVALID, before anything is launched and with the outputs untouched: n, num_classes, r, min_pts or by_class out of range, a null
 * pointer (m always, the others with n > 0), a bounding box that is empty or reaches +-2^27 (so: any coordinate out of range).
 * NUHTC_E_INVALID after the binning, the outputs still untouched: a point lies outside the stated bounding box. */
int nuhtc_cell_clusters(int device, const int32_t* points, const int32_t* labels, int64_t n, int num_classes, int r, int min_pts, int by_class,
                        int x_min, int y_min, int x_max, int y_max, int32_t* cluster, uint8_t* core, int32_t* degree, int32_t* size,
                        int32_t* n_core, int32_t* class_count, int64_t* sum_xy, int32_t* bbox, int64_t* m, void* stream);

/* Minimum spanning forest of a slide's nuclei (csrc/cellmst.hip; nuhtc_amd/mst.py holds the definition and the brute-force restatement
 * `mst_reference`): the minimum spanning tree descriptors of a tissue section, and the single-linkage dendrogram of the slide up to the
 * radius.  Not in the reference.  Engine-free like the clusters' call: points, labels and the three outputs are device memory of `device`,
 * the call allocates and frees its own scratch, runs on `stream` and synchronises it (once per Boruvka round and once at the end) before
 * returning.  nuhtc_config is unchanged (no ABI bump).
 *   points [n][2] int32: node positions in HALF pixels (as for the cell graph), |p| < 2^27.  labels [n] int32.  0 <= n <= 2^24: a row takes
 *     24 bits of the 64-bit pick key, and the edge order scans one count per point in at most 1024 chunks of 16384.
 *   num_classes C: 1 .. 14 (checked; the labels are only compared with each other).  r: the radius in half pixels, 1 .. 16384.
 *   by_class: 0 or 1.  x_min, y_min, x_max, y_max: the bounding box of the points (inclusive), computed by the caller on the host (cell
 *     side = the smallest multiple of r whose grid over the box has at most 2^22 cells; ignored when n == 0).
 * All arithmetic is integer.  An EDGE is an unordered pair i < j with dx * dx + dy * dy <= r * r (inclusive; coincident points are joined
 * with d2 = 0) and, with by_class, labels[i] == labels[j] (plain equality, also for labels outside [0, C)).  Edges are ordered by the key
 * (d2, i, j), lexicographically: a strict total order, so the minimum spanning forest of the edge set is unique -- what Kruskal's
 * algorithm returns on the edges in ascending key order.  That forest is the result.
 *   edges [n][2] int32 and edge_d2 [n] int32 (n rows of capacity, the first m written and the rest untouched): the forest's edges (i, j),
 *     i < j, in ascending (i, j) order, and their squared lengths in half pixels.
 *   tree [n] int32: the tree of every point, numbered 0 .. T - 1 by ascending smallest row; an isolated point is a tree of size 1.
 *   m, trees, rounds: HOST memory, written on success only: the edges (m = n - T), T, and the Boruvka rounds that added an edge.
 * The result is a pure function of the input: bitwise the same on every call.  n == 0 sets m = trees = rounds = 0, launches nothing and
 * returns NUHTC_OK.
 * NUHTC_E_INVALID, before anything is launched and with the outputs untouched: n, num_classes, r or by_class out of range, a null pointer
 * (m, trees, rounds always, the others with n > 0), a bounding box that is empty or reaches +-2^27 (so: any coordinate out of range).
 * NUHTC_E_INVALID after the binning, the outputs still untouched: a point lies outside the stated bounding box.
 * NUHTC_E_HIP: a HIP call failed, or round 25 still added edges (impossible for n <= 2^24: every round halves the components). */
int nuhtc_cell_mst(int device, const int32_t* points, const int32_t* labels, int64_t n, int num_classes, int r, int by_class,
                   int x_min, int y_min, int x_max, int y_max, int32_t* edges, int32_t* edge_d2, int32_t* tree,
                   int64_t* m, int64_t* trees, int64_t* rounds, void* stream);

/* Proximity graphs of a slide's nuclei (csrc/cellprox.hip; nuhtc_amd/proximity.py holds the definition and the brute-force restatement
 * `proximity_reference`): the Gabriel graph and the relative neighbourhood graph (RNG), the parameter-free "who touches whom" relations,
 * both subgraphs of the Delaunay graph and both supergraphs of the minimum spanning forest at the same radius.  Not in the reference.
 * Engine-free like the forest's call: points, labels and the four outputs are device memory of `device`, the call allocates and frees
 * its own scratch, runs on `stream` and synchronises it (once after the count, once at the end) before returning.  nuhtc_config is
 * unchanged (no ABI bump).
 *   points [n][2] int32: node positions in HALF pixels, |p| < 2^27.  labels [n] int32.  0 <= n <= 2^24 (one count per point is scanned in
 *     at most 1024 chunks of 16384).  num_classes C: 1 .. 14 (checked; the labels are only compared with each other).  r: the radius in
 *     half pixels, 1 .. 16384.  by_class: 0 or 1.  edge_cap: the rows of capacity of the three edge arrays, 0 .. 2^31 - 1.
 *   x_min, y_min, x_max, y_max: the bounding box of the points (inclusive), computed by the caller on the host (ignored when n == 0).
 * All arithmetic is integer; write d2(a, b) for the squared distance.  A CANDIDATE is an unordered pair i < j with d2(i, j) <= r * r
 * (inclusive) and, with by_class, labels[i] == labels[j] (plain equality, also for labels outside [0, C)).  A WITNESS is any other row k,
 * with by_class of the same label.  The candidate is a GABRIEL edge when no witness has d2(i, k) + d2(j, k) < d2(i, j), and an RNG edge
 * when no witness has max(d2(i, k), d2(j, k)) < d2(i, j): both strict, so a witness on the circle or at equal distance does not block,
 * and coincident points are joined (d2 = 0, rng = 1).  Every RNG edge is a Gabriel edge.
 *   edges [edge_cap][2] int32, edge_d2 [edge_cap] int32, edge_rng [edge_cap] uint8: the Gabriel edges (i, j), i < j, in ascending (i, j)
 *     order, their squared lengths, and 1 where the edge is an RNG edge too.  Written ONLY when m <= edge_cap (the first m rows, the rest
 *     untouched); with m > edge_cap the three arrays are untouched, the call still returns NUHTC_OK, and the caller calls again with
 *     edge_cap = m.  m is not bounded by a multiple of n: k coincident points are a clique of k (k - 1) / 2 edges.
 *   degree [n][2] int32: the Gabriel and the RNG edges at every row, always written.
 *   m, m_rng: HOST memory, written on success only: the Gabriel edges and how many of them are RNG edges.
 * The result is a pure function of the input: bitwise the same on every call.  n == 0 sets m = m_rng = 0, launches nothing and returns
 * NUHTC_OK.
 * NUHTC_E_INVALID, before anything is launched and with the outputs untouched: n, num_classes, r, by_class or edge_cap out of range, a
 * null pointer (m, m_rng always, the others with n > 0), a bounding box that is empty or reaches +-2^27.
 * NUHTC_E_INVALID after the binning, the outputs still untouched: a point lies outside the stated bounding box. */
int nuhtc_cell_proximity(int device, const int32_t* points, const int32_t* labels, int64_t n, int num_classes, int r, int by_class,
                         int64_t edge_cap, int x_min, int y_min, int x_max, int y_max, int32_t* edges, int32_t* edge_d2,
                         uint8_t* edge_rng, int32_t* degree, int64_t* m, int64_t* m_rng, void* stream);

/* Nucleus density maps of a slide (csrc/celldensity.hip; nuhtc_amd/density.py holds the definition and the brute-force restatement
 * `density_reference`): class-wise kernel rasters of the nucleus centres on a lattice anchored at the slide's origin -- "where on the slide".
 * Not in the reference.  Engine-free like the forest's and the proximity call: points, labels and the two outputs are device memory of
 * `device`, the call allocates and frees its own scratch, runs on `stream` and synchronises it before returning.  nuhtc_config is unchanged
 * (no ABI bump).
 *   points [n][2] int32: node positions in HALF pixels, |p| < 2^27.  labels [n] int32.  0 <= n <= 2^24.  num_classes C: 1 .. 14.
 *   h: the bandwidth in half pixels, 1 .. 16384.  s: the pitch in half pixels, 1 .. 2^20.
 *   gx0, gy0, W, H: the window in lattice units; W, H >= 1, W * H <= 2^24, and every site coordinate |g * s| < 2^28 (checked in 64 bits).
 *     Any window is accepted: a sub-window, one partly off the points, or one nowhere near them (all zeros).
 *   x_min, y_min, x_max, y_max: the bounding box of the points (inclusive), computed by the caller on the host (ignored when n == 0).
 * Site (u, v) lies at q = ((gx0 + u) * s, (gy0 + v) * s): the lattice is anchored at the slide's origin, not at the points, so maps of
 * different runs and radii align.  For every class c in 0 .. C - 1 and every site:
 *   count [C][H][W] int32: the points i with labels[i] == c and d2(q, p_i) <= h * h (the radius is inclusive).
 *   weight [C][H][W] int64: the sum over those points of h * h - d2(q, p_i) (the Epanechnikov kernel, un-normalised).
 * A point with a label outside 0 .. C - 1 is counted nowhere; a point exactly at distance h adds 1 to count and 0 to weight.  All
 * arithmetic is integer: |q - p| < 2^28 + 2^27 is an exact int32, the box test against h comes before the products, a term is at most 2^28
 * and a weight below 2^52.  Both outputs are always fully written on success, zeros included; with n == 0 both are cleared and nothing
 * else runs.  The result is a pure function of the input: bitwise the same on every call.
 * NUHTC_E_INVALID, before anything is launched and with the outputs untouched: n, num_classes, h, s or the window out of range, a null
 * pointer (count, weight always, the others with n > 0), with n > 0 a bounding box that is empty or reaches +-2^27.
 * NUHTC_E_INVALID after the binning, the outputs still untouched: a point lies outside the stated bounding box. */
int nuhtc_cell_density(int device, const int32_t* points, const int32_t* labels, int64_t n, int num_classes, int h, int s, int gx0, int gy0,
                       int W, int H, int x_min, int y_min, int x_max, int y_max, int32_t* count, int64_t* weight, void* stream);

/* Nucleus territories of a slide (csrc/cellterritory.hip; nuhtc_amd/territory.py holds the definition and the brute-force restatement
 * `territory_reference`): the nearest-nucleus raster on the lattice of the density maps -- which nucleus, and so which class, each
 * piece of the plane belongs to (the Voronoi family in raster form).  Not in the reference.  Engine-free like the density call: every
 * array is device memory of `device`, the call allocates and frees its own scratch, runs on `stream` and synchronises it before
 * returning.  nuhtc_config is unchanged (no ABI bump).
 *   points [n][2] int32: node positions in HALF pixels, |p| < 2^27.  labels [n] int32.  0 <= n <= 2^24.  num_classes C: 1 .. 14.
 *   reach R: half pixels, 1 .. 16384.  s: the pitch in half pixels, 1 .. 2^20.
 *   gx0, gy0, W, H: the window in lattice units; W, H >= 1, W * H <= 2^28, and every site coordinate |g * s| < 2^28 (checked in 64 bits).
 *   x_min, y_min, x_max, y_max: the bounding box of the points (inclusive), computed by the caller on the host (ignored when n == 0).
 * Site (u, v) lies at q = ((gx0 + u) * s, (gy0 + v) * s).  The rows with a label in 0 .. C - 1 compete; any other row owns nothing and
 * blocks nothing.
 *   owner [H][W] int32: the competitor i that minimises (d2(q, p_i), i) among those with d2 <= R * R (inclusive; a tie goes to the
 *     smaller row), or -1.  It does not depend on the window: a sub-window is a slice of the full map.
 *   nearest_d2 [H][W] int32: that d2, or -1.
 * The tallies are over the window (a site's 4-neighbours are those inside it) and are zeroed by the call:
 *   area [n] int32: the sites a row owns.  border [n] int32: its sites with a 4-neighbour whose owner differs (-1 differs).
 *   open [n] int32, 0 / 1: the row owns a site on the window's outer row or column, or one with a 4-neighbour nobody owns.
 *   contact [C][C] int64: over every ordered pair (site, 4-neighbour) with owners i != j, both >= 0, one count at [label_i][label_j].
 *   class_sites [C] int64: the sites owned by each class.  free_sites [1] int64: the sites nobody owns.
 * All arithmetic is integer: q - p is an exact int32, the box test against R comes before the products, d2 <= 2^28, and (d2, row) is one
 * 64-bit key.  With n == 0 the maps are -1, the tables zero and free_sites = W * H.  A pure function of the input: bitwise the same on
 * every call.
 * NUHTC_E_INVALID, before anything is launched and with the outputs untouched: n, num_classes, reach, s or the window out of range, a
 * null pointer (the maps and the three tables always, the others with n > 0), with n > 0 a bounding box that is empty or reaches +-2^27.
 * NUHTC_E_INVALID after the binning, the outputs still untouched: a point lies outside the stated bounding box. */
int nuhtc_cell_territory(int device, const int32_t* points, const int32_t* labels, int64_t n, int num_classes, int reach, int s, int gx0,
                         int gy0, int W, int H, int x_min, int y_min, int x_max, int y_max, int32_t* owner, int32_t* nearest_d2, int32_t* area,
                         int32_t* border, int32_t* open, int64_t* contact, int64_t* class_sites, int64_t* free_sites, void* stream);

/* Territory adjacency of a slide (csrc/celladjacency.hip; nuhtc_amd/adjacency.py holds the definition and the numpy restatement
 * `adjacency_reference`): the discrete Delaunay graph of the nucleus centres, read off the owner map nuhtc_cell_territory wrote -- which
 * nuclei are neighbours and how long their common border is.  Not in the reference.  Engine-free like the territory call: the map and the
 * three outputs are device memory of `device`, the call allocates and frees its own scratch, runs on `stream` and synchronises it (once
 * after the count, once at the end) before returning.  It takes no points and no labels: the map holds everything.  nuhtc_config is
 * unchanged (no ABI bump).
 *   owner [H][W] int32: every entry in -1 .. n - 1 (-1: nobody's).  W, H >= 1, W * H <= 2^28.  0 <= n <= 2^24.
 *   edge_cap: the rows of capacity of `edges` and `shared`, 0 .. 2^31 - 1.
 * A SITE PAIR is an unordered pair of 4-adjacent sites inside the window, counted once.  {i, j} with i < j is an EDGE when some site pair
 * has the owners i and j, both >= 0; a site nobody owns makes no edge, and two territories that meet only diagonally are not adjacent.
 *   edges [edge_cap][2] int32: the edges (i, j), i < j, in ascending (i, j) order.
 *   shared [edge_cap] int32: the site pairs with the owners {i, j} -- the length of the common border in lattice steps, at most 2^29.
 *     Both are written ONLY when m <= edge_cap (the first m rows, the rest untouched); with m > edge_cap both are untouched, the call still
 *     returns NUHTC_OK, and the caller calls again with edge_cap >= m.
 *   degree [n] int32: the distinct neighbours of every row, always written.
 *   m: HOST memory, written on success only: the number of edges.
 * Integer adds and a rank: a pure function of the map, bitwise the same on every call.  With n == 0 (every owner -1) m = 0.
 * NUHTC_E_INVALID, before anything is launched and with the outputs untouched: W, H, n or edge_cap out of range, a null pointer (owner and
 * m always, degree with n > 0, edges and shared with edge_cap > 0).
 * NUHTC_E_INVALID after the first pass over the map, the outputs still untouched: an owner outside -1 .. n - 1 (no owner is used as an
 * index before that pass has ended).
 * NUHTC_E_HIP: a HIP call failed; an allocation that fails does so before any output is written. */
int nuhtc_territory_adjacency(int device, const int32_t* owner, int W, int H, int64_t n, int64_t edge_cap, int32_t* edges, int32_t* shared,
                              int32_t* degree, int64_t* m, void* stream);

/* The alpha complex of a slide's nuclei (csrc/cellalpha.hip; nuhtc_amd/alphacomplex.py holds the definition and the brute-force
 * restatement `alpha_reference`): the exact Delaunay edges within a radius -- the continuous statement of what nuhtc_territory_adjacency
 * reads off a lattice, and a supergraph of the Gabriel graph of nuhtc_cell_proximity at radius 2 r.  Not in the reference.  Engine-free
 * like the proximity call, with its argument order and its capacity protocol: points, labels and the five outputs are device memory of
 * `device`, the call allocates and frees its own scratch, runs on `stream` and synchronises it (once after the count, once at the end)
 * before returning.  nuhtc_config is unchanged (no ABI bump).
 *   points [n][2] int32: node positions in HALF pixels, |p| < 2^27.  labels [n] int32.  0 <= n <= 2^24.  num_classes C: 1 .. 14 (checked;
 *     the labels are only compared with each other).  r: the radius in half pixels, 1 .. 512; D = 2 r is the diameter.  by_class: 0 or 1.
 *     edge_cap: the rows of capacity of the four edge arrays, 0 .. 2^31 - 1.
 *   x_min, y_min, x_max, y_max: the bounding box of the points (inclusive), computed by the caller on the host (ignored when n == 0).
 * A CANDIDATE is an unordered pair i < j with d2(i, j) <= D * D (inclusive) and, with by_class, labels[i] == labels[j] (plain equality).
 * A WITNESS is any other row k, with by_class of the same label.  The candidate is an EDGE when some disc of radius <= r has both ends on
 * its boundary and no witness strictly inside: with q = p_j - p_i the discs through both ends have the centres (q + t q_perp) / 2, t real,
 * radius <= r is t^2 <= T^2 = (D^2 - d2) / d2, and a witness at rho = p_k - p_i with s = q x rho and m = rho . (rho - q) allows
 * t <= m / s (s > 0), t >= m / s (s < 0), blocks the pair (s == 0, m < 0) or does not bind.  hi is the smallest upper bound, lo the
 * largest lower one (either may be open); the pair is an edge when it is not blocked, hi >= -T, lo <= T and lo <= hi, all inclusive, so
 * four cocircular points keep both diagonals.  Every decision is a comparison of two rationals in int64.
 *   edges [edge_cap][2] int32: the edges (i, j), i < j, in ascending (i, j) order.  edge_d2 [edge_cap] int32: their squared lengths.
 *   apex [edge_cap][2] int32: [0] the smallest row that attains hi when hi <= T, [1] the smallest that attains lo when lo >= -T, else -1:
 *     the third corner of a triangle with an empty circumcircle of radius <= r on that side of the edge.
 *   edge_gabriel [edge_cap] uint8: 1 where no witness has m < 0 (none strictly inside the disc with diameter ij).
 *     All four are written ONLY when m <= edge_cap (the first m rows, the rest untouched); with m > edge_cap they are untouched, the call
 *     still returns NUHTC_OK, and the caller calls again with edge_cap >= m.  m is not bounded by a multiple of n: k coincident points are
 *     a clique of k (k - 1) / 2 edges (d2 = 0, both apexes -1, Gabriel).
 *   degree [n][2] int32: the edges and the Gabriel edges at every row, always written.
 *   m, m_gabriel: HOST memory, written on success only.
 * The result is a pure function of the input: bitwise the same on every call.  n == 0 sets m = m_gabriel = 0, launches nothing and
 * returns NUHTC_OK.
 * NUHTC_E_INVALID, before anything is launched and with the outputs untouched: n, num_classes, r, by_class or edge_cap out of range, a
 * null pointer (m, m_gabriel always, the others with n > 0), a bounding box that is empty or reaches +-2^27.
 * NUHTC_E_INVALID after the binning, the outputs still untouched: a point lies outside the stated bounding box. */
int nuhtc_cell_alpha(int device, const int32_t* points, const int32_t* labels, int64_t n, int num_classes, int r, int by_class,
                     int64_t edge_cap, int x_min, int y_min, int x_max, int y_max, int32_t* edges, int32_t* edge_d2, int32_t* apex,
                     uint8_t* edge_gabriel, int32_t* degree, int64_t* m, int64_t* m_gabriel, void* stream);

/* The alpha-shape outline (csrc/celloutline.hip; nuhtc_amd/outline.py holds the definition and the plain walk `outline_reference`): the
 * rings and the components of the alpha complex that nuhtc_cell_alpha left on the device.  Not in the reference.  Engine-free: every
 * pointer but `counts` is device memory of `device`, the call allocates and frees its own scratch, runs on `stream` and synchronises it
 * (once after the outline edges are counted, once at the end) before returning.  nuhtc_config is unchanged (no ABI bump).
 *   points [n][2] int32, labels [n] int32: as given to nuhtc_cell_alpha; 0 <= n <= 2^24.  by_class: 0 or 1, as given there.
 *   edges [m][2], edge_d2 [m], apex [m][2] int32: the first m rows of its outputs; 0 <= m <= 2^24 (the scans over the edges).
 * A row is a REPRESENTATIVE unless it is the larger end of an edge with edge_d2 == 0; an edge between two representatives is KEPT.  A kept
 * edge with exactly one apex gives one HALF-EDGE with the apex on its left (i -> j when apex[e][0] >= 0, else j -> i) and the id e.  The
 * successor of u -> v is the half-edge v -> w met first when turning clockwise from v -> u, decided by signs of cross and dot products in
 * int64.  The RINGS are the cycles of that map: led by their smallest id, written from the leader's tail onward, ordered by leader.  Two
 * kept edges with an apex are joined when they are sides of one triangle (i, j, apex); a COMPONENT is numbered by the rank of its
 * smallest edge index.
 *   ring_vertex [m] int32: the rows in ring order, rings concatenated (the first h written).  ring_start [m + 1] int32: where each ring
 *     begins (the first R + 1 written; ring_start[R] == h).  ring_area2 [m] int64: the shoelace sum of each ring in half pixels squared,
 *     relative to its first vertex: positive for an outer ring, negative for a hole (the first R written).  component_of_ring [m] int32
 *     (R written).  component [n] int32: the smallest component among the apexed kept edges at a representative, -1 for a row in no
 *     triangle; any other row has its representative's value (all n written).  component_label [m] int32: with by_class the label all
 *     rows of the component share, else -1 (the first K written).
 *   counts: HOST memory, int64 [3] = h, R, K, written on success only.
 * The result is a pure function of the input: bitwise the same on every call.  m == 0 writes ring_start[0] = 0 and component = -1.
 * NUHTC_E_INVALID, before anything is launched and with the outputs untouched: n, m or by_class out of range, a null pointer (counts and
 * ring_start always; points, labels and component with n > 0; the others with m > 0), m > 0 with n == 0.
 * NUHTC_E_INVALID after the first kernels, the outputs still untouched: an edge that is not (i, j) with 0 <= i < j < n or does not come
 * behind the edge in front of it, an apex outside -1 .. n - 1, an apex that is not strictly on its side of the edge (apex[e][0] left of
 * i -> j, apex[e][1] right), a point of an edge or an apex outside |p| < 2^27.
 * An edge list that passes these checks and is no alpha complex is worked off without any access outside the tables; its rings mean
 * nothing. */
int nuhtc_alpha_outline(int device, const int32_t* points, const int32_t* labels, int64_t n, int by_class, const int32_t* edges,
                        const int32_t* edge_d2, const int32_t* apex, int64_t m, int32_t* ring_vertex, int32_t* ring_start,
                        int64_t* ring_area2, int32_t* component_of_ring, int32_t* component, int32_t* component_label, int64_t* counts,
                        void* stream);

/* Nuclei by region (csrc/cellregion.hip; nuhtc_amd/regions.py holds the definition and the brute-force restatement `regions_reference`):
 * an exact point-in-polygon census of the nucleus centres against annotated regions -- "how many nuclei of each class lie in this
 * region".  Not in the reference.  Engine-free like the density call: every pointer but `slots` is device memory of `device`, the call
 * allocates and frees its own scratch, runs on `stream` and synchronises it before returning.  nuhtc_config is unchanged (no ABI bump).
 *   points [n][2] int32: node positions in HALF pixels, |p| < 2^27.  labels [n] int32.  0 <= n <= 2^24.  num_classes C: 1 .. 14.
 *   edges [E][4] int32 (ax, ay, bx, by): the edges of the regions' rings in half pixels, every |v| < 2^27, 16-byte aligned; a ring's
 *     closing edge is included, a zero-length edge is legal.  0 <= E <= 2^22.
 *   edge_region [E] int32: the region of every edge, in 0 .. G - 1 and non-decreasing.  0 <= G <= 2^16 (G == 0 needs E == 0).
 *   slab: the height in half pixels, 1 .. 16384, of the horizontal slabs the points and the edges are binned by.  Every output is
 *     independent of it; it decides the time only.
 *   slot_cap: 0 .. 2^28, the (edge, slab) records the call may hold: an edge has one record per slab its y-range meets inside the box.
 *     *slots (host memory, never null) receives the number M the call needs whenever it returns NUHTC_OK.  With M > slot_cap nothing
 *     else is written: call again with slot_cap >= M (nuhtc_amd/regions.py states M exactly on the host).
 *   x_min, y_min, x_max, y_max: the bounding box of the points (inclusive), computed by the caller on the host (ignored when n == 0).
 * Inside is even-odd and half-open: an edge with ay != by straddles p when (ay <= py) != (by <= py); oriented upward (lo -> hi) it is
 * crossed when (hi - lo) x (p - lo) > 0, an exact int64 cross product (differences < 2^28, products < 2^56); p is inside region g when an
 * odd number of g's edges are crossed.  Ring orientation, holes and multipolygons need no special case; regions that share an edge tile.
 * p is ON an edge when the cross product on a -> b is 0 and p lies in the edge's closed bounding box.
 *   region [n] int32: the LARGEST region index that holds the point, -1 for none.   depth [n] int32: how many regions hold it.
 *   on_boundary [n] uint8: 1 when the point lies on an edge of any region.
 *   census [G][C] int64: the points of label c inside region g, counted in EVERY region that holds them; a label outside 0 .. C - 1 is
 *     counted nowhere.
 * All four are always fully written on success with M <= slot_cap (n == 0: census is cleared).  The result is a pure function of the
 * input: bitwise the same on every call.
 * NUHTC_E_INVALID, before anything is launched and with the outputs untouched: n, num_classes, E, G, slab or slot_cap out of range, a
 * null pointer where the count is not 0, with n > 0 a bounding box that is empty or reaches +-2^27.
 * NUHTC_E_INVALID after the first kernels, the outputs still untouched: a vertex outside +-2^27, an edge_region outside 0 .. G - 1 or
 * decreasing, a point outside the stated bounding box. */
int nuhtc_cell_regions(int device, const int32_t* points, const int32_t* labels, int64_t n, int num_classes, const int32_t* edges,
                       const int32_t* edge_region, int64_t E, int64_t G, int slab, int64_t slot_cap, int x_min, int y_min, int x_max, int y_max,
                       int32_t* region, int32_t* depth, uint8_t* on_boundary, int64_t* census, int64_t* slots, void* stream);

/* Margin bands (csrc/cellmargin.hip; nuhtc_amd/margin.py holds the definition and the brute-force restatement `margin_reference`): the
 * nuclei of each class by distance to the boundary of every region, inside it and outside it -- the invasive-margin profile.  A sibling
 * of nuhtc_cell_regions with the same points, labels, edges, edge_region, slab, slot_cap / *slots protocol and bounding box, engine-free
 * like it.  Not in the reference.  nuhtc_config is unchanged (no ABI bump).
 *   thresholds [B] int32, HOST memory: e_0 < e_1 < .. < e_{B-1} in half pixels, 1 <= e_0, e_{B-1} <= 16384, 1 <= B <= 32.
 *   slot_cap: an edge has one record per slab of the box that its y-range grown by e_{B-1} meets (nuhtc_amd/margin.py states M exactly).
 * near(p, a -> b, e), inclusive and in exact integers: with d = b - a, w = p - a, L2 = d.d, s = w.d -- |w|^2 <= e^2 when L2 == 0 or
 * s <= 0; |p - b|^2 <= e^2 when s >= L2; else (d x w)^2 <= e^2 * L2, a 128-bit unsigned compare (cross < 2^57; e^2 * L2 < 2^85).
 * band(p, g) = the smallest t with near(p, edge, e_t) for some edge of g, B when none.  inside(p, g) is the even-odd, half-open rule of
 * nuhtc_cell_regions.
 *   band_census [G][2][B][C] int64: the points of label c with band(p, g) == t and inside(p, g) == side (0 outside, 1 inside); a point is
 *     counted for every region it is near, a label outside 0 .. C - 1 nowhere, a band of B nowhere.
 *   census [G][C] int64: the points of label c inside region g -- the census of nuhtc_cell_regions.
 *   band [n] int32: the minimum over g of band(p, g), B when none.   band_region [n] int32: the smallest g that attains it, -1 when none.
 *   band_inside [n] uint8: inside(p, band_region), 0 when there is none.
 * All five are always fully written on success with M <= slot_cap (n == 0: the two tables are cleared).  The result is a pure function
 * of the input: bitwise the same on every call.
 * NUHTC_E_INVALID, before anything is launched and with the outputs untouched: everything nuhtc_cell_regions refuses there, B outside
 * 1 .. 32, thresholds null, not strictly increasing or outside 1 .. 16384, a null pointer where the count is not 0.
 * NUHTC_E_INVALID after the first kernels, the outputs still untouched: as nuhtc_cell_regions. */
int nuhtc_cell_margin(int device, const int32_t* points, const int32_t* labels, int64_t n, int num_classes, const int32_t* edges,
                      const int32_t* edge_region, int64_t E, int64_t G, const int32_t* thresholds, int B, int slab, int64_t slot_cap, int x_min,
                      int y_min, int x_max, int y_max, int64_t* band_census, int64_t* census, int32_t* band, int32_t* band_region,
                      uint8_t* band_inside, int64_t* slots, void* stream);

/* Neighbourhood enrichment of a slide (csrc/cellenrich.hip; nuhtc_amd/enrichment.py holds the definition and the brute-force restatement
 * `enrichment_reference`): the class-pair contact counts of the nucleus centres, observed and under num_perms label permutations -- the
 * integers of the neighbourhood-enrichment permutation test (positions kept, labels shuffled).  Not in the reference.  Engine-free like
 * the spatial call: points, labels and the three outputs are device memory of `device`, the call allocates and frees its own scratch,
 * runs on `stream` and synchronises it before returning.  nuhtc_config is unchanged (no ABI bump).
 *   points [n][2] int32: node positions in HALF pixels, |p| < 2^27.  labels [n] int32.  0 <= n <= 2^24.  num_classes C: 1 .. 14.
 *   r: the contact radius in half pixels, 1 .. 16384, inclusive.  num_perms P: 1 .. 1024.  seed: any 32-bit value.
 *   x_min, y_min, x_max, y_max: the bounding box of the points (inclusive), computed by the caller on the host (cell side = the smallest
 *     multiple of r whose grid over the box has at most 2^22 cells; ignored when n == 0).
 * All arithmetic is integer.  An ordered pair (i, j), i != j, is a contact when dx * dx + dy * dy <= r * r; coincident points are
 * contacts.  Permutation p = 1 .. P of the rows is pi_p, a keyed six-round Feistel network with cycle-walking, an exact function of
 * (n, seed, p) (csrc/cellenrich_host.h); the shuffled labels are lab_p[i] = labels[pi_p(i)], every row taking part.
 *   observed    [C][C] int64:    the contacts with label_i = a and label_j = b; a label outside [0, C) is counted in no row and no column.
 *   perm_counts [P][C][C] int64: row p - 1 is the same count under lab_p.
 *   class_n     [C] int64:       the points of each class.
 * The call zeroes all three itself.  The result is a pure function of the input, the ORDER of the rows included (pi acts on row
 * numbers; observed and class_n do not depend on it): bitwise the same on every call.  n == 0 zeroes the outputs and returns NUHTC_OK.
 * NUHTC_E_INVALID, before anything is launched and with the outputs untouched: num_perms, r, num_classes or n out of range, a null
 * pointer, a bounding box that is empty or reaches +-2^27 (so: any coordinate out of range).  NUHTC_E_INVALID after the binning, the
 * outputs still untouched: a point lies outside the stated bounding box. */
int nuhtc_cell_enrichment(int device, const int32_t* points, const int32_t* labels, int64_t n, int num_classes, int r, int num_perms,
                          uint32_t seed, int x_min, int y_min, int x_max, int y_max, int64_t* observed, int64_t* perm_counts, int64_t* class_n,
                          void* stream);
/* The generator alone, on the HOST (no GPU is touched): out[i] = pi_p(i) for i < n, through the same header the kernels use.
 * 0 <= n <= 2^24, 1 <= p <= 1024; NUHTC_E_INVALID otherwise or when out is null with n > 0. */
int nuhtc_enrichment_permutation(int64_t n, uint32_t seed, int p, int32_t* out);

/* Cellular neighbourhoods of a slide (csrc/cellhood.hip; nuhtc_amd/neighbourhoods.py holds the definition and the numpy restatement
 * `neighbourhoods_reference`): the class composition of every nucleus's window -- itself and the neighbours nuhtc_cell_graph listed --
 * clustered by k-means into num_types neighbourhood types, in integers throughout.  Not in the reference.  Engine-free like the outline
 * call: it takes the tensors nuhtc_cell_graph took and left on the device and needs no points and no bounds; every pointer but `counts`
 * is device memory of `device`, the call allocates and frees its own scratch, runs on `stream` and synchronises it (once per batch of
 * 8 iterations, once at the end; with given centres once more at the start) before returning.  nuhtc_config is unchanged (no ABI bump).
 *   neighbors [n][k] int32: row indices or -1, as nuhtc_cell_graph wrote them.  labels [n] int32.  0 <= n <= 2^24, 1 <= k <= 32.
 *   num_classes C: 1 .. 14.  num_types K: 1 .. 32.  seed: any 32-bit value.  max_iter: 1 .. 1000.  centres_given: 0 or 1.
 *   window [n][C] int32: w[i][c] = the rows of label c among row i and its listed neighbours; a label outside [0, C) is counted nowhere.
 * centres_given == 0: k-means++ seeding in exact integers (draws u_j from the murmur3 finaliser; row_0 = u_0 mod n; then the smallest row
 * whose inclusive prefix sum of the squared distances to the nearest chosen window exceeds u_j mod T, row_0 again when T == 0;
 * centre = 1024 * window), then Lloyd on the fixed-point centres: argmin with ties to the smaller type, stop at the first iteration whose
 * assignment repeats the one before (converged) or at max_iter, else centre = floor((2048 sum + members) / (2 members)) for every type
 * with members.  centres_given == 1: centre_q holds the centres on entry, every entry 0 .. 34000; one assignment, no update.
 *   hood [n] int32: the final type of each row.  centre_q [K][C] int32 (in/out): the centres the final assignment was made against.
 *   centre_sum [K][C] int64, centre_n [K] int64: the window sums and members of that assignment.  seed_rows [K] int32: the seeding rows,
 *     -1 with given centres.
 *   counts: HOST memory, int64 [3] = n_iter (the iteration that stopped; 0 with given centres), converged (0 / 1), inertia (the sum over
 *     the rows of the squared fixed-point distance to the row's centre), written on success only.
 * The result is a pure function of the input, the ORDER of the rows included: bitwise the same on every call.  n == 0 writes centre_q
 * (the given centres, or zeros), zero sums, seed_rows = -1 and counts = 0, 1, 0.
 * NUHTC_E_INVALID, before anything is launched and with the outputs untouched: n, k, num_classes, num_types, max_iter or centres_given
 * out of range, a null pointer (neighbors, labels, window and hood only with n > 0), a given centre outside 0 .. 34000.
 * NUHTC_E_INVALID after the first kernels, the outputs still untouched: a neighbour index outside -1 .. n - 1. */
int nuhtc_cell_neighbourhoods(int device, const int32_t* neighbors, const int32_t* labels, int64_t n, int k, int num_classes, int num_types,
                              uint32_t seed, int max_iter, int centres_given, int32_t* centre_q, int32_t* window, int32_t* hood,
                              int64_t* centre_sum, int64_t* centre_n, int32_t* seed_rows, int64_t* counts, void* stream);
/* The rules of the neighbourhoods alone, on the HOST (no GPU is touched), through the same header the kernels use (csrc/cellhood_host.h).
 * nuhtc_neighbourhood_draws: out[j] = u_j, j < num_types (1 .. 32).  nuhtc_neighbourhood_rule: what == 0, the pick: *out = the smallest
 * i < x whose inclusive prefix a[i] exceeds t = y (0 <= y < a[x - 1]); what == 1, the rounding: *out = floor((2048 x + y) / (2 y)), z when
 * y == 0; what == 2, the distance: *out = sum_c (1024 a[c] - b[c])^2 over x == y <= 14 classes, a[c] 0 .. 33, b[c] 0 .. 34000.
 * NUHTC_E_INVALID for anything else. */
int nuhtc_neighbourhood_draws(uint32_t seed, int num_types, uint64_t* out);
int nuhtc_neighbourhood_rule(int what, const int64_t* a, const int64_t* b, int64_t x, int64_t y, int64_t z, int64_t* out);

/* Per-kernel timing with HIP events recorded on the launch stream (process-wide switch; off by default).
 * nuhtc_profile_read synchronises the device and writes one text line per kernel tag,
 * "tag launches total_ms algorithmic_flops algorithmic_bytes", then resets the records. */
int nuhtc_profile_enable(int on);
int nuhtc_profile_read(char* buf, size_t cap);
/* Shader clock under load (measurement): enqueues on `stream` a one-wave kernel that spins for `ticks_100mhz` periods of the 100 MHz
 * reference clock and writes out_dev[0] = shader cycles elapsed, out_dev[1] = reference ticks elapsed.  Launched on a stream of
 * its own beside the kernels being timed, out[0] / out[1] x 100 MHz is the clock the chip held under them.  Does not synchronise. */
int nuhtc_clock_probe(int device, uint64_t ticks_100mhz, uint64_t* out_dev, void* stream);
/* Development builds (-DNUHTC_DEV) only: set an integer switch of the launch heuristics (the NUHTC_<NAME> environment variables) at
 * run time.  The default build compiles every switch to its default and returns NUHTC_E_STATE here. */
int nuhtc_dev_knob(const char* name, int value);

#ifdef __cplusplus
}
#endif
#endif /* NUHTC_HIP_H */
