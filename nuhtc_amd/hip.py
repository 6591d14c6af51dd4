"""ctypes binding of libnuhtc_hip.so — the C ABI declared in include/nuhtc_hip.h.

There is no fallback: if the shared library is missing or fails to load, importing callers get an
ImportError/OSError that says how to build it (`python -m nuhtc_amd.build`).
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, 'libnuhtc_hip.so')

RLE_MAX_RUNS = 15360      # RLE_LDS_RUNS of csrc/rle.hip: the largest run_cap nuhtc_rle_encode honours (60 KB of LDS positions)
ABI_VERSION = 12          # NUHTC_ABI_VERSION of include/nuhtc_hip.h: the layout of Config below

OK, E_INVALID, E_HIP, E_STATE, E_CAPACITY, E_NOTFOUND = 0, -1, -2, -3, -4, -5
CH_AS_IS, CH_SWAP = 0, 1
OVERLAP_MASK, OVERLAP_POLYGON = 0, 1
PIPE_BF16_SPLIT, PIPE_FP32 = 0, 1
ORDER_TOKEN, ORDER_COMPACT = 0, 1
SCHED_LATENCY, SCHED_THROUGHPUT = 0, 1
EVAL_PANNUKE, EVAL_CONIC = 0, 1
TISSUE_ALL, TISSUE_MEDIAN, TISSUE_THRESHOLD = 0, 1, 2


class Config(ctypes.Structure):
    _fields_ = [
        ('abi_version', ctypes.c_int32), ('num_classes', ctypes.c_int32),
        ('tile_h', ctypes.c_int32), ('tile_w', ctypes.c_int32), ('valid_h', ctypes.c_int32), ('valid_w', ctypes.c_int32), ('max_batch', ctypes.c_int32),
        ('scale_factor', ctypes.c_float), ('mean', ctypes.c_float * 3), ('std', ctypes.c_float * 3),
        ('rpn_nms_pre', ctypes.c_int32), ('rpn_max_per_img', ctypes.c_int32),
        ('rpn_nms_iou', ctypes.c_float), ('rpn_min_bbox_size', ctypes.c_float),
        ('score_thr', ctypes.c_float), ('nms_iou', ctypes.c_float), ('max_per_img', ctypes.c_int32),
        ('mask_thr_binary', ctypes.c_float), ('att_thres', ctypes.c_float),
        ('watershed_proposal', ctypes.c_int32), ('max_cc_proposals', ctypes.c_int32),
        ('stage_stds', (ctypes.c_float * 4) * 3),
        ('margin', ctypes.c_int32), ('min_area', ctypes.c_int32), ('mask_nms_thr', ctypes.c_float),
        ('matrix_pipe', ctypes.c_int32), ('schedule', ctypes.c_int32), ('att_pool_fp16', ctypes.c_int32),
        ('features_only', ctypes.c_int32),
    ]


class Conv3Args(ctypes.Structure):
    """nuhtc_conv3_args: the arguments of nuhtc_op_conv3 (a 3x3 convolution and its fused epilogue options)."""
    _fields_ = [
        ('inp', ctypes.c_void_p), ('out', ctypes.c_void_p), ('w', ctypes.c_void_p), ('bias', ctypes.c_void_p),
        ('nimg', ctypes.c_int32), ('H', ctypes.c_int32), ('W', ctypes.c_int32), ('act', ctypes.c_int32),
        ('nimg_dev', ctypes.c_void_p), ('pipe', ctypes.c_int32), ('N2', ctypes.c_int32),
        ('w2', ctypes.c_void_p), ('b2', ctypes.c_void_p), ('act2', ctypes.c_int32), ('store_out', ctypes.c_int32),
        ('out2', ctypes.c_void_p), ('res2', ctypes.c_void_p), ('out3', ctypes.c_void_p),
        ('wn1', ctypes.c_void_p), ('bn1', ctypes.c_void_p), ('outn1', ctypes.c_void_p),
        ('n_more', ctypes.c_int32), ('more_in', ctypes.c_void_p * 3), ('more_out2', ctypes.c_void_p * 3),
        ('more_H', ctypes.c_int32 * 3), ('more_W', ctypes.c_int32 * 3),
    ]


class WmsaArgs(ctypes.Structure):
    """nuhtc_wmsa_args: the arguments of nuhtc_op_window_msa (the attention half of a Swin block up to the attention output)."""
    _fields_ = [
        ('x', ctypes.c_void_p), ('out', ctypes.c_void_p), ('ln_g', ctypes.c_void_p), ('ln_b', ctypes.c_void_p),
        ('qkv_w', ctypes.c_void_p), ('qkv_b', ctypes.c_void_p), ('rel_table', ctypes.c_void_p),
        ('B', ctypes.c_int32), ('H', ctypes.c_int32), ('W', ctypes.c_int32), ('C', ctypes.c_int32),
        ('shifted', ctypes.c_int32), ('pipe', ctypes.c_int32), ('out_order', ctypes.c_int32),
    ]


class BboxTailArgs(ctypes.Structure):
    """nuhtc_bbox_tail_args: the arguments of nuhtc_op_bbox_tail (classifier, regression rows and cascade refinement of one bbox head)."""
    _fields_ = [
        ('h', ctypes.c_void_p), ('cls_w', ctypes.c_void_p), ('cls_b', ctypes.c_void_p), ('reg_w', ctypes.c_void_p), ('reg_b', ctypes.c_void_p),
        ('nc', ctypes.c_int32), ('cap', ctypes.c_int32), ('refine', ctypes.c_int32),
        ('stds', ctypes.c_float * 4), ('img_w', ctypes.c_float), ('img_h', ctypes.c_float),
        ('r_dev', ctypes.c_void_p), ('rois', ctypes.c_void_p), ('cls', ctypes.c_void_p), ('reg', ctypes.c_void_p),
    ]


class DetPostArgs(ctypes.Structure):
    """nuhtc_det_post_args: the arguments of nuhtc_op_det_post (Seesaw candidates, multiclass NMS, labels and mask RoIs)."""
    _fields_ = [
        ('rois', ctypes.c_void_p), ('cls0', ctypes.c_void_p), ('cls1', ctypes.c_void_p), ('cls2', ctypes.c_void_p), ('reg2', ctypes.c_void_p),
        ('roi_off', ctypes.c_void_p), ('roi_cnt', ctypes.c_void_p),
        ('B', ctypes.c_int32), ('nc', ctypes.c_int32), ('total', ctypes.c_int32), ('cap', ctypes.c_int32),
        ('stds', ctypes.c_float * 4), ('img_w', ctypes.c_float), ('img_h', ctypes.c_float), ('scale', ctypes.c_float),
        ('score_thr', ctypes.c_float), ('nms_iou', ctypes.c_float), ('max_per_img', ctypes.c_int32), ('limit', ctypes.c_int32),
        ('dets', ctypes.c_void_p), ('labels', ctypes.c_void_p), ('counts', ctypes.c_void_p), ('mask_rois', ctypes.c_void_p),
        ('det_off', ctypes.c_void_p), ('det_total', ctypes.c_void_p),
        ('cand_count', ctypes.c_void_p), ('cand_scores', ctypes.c_void_p), ('cand_ids', ctypes.c_void_p), ('cand_boxes', ctypes.c_void_p),
    ]


class PasteArgs(ctypes.Structure):
    """nuhtc_paste_args: the arguments of nuhtc_op_paste (28x28 probabilities -> bit-packed masks and areas)."""
    _fields_ = [
        ('prob', ctypes.c_void_p), ('mask_rois', ctypes.c_void_p), ('det_off', ctypes.c_void_p), ('det_counts', ctypes.c_void_p),
        ('B', ctypes.c_int32), ('D', ctypes.c_int32), ('max_keep', ctypes.c_int32), ('H', ctypes.c_int32), ('W', ctypes.c_int32),
        ('vH', ctypes.c_int32), ('vW', ctypes.c_int32), ('scale', ctypes.c_float), ('thr', ctypes.c_float),
        ('masks', ctypes.c_void_p), ('areas', ctypes.c_void_p),
    ]


class TilePostArgs(ctypes.Structure):
    """nuhtc_tile_post_args: the arguments of nuhtc_op_tile_post (margin / area filter and greedy mask-NMS of a tile)."""
    _fields_ = [
        ('dets', ctypes.c_void_p), ('labels', ctypes.c_void_p), ('areas', ctypes.c_void_p), ('det_counts', ctypes.c_void_p),
        ('masks', ctypes.c_void_p), ('keep', ctypes.c_void_p),
        ('B', ctypes.c_int32), ('max_keep', ctypes.c_int32), ('H', ctypes.c_int32), ('W', ctypes.c_int32), ('vH', ctypes.c_int32),
        ('vW', ctypes.c_int32), ('margin', ctypes.c_int32), ('min_area', ctypes.c_int32), ('thr', ctypes.c_float),
    ]


class RoiFeatsArgs(ctypes.Structure):
    """nuhtc_roi_feats_args: the arguments of nuhtc_op_roi_feats (the fused RoI features of the box head, P = 7, and the mask head, P = 14)."""
    _fields_ = [
        ('x0', ctypes.c_void_p), ('x1', ctypes.c_void_p), ('sem', ctypes.c_void_p), ('x0sem', ctypes.c_void_p), ('G2', ctypes.c_void_p),
        ('G3', ctypes.c_void_p), ('rois', ctypes.c_void_p), ('r_dev', ctypes.c_void_p),
        ('B', ctypes.c_int32), ('cap', ctypes.c_int32), ('P', ctypes.c_int32), ('H', ctypes.c_int32 * 4), ('W', ctypes.c_int32 * 4),
        ('out', ctypes.c_void_p), ('fb_flag', ctypes.c_void_p), ('counts', ctypes.c_void_p),
    ]


AP_ROUTES = {'auto': 0, 'gemm': 1, 'kernel': 2, 'fp16': 3}      # NUHTC_AP_*


class EvalArgs(ctypes.Structure):
    """nuhtc_eval_args: the arguments of nuhtc_eval_batch (selection, pair tables, label maps and joint histograms of a finished inference)."""
    _fields_ = [
        ('gt_maps', ctypes.c_void_p), ('t_cap', ctypes.c_int32), ('trip_cap', ctypes.c_int32), ('joint_cap', ctypes.c_int32), ('format', ctypes.c_int32),
        ('fg_thr', ctypes.c_float), ('mask_nms_thr', ctypes.c_double),
        ('sel', ctypes.c_void_p), ('nsel', ctypes.c_void_p), ('sel_labels', ctypes.c_void_p), ('area_t', ctypes.c_void_p), ('area_p', ctypes.c_void_p),
        ('trips', ctypes.c_void_p), ('joint', ctypes.c_void_p), ('counters', ctypes.c_void_p), ('pred_maps', ctypes.c_void_p),
    ]


class StitchStore(ctypes.Structure):
    """nuhtc_stitch_store: the candidate records and crop pools of the images being stitched (csrc/stitch.hip)."""
    _fields_ = [
        ('n_img', ctypes.c_int32), ('cand_cap', ctypes.c_int32), ('pool_cap', ctypes.c_int32), ('work_cap', ctypes.c_int32),
        ('box', ctypes.c_void_p), ('area', ctypes.c_void_p), ('score', ctypes.c_void_p), ('label', ctypes.c_void_p), ('key', ctypes.c_void_p),
        ('off', ctypes.c_void_p), ('pool', ctypes.c_void_p), ('counters', ctypes.c_void_p), ('work', ctypes.c_void_p),
    ]


class Dets(ctypes.Structure):
    _fields_ = [('boxes', ctypes.c_void_p), ('labels', ctypes.c_void_p), ('counts', ctypes.c_void_p),
                ('masks', ctypes.c_void_p), ('areas', ctypes.c_void_p), ('keep', ctypes.c_void_p)]


EXPORTS = ['nuhtc_default_config', 'nuhtc_create', 'nuhtc_destroy', 'nuhtc_last_error', 'nuhtc_load_weight',
           'nuhtc_finalize', 'nuhtc_infer', 'nuhtc_infer_fixed_load', 'nuhtc_check', 'nuhtc_get_buffer',
           'nuhtc_op_gemm', 'nuhtc_op_gemm_split', 'nuhtc_op_roi_align', 'nuhtc_op_nms', 'nuhtc_profile_enable', 'nuhtc_profile_read', 'nuhtc_dev_knob', 'nuhtc_export_crops',
           'nuhtc_mask_contours', 'nuhtc_merge_overlap', 'nuhtc_export_kept', 'nuhtc_clock_probe', 'nuhtc_op_swin_mlp', 'nuhtc_stream', 'nuhtc_op_swin_proj_mlp', 'nuhtc_bind_host_thread',
           'nuhtc_bind_host_thread_pci', 'nuhtc_bind_host_thread_at', 'nuhtc_restore_host_thread', 'nuhtc_op_ln_gemm', 'nuhtc_op_gemm_ln_gemm', 'nuhtc_op_merge_ln_gemm', 'nuhtc_write_ring_features',
           'nuhtc_write_point_features', 'nuhtc_join_features', 'nuhtc_fill_rings', 'nuhtc_features', 'nuhtc_op_cc_mask', 'nuhtc_op_cc_proposals',
           'nuhtc_op_conv3', 'nuhtc_op_window_msa', 'nuhtc_op_bbox_tail', 'nuhtc_op_det_post', 'nuhtc_op_paste', 'nuhtc_op_tile_post',
           'nuhtc_op_rpn_select', 'nuhtc_op_nms_levels', 'nuhtc_op_build_rois', 'nuhtc_op_attn_pool', 'nuhtc_op_roi_feats',
           'nuhtc_eval_batch', 'nuhtc_op_eval_select', 'nuhtc_op_eval_pairs', 'nuhtc_op_eval_render', 'nuhtc_op_eval_joint',
           'nuhtc_stitch_gather', 'nuhtc_stitch_pairs', 'nuhtc_stitch_render', 'nuhtc_op_stitch_gather', 'nuhtc_op_stitch_pairs', 'nuhtc_op_stitch_render',
           'nuhtc_tissue_mask', 'nuhtc_points_polygon_test', 'nuhtc_grid_in_contour', 'nuhtc_rle_encode',
           'nuhtc_nucleus_features', 'nuhtc_op_nucleus_pool', 'nuhtc_cell_graph', 'nuhtc_nucleus_morph', 'nuhtc_op_nucleus_morph',
           'nuhtc_nucleus_texture', 'nuhtc_op_nucleus_texture', 'nuhtc_op_nucleus_gradient', 'nuhtc_op_nucleus_shape', 'nuhtc_op_ring_fill', 'nuhtc_op_frame_gather', 'nuhtc_op_ring_fsd',
           'nuhtc_op_patch_embed', 'nuhtc_op_layernorm', 'nuhtc_op_merge_ln', 'nuhtc_op_fpn_lateral', 'nuhtc_op_sem_fuse', 'nuhtc_op_pointwise64',
           'nuhtc_op_fpn_mean_pool', 'nuhtc_cell_spatial', 'nuhtc_cell_clusters', 'nuhtc_cell_mst', 'nuhtc_cell_proximity', 'nuhtc_cell_density', 'nuhtc_cell_regions', 'nuhtc_cell_margin',
           'nuhtc_cell_enrichment', 'nuhtc_enrichment_permutation', 'nuhtc_cell_territory', 'nuhtc_territory_adjacency', 'nuhtc_cell_alpha', 'nuhtc_alpha_outline',
           'nuhtc_cell_neighbourhoods', 'nuhtc_neighbourhood_draws', 'nuhtc_neighbourhood_rule']

_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f'{LIB_PATH} not found: the HIP extension is required (no CPU fallback exists). '
                          'Build it with `python -m nuhtc_amd.build` (hipcc, --offload-arch=gfx950).')
    # torch first: it brings its own copy of the HIP runtime, and a process must hold ONE -- loaded after torch, this library's libamdhip64
    # dependency resolves to the copy torch loaded; loaded before it (e.g. __graft_entry__.build() followed by smoke() in one process), the
    # process ends up with two runtimes and the second one finds no device (nuhtc_create: "no such HIP device")
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.nuhtc_default_config.argtypes = [ctypes.POINTER(Config)]
    lib.nuhtc_default_config.restype = None
    lib.nuhtc_create.argtypes = [ctypes.POINTER(Config), ci, ctypes.POINTER(vp)]
    lib.nuhtc_destroy.argtypes = [vp]
    lib.nuhtc_destroy.restype = None
    lib.nuhtc_last_error.argtypes = [vp]
    lib.nuhtc_last_error.restype = ctypes.c_char_p
    lib.nuhtc_load_weight.argtypes = [vp, ctypes.c_char_p, vp, ctypes.POINTER(ctypes.c_int64), ci]
    lib.nuhtc_finalize.argtypes = [vp]
    lib.nuhtc_infer.argtypes = [vp, vp, ci, ci, vp, ctypes.POINTER(Dets)]
    lib.nuhtc_features.argtypes = [vp, vp, ci, ci, vp, vp]
    lib.nuhtc_infer_fixed_load.argtypes = [vp, vp, ci, ci, vp, ci, ci, vp, ctypes.POINTER(Dets)]
    lib.nuhtc_check.argtypes = [vp, vp]
    lib.nuhtc_get_buffer.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_int64),
                                     ctypes.POINTER(ci), ctypes.POINTER(ci)]
    lib.nuhtc_op_gemm.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, vp]
    lib.nuhtc_op_gemm_split.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, vp]
    lib.nuhtc_op_ln_gemm.argtypes = [vp, vp, ci, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, vp]
    lib.nuhtc_op_gemm_ln_gemm.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, vp]
    lib.nuhtc_op_merge_ln_gemm.argtypes = [vp, vp, ci, ci, ci, ci, vp, vp, vp, vp, vp]
    lib.nuhtc_op_swin_mlp.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, vp]
    lib.nuhtc_op_swin_proj_mlp.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, vp]
    lib.nuhtc_op_roi_align.argtypes = [vp, vp, ci, ci, ci, vp, ci, ci, cf, ci, vp, vp]
    lib.nuhtc_op_nms.argtypes = [vp, vp, vp, ci, cf, vp, vp, vp]
    lib.nuhtc_op_cc_mask.argtypes = [vp, vp, ci, ci, ci, ci, ci, vp, vp]
    lib.nuhtc_op_cc_proposals.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.nuhtc_op_conv3.argtypes = [vp, ctypes.POINTER(Conv3Args), vp]
    lib.nuhtc_op_window_msa.argtypes = [vp, ctypes.POINTER(WmsaArgs), vp]
    f3 = ctypes.POINTER(cf)
    lib.nuhtc_op_patch_embed.argtypes = [vp, vp, ci, ci, ci, ci, ci, cf, ci, f3, f3, vp, vp, vp, vp, vp, vp, vp]
    lib.nuhtc_op_layernorm.argtypes = [vp, vp, vp, vp, vp, ci, ci, vp]
    lib.nuhtc_op_merge_ln.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, vp]
    lib.nuhtc_op_fpn_lateral.argtypes = [vp, vp, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp]
    lib.nuhtc_op_sem_fuse.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, ci, vp]
    lib.nuhtc_op_pointwise64.argtypes = [vp, vp, vp, vp, vp, ci, vp, ci, ci, vp]
    lib.nuhtc_op_fpn_mean_pool.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_int32), ci, vp, vp]
    lib.nuhtc_op_bbox_tail.argtypes = [vp, ctypes.POINTER(BboxTailArgs), vp]
    lib.nuhtc_op_det_post.argtypes = [vp, ctypes.POINTER(DetPostArgs), vp]
    lib.nuhtc_op_paste.argtypes = [vp, ctypes.POINTER(PasteArgs), vp]
    lib.nuhtc_op_tile_post.argtypes = [vp, ctypes.POINTER(TilePostArgs), vp]
    i4 = ctypes.POINTER(ctypes.c_int32)
    lib.nuhtc_op_rpn_select.argtypes = [vp, ctypes.POINTER(vp), i4, i4, ci, ci, ci, ci, cf, vp, vp, vp, vp]
    lib.nuhtc_op_nms_levels.argtypes = [vp, vp, vp, vp, ci, ci, ci, cf, ci, ci, vp, vp, vp, vp]
    lib.nuhtc_op_build_rois.argtypes = [vp, vp, vp, ci, vp, vp, ci, vp, ci, ci, ci, vp, vp, vp, vp, vp]
    lib.nuhtc_op_attn_pool.argtypes = [vp, vp, ci, ci, cf, ci, vp, vp]
    lib.nuhtc_op_roi_feats.argtypes = [vp, ctypes.POINTER(RoiFeatsArgs), vp]
    lib.nuhtc_eval_batch.argtypes = [vp, ctypes.POINTER(Dets), ci, ctypes.POINTER(EvalArgs), vp]
    lib.nuhtc_op_eval_select.argtypes = [vp, vp, ci, vp, vp, vp, ci, ci, ci, ci, cf, ctypes.c_double, vp, vp, vp, vp]
    lib.nuhtc_op_eval_pairs.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp]
    lib.nuhtc_op_eval_render.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, vp, vp]
    lib.nuhtc_op_eval_joint.argtypes = [vp, vp, ci, vp, ci, ci, ci, ci, ci, ci, vp, vp, vp]
    sst = ctypes.POINTER(StitchStore)
    lib.nuhtc_stitch_gather.argtypes = [vp, ctypes.POINTER(Dets), ci, vp, cf, cf, sst, vp]
    lib.nuhtc_op_stitch_gather.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, cf, cf, sst, vp]
    lib.nuhtc_stitch_pairs.argtypes = lib.nuhtc_op_stitch_pairs.argtypes = [vp, sst, ci, vp, ci, vp, ci, ci, ci, ci, vp, vp, vp, vp]
    lib.nuhtc_stitch_render.argtypes = lib.nuhtc_op_stitch_render.argtypes = [vp, sst, ci, vp, ci, ci, ci, vp, vp, vp, vp]
    lib.nuhtc_mask_contours.argtypes = [vp, ctypes.POINTER(Dets), ci, ci, vp, vp, vp]
    lib.nuhtc_merge_overlap.argtypes = [ci, vp, vp, vp, vp, vp, ctypes.c_int64, ctypes.c_int64, ci, ctypes.c_double, ci, ci, ci, ci, vp, vp]
    lib.nuhtc_tissue_mask.argtypes = [ci, vp, ci, ci, ctypes.c_int64, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp]
    lib.nuhtc_points_polygon_test.argtypes = [ci, vp, ctypes.c_int64, vp, ctypes.c_int64, vp, vp]
    lib.nuhtc_grid_in_contour.argtypes = [ci, ci, ci, ci, ci, ci, vp, ci, ci, vp, ctypes.c_int64, vp, ctypes.c_int64, vp, ci, ci, ci, vp, vp]
    lib.nuhtc_rle_encode.argtypes = [ci, vp, vp, ci, ci, ci, ci, vp, vp, vp, ctypes.c_int64, vp, vp]
    lib.nuhtc_nucleus_features.argtypes = [vp, ctypes.POINTER(Dets), ci, vp, vp, ci, vp, vp]
    lib.nuhtc_op_nucleus_pool.argtypes = [vp, ctypes.POINTER(vp), i4, i4, i4, ci, vp, ci, ci, ci, vp, vp, ci, vp, vp]
    lib.nuhtc_cell_graph.argtypes = [ci, vp, vp, ctypes.c_int64, ci, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp]
    lib.nuhtc_cell_spatial.argtypes = [ci, vp, vp, ctypes.c_int64, ci, i4, ci, ci, ci, ci, ci, vp, vp, vp, vp]
    lib.nuhtc_cell_clusters.argtypes = [ci, vp, vp, ctypes.c_int64, ci, ci, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp,
                                        ctypes.POINTER(ctypes.c_int64), vp]
    lib.nuhtc_cell_mst.argtypes = [ci, vp, vp, ctypes.c_int64, ci, ci, ci, ci, ci, ci, ci, vp, vp, vp] + [ctypes.POINTER(ctypes.c_int64)] * 3 + [vp]
    lib.nuhtc_cell_proximity.argtypes = [ci, vp, vp, ctypes.c_int64, ci, ci, ci, ctypes.c_int64, ci, ci, ci, ci, vp, vp, vp, vp] + [ctypes.POINTER(ctypes.c_int64)] * 2 + [vp]
    lib.nuhtc_cell_alpha.argtypes = [ci, vp, vp, ctypes.c_int64, ci, ci, ci, ctypes.c_int64, ci, ci, ci, ci, vp, vp, vp, vp, vp] + [ctypes.POINTER(ctypes.c_int64)] * 2 + [vp]
    lib.nuhtc_alpha_outline.argtypes = [ci, vp, vp, ctypes.c_int64, ci, vp, vp, vp, ctypes.c_int64, vp, vp, vp, vp, vp, vp, ctypes.POINTER(ctypes.c_int64), vp]
    lib.nuhtc_cell_density.argtypes = [ci, vp, vp, ctypes.c_int64] + [ci] * 11 + [vp, vp, vp]
    lib.nuhtc_cell_territory.argtypes = [ci, vp, vp, ctypes.c_int64] + [ci] * 11 + [vp] * 9
    lib.nuhtc_territory_adjacency.argtypes = [ci, vp, ci, ci, ctypes.c_int64, ctypes.c_int64, vp, vp, vp, ctypes.POINTER(ctypes.c_int64), vp]
    lib.nuhtc_cell_regions.argtypes = [ci, vp, vp, ctypes.c_int64, ci, vp, vp, ctypes.c_int64, ctypes.c_int64, ci, ctypes.c_int64, ci, ci, ci, ci, vp, vp, vp, vp,
                                       ctypes.POINTER(ctypes.c_int64), vp]
    lib.nuhtc_cell_margin.argtypes = [ci, vp, vp, ctypes.c_int64, ci, vp, vp, ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(ctypes.c_int32), ci, ci, ctypes.c_int64,
                                      ci, ci, ci, ci, vp, vp, vp, vp, vp, ctypes.POINTER(ctypes.c_int64), vp]
    lib.nuhtc_cell_enrichment.argtypes = [ci, vp, vp, ctypes.c_int64, ci, ci, ci, ctypes.c_uint32, ci, ci, ci, ci, vp, vp, vp, vp]
    lib.nuhtc_enrichment_permutation.argtypes = [ctypes.c_int64, ctypes.c_uint32, ci, vp]
    lib.nuhtc_cell_neighbourhoods.argtypes = [ci, vp, vp, ctypes.c_int64, ci, ci, ci, ctypes.c_uint32, ci, ci, vp, vp, vp, vp, vp, vp, ctypes.POINTER(ctypes.c_int64), vp]
    lib.nuhtc_neighbourhood_draws.argtypes = [ctypes.c_uint32, ci, vp]
    lib.nuhtc_neighbourhood_rule.argtypes = [ci, vp, vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
    lib.nuhtc_nucleus_morph.argtypes = [vp, ctypes.POINTER(Dets), ci, vp, ci, vp, i4, vp, vp, ci, vp, vp, vp]
    lib.nuhtc_op_nucleus_morph.argtypes = [vp, vp, ci, vp, i4, ci, vp, ci, ci, ci, vp, vp, ci, vp, vp, vp]
    lib.nuhtc_nucleus_texture.argtypes = [vp, ctypes.POINTER(Dets), ci, vp, ci, vp, i4, vp, vp, ci, vp, vp]
    lib.nuhtc_op_nucleus_texture.argtypes = [vp, vp, ci, vp, i4, ci, vp, ci, ci, ci, vp, vp, ci, vp, vp]
    lib.nuhtc_op_nucleus_gradient.argtypes = [vp, vp, ci, vp, i4, ci, vp, ci, ci, ci, vp, vp, ci, ci, vp, vp]
    lib.nuhtc_op_nucleus_shape.argtypes = [vp, ci, vp, ci, ci, ci, vp, vp, ci, vp, vp]
    lib.nuhtc_op_ring_fill.argtypes =[ci, vp, ctypes.c_int64, vp, vp, ci, ci, vp, vp, vp]
    lib.nuhtc_op_frame_gather.argtypes = [ci, vp, ci, ci, ci, ci, vp, ci, ci, vp, vp]
    lib.nuhtc_op_ring_fsd.argtypes = [ci, vp, ctypes.c_int64, vp, ci, vp, vp, vp]
    lib.nuhtc_export_kept.argtypes = [vp, ctypes.POINTER(Dets), ci, vp, vp, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.nuhtc_export_crops.argtypes = [vp, vp, vp, ci, vp, vp, vp, vp, ci, vp]
    lib.nuhtc_profile_enable.argtypes = [ci]
    lib.nuhtc_clock_probe.argtypes = [ci, ctypes.c_uint64, vp, vp]
    lib.nuhtc_dev_knob.argtypes = [ctypes.c_char_p, ci]
    lib.nuhtc_bind_host_thread.argtypes = [ci]
    lib.nuhtc_bind_host_thread_pci.argtypes = [ctypes.c_char_p]
    lib.nuhtc_bind_host_thread_at.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    lib.nuhtc_restore_host_thread.argtypes = []
    lib.nuhtc_stream.argtypes = [vp]
    lib.nuhtc_profile_read.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    pcp = ctypes.POINTER(ctypes.c_char_p)
    lib.nuhtc_write_ring_features.argtypes = [vp, vp, vp, vp, ctypes.c_int64, ctypes.c_char_p, pcp, pcp, ctypes.c_int32, vp, ctypes.c_int64, vp, ctypes.c_int32]
    lib.nuhtc_write_point_features.argtypes = [vp, vp, vp, ctypes.c_int64, ctypes.c_char_p, pcp, pcp, ctypes.c_int32, vp, ctypes.c_int64]
    lib.nuhtc_join_features.argtypes = [vp, vp, vp, ctypes.c_int64, vp, ctypes.c_int64, ctypes.c_int32]
    lib.nuhtc_fill_rings.argtypes = [vp, vp, ctypes.c_int64, vp, vp, vp, vp, ctypes.c_int64, ctypes.c_int32]
    for name in EXPORTS:
        fn = getattr(lib, name)
        if fn.restype is ctypes.c_int or name not in ('nuhtc_default_config', 'nuhtc_destroy', 'nuhtc_last_error', 'nuhtc_stream'):
            fn.restype = ci
    lib.nuhtc_last_error.restype = ctypes.c_char_p
    lib.nuhtc_default_config.restype = None
    lib.nuhtc_destroy.restype = None
    lib.nuhtc_stream.restype = ctypes.c_void_p
    for fn in (lib.nuhtc_write_ring_features, lib.nuhtc_write_point_features, lib.nuhtc_join_features, lib.nuhtc_fill_rings):
        fn.restype = ctypes.c_int64
    _lib = lib
    return lib


def default_config():
    cfg = Config()
    load().nuhtc_default_config(ctypes.byref(cfg))
    if cfg.abi_version != ABI_VERSION:
        raise ImportError(f'{LIB_PATH} speaks ABI {cfg.abi_version}, this binding {ABI_VERSION}: rebuild it (`python -m nuhtc_amd.build --force`)')
    return cfg


def op_nucleus(lib, h, spec, dims, masks, pairs, outs, stream, tiles=None, stain=None, channel_mode=CH_AS_IS, n=None, ints=()):
    """THE argument list of the mask-list ops nuhtc_op_nucleus_{morph,texture,gradient,shape} (Engine.op_nucleus_* and ringfeat._Ops call
    nothing else).  spec: anything with .call (the C entry) and .reads ('tiles': the entry takes tiles, channel mode, stain table and
    coefficients in front of the masks; 'masks': it does not) -- an entry of ringfeat.FAMILIES; dims = (B, K, H, W) of the masks, ints; tiles,
    masks, pairs, outs (one per output field, in the entry's order) and n (None: all of pairs) are checked device tensors; stain = (device
    table, host coefficients); ints: the entry's extra integers, passed behind n_max.  -> the entry's return code."""
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    src = (vp(tiles), int(channel_mode), vp(stain[0]), stain[1]) if spec.reads == 'tiles' else ()
    B, K, H, W = dims
    return getattr(lib, spec.call)(h, *src, B, vp(masks), K, H, W, vp(pairs), vp(n) if n is not None else None, int(pairs.shape[0]),
                                   *[int(i) for i in ints], *[vp(o) for o in outs], stream)


BIND_REASON = {0: 'bound', -1: 'not a PCI address', -2: 'no such HIP device', -3: "the thread's own CPU mask excludes the GPU's NUMA node",
               -5: 'the host exposes no NUMA node for the device'}
bind_reason = 'never called'          # why the last bind_host_thread of this process returned what it did (BIND_REASON)


def bind_host_thread(device=0, pci_bdf=None, sysfs_root=None):
    """Restrict the calling thread to the CPUs of the NUMA node the GPU is attached to (nuhtc_bind_host_thread: the thread that submits
    an engine's work should run there -- from the other socket every dispatch packet costs the command processor 1.4-2.9 us more),
    intersected with the mask the thread had before its first placement (`restore_host_thread` gives that mask back).
    Returns True when the thread now runs inside that node, False when nothing was changed; `hip.bind_reason` then says why (no NUMA
    node for the device / the caller's own mask excludes it / not a PCI address).  A device the runtime cannot name raises.
    `sysfs_root`: the test entry point (nuhtc_bind_host_thread_at)."""
    global bind_reason
    lib = load()
    if sysfs_root is not None:
        rc = lib.nuhtc_bind_host_thread_at(str(sysfs_root).encode(), pci_bdf.encode())
    else:
        rc = lib.nuhtc_bind_host_thread_pci(pci_bdf.encode()) if pci_bdf else lib.nuhtc_bind_host_thread(int(device))
    bind_reason = BIND_REASON.get(rc, f'error {rc}')
    if rc == -2:
        raise RuntimeError(f'nuhtc_bind_host_thread: no such device ({device})')
    return rc == 0


def restore_host_thread():
    """The calling thread gets back the CPU mask it had before its first bind_host_thread (no-op when it was never placed)."""
    return load().nuhtc_restore_host_thread() == 0


def profile_enable(on=True):
    load().nuhtc_profile_enable(1 if on else 0)


def dev_knob(name, value):
    """Development: set a switch of the launch heuristics (NUHTC_<NAME>) at run time."""
    rc = load().nuhtc_dev_knob(name.encode(), int(value))
    if rc:
        raise RuntimeError('nuhtc_dev_knob: not a development build (NUHTC_EXTRA_CFLAGS=-DNUHTC_DEV python -m nuhtc_amd.build --force)')


def profile_read():
    """{tag: dict(launches, ms, flops, bytes)} of the kernels launched since profile_enable / the last read."""
    buf = ctypes.create_string_buffer(1 << 16)
    rc = load().nuhtc_profile_read(buf, len(buf))
    if rc:
        raise RuntimeError(f'nuhtc_profile_read failed ({rc})')
    out = {}
    for line in buf.value.decode().splitlines():
        tag, n, ms, fl, by = line.rsplit(' ', 4)
        out[tag] = dict(launches=int(n), ms=float(ms), flops=float(fl), bytes=float(by))
    return out


class ClockProbe:
    """Shader clock held while other kernels run: start() enqueues the one-wave probe for `ms` milliseconds, ghz() waits for it and
    returns cycles / reference ticks x 0.1 GHz.  The probe runs on a NON-BLOCKING stream of its own (never the legacy null stream:
    a kernel spinning there serialises every blocking stream of the process, torch's default stream included, for the whole probe).
    Create the probe AFTER the engines: streams are dealt round the runtime's hardware queues in creation order, and a probe that
    shares a queue with an engine runs alone, ahead of the steps it is meant to run beside (it then reports the idle clock: with
    four one-stream engines on the default four queues that cannot be avoided, and ghz() is then the clock between their batches)."""

    def __init__(self, device=0, stream=None):
        import torch
        self.device = device
        if stream is None:          # torch's pool streams are created with hipStreamNonBlocking
            stream = torch.cuda.Stream(device=torch.device('cuda', device))
        self.stream = stream
        with torch.cuda.stream(self.stream):
            self.out = torch.zeros(2, dtype=torch.int64, device=torch.device('cuda', device))
        self.stream.synchronize()

    def start(self, ms):
        rc = load().nuhtc_clock_probe(self.device, int(ms * 1e5), ctypes.c_void_p(self.out.data_ptr()), ctypes.c_void_p(self.stream.cuda_stream))
        if rc:
            raise RuntimeError(f'nuhtc_clock_probe failed ({rc})')

    def ghz(self):
        self.stream.synchronize()
        with __import__('torch').cuda.stream(self.stream):
            c, r = (int(v) for v in self.out.cpu())
        return 0.1 * c / r if r else None
