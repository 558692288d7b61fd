"""ctypes binding of libcatseg_hip.so (C ABI declared in include/*.h).

There is no CPU fallback: importing this module without the built library raises.
PyTorch is used only to own device memory and streams; every kernel is launched
through the C ABI with raw pointers.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CATSEG_LIB") or os.path.join(_HERE, "libcatseg_hip.so")  # CATSEG_LIB: A/B builds of the library

if not os.path.exists(LIB_PATH):
    raise ImportError(
        "libcatseg_hip.so is missing (%s). Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
        "or `make -C miccai2021_cataract_semantic_segmentation_amd/csrc`. There is no CPU fallback." % LIB_PATH)

lib = C.CDLL(LIB_PATH)

P, I, L, F, SZ = C.c_void_p, C.c_int, C.c_longlong, C.c_float, C.c_size_t


class ConvDesc(C.Structure):
    _fields_ = [(n, I) for n in ("B", "H", "W", "Cin", "Ho", "Wo", "Cout", "kh", "kw", "stride", "pad", "dil",
                                 "ldx", "ldy", "stem4", "groups")]


# catseg_conv_fwd_desc / _bwd_data_desc / _bwd_weight_desc, filled by keyword: a field left out is NULL / 0.  operands: how both GEMM operands
# of the call are stored (CATSEG_OPERANDS_*)
OPERANDS_F32, OPERANDS_BF16X3, OPERANDS_BF16X3_BLOCKED, OPERANDS_F16X2, OPERANDS_F16X2_BLOCKED = range(5)


class ConvFwdDesc(C.Structure):
    _fields_ = [("geo", ConvDesc), ("operands", I), ("x", P), ("x_scale", P), ("w", P), ("w_scale", P), ("bias", P), ("y", P), ("zero_to", I),
                ("bn_part", P), ("bn_part_floats", SZ), ("tile_rows", P), ("n_tiles", P), ("residual", P), ("ldr", I), ("relu", I)]


class ConvBwdDataDesc(C.Structure):
    _fields_ = [("geo", ConvDesc), ("operands", I), ("dy", P), ("dy_scale", P), ("w", P), ("w_scale", P), ("dx", P), ("accumulate", I)]


class ConvBwdWeightDesc(C.Structure):
    _fields_ = [("geo", ConvDesc), ("operands", I), ("x", P), ("x_scale", P), ("dy", P), ("dy_scale", P), ("dw", P), ("dbias", P),
                ("workspace", P), ("workspace_bytes", SZ)]


# catseg_bn_apply_desc / catseg_bn_backward_desc, filled by keyword: a field left out is NULL / 0
class BnApplyDesc(C.Structure):
    _fields_ = [("y", P), ("ldy", I), ("mean", P), ("scale", P), ("beta", P), ("residual", P), ("ldr", I), ("residual_record", P), ("z", P), ("ldz", I),
                ("z_planes", P), ("rows", L), ("C", I), ("relu", I), ("record", P), ("mask", P)]


class BnBackwardDesc(C.Structure):
    _fields_ = [("dz", P), ("lddz", I), ("y", P), ("ldy", I), ("stats", P), ("gamma", P), ("rows", L), ("C", I), ("relu", I), ("z", P), ("ldz", I),
                ("beta", P), ("mask", P), ("partials", P), ("n_blocks", I), ("dres", P), ("lddres", I), ("dres_accumulate", I), ("g_record", P),
                ("y_record", P), ("dy_record", P), ("dgamma", P), ("dbeta", P), ("workspace", P), ("workspace_bytes", SZ), ("dy", P), ("lddy", I),
                ("dy_planes", P), ("dy_h2_planes", P), ("dy_h2_scale", P), ("dbias", P), ("frozen", I), ("running_mean", P), ("running_var", P),
                ("eps", F), ("scale", P)]


class PointrendGatherDesc(C.Structure):
    _fields_ = [("src", P * 5), ("ld", I * 5), ("H", I * 5), ("W", I * 5), ("C", I * 5), ("n_sources", I), ("idx", P), ("N", I), ("k", I), ("h", I),
                ("w", I), ("out", P), ("ld_out", I), ("extra", P * 4), ("extra_ld", I * 4), ("extra_off", I * 4), ("n_extra", I)]


class PointrendGatherBwdDesc(C.Structure):
    _fields_ = [("dst", P * 5), ("ld", I * 5), ("H", I * 5), ("W", I * 5), ("C", I * 5), ("accumulate", I * 5), ("n_sources", I), ("coords", P),
                ("N", I), ("P", I), ("dx", P), ("ld_dx", I)]


_SIGS = {
    # include/catseg.h, include/catseg_debug.h
    "catseg_last_error": (C.c_char_p, []),
    "catseg_version": (I, []),
    "catseg_conv2d_fwd": (I, [P, P]),
    "catseg_bn_finalize": (I, [P, I, L, L, I, P, F, F, P, P, P, P, P]),
    "catseg_bn_finalize_counts": (I, [P, I, P, L, I, P, F, F, P, P, P, P, P]),
    "catseg_dconv3_supported": (I, [I]),
    "catseg_dconv3_wimg_bytes": (SZ, [I]),
    "catseg_dconv3_tiles": (I, [I, I, I, I, P, P]),
    "catseg_dconv3_prep": (I, [P, I, I, P, P]),
    "catseg_dconv3_layout": (I, [I, P, P]),
    "catseg_dwgrad3_supported": (I, [I]),
    "catseg_dwgrad3_workspace": (SZ, [I, I, I, I]),
    "catseg_dwgrad3": (I, [I, I, I, I, P, I, P, I, P, P, SZ, P]),
    "catseg_debug_set_dwgrad3_blocks": (I, [I]),
    "catseg_dconv3_prep_batch": (I, [P, I, P, P, P]),
    "catseg_dconv3": (I, [I, I, I, I, P, I, P, P, P, I, I, P, SZ, P, P]),
    "catseg_dconv3_bnbwd": (I, [I, I, I, I, P, I, P, P, I, P, I, P, P, P, P, SZ, P]),
    "catseg_dwgrad3_f16x2": (I, [I, I, I, I, P, I, P, P, I, P, P, P, SZ, P]),
    "catseg_dconv3_f16x2_wimg_bytes": (SZ, [I]),
    "catseg_dconv3_f16x2_prep_batch": (I, [P, I, P, P, P, P]),
    "catseg_dconv3_f16x2": (I, [I, I, I, I, P, I, P, P, P, P, P, I, I, P, SZ, P, P]),
    "catseg_dconv3_bnbwd_f16x2": (I, [I, I, I, I, P, I, P, P, P, P, I, P, I, P, P, P, P, SZ, P]),
    "catseg_dconv3_pl_supported": (I, [I]),
    "catseg_dconv3_pl_rows": (I, [I, I, I, I]),
    "catseg_planes_bytes": (SZ, [L, I]),
    "catseg_planes_from_f32": (I, [P, I, L, I, P, P, I, P]),
    "catseg_dconv3_pl": (I, [I, I, I, I, P, P, P, P, P, P, I, I, P, SZ, P, P, P]),
    "catseg_dconv3_pl_bnbwd": (I, [I, I, I, I, P, P, P, P, P, I, P, I, P, P, P, P, SZ, P, P]),
    "catseg_dwgrad3_pl_supported": (I, [I]),
    "catseg_dwgrad3_pl_workspace": (SZ, [I, I, I, I]),
    "catseg_dwgrad3_pl": (I, [I, I, I, I, P, P, P, P, P, P, SZ, P]),
    "catseg_bn_finalize_counts_bound": (I, [P, I, P, L, I, P, P, F, F, P, P, P, P, P, P, P]),
    "catseg_bn_backward_h2_workspace": (SZ, [L, I]),
    "catseg_head_fwd": (I, [P, I, P, P, P, P, P, I, L, I, P, I, I, P]),
    "catseg_head_backward_workspace": (SZ, [L, I]),
    "catseg_head_backward": (I, [P, I, P, I, P, P, P, P, I, L, I, P, P, P, P, P, P, P, P, P, P, P, SZ, P]),
    "catseg_head_fwd_drop": (I, [P, I, P, P, P, P, P, I, L, I, P, I, I, P, L, F, P]),
    "catseg_head_backward_drop": (I, [P, I, P, I, P, P, P, P, I, L, I, P, P, P, P, P, P, P, P, P, P, P, SZ, P, L, F, P]),
    "catseg_dropout2d_mask": (I, [P, F, I, I, P, P, P]),
    "catseg_dropout2d_mask_fixed": (I, [P, F, I, I, P, P, P]),
    "catseg_dropout2d_apply": (I, [P, I, P, L, I, L, P, I, P]),
    "catseg_maxpool2x2_fwd": (I, [P, I, P, I, P, I, I, I, I, P]),
    "catseg_maxpool2x2_bwd": (I, [P, I, P, P, I, I, I, I, I, P]),
    "catseg_bias_rows": (I, [P, P, I, L, I, P]),
    "catseg_amax_record": (I, [P, I, L, I, P, P]),
    "catseg_maxpool2x2_fwd_rec": (I, [P, I, P, I, P, I, I, I, I, P, P, P]),
    "catseg_upcat2x_fwd": (I, [P, I, P, I, P, I, I, I, I, I, I, P, P]),
    "catseg_relu_bwd_rec": (I, [P, I, P, I, P, P, I, P, I, I, I, I, I, P, P]),
    "catseg_bn_mask_bytes": (SZ, [L, I]),
    "catseg_fold_bn": (I, [P, P, P, P, P, P, F, I, I, P, P, P]),
    "catseg_conv2d_bwd_data": (I, [P, P]),
    "catseg_conv2d_bwd_weight_workspace": (SZ, [P, I]),
    "catseg_conv2d_bwd_weight": (I, [P, P]),
    "catseg_gemm_batched": (I, [I, I, I, I, I, P, I, L, P, I, L, P, I, L, I, I, P]),
    "catseg_sum_slabs": (I, [P, P, L, I, I, I, P]),
    "catseg_debug_set_tile": (I, [I, I]),
    "catseg_debug_set_splits": (I, [I]),
    "catseg_debug_set_strided_multi": (I, [I]),
    "catseg_debug_set_lovasz_prune": (I, [I]),
    "catseg_debug_set_wgrad_direct": (I, [I]),
    "catseg_debug_plan_conv": (I, [P, I, P]),
    "catseg_debug_set_b3_tile": (I, [I]),
    "catseg_debug_set_dconv3_blocks": (I, [I]),
    "catseg_debug_set_dconv3_pl_slots": (I, [I]),
    "catseg_debug_set_dconv3_pl_pair": (I, [I]),
    "catseg_debug_set_dwgrad3_pl_blocks": (I, [I]),
    "catseg_debug_set_dwgrad3_pl_form": (I, [I]),
    "catseg_debug_dconv3_pl_occupancy": (I, [I, I]),
    "catseg_debug_dwgrad3_pl_occupancy": (I, [I]),
    "catseg_debug_set_dconv3_spec": (I, [I]),
    "catseg_debug_set_dconv3_alt96": (I, [I]),
    "catseg_aug_pad_flip_u8": (I, [P, P, I, I, I, I, P, I, I, P]),
    "catseg_aug_box_blur": (I, [P, P, I, I, I, I, P, P, P, P]),
    "catseg_aug_color_op": (I, [P, I, I, I, P, P, P, SZ, P]),
    "catseg_split3_elems": (SZ, [L, I]),
    "catseg_split3": (I, [P, I, L, I, P, P]),
    "catseg_split3_weight_t": (I, [P, I, I, I, P, P]),
    "catseg_split3_blocked_elems": (SZ, [L, I]),
    "catseg_split3_blocked": (I, [P, L, I, I, P, P, P]),
    "catseg_split3_weight_blocked": (I, [P, I, I, I, P, P]),
    "catseg_split3_weight_t_blocked": (I, [P, I, I, I, P, P]),
    "catseg_split2h_blocked_elems": (SZ, [L, I]),
    "catseg_split2h_planar_elems": (SZ, [L, I]),
    "catseg_split2h": (I, [P, L, I, I, P, P, P, P]),
    "catseg_split2h_bound": (I, [P, L, I, I, P, P, P, P, P, P, P, P]),
    "catseg_concat_bilinear_split2h": (I, [I, P, P, P, P, P, P, I, I, I, P, P, P]),
    "catseg_stem3_supported": (I, [I, I, I]),
    "catseg_stem3_partial_rows": (I, [I, I, I]),
    "catseg_stem3_wgrad_workspace": (SZ, []),
    "catseg_stem3_fwd": (I, [P, L, L, L, L, I, I, I, P, P, P, I, P, P, P]),
    "catseg_stem3_bwd_weight": (I, [P, L, L, L, L, I, I, I, P, I, P, P, SZ, P]),
    "catseg_stem7_supported": (I, [I, I, I]),
    "catseg_stem7_partial_rows": (I, [I, I, I]),
    "catseg_stem7_fwd": (I, [P, L, L, L, L, I, I, I, P, P, P, I, P, P, P]),
    "catseg_split2h_weight_blocked": (I, [P, I, I, I, P, P, P]),
    "catseg_split2h_weight_t_blocked": (I, [P, I, I, I, P, P, P]),
    "catseg_bias_grad": (I, [P, I, L, I, P, P, SZ, P]),
    "catseg_bn_workspace": (SZ, [L, I]),
    "catseg_bn_train_stats": (I, [P, L, I, I, P, F, F, P, P, P, P, P, SZ, P]),
    "catseg_bn_eval_scale": (I, [I, P, P, F, P, P]),
    "catseg_bn_apply": (I, [P, P]),
    "catseg_bn_backward": (I, [P, P]),
    "catseg_nchw3_to_nhwc4": (I, [P, P, I, I, I, P]),
    "catseg_nchw3_to_nhwc4_norm": (I, [P, P, I, I, I, P, P, P]),
    "catseg_stem_pack_weight": (I, [P, P, I, P]),
    "catseg_stem_unpack_grad": (I, [P, P, I, P]),
    "catseg_axpy2d": (I, [P, I, P, I, L, I, F, I, P]),
    "catseg_add_n_act": (I, [P, P, P, I, P, I, P, L, I, I, P, P]),
    "catseg_relu_bwd": (I, [P, I, P, I, P, I, L, I, P]),
    "catseg_weight_pad_cin": (I, [P, P, I, I, I, I, I, P]),
    "catseg_scale_by_device_scalar": (I, [P, L, P, P]),
    "catseg_maxpool3x3s2_fwd": (I, [P, I, P, I, P, I, I, I, I, I, I, P]),
    "catseg_maxpool3x3s2_bwd": (I, [P, I, P, P, I, I, I, I, I, I, I, P]),
    "catseg_bilinear_fwd": (I, [P, I, P, I, I, I, I, I, I, I, I, I, P]),
    "catseg_bilinear_bwd": (I, [P, I, P, I, I, I, I, I, I, I, I, I, I, P, SZ, P]),
    "catseg_global_avgpool_fwd": (I, [P, I, P, I, I, I, P]),
    "catseg_global_avgpool_bwd": (I, [P, P, I, I, I, I, I, P]),
    "catseg_adaptive_avgpool_fwd": (I, [P, I, P, I, I, I, I, I, P]),
    "catseg_adaptive_avgpool_bwd": (I, [P, P, I, I, I, I, I, I, I, P]),
    "catseg_softmax_spatial_workspace": (SZ, [I, I]),
    "catseg_softmax_spatial_fwd": (I, [P, P, I, I, I, I, P, SZ, P]),
    "catseg_softmax_spatial_bwd": (I, [P, P, P, I, I, I, I, I, P, SZ, P]),
    "catseg_softmax_rows_fwd": (I, [P, P, L, I, I, F, P]),
    "catseg_softmax_rows_bwd": (I, [P, P, P, L, I, I, F, P]),
    "catseg_lovasz_workspace": (SZ, [L, I]),
    "catseg_lovasz_softmax": (I, [P, P, L, I, F, P, P, I, P, SZ, P]),
    "catseg_lovasz_softmax_fwd": (I, [P, P, L, I, F, P, I, P, SZ, P]),
    "catseg_lovasz_softmax_bwd": (I, [P, L, I, F, P, P, I, P, SZ, P]),
    "catseg_ce_workspace": (SZ, [L]),
    "catseg_cross_entropy": (I, [P, P, L, I, L, F, P, P, P, SZ, P]),
    "catseg_ohem_workspace": (SZ, [L]),
    "catseg_ohem_cross_entropy": (I, [P, P, L, I, L, F, L, F, P, P, P, SZ, P]),
    "catseg_overlap_workspace": (SZ, [L, I]),
    "catseg_overlap_fwd": (I, [P, P, L, I, L, I, I, I, P, P, P, P, P, SZ, P]),
    "catseg_overlap_bwd": (I, [P, P, L, I, L, P, P, P, P]),
    "catseg_focal_workspace": (SZ, [L]),
    "catseg_focal_fwd": (I, [P, P, L, I, F, P, P, P, P, SZ, P]),
    "catseg_focal_bwd": (I, [P, P, L, I, F, P, P, P, P]),
    "catseg_ingest_u8": (I, [P, P, I, I, I, P, P, I, I, P, P, P, P, P, P]),
    "catseg_ingest_warp_u8": (I, [P, P, I, I, I, P, P, P, I, I, P, I, I, I, I, P, P, P, P, P, P, P]),
    "catseg_resize_nearest": (I, [P, I, P, I, I, I, I, I, I, I, I, I, F, P]),
    "catseg_ensemble_merge": (I, [P, P, I, L, I, I, P, I, P, P]),
    "catseg_egress_u8": (I, [P, I, I, I, I, I, I, I, I, F, I, P, P, P, I, P, P, I, P, P, P, P, P]),
    "catseg_confusion_matrix": (I, [P, P, L, I, P, P]),
    "catseg_adam_step": (I, [P, P, P, P, L, F, F, F, F, I, F, P]),
    "catseg_pconv1_supported": (I, [I, I]),
    "catseg_pconv1_wimg_bytes": (SZ, [I, I]),
    "catseg_pconv1_prep_batch": (I, [P, I, P, P, P, P]),
    "catseg_pconv1": (I, [L, I, I, P, I, P, P, P, P, P, I, I, P, SZ, P, P, P]),
    "catseg_pconv1_wgrad_supported": (I, [I, I]),
    "catseg_pconv1_wgrad_workspace": (SZ, [L, I, I]),
    "catseg_pconv1_wgrad": (I, [L, I, I, P, I, P, P, I, P, P, P, SZ, P]),
    "catseg_debug_set_pconv1_wgrad_blocks": (I, [I]),
    "catseg_debug_set_h2w_waves": (I, [I]),
    "catseg_debug_set_h2w_slow_epilogue": (I, [I]),
    "catseg_debug_set_bilinear_bwd_fused": (I, [I]),
    "catseg_gconv_supported": (I, [P]),
    "catseg_gconv_class_bytes": (SZ, [P]),
    "catseg_gconv_wimg_bytes": (SZ, [P, I]),
    "catseg_gconv_entries": (I, [P, I, L, L, P]),
    "catseg_gconv_fwd": (I, [P, P, P, P, P, P, P, P, SZ, P, P, P]),
    "catseg_gconv_bwd_data": (I, [P, P, P, P, P, P, I, P]),
    "catseg_gconv_wgrad_supported": (I, [P]),
    "catseg_gconv_wgrad_workspace": (SZ, [P]),
    "catseg_gconv_bwd_weight": (I, [P, P, P, P, P, P, P, SZ, P]),
    "catseg_adam_hyper": (None, [F, F, F, I, F, P]),
    "catseg_adam_step_dev": (I, [P, P, P, P, L, P, F, F, F, P]),
    "catseg_lds_limits": (I, [P, P]),
    "catseg_pointrend_uncertainty": (I, [P, I, P, L, I, P]),
    "catseg_pointrend_topk_workspace": (SZ, [I, L]),
    "catseg_pointrend_topk": (I, [P, I, L, I, P, P, SZ, P]),
    "catseg_pointrend_gather": (I, [P, P]),
    "catseg_pointrend_scatter": (I, [P, I, P, I, I, L, P, I, I, P]),
    "catseg_pointrend_draw": (I, [P, P, I, I, P, P]),
    "catseg_pointrend_point_uncertainty": (I, [P, I, I, I, I, I, P, I, P, P]),
    "catseg_pointrend_gather_at": (I, [P, P, P]),
    "catseg_pointrend_compose": (I, [P, I, P, I, P, I, I, I, I, P, I, I, P, P, P, P]),
    "catseg_pointrend_gather_bwd": (I, [P, P]),
    "catseg_pointrend_scatter_last": (I, [P, I, P, I, I, L, P, I, I, P]),
    "catseg_pointrend_scatter_bwd": (I, [P, I, P, I, I, L, P, I, I, I, P]),
    # include/catseg_cropfreq.h
    "catseg_crop_freq_workspace": (SZ, [I, I, I, I]),
    "catseg_crop_freq_pick": (I, [P, I, I, I, P, P, P, I, I, I, P, P, P, P, P, P, SZ, P]),
    # include/catseg_ingest_tables.h: the plain entry's arguments with (T, table_of_frame) after the tables
    "catseg_ingest_u8_tables": (I, [P, P, I, I, I, P, I, P, P, I, I, P, P, P, P, P, P]),
    "catseg_ingest_warp_u8_tables": (I, [P, P, I, I, I, P, I, P, P, P, I, I, P, I, I, I, I, P, P, P, P, P, P, P]),
    "catseg_crop_freq_pick_tables": (I, [P, I, I, I, P, I, P, P, P, I, I, I, P, P, P, P, P, P, SZ, P]),
    # include/catseg_census.h
    "catseg_label_census_u8": (I, [P, I, I, I, P, I, P, I, P]),
    "catseg_iou_ema": (I, [P, P, I, F, F, P, P, P]),
    # include/catseg_optim.h
    "catseg_optim_hyper": (None, [I, F, F, F, F, I, P, P, P]),
    "catseg_adam_step_ex": (I, [P, P, P, P, P, L, P, I, P, P, F, F, F, I, P, P]),
    "catseg_sgd_step": (I, [P, P, P, L, P, I, P, P, F, I, I, P, P]),
    "catseg_grad_norm_workspace": (SZ, [L]),
    "catseg_grad_norm": (I, [P, L, F, P, F, P, SZ, P, P]),
    "catseg_optim_grid_cap": (I, []),
    # include/catseg_ema.h
    "catseg_ema_update": (I, [P, P, L, F, P, P]),
    "catseg_ema_swap": (I, [P, P, L, P]),
    "catseg_ema_table": (I, [P, I, P, I, F, P, P]),
    "catseg_ema_grid_cap": (I, []),
}
# include/ext/catseg_contrast.h: the entry points of the dense contrastive loss, a table of their own beside the core surface (EXPORTS is
# what the headers directly under include/ declare)
_SIGS_CONTRAST = {
    "catseg_contrast_pick_workspace": (SZ, [I, I, I, I]),
    "catseg_contrast_pick": (I, [P, I, I, I, I, I, I, I, P, P, I, P, P, P, P, SZ, P]),
    "catseg_contrast_gather": (I, [P, I, L, I, P, I, F, P, P, P]),
    "catseg_contrast_rows": (I, [P, I, I, P, P, I, F, P, P, P]),
    "catseg_contrast_finalize": (I, [P, I, P, P, P]),
    "catseg_contrast_scatter_bwd": (I, [P, P, I, P, P, I, I, P, F, P, L, P]),
}
for _name, (_res, _args) in list(_SIGS.items()) + list(_SIGS_CONTRAST.items()):
    _fn = getattr(lib, _name)  # AttributeError here = header / library mismatch
    _fn.restype = _res
    _fn.argtypes = _args

EXPORTS = tuple(_SIGS)

if os.environ.get("CATSEG_SYNC"):  # debugging aid: synchronise after every entry point so a device fault names its launch
    class _SyncLib:
        def __init__(self, inner):
            self._inner = inner

        def __getattr__(self, name):
            fn = getattr(self._inner, name)
            if name in ("catseg_last_error", "catseg_version") or name.endswith("_workspace"):
                return fn

            def fields(st):     # (a descriptor's geometry is a nested structure)
                return {f: fields(v) if isinstance(v, C.Structure) else v for f, v in ((f, getattr(st, f)) for f, _ in st._fields_)}

            def call(*a):
                desc = [fields(x._obj) for x in a if isinstance(getattr(x, "_obj", None), C.Structure)]
                print("[catseg]", name, desc, [x for x in a if isinstance(x, (int, float))], flush=True)
                rc = fn(*a)
                torch.cuda.synchronize()
                return rc
            return call

    lib = _SyncLib(lib)


class CatsegError(RuntimeError):
    pass


def check(rc):
    if rc != 0:
        raise CatsegError("libcatseg_hip: error %d: %s" % (rc, lib.catseg_last_error().decode()))


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return 0 if t is None else t.data_ptr()
