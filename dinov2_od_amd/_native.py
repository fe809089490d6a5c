"""ctypes binding of libdinodet.so (include/dinodet.h).  PyTorch is used only for device
memory (tensor.data_ptr()) and the current HIP stream; no torch type crosses the ABI.

There is NO fallback: if the library is missing or a GPU op is requested without it,
loading raises.  Build with `python -m dinov2_od_amd._build`.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DINODET_LIB") or os.path.join(_HERE, "lib", "libdinodet.so")      # DINODET_LIB: another build of the same ABI (A/B runs)

DOD_F32, DOD_BF16 = 0, 1
PREC = {"fp32": 0, "bf16": 1, "fp8": 2, "bf16x3": 3, "fp16x2": 4}
ACT = {"none": 0, "relu": 1, "gelu": 2, "sigmoid": 3, "swiglu_pairs": 4}
LN_FORM = {"f32": 0, "bf16": 1, "f32_bf16": 2, "pair": 3, "h2": 4, "fp8": 5, "fp8_mx": 6, "f32_s3": 7}      # enum DOD_LN_*
PW = {"gelu_bwd": 0, "swiglu_bwd": 1, "relu_drop_bwd": 2, "dropout_add": 3, "sigmoid_bwd4": 4}      # enum dod_pointwise_op


class DodConfig(C.Structure):
    _fields_ = [
        ("hidden", C.c_int32), ("layers", C.c_int32), ("heads", C.c_int32), ("swiglu", C.c_int32),
        ("patch", C.c_int32), ("pos_grid", C.c_int32), ("ffn_hidden", C.c_int32), ("ln_eps", C.c_float),
        ("lora_r", C.c_int32), ("lora_alpha", C.c_float), ("target_dim", C.c_int32),
        ("num_queries", C.c_int32), ("dec_hidden", C.c_int32), ("dec_heads", C.c_int32),
        ("dec_layers", C.c_int32), ("num_classes", C.c_int32), ("dim_feedforward", C.c_int32),
        ("n_points", C.c_int32), ("use_deformable", C.c_int32), ("dec_ln_eps", C.c_float),
        ("precision", C.c_int32),
    ]


_P, _I, _F, _SZ, _I64 = C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_int64


class DodDetection(C.Structure):
    """struct dod_detection (include/dinodet.h): one COCO-style record of evaluate_coco, utils.py:225-233"""
    _fields_ = [("image_id", C.c_int64), ("category_id", C.c_int32), ("query", C.c_int32), ("bbox", C.c_float * 4),
                ("score", C.c_float), ("reserved", C.c_int32)]

# struct dod_dec_train_params: 31 device pointers in this order (the same struct carries the gradient accumulators)
DEC_TRAIN_FIELDS = ["query_embed", "class_w", "class_b", "bb0_w", "bb0_b", "bb2_w", "bb2_b", "in_proj_w", "in_proj_b", "out_proj_w",
                    "out_proj_b", "norm1_w", "norm1_b", "norm2_w", "norm2_b", "norm3_w", "norm3_b", "lin1_w", "lin1_b", "lin2_w", "lin2_b",
                    "refp_w", "refp_b", "off_w", "off_b", "aw_w", "aw_b", "vp_w", "vp_b", "op_w", "op_b"]


class DodDecTrainParams(C.Structure):
    _fields_ = [(f, C.c_void_p) for f in DEC_TRAIN_FIELDS]


DENSE_LAYER_FIELDS = ["sa_in_w", "sa_in_b", "sa_out_w", "sa_out_b", "ca_in_w", "ca_in_b", "ca_out_w", "ca_out_b", "lin1_w", "lin1_b", "lin2_w", "lin2_b",
                      "norm1_w", "norm1_b", "norm2_w", "norm2_b", "norm3_w", "norm3_b"]


class DodDenseLayerParams(C.Structure):
    _fields_ = [(f, C.c_void_p) for f in DENSE_LAYER_FIELDS]


class DodDenseDecTrainParams(C.Structure):
    _fields_ = [("nlayers", C.c_int32), ("reserved", C.c_int32), ("layers", C.POINTER(DodDenseLayerParams))] + \
               [(f, C.c_void_p) for f in ("query_embed", "class_w", "class_b", "bb0_w", "bb0_b", "bb2_w", "bb2_b")]


class DodLoraLinear(C.Structure):
    _fields_ = [("w", C.c_void_p), ("b", C.c_void_p), ("A", C.c_void_p), ("Bm", C.c_void_p)]


class DodBbBlockParams(C.Structure):
    _fields_ = [(f, C.c_void_p) for f in ("ln1_w", "ln1_b", "ln2_w", "ln2_b", "ls1", "ls2")] + \
               [(f, DodLoraLinear) for f in ("q", "k", "v", "o", "fc1", "fc2")]


class DodBbTailParams(C.Structure):
    _fields_ = [("nblocks", C.c_int32), ("reserved", C.c_int32), ("blocks", C.POINTER(DodBbBlockParams)),
                ("lnf_w", C.c_void_p), ("lnf_b", C.c_void_p), ("proj_w", C.c_void_p), ("proj_b", C.c_void_p)]


class DodOptimTensor(C.Structure):
    """struct dod_optim_tensor (include/dinodet.h): one parameter of the optimizer step"""
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("n", C.c_int64),
                ("step_size", C.c_float), ("bc2_sqrt", C.c_float)]


class DodOptimOptions(C.Structure):
    """struct dod_optim_options (include/dinodet.h): what dod_optim_step takes beside the lists"""
    _fields_ = [("beta1", C.c_double), ("beta2", C.c_double), ("weight_decay", C.c_double), ("ema_w", C.c_double), ("eps", C.c_float),
                ("max_norm", C.c_float), ("skip_nonfinite", C.c_int32), ("norm_ready", C.c_int32), ("total_norm_dev", C.c_void_p),
                ("skipped_dev", C.c_void_p)]


class DodOptimEmaTensor(C.Structure):
    """struct dod_optim_ema_tensor (include/dinodet.h): one (average, parameter) pair of dod_optim_ema_update"""
    _fields_ = [("e", C.c_void_p), ("p", C.c_void_p), ("n", C.c_int64)]


class DodLnFold(C.Structure):
    """struct dod_ln_fold (include/dinodet.h): the folded-LayerNorm legs of dod_op_linear_ln"""
    _fields_ = [("stats", C.c_void_p), ("csum", C.c_void_p), ("op_out", C.c_void_p), ("part", C.c_void_p), ("shift", C.c_void_p),
                ("part_in", C.c_void_p), ("stats_out", C.c_void_p), ("eps", C.c_float)]


class DodDrawLayer(C.Structure):
    """struct dod_draw_layer (include/dinodet.h): one layer of boxes of dod_draw_detections"""
    _fields_ = [("boxes", C.c_void_p), ("counts", C.c_void_p), ("labels", C.c_void_p), ("scores", C.c_void_p), ("K", C.c_int32),
                ("format", C.c_int32), ("score_threshold", C.c_float), ("use_palette", C.c_int32), ("color", C.c_uint8 * 4)]


class DodDrawStyle(C.Structure):
    """struct dod_draw_style (include/dinodet.h)"""
    _fields_ = [("thickness", C.c_int32), ("fill_alpha", C.c_int32), ("font_scale", C.c_int32), ("palette_size", C.c_int32),
                ("palette", C.c_void_p), ("names", C.c_void_p), ("n_names", C.c_int32), ("name_len", C.c_int32), ("font", C.c_void_p)]


class DodTrackParams(C.Structure):
    """struct dod_track_params (include/dinodet.h): the thresholds of dod_track_update"""
    _fields_ = [("track_thresh", C.c_float), ("low_thresh", C.c_float), ("new_thresh", C.c_float), ("match_thresh", C.c_float),
                ("second_thresh", C.c_float), ("tentative_thresh", C.c_float), ("max_age", C.c_int32), ("fuse_score", C.c_int32),
                ("class_aware", C.c_int32)]


class DodTrackAppParams(C.Structure):
    """struct dod_track_app_params (include/dinodet.h): the gates and the momentum of dod_track_update_app / dod_track_embed_commit"""
    _fields_ = [("appearance_thresh", C.c_float), ("proximity_thresh", C.c_float), ("momentum", C.c_float)]


# include/dinodet_tuning.h: exported by -DDINODET_TUNING builds only (tools/ load one through DINODET_LIB); bound when present
TUNING_SYMBOLS = {
    "dod_debug_gemm_stamps": (_I, [_P]),
    "dod_debug_pp_stamps": (_I, [_P]),
    "dod_debug_attn_stamps": (_I, [_P]),
    "dod_debug_mfma_peak": (_I, [_I, _I, _I, _P, _P]),
    "dod_debug_mfma_valu_probe": (_I, [_I, _I, _I, _I, _P, _P]),
}

# name -> (restype, argtypes): every symbol include/dinodet.h declares
SYMBOLS = {
    "dod_create": (_I, [C.POINTER(DodConfig), C.POINTER(_P)]),
    "dod_destroy": (None, [_P]),
    "dod_last_error": (C.c_char_p, [_P]),
    "dod_set_weight": (_I, [_P, C.c_char_p, _P, C.POINTER(C.c_int64), _I, _I]),
    "dod_finalize_weights": (_I, [_P, _P]),
    "dod_prepare": (_I, [_P, _I, _I, _P]),
    "dod_workspace_bytes": (_SZ, [_P, _I, _I, _I]),
    "dod_num_tokens": (_I, [_P, _I, _I]),
    "dod_forward": (_I, [_P, _P, _I, _I, _I, _P, _P, _SZ, _P]),
    "dod_forward_mem": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _SZ, _P]),
    "dod_forward_u8": (_I, [_P, _P, _I, _I, _I, _P, _P, _SZ, _P]),
    "dod_backbone_forward": (_I, [_P, _P, _I, _I, _I, _P, _P, _SZ, _P]),
    "dod_backbone_prefix": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _SZ, _P]),
    "dod_decoder_forward": (_I, [_P, _P, _I, _I, _P, _P, _SZ, _P]),
    "dod_decoder_workspace_bytes": (_SZ, [_P, _I, _I]),
    "dod_set_tap": (_I, [_P, _I, _P]),
    "dod_profile": (_I, [_P, _I]),
    "dod_profile_read": (_I, [_P, _I, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "dod_op_linear": (_I, [_I, _P, _I, _P, _I, _I, _I, _I, _P, _P, _P, _I, _P, _I, _I, _I, _P]),
    "dod_op_gemm_f32x": (_I, [_P, _I, _I, C.c_longlong, C.c_longlong, _P, _I, _I, C.c_longlong, C.c_longlong, _P, _I, C.c_longlong, C.c_longlong,
                         _I, _I, _I, _I, _I, _F, _I, _I, _P]),
    "dod_op_gemm_f32x3": (_I, [_P, _I, _I, C.c_longlong, C.c_longlong, _P, _I, _I, C.c_longlong, C.c_longlong, _P, _I, C.c_longlong, C.c_longlong,
                          _I, _I, _I, _I, _I, _F, _I, _I, _P]),
    "dod_op_linear_f32x3": (_I, [_P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _P, _I, _I, _P]),
    "dod_op_linear_fp8": (_I, [_P, _I, _P, _P, _I, _P, _I, _I, _I, _P, _P, _P, _I, _P, _I, _I, _I, _P]),
    "dod_op_quant_rows_fp8": (_I, [_P, _I, _I, _I, _I, _P, _I, _P, _P]),
    "dod_op_quant_mx_fp8": (_I, [_P, _I, _I, _I, _I, _P, _I, _P, _P]),
    "dod_op_linear_fp8_glu_mx": (_I, [_P, _I, _P, _P, _I, _P, _I, _I, _I, _P, _P, _I, _P, _P]),
    "dod_op_linear_fp8_mx": (_I, [_P, _I, _P, _P, _I, _P, _I, _I, _I, _P, _P, _P, _I, _P, _I, _I, _I, _P]),
    "dod_op_linear_fp8_mx2": (_I, [_P, _I, _P, _P, _I, _P, _I, _I, _I, _P, _P, _P, _I, _P, _I, _I, _I, _P, _P]),
    "dod_op_split_pair": (_I, [_P, _I, _I, _I, _P, _P]),
    "dod_op_linear_x3": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _I, _P, _I, _I, _I, _P]),
    "dod_op_attention_x3": (_I, [_P, _P, _I, _I, _I, _F, _P]),
    "dod_op_attention_x3_h2": (_I, [_P, _P, _I, _I, _I, _F, _P]),
    "dod_op_split_h2": (_I, [_P, _I, _I, _I, _P, _P, _P]),
    "dod_op_linear_h2": (_I, [_P, _P, _P, _I, _I, _I, _P, _P, _P, _I, _P, _I, _I, _I, _P]),
    "dod_op_layernorm": (_I, [_P, _P, _P, _P, _F, _I, _I, _P, _I, _P]),
    "dod_op_layernorm_form": (_I, [_P, _P, _P, _P, _F, _I, _I, _I, _P, _P, _P]),
    "dod_op_swiglu": (_I, [_P, _P, _I, _I, _I, _P]),
    "dod_op_split3": (_I, [_P, _I, _I, _I, _I, _P, _P]),
    "dod_op_deform_sample_ex": (_I, [_P, _I, _I, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P]),
    "dod_op_linear_ln": (_I, [_I, _P, _P, _P, _I, _I, _I, _P, _P, _P, _I, _P, _I, _I, _I, C.POINTER(DodLnFold), _P]),
    "dod_op_rowstats": (_I, [_P, _I, _I, _F, _P, _I, _P, _P]),
    "dod_op_ln_finalize": (_I, [_P, _I, _I, _F, _P, _P]),
    "dod_op_attention_bf16": (_I, [_P, _P, _I, _I, _I, _F, _P]),
    "dod_op_attention_bf16_mx": (_I, [_P, _P, _P, _I, _I, _I, _F, _P]),
    "dod_op_attention_f32": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _F, _P]),
    "dod_op_deform_sample": (_I, [_P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    "dod_op_pos_resize": (_I, [_P, _I, _I, _I, _I, _P, _P]),
    "dod_op_im2col": (_I, [_P, _I, _I, _I, _I, _I, _P, _I, _P]),
    "dod_postprocess_workspace_bytes": (_SZ, [_I, _I, _I]),
    "dod_postprocess": (_I, [_P, _I, _I, _I, _P, _F, _P, C.c_int64, _P, _P, _SZ, _P]),
    "dod_detect_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "dod_detect": (_I, [_P, _I, _I, _I, _I, _P, _F, _I, _F, _I, _I, _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "dod_detect_views_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "dod_detect_views": (_I, [_P, _I, _I, _I, _I, _P, _P, _P, _P, _I, _F, _I, _F, _I, _I, _I, _F, _P, _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "dod_fuse_views_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "dod_fuse_views": (_I, [_P, _I, _I, _I, _I, _P, _P, _P, _P, _I, _F, _I, _F, _I, _I, _F, _I, _P, _P, _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "dod_draw_detections": (_I, [_P, _I, _I, _I, _I, C.POINTER(DodDrawLayer), C.POINTER(DodDrawLayer), C.POINTER(DodDrawStyle), _P, _P]),
    "dod_preprocess": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "dod_preprocess_u8": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "dod_preprocess_aug": (_I, [_P, _P, _P, _P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P]),
    "dod_preprocess_aug_u8": (_I, [_P, _P, _P, _P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P]),
    "dod_preprocess_compose": (_I, [_P, _P, _P, _P, _I, _P, _P, _I, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "dod_preprocess_compose_u8": (_I, [_P, _P, _P, _P, _I, _P, _P, _I, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "dod_preprocess_warp": (_I, [_P, _P, _P, _P, _I, _P, _P, _I, _I, _I, _P, _P]),
    "dod_preprocess_warp_u8": (_I, [_P, _P, _P, _P, _I, _P, _P, _I, _I, _I, _P, _P]),
    "dod_jpeg_entropy_host": (_I, [_P, _I64, _P, _I, _I, _P, _I, _P, _I64, _P]),
    "dod_jpeg_entropy_device": (_I, [_P, _I64, _P, _I, _P, _I, _P, _I, _P, _I64, _P, _P]),
    "dod_jpeg_idct": (_I, [_P, _I64, _P, _I, _P, _I, _P, _P]),
    "dod_jpeg_color": (_I, [_P, _P, _I, _I64, _P, _P]),
    "dod_match_cost": (_I, [_P, _I, _I, _I, _P, _P, _P, _I, _F, _F, _F, _F, _F, _I, _P, _P]),
    "dod_match_assign_workspace_bytes": (_SZ, [_I, _I, _I]),
    "dod_match_assign": (_I, [_P, _P, _I, _I, _I, _P, _I, _P, _P, _P, _SZ, _P]),
    "dod_track_state_bytes": (_SZ, [_I, _I]),
    "dod_track_workspace_bytes": (_SZ, [_I, _I, _I]),
    "dod_track_reset": (_I, [_P, _I, _I, _P, _P]),
    "dod_track_update": (_I, [_P, _I, _I, _P, _P, _P, _P, _I, C.POINTER(DodTrackParams), _P, _P, _P, _SZ, _P]),
    "dod_track_export": (_I, [_P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "dod_roi_embed": (_I, [_P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _I, _I, _P, _P]),
    "dod_track_embed_dots": (_I, [_P, _P, _I, _I, _I, _I, _P, _P]),
    "dod_track_update_app": (_I, [_P, _I, _I, _P, _P, _P, _P, _I, C.POINTER(DodTrackParams), C.POINTER(DodTrackAppParams), _P, _P, _P, _P, _P, _SZ, _P]),
    "dod_track_embed_commit": (_I, [_P, _P, _P, _I, _I, _I, _I, _F, _P]),
    "dod_coco_eval_workspace_bytes": (_SZ, [_I64, _I, _I, _I64]),
    "dod_coco_eval_set_gt": (_I, [_P, _SZ, _I64, _I, _I, _I64, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "dod_coco_eval_reset": (_I, [_P, _SZ, _I64, _I, _I, _I64, _P]),
    "dod_coco_eval_append": (_I, [_P, _SZ, _I64, _I, _I, _I64, _P, _P, _I64, _P]),
    "dod_coco_eval_append_host": (_I, [_P, _SZ, _I64, _I, _I, _I64, _P, _I64, _P]),
    "dod_coco_eval_evaluate": (_I, [_P, _SZ, _I64, _I, _I, _I64, _P, _P, _P, _P, _P, _P]),
    "dod_coco_eval_matches": (_I, [_P, _SZ, _I64, _I, _I, _I64, _I64, _P, _P, _P, _P, _I, _P, _P, _P]),
    "dod_coco_eval_append_detections": (_I, [_P, _SZ, _I64, _I, _I, _I64, _P, _P, _P, _P, _I, _I, _P, _P, _I, _P]),
    "dod_coco_eval_confusion": (_I, [_P, _SZ, _I64, _I, _I, _I64, C.c_double, C.c_double, _P, _P]),
    "dod_op_sort_pairs_workspace_bytes": (_SZ, [_I64]),
    "dod_op_sort_pairs_u64": (_I, [_P, _P, _P, _P, _I64, _I, _I, _P, _SZ, _P]),
    "dod_set_criterion_workspace_bytes": (_SZ, [_I, _I, _I]),
    "dod_set_criterion_forward": (_I, [_P, C.c_int64, _P, C.c_int64, _I, _I, _I, _P, _P, _I, _P, _I, _P, _F, _F, _P, _P, _P, _SZ, _P]),
    "dod_set_criterion_backward": (_I, [_P, C.c_int64, _P, C.c_int64, _I, _I, _I, _P, _P, _I, _P, _I, _P, _F, _F, _P, _P, _P, _P, _P]),
    "dod_set_criterion_layers_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "dod_set_criterion_layers_forward": (_I, [_P, C.c_int64, _P, C.c_int64, _I, _I, _I, _I, _P, _P, _I, _P, _I, _P, _F, _F, _P, _P, _P, _SZ, _P]),
    "dod_set_criterion_layers_backward": (_I, [_P, C.c_int64, _P, C.c_int64, _I, _I, _I, _I, _P, _P, _I, _P, _I, _P, _F, _F, _P, _P, _P, _P, _P]),
    "dod_decoder_train_aux_tape_bytes": (_SZ, [C.POINTER(DodConfig), _I, _I]),
    "dod_decoder_train_aux_workspace_bytes": (_SZ, [C.POINTER(DodConfig), _I, _I]),
    "dod_decoder_train_aux_forward": (_I, [C.POINTER(DodConfig), _P, _P, _I, _I, _F, C.c_uint64, _P, _P, _SZ, _P, _SZ, _P]),
    "dod_decoder_train_aux_backward": (_I, [C.POINTER(DodConfig), _P, _P, _I, _I, _F, C.c_uint64, _P, _P, _SZ, _P, _P, _P, _SZ, _P]),
    "dod_decoder_train_tape_bytes": (_SZ, [C.POINTER(DodConfig), _I, _I]),
    "dod_decoder_train_workspace_bytes": (_SZ, [C.POINTER(DodConfig), _I, _I]),
    "dod_decoder_train_forward": (_I, [C.POINTER(DodConfig), _P, _P, _I, _I, _F, C.c_uint64, _P, _P, _SZ, _P, _SZ, _P]),
    "dod_decoder_train_backward": (_I, [C.POINTER(DodConfig), _P, _P, _I, _I, _F, C.c_uint64, _P, _P, _SZ, _P, _P, _P, _SZ, _P]),
    "dod_decoder_train_last_error": (C.c_char_p, []),
    "dod_dense_decoder_train_tape_bytes": (_SZ, [C.POINTER(DodConfig), _I, _I]),
    "dod_dense_decoder_train_workspace_bytes": (_SZ, [C.POINTER(DodConfig), _I, _I]),
    "dod_dense_decoder_train_forward": (_I, [C.POINTER(DodConfig), _P, _P, _I, _I, _F, C.c_uint64, _P, _P, _SZ, _P, _SZ, _P]),
    "dod_dense_decoder_train_backward": (_I, [C.POINTER(DodConfig), _P, _P, _I, _I, _F, C.c_uint64, _P, _P, _SZ, _P, _P, _P, _SZ, _P]),
    "dod_backbone_tail_tape_bytes": (_SZ, [C.POINTER(DodConfig), _I, _I, _I]),
    "dod_backbone_tail_workspace_bytes": (_SZ, [C.POINTER(DodConfig), _I, _I, _I]),
    "dod_backbone_tail_train_forward": (_I, [C.POINTER(DodConfig), _P, _P, _I, _I, _P, _P, _SZ, _P, _SZ, _P]),
    "dod_backbone_tail_train_backward": (_I, [C.POINTER(DodConfig), _P, _I, _I, _P, _P, _SZ, _P, _P, _SZ, _P]),
    "dod_op_layernorm_bwd": (_I, [_P, _P, _P, _F, _I, _I, _P, _P, _P, _P]),
    "dod_op_attention_f32_vjp_workspace_bytes": (_SZ, [_I, _I, _I, _I, _I, _I]),
    "dod_op_attention_f32_vjp": (_I, [_P, _I, _P, _P, _I, _P, _P, _I, _P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _F, _I, _F, C.c_uint64, _P, _SZ, _P]),
    "dod_op_deform_sample_bwd": (_I, [_P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P]),
    "dod_op_lora_grads_workspace_bytes": (_SZ, [_I, _I]),
    "dod_op_lora_grads": (_I, [_P, _I, _P, _I, _I, _P, _P, _I, _I, _F, _P, _P, _P, _SZ, _P]),
    "dod_op_train_pointwise": (_I, [_I, _P, _P, _P, _SZ, _I, _F, C.c_uint64, _P]),
    "dod_op_colsum_add": (_I, [_P, _I, _I, _I, _P, _P]),
    "dod_optim_workspace_bytes": (_SZ, [_I, _I64]),
    "dod_optim_clip_grad_norm": (_I, [_P, _I, _F, _P, _P, _SZ, _P]),
    "dod_optim_adam_step": (_I, [_P, _I, C.c_double, C.c_double, _F, C.c_double, _F, _P, _P, _SZ, _P]),
    "dod_optim_step": (_I, [_P, _P, _P, _I, _P, _P, _SZ, _P]),
    "dod_optim_ema_update": (_I, [_P, _I, C.c_double, _P]),
    "dod_optim_last_error": (C.c_char_p, []),
    "dod_reserve_gemm_scratch": (_I, [C.c_size_t]),
    "dod_test_set_option": (_I, [C.c_char_p, _I]),
    "dod_test_counter": (C.c_long, [C.c_char_p]),
    "dod_test_gemm_plan": (_I, [_I, _I, _I, _I, C.c_uint, _I, C.c_size_t, _P, _I]),
    "dod_test_packed_info": (_I, [_P, C.c_char_p, _P]),
    "dod_test_packed_copy": (_I, [_P, C.c_char_p, _I, _P, C.c_size_t, _P]),
    "dod_version": (C.c_char_p, []),
    "dod_abi_version": (_I, []),
    "dod_device_count": (_I, []),
}

_lib = None
ABI_VERSION = 7     # include/dinodet.h DOD_ABI_VERSION


def lib():
    """Load the library (once).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        # libdinodet.so must share ONE HIP runtime with PyTorch (device pointers and streams cross the
        # ABI).  The PyTorch wheel bundles its own libamdhip64.so and publishes it in the global symbol
        # scope; importing torch first makes libdinodet's hip* references bind to that copy.  Loaded the
        # other way round, the process would hold two HIP runtimes.
        import torch  # noqa: F401
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: the HIP extension is required (no CPU fallback). "
                "Build it with `python -m dinov2_od_amd._build`.")
        L = C.CDLL(LIB_PATH)
        other = bool(os.environ.get("DINODET_LIB"))      # an A/B build may be an earlier ABI revision: its missing entry points stay unbound
        for name, (res, args) in SYMBOLS.items():
            if other and not hasattr(L, name):
                continue
            fn = getattr(L, name)   # AttributeError if a declared symbol is not exported
            fn.restype = res
            fn.argtypes = args
        for name, (res, args) in TUNING_SYMBOLS.items():
            if hasattr(L, name):
                fn = getattr(L, name)
                fn.restype = res
                fn.argtypes = args
        if L.dod_abi_version() != ABI_VERSION and not other:
            raise RuntimeError(f"{LIB_PATH} has ABI revision {L.dod_abi_version()}, this binding expects {ABI_VERSION}: rebuild it "
                               "(`python -m dinov2_od_amd._build --force`)")
        try:
            if torch.cuda.is_available() and L.dod_device_count() <= 0:
                raise RuntimeError("libdinodet.so is bound to a different HIP runtime than PyTorch "
                                   "(it sees no device): import torch before loading it")
        except AttributeError:
            pass
        _lib = L
    return _lib


class DodGemmStep(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("form", "row0", "rows", "kslices", "regmath", "gm")]


def gemm_plan(family, M, N, K, epi_flags, cus, scratch_bytes):
    """dod_test_gemm_plan (include/dinodet.h): the launches the inference GEMM launchers would make, as (form, row0, rows, kslices, regmath, gm)
    tuples in launch order.  Host only: no device is touched"""
    steps = (DodGemmStep * 4)()
    n = lib().dod_test_gemm_plan(family, M, N, K, epi_flags, cus, scratch_bytes, steps, 4)
    if n < 0:
        raise ValueError(f"dod_test_gemm_plan rejected family={family} M={M} N={N} K={K} cus={cus}")
    return [(s.form, s.row0, s.rows, s.kslices, s.regmath, s.gm) for s in steps[:n]]


PK_FORMAT = {-1: "absent", 0: "f32", 1: "bf16", 2: "pair", 3: "h2w", 4: "e4m3_rows", 5: "e4m3_mx", 6: "split3w"}      # enum dod_packed_format
PK_ARRAY = {"w": 0, "bias": 1, "csum": 2, "wscale": 3, "wbs": 4, "wexp": 5}                                           # enum dod_packed_array


class DodPackedInfo(C.Structure):
    _fields_ = [("format", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32), ("arrays", C.c_int32), ("pitch", C.c_int64),
                ("bytes", C.c_int64 * 6), ("glu", C.c_int32), ("fold", C.c_int32), ("vp_alias", C.c_int32), ("reserved", C.c_int32)]


def packed_info(handle, name):
    """dod_test_packed_info (include/dinodet.h) -> dict(format, rows, cols, pitch, arrays: {name: bytes}, glu, fold, vp_alias)"""
    info = DodPackedInfo()
    check(lib().dod_test_packed_info(handle, name.encode(), C.byref(info)), handle)
    arrays = {k: int(info.bytes[a]) for k, a in PK_ARRAY.items() if info.arrays >> a & 1}
    return dict(format=PK_FORMAT[info.format], rows=info.rows, cols=info.cols, pitch=int(info.pitch), arrays=arrays, glu=bool(info.glu),
                fold=bool(info.fold), vp_alias=info.vp_alias)


def packed_array(handle, name, array="w", info=None):
    """dod_test_packed_copy: one array of a packed operand as a uint8 CUDA tensor of exactly its bytes (copied on torch's current stream)"""
    import torch
    info = info or packed_info(handle, name)
    out = torch.empty(info["arrays"][array], dtype=torch.uint8, device="cuda")
    check(lib().dod_test_packed_copy(handle, name.encode(), PK_ARRAY[array], ptr(out), out.numel(), stream_ptr()), handle)
    return out


def set_option(name, value):
    """dod_test_set_option (include/dinodet.h): a process-wide test option; -1 hands the shipped behaviour back"""
    check(lib().dod_test_set_option(name.encode(), int(value)))


class DodError(RuntimeError):
    pass


_EXC = {1: ValueError, 2: KeyError, 3: RuntimeError, 4: RuntimeError}


def check(rc, handle=None, exc=_EXC, default=DodError):
    """raise the exception of a non-zero dod_status with the message of the handle, or (no handle) of the calling thread;
    exc / default: the status -> exception type mapping of a call site whose types are not _EXC's"""
    if rc != 0:
        msg = lib().dod_last_error(handle)
        msg = msg.decode() if msg else f"dinodet error {rc}"
        raise exc.get(rc, default)(msg)


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
