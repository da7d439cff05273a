"""ctypes binding of the C ABI declared in include/controlanimate_hip.h.

The product path has NO CPU / eager fallback: if the shared library is missing, `lib()` raises
(`CAHipUnavailable`) with the build command.  Struct layouts mirror the header field by field.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CA_HIP_LIB") or os.path.join(_HERE, "csrc", "libcontrolanimate_hip.so")  # (CA_HIP_LIB: another build of the same ABI, for same-box A/B timing)

CA_BF16, CA_F16 = 0, 1
CA_F32 = 2  # control tensor of ca_canny_emit / ca_hed_fuse only
CA_ACT_NONE, CA_ACT_SILU = 0, 1
CA_ACT_QUICK_GELU, CA_ACT_GELU = 2, 3  # the CLIP MLPs (clip.py)
CA_ACT_RELU = 4  # the VGG stack of the HED annotator (hed.py)
CA_ACT_RELU6 = 5  # the MobileNetV2 backbone of the M-LSD annotator (mlsd.py)
CA_ACT_LEAKY02 = 6  # LeakyReLU(0.2): the U-Net and the SFT branches of the GFPGAN face restorer (gfpgan.py)
CA_ACT_LEAKY001 = 7  # LeakyReLU(0.01): the decoder of the NormalBae annotator (normalbae.py)
CA_MLSD_TOPK = 200
CA_POSE_MAX_PEAKS, CA_POSE_MAX_PEOPLE, CA_POSE_AREA_TAPS = 64, 64, 8  # the OpenPose annotator (openpose.py)
CA_POSE_OVERFLOW_PEAKS, CA_POSE_OVERFLOW_PEOPLE = 1, 2
CA_POSE_OVERFLOW_FACES, CA_POSE_OVERFLOW_FACE_RESIZE = 4, 8  # the face stage (openpose_face.py)
CA_FACE_SIZE, CA_FACE_HEAT, CA_FACE_PARTS, CA_FACE_MIN_SIDE, CA_FACE_SLOT_INTS = 384, 48, 71, 11, 8
CA_FACE_MODE_NONE, CA_FACE_MODE_LANCZOS4, CA_FACE_MODE_AREA = 0, 1, 2
CA_POSE_OVERFLOW_HANDS, CA_POSE_OVERFLOW_HAND_RESIZE = 16, 32  # the hand stage (openpose_hand.py)
CA_HAND_PARTS, CA_HAND_HEAT_COLS, CA_HAND_MAP, CA_HAND_SCALES, CA_HAND_SLOT_INTS = 21, 24, 128, 4, 8
CA_HAND_MODE_NONE, CA_HAND_MODE_RESIZE, CA_HAND_MIN_BOX, CA_HAND_AREA_TAPS = 0, 1, 20, 16
CA_RFACE_MAX_CAND, CA_RFACE_HEAD_COLS, CA_RFACE_DET_COLS, CA_RFACE_MAX_FACES = 1024, 32, 15, 64  # face detection and alignment (face_align.py)
CA_RFACE_OVERFLOW_CAND, CA_RFACE_OVERFLOW_FACES, CA_RFACE_CENTER, CA_RFACE_LARGEST, CA_FACE_ALIGN_SIZE = 1, 2, 1, 2, 512
CA_PARSE_CLASSES, CA_PARSE_CPAD, CA_BLUR_TAPS = 19, 32, 51  # the paste-back behind the face restorer (face_paste.py)
CA_RING_IN, CA_RING_OUT, CA_RING_RES, CA_RING_REFLECT, CA_RING_REPLICATE = 1, 2, 4, 0, 1
ABI_VERSION = 16


class CAHipUnavailable(RuntimeError):
    pass


class CAHipError(RuntimeError):
    pass


class GemmArgs(C.Structure):
    _fields_ = [
        ("a", C.c_void_p), ("a2", C.c_void_p), ("w", C.c_void_p), ("c", C.c_void_p),
        ("bias", C.c_void_p), ("rowbias", C.c_void_p), ("residual", C.c_void_p),
        ("lda", C.c_int64), ("lda2", C.c_int64), ("ldc", C.c_int64), ("ld_res", C.c_int64),
        ("ld_rowbias", C.c_int64),
        ("m", C.c_int32), ("n", C.c_int32), ("k1", C.c_int32), ("k2", C.c_int32),
        ("rows_per_group", C.c_int32),
        ("alpha", C.c_float), ("post_scale", C.c_float),
        ("act", C.c_int32), ("geglu", C.c_int32), ("out_f32", C.c_int32), ("dtype", C.c_int32),
        ("ln_stats", C.c_void_p), ("ln_colsum", C.c_void_p), ("ln_eps", C.c_float),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
        ("row_sums_out", C.c_void_p), ("ln_parts", C.c_int32),
        ("w_frag", C.c_void_p),
    ]


class FfArgs(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("w1_frag", C.c_void_p), ("bias1", C.c_void_p), ("colsum1", C.c_void_p), ("ln_stats", C.c_void_p),
        ("w2_frag", C.c_void_p), ("bias2", C.c_void_p), ("residual", C.c_void_p), ("y", C.c_void_p),
        ("lda", C.c_int64), ("ldc", C.c_int64), ("ld_res", C.c_int64),
        ("m", C.c_int32), ("c", C.c_int32), ("inner", C.c_int32), ("ln_eps", C.c_float), ("dtype", C.c_int32),
        ("w_out_frag", C.c_void_p), ("bias_out", C.c_void_p), ("residual_out", C.c_void_p), ("ld_res_out", C.c_int64),  # ABI v12
    ]


class TattnArgs(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("w_frag", C.c_void_p), ("gamma", C.c_void_p), ("bias_pe", C.c_void_p), ("o", C.c_void_p),
        ("lda", C.c_int64), ("ldo", C.c_int64), ("ld_bias_pe", C.c_int64),
        ("batch", C.c_int32), ("frames", C.c_int32), ("tokens", C.c_int32), ("heads", C.c_int32), ("c", C.c_int32),
        ("ln_eps", C.c_float), ("scale", C.c_float), ("dtype", C.c_int32),
        ("w_out_frag", C.c_void_p), ("bias_out", C.c_void_p), ("residual", C.c_void_p), ("ld_res", C.c_int64),  # ABI v12
    ]


ATTN_WOUT_FRAG_ELEMS = 102400  # CA_ATTN_WOUT_FRAG_ELEMS
TATTN_W_FRAG_ELEMS = 368640  # CA_TATTN_W_FRAG_ELEMS


class XattnArgs(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("wq_frag", C.c_void_p), ("bias", C.c_void_p), ("kv_frag", C.c_void_p), ("o", C.c_void_p),
        ("lda", C.c_int64), ("ldo", C.c_int64),
        ("m", C.c_int32), ("tokens", C.c_int32), ("frames_per_kv", C.c_int32), ("kv_mod", C.c_int32), ("kv_batches", C.c_int32),
        ("nk", C.c_int32), ("heads", C.c_int32), ("c", C.c_int32),
        ("ln_eps", C.c_float), ("dtype", C.c_int32),
        ("w_out_frag", C.c_void_p), ("bias_out", C.c_void_p), ("residual", C.c_void_p), ("ld_res", C.c_int64),  # ABI v12
        ("kv_frag_ip", C.c_void_p), ("nk_ip", C.c_int32), ("ip_scale", C.c_float),                              # ABI v13
    ]


XATTN_W_FRAG_ELEMS = 122880   # CA_XATTN_W_FRAG_ELEMS
XATTN_KV_FRAG_ELEMS = 7680    # CA_XATTN_KV_FRAG_ELEMS, per (text batch, head)


class ConvArgs(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("x2", C.c_void_p), ("w", C.c_void_p), ("y", C.c_void_p),
        ("bias", C.c_void_p), ("rowbias", C.c_void_p), ("residual", C.c_void_p),
        ("ld_res", C.c_int64), ("ld_rowbias", C.c_int64),
        ("images", C.c_int32), ("hin", C.c_int32), ("win", C.c_int32),
        ("cin1", C.c_int32), ("cin2", C.c_int32), ("cout", C.c_int32),
        ("stride", C.c_int32), ("upsample", C.c_int32), ("rows_per_group", C.c_int32),
        ("alpha", C.c_float), ("post_scale", C.c_float),
        ("act", C.c_int32), ("out_f32", C.c_int32), ("dtype", C.c_int32),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64), ("pad_asym", C.c_int32),
        ("w_wino", C.c_void_p), ("x_is_wino_v", C.c_int32),  # ABI v12
    ]


class GroupNormArgs(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("x2", C.c_void_p), ("y", C.c_void_p),
        ("gamma", C.c_void_p), ("beta", C.c_void_p), ("partials", C.c_void_p),
        ("images", C.c_int32), ("hw", C.c_int32), ("c1", C.c_int32), ("c2", C.c_int32),
        ("groups", C.c_int32), ("frames_per_stat", C.c_int32),
        ("eps", C.c_float), ("act", C.c_int32), ("dtype", C.c_int32),
        ("wino_v", C.c_void_p), ("wino_h", C.c_int32), ("wino_w", C.c_int32),  # ABI v12
    ]


class LayerNormArgs(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("y", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p),
        ("pos", C.c_void_p),
        ("rows", C.c_int64),
        ("c", C.c_int32), ("rows_per_frame", C.c_int32), ("frames", C.c_int32),
        ("eps", C.c_float), ("dtype", C.c_int32), ("stats", C.c_void_p),
    ]


class AttnArgs(C.Structure):
    _fields_ = [
        ("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p), ("o", C.c_void_p),
        ("q_outer", C.c_int64), ("q_inner", C.c_int64), ("q_row", C.c_int64),
        ("o_outer", C.c_int64), ("o_inner", C.c_int64), ("o_row", C.c_int64),
        ("k_outer", C.c_int64), ("k_inner", C.c_int64), ("k_row", C.c_int64),
        ("inner_count", C.c_int32), ("kv_inner_count", C.c_int32), ("kv_div", C.c_int32), ("kv_mod", C.c_int32),
        ("batches", C.c_int32), ("heads", C.c_int32), ("head_dim", C.c_int32),
        ("nq", C.c_int32), ("nk", C.c_int32),
        ("scale", C.c_float), ("out_scale", C.c_float),
        ("accumulate", C.c_int32), ("dtype", C.c_int32), ("causal", C.c_int32),
        ("key_mask", C.c_void_p), ("key_mask_stride", C.c_int64),
    ]


class ConvNarrowArgs(C.Structure):  # ABI v14: ca_conv3x3_narrow_args (the RRDBNet upscaler)
    _fields_ = [
        ("x", C.c_void_p), ("w", C.c_void_p), ("y", C.c_void_p), ("bias", C.c_void_p), ("r1", C.c_void_p), ("r2", C.c_void_p),
        ("ldx", C.c_int64), ("ldy", C.c_int64), ("ld_r1", C.c_int64), ("ld_r2", C.c_int64),
        ("images", C.c_int32), ("hin", C.c_int32), ("win", C.c_int32), ("cin", C.c_int32), ("cout", C.c_int32),
        ("channel_offset", C.c_int32), ("upsample", C.c_int32), ("leaky_relu", C.c_int32),
        ("s0", C.c_float), ("s1", C.c_float), ("s2", C.c_float),
        ("out_u8", C.c_int32), ("dtype", C.c_int32),
    ]


class PerceiverAttnArgs(C.Structure):  # ca_perceiver_attn_args (the IP-Adapter Plus Resampler)
    _fields_ = [
        ("q", C.c_void_p), ("x", C.c_void_p), ("l", C.c_void_p), ("o", C.c_void_p),
        ("q_row", C.c_int64), ("q_batch", C.c_int64),
        ("x_row", C.c_int64), ("x_batch", C.c_int64), ("x_v_off", C.c_int64),
        ("l_row", C.c_int64), ("l_batch", C.c_int64), ("l_v_off", C.c_int64),
        ("o_row", C.c_int64), ("o_batch", C.c_int64),
        ("batches", C.c_int32), ("heads", C.c_int32), ("head_dim", C.c_int32),
        ("nq", C.c_int32), ("n_x", C.c_int32), ("n_l", C.c_int32),
        ("scale", C.c_float), ("dtype", C.c_int32),
    ]


class ModconvArgs(C.Structure):  # ca_modconv_args (the StyleConv of the GFPGAN face restorer)
    _fields_ = [
        ("x", C.c_void_p), ("wt", C.c_void_p), ("s", C.c_void_p), ("demod", C.c_void_p), ("noise", C.c_void_p), ("bias", C.c_void_p),
        ("sft_scale", C.c_void_p), ("sft_shift", C.c_void_p), ("y", C.c_void_p),
        ("s_stride", C.c_int64), ("demod_stride", C.c_int64),
        ("images", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("cin", C.c_int32), ("cout", C.c_int32),
        ("upsample", C.c_int32), ("x_shared", C.c_int32),
        ("noise_weight", C.c_float), ("dtype", C.c_int32),
    ]


class Conv7x7Args(C.Structure):  # ca_conv7x7_args (the refinement stages of the OpenPose annotator)
    _fields_ = [
        ("x", C.c_void_p * 2), ("w", C.c_void_p * 2), ("bias", C.c_void_p * 2), ("y", C.c_void_p * 2),
        ("ldx", C.c_int64), ("ldy", C.c_int64),
        ("groups", C.c_int32), ("images", C.c_int32), ("h", C.c_int32), ("w_px", C.c_int32), ("cin", C.c_int32), ("cout", C.c_int32),
        ("relu", C.c_int32), ("dtype", C.c_int32),
    ]


# symbol -> (restype, argtypes); this table is also what tests/test_capi_symbols.py checks
# against the declarations in include/controlanimate_hip.h.
SYMBOLS = {
    "ca_abi_version": (C.c_int, []),
    "ca_last_error": (C.c_char_p, []),
    "ca_gemm": (C.c_int, [C.POINTER(GemmArgs), C.c_void_p]),
    "ca_pack_w_frag": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "ca_pack_w2_frag": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "ca_ff_fused": (C.c_int, [C.POINTER(FfArgs), C.c_void_p]),
    "ca_ff_fused_supported": (C.c_int, [C.POINTER(FfArgs)]),
    "ca_tattn_fused": (C.c_int, [C.POINTER(TattnArgs), C.c_void_p]),
    "ca_tattn_fused_supported": (C.c_int, [C.POINTER(TattnArgs)]),
    "ca_pack_w_tattn": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "ca_pack_w_out": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "ca_xattn_fused": (C.c_int, [C.POINTER(XattnArgs), C.c_void_p]),
    "ca_xattn_fused_supported": (C.c_int, [C.POINTER(XattnArgs)]),
    "ca_xattn_pack_w": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "ca_xattn_pack_kv": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_void_p, C.c_void_p]),
    "ca_gemm_ln_inline_supported": (C.c_int, [C.POINTER(GemmArgs)]),
    "ca_gemm_wants_finished_stats": (C.c_int, [C.POINTER(GemmArgs)]),
    "ca_ln_finish_sums": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "ca_gemm_workspace_bytes": (C.c_int64, [C.POINTER(GemmArgs)]),
    "ca_gemm_row_sums_parts": (C.c_int, [C.POINTER(GemmArgs)]),
    "ca_gemm_plan_name": (C.c_int, [C.POINTER(GemmArgs), C.c_char_p, C.c_int32]),
    "ca_conv3x3_plan_name": (C.c_int, [C.POINTER(ConvArgs), C.c_char_p, C.c_int32]),
    "ca_conv3x3": (C.c_int, [C.POINTER(ConvArgs), C.c_void_p]),
    "ca_pack_w_wino": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "ca_conv3x3_workspace_bytes": (C.c_int64, [C.POINTER(ConvArgs)]),
    "ca_softmax_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_float, C.c_int32, C.c_void_p]),
    "ca_groupnorm_partials_floats": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "ca_groupnorm_stats": (C.c_int, [C.POINTER(GroupNormArgs), C.c_void_p]),
    "ca_groupnorm_apply": (C.c_int, [C.POINTER(GroupNormArgs), C.c_void_p]),
    "ca_groupnorm": (C.c_int, [C.POINTER(GroupNormArgs), C.c_void_p]),
    "ca_groupnorm_wino_supported": (C.c_int, [C.POINTER(GroupNormArgs)]),
    "ca_layernorm": (C.c_int, [C.POINTER(LayerNormArgs), C.c_void_p]),
    "ca_attention": (C.c_int, [C.POINTER(AttnArgs), C.c_void_p]),
    "ca_attention_plan_name": (C.c_int, [C.POINTER(AttnArgs), C.c_char_p, C.c_int32]),
    "ca_add_bcast": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p]),
    "ca_repeat": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]),
    "ca_silu_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "ca_timestep_embedding": (C.c_int, [C.c_void_p, C.c_float, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "ca_latents_to_nhwc": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                      C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_void_p]),
    "ca_nhwc_to_ncfhw_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                        C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "ca_ncfhw_to_nhwc": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.c_void_p, C.c_int32, C.c_int32,
                                    C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "ca_cfg_scheduler_step": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                         C.POINTER(C.c_float), C.c_float, C.c_void_p]),
    "ca_lincomb": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_float), C.c_int32, C.c_int64, C.c_void_p]),
    # ABI v14
    "ca_conv3x3_narrow": (C.c_int, [C.POINTER(ConvNarrowArgs), C.c_void_p]),
    "ca_conv3x3_narrow_plan_name": (C.c_int, [C.POINTER(ConvNarrowArgs), C.c_char_p, C.c_int32]),
    "ca_rgb8_to_nhwc": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "ca_resize_lanczos4_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # ABI v15: the colour match (controlanimate_amd/color_match.py)
    "ca_color_match_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int64]),
    "ca_hist_u8x3": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p]),
    "ca_color_moments_f64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "ca_color_transform_f64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p]),
    "ca_sort_f64_segments": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "ca_color_rank_map_f64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64,
                                         C.c_void_p, C.c_int64, C.c_void_p]),
    "ca_color_finish_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    # ABI v16: the canny annotator (controlanimate_amd/annotators.py: CannyAnnotator)
    "ca_canny_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "ca_canny_tile_w": (C.c_int32, []),
    "ca_canny_tile_h": (C.c_int32, []),
    "ca_canny_classify": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "ca_canny_link": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "ca_canny_link_stage": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]),
    "ca_canny_emit": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    # added to ABI v16 (no struct or existing function changes, the number stays): the nearest-x2 upsampling convolution as four 2x2 phase convolutions (ConvArgs.w = w_phase [4, Cout, 2, 2, Cin])
    "ca_conv_up2_phase_supported": (C.c_int, [C.POINTER(ConvArgs)]),
    "ca_conv_up2_phase": (C.c_int, [C.POINTER(ConvArgs), C.c_void_p]),
    "ca_conv_up2_phase_plan_name": (C.c_int, [C.POINTER(ConvArgs), C.c_char_p, C.c_int32]),
    # added to ABI v16 likewise: the Resampler's attention over two key/value sources under one softmax (controlanimate_amd/resampler.py)
    "ca_perceiver_attn": (C.c_int, [C.POINTER(PerceiverAttnArgs), C.c_void_p]),
    # added to ABI v16 likewise: the stages of the HED annotator around its convolutions (controlanimate_amd/hed.py)
    "ca_hed_prep": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "ca_hed_pool_side": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "ca_hed_fuse": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    # added to ABI v16 likewise: the lineart annotator's stages beside ca_conv3x3 / ca_gemm (controlanimate_amd/lineart.py)
    "ca_lineart_conv_in": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "ca_instnorm_partials_floats": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "ca_instnorm_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "ca_instnorm_apply": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                    C.c_int32, C.c_float, C.c_int32, C.c_void_p]),
    "ca_convt3x3s2_gather": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "ca_lineart_conv_out": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "ca_lineart_finish": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    # added to ABI v16 likewise: the M-LSD annotator's stages beside ca_conv3x3 / ca_gemm / ca_add_bcast (controlanimate_amd/mlsd.py)
    "ca_mlsd_prep": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "ca_dwconv3x3": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "ca_upsample2x_bilinear_ac": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p]),
    "ca_conv3x3_dil": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "ca_mlsd_decode_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "ca_mlsd_decode": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ca_mlsd_draw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    # added to ABI v16 likewise: the softedge (PiDiNet) annotator's stages beside ca_conv3x3 / ca_gemm (controlanimate_amd/softedge.py)
    "ca_softedge_prep": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "ca_relu": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]),
    "ca_dwconv_k": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "ca_maxpool2x2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "ca_pdc_block_supported": (C.c_int, [C.c_int32, C.c_int32]),
    "ca_pdc_block": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "ca_cdcm_dil4": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "ca_csam_reduce": (C.c_int, [C.c_void_p] * 9 + [C.c_int32] * 5 + [C.c_void_p]),
    "ca_softedge_fuse": (C.c_int, [C.c_void_p] * 5 + [C.c_int32] * 4 + [C.c_void_p] * 3 + [C.c_int32, C.c_int32, C.c_void_p]),
    # added to ABI v16 likewise: the lineart_anime annotator's U-Net layers (controlanimate_amd/lineart_anime.py)
    "ca_lanime_conv_in": (C.c_int, [C.c_void_p] * 5 + [C.c_int32] * 4 + [C.c_void_p]),
    "ca_conv4x4s2": (C.c_int, [C.c_void_p] * 4 + [C.c_int32] * 7 + [C.c_void_p]),
    "ca_im2col4x4s2": (C.c_int, [C.c_void_p] * 2 + [C.c_int32] * 5 + [C.c_void_p]),
    "ca_convt4x4s2": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 6 + [C.c_void_p]),
    "ca_instnorm_act_partials_floats": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "ca_instnorm_act": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_void_p, C.c_int32, C.c_int32, C.c_int32] * 2 + [C.c_int32] * 4 + [C.c_float, C.c_int32, C.c_void_p]),
    "ca_lanime_conv_out": (C.c_int, [C.c_void_p] * 4 + [C.c_int32] * 4 + [C.c_void_p]),
    "ca_lanime_finish": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    # added to ABI v16 likewise: the GFPGAN face restorer's stages beside ca_conv3x3 / ca_gemm (controlanimate_amd/gfpgan.py)
    "ca_gfp_prep": (C.c_int, [C.c_void_p] * 4 + [C.c_int32] * 6 + [C.c_void_p]),
    "ca_resample2x": (C.c_int, [C.c_void_p] * 2 + [C.c_int32] * 6 + [C.c_void_p]),
    "ca_gfp_styles": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p]),
    "ca_modconv3x3": (C.c_int, [C.POINTER(ModconvArgs), C.c_void_p]),
    "ca_gfp_modulate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p] + [C.c_int32] * 7 + [C.c_void_p]),
    "ca_gfp_style_epilogue": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_float] + [C.c_void_p] * 4 + [C.c_int32] * 5 + [C.c_void_p]),
    "ca_gfp_to_rgb": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int32] * 5 + [C.c_void_p]),
    "ca_gfp_finish": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]),
    # added to ABI v16 likewise: the depth annotator's stages beside ca_gemm / ca_attention / ca_conv3x3 (controlanimate_amd/depth.py)
    "ca_resize_pil_u8": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 5 + [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "ca_dpt_patches": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int32] * 4 + [C.c_void_p]),
    "ca_depth_to_space": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int32] * 5 + [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "ca_dpt_head_supported": (C.c_int, [C.c_int32]),
    "ca_dpt_head": (C.c_int, [C.c_void_p] * 6 + [C.c_int32] * 5 + [C.c_void_p]),
    "ca_dpt_logit": (C.c_int, [C.c_void_p] * 4 + [C.c_int64, C.c_void_p]),
    "ca_resize_bicubic_f32": (C.c_int, [C.c_void_p] * 4 + [C.c_int32] * 5 + [C.c_void_p]),
    "ca_depth_finish": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int32] * 4 + [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    # added to ABI v16 likewise: the OpenPose body annotator's stages beside ca_conv3x3 / ca_maxpool2x2 / ca_gemm (controlanimate_amd/openpose.py)
    "ca_pose_prep": (C.c_int, [C.c_void_p] * 8 + [C.c_int32] * 8 + [C.c_void_p]),
    "ca_conv7x7": (C.c_int, [C.POINTER(Conv7x7Args), C.c_void_p]),
    "ca_im2col7x7": (C.c_int, [C.c_void_p] * 2 + [C.c_int32] * 4 + [C.c_int64, C.c_int32, C.c_void_p]),
    "ca_copy_cols": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p]),
    "ca_pose_maps_workspace_bytes": (C.c_int64, [C.c_int32] * 3),
    "ca_pose_maps": (C.c_int, [C.c_void_p] * 4 + [C.c_int64] + [C.c_void_p] * 3 + [C.c_int32] * 5 + [C.c_void_p]),
    "ca_pose_peaks": (C.c_int, [C.c_void_p] * 6 + [C.c_int32] * 3 + [C.c_void_p]),
    "ca_pose_connect": (C.c_int, [C.c_void_p] * 6 + [C.c_int32] * 3 + [C.c_void_p]),
    "ca_pose_assemble": (C.c_int, [C.c_void_p] * 9 + [C.c_int32] * 3 + [C.c_void_p]),
    "ca_pose_draw": (C.c_int, [C.c_void_p] * 6 + [C.c_int32] * 5 + [C.c_void_p]),
    # added to ABI v16 likewise: the face stage of the OpenPose annotator around its network (controlanimate_amd/openpose_face.py)
    "ca_face_boxes": (C.c_int, [C.c_void_p] * 6 + [C.c_int32] * 4 + [C.c_void_p]),
    "ca_face_crop": (C.c_int, [C.c_void_p] * 8 + [C.c_int32] * 8 + [C.c_void_p]),
    "ca_face_peaks": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 4 + [C.c_void_p]),
    "ca_pose_draw_faces": (C.c_int, [C.c_void_p] * 9 + [C.c_int32] * 5 + [C.c_void_p]),
    # added to ABI v16 likewise: the hand stage of the OpenPose annotator around its network (controlanimate_amd/openpose_hand.py)
    "ca_hand_boxes": (C.c_int, [C.c_void_p] * 6 + [C.c_int32] * 4 + [C.c_void_p]),
    "ca_hand_crop": (C.c_int, [C.c_void_p] * 10 + [C.c_int32] * 10 + [C.c_void_p]),
    "ca_hand_maps": (C.c_int, [C.c_void_p] * 7 + [C.c_int32] + [C.c_void_p]),
    "ca_hand_peaks": (C.c_int, [C.c_void_p] * 6 + [C.c_int32] * 4 + [C.c_void_p]),
    "ca_pose_draw_hands": (C.c_int, [C.c_void_p] * 10 + [C.c_int32] * 5 + [C.c_void_p]),
    # added to ABI v16 likewise: the NormalBae annotator's stages beside ca_gemm / ca_conv3x3 / ca_upsample2x_bilinear_ac (controlanimate_amd/normalbae.py)
    "ca_nbae_stem": (C.c_int, [C.c_void_p] * 4 + [C.c_int32] * 5 + [C.c_void_p]),
    "ca_dwconv_same_partials_floats": (C.c_int64, [C.c_int32] * 5),
    "ca_dwconv_same": (C.c_int, [C.c_void_p] * 6 + [C.c_int32] * 7 + [C.c_void_p]),
    "ca_se_gate": (C.c_int, [C.c_void_p] * 6 + [C.c_int32] * 3 + [C.c_float, C.c_void_p]),
    "ca_scale_channels": (C.c_int, [C.c_void_p] * 3 + [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p]),
    "ca_nbae_cat_pred": (C.c_int, [C.c_void_p] * 2 + [C.c_int32] * 3 + [C.c_int64, C.c_int32, C.c_int32, C.c_void_p]),
    "ca_nbae_normalize": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_float, C.c_void_p]),
    "ca_nbae_refine": (C.c_int, [C.c_void_p] * 11 + [C.c_int32] * 4 + [C.c_float, C.c_int32, C.c_void_p]),
    "ca_nbae_finish": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    # added to ABI v16 likewise: face detection and alignment beside ca_gemm / ca_conv3x3 / ca_copy_cols (controlanimate_amd/face_align.py)
    "ca_rface_stem": (C.c_int, [C.c_void_p] * 4 + [C.c_int32] * 6 + [C.c_void_p]),
    "ca_maxpool3x3s2": (C.c_int, [C.c_void_p] * 2 + [C.c_int32] * 5 + [C.c_void_p]),
    "ca_subsample2": (C.c_int, [C.c_void_p] * 2 + [C.c_int32] * 5 + [C.c_void_p]),
    "ca_add_up2": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 5 + [C.c_void_p]),
    "ca_rface_decode_workspace_bytes": (C.c_int64, [C.c_int32] * 3),
    "ca_rface_decode": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 3 + [C.c_float] * 3 + [C.c_int32] * 2 + [C.c_void_p, C.c_int64] + [C.c_void_p] * 3 + [C.c_void_p]),
    "ca_face_align": (C.c_int, [C.c_void_p] * 2 + [C.c_int32] * 2 + [C.c_double] + [C.c_void_p] * 2 + [C.c_void_p]),
    "ca_face_warp": (C.c_int, [C.c_void_p] * 4 + [C.c_int32] * 5 + [C.c_void_p]),
    # added to ABI v16 likewise: the paste-back behind the face restorer -- ParseNet, the mask blur, the inverse warp and the blend (controlanimate_amd/face_paste.py)
    "ca_parse_prep": (C.c_int, [C.c_void_p] * 2 + [C.c_int32] * 5 + [C.c_void_p]),
    "ca_conv3x3_reflect": (C.c_int, [C.c_void_p] * 5 + [C.c_int32] * 11 + [C.c_void_p]),
    "ca_parse_mask": (C.c_int, [C.c_void_p] * 4 + [C.c_int32] * 7 + [C.c_void_p]),
    "ca_parse_labels": (C.c_int, [C.c_void_p] * 3 + [C.c_int64, C.c_int32, C.c_int32, C.c_void_p]),
    "ca_ring_fill": (C.c_int, [C.c_void_p] + [C.c_int32] * 6 + [C.c_void_p]),
    "ca_mask_blur": (C.c_int, [C.c_void_p] * 4 + [C.c_int32] * 3 + [C.c_void_p]),
    "ca_face_paste": (C.c_int, [C.c_void_p] * 6 + [C.c_int32] * 4 + [C.c_double, C.c_void_p]),
}

_lib = None


def lib() -> C.CDLL:
    """Loads (once) and returns the shared library; raises CAHipUnavailable if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    # torch bundles its own HIP runtime: it must be loaded FIRST so that this library binds to the
    # same libamdhip64 instance (otherwise the process ends up with two runtimes and launches from
    # here fail with "no ROCm-capable device is detected").
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise CAHipUnavailable(
            f"{LIB_PATH} is missing: the HIP extension is not built. Run "
            "`python -m controlanimate_amd._build` (needs hipcc); there is no CPU fallback.")
    try:
        handle = C.CDLL(LIB_PATH)
    except OSError as e:  # e.g. libamdhip64 missing
        raise CAHipUnavailable(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(handle, name)
        fn.restype = res
        fn.argtypes = args
    if handle.ca_abi_version() != ABI_VERSION:
        raise CAHipUnavailable(f"ABI mismatch: library {handle.ca_abi_version()} vs binding {ABI_VERSION}; rebuild")
    _lib = handle
    return handle


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().ca_last_error()
        raise CAHipError(f"{what} failed with code {rc}: {msg.decode() if msg else ''}")
