"""ctypes binding of libpdm.so (include/pdm.h).

The product path has no fallback: if the HIP library is missing, cannot be loaded, or no GPU is
present, calls raise.  Status codes map to the exception types of the reference (ValueError for bad
arguments / unsupported shapes, RuntimeError otherwise).
"""
import collections
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpdm.so")
# A/B timing of two builds in one box session (tools/ab_build.sh): PDM_LIB_PATH names another in-tree build;
# entry points that build lacks are left unbound instead of failing the load
_AB = os.environ.get("PDM_LIB_PATH")
if _AB:
    LIB_PATH = _AB if os.path.isabs(_AB) else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), _AB)

PDM_F32, PDM_BF16, PDM_FP8, PDM_E8M0 = 0, 1, 2, 3
EPI_BF16, EPI_GELU, EPI_F32, EPI_RES = 0, 1, 2, 3


class PdmUvitCfg(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in (
        "img_size", "patch_size", "in_chans", "embed_dim", "depth", "num_heads", "mlp_hidden", "num_classes",
        "conv", "skip", "qkv_bias", "mlp_time_embed", "t2i", "clip_dim", "num_clip_token", "separate",
        "enable_panoptic", "num_panoptic_class", "fp8", "fp8_linears", "residual_fp32")]


class PdmDecoderCfg(ctypes.Structure):
    _fields_ = [("ch", ctypes.c_int), ("ch_mult", ctypes.c_int * 4), ("num_levels", ctypes.c_int),
                ("num_res_blocks", ctypes.c_int), ("z_channels", ctypes.c_int), ("out_ch", ctypes.c_int),
                ("latent_size", ctypes.c_int), ("scale_factor", ctypes.c_float)]


class PdmEncoderCfg(ctypes.Structure):
    _fields_ = [("ch", ctypes.c_int), ("ch_mult", ctypes.c_int * 4), ("num_levels", ctypes.c_int),
                ("num_res_blocks", ctypes.c_int), ("in_channels", ctypes.c_int), ("z_channels", ctypes.c_int),
                ("double_z", ctypes.c_int), ("latent_size", ctypes.c_int)]


class PdmClipCfg(ctypes.Structure):
    _fields_ = [("vocab", ctypes.c_int), ("width", ctypes.c_int), ("layers", ctypes.c_int), ("heads", ctypes.c_int),
                ("mlp_hidden", ctypes.c_int), ("max_position", ctypes.c_int), ("eps", ctypes.c_float)]


class PdmStageEpilogueArgs(ctypes.Structure):
    _fields_ = [
        ("pre", ctypes.c_void_p), ("conv_w", ctypes.c_void_p), ("conv_b", ctypes.c_void_p),
        ("B", ctypes.c_int), ("C", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int),
        ("has_uncond", ctypes.c_int), ("cfg_scale", ctypes.c_float), ("act_tanh", ctypes.c_int),
        ("xin", ctypes.c_void_p), ("ax", ctypes.c_float), ("ae", ctypes.c_float),
        ("m_out", ctypes.c_void_p),
        ("n_terms", ctypes.c_int), ("T", ctypes.c_void_p * 6), ("c", ctypes.c_float * 6), ("cm", ctypes.c_float),
        ("x_out", ctypes.c_void_p), ("x_out2", ctypes.c_void_p), ("x_out3", ctypes.c_void_p),
    ]


class PdmEmStepArgs(ctypes.Structure):
    _fields_ = [
        ("pre", ctypes.c_void_p), ("conv_w", ctypes.c_void_p), ("conv_b", ctypes.c_void_p),
        ("B", ctypes.c_int), ("C", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int),
        ("has_uncond", ctypes.c_int), ("cfg_scale", ctypes.c_float),
        ("x", ctypes.c_void_p), ("xin", ctypes.c_void_p),
        ("table", ctypes.c_void_p), ("steps", ctypes.c_int),
        ("counter", ctypes.c_void_p), ("t_next", ctypes.c_void_p),
        ("seed", ctypes.c_ulonglong), ("sample_offset", ctypes.c_ulonglong), ("sample_offset_dev", ctypes.c_void_p),
    ]


class PdmAssembleArgs(ctypes.Structure):
    _fields_ = [
        ("img", ctypes.c_void_p), ("C", ctypes.c_int), ("Himg", ctypes.c_int), ("Wimg", ctypes.c_int),
        ("p", ctypes.c_int), ("patch_w", ctypes.c_void_p), ("patch_b", ctypes.c_void_p), ("t", ctypes.c_void_p),
        ("time_emb", ctypes.c_void_p), ("y", ctypes.c_void_p), ("label_emb", ctypes.c_void_p),
        ("ctx_tokens", ctypes.c_void_p), ("n_ctx", ctypes.c_int), ("pos", ctypes.c_void_p), ("out", ctypes.c_void_p),
        ("ld_out", ctypes.c_int), ("B", ctypes.c_int), ("D", ctypes.c_int), ("L_total", ctypes.c_int),
        ("row0_patch", ctypes.c_int), ("time_row", ctypes.c_int), ("label_row", ctypes.c_int),
        ("ctx_row", ctypes.c_int),
    ]


class PdmGemmArgs(ctypes.Structure):
    _fields_ = [
        ("A1", ctypes.c_void_p), ("lda1", ctypes.c_int), ("A2", ctypes.c_void_p), ("lda2", ctypes.c_int),
        ("K1", ctypes.c_int), ("W", ctypes.c_void_p), ("ldw", ctypes.c_int), ("bias", ctypes.c_void_p),
        ("M", ctypes.c_int), ("N", ctypes.c_int), ("K", ctypes.c_int),
        ("out_bf16", ctypes.c_void_p), ("ldo", ctypes.c_int), ("out_f32", ctypes.c_void_p), ("ldr", ctypes.c_int),
        ("accumulate", ctypes.c_int), ("stats_out", ctypes.c_void_p), ("ln_stats", ctypes.c_void_p),
        ("ln_colsum", ctypes.c_void_p), ("ln_eps", ctypes.c_float), ("fp8", ctypes.c_int),
        ("a_scale", ctypes.c_void_p), ("a_scale_ld", ctypes.c_int), ("w_scale", ctypes.c_void_p),
        ("w_scale_ld", ctypes.c_int), ("out_fp8", ctypes.c_void_p), ("ldo8", ctypes.c_int),
        ("out_scale", ctypes.c_void_p), ("out_scale_ld", ctypes.c_int),
        ("mx_center", ctypes.c_int), ("ln_gcol", ctypes.c_void_p),
        ("res_in", ctypes.c_void_p), ("ldri", ctypes.c_int),
        ("res_f32", ctypes.c_void_p), ("ldrf", ctypes.c_int),
        ("a_rows_per_group", ctypes.c_int), ("a_group_stride", ctypes.c_int),
        ("out2", ctypes.c_void_p), ("out2_rows_per_group", ctypes.c_int), ("out2_group_stride", ctypes.c_int),
        ("stats_out2", ctypes.c_void_p),
    ]


class PdmGemmPlanOpts(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in (
        "convH", "convW", "convC", "conv_up", "batch", "act", "gn_P", "sk_attached", "algo", "sk_mode", "raster", "dbg",
        "mx_res_persist", "ncu", "persist_ok")]


_SIGS = {
    "pdm_gemm_args_size": (ctypes.c_int, []),
    "pdm_gemm_plan": (ctypes.c_int, [ctypes.POINTER(PdmGemmArgs), ctypes.POINTER(PdmGemmArgs), ctypes.c_int,
                                     ctypes.POINTER(PdmGemmPlanOpts), ctypes.POINTER(ctypes.c_int)]),
    "pdm_last_error": (ctypes.c_char_p, []),
    "pdm_version": (ctypes.c_int, []),
    "pdm_device_arch": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_int]),
    "pdm_set_gemm_algo": (ctypes.c_int, [ctypes.c_int]),
    "pdm_set_gemm_sk": (ctypes.c_int, [ctypes.c_int]),
    "pdm_gemm_sk_launches": (ctypes.c_longlong, []),
    "pdm_gemm_sk_stats": (ctypes.c_int, [ctypes.POINTER(ctypes.c_ulonglong)]),
    "pdm_gemm_seg_stats": (ctypes.c_int, [ctypes.POINTER(ctypes.c_ulonglong)]),
    "pdm_set_attention_algo": (ctypes.c_int, [ctypes.c_int]),
    "pdm_attention_plan": (ctypes.c_int, [ctypes.c_int] * 6 + [ctypes.POINTER(ctypes.c_int)]),
    "pdm_set_gemm_tuning": (ctypes.c_int, [ctypes.c_int, ctypes.c_int]),
    "pdm_uvit_create": (ctypes.c_int, [ctypes.POINTER(PdmUvitCfg), ctypes.POINTER(ctypes.c_void_p)]),
    "pdm_uvit_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "pdm_uvit_set_param": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_int,
                                          ctypes.c_longlong]),
    "pdm_uvit_param_count": (ctypes.c_int, [ctypes.c_void_p]),
    "pdm_uvit_param_info": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int,
                                           ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_longlong)]),
    "pdm_uvit_validate": (ctypes.c_int, [ctypes.c_void_p]),
    "pdm_uvit_workspace_size": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_size_t)]),
    "pdm_uvit_forward": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                        ctypes.c_void_p]),
    "pdm_uvit_t2i_forward": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "pdm_uvit_profile": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "pdm_uvit_profile_read": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float),
                                             ctypes.POINTER(ctypes.c_double), ctypes.c_int,
                                             ctypes.POINTER(ctypes.c_int)]),
    "pdm_stage_epilogue": (ctypes.c_int, [ctypes.POINTER(PdmStageEpilogueArgs), ctypes.c_void_p]),
    "pdm_lincomb": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
                                   ctypes.POINTER(ctypes.c_float), ctypes.c_longlong, ctypes.c_void_p]),
    "pdm_em_step": (ctypes.c_int, [ctypes.POINTER(PdmEmStepArgs), ctypes.c_void_p]),
    "pdm_philox_normal": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_ulonglong,
                                         ctypes.c_ulonglong, ctypes.c_int, ctypes.c_void_p]),
    "pdm_philox_raw": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_ulonglong,
                                      ctypes.c_ulonglong, ctypes.c_int, ctypes.c_void_p]),
    "pdm_gemm_bf16": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                     ctypes.c_int, ctypes.c_void_p]),
    "pdm_gemm": (ctypes.c_int, [ctypes.POINTER(PdmGemmArgs), ctypes.c_int, ctypes.c_void_p]),
    "pdm_gemm_pair": (ctypes.c_int, [ctypes.POINTER(PdmGemmArgs), ctypes.POINTER(PdmGemmArgs), ctypes.c_int,
                                     ctypes.c_void_p]),
    "pdm_gemm_bf16_ln": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                        ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p]),
    "pdm_rowstats": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                    ctypes.c_void_p, ctypes.c_void_p]),
    "pdm_gemm_conv3x3_bf16": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                             ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "pdm_gemm_batched_bf16": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p,
                                             ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_int,
                                             ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                             ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_int,
                                             ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p]),
    "pdm_layernorm": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                     ctypes.c_void_p]),
    "pdm_attention": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_void_p]),
    "pdm_attention_log2": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    "pdm_f32_to_bf16": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p]),
    "pdm_mx_quantize": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "pdm_images_to_u8": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_int, ctypes.c_void_p]),
    "pdm_mask_bits_to_rgb": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    "pdm_clip_create": (ctypes.c_int, [ctypes.POINTER(PdmClipCfg), ctypes.POINTER(ctypes.c_void_p)]),
    "pdm_clip_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "pdm_clip_param_count": (ctypes.c_int, [ctypes.c_void_p]),
    "pdm_clip_param_info": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int,
                                           ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_longlong)]),
    "pdm_clip_set_param": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_int,
                                          ctypes.c_longlong]),
    "pdm_clip_workspace_size": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_size_t)]),
    "pdm_clip_encode": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "pdm_decoder_create": (ctypes.c_int, [ctypes.POINTER(PdmDecoderCfg), ctypes.POINTER(ctypes.c_void_p)]),
    "pdm_decoder_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "pdm_decoder_param_count": (ctypes.c_int, [ctypes.c_void_p]),
    "pdm_decoder_param_info": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int,
                                              ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_longlong)]),
    "pdm_decoder_set_param": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_int,
                                             ctypes.c_longlong]),
    "pdm_decoder_workspace_size": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_size_t)]),
    "pdm_decoder_decode": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                          ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "pdm_decoder_set_gn_fusion": (ctypes.c_int, [ctypes.c_int]),
    "pdm_encoder_create": (ctypes.c_int, [ctypes.POINTER(PdmEncoderCfg), ctypes.POINTER(ctypes.c_void_p)]),
    "pdm_encoder_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "pdm_encoder_param_count": (ctypes.c_int, [ctypes.c_void_p]),
    "pdm_encoder_param_info": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int,
                                              ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_longlong)]),
    "pdm_encoder_set_param": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_int,
                                             ctypes.c_longlong]),
    "pdm_encoder_workspace_size": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_size_t)]),
    "pdm_encoder_encode_moments": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                                  ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "pdm_moments_sample": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                          ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_void_p]),
    # the autoencoder's kernels on their own (include/pdm.h, parity tests)
    "pdm_vae_groupnorm": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_void_p,
                                         ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p]),
    "pdm_gemm_bf16_gn": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                        ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                        ctypes.c_void_p]),
    "pdm_gemm_conv3x3_bf16_gn": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                                ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                                ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int),
                                                ctypes.c_void_p]),
    "pdm_vae_softmax_rows": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int,
                                            ctypes.c_float, ctypes.c_void_p]),
    "pdm_vae_transpose": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                         ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    "pdm_vae_dec_conv_in": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_float] + [ctypes.c_void_p] * 5 +
                            [ctypes.c_int] * 4 + [ctypes.c_void_p]),
    "pdm_vae_dec_conv_out": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                            ctypes.c_int, ctypes.c_void_p]),
    "pdm_vae_enc_conv_in": (ctypes.c_int, [ctypes.c_void_p] * 4 + [ctypes.c_int] * 4 + [ctypes.c_void_p]),
    "pdm_vae_down_gather": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p]),
    "pdm_vae_enc_tail": (ctypes.c_int, [ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 6),
    # training step (include/pdm.h "training")
    "pdm_train_create": (ctypes.c_int, [ctypes.POINTER(PdmUvitCfg), ctypes.POINTER(ctypes.c_void_p)]),
    "pdm_train_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "pdm_train_param_count": (ctypes.c_int, [ctypes.c_void_p]),
    "pdm_train_param_info": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int,
                                            ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong)]),
    "pdm_train_sizes": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_longlong),
                                       ctypes.POINTER(ctypes.c_longlong)]),
    "pdm_train_set_buffers": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p]),
    "pdm_train_refresh": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "pdm_train_workspace_size": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_size_t)]),
    "pdm_train_step": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_void_p,
                                      ctypes.c_size_t, ctypes.c_void_p]),
    "pdm_train_step_t2i": (ctypes.c_int, [ctypes.c_void_p] + [ctypes.c_void_p] * 8 + [ctypes.c_int, ctypes.c_float,
                                                                                      ctypes.c_void_p, ctypes.c_size_t,
                                                                                      ctypes.c_void_p]),
    "pdm_train_adamw": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                       ctypes.c_int, ctypes.c_float, ctypes.c_void_p]),
    "pdm_train_active": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_longlong)]),
    "pdm_train_grad_norm": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "pdm_grad_norm_clip": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_float,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "pdm_set_wgrad_tile": (ctypes.c_int, [ctypes.c_int]),
    "pdm_wgrad": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                 ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                 ctypes.c_size_t, ctypes.c_void_p]),
    "pdm_attention_backward": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    "pdm_attention_backward_scratch_size": (ctypes.c_int, [ctypes.c_int] * 4 + [ctypes.POINTER(ctypes.c_size_t)]),
    "pdm_attention_backward_ex": (ctypes.c_int, [ctypes.c_void_p] * 4 + [ctypes.c_int] * 5 +
                                  [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "pdm_layernorm_backward": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                              ctypes.c_size_t, ctypes.c_void_p]),
    # the training step's other kernels on their own (include/pdm.h, parity tests)
    "pdm_wgrad_gather": (ctypes.c_int, [ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p] + [ctypes.c_int] * 4 +
                         [ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                                                   ctypes.c_size_t, ctypes.c_void_p]),
    "pdm_colsum": (ctypes.c_int, [ctypes.c_void_p] + [ctypes.c_int] * 7 + [ctypes.c_void_p, ctypes.c_int,
                                                                           ctypes.c_void_p, ctypes.c_size_t,
                                                                           ctypes.c_void_p]),
    "pdm_layernorm_backward_rows": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                                   ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p] +
                                    [ctypes.c_int] * 5 + [ctypes.c_float, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                          ctypes.c_size_t, ctypes.c_void_p]),
    "pdm_layernorm_rows": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p] + [ctypes.c_int] * 6 + [ctypes.c_float, ctypes.c_void_p]),
    "pdm_gelu_forward": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p]),
    "pdm_gelu_backward": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p]),
    "pdm_lsimple": (ctypes.c_int, [ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_int,
                                                           ctypes.c_void_p]),
    "pdm_conv3x3_backward": (ctypes.c_int, [ctypes.c_void_p] * 6 + [ctypes.c_int] * 4 + [ctypes.c_void_p]),
    "pdm_head_forward": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 8 + [ctypes.c_void_p]),
    "pdm_head_backward": (ctypes.c_int, [ctypes.c_void_p] * 4 + [ctypes.c_int] * 7 + [ctypes.c_void_p]),
    "pdm_assemble": (ctypes.c_int, [ctypes.POINTER(PdmAssembleArgs), ctypes.c_void_p]),
    "pdm_patchify": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 6 + [ctypes.c_void_p]),
    "pdm_label_scatter": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "pdm_rows_add_cast": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 3 + [ctypes.c_void_p] +
                          [ctypes.c_int] * 6 + [ctypes.c_void_p]),
    "pdm_add_cast": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong,
                                    ctypes.c_void_p]),
    "pdm_transpose_bf16": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_void_p]),
}

EXPORTED_SYMBOLS = tuple(_SIGS)

_lib = None


def load():
    """Load libpdm.so (no GPU needed to load; every compute call needs one)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"libpdm.so not found at {LIB_PATH}: build it with `python -c 'import __graft_entry__ as g; "
                           f"g.build()'` (or `make -C panopticdiffusionmodels_amd/csrc`)")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _SIGS.items():
        if _AB and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(status, what=""):
    if status != 0:
        msg = load().pdm_last_error().decode()
        if status == 1:
            raise ValueError(f"{what}: {msg}" if what else msg)
        raise RuntimeError(f"{what}: {msg}" if what else msg)


# Priority of the lane streams.  HIP keeps one pool of hardware queues per stream priority, each capped at
# GPU_MAX_HW_QUEUES (4 by default): a normal-priority lane stream shares a queue with the caller's stream or RCCL's
# once the process has made a few streams (torchrun / accelerate), and the lanes then run one after the other.
LANE_STREAM_PRIORITY = int(os.environ.get("PDM_LANE_PRIORITY", "-1"))
_LANE_STREAMS = {}


def lane_streams(device, n):
    """The process's n side streams on `device` (LANE_STREAM_PRIORITY), shared by every multi-lane user (the
    samplers' lanes, the decoder's lanes): each extra stream a process makes can take a hardware queue the sampling
    lanes need (two decoder streams of their own cost the L/2 bench 55-60 ms of sampling per step), so lanes reuse
    these few instead of making their own.  Users run one after the other from one host thread and order their lanes
    against the caller's stream on entry and exit."""
    dev = torch.device(device)
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    pool = _LANE_STREAMS.setdefault(key, [])
    while len(pool) < n:
        pool.append(torch.cuda.Stream(device=dev, priority=LANE_STREAM_PRIORITY))
    return pool[:n]


def require_gpu(t=None):
    if not torch.cuda.is_available():
        raise RuntimeError("panopticdiffusionmodels_amd runs on an MI355X (gfx950) GPU; no GPU is visible "
                           "(there is no CPU fallback in the product path)")
    if t is not None and t.device.type != "cuda":
        raise RuntimeError(f"expected a tensor on the GPU, got device {t.device}")


def stream_ptr(device=None):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


# ---- thin op wrappers (used by tests and the generic solver path) ----------------------------------

def gemm(a, w, bias=None, epi=EPI_BF16, out=None, out_f32=None, accumulate=False, a2=None):
    """C = [a | a2] @ w.T (+ bias) with the selected epilogue.  a/a2/w bf16 2-D contiguous rows."""
    lib = load()
    require_gpu(a)
    M, K1 = a.shape
    K = K1 + (a2.shape[1] if a2 is not None else 0)
    N = w.shape[0]
    assert w.shape[1] == K
    if epi in (EPI_BF16, EPI_GELU) and out is None:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=a.device)
    if epi == EPI_F32 and out_f32 is None:
        out_f32 = torch.zeros(M, N, dtype=torch.float32, device=a.device)
    check(lib.pdm_gemm_bf16(ptr(a), a.stride(0), ptr(a2), a2.stride(0) if a2 is not None else 0, K1, ptr(w),
                            ptr(bias), M, N, K, epi, ptr(out), out.stride(0) if out is not None else 0,
                            ptr(out_f32), out_f32.stride(0) if out_f32 is not None else 0, int(accumulate),
                            stream_ptr(a.device)), "pdm_gemm_bf16")
    return out_f32 if epi == EPI_F32 else out


def rowstats(x, want_bf16=True):
    """(bf16 copy, LayerNorm partials [rows, ceil(D/256), 2]) of fp32 rows x [rows, D]."""
    lib = load()
    require_gpu(x)
    rows, D = x.shape
    st = torch.empty(rows, (D + 255) // 256, 2, dtype=torch.float32, device=x.device)
    xb = torch.empty(rows, D, dtype=torch.bfloat16, device=x.device) if want_bf16 else None
    check(lib.pdm_rowstats(ptr(x), x.stride(0), rows, D, ptr(xb), ptr(st), stream_ptr(x.device)), "pdm_rowstats")
    return xb, st


def gemm_ln(a, w, bias, epi, ln_stats=None, ln_colsum=None, out=None, out_f32=None, accumulate=False,
            stats_out=False, eps=1e-5):
    """GEMM with the fused-LayerNorm operands (see include/pdm.h pdm_gemm_bf16_ln).  Returns the output, plus
    the produced partials when stats_out."""
    lib = load()
    require_gpu(a)
    M, K = a.shape
    N = w.shape[0]
    if epi in (EPI_BF16, EPI_GELU) and out is None:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=a.device)
    if epi == EPI_F32 and out_f32 is None:
        out_f32 = torch.zeros(M, N, dtype=torch.float32, device=a.device)
    st = torch.empty(M, (N + 255) // 256, 2, dtype=torch.float32, device=a.device) if stats_out else None
    check(lib.pdm_gemm_bf16_ln(ptr(a), a.stride(0), ptr(w), ptr(bias), M, N, K, epi, ptr(out),
                               out.stride(0) if out is not None else 0, ptr(out_f32),
                               out_f32.stride(0) if out_f32 is not None else 0, int(accumulate), ptr(st),
                               ptr(ln_stats), ptr(ln_colsum), eps, stream_ptr(a.device)), "pdm_gemm_bf16_ln")
    res = out_f32 if epi == EPI_F32 else out
    return (res, st) if stats_out else res


# ---- MXFP8 (OCP e4m3 + E8M0 per 32 elements) host reference and GEMM wrapper --------------------------

def mx_quantize(x):
    """MXFP8 of x [R, K] (K % 32 == 0) exactly as the GPU epilogue quantises (csrc/pdm_common.h mx_quant8):
    E8M0 exponent e = ceil(log2(amax/448)) + 127 per 32 consecutive elements, e4m3 = RNE(x * 2^(127 - e)).
    Returns (q [R, K] float8_e4m3fn, scale dwords [K/128, R] int32: byte j of (kt, r) = block kt*4 + j)."""
    R, K = x.shape
    xb = x.float().reshape(R, K // 32, 32)
    amax = xb.abs().amax(-1)
    bits = (amax * (1.0 / 448.0)).view(torch.int32)
    e = ((bits >> 23) & 0xFF) + ((bits & 0x7FFFFF) != 0).to(torch.int32)
    e = e.clamp(max=254)
    inv = ((254 - e) << 23).view(torch.float32)
    q = (xb * inv[..., None]).reshape(R, K).to(torch.float8_e4m3fn)
    kt = (K + 127) // 128   # K % 128 != 0: the last scale dword is zero-padded
    e8 = torch.zeros(R, kt * 4, dtype=torch.uint8, device=x.device)
    e8[:, : K // 32] = e.to(torch.uint8)
    sc = e8.reshape(R, kt, 4).permute(1, 0, 2).contiguous().view(torch.int32).reshape(kt, R)
    return q, sc


def mx_dequantize(q, sc):
    R, K = q.shape
    e = sc.contiguous().view(torch.uint8).reshape(K // 128, R, 4).permute(1, 0, 2).reshape(R, K // 32).to(torch.int32)
    scale = torch.pow(2.0, (e - 127).double()).float()
    return (q.float().reshape(R, K // 32, 32) * scale[..., None]).reshape(R, K)


def mx_quantize_gpu(x):
    """MXFP8 of fp32 / bf16 rows x [R, K] on the GPU (pdm_mx_quantize): (q float8_e4m3fn [R, K], scale dwords
    int32 [ceil(K/128), R]), bit-identical to mx_quantize."""
    lib = load()
    require_gpu(x)
    R, K = x.shape
    q = torch.empty(R, K, dtype=torch.float8_e4m3fn, device=x.device)
    s = torch.zeros((K + 127) // 128, R, dtype=torch.int32, device=x.device)
    dt = PDM_F32 if x.dtype == torch.float32 else PDM_BF16
    check(lib.pdm_mx_quantize(ptr(x), dt, x.stride(0), R, K, ptr(q), q.stride(0), ptr(s), R, stream_ptr(x.device)),
          "pdm_mx_quantize")
    return q, s


def gemm_ex(epi, a, w, bias=None, *args, **kw):
    """pdm_gemm with every option (include/pdm.h pdm_gemm_args; positional after bias: a_scale, w_scale, out, ...).
    a / w are bf16, or float8_e4m3fn with their scale dword arrays (MXFP8); a2 (bf16) continues a along K (the
    split-K skip_linear operand)."""
    g = _gemm_args(a, w, bias, *args, **kw)
    check(load().pdm_gemm(ctypes.byref(g), epi, stream_ptr(a.device)), "pdm_gemm")


def gemm_pair(epi, first, second):
    """pdm_gemm_pair: two GEMMs of one epilogue / N / K given as gemm_ex keyword dicts (a, w, bias, ...), grouped
    into one persistent launch where the kernel takes both."""
    ga, gb = _gemm_args(**first), _gemm_args(**second)
    check(load().pdm_gemm_pair(ctypes.byref(ga), ctypes.byref(gb), epi, stream_ptr(first["a"].device)),
          "pdm_gemm_pair")


def _gemm_args(a, w, bias=None, a_scale=None, w_scale=None, out=None, out_f32=None, accumulate=False,
               ln_stats=None, ln_colsum=None, stats_out=None, out_fp8=None, out_scale=None, eps=1e-5,
               mx_center=False, ln_gcol=None, res_in=None, res_f32=None, a2=None, a_gather=None, out2=None,
               out2_gather=None, stats_out2=None):
    require_gpu(a)
    M, K = a.shape
    N = w.shape[0]
    g = PdmGemmArgs()
    g.A1, g.lda1 = a.data_ptr(), a.stride(0)
    g.K1 = K
    if a2 is not None:
        g.A2, g.lda2 = a2.data_ptr(), a2.stride(0)
        K = K + a2.shape[1]
    g.W, g.ldw = w.data_ptr(), w.stride(0)
    g.bias = bias.data_ptr() if bias is not None else None
    g.M, g.N, g.K = M, N, K
    if out is not None:
        g.out_bf16, g.ldo = out.data_ptr(), out.stride(0)
    if out_f32 is not None:
        g.out_f32, g.ldr = out_f32.data_ptr(), out_f32.stride(0)
    g.accumulate = int(accumulate)
    g.stats_out = stats_out.data_ptr() if stats_out is not None else None
    g.ln_stats = ln_stats.data_ptr() if ln_stats is not None else None
    g.ln_colsum = ln_colsum.data_ptr() if ln_colsum is not None else None
    g.ln_eps = eps
    if a.dtype == torch.float8_e4m3fn:
        g.fp8 = 1
        g.a_scale, g.a_scale_ld = a_scale.data_ptr(), a_scale.shape[1]
        g.w_scale, g.w_scale_ld = w_scale.data_ptr(), w_scale.shape[1]
    if out_fp8 is not None:
        g.out_fp8, g.ldo8 = out_fp8.data_ptr(), out_fp8.stride(0)
        g.out_scale, g.out_scale_ld = out_scale.data_ptr(), out_scale.shape[1]
    g.mx_center = int(mx_center)
    g.ln_gcol = ln_gcol.data_ptr() if ln_gcol is not None else None
    if res_in is not None:
        g.res_in, g.ldri = res_in.data_ptr(), res_in.stride(0)
    if res_f32 is not None:
        g.res_f32, g.ldrf = res_f32.data_ptr(), res_f32.stride(0)
    if a_gather is not None:   # (M, rows_per_group, group_stride): row m reads a[(m // rpg) * gs + m % rpg]
        g.M, g.a_rows_per_group, g.a_group_stride = a_gather
    if out2 is not None:       # out2_gather = (rows_per_group, group_stride) of the second residual output
        g.out2 = out2.data_ptr()
        g.out2_rows_per_group, g.out2_group_stride = out2_gather
        g.stats_out2 = stats_out2.data_ptr() if stats_out2 is not None else None
    return g


def mx_quantize_centred(x, stats):
    """The group-centred MXFP8 copy a producing epilogue writes (include/pdm.h pdm_gemm_args.mx_center): x [R, K]
    minus mu_t = stats[r, t, 0] / width_t per 256-column group (fp32, as the kernel divides), quantised with
    mx_quantize."""
    R, K = x.shape
    st = stats.reshape(R, -1, 2)
    xc = x.float().clone()
    for t in range((K + 255) // 256):
        w = min(256, K - 256 * t)
        xc[:, 256 * t: 256 * t + w] -= (st[:, t, 0] / float(w))[:, None]
    return mx_quantize(xc)


def gemm_conv3x3(x, w, bias=None, epi=EPI_F32, up=0, out=None, out_f32=None, accumulate=False):
    """Implicit-GEMM conv3x3 (pad 1) on NHWC bf16 x [B, h, w, Cin]; w [N, Cin, 3, 3] bf16 (torch layout, repacked
    here to the kernel's (ky, kx, ci) K order).  up=1 convolves the nearest-x2 upsample of x."""
    lib = load()
    require_gpu(x)
    B, h, wd, C = x.shape
    H, W = h << up, wd << up
    N = w.shape[0]
    wk = w.permute(0, 2, 3, 1).reshape(N, 9 * C).contiguous()
    if epi in (EPI_BF16, EPI_GELU) and out is None:
        out = torch.empty(B * H * W, N, dtype=torch.bfloat16, device=x.device)
    if epi == EPI_F32 and out_f32 is None:
        out_f32 = torch.zeros(B * H * W, N, dtype=torch.float32, device=x.device)
    check(lib.pdm_gemm_conv3x3_bf16(ptr(x), B, H, W, C, up, ptr(wk), ptr(bias), N, epi, ptr(out), ptr(out_f32),
                                    int(accumulate), stream_ptr(x.device)), "pdm_gemm_conv3x3_bf16")
    return out_f32 if epi == EPI_F32 else out


# ---- the autoencoder's kernels on their own (include/pdm.h pdm_vae_*, parity tests) -------------------

def gn_part_elems(B, gn_P):
    """doubles in the GroupNorm partials [B, gn_P / 256, 32, 2] a GEMM epilogue writes."""
    return B * (gn_P // 256) * 64


def vae_groupnorm(x, gamma, beta, eps=1e-6, swish=False, partials=None):
    """GroupNorm(32) [+ swish] of NHWC x [B, P, C] (fp32 / bf16) -> (y bf16 [B, P, C], stats fp32 [B, 32, 2]).
    partials: ready-made fp64 [B, P / 256, 32, 2] (sum, sum of squares), replacing the statistics pass."""
    lib = load()
    require_gpu(x)
    B, P, C = x.shape
    y = torch.empty(B, P, C, dtype=torch.bfloat16, device=x.device)
    stats = torch.empty(B, 32, 2, dtype=torch.float32, device=x.device)
    part = partials if partials is not None else torch.empty(B * ((P + 63) // 64) * 64, dtype=torch.float64,
                                                             device=x.device)
    check(lib.pdm_vae_groupnorm(ptr(x), PDM_F32 if x.dtype == torch.float32 else PDM_BF16, B, P, C, ptr(gamma),
                                ptr(beta), eps, int(swish), ptr(part), part.numel(), int(partials is not None), ptr(y),
                                ptr(stats), stream_ptr(x.device)), "pdm_vae_groupnorm")
    return y, stats


def gemm_gn(a, w, bias, epi, gn_part, gn_P, out=None, out_f32=None, accumulate=False):
    """pdm_gemm_bf16_gn: gemm() whose epilogue also writes the GroupNorm partials to gn_part (fp64) where the tile
    policy can.  Returns (output, fused)."""
    lib = load()
    require_gpu(a)
    M, K = a.shape
    N = w.shape[0]
    if epi == EPI_BF16 and out is None:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=a.device)
    if epi == EPI_F32 and out_f32 is None:
        out_f32 = torch.zeros(M, N, dtype=torch.float32, device=a.device)
    fused = ctypes.c_int(-1)
    check(lib.pdm_gemm_bf16_gn(ptr(a), a.stride(0), None, 0, K, ptr(w), ptr(bias), M, N, K, epi, ptr(out),
                               out.stride(0) if out is not None else 0, ptr(out_f32),
                               out_f32.stride(0) if out_f32 is not None else 0, int(accumulate), ptr(gn_part), gn_P,
                               ctypes.byref(fused), stream_ptr(a.device)), "pdm_gemm_bf16_gn")
    return (out_f32 if epi == EPI_F32 else out), fused.value


def gemm_conv3x3_gn(x, w, bias, epi, gn_part, up=0, out=None, out_f32=None, accumulate=False):
    """pdm_gemm_conv3x3_bf16_gn: gemm_conv3x3() with the GroupNorm partials of its output (H * W rows per image).
    Returns (output, fused)."""
    lib = load()
    require_gpu(x)
    B, h, wd, C = x.shape
    H, W = h << up, wd << up
    N = w.shape[0]
    wk = w.permute(0, 2, 3, 1).reshape(N, 9 * C).contiguous()
    if epi == EPI_BF16 and out is None:
        out = torch.empty(B * H * W, N, dtype=torch.bfloat16, device=x.device)
    if epi == EPI_F32 and out_f32 is None:
        out_f32 = torch.zeros(B * H * W, N, dtype=torch.float32, device=x.device)
    zero = torch.zeros(256, dtype=torch.uint8, device=x.device)
    fused = ctypes.c_int(-1)
    check(lib.pdm_gemm_conv3x3_bf16_gn(ptr(x), B, H, W, C, up, ptr(wk), ptr(bias), N, epi, ptr(out), ptr(out_f32),
                                       int(accumulate), ptr(zero), ptr(gn_part), ctypes.byref(fused),
                                       stream_ptr(x.device)), "pdm_gemm_conv3x3_bf16_gn")
    return (out_f32 if epi == EPI_F32 else out), fused.value


def vae_softmax_rows(scores, scale):
    """bf16 softmax(scores * scale) over the last dim of fp32 scores [rows, n], n <= 4096."""
    require_gpu(scores)
    rows, n = scores.shape
    p = torch.empty(rows, n, dtype=torch.bfloat16, device=scores.device)
    check(load().pdm_vae_softmax_rows(ptr(scores), ptr(p), rows, n, scale, stream_ptr(scores.device)),
          "pdm_vae_softmax_rows")
    return p


def vae_transpose(src, col0, C):
    """bf16 src [B, n, ld] columns col0 .. col0 + C - 1 -> [B, C, n]."""
    require_gpu(src)
    B, n, ld = src.shape
    dst = torch.empty(B, C, n, dtype=torch.bfloat16, device=src.device)
    check(load().pdm_vae_transpose(ptr(src), ld, col0, ptr(dst), B, n, C, stream_ptr(src.device)), "pdm_vae_transpose")
    return dst


def vae_dec_conv_in(z, scale_factor, pq_w, pq_b, w, bias):
    """z fp32 [B, 4, h, w] / scale_factor -> post_quant_conv -> conv_in (w [Cout, 4, 3, 3]) -> fp32 NHWC."""
    require_gpu(z)
    B, _, h, wd = z.shape
    Cout = w.shape[0]
    out = torch.empty(B, h, wd, Cout, dtype=torch.float32, device=z.device)
    check(load().pdm_vae_dec_conv_in(ptr(z), scale_factor, ptr(pq_w), ptr(pq_b), ptr(w), ptr(bias), ptr(out), B, h, wd,
                                     Cout, stream_ptr(z.device)), "pdm_vae_dec_conv_in")
    return out


def vae_dec_conv_out(g, w, bias, out_ch=3, force_valu=False):
    """g bf16 NHWC [B, H, W, C], w bf16 [4, 3, 3, C] (ky, kx, ci), bias fp32 [4] -> fp32 NCHW [B, out_ch, H, W]."""
    require_gpu(g)
    B, H, W, C = g.shape
    img = torch.empty(B, out_ch, H, W, dtype=torch.float32, device=g.device)
    check(load().pdm_vae_dec_conv_out(ptr(g), B, H, W, C, ptr(w), ptr(bias), ptr(img), out_ch, int(force_valu),
                                      stream_ptr(g.device)), "pdm_vae_dec_conv_out")
    return img


def vae_enc_conv_in(img, w, bias):
    """img fp32 NCHW [B, 3, H, W], w fp32 [C, 3, 3, 3] -> fp32 NHWC [B, H, W, C]."""
    require_gpu(img)
    B, _, H, W = img.shape
    C = w.shape[0]
    out = torch.empty(B, H, W, C, dtype=torch.float32, device=img.device)
    check(load().pdm_vae_enc_conv_in(ptr(img), ptr(w), ptr(bias), ptr(out), B, H, W, C, stream_ptr(img.device)),
          "pdm_vae_enc_conv_in")
    return out


def vae_down_gather(x):
    """x fp32 NHWC [B, H, W, C] -> the stride-2 downsample's GEMM operand bf16 [B * (H/2) * (W/2), 9 C]."""
    require_gpu(x)
    B, H, W, C = x.shape
    A = torch.empty(B * (H // 2) * (W // 2), 9 * C, dtype=torch.bfloat16, device=x.device)
    check(load().pdm_vae_down_gather(ptr(x), ptr(A), B, H, W, C, stream_ptr(x.device)), "pdm_vae_down_gather")
    return A


def vae_enc_tail(g, w, cbias, qw, qb):
    """g bf16 NHWC [B, H, W, C], conv_out w bf16 [8, 3, 3, C] + quant_conv qw [8, 8] -> moments fp32 [B, 8, H, W]."""
    require_gpu(g)
    B, H, W, C = g.shape
    m = torch.empty(B, 8, H, W, dtype=torch.float32, device=g.device)
    check(load().pdm_vae_enc_tail(ptr(g), B, H, W, C, ptr(w), ptr(cbias), ptr(qw), ptr(qb), ptr(m),
                                  stream_ptr(g.device)), "pdm_vae_enc_tail")
    return m


def gemm_batched(a, w, bias=None, epi=EPI_F32):
    """out[z] = a[z] @ w[z].T (+ bias) for a [Z, M, K], w [Z, N, K] bf16 contiguous."""
    lib = load()
    require_gpu(a)
    Z, M, K = a.shape
    N = w.shape[1]
    if epi == EPI_F32:
        ob, of = None, torch.zeros(Z, M, N, dtype=torch.float32, device=a.device)
    else:
        ob, of = torch.empty(Z, M, N, dtype=torch.bfloat16, device=a.device), None
    check(lib.pdm_gemm_batched_bf16(ptr(a), K, M * K, ptr(w), K, N * K, ptr(bias), M, N, K, Z, epi, ptr(ob), N, M * N,
                                    ptr(of), N, M * N, 0, stream_ptr(a.device)), "pdm_gemm_batched_bf16")
    return of if epi == EPI_F32 else ob


def layernorm(x, gamma, beta, eps=1e-5):
    lib = load()
    require_gpu(x)
    rows, D = x.shape
    y = torch.empty(rows, D, dtype=torch.bfloat16, device=x.device)
    check(lib.pdm_layernorm(ptr(x), x.stride(0), ptr(gamma), ptr(beta), ptr(y), y.stride(0), rows, D, eps,
                            stream_ptr(x.device)), "pdm_layernorm")
    return y


ATTENTION_FAMILIES = ("streamed", "kv2", "kv3", "v2", "v2_valu", "v3", "h72", "h72p")   # PDM_ATTN_* of include/pdm.h
AttentionPlan = collections.namedtuple("AttentionPlan", "family waves tail1 variant grid lds_bytes")


def attention_plan(B, L, H, Dh, algo=0, ncu=256):
    """What `attention` launches for this shape under pdm_set_attention_algo(algo) on a device of ncu compute units:
    AttentionPlan(family name, waves per workgroup, tail1, timing variant 0/1/2, grid, dynamic LDS bytes).  Pure
    host code (no GPU, no global read or changed); the launcher decides with the same function."""
    out = (ctypes.c_int * 6)()
    check(load().pdm_attention_plan(B, L, H, Dh, int(algo), int(ncu), out), "pdm_attention_plan")
    return AttentionPlan(ATTENTION_FAMILIES[out[0]], out[1], bool(out[2]), out[3], out[4], out[5])


GEMM_FAMILIES = ("128", "ring32", "ring64", "8p", "8d", "8d_hn", "8t", "8s", "8s_mx", "8g", "mx")   # PDM_GEMM_*
GEMM_PLAN_ERRORS = (None, "fp8_range", "nostore", "guard", "epi")                                  # PDM_GEMM_ERR_*
GemmPlan = collections.namedtuple(
    "GemmPlan", "error family epi conv sched mxo sk fp8 dual grid_x grid_y block lds_bytes tiles_n ntiles nt0 raster "
                "split_m1 rowstats out2_copy writes_gn gn_fusable grouped kernel")


def gemm_plan(g, epi, second=None, conv=None, batch=0, act=0, gn_P=0, sk_attached=False, algo=-1, sk_mode=-1,
              raster=-1, dbg=-1, mx_res_persist=-1, ncu=-1, persist_ok=-1):
    """What pdm_gemm(g, epi) -- with `second`, pdm_gemm_pair -- launches: GemmPlan(error name or None, family name,
    the instantiation's template coordinates, launch geometry, row split, post-passes, writes_gn, gn_fusable, grouped,
    kernel-table row).  g / second: PdmGemmArgs (`_gemm_args(...)` of tensors, or made-up addresses: nothing is
    dereferenced).  conv = (H, W, Cin, up), batch, act, gn_P, sk_attached: what the struct lacks.  The policy fields
    default to this process's current values; ncu / persist_ok then ask the device, so pass both without a GPU.  The
    launcher, the pairing rule and the GroupNorm-partials rule decide with the same function."""
    o = PdmGemmPlanOpts()
    if conv is not None:
        o.convH, o.convW, o.convC, o.conv_up = conv
    o.batch, o.act, o.gn_P, o.sk_attached = int(batch), int(act), int(gn_P), int(bool(sk_attached))
    o.algo, o.sk_mode, o.raster, o.dbg = int(algo), int(sk_mode), int(raster), int(dbg)
    o.mx_res_persist, o.ncu, o.persist_ok = int(mx_res_persist), int(ncu), int(persist_ok)
    out = (ctypes.c_int * 24)()
    check(load().pdm_gemm_plan(ctypes.byref(g), ctypes.byref(second) if second is not None else None, int(epi),
                               ctypes.byref(o), out), "pdm_gemm_plan")
    v = list(out)
    return GemmPlan(GEMM_PLAN_ERRORS[v[0]], GEMM_FAMILIES[v[1]] if v[1] >= 0 else None, *v[2:17], v[17],
                    *(bool(x) for x in v[18:23]), v[23])


def gemm_shape_args(M, N, K, epi, K1=None, copy=False, ln=False, stats=False, accumulate=False, fp8=False,
                    out_fp8=False, gather=None, out2=None, conv_C=0):
    """PdmGemmArgs of a GEMM on dense, aligned operands -- what the wrappers above pass for contiguous tensors -- on
    stand-in addresses, for gemm_plan (which dereferences nothing).  K1 < K: the split-K second operand; copy: the
    fp32 epilogue's bf16 copy; ln / stats: LayerNorm consumer / producer; out_fp8: the MXFP8 copy (alone on the bf16 /
    GELU epilogues); gather = (rows_per_group, group_stride); out2 likewise; conv_C: a conv's input channels."""
    g = PdmGemmArgs()
    at = iter(range(1 << 20, 1 << 26, 1 << 20))
    g.M, g.N, g.K, g.K1 = M, N, K, K if K1 is None else K1
    g.A1, g.lda1, g.W = next(at), conv_C or g.K1, next(at)
    if g.K1 < K:
        g.A2, g.lda2 = next(at), K - g.K1
    if epi == EPI_F32:
        g.out_f32, g.ldr = next(at), N
    if (epi != EPI_F32 and not (out_fp8 and epi != EPI_RES)) or copy:
        g.out_bf16, g.ldo = next(at), N
    g.accumulate = int(accumulate)
    if accumulate and epi == EPI_RES:
        g.res_in, g.ldri = g.out_bf16, N
    if ln:
        g.ln_stats, g.ln_colsum, g.ln_eps = next(at), next(at), 1e-5
        g.ln_gcol = next(at) if fp8 else None
    if stats:
        g.stats_out = next(at)
    if fp8:
        g.fp8, g.a_scale, g.a_scale_ld, g.w_scale, g.w_scale_ld = 1, next(at), M, next(at), N
    if out_fp8:
        g.out_fp8, g.ldo8, g.out_scale, g.out_scale_ld = next(at), N, next(at), M
    if gather:
        g.a_rows_per_group, g.a_group_stride = gather
    if out2:
        g.out2, (g.out2_rows_per_group, g.out2_group_stride) = next(at), out2
        g.stats_out2 = next(at) if stats else None
    return g


def attention(qkv, B, L, H, Dh, scale=None, q_log2=False, out=None):
    """q_log2: q already carries Dh^-0.5 * log2(e) (pdm_attention_log2, the U-ViT forward's layout).
    qkv: bf16 rows of 3*H*Dh columns; its row stride is passed on (a multiple of 8 elements, so a view works).
    out: where to write, bf16 with >= B*L rows of H*Dh columns and unit column stride (a view with its own row stride,
    a multiple of 4 elements, is fine); allocated here when None."""
    lib = load()
    require_gpu(qkv)
    if out is None:
        out = torch.empty(B * L, H * Dh, dtype=torch.bfloat16, device=qkv.device)
    elif (out.dtype != torch.bfloat16 or out.dim() != 2 or out.shape[0] < B * L or out.shape[1] != H * Dh
          or out.stride(1) != 1 or out.device != qkv.device):
        raise ValueError(f"attention: out must be bf16 [>= {B * L}, {H * Dh}] with unit column stride on {qkv.device}, "
                         f"got {out.dtype} {tuple(out.shape)} strides {tuple(out.stride())} on {out.device}")
    if q_log2:
        check(lib.pdm_attention_log2(ptr(qkv), qkv.stride(0), ptr(out), out.stride(0), B, L, H, Dh,
                                     stream_ptr(qkv.device)), "pdm_attention_log2")
        return out
    scale = Dh ** -0.5 if scale is None else scale
    check(lib.pdm_attention(ptr(qkv), qkv.stride(0), ptr(out), out.stride(0), B, L, H, Dh, scale,
                            stream_ptr(qkv.device)), "pdm_attention")
    return out


def lincomb(terms, coeffs, out=None):
    """out = sum_i coeffs[i] * terms[i] (fp32, same shape, contiguous)."""
    lib = load()
    t0 = terms[0]
    require_gpu(t0)
    n = len(terms)
    if n > 8:
        raise ValueError("lincomb supports at most 8 terms")
    if out is None:
        out = torch.empty_like(t0)
    arr = (ctypes.c_void_p * max(n, 1))(*[t.data_ptr() for t in terms])
    cs = (ctypes.c_float * max(n, 1))(*[float(c) for c in coeffs])
    check(lib.pdm_lincomb(ptr(out), n, arr, cs, t0.numel(), stream_ptr(t0.device)), "pdm_lincomb")
    return out


def stage_epilogue(pre, B, conv_w=None, conv_b=None, cfg_scale=None, act_tanh=False, xin=None, ax=0.0, ae=1.0,
                   m_out=None, terms=(), coeffs=(), cm=0.0, x_out=None, x_out2=None, x_out3=None):
    """See pdm_stage_epilogue in include/pdm.h.  pre [B or 2B, C, H, W] fp32 contiguous."""
    lib = load()
    require_gpu(pre)
    _, C, H, W = pre.shape
    a = PdmStageEpilogueArgs()
    a.pre = pre.data_ptr()
    a.conv_w = conv_w.data_ptr() if conv_w is not None else None
    a.conv_b = conv_b.data_ptr() if conv_b is not None else None
    a.B, a.C, a.H, a.W = B, C, H, W
    a.has_uncond = int(cfg_scale is not None)
    a.cfg_scale = float(cfg_scale or 0.0)
    a.act_tanh = int(act_tanh)
    a.xin = xin.data_ptr() if xin is not None else None
    a.ax, a.ae = float(ax), float(ae)
    a.m_out = m_out.data_ptr() if m_out is not None else None
    if len(terms) > 6:
        raise ValueError("stage_epilogue supports at most 6 terms")
    a.n_terms = len(terms)
    for i, (t, c) in enumerate(zip(terms, coeffs)):
        a.T[i] = t.data_ptr()
        a.c[i] = float(c)
    a.cm = float(cm)
    a.x_out = x_out.data_ptr() if x_out is not None else None
    a.x_out2 = x_out2.data_ptr() if x_out2 is not None else None
    a.x_out3 = x_out3.data_ptr() if x_out3 is not None else None
    check(lib.pdm_stage_epilogue(ctypes.byref(a), stream_ptr(pre.device)), "pdm_stage_epilogue")


def em_step_args(pre, B, x, xin, table, counter, t_next, conv_w=None, conv_b=None, cfg_scale=None, seed=0,
                 sample_offset=0, sample_offset_dev=None):
    """The pdm_em_step_args of one Euler-Maruyama step (include/pdm.h); host-side checks only, no GPU call.
    sample_offset_dev: an int64 device tensor whose first element is added to sample_offset by the kernel."""
    if pre.dim() != 4:
        raise ValueError("em_step: pre must be [B or 2B, C, H, W]")
    rows = 2 * B if cfg_scale is not None else B
    _, C, H, W = pre.shape
    if B <= 0 or pre.shape[0] != rows or tuple(x.shape) != (B, C, H, W) or tuple(xin.shape) != (rows, C, H, W):
        raise ValueError(f"em_step: pre / xin must hold {rows} rows and x {B} rows of one [C, H, W] shape")
    if table.dim() != 2 or table.shape[1] != 4 or table.shape[0] < 1 or table.dtype != torch.float32:
        raise ValueError("em_step: table must be fp32 [steps, 4] with steps >= 1")
    if counter.dtype != torch.int32 or counter.numel() < 1:
        raise ValueError("em_step: counter must be an int32 tensor")
    if t_next.dtype != torch.float32 or t_next.numel() != rows:
        raise ValueError(f"em_step: t_next must be fp32 [{rows}]")
    for t in (pre, x, xin, table):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("em_step: tensors must be contiguous fp32")
    if (conv_w is None) != (conv_b is None):
        raise ValueError("em_step: conv weight and bias go together")
    if not 0 <= int(seed) < 2 ** 64 or not 0 <= int(sample_offset) < 2 ** 64:
        raise ValueError("em_step: seed and sample_offset must fit 64 bits")
    a = PdmEmStepArgs()
    a.pre = pre.data_ptr()
    a.conv_w = conv_w.data_ptr() if conv_w is not None else None
    a.conv_b = conv_b.data_ptr() if conv_b is not None else None
    a.B, a.C, a.H, a.W = B, C, H, W
    a.has_uncond = int(cfg_scale is not None)
    a.cfg_scale = float(cfg_scale or 0.0)
    a.x, a.xin = x.data_ptr(), xin.data_ptr()
    a.table, a.steps = table.data_ptr(), table.shape[0]
    a.counter, a.t_next = counter.data_ptr(), t_next.data_ptr()
    a.seed, a.sample_offset = int(seed), int(sample_offset)
    if sample_offset_dev is not None:
        if sample_offset_dev.dtype != torch.int64 or sample_offset_dev.numel() < 1:
            raise ValueError("em_step: sample_offset_dev must be an int64 tensor")
        a.sample_offset_dev = sample_offset_dev.data_ptr()
    return a


def em_step(pre, B, x, xin, table, counter, t_next, **kw):
    """One Euler-Maruyama step on the GPU (pdm_em_step): x, xin, t_next and counter are updated in place."""
    a = em_step_args(pre, B, x, xin, table, counter, t_next, **kw)
    require_gpu(pre)
    check(load().pdm_em_step(ctypes.byref(a), stream_ptr(pre.device)), "pdm_em_step")


def philox_normal(B, per_sample, seed=0, sample_offset=0, step=0, device="cuda", raw=False):
    """The noise pdm_em_step draws at `step` for samples sample_offset .. + B - 1 (pdm_philox_normal): fp32
    [B, per_sample]; raw=True returns the Philox words instead (pdm_philox_raw: int32 holding the uint32 bits)."""
    if B <= 0 or per_sample <= 0 or step < 0:
        raise ValueError("philox_normal: B, per_sample must be positive and step >= 0")
    if not 0 <= int(seed) < 2 ** 64 or not 0 <= int(sample_offset) < 2 ** 64:
        raise ValueError("philox_normal: seed and sample_offset must fit 64 bits")
    require_gpu()
    dev = torch.device(device)
    out = torch.empty(B, per_sample, dtype=torch.int32 if raw else torch.float32, device=dev)
    fn = load().pdm_philox_raw if raw else load().pdm_philox_normal
    check(fn(ptr(out), B, per_sample, int(seed), int(sample_offset), int(step), stream_ptr(dev)),
          "pdm_philox_raw" if raw else "pdm_philox_normal")
    return out


def wgrad(dy, x, out=None, accumulate=False, scratch_mb=64):
    """Weight gradient dW = dy^T @ x (fp32 [N, K]) of bf16 rows dy [M, N], x [M, K] (pdm_wgrad)."""
    lib = load()
    require_gpu(dy)
    M, N = dy.shape
    K = x.shape[1]
    if out is None:
        out = torch.zeros(N, K, dtype=torch.float32, device=dy.device)
    scratch = torch.empty(scratch_mb << 18, dtype=torch.float32, device=dy.device) if scratch_mb else None
    check(lib.pdm_wgrad(ptr(dy), dy.stride(0), ptr(x), x.stride(0), ptr(out), out.stride(0), M, N, K, int(accumulate),
                        ptr(scratch), scratch.numel() * 4 if scratch is not None else 0, stream_ptr(dy.device)),
          "pdm_wgrad")
    return out


# what pdm_attention_backward (no scratch, the head-in-LDS kernels) takes per head dim (include/pdm.h)
_ATTN_BWD_MAXL = {64: 608, 72: 415}


def attention_backward(qkv, o, dout, B, L, H, Dh=64, algo=0, out=None, scratch=None):
    """d qkv (bf16 [B*L, 3*H*Dh]) of softmax attention (scale Dh^-0.5) from the forward's packed qkv, its output o
    and the output gradient dout.  algo 0: the head-in-LDS kernels up to their limits (Dh 64: L <= 608, Dh 72:
    L <= 415), the streaming kernels above; 1: the former only; 2: the streaming kernels at any L.  Goes through
    pdm_attention_backward_ex with a scratch allocated here (or `scratch`, an fp32 tensor of at least
    pdm_attention_backward_scratch_size bytes); a plain call within the old limits keeps the scratch-free
    pdm_attention_backward, which runs the same kernels.  out: where to write (>= B*L rows of qkv's layout)."""
    lib = load()
    require_gpu(qkv)
    dqkv = torch.empty_like(qkv) if out is None else out
    if algo == 0 and scratch is None and L <= _ATTN_BWD_MAXL.get(Dh, 0):
        check(lib.pdm_attention_backward(ptr(qkv), ptr(o), ptr(dout), ptr(dqkv), B, L, H, Dh, stream_ptr(qkv.device)),
              "pdm_attention_backward")
        return dqkv
    if scratch is None:
        nbytes = ctypes.c_size_t(0)
        check(lib.pdm_attention_backward_scratch_size(B, L, H, Dh, ctypes.byref(nbytes)),
              "pdm_attention_backward_scratch_size")
        scratch = torch.empty((nbytes.value + 3) // 4, dtype=torch.float32, device=qkv.device)
    check(lib.pdm_attention_backward_ex(ptr(qkv), ptr(o), ptr(dout), ptr(dqkv), B, L, H, Dh, int(algo), ptr(scratch),
                                        scratch.numel() * 4, stream_ptr(qkv.device)), "pdm_attention_backward_ex")
    return dqkv


def layernorm_backward(x, dh, gamma, dx=None, accumulate=False):
    """(dx fp32, dx bf16, dgamma, dbeta) of nn.LayerNorm(D) over fp32 rows x with output gradient dh (fp32 / bf16)."""
    lib = load()
    require_gpu(x)
    rows, D = x.shape
    if dx is None:
        dx = torch.zeros(rows, D, dtype=torch.float32, device=x.device)
    dxb = torch.empty(rows, D, dtype=torch.bfloat16, device=x.device)
    dg = torch.empty(D, dtype=torch.float32, device=x.device)
    db = torch.empty(D, dtype=torch.float32, device=x.device)
    scratch = torch.empty((4 * ((rows + 3) // 4) + 8) * 2 * D, dtype=torch.float32, device=x.device)
    check(lib.pdm_layernorm_backward(ptr(x), ptr(dh), int(dh.dtype == torch.bfloat16), ptr(gamma), ptr(dx), ptr(dxb),
                                     ptr(dg), ptr(db), rows, D, int(accumulate), ptr(scratch), scratch.numel() * 4,
                                     stream_ptr(x.device)), "pdm_layernorm_backward")
    return dx, dxb, dg, db


# ---- the training step's other kernels on their own (include/pdm.h, parity tests) ------------------------------
# The caller owns every tensor, outputs included (tests pre-fill them with sentinels); a gather is (rpg, gs, off).

def _nbytes(t):
    return t.numel() * t.element_size() if t is not None else 0


def wgrad_gather(a, lda, b, ldb, c, ldc, M, N, K, a_gather=(0, 0, 0), b_gather=(0, 0, 0), accumulate=False,
                 bias_out=None, bias_acc=False, scratch=None):
    """pdm_wgrad_gather: c[n][k] (+)= sum_m a[ga(m)][n] b[gb(m)][k], bias_out[n] (+)= sum_m a[ga(m)][n]."""
    require_gpu(a)
    check(load().pdm_wgrad_gather(ptr(a), lda, int(a_gather[0]), int(a_gather[1]), int(a_gather[2]), ptr(b), ldb,
                                  int(b_gather[0]), int(b_gather[1]), int(b_gather[2]), ptr(c), ldc, M, N, K,
                                  int(accumulate), ptr(bias_out), int(bias_acc), ptr(scratch), _nbytes(scratch),
                                  stream_ptr(a.device)), "pdm_wgrad_gather")


def colsum(x, ld, rows, ncols, dst, gather=(0, 0, 0), accumulate=False, scratch=None):
    """pdm_colsum: dst[c] (+)= sum_r x[gather(r)][c] of fp32 / bf16 x."""
    require_gpu(x)
    check(load().pdm_colsum(ptr(x), int(x.dtype == torch.bfloat16), ld, rows, ncols, int(gather[0]), int(gather[1]),
                            int(gather[2]), ptr(dst), int(accumulate), ptr(scratch), _nbytes(scratch),
                            stream_ptr(x.device)), "pdm_colsum")


def layernorm_backward_rows(x, ldx, dh, lddh, gamma, dx, lddx, dxb, dgamma, dbeta, rows, D, scratch, gather=(0, 0, 0),
                            eps=1e-5, accumulate=False, accumulate_params=False):
    """pdm_layernorm_backward_rows (the general form of layernorm_backward)."""
    require_gpu(x)
    check(load().pdm_layernorm_backward_rows(ptr(x), ldx, ptr(dh), int(dh.dtype == torch.bfloat16), lddh, ptr(gamma),
                                             ptr(dx), lddx, ptr(dxb), ptr(dgamma), ptr(dbeta), rows, D, int(gather[0]),
                                             int(gather[1]), int(gather[2]), eps, int(accumulate),
                                             int(accumulate_params), ptr(scratch), _nbytes(scratch),
                                             stream_ptr(x.device)), "pdm_layernorm_backward_rows")


def layernorm_rows(x, ldx, gamma, beta, y, ldy, rows, D, gather, eps=1e-5):
    """pdm_layernorm_rows: y[r] = LayerNorm(x[gather(r)]) (bf16); gather = (rows_per_group > 0, group_stride, offset)."""
    require_gpu(x)
    check(load().pdm_layernorm_rows(ptr(x), ldx, ptr(gamma), ptr(beta), ptr(y), ldy, rows, D, int(gather[0]),
                                    int(gather[1]), int(gather[2]), eps, stream_ptr(x.device)), "pdm_layernorm_rows")


def gelu_forward(u, g, n=None):
    require_gpu(u)
    check(load().pdm_gelu_forward(ptr(u), ptr(g), u.numel() if n is None else n, stream_ptr(u.device)),
          "pdm_gelu_forward")


def gelu_backward(dg, u, n=None):
    require_gpu(u)
    check(load().pdm_gelu_backward(ptr(dg), ptr(u), u.numel() if n is None else n, stream_ptr(u.device)),
          "pdm_gelu_backward")


def lsimple(pred, target, loss, dpred, B, per, gscale, tanh_bwd=False):
    require_gpu(pred)
    check(load().pdm_lsimple(ptr(pred), ptr(target), ptr(loss), ptr(dpred), B, per, float(gscale), int(tanh_bwd),
                             stream_ptr(pred.device)), "pdm_lsimple")


GRAD_NORM_SCRATCH_BYTES = 4096   # PDM_GRAD_NORM_SCRATCH_BYTES: enough for any n


def grad_norm_clip(g, g2, n, max_norm, out2, scratch):
    """pdm_grad_norm_clip: out2 = {||g (+ g2)||, coef}; with max_norm > 0, g (and g2) *= coef in place if coef < 1."""
    require_gpu(g)
    check(load().pdm_grad_norm_clip(ptr(g), ptr(g2), int(n), float(max_norm), ptr(out2), ptr(scratch),
                                    _nbytes(scratch), stream_ptr(g.device)), "pdm_grad_norm_clip")


def conv3x3_backward(dout, x, w, din, dw, db):
    """pdm_conv3x3_backward of nn.Conv2d(C, C, 3, padding=1): dout, x [B, C, H, W], w [C, C, 3, 3]."""
    require_gpu(dout)
    B, C, H, W = dout.shape
    check(load().pdm_conv3x3_backward(ptr(dout), ptr(x), ptr(w), ptr(din), ptr(dw), ptr(db), B, C, H, W,
                                      stream_ptr(dout.device)), "pdm_conv3x3_backward")


def head_forward(x, ldx, group_stride, row_offset, w, bias, out, B, D, C, p, H, W, P_pad, act_tanh=False):
    require_gpu(x)
    check(load().pdm_head_forward(ptr(x), ldx, group_stride, row_offset, ptr(w), ptr(bias), ptr(out), B, D, C, p, H, W,
                                  P_pad, int(act_tanh), stream_ptr(x.device)), "pdm_head_forward")


def head_backward(dpre, w, dtok, dx, B, D, C, p, H, W, P_pad):
    require_gpu(dpre)
    check(load().pdm_head_backward(ptr(dpre), ptr(w), ptr(dtok), ptr(dx), B, D, C, p, H, W, P_pad,
                                   stream_ptr(dpre.device)), "pdm_head_backward")


def assemble(img, p, patch_w, patch_b, pos, out, ld_out, D, L_total, row0_patch, t=None, time_emb=None, time_row=-1,
             y=None, label_emb=None, label_row=-1, ctx_tokens=None, ctx_row=-1):
    """pdm_assemble: token assembly of img [B, C, H, W] into out [B][L_total][ld_out]."""
    require_gpu(img)
    a = PdmAssembleArgs()
    a.img = img.data_ptr()
    a.B, a.C, a.Himg, a.Wimg = img.shape
    a.p = p
    a.patch_w, a.patch_b, a.pos, a.out = patch_w.data_ptr(), patch_b.data_ptr(), pos.data_ptr(), out.data_ptr()
    a.t = t.data_ptr() if t is not None else None
    a.time_emb = time_emb.data_ptr() if time_emb is not None else None
    a.y = y.data_ptr() if y is not None else None
    a.label_emb = label_emb.data_ptr() if label_emb is not None else None
    a.ctx_tokens = ctx_tokens.data_ptr() if ctx_tokens is not None else None
    a.n_ctx = ctx_tokens.shape[1] if ctx_tokens is not None else 0
    a.ld_out, a.D, a.L_total = ld_out, D, L_total
    a.row0_patch, a.time_row, a.label_row, a.ctx_row = row0_patch, time_row, label_row, ctx_row
    check(load().pdm_assemble(ctypes.byref(a), stream_ptr(img.device)), "pdm_assemble")


def patchify(img, pv, p, ldp):
    require_gpu(img)
    B, C, H, W = img.shape
    check(load().pdm_patchify(ptr(img), ptr(pv), B, C, H, W, p, ldp, stream_ptr(img.device)), "pdm_patchify")


def label_scatter(dx, L, row, D, y, dlab, B):
    require_gpu(dx)
    check(load().pdm_label_scatter(ptr(dx), L, row, D, ptr(y), ptr(dlab), B, stream_ptr(dx.device)),
          "pdm_label_scatter")


def rows_add_cast(dst, dstb, dst_gather, src, src_gather, rows, D, accumulate=False):
    require_gpu(dst)
    check(load().pdm_rows_add_cast(ptr(dst), ptr(dstb), int(dst_gather[0]), int(dst_gather[1]), int(dst_gather[2]),
                                   ptr(src), int(src_gather[0]), int(src_gather[1]), int(src_gather[2]), rows, D,
                                   int(accumulate), stream_ptr(dst.device)), "pdm_rows_add_cast")


def add_cast(dx, add, dxb, n=None):
    require_gpu(dx)
    check(load().pdm_add_cast(ptr(dx), ptr(add), ptr(dxb), dx.numel() if n is None else n, stream_ptr(dx.device)),
          "pdm_add_cast")


def transpose_bf16(w, wt, N, K):
    require_gpu(w)
    check(load().pdm_transpose_bf16(ptr(w), ptr(wt), N, K, stream_ptr(w.device)), "pdm_transpose_bf16")


class GemmProfiler:
    """HIP-event timing of every GEMM launch of a forward (pdm_uvit_profile)."""

    def __init__(self, native, max_launches=512):
        self.nat = native
        self.cap = max_launches

    def enable(self):
        check(self.nat.lib.pdm_uvit_profile(self.nat.h, self.cap), "pdm_uvit_profile")

    def disable(self):
        check(self.nat.lib.pdm_uvit_profile(self.nat.h, 0), "pdm_uvit_profile")

    def read(self):
        ms = (ctypes.c_float * self.cap)()
        fl = (ctypes.c_double * self.cap)()
        n = ctypes.c_int()
        check(self.nat.lib.pdm_uvit_profile_read(self.nat.h, ms, fl, self.cap, ctypes.byref(n)), "pdm_uvit_profile_read")
        k = min(n.value, self.cap)
        return [ms[i] for i in range(k)], [fl[i] for i in range(k)]
