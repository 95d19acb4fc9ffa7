"""ctypes binding of include/captioner_hip.h (libcaptioner_hip.so).

There is no fallback: if the library cannot be found, built or loaded this module raises - the product path never
routes through PyTorch ops or the test oracle.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libcaptioner_hip.so")

CAP_F32, CAP_BF16, CAP_F32_SPLIT = 0, 1, 2
CAP_PIX_F32_NCHW, CAP_PIX_U8_NHWC = 0, 1
CAP_PIX_IMAGE_STATE = 2  # `pixels` = B image-state records (cap_encode_image_state): the decoding calls only
CAP_ARCH_CLIP = 4
CAP_ARCH_BLIP2_ITM = 5
CAP_ACT_QUICK_GELU, CAP_ACT_GELU = 0, 1
CAP_MAX_PROMPT = 32      # prompt tokens per caption (BOS included) cap_generate_prompted takes


class CapConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("arch", C.c_int32), ("compute_dtype", C.c_int32),
        ("image_size", C.c_int32), ("patch_size", C.c_int32), ("v_hidden", C.c_int32), ("v_layers", C.c_int32),
        ("v_heads", C.c_int32), ("v_mlp", C.c_int32), ("v_eps", C.c_float),
        ("t_hidden", C.c_int32), ("t_layers", C.c_int32), ("t_heads", C.c_int32), ("t_ffn", C.c_int32),
        ("vocab", C.c_int32), ("max_pos", C.c_int32), ("t_eps", C.c_float),
        ("bos", C.c_int32), ("eos", C.c_int32), ("pad", C.c_int32),
        ("max_batch", C.c_int32), ("max_beams", C.c_int32), ("max_len", C.c_int32),
        ("pix_mean", C.c_float * 3), ("pix_std", C.c_float * 3),
        ("embed_dim", C.c_int32), ("pool_queries", C.c_int32), ("pool_heads", C.c_int32), ("mm_layers", C.c_int32),
        ("min_len", C.c_int32),
        ("q_hidden", C.c_int32), ("q_layers", C.c_int32), ("q_heads", C.c_int32), ("q_ffn", C.c_int32),
        ("q_cross_freq", C.c_int32), ("num_query_tokens", C.c_int32), ("q_eps", C.c_float),
        ("cross_kv_fp32", C.c_int32), ("weight_int8", C.c_int32), ("hidden_act", C.c_int32),
        ("max_prompt", C.c_int32), ("max_score_rows", C.c_int32),
    ]


class CapSmallLN(C.Structure):
    _fields_ = [
        ("part", C.c_void_p), ("S", C.c_int32), ("bias", C.c_void_p), ("resid", C.c_void_p), ("gamma", C.c_void_p),
        ("beta", C.c_void_p), ("eps", C.c_float), ("x_out", C.c_void_p), ("x_is_sum", C.c_int32),
    ]


class CapSmallSA(C.Structure):
    _fields_ = [
        ("qkv_part", C.c_void_p), ("qkv_bias", C.c_void_p), ("qkv_S", C.c_int32), ("kc", C.c_void_p), ("vc", C.c_void_p),
        ("anc", C.c_void_p), ("anc_ld", C.c_int32), ("kv_ld", C.c_int32), ("n_keys", C.c_int32), ("H", C.c_int32),
        ("skip", C.c_void_p),
    ]


class CapSmallGemm(C.Structure):
    _fields_ = [
        ("W", C.c_void_p), ("A", C.c_void_p), ("R", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("S", C.c_int32),
        ("pro", C.c_int32), ("epi", C.c_int32), ("nchain", C.c_int32), ("ln", CapSmallLN), ("sa", CapSmallSA),
        ("out_part", C.c_void_p), ("bias", C.c_void_p), ("act", C.c_int32), ("out", C.c_void_p), ("ldc", C.c_int32),
    ]


class CapSmallCross(C.Structure):
    _fields_ = [
        ("W", C.c_void_p), ("bias", C.c_void_p), ("R", C.c_int32), ("D", C.c_int32), ("H", C.c_int32), ("S", C.c_int32),
        ("ln", CapSmallLN), ("kbase", C.c_void_p), ("vbase", C.c_void_p), ("kv_row0", C.c_size_t),
        ("rows_per_kv", C.c_int32), ("kv_ld", C.c_int32), ("n_keys", C.c_int32), ("kv_kind", C.c_int32),
        ("skip", C.c_void_p), ("out", C.c_void_p),
    ]


class CapGemmEpi(C.Structure):
    _fields_ = [
        ("A", C.c_void_p), ("lda", C.c_int32), ("W", C.c_void_p), ("ldw", C.c_int32), ("bias", C.c_void_p), ("C", C.c_void_p),
        ("ldc", C.c_int32), ("C2", C.c_void_p), ("aux", C.c_void_p),
        ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("gelu", C.c_int32), ("out_f32", C.c_int32), ("epi", C.c_int32),
        ("splitk", C.c_int32), ("p0", C.c_int32), ("p1", C.c_int32), ("p2", C.c_int32), ("p3", C.c_int32), ("kv16", C.c_int32),
        ("m_live", C.c_void_p), ("tile", C.c_int32),
    ]


class CapGenerateArgs(C.Structure):
    _fields_ = [
        ("pixels", C.c_void_p), ("pixel_fmt", C.c_int32), ("B", C.c_int32), ("num_beams", C.c_int32), ("num_beam_groups", C.c_int32),
        ("max_len", C.c_int32), ("length_penalty", C.c_float), ("out_ids", C.c_void_p), ("out_len", C.c_void_p),
        ("out_scores", C.c_void_p), ("out_step_logits", C.c_void_p), ("out_logprobs", C.c_void_p), ("out_scored", C.c_void_p),
        ("out_vocab", C.c_void_p), ("acc_ld", C.c_int32), ("prompt_ids", C.c_void_p), ("prompt_rows", C.c_int32),
        ("prompt_len", C.c_int32),
    ]


_SIGNATURES = {
    "cap_last_error": (C.c_char_p, []),
    "cap_version": (C.c_int, []),
    "cap_create": (C.c_int, [C.POINTER(CapConfig), C.POINTER(C.c_void_p)]),
    "cap_create_shared": (C.c_int, [C.POINTER(CapConfig), C.c_void_p, C.POINTER(C.c_void_p)]),
    "cap_destroy": (C.c_int, [C.c_void_p]),
    "cap_load_weight": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_void_p]),
    "cap_finalize_weights": (C.c_int, [C.c_void_p]),
    "cap_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cap_image_state_bytes": (C.c_size_t, [C.c_void_p]),
    "cap_encode_image_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cap_generate_request": (C.c_int, [C.c_void_p, C.POINTER(CapGenerateArgs), C.c_void_p]),
    "cap_generate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cap_generate_scored": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cap_generate_vocab": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "cap_generate_prompted": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "cap_last_prefill_passes": (C.c_int, [C.c_void_p]),
    "cap_score_captions": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cap_last_score_passes": (C.c_int, [C.c_void_p]),
    "cap_score_pass_captions": (C.c_int, [C.c_void_p, C.c_int]),
    "cap_embed_text": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cap_crop_resize_tables": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "cap_crop_resize_u8": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                     C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cap_crop_resize_u8_frames": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                            C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cap_generate_groups": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    "cap_set_early_exit": (C.c_int, [C.c_void_p, C.c_int]),
    "cap_last_decode_steps": (C.c_int, [C.c_void_p]),
    "cap_set_bad_words": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "cap_bad_words": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "cap_op_ban_words": (C.c_int, [C.c_int]),
    "cap_op_select_banned": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "cap_op_beam_step_banned": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                          C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "cap_set_repeat_controls": (C.c_int, [C.c_void_p, C.c_float, C.c_int]),
    "cap_repeat_controls": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "cap_set_image_token": (C.c_int, [C.c_void_p, C.c_int]),
    "cap_op_select_processed": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int,
                                          C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "cap_op_beam_step_processed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                             C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int,
                                             C.c_int, C.c_void_p]),
    "cap_generate_sampled": (C.c_int, [C.c_void_p, C.POINTER(CapGenerateArgs), C.c_void_p, C.c_void_p]),
    "cap_set_sampling": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_float, C.c_uint64]),
    "cap_sampling": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_float),
                               C.POINTER(C.c_uint64)]),
    "cap_op_select_sampled": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int,
                                        C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, C.c_uint64, C.c_void_p, C.c_int,
                                        C.c_void_p, C.c_void_p]),
    "cap_set_decode_path": (C.c_int, [C.c_void_p, C.c_int]),
    "cap_last_decode_path": (C.c_int, [C.c_void_p]),
    "cap_set_row_compaction": (C.c_int, [C.c_void_p, C.c_int]),
    "cap_last_row_compaction": (C.c_int, [C.c_void_p]),
    "cap_cross_cache_kind": (C.c_int, [C.c_void_p]),
    "cap_device_bytes": (C.c_size_t, [C.c_void_p]),
    "cap_debug_fill_arena": (C.c_longlong, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "cap_debug_arena_kinds": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t]),
    "cap_g8_saturations": (C.c_longlong, [C.c_int]),
    "cap_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "cap_profile_report": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t]),
    "cap_op_gemm": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                              C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "cap_op_pack_kv16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "cap_op_image_state_pack": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cap_op_image_state_unpack": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cap_op_gemm_crosskv": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "cap_op_gemm_partial": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "cap_op_layernorm": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p,
                                   C.c_int, C.c_int, C.c_void_p]),
    "cap_op_vit_attention": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "cap_op_reduce_layernorm": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "cap_op_gemm_skinny": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                     C.c_int, C.c_void_p]),
    "cap_op_gemm_skinny_slices": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "cap_op_quant_i8_pack": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "cap_op_gemm_skinny_i8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                        C.c_int, C.c_int, C.c_void_p]),
    "cap_op_gemm_skinny_i8_slices": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "cap_op_vit_attention_hd": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_void_p]),
    "cap_op_decode_attention": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                          C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "cap_op_decode_attention_fused": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                                C.c_int, C.c_int, C.c_void_p]),
    "cap_op_gemm_live": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_int, C.c_void_p, C.c_void_p]),
    "cap_op_layernorm_live": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                        C.c_void_p, C.c_void_p]),
    "cap_op_decode_attention_live": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                               C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                               C.c_int, C.c_void_p]),
    "cap_op_small_gemm": (C.c_int, [C.c_int, C.POINTER(CapSmallGemm), C.c_void_p]),
    "cap_op_small_cross": (C.c_int, [C.c_int, C.POINTER(CapSmallCross), C.c_void_p]),
    "cap_op_gemm_epi": (C.c_int, [C.c_int, C.POINTER(CapGemmEpi), C.c_void_p]),
    "cap_op_beam_candidates": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    "cap_op_beam_state_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "cap_op_beam_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "cap_op_beam_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                   C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "cap_op_beam_finalize": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cap_op_beam_peek": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cap_clip_embed_images": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cap_clip_embed_text": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cap_clip_logits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_void_p]),
    "cap_clip_logit_scale": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "cap_cosine_matrix": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "cap_group_similarity_workspace": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "cap_group_similarity": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "cap_blip2_itm_encode_images": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "cap_blip2_itc_image_features": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "cap_blip2_itc_text_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cap_blip2_itc_scores": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "cap_blip2_itm_logits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cap_op_generic_attention": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "cap_op_itm_self_attention": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                            C.c_int, C.c_int, C.c_void_p]),
    "cap_op_attention": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64,
                                   C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "cap_op_opt_decode_attention": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                              C.c_int, C.c_void_p]),
    "cap_op_opt_prefix_attention": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                              C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "cap_op_opt_beam_decode_attention": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                   C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "cap_op_kv_append": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "cap_op_prefill_self_attention": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                                C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "cap_op_opt_prefill_inputs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "cap_op_opt_token_inputs": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                          C.c_void_p]),
    "cap_op_rows_broadcast": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "cap_op_dequant_i8_rowmajor": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "cap_op_scale_cols": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "cap_op_pool_attention": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "cap_op_text_attention": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "cap_op_target_logprob": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "cap_op_select_logprob": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                        C.c_void_p]),
    "cap_op_select_vocab": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                      C.c_void_p, C.c_int, C.c_void_p]),
    "cap_op_vocab_group_threshold": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float,
                                               C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cap_op_embed": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cap_op_embed_prompt": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "cap_op_embed_tokens": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "cap_op_init_prompt_seq": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                         C.c_int, C.c_void_p]),
    "cap_op_compact_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cap_op_reduce_bias_act": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "cap_op_mean_pool_normalize": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cap_op_patchify": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p]),
    "cap_op_cls_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "cap_op_convert2d": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p]),
    "cap_op_absmax": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "cap_op_convert": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "cap_op_convert_weight": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "cap_op_clip_embed_text": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "cap_op_clip_head": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_int,
                                   C.c_int, C.c_int, C.c_void_p]),
    "cap_op_itm_embed_text": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float,
                                        C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "cap_op_itc_head": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "cap_op_itm_head": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
}

EXPORTS = tuple(_SIGNATURES)

_lib = None
_lock = threading.Lock()


class CaptionerHipError(RuntimeError):
    pass


def load_library(build_if_missing: bool = True) -> C.CDLL:
    """Load (building first if the .so is absent and hipcc exists).  Raises CaptionerHipError otherwise."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            if not build_if_missing:
                raise CaptionerHipError(f"{LIB_PATH} is missing - run `python -m embodied_captioning_amd.build`")
            from . import build as _build
            try:
                _build.build(verbose=False)
            except Exception as e:  # noqa: BLE001
                raise CaptionerHipError(f"HIP extension missing and could not be built: {e}") from e
        # torch (when present) must load its bundled HIP runtime first so both share one libamdhip64.so.7
        try:
            import torch  # noqa: F401
        except Exception:  # noqa: BLE001
            pass
        try:
            lib = C.CDLL(LIB_PATH)
        except OSError as e:
            raise CaptionerHipError(f"cannot load {LIB_PATH}: {e}") from e
        for name, (res, args) in _SIGNATURES.items():
            try:
                fn = getattr(lib, name)
            except AttributeError as e:
                raise CaptionerHipError(f"{LIB_PATH} does not export {name}") from e
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return lib


def last_error() -> str:
    return load_library().cap_last_error().decode(errors="replace")


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise CaptionerHipError(f"{what} failed (rc={rc}): {last_error()}")
