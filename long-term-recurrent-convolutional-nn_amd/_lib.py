"""ctypes binding of liblrcn_hip.so (the C ABI declared in include/lrcn.h).

There is NO fallback: if the shared library is missing or a symbol is absent this module raises, and every
compute entry point needs a visible MI355X.  Nothing here imports or calls the CPU oracle.
"""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_PATH = os.environ.get("LRCN_HIP_LIB") or os.path.join(CSRC, "liblrcn_hip.so")  # override: A/B builds of the kernels in one session
HEADER = os.path.normpath(os.path.join(HERE, "..", "include", "lrcn.h"))
SAMPLE_HEADER = os.path.normpath(os.path.join(HERE, "..", "include", "lrcn_sample.h"))  # lrcn_sample_batch (not in lrcn.h)
SCORE_HEADER = os.path.normpath(os.path.join(HERE, "..", "include", "lrcn_score.h"))    # lrcn_score_matrix / _pairs (not in lrcn.h)
NUCLEUS_HEADER = os.path.normpath(os.path.join(HERE, "..", "include", "lrcn_nucleus.h"))  # lrcn_sample_batch_p / lrcn_sample_logits (not in lrcn.h)
NBEST_HEADER = os.path.normpath(os.path.join(HERE, "..", "include", "lrcn_nbest.h"))    # lrcn_beam_nbest_batch (not in lrcn.h)
DIVERSE_HEADER = os.path.normpath(os.path.join(HERE, "..", "include", "lrcn_diverse.h"))  # lrcn_beam_diverse_batch (not in lrcn.h)
CONSTRAIN_HEADER = os.path.normpath(os.path.join(HERE, "..", "include", "lrcn_constrain.h"))  # lrcn_beam_constrained_batch / lrcn_constrained_topk_logits (not in lrcn.h)
ENSEMBLE_HEADER = os.path.normpath(os.path.join(HERE, "..", "include", "lrcn_ensemble.h"))  # lrcn_beam_ensemble_batch / lrcn_ensemble_mix_logits (not in lrcn.h)
FORCED_HEADER = os.path.normpath(os.path.join(HERE, "..", "include", "lrcn_forced.h"))  # lrcn_beam_forced_batch / lrcn_forced_topk_logits (not in lrcn.h)
ACTIVITY_HEADER = os.path.normpath(os.path.join(HERE, "..", "include", "lrcn_activity.h"))  # lrcn_act_* (not in lrcn.h)
ACT_DROPOUT_HEADER = os.path.normpath(os.path.join(HERE, "..", "include", "lrcn_act_dropout.h"))  # lrcn_act_loss_grad_drop (not in lrcn_activity.h)
VARLEN_HEADER = os.path.normpath(os.path.join(HERE, "..", "include", "lrcn_varlen.h"))      # lrcn_*_var (not in lrcn.h)
CLIP_HEADER = os.path.normpath(os.path.join(HERE, "..", "include", "lrcn_clip.h"))          # lrcn_clip_* / *_clipped / *_clip (not in lrcn.h)
WEIGHTED_HEADER = os.path.normpath(os.path.join(HERE, "..", "include", "lrcn_weighted.h"))  # lrcn_*_w (not in lrcn.h)
SCHED_HEADER = os.path.normpath(os.path.join(HERE, "..", "include", "lrcn_sched.h"))        # lrcn_*_sched (not in lrcn.h)
SMOOTH_HEADER = os.path.normpath(os.path.join(HERE, "..", "include", "lrcn_smooth.h"))      # lrcn_*_smooth / lrcn_xent_logits (not in lrcn.h)
GEMM_DEBUG_HEADER = os.path.normpath(os.path.join(HERE, "..", "include", "lrcn_gemm_debug.h"))  # lrcn_debug_gemm (not in lrcn.h)
CONV_DEBUG_HEADER = os.path.normpath(os.path.join(HERE, "..", "include", "lrcn_conv_debug.h"))  # lrcn_debug_conv11 and the fp8 seams (not in lrcn.h)
DECODE_DEBUG_HEADER = os.path.normpath(os.path.join(HERE, "..", "include", "lrcn_decode_debug.h"))  # lrcn_debug_decode_steps (not in lrcn.h)
CIDER_HEADER = os.path.normpath(os.path.join(HERE, "..", "include", "lrcn_cider.h"))  # lrcn_cider_* (not in lrcn.h)

LRCN_F32, LRCN_BF16, LRCN_FP8 = 0, 1, 2
LRCN_ABI_VERSION = 5   # include/lrcn.h: the revision this binding's struct layouts and signatures were written against
LRCN_OPT_FUSED_UPDATE, LRCN_OPT_DETERMINISTIC, LRCN_OPT_CONV_CHUNK_BYTES = 1, 2, 3
SEGMENTS = ("update", "rec_fwd", "rec_bwd", "embed_gather", "embed_grad", "preprocess", "upload")   # LRCN_SEG_* of include/lrcn.h, in order
EOS, BOS, UNK = 0, 1, 2
CNNOUT = 4096
MAX_T = 28


class LrcnError(RuntimeError):
    pass


class Config(C.Structure):
    _fields_ = [("device", C.c_int), ("E", C.c_int), ("H1", C.c_int), ("H2", C.c_int), ("V", C.c_int),
                ("max_B", C.c_int), ("max_T", C.c_int), ("lstm_dtype", C.c_int), ("vgg_dtype", C.c_int),
                ("max_images", C.c_int), ("n_layers", C.c_int)]


class ActConfig(C.Structure):   # lrcn_act_config of include/lrcn_activity.h
    _fields_ = [("device", C.c_int), ("F", C.c_int), ("H", C.c_int), ("C", C.c_int), ("max_B", C.c_int), ("max_T", C.c_int),
                ("dtype", C.c_int), ("deterministic", C.c_int)]


class ActDropout(C.Structure):   # lrcn_act_dropout of include/lrcn_act_dropout.h
    _fields_ = [("p_in", C.c_float), ("p_out", C.c_float), ("seed", C.c_uint64), ("mask_in", C.c_void_p), ("mask_out", C.c_void_p)]


class GemmDebug(C.Structure):   # lrcn_gemm_debug of include/lrcn_gemm_debug.h
    _fields_ = [("dtype", C.c_int), ("A", C.c_void_p), ("B", C.c_void_p), ("C", C.c_void_p), ("bias", C.c_void_p),
                ("lda", C.c_int64), ("ldb", C.c_int64), ("ldc", C.c_int64), ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
                ("c_f32", C.c_int), ("beta", C.c_int), ("relu", C.c_int), ("c_is_zero", C.c_int), ("deterministic", C.c_int),
                ("free_cus", C.c_int), ("bg_cus", C.c_int), ("wg_cap", C.c_int)]


class ConvGemmDebug(C.Structure):   # lrcn_conv_gemm_debug of include/lrcn_gemm_debug.h
    _fields_ = [("dtype", C.c_int), ("x", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("y", C.c_void_p), ("ldc", C.c_int64),
                ("N", C.c_int), ("H", C.c_int), ("W", C.c_int), ("Cin", C.c_int), ("Cout", C.c_int), ("relu", C.c_int), ("pool", C.c_int),
                ("wg_cap", C.c_int)]


class Conv64Debug(C.Structure):   # lrcn_conv64_debug of include/lrcn_conv_debug.h
    _fields_ = [("x", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("y", C.c_void_p), ("N", C.c_int), ("H", C.c_int), ("W", C.c_int),
                ("Cout", C.c_int), ("relu", C.c_int), ("pool", C.c_int), ("wg_cap", C.c_int)]


class DecodeDebug(C.Structure):   # lrcn_decode_debug of include/lrcn_decode_debug.h
    _fields_ = [("params", C.POINTER(C.c_void_p)), ("feats", C.c_void_p), ("N", C.c_int), ("per_image", C.c_int), ("steps", C.c_int),
                ("tokens", C.POINTER(C.c_int32)), ("parents", C.POINTER(C.c_int32)), ("h1", C.c_void_p), ("h2", C.c_void_p),
                ("c1", C.c_void_p), ("c2", C.c_void_p), ("logits", C.c_void_p), ("route", C.c_int)]


class Constraints(C.Structure):   # lrcn_constraints of include/lrcn_constrain.h
    _fields_ = [("banned", C.POINTER(C.c_int32)), ("nbanned", C.c_int), ("min_len", C.c_int), ("no_repeat_ngram", C.c_int)]


class Forced(C.Structure):   # lrcn_forced of include/lrcn_forced.h
    _fields_ = [("words", C.POINTER(C.c_int32)), ("C", C.c_int), ("A", C.c_int)]


class Dropout(C.Structure):
    _fields_ = [("pdrop", C.c_float), ("seed", C.c_uint64), ("mask1", C.c_void_p), ("mask2", C.c_void_p)]


class Sched(C.Structure):   # lrcn_sched of include/lrcn_sched.h
    _fields_ = [("eps", C.c_float), ("temperature", C.c_float), ("seed", C.c_uint64), ("row0", C.c_int64)]


P9 = C.c_void_p * 9
P4 = C.c_void_p * 4
P13 = C.c_void_p * 13

# name -> (restype, argtypes); exactly the symbols include/lrcn.h declares
SIGNATURES = {
    "lrcn_create": (C.c_int, [C.POINTER(Config), C.POINTER(C.c_void_p)]),
    "lrcn_destroy": (None, [C.c_void_p]),
    "lrcn_last_error": (C.c_char_p, [C.c_void_p]),
    "lrcn_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lrcn_set_wg_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lrcn_sync": (C.c_int, [C.c_void_p]),
    "lrcn_malloc": (C.c_int, [C.POINTER(C.c_void_p), C.c_size_t]),
    "lrcn_free": (C.c_int, [C.c_void_p]),
    "lrcn_memcpy_h2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "lrcn_memcpy_d2h": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "lrcn_version": (C.c_char_p, []),
    "lrcn_abi_version": (C.c_int, []),
    "lrcn_set_option": (C.c_int, [C.c_void_p, C.c_int, C.c_int64]),
    "lrcn_params_touched": (C.c_int, [C.c_void_p]),
    "lrcn_comm_probe": (C.c_int, [C.c_void_p]),
    "lrcn_param_sizes": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "lrcn_param_sizes_n": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "lrcn_init_weights": (C.c_int, [C.c_void_p, P9, C.c_uint64]),
    "lrcn_lstm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                            C.c_void_p, C.c_void_p, C.c_void_p]),
    "lrcn_step": (C.c_int, [C.c_void_p, P9, P4, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lrcn_loss": (C.c_int, [C.c_void_p, P9, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Dropout),
                            C.POINTER(C.c_double)]),
    "lrcn_loss_grad": (C.c_int, [C.c_void_p, P9, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Dropout),
                                 P9, C.POINTER(C.c_double)]),
    "lrcn_refresh_shadows_group": (C.c_int, [C.c_void_p, P9, C.c_int, C.c_void_p]),
    "lrcn_avg_loss_batch": (C.c_int, [C.c_void_p, P9, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "lrcn_grad_group_wait": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "lrcn_last_loss": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "lrcn_forward_logits": (C.c_int, [C.c_void_p, P9, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "lrcn_adam_update": (C.c_int, [C.c_void_p, P9, P9, P9, P9, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float]),
    "lrcn_adam_update_group": (C.c_int, [C.c_void_p, P9, P9, P9, P9, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float,
                                         C.c_void_p]),
    "lrcn_adam_update_flat": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_float, C.c_float,
                                        C.c_float, C.c_void_p]),
    "lrcn_train_step": (C.c_int, [C.c_void_p, P9, P9, P9, P9, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                  C.POINTER(Dropout), C.c_int, C.c_float, C.c_float, C.c_float, C.c_float,
                                  C.POINTER(C.c_double)]),
    "lrcn_comm_unique_id": (C.c_int, [C.c_void_p]),
    "lrcn_comm_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "lrcn_comm_destroy": (C.c_int, [C.c_void_p]),
    "lrcn_comm_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lrcn_set_embed_rows_buffer": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "lrcn_embed_grad_from_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "lrcn_allreduce_grads": (C.c_int, [C.c_void_p, P9, C.c_int]),
    "lrcn_comm_join": (C.c_int, [C.c_void_p]),
    "lrcn_train_step_dp": (C.c_int, [C.c_void_p, P9, P9, P9, P9, C.c_void_p, C.POINTER(C.c_float), C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                     C.c_int, C.c_int, C.POINTER(Dropout), C.c_int, C.c_float, C.c_float, C.c_float, C.c_float,
                                     C.POINTER(C.c_double)]),
    "lrcn_beam_search": (C.c_int, [C.c_void_p, P9, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int32),
                                   C.POINTER(C.c_int), C.POINTER(C.c_float)]),
    "lrcn_beam_search_batch": (C.c_int, [C.c_void_p, P9, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32),
                                         C.POINTER(C.c_int), C.POINTER(C.c_float)]),
    "lrcn_vgg_load": (C.c_int, [C.c_void_p, P13, P13, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lrcn_vgg_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "lrcn_preprocess_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_void_p]),
    "lrcn_vgg_forward_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_void_p]),
    "lrcn_vgg_forward_u8_blocks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_void_p]),
    "lrcn_set_average_image": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lrcn_resize_crop_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                      C.c_int, C.c_void_p]),
    "lrcn_normalize_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "lrcn_host_alloc": (C.c_int, [C.POINTER(C.c_void_p), C.c_size_t]),
    "lrcn_host_free": (C.c_int, [C.c_void_p]),
    "lrcn_upload_crops": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "lrcn_upload_wait": (C.c_int, [C.c_void_p]),
    "lrcn_profile": (C.c_int, [C.c_void_p, C.c_int]),
    "lrcn_profile_get": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "lrcn_profile_segment": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "lrcn_debug_stamps": (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong), C.c_int64]),
    "lrcn_bench_conv": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "lrcn_bench_gemm": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "lrcn_conv1_fused": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p]),
    "lrcn_conv3x3": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                               C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "lrcn_vgg_set_wg_cap": (C.c_int, [C.c_void_p, C.c_int]),
    "lrcn_vgg_calibrate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_float]),
    "lrcn_debug_route": (C.c_char_p, [C.c_void_p, C.c_int]),
    "lrcn_conv3x3_fp8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                   C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
}

# name -> (restype, argtypes); exactly the symbols include/lrcn_sample.h declares (bound by lib() as well)
SAMPLE_SIGNATURES = {
    "lrcn_sample_batch": (C.c_int, [C.c_void_p, P9, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_uint64,
                                    C.POINTER(C.c_int32), C.POINTER(C.c_int), C.POINTER(C.c_float)]),
}

# name -> (restype, argtypes); exactly the symbols include/lrcn_nucleus.h declares (bound by lib() as well)
NUCLEUS_SIGNATURES = {
    "lrcn_sample_batch_p": (C.c_int, [C.c_void_p, P9, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, C.c_uint64,
                                      C.POINTER(C.c_int32), C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_int32)]),
    "lrcn_sample_logits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float,
                                     C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
}

# name -> (restype, argtypes); exactly the symbols include/lrcn_score.h declares (bound by lib() as well)
SCORE_SIGNATURES = {
    "lrcn_score_matrix": (C.c_int, [C.c_void_p, P9, C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_void_p]),
    "lrcn_score_pairs": (C.c_int, [C.c_void_p, P9, C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int), C.c_int, C.c_int,
                                   C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.c_void_p]),
}

# name -> (restype, argtypes); exactly the symbols include/lrcn_nbest.h declares (bound by lib() as well)
NBEST_SIGNATURES = {
    "lrcn_beam_nbest_batch": (C.c_int, [C.c_void_p, P9, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.POINTER(C.c_int32),
                                        C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
}

# name -> (restype, argtypes); exactly the symbols include/lrcn_diverse.h declares (bound by lib() as well)
DIVERSE_SIGNATURES = {
    "lrcn_beam_diverse_batch": (C.c_int, [C.c_void_p, P9, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float,
                                          C.POINTER(C.c_int32), C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
}

# name -> (restype, argtypes); exactly the symbols include/lrcn_constrain.h declares (bound by lib() as well)
CONSTRAIN_SIGNATURES = {
    "lrcn_beam_constrained_batch": (C.c_int, [C.c_void_p, P9, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float,
                                              C.POINTER(Constraints), C.POINTER(C.c_int32), C.POINTER(C.c_int), C.POINTER(C.c_float),
                                              C.POINTER(C.c_float)]),
    "lrcn_constrained_topk_logits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.POINTER(Constraints), C.c_void_p,
                                               C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
}

# name -> (restype, argtypes); exactly the symbols include/lrcn_ensemble.h declares (bound by lib() as well)
ENSEMBLE_SIGNATURES = {
    "lrcn_beam_ensemble_batch": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_float), C.c_int, C.c_void_p, C.c_int,
                                           C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, C.POINTER(Constraints), C.POINTER(C.c_int32),
                                           C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "lrcn_ensemble_mix_logits": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_int, C.POINTER(C.c_float), C.c_int,
                                           C.c_int, C.c_int, C.c_void_p, C.c_int64]),
}

# name -> (restype, argtypes); exactly the symbols include/lrcn_forced.h declares (bound by lib() as well)
FORCED_SIGNATURES = {
    "lrcn_beam_forced_batch": (C.c_int, [C.c_void_p, P9, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.POINTER(Constraints), C.POINTER(Forced),
                                         C.POINTER(C.c_int32), C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "lrcn_forced_topk_logits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.POINTER(Constraints), C.POINTER(C.c_int32),
                                          C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}

# name -> (restype, argtypes); exactly the symbols include/lrcn_activity.h declares (bound by lib() as well)
ACTIVITY_SIGNATURES = {
    "lrcn_act_create": (C.c_int, [C.POINTER(ActConfig), C.POINTER(C.c_void_p)]),
    "lrcn_act_destroy": (None, [C.c_void_p]),
    "lrcn_act_last_error": (C.c_char_p, [C.c_void_p]),
    "lrcn_act_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lrcn_act_param_sizes": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "lrcn_act_init_weights": (C.c_int, [C.c_void_p, P4, C.c_uint64]),
    "lrcn_act_loss_grad": (C.c_int, [C.c_void_p, P4, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_void_p,
                                     C.POINTER(C.c_double)]),
    "lrcn_act_predict": (C.c_int, [C.c_void_p, P4, C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
}

# name -> (restype, argtypes); exactly the symbols include/lrcn_act_dropout.h declares (bound by lib() as well)
ACT_DROPOUT_SIGNATURES = {
    "lrcn_act_loss_grad_drop": (C.c_int, [C.c_void_p, P4, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.c_int,
                                          C.POINTER(ActDropout), C.c_void_p, C.POINTER(C.c_double)]),
}

# name -> (restype, argtypes); exactly the symbols include/lrcn_varlen.h declares (bound by lib() as well)
VARLEN_SIGNATURES = {
    "lrcn_loss_var": (C.c_int, [C.c_void_p, P9, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int64, C.POINTER(Dropout),
                                C.POINTER(C.c_double)]),
    "lrcn_loss_grad_var": (C.c_int, [C.c_void_p, P9, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int64,
                                     C.POINTER(Dropout), P9, C.POINTER(C.c_double)]),
    "lrcn_train_step_var": (C.c_int, [C.c_void_p, P9, P9, P9, P9, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int64,
                                      C.POINTER(Dropout), C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.POINTER(C.c_double)]),
}

# name -> (restype, argtypes); exactly the symbols include/lrcn_weighted.h declares (bound by lib() as well)
WEIGHTED_SIGNATURES = {
    "lrcn_loss_w": (C.c_int, [C.c_void_p, P9, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int64,
                              C.POINTER(Dropout), C.POINTER(C.c_double)]),
    "lrcn_loss_grad_w": (C.c_int, [C.c_void_p, P9, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_int, C.c_int,
                                   C.c_int64, C.POINTER(Dropout), P9, C.POINTER(C.c_double)]),
    "lrcn_train_step_w": (C.c_int, [C.c_void_p, P9, P9, P9, P9, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_int,
                                    C.c_int, C.c_int64, C.POINTER(Dropout), C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                    C.POINTER(C.c_double)]),
}

# name -> (restype, argtypes); exactly the symbols include/lrcn_sched.h declares (bound by lib() as well)
SCHED_SIGNATURES = {
    "lrcn_loss_sched": (C.c_int, [C.c_void_p, P9, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int64,
                                  C.POINTER(Dropout), C.POINTER(Sched), C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]),
    "lrcn_loss_grad_sched": (C.c_int, [C.c_void_p, P9, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_int, C.c_int,
                                       C.c_int64, C.POINTER(Dropout), C.POINTER(Sched), P9, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]),
    "lrcn_train_step_sched": (C.c_int, [C.c_void_p, P9, P9, P9, P9, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_int,
                                        C.c_int, C.c_int64, C.POINTER(Dropout), C.POINTER(Sched), C.c_int, C.c_float, C.c_float, C.c_float,
                                        C.c_float, C.c_float, C.POINTER(C.c_double)]),
    "lrcn_sched_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
}

# name -> (restype, argtypes); exactly the symbols include/lrcn_smooth.h declares (bound by lib() as well)
SMOOTH_SIGNATURES = {
    "lrcn_loss_smooth": (C.c_int, [C.c_void_p, P9, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int64,
                                   C.POINTER(Dropout), C.POINTER(Sched), C.c_void_p, C.c_float, C.POINTER(C.c_double)]),
    "lrcn_loss_grad_smooth": (C.c_int, [C.c_void_p, P9, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_int, C.c_int,
                                        C.c_int64, C.POINTER(Dropout), C.POINTER(Sched), C.c_void_p, C.c_float, P9, C.POINTER(C.c_double)]),
    "lrcn_train_step_smooth": (C.c_int, [C.c_void_p, P9, P9, P9, P9, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_int,
                                         C.c_int, C.c_int64, C.POINTER(Dropout), C.POINTER(Sched), C.c_float, C.c_int, C.c_float, C.c_float,
                                         C.c_float, C.c_float, C.c_float, C.POINTER(C.c_double)]),
    "lrcn_smooth_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "lrcn_xent_logits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                   C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
}



class ClipStats(C.Structure):
    """lrcn_clip_stats_t (include/lrcn_clip.h)."""
    _fields_ = [("last_norm", C.c_double), ("last_scale", C.c_float), ("last_skipped", C.c_int32), ("steps", C.c_int64),
                ("clipped", C.c_int64), ("skipped", C.c_int64)]


# name -> (restype, argtypes); exactly the symbols include/lrcn_clip.h declares (bound by lib() as well)
CLIP_SIGNATURES = {
    "lrcn_grad_sumsq": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    "lrcn_grad_sumsq_model": (C.c_int, [C.c_void_p, P9, C.c_int, C.c_void_p]),
    "lrcn_clip_slots": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "lrcn_clip_set": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_void_p]),
    "lrcn_adam_update_clipped": (C.c_int, [C.c_void_p, P9, P9, P9, P9, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float]),
    "lrcn_adam_update_group_clipped": (C.c_int, [C.c_void_p, P9, P9, P9, P9, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float,
                                                 C.c_void_p]),
    "lrcn_adam_update_flat_clipped": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_float,
                                                C.c_float, C.c_float, C.c_float, C.c_void_p]),
    "lrcn_train_step_clip": (C.c_int, [C.c_void_p, P9, P9, P9, P9, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Dropout),
                                       C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.POINTER(C.c_double)]),
    "lrcn_train_step_var_clip": (C.c_int, [C.c_void_p, P9, P9, P9, P9, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_int,
                                           C.c_int64, C.POINTER(Dropout), C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                           C.POINTER(C.c_double)]),
    "lrcn_clip_stats": (C.c_int, [C.c_void_p, C.POINTER(ClipStats)]),
}

# name -> (restype, argtypes); exactly the symbols include/lrcn_gemm_debug.h declares (bound by lib() as well)
GEMM_DEBUG_SIGNATURES = {
    "lrcn_debug_gemm": (C.c_int, [C.c_void_p, C.POINTER(GemmDebug)]),
    "lrcn_debug_conv_gemm": (C.c_int, [C.c_void_p, C.POINTER(ConvGemmDebug)]),
}

# name -> (restype, argtypes); exactly the symbols include/lrcn_conv_debug.h declares (bound by lib() as well)
CONV_DEBUG_SIGNATURES = {
    "lrcn_debug_conv11": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.c_void_p]),
    "lrcn_debug_fp8_cast": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_float, C.c_void_p]),
    "lrcn_debug_amax": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "lrcn_debug_conv64_f8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p]),
    "lrcn_debug_conv64": (C.c_int, [C.c_void_p, C.POINTER(Conv64Debug)]),
    "lrcn_debug_fp8_scales": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
}

# name -> (restype, argtypes); exactly the symbols include/lrcn_decode_debug.h declares (bound by lib() as well)
DECODE_DEBUG_SIGNATURES = {
    "lrcn_debug_decode_steps": (C.c_int, [C.c_void_p, C.POINTER(DecodeDebug)]),
}

class CiderStats(C.Structure):   # lrcn_cider_stats_t of include/lrcn_cider.h
    _fields_ = [("images", C.c_int64), ("references", C.c_int64), ("ngrams", C.c_int64 * 4), ("slots", C.c_int64 * 4),
                ("ref_entries", C.c_int64 * 4), ("device_bytes", C.c_int64)]


# name -> (restype, argtypes); exactly the symbols include/lrcn_cider.h declares (bound by lib() as well)
CIDER_SIGNATURES = {
    "lrcn_cider_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int,
                                    C.POINTER(C.c_void_p)]),
    "lrcn_cider_destroy": (None, [C.c_void_p]),
    "lrcn_cider_last_error": (C.c_char_p, [C.c_void_p]),
    "lrcn_cider_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lrcn_cider_stats": (C.c_int, [C.c_void_p, C.POINTER(CiderStats)]),
    "lrcn_cider_score": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int,
                                   C.POINTER(C.c_double)]),
    "lrcn_cider_score_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
}


def build(force=False):
    """hipcc --offload-arch=gfx950 -> csrc/liblrcn_hip.so (cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))] + [HEADER, SAMPLE_HEADER, NUCLEUS_HEADER, SCORE_HEADER, NBEST_HEADER, DIVERSE_HEADER, CONSTRAIN_HEADER, ENSEMBLE_HEADER, FORCED_HEADER,
                                                                                                   ACTIVITY_HEADER, ACT_DROPOUT_HEADER, VARLEN_HEADER, CLIP_HEADER, WEIGHTED_HEADER, SCHED_HEADER, SMOOTH_HEADER, GEMM_DEBUG_HEADER, CONV_DEBUG_HEADER, DECODE_DEBUG_HEADER, CIDER_HEADER]
    stale = force or not os.path.exists(LIB_PATH) or os.path.getmtime(LIB_PATH) < max(os.path.getmtime(s) for s in srcs)
    if stale:
        subprocess.check_call(["make", "-s", "-j4", "-C", CSRC, "-f", os.path.join(CSRC, "Makefile")])
    return LIB_PATH


_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise LrcnError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                            "(there is no CPU fallback)" % LIB_PATH)
        # torch ships its own libamdhip64; device pointers and streams are shared with it, so its HIP runtime must be
        # the one this process uses: import torch BEFORE the library so the dynamic linker binds to that instance.
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in list(SIGNATURES.items()) + list(SAMPLE_SIGNATURES.items()) + list(NUCLEUS_SIGNATURES.items()) + list(SCORE_SIGNATURES.items()) + list(NBEST_SIGNATURES.items()) + list(DIVERSE_SIGNATURES.items()) + list(CONSTRAIN_SIGNATURES.items()) + list(ENSEMBLE_SIGNATURES.items()) + list(FORCED_SIGNATURES.items()) + \
                list(ACTIVITY_SIGNATURES.items()) + list(ACT_DROPOUT_SIGNATURES.items()) + list(VARLEN_SIGNATURES.items()) + list(CLIP_SIGNATURES.items()) + list(WEIGHTED_SIGNATURES.items()) + list(SCHED_SIGNATURES.items()) + list(SMOOTH_SIGNATURES.items()) + \
                list(GEMM_DEBUG_SIGNATURES.items()) + list(CONV_DEBUG_SIGNATURES.items()) + list(DECODE_DEBUG_SIGNATURES.items()) + list(CIDER_SIGNATURES.items()):
            fn = getattr(L, name)  # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        if L.lrcn_abi_version() != LRCN_ABI_VERSION:
            raise LrcnError("%s implements ABI revision %d, this binding was written against %d (lrcn_config's layout differs)"
                            % (LIB_PATH, L.lrcn_abi_version(), LRCN_ABI_VERSION))
        _LIB = L
    return _LIB


def check(ctx_handle, rc):
    if rc != 0:
        msg = lib().lrcn_last_error(ctx_handle)
        raise LrcnError("liblrcn_hip error %d: %s" % (rc, msg.decode() if msg else "?"))
