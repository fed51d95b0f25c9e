"""ctypes binding of ``csrc/libgim_hip.so`` (the C ABI declared in ``include/gim_hip.h``).

The product path has NO fallback: if the library is missing or a tensor is not a CUDA(HIP) fp32
tensor the call raises.  Build the library with ``python -c "import __graft_entry__ as g; g.build()"``
(or ``make -C optimalstrategiesagainstgenerativeattacks_amd/csrc``).
"""
import ctypes
import os
from ctypes import POINTER, c_float, c_int, c_int32, c_int64, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GIM_LIB_PATH") or os.path.join(_HERE, "csrc", "libgim_hip.so")  # override: timing experiments


class GimConvShape(ctypes.Structure):
    _fields_ = [("N", c_int32), ("H", c_int32), ("W", c_int32), ("Cin", c_int32), ("Cout", c_int32),
                ("KH", c_int32), ("ups", c_int32), ("pre_slope", c_float),
                ("pool", c_int32), ("wfold", c_int32), ("res_ups", c_int32),
                ("tune_tile", c_int32), ("tune_ksplit", c_int32), ("tune_wgrad", c_int32),
                ("out_zeroed", c_int32), ("post_slope", c_float), ("prec", c_int32)]


class GimInferConv(ctypes.Structure):
    _fields_ = [("N", c_int32), ("H", c_int32), ("W", c_int32), ("Cin", c_int32), ("Cout", c_int32),
                ("KH", c_int32), ("stride", c_int32)]


P = c_void_p
SP = POINTER(GimConvShape)


# Rows of the job tables that the grouped launches read from device memory (ops.layout_tables).  Every `typedef struct` of
# include/gim_hip.h has its mirror here under the same name in camel case (gim_sn_job -> GimSnJob); tests/test_host.py compares them.
class GimFoldJob(ctypes.Structure):
    _fields_ = [("w", P), ("f", P), ("Cout", c_int32), ("Cin", c_int32), ("KH", c_int32), ("reserved", c_int32)]


class GimSnJob(ctypes.Structure):
    _fields_ = [("w", P), ("u", P), ("v", P), ("off_sigma", c_int64), ("off_u", c_int64), ("off_v", c_int64), ("off_scratch", c_int64),
                ("Cout", c_int32), ("Cin", c_int32), ("KH", c_int32), ("reserved", c_int32)]


class GimWgradJob(ctypes.Structure):
    _fields_ = [("src", P), ("bias_src", P), ("w", P), ("sigma", P), ("u", P), ("v", P), ("tmp", P), ("partial", P),
                ("grad_w", P), ("grad_b", P), ("Cout", c_int32), ("Cin", c_int32), ("K", c_int32), ("fold", c_int32),
                ("n_chunks", c_int32), ("exclusive", c_int32)]


class GimGemmJob(ctypes.Structure):
    _fields_ = [("A", P), ("B", P), ("C", P), ("bias", P), ("M", c_int32), ("N", c_int32), ("K", c_int32), ("ldc", c_int32),
                ("sAi", c_int64), ("sAk", c_int64), ("sBk", c_int64), ("sBj", c_int64), ("flags", c_int32), ("reserved", c_int32)]


# name -> argtypes (all return int unless noted); this table is also what tests check against the header
SIGNATURES = {
    "gim_conv2d_fwd": [P, P, P, P, P, P, SP, P],
    "gim_conv2d_dgrad": [P, P, P, P, P, SP, P],
    "gim_conv2d_dgrad_res": [P, P, P, P, P, c_float, P, SP, P],
    "gim_conv2d_wgrad_slabs": [SP],
    "gim_conv2d_wgrad": [P, P, P, P, c_int, SP, P],
    "gim_wgrad_finish": [P, P, c_int, P, P, P, P, P, P, P, c_int, c_int, c_int, c_int, P, P, P],
    "gim_conv2d_fold_weights": [P, P, c_int, c_int, c_int, P],
    "gim_conv2d_fold_weights_batched": [P, P, c_int, P],
    "gim_spectral_sigma": [P, P, P, P, P, P, P, c_int, c_int, c_int, c_int, P],
    "gim_spectral_sigma_batched": [P, c_int, P, c_int, P, c_int, P, c_int, P],
    "gim_colsum": [P, P, P, c_int64, c_int, P],
    "gim_norm_fwd": [P, P, P, P, P, P, c_int, c_int, c_int, c_int, c_float, P],
    "gim_norm_fwd_act": [P, P, P, P, P, P, c_int, c_int, c_int, c_int, c_float, c_float, P],
    "gim_norm_bwd": [P, P, P, P, P, P, P, c_int, c_int, c_int, c_int, P],
    "gim_avgpool2_fwd": [P, P, c_int, c_int, c_int, c_int, P],
    "gim_avgpool2_fwd_act": [P, P, c_int, c_int, c_int, c_int, c_float, P],
    "gim_box2_fwd": [P, P, c_int, c_int, c_int, c_int, c_float, P],
    "gim_add_n": [P, P, P, P, P, c_int64, P],
    "gim_add_avgpool2_bwd": [P, P, P, c_int, c_int, c_int, c_int, P],
    "gim_avgpool2_bwd": [P, P, c_int, c_int, c_int, c_int, P],
    "gim_upsample2x_bwd": [P, P, c_float, P, c_int, c_int, c_int, c_int, P],
    "gim_maxpool_lrelu_fwd": [P, P, P, c_int, c_int, c_int, c_float, P],
    "gim_maxpool_lrelu_bwd": [P, P, P, P, c_int, c_int, c_int, c_float, P],
    "gim_bgemm": [P, P, P, c_int, c_int, c_int, c_int, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, P],
    "gim_attn_prob_fwd": [P, P, P, c_int, c_int, c_int, P],
    "gim_softmax_dim1_fwd": [P, P, c_int, c_int, c_int, P],
    "gim_softmax_dim1_bwd": [P, P, P, c_int, c_int, c_int, P],
    "gim_bgemm_grouped": [P, P, c_int, P],
    "gim_colsum_grouped": [P, P, c_int, P],
    "gim_scale_add_fwd": [P, P, P, P, c_int64, P],
    "gim_scale_add_fwd_act": [P, P, P, P, c_int64, c_float, P],
    "gim_scale_add_bwd": [P, P, P, P, P, P, c_int64, P],
    "gim_tanh_fwd": [P, P, c_int64, P],
    "gim_tanh_bwd": [P, P, P, c_int64, P],
    "gim_nchw_to_nhwc": [P, P, c_int, c_int, c_int, P],
    "gim_nhwc_to_nchw": [P, P, c_int, c_int, c_int, P],
    "gim_set_stats_fwd": [P, P, P, c_int, c_int, c_int, c_int64, c_int64, P],
    "gim_set_stats_bwd": [P, P, P, P, c_int, c_int, c_int, c_int64, c_int64, P],
    "gim_bce_logits_fwd": [P, P, c_float, c_int, P],
    "gim_bce_logits_bwd": [P, P, P, c_float, c_int, P],
    "gim_sum_dim1": [P, P, c_int, c_int, c_int, c_float, P],
    "gim_repeat_dim1": [P, P, c_int, c_int, c_int, c_float, P],
    "gim_noise_combine": [P, P, P, c_int, c_int, c_int, c_int, P],
    "gim_concat2": [P, P, P, c_int64, c_int, c_int, c_int, c_int, P],
    "gim_slice_channels": [P, P, c_int64, c_int, c_int, P],
    "gim_conv2d_wgrad_acc": [P, P, P, P, SP, P],
    "gim_wgrad_finish_batched": [P, c_int, P, c_int, P, c_int, P],
    "gim_colsum_acc": [P, P, P, c_int64, c_int, P],
    "gim_colsum2": [P, P, P, P, c_int, c_int, c_int, P],
    "gim_conv_launch_plan": [SP, c_int, P],
    "gim_conv2d_transpose_weights": [P, P, c_int, c_int, c_int, P],
    "gim_conv2d_dgrad_t": [P, P, P, P, P, SP, P],
    "gim_conv2d_xfold_weights": [P, P, c_int, c_int, c_int, c_int, P],
    "gim_conv2d_dgrad_xfold": [P, P, P, P, P, SP, c_int, P],
    "gim_episode_gather": [P, P, P, P, c_int, c_int, c_int, c_int, P],
    "gim_resize_bilinear_u8": [P, c_int64, c_int, c_int, c_int, c_int, P, c_int, c_int, P, P, c_int, P, P, c_int, P],
    "gim_maxpool_gather": [P, P, P, P, c_int, c_int, c_int, c_float, P],
    "gim_softmax_dim1_bwd_dp": [P, P, P, P, c_int, c_int, c_int, P],
    "gim_set_stats_bwd_bwd": [P, P, P, P, P, P, c_int, c_int, c_int, c_int64, c_int64, P],
    "gim_lrelu_mask_mul": [P, P, c_float, P, c_int64, P],
    "gim_sqsum_rows_fwd": [P, P, c_int, c_int64, P],
    "gim_sqsum_rows_bwd": [P, P, P, c_int, c_int64, P],
    "gim_img_att_mix_fwd": [P, P, P, P, P, P, P, P, c_int64, c_int, P],
    "gim_img_att_mix_bwd": [P, P, P, P, P, P, P, P, P, P, P, P, P, P, c_int64, c_int, P],
    "gim_adam_step": [P, P, P, P, c_int64, P, P, c_int, c_float, c_float, c_float, c_float, P, P],
    "gim_adam_step_scaled": [P, P, P, P, c_int64, P, P, c_int, c_float, c_float, c_float, c_float, P, P, P],
    "gim_ema_update": [P, P, c_int64, c_float, P, P],
    "gim_buffer_exchange": [P, P, c_int64, P],
    "gim_adam_optimism": [P, P, P, P, c_int64, P, P, c_int, c_float, c_float, c_float, c_float, P, P, P],
    "gim_spin": [c_int, P],
    "gim_pad_image": [P, P, c_int, c_int, c_int, c_int, c_int, c_float, P],
    "gim_conv2d_pack_rows_weights": [P, P, c_int, c_int, c_int, P],
    "gim_conv2d_pack_subpixel_weights": [P, P, c_int, c_int, c_int, P],
    "gim_depth_to_space2": [P, P, P, c_int, c_int, c_int, c_int, c_float, P],
    "gim_conv2d_fwd_rows": [P, P, P, P, P, P, SP, P],
    "gim_conv2d_wgrad_rows_acc": [P, P, P, P, SP, P],
    "gim_conv2d_infer": [P, P, P, P, P, POINTER(GimInferConv), P],
    "gim_maxpool2_act": [P, P, c_int, c_int, c_int, c_int, c_int, P],
    "gim_channel_affine": [P, P, P, P, c_int64, c_int, P],
    "gim_se_tail": [P, P, P, P, P, P, P, c_int, c_int, c_int, c_int, c_int, P],
    "gim_pair_score": [P, P, P, c_int, c_int, P],
    "gim_l2norm_rows": [P, P, c_int, c_int, P],
    "gim_absdiff": [P, P, P, c_int64, P],
    "gim_bn_slabs": [c_int64],
    "gim_bn_partials_floats": [c_int64, c_int],
    "gim_bn_stats": [P, P, P, P, P, P, P, c_int64, c_int, c_float, c_float, P],
    "gim_bn_relu_maxpool2_fwd": [P, P, P, P, P, P, c_int, c_int, c_int, c_int, P],
    "gim_bn_pool_bwd_reduce": [P, P, P, P, P, P, P, P, P, P, P, c_int, c_int, c_int, c_int, P],
    "gim_bn_pool_bwd_dx": [P, P, P, P, P, P, P, P, P, c_int, c_int, c_int, c_int, P],
    "gim_bn_stats_record": [P, P, P, c_int64, c_int, P],
    "gim_bn_stats_merge": [P, POINTER(c_int64), c_int, c_int, P, P, P, P, P, c_float, c_float, P],
    "gim_bn_pool_bwd_dx_total": [P, P, P, P, P, P, P, P, P, c_int, c_int, c_int, c_int, c_int64, P],
    "gim_absdiff_bwd": [P, P, P, P, P, c_int64, P],
    "gim_logit_accuracy": [P, c_int, c_int, P, P],
    "gim_bn_apply_fwd": [P, P, P, P, P, P, P, c_int64, c_int, P],
    "gim_bn_bwd_reduce": [P, P, P, P, P, P, P, P, P, P, P, P, P, P, c_int64, c_int, P],
    "gim_bn_bwd_dx": [P, P, P, P, P, P, P, P, P, P, c_int64, c_int, P],
    "gim_bn_bwd_dx_total": [P, P, P, P, P, P, P, P, P, P, c_int64, c_int64, c_int, P],
    "gim_prelu_fwd": [P, P, P, c_int64, c_int, P],
    "gim_prelu_bwd": [P, P, P, P, P, P, P, c_int64, c_int, P],
    "gim_se_tail_bwd": [P, P, P, P, P, c_int, c_int, c_int, c_int, P],
    "gim_subsample2_fwd": [P, P, c_int, c_int, c_int, c_int, P],
    "gim_subsample2_bwd": [P, P, c_int, c_int, c_int, c_int, P],
    "gim_dropout": [P, P, c_int64, c_float, c_uint64, c_uint64, P],
    "gim_l2norm_rows_bwd": [P, P, P, c_int, c_int, P],
    "gim_col_l2norm_fwd": [P, P, c_int, c_int, P],
    "gim_col_l2norm_bwd": [P, P, P, c_int, c_int, P],
    "gim_arcface_margin_fwd": [P, P, P, c_int, c_int, c_float, c_float, c_float, c_float, c_float, P],
    "gim_arcface_margin_bwd": [P, P, P, P, c_int, c_int, c_float, c_float, c_float, c_float, c_float, P],
    "gim_softmax_ce_fwd": [P, P, P, P, P, c_int, c_int, P],
    "gim_softmax_ce_bwd": [P, P, P, P, P, c_int, c_int, P],
    "gim_conv2d_strided_fwd": [P, P, P, P, POINTER(GimInferConv), P],
    "gim_conv2d_strided_dgrad": [P, P, P, POINTER(GimInferConv), c_int, P],
    "gim_conv2d_strided_wgrad_workspace": [POINTER(GimInferConv), POINTER(c_int64)],
    "gim_conv2d_strided_wgrad": [P, P, P, P, POINTER(GimInferConv), c_int, P, P],
    "gim_conv2d_strided_plan": [POINTER(GimInferConv), c_int, P],
    "gim_roc_slices": [c_int64, c_int64],
    "gim_roc_counts": [P, c_int, P, c_int, P, c_int, P, P],
    "gim_roc_calibrate": [P, c_int, P, c_int, P, P, P],
    "gim_version": [],
}

_lib = None


def load():
    """Load (once) and return the ctypes library; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libgim_hip.so not found at %s: the HIP extension is not built "
            "(run __graft_entry__.build()); there is no CPU fallback" % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = c_int
    lib.gim_last_error.argtypes = []
    lib.gim_last_error.restype = ctypes.c_char_p
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().gim_last_error()
        raise RuntimeError("libgim_hip %s failed (%d): %s" % (what, rc, msg.decode() if msg else "?"))
