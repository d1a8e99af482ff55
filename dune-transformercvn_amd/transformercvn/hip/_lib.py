"""ctypes binding of libtcvn_hip.so (the C ABI declared in include/tcvn_hip.h).

The library is built in-tree by ``make -C dune-transformercvn_amd/csrc`` (or ``__graft_entry__.build()``).  There is no
CPU fallback: if the shared object is missing or fails to load, importing this module raises.
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  -- first: the library must bind to the HIP runtime PyTorch ships (one runtime per process); loading
#                              /opt/rocm's copy ahead of torch's leaves this library without a device ("no ROCm-capable device")

from . import _libselect

_HERE = os.path.dirname(os.path.abspath(__file__))
# libtcvn_hip.so unless a test child process selected the debug build explicitly (_libselect.use) before this import; no
# environment variable is read here or in the product library.
LIB_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "lib", _libselect.NAME))
_libselect._bound = True

MODE_F32, MODE_BF16 = 0, 1
SLOT_PARAM, SLOT_BUFFER, SLOT_COUNTER = 0, 1, 2
FUSE_MEAN, FUSE_MAX = 0, 1          # TCVN_FUSE_*: head fusion of the attention rollout
LOO_MAX_PASS = 256                  # TCVN_LOO_MAX_PASS: sequences per encoder pass of the leave-one-prong-out scan
SHAP_MAX_PASS = 1024                # TCVN_SHAP_MAX_PASS: sequences per encoder pass of the prong Shapley scan
SHAP_MAX_EXACT = 16                 # TCVN_SHAP_MAX_EXACT: the widest event whose 2^n coalitions are all run
SHAP_VALUE_PROB, SHAP_VALUE_LOGIT = 0, 1       # TCVN_SHAP_VALUE_*: what a coalition is worth, class probability or raw logit
OCC_MAX_PASS = 256                  # TCVN_OCC_MAX_PASS: maps per embedder / token-path pass of the occlusion scan
OCC_TARGET_EVENT, OCC_TARGET_PRONG = 0, 1      # TCVN_OCC_TARGET_*: which logits the occlusion heat map is taken from
OCC_GROUP_EVENT, OCC_GROUP_MAP = 0, 1          # TCVN_OCC_GROUP_*: whose largest score a refinement level's variants are held against
OCC_MAX_LEVELS = 16                 # TCVN_OCC_MAX_LEVELS: levels of one coarse-to-fine occlusion scan
CURVE_MAX_STEPS, CURVE_MAX_TILES = 64, 4096    # TCVN_CURVE_MAX_*: steps of a deletion / insertion curve, tiles per map it can rank
CURVE_DELETION, CURVE_INSERTION = 0, 1         # TCVN_CURVE_*: which hits a curve variant keeps
TSHAP_MAX_TILES, TSHAP_MAX_SAMPLES, TSHAP_MAX_EXACT = 1024, 256, 10    # TCVN_TSHAP_MAX_*: limits of the tile Shapley scan
DET_MAX_EFFECTS = 64                # TCVN_DET_MAX_EFFECTS: settings of one detector-effect scan
DET_SCOPE_EVENT, DET_SCOPE_MAP = 0, 1          # TCVN_DET_SCOPE_*: an effect hits every map of an event, or one map at a time
MC_MAX_CLASSES = 256                # TCVN_MC_MAX_CLASSES: the widest logit row tcvn_mc_dropout_stats takes
SCONV_KERNELS = ("generic", "c64", "g", "s2", "in")    # TCVN_SCONV_*: kernel families of the SDXL embedder's convolutions
# TCVN_SDXL_OP_*: the fields of tcvn_sdxl_op, in order;  TCVN_SDXL_REGION_*: what tcvn_sdxl_region locates
SDXL_OP_FIELDS = ("kind", "in", "out", "res", "w", "ks", "stride", "pad", "act", "conv_id", "gn_id", "stats_gn", "stats_given", "final_f32")
SDXL_REGIONS = ("act", "grad", "wk", "wkt", "gwk", "stats", "bstats")


class DenseNetCfg(C.Structure):
    _fields_ = [("in_ch", C.c_int), ("out_dim", C.c_int), ("init_ch", C.c_int), ("growth", C.c_int), ("bn_size", C.c_int),
                ("n_blocks", C.c_int), ("layers", C.c_int * 8), ("H", C.c_int), ("W", C.c_int), ("dropout", C.c_float),
                ("mode", C.c_int)]


class SdxlCfg(C.Structure):
    _fields_ = [("in_ch", C.c_int), ("out_dim", C.c_int), ("init_ch", C.c_int), ("repeat", C.c_int), ("num_blocks", C.c_int),
                ("H", C.c_int), ("W", C.c_int), ("mode", C.c_int)]


class HeadCfg(C.Structure):
    _fields_ = [("hidden_dim", C.c_int), ("heads", C.c_int), ("n_layers", C.c_int), ("in_dim", C.c_int),
                ("event_classes", C.c_int), ("prong_classes", C.c_int), ("n_dec", C.c_int), ("dec_dims", C.c_int * 8),
                ("dec_out_in", C.c_int), ("gelu", C.c_int), ("norm_first", C.c_int), ("dropout_modules", C.c_int),
                ("dropout", C.c_float), ("gamma", C.c_float), ("event_weight", C.c_float),
                ("no_linear_bn", C.c_int), ("linear_relu", C.c_int)]


class DetectorEffectC(C.Structure):
    """struct tcvn_detector_effect"""
    _fields_ = [("scale", C.c_float), ("threshold", C.c_float), ("drop", C.c_float), ("dead_y0", C.c_int32), ("dead_y1", C.c_int32),
                ("dead_x0", C.c_int32), ("dead_x1", C.c_int32), ("shift_y", C.c_int32), ("shift_x", C.c_int32), ("seed", C.c_uint64)]


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"libtcvn_hip.so not found at {LIB_PATH}: build it with `make -C dune-transformercvn_amd/csrc -j8` "
            "(hipcc, --offload-arch=gfx950). There is no CPU fallback for the TransformerCVN hot path.")
    lib = C.CDLL(LIB_PATH)
    vp, i32, i64, u64, f32 = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_float
    P = C.POINTER

    def sig(name, res, *args):
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = list(args)
        return fn

    sig("tcvn_version", i32)
    sig("tcvn_densenet_create", i32, P(DenseNetCfg), P(vp))
    sig("tcvn_densenet_destroy", None, vp)
    sig("tcvn_densenet_num_slots", i32, vp)
    sig("tcvn_densenet_slot", i32, vp, i32, C.c_char_p, i32, P(i64), P(i32))
    sig("tcvn_densenet_bind", i32, vp, P(vp), P(vp))
    sig("tcvn_densenet_workspace_bytes", i64, vp, i32, i32)
    sig("tcvn_densenet_forward", i32, vp, i32, vp, vp, i64, i32, f32, vp, i64, vp, i64, i32, u64, vp)
    sig("tcvn_densenet_backward", i32, vp, i32, vp, i64, vp, i64, vp)
    sig("tcvn_densenet_num_blocks", i32, vp)
    sig("tcvn_densenet_backward_blocks", i32, vp, i32, vp, i64, vp, i64, i32, i32, vp)
    sig("tcvn_densenet_tap", i32, vp, i32, C.c_char_p, P(i64), P(i32), P(i32), P(i32), P(i32), P(i32), P(i32))
    sig("tcvn_sdxl_create", i32, P(SdxlCfg), P(vp))
    sig("tcvn_sdxl_destroy", None, vp)
    sig("tcvn_sdxl_num_slots", i32, vp)
    sig("tcvn_sdxl_slot", i32, vp, i32, C.c_char_p, i32, P(i64), P(i32))
    sig("tcvn_sdxl_bind", i32, vp, P(vp), P(vp))
    sig("tcvn_sdxl_workspace_bytes", i64, vp, i32, i32)
    sig("tcvn_sdxl_forward", i32, vp, i32, vp, vp, i64, i32, f32, vp, i64, vp, i64, i32, u64, vp)
    sig("tcvn_sdxl_backward", i32, vp, i32, vp, i64, vp, i64, vp)
    sig("tcvn_sdxl_tap", i32, vp, i32, C.c_char_p, P(i64), P(i32), P(i32), P(i32), P(i32), P(i32), P(i32))
    sig("tcvn_sdxl_num_convs", i32, vp)
    sig("tcvn_sdxl_conv_kernels", i32, vp, i32, i32, P(i32), P(i32), P(i32))
    sig("tcvn_sdxl_num_ops", i32, vp)
    sig("tcvn_sdxl_op", i32, vp, i32, P(i32), i32)
    sig("tcvn_sdxl_region", i32, vp, i32, i32, i32, i32, P(i64), P(i64), P(i32), P(i32))
    sig("tcvn_head_create", i32, P(HeadCfg), P(vp))
    sig("tcvn_head_destroy", None, vp)
    sig("tcvn_head_num_slots", i32, vp)
    sig("tcvn_head_slot", i32, vp, i32, C.c_char_p, i32, P(i64), P(i32))
    sig("tcvn_head_bind", i32, vp, P(vp), P(vp))
    sig("tcvn_head_workspace_bytes", i64, vp, i32, i32, i32)
    sig("tcvn_head_forward", i32, vp, i32, i32, i32, vp, vp, vp, vp, vp, i64, i32, u64, vp)
    sig("tcvn_head_loss", i32, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp)
    sig("tcvn_head_backward", i32, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, i64, vp)
    sig("tcvn_head_set_fused_encoder", None, vp, i32)
    sig("tcvn_head_embed", i32, vp, i32, i32, i32, vp, vp, vp, vp, i64, i32, u64, vp)
    sig("tcvn_head_encode", i32, vp, i32, i32, vp, vp, vp, vp, i64, i32, u64, vp)
    sig("tcvn_head_decode", i32, vp, i32, i32, vp, vp, vp, vp, i64, i32, u64, vp)
    sig("tcvn_head_attention", i32, vp, i32, i32, vp, vp, i64, vp, vp)
    sig("tcvn_attention_rollout", i32, vp, vp, i32, i32, i32, i32, i32, vp, vp)
    sig("tcvn_head_leave_one_out_workspace_bytes", i64, vp, i32, i32)
    sig("tcvn_head_leave_one_out", i32, vp, i32, i32, vp, vp, vp, vp, vp, i64, vp)
    sig("tcvn_head_shapley_workspace_bytes", i64, vp, i32, i32, i32, i32)
    sig("tcvn_head_shapley_count", i64, i32, i32, vp, i32, i32, vp)
    sig("tcvn_head_shapley", i32, vp, i32, i32, vp, vp, i32, i32, u64, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp, vp, i64, vp)
    sig("tcvn_occlusion_workspace_bytes", i64, i32, i32, i32, i32, i32, i32)
    sig("tcvn_occlusion_variants", i32, vp, i64, i32, i32, i32, i32, i32, vp, i32, vp, vp, vp, i64, P(i64), i64, vp)
    sig("tcvn_occlusion_build_pass", i32, vp, vp, i64, i32, i32, i32, i32, i32, i32, i32, vp, vp, i64, i32, i32, vp, vp, i64, vp)
    sig("tcvn_head_occlusion_workspace_bytes", i64, vp, i32)
    sig("tcvn_head_occlusion", i32, vp, i32, i32, i32, vp, vp, vp, i32, vp, vp, i32, vp, i64, i32, i32, vp, vp, vp, i64, vp)
    sig("tcvn_occlusion_heatmap", i32, vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp)
    sig("tcvn_occlusion_select", i32, vp, vp, i64, i32, i32, i32, i32, i32, f32, vp, vp, vp)
    sig("tcvn_occlusion_refine_variants", i32, vp, i64, i32, i32, i32, i32, i32, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, i64, P(i64),
        i64, vp)
    sig("tcvn_occlusion_mark", i32, vp, i64, i32, i32, i32, i32, vp, vp)
    sig("tcvn_occlusion_occupancy", i32, vp, i64, i32, i32, i32, i32, i32, vp, i32, i32, vp, vp)
    sig("tcvn_occlusion_paint", i32, i32, P(vp), P(vp), P(i32), P(i32), vp, i32, i32, vp, vp)
    sig("tcvn_occlusion_curve_workspace_bytes", i64, i32, i32, i32, i32, i32, i32, i32)
    sig("tcvn_occlusion_curve_variants", i32, vp, i64, i32, i32, i32, i32, i32, vp, vp, i32, i32, i32, i32, vp, i32, vp, vp, vp, i64, P(i64),
        i64, vp)
    sig("tcvn_occlusion_curve_build_pass", i32, vp, vp, i64, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, i64, i32, i32, vp, vp, i64,
        vp)
    sig("tcvn_occlusion_curve", i32, vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp)
    sig("tcvn_occlusion_shapley_workspace_bytes", i64, i32, i32, i32, i32, i32, i32, i32, i32)
    sig("tcvn_occlusion_shapley_variants", i32, vp, i64, i32, i32, i32, i32, i32, vp, i32, i32, i32, i32, u64, vp, vp, vp, i32, vp, vp, vp,
        i64, P(i64), i64, vp)
    sig("tcvn_occlusion_shapley_build", i32, vp, vp, i64, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, i64, i32, i32, vp, vp, i64,
        vp)
    sig("tcvn_occlusion_shapley_values", i32, vp, vp, vp, vp, vp, i64, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, i32, vp, vp,
        vp, vp, vp, i64, vp)
    sig("tcvn_detector_workspace_bytes", i64, i32, i32, i32)
    sig("tcvn_detector_variants", i32, vp, i64, i32, i32, i32, i32, vp, vp, P(DetectorEffectC), i32, i32, vp, vp, vp, i64, P(i64), i64, vp)
    sig("tcvn_detector_build_pass", i32, vp, vp, i64, i32, i32, i32, i32, vp, i32, i32, vp, vp, i64, i32, i32, vp, vp, i64, vp)
    sig("tcvn_detector_response", i32, vp, vp, vp, vp, vp, i64, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp)
    sig("tcvn_linear_forward", i32, vp, i64, vp, vp, vp, i64, i32, i32, i32, vp)
    sig("tcvn_rows_bn_prelu_forward", i32, vp, i64, i32, i32, vp, vp, vp, vp, vp, vp, i64, vp, i32, f32, u64, C.c_uint32, vp)
    sig("tcvn_densenet_forward_mc", i32, vp, i32, vp, vp, i64, i32, vp, i64, vp, i64, u64, i32, vp)
    sig("tcvn_head_forward_mc", i32, vp, i32, i32, i32, vp, vp, vp, vp, vp, i64, u64, vp)
    sig("tcvn_rows_bn_prelu_forward_mc", i32, vp, i64, i32, i32, vp, vp, vp, vp, vp, vp, i64, f32, u64, C.c_uint32, vp)
    sig("tcvn_mc_dropout_stats", i32, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp)
    sig("tcvn_densenet_forward_frozen", i32, vp, i32, vp, vp, i64, i32, vp, i64, vp, i64, vp)
    sig("tcvn_densenet_input_gradient", i32, vp, i32, vp, i64, vp, vp, i64, vp)
    sig("tcvn_head_forward_frozen", i32, vp, i32, i32, i32, vp, vp, vp, vp, vp, i64, vp)
    sig("tcvn_head_input_gradient", i32, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, i64, vp)
    sig("tcvn_hit_gradient_workspace_bytes", i64, i32, i32, i32, i32)
    sig("tcvn_hit_gradient_gather", i32, i32, vp, vp, i64, i32, i32, i32, i32, i32, vp, i64, i32, vp, vp, vp, i64, vp)
    sig("tcvn_hit_gradient_seed", i32, vp, vp, i32, i32, i32, vp, vp)
    sig("tcvn_ig_scale", i32, vp, f32, vp, i64, vp)
    sig("tcvn_ig_accumulate", i32, vp, vp, C.c_double, i64, vp)
    sig("tcvn_ig_finish", i32, vp, vp, vp, i64, vp)
    sig("tcvn_noise_workspace_bytes", i64, i32)
    sig("tcvn_noise_sigma", i32, vp, vp, i64, i32, i32, i32, i32, vp, i32, i32, C.c_double, vp, vp, i64, vp)
    sig("tcvn_noise_replicate", i32, vp, vp, i64, i32, i32, i32, i32, vp, i32, i32, vp, u64, i32, i32, vp, vp, vp)
    sig("tcvn_noise_accumulate", i32, vp, vp, vp, i64, i32, i32, vp)
    sig("tcvn_noise_finish", i32, vp, i64, i32, vp, vp)
    sig("tcvn_linear_backward", i32, vp, i64, vp, i64, vp, vp, i64, vp, vp, i32, i32, i32, vp)
    sig("tcvn_rows_bn_prelu_backward", i32, vp, i64, vp, i64, i32, i32, vp, vp, vp, vp, vp, i64, vp, vp, vp, f32, u64, C.c_uint32, vp)
    sig("tcvn_focal_loss", i32, vp, vp, i32, i32, f32, f32, vp, vp, vp)
    sig("tcvn_grad_sumsq", i32, vp, i64, vp, i32, vp, vp)
    sig("tcvn_adamw_step", i32, vp, vp, vp, vp, vp, i64, f32, f32, f32, f32, i64, vp, f32, vp)
    sig("tcvn_dropout_keep", i32, i32, f32, u64, C.c_uint32, i64, i32, vp, vp)
    sig("tcvn_backward_overlap", None, i32)
    sig("tcvn_profile_enable", None, i32)
    sig("tcvn_profile_filter", None, C.c_char_p)
    sig("tcvn_profile_reset", None)
    sig("tcvn_profile_count", i32)
    sig("tcvn_profile_get", i32, i32, C.c_char_p, i32, P(f32), P(C.c_double), P(C.c_double))
    return lib


def profile_records():
    """[(kernel name, ms, flops, bytes)] of the launches recorded since the last reset (blocks until they finished)."""
    out = []
    buf = C.create_string_buffer(128)
    ms, fl, by = C.c_float(), C.c_double(), C.c_double()
    for i in range(lib.tcvn_profile_count()):
        check(lib.tcvn_profile_get(i, buf, 128, C.byref(ms), C.byref(fl), C.byref(by)), "profile_get")
        out.append((buf.value.decode(), ms.value, fl.value, by.value))
    return out


EXPORTS = [
    "tcvn_grad_sumsq", "tcvn_adamw_step", "tcvn_backward_overlap", "tcvn_profile_enable", "tcvn_profile_filter", "tcvn_profile_reset", "tcvn_profile_count", "tcvn_profile_get",
    "tcvn_focal_loss", "tcvn_dropout_keep", "tcvn_head_set_fused_encoder", "tcvn_head_embed", "tcvn_head_encode", "tcvn_head_decode", "tcvn_linear_forward",
    "tcvn_rows_bn_prelu_forward", "tcvn_linear_backward", "tcvn_rows_bn_prelu_backward", "tcvn_sdxl_create", "tcvn_sdxl_destroy", "tcvn_sdxl_num_slots", "tcvn_sdxl_slot", "tcvn_sdxl_bind",
    "tcvn_sdxl_workspace_bytes", "tcvn_sdxl_forward", "tcvn_sdxl_backward", "tcvn_sdxl_tap", "tcvn_sdxl_num_convs", "tcvn_sdxl_conv_kernels",
    "tcvn_sdxl_num_ops", "tcvn_sdxl_op", "tcvn_sdxl_region",
    "tcvn_version", "tcvn_densenet_create", "tcvn_densenet_destroy", "tcvn_densenet_num_slots", "tcvn_densenet_slot",
    "tcvn_densenet_bind", "tcvn_densenet_workspace_bytes", "tcvn_densenet_forward", "tcvn_densenet_backward",
    "tcvn_densenet_tap", "tcvn_densenet_num_blocks", "tcvn_densenet_backward_blocks", "tcvn_head_create", "tcvn_head_destroy", "tcvn_head_num_slots", "tcvn_head_slot", "tcvn_head_bind",
    "tcvn_head_workspace_bytes", "tcvn_head_forward", "tcvn_head_loss", "tcvn_head_backward",
    "tcvn_head_attention", "tcvn_attention_rollout", "tcvn_head_leave_one_out_workspace_bytes", "tcvn_head_leave_one_out",
    "tcvn_occlusion_workspace_bytes", "tcvn_occlusion_variants", "tcvn_occlusion_build_pass", "tcvn_head_occlusion_workspace_bytes",
    "tcvn_head_occlusion", "tcvn_occlusion_heatmap",
    "tcvn_occlusion_select", "tcvn_occlusion_refine_variants", "tcvn_occlusion_mark", "tcvn_occlusion_occupancy", "tcvn_occlusion_paint",
    "tcvn_occlusion_curve_workspace_bytes", "tcvn_occlusion_curve_variants", "tcvn_occlusion_curve_build_pass", "tcvn_occlusion_curve",
    "tcvn_occlusion_shapley_workspace_bytes", "tcvn_occlusion_shapley_variants", "tcvn_occlusion_shapley_build",
    "tcvn_occlusion_shapley_values",
    "tcvn_head_shapley_workspace_bytes", "tcvn_head_shapley_count", "tcvn_head_shapley",
    "tcvn_densenet_forward_mc", "tcvn_head_forward_mc", "tcvn_rows_bn_prelu_forward_mc", "tcvn_mc_dropout_stats",
    "tcvn_detector_workspace_bytes", "tcvn_detector_variants", "tcvn_detector_build_pass", "tcvn_detector_response",
    "tcvn_densenet_forward_frozen", "tcvn_densenet_input_gradient", "tcvn_head_forward_frozen", "tcvn_head_input_gradient",
    "tcvn_hit_gradient_workspace_bytes", "tcvn_hit_gradient_gather", "tcvn_hit_gradient_seed",
    "tcvn_ig_scale", "tcvn_ig_accumulate", "tcvn_ig_finish",
    "tcvn_noise_workspace_bytes", "tcvn_noise_sigma", "tcvn_noise_replicate", "tcvn_noise_accumulate", "tcvn_noise_finish",
]

lib = _load()


def check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"libtcvn_hip: {what} failed with code {rc}")
