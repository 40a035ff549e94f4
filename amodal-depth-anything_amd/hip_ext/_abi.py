"""The boundary to libada_hip.so, described once: the constants and structs of include/ada_hip.h, one prototype per export, the loader.

Adding an export: its declaration in include/ada_hip.h, one PROTOTYPES row here (in the header's order), the wrapper in hip_ext/__init__.py.
tests/test_abi_cpu.py compares every row, every constant and both struct layouts with the header, so a row that drifts fails there and not on the device.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_uint16, c_uint32, c_void_p
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(_HERE), "csrc")

# --- constants mirrored from include/ada_hip.h (ADA_<name> there) -----------------------------
ABI_VERSION = 10
OK, EINVAL, EUNSUPPORTED, ELAUNCH = 0, -1, -2, -3
DT_F32, DT_F16, DT_BF16 = 0, 1, 2
DT_U8 = 3      # x / out of the rank filters
A_PLAIN, A_CONV3 = 0, 1
MAP_PLAIN, MAP_PAD, MAP_TOKEN, MAP_SHUFFLE = 0, 1, 2, 3
EP_BIAS, EP_GELU, EP_GAMMA, EP_RESIDUAL, EP_RELU_OP, EP_SWIGLU, EP_TAIL, EP_RELU_F32 = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40, 0x80
ACT_NONE, ACT_SIGMOID, ACT_RELU = 0, 1, 2
# indices into the per-image sums of ada_depth_eval_fwd
EVAL_N, EVAL_SUM_P, EVAL_SUM_G, EVAL_SUM_PP, EVAL_SUM_PG, EVAL_ABS_REL, EVAL_SQ_REL, EVAL_SQ, EVAL_LOG_SQ, EVAL_LOG, \
    EVAL_LOG10_ABS, EVAL_D1, EVAL_D2, EVAL_D3, EVAL_INV_SQ = range(15)
EVAL_NSUM = 16
# ada_protocol_fit_fwd / ada_protocol_eval_fwd: columns of a fit row, pixels per chunk and fp64 words of workspace per chunk
FIT_N, FIT_SUM_P, FIT_SUM_O, FIT_SUM_PP, FIT_SUM_PO, FIT_MIN_P, FIT_MAX_P, FIT_N_VISIBLE, FIT_N_WHOLE, FIT_SCALE, FIT_SHIFT = range(11)
FIT_NCOL = 12
PROTOCOL_CHUNK = 4096
PROTOCOL_WS_DOUBLES = 32
# ada_pil_resize_u8_fwd's filters (Pillow's own numbers) and ada_label_combine_fwd's casts
PIL_NEAREST, PIL_BICUBIC = 0, 3
LABEL_WRAP, LABEL_CLIP = 0, 1
# ada_quantile_fwd: modes, population flags, quantiles per call, elements per workgroup, bytes of workspace per image
Q_NUMPY, Q_TORCH = 0, 1
Q_EXCLUDE_VALUE, Q_POSITIVE_ONLY = 0x1, 0x2
QUANTILE_MAX_Q = 4
QUANTILE_CHUNK = 4096
QUANTILE_WS_BYTES_PER_IMAGE = 33792
# ada_mesh_triangles_fwd / ada_mesh_compact_fwd: candidates per ballot, cells or vertices per workgroup, workgroup sums per step of the scan
GEOM_WAVE = 64
GEOM_CHUNK = 1024
GEOM_SCAN_BLOCK = 1024
# ada_mesh_raster_fwd: samples in a box walked by the triangle's own thread / by one wave, a workgroup's tile of a larger box, the walking launch's
# grid and the least number of its workgroups that share a larger box, the depth modes
RASTER_SMALL_MAX = 16
RASTER_WAVE_MAX = 4096
RASTER_TILE_W, RASTER_TILE_H = 32, 8
RASTER_WALK_BLOCKS = 2048
RASTER_WALK_SHARE = 16
RASTER_OUT_W, RASTER_OUT_Z, RASTER_OUT_NORMALISED = 0, 1, 2
# ada_mesh_adaptive_fwd: midpoints of a level at or below which the remaining levels share one workgroup, the width of a subtree's cell, the largest
# side of the virtual grid
ADAPT_FOLD = 1024
ADAPT_CELL = 32
ADAPT_MAX_N = 16384
# ada_canny_fwd: pre-transforms and the Gaussian's radius cap; ada_soft_edge_fwd's radius cap; partial rows per image and columns of the edge sums
CANNY_PRE_NONE, CANNY_PRE_LOG, CANNY_PRE_LOG15 = 0, 1, 2
CANNY_MAX_RADIUS = 16
SOFT_EDGE_MAX_RADIUS = 8
EDGE_SUM_BLOCKS = 256
EDGE_N_BDE, EDGE_SUM_DT, EDGE_N_GT, EDGE_SUM_DP = range(4)
# ada_rank_filter_fwd / ada_extreme_filter_fwd: border rules, the named ranks (0 .. 100 are integer percents), the window limits, the workgroups' tiles
BORDER_MIRROR, BORDER_NEAREST, BORDER_IGNORE = 0, 1, 2
RANK_MIN, RANK_MEDIAN, RANK_MAX = 101, 102, 103
FILTER_MAX_WINDOW = 81
FILTER_MAX_EXTREME = 63
FILTER_TILE_W, FILTER_TILE_H = 64, 4
FILTER_COL_TILE_H = 16
# ada_nearest_valid_fwd: columns of a row staged per step of the row pass
INPAINT_CHUNK = 1024
# ada_membrane_*_fwd: a workgroup's tile, which is also the partition of every reduction (one partial sum per tile and plane)
MEMBRANE_TILE_H = 16
MEMBRANE_TILE_W = 64
# ada_guided_coeff_fwd / ada_guided_apply_fwd: the radius cap, outputs of a row per workgroup of the row passes, pixels per thread of the apply pass
GUIDED_MAX_RADIUS = 31
GUIDED_TILE_W = 256
GUIDED_APPLY_PX = 4


class IgemmArgs(ctypes.Structure):
    """struct ada_igemm_args (include/ada_hip.h) -- field order and types must match exactly."""
    _fields_ = [
        ("M", c_int32), ("N", c_int32), ("K", c_int32), ("a_mode", c_int32),
        ("A", c_void_p), ("lda", c_int64),
        ("Ho", c_int32), ("Wo", c_int32), ("Hp", c_int32), ("Wp", c_int32), ("stride", c_int32),
        ("W", c_void_p), ("bias", c_void_p), ("gamma", c_void_p), ("res", c_void_p), ("ldr", c_int64),
        ("res_row_mod", c_int32), ("res_row_off", c_int32), ("flags", c_int32),
        ("out_f32", c_void_p), ("ldo_f32", c_int64), ("map_f32", c_int32),
        ("out_op", c_void_p), ("ldo_op", c_int64), ("map_op", c_int32),
        ("map_h", c_int32), ("map_w", c_int32), ("shuffle_s", c_int32), ("shuffle_c", c_int32),
        ("tail_w", c_void_p), ("tail_b", c_float), ("tail_act", c_int32),
        ("split_seg", c_int32), ("a_dup_seg", c_int32),
        ("tap_cols", c_int32), ("tap_mask", c_uint16 * 16), ("a_wrap", c_int32), ("bias_row_mod", c_int32),
        ("f8_from", c_int32), ("f8_mid", c_int32), ("f8_scales", c_uint32),
    ]


class LayerNormArgs(ctypes.Structure):
    """struct ada_layernorm_args (include/ada_hip.h)."""
    _fields_ = [
        ("in_", c_void_p), ("ld_in", c_int64), ("rows_out", c_int32), ("dim", c_int32), ("group_in", c_int32), ("skip", c_int32),
        ("weight", c_void_p), ("bias", c_void_p), ("eps", c_float),
        ("out_op", c_void_p), ("ld_op", c_int64), ("map_op", c_int32), ("map_h", c_int32), ("map_w", c_int32), ("relu", c_int32),
        ("out_f32", c_void_p), ("ld_f32", c_int64), ("split_seg", c_int32),
        ("weight2", c_void_p), ("bias2", c_void_p), ("out2_op", c_void_p), ("ld2_op", c_int64),
        ("out2_group", c_int32), ("out2_skip", c_int32), ("split_seg2", c_int32), ("unshuffle_s", c_int32), ("tap_bias", c_void_p), ("identity", c_int32),
    ]


# --- one row per export, in the header's order: name -> (restype, argtypes) ---------------------
# A pointer to device memory is c_void_p (the wrappers pass tensor.data_ptr()); a pointer to a host array that ctypes builds is POINTER(T).
PROTOTYPES = {
    "ada_abi_version": (c_int, []),
    "ada_operand_dtype": (c_int, []),
    "ada_last_error": (c_char_p, []),
    "ada_igemm": (c_int, [POINTER(IgemmArgs), c_void_p]),
    "ada_attention_fwd": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "ada_attention_ex": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int64, c_int32, c_void_p]),
    "ada_layernorm_fwd": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_float, c_void_p, c_int64, c_int32, c_int32,
                                  c_int32, c_int32, c_void_p, c_int64, c_int32, c_void_p]),
    "ada_layernorm_ex": (c_int, [POINTER(LayerNormArgs), c_void_p]),
    "ada_tapsum_resize_fwd": (c_int, [c_void_p, c_int32, c_int64, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int64, c_void_p]),
    "ada_patchify": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, POINTER(c_float), POINTER(c_float), c_void_p, c_int64, c_int32, c_void_p]),
    "ada_pos_embed_resize": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_double, c_double, c_void_p, c_void_p]),
    "ada_write_cls": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "ada_bilinear_fwd": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64,
                                 c_int32, c_int32, c_int32, c_void_p]),
    "ada_dpt_tail_fwd": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_float, c_int32, c_void_p,
                                 c_void_p]),
    "ada_depth_eval_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_void_p, c_float, c_float, c_void_p, c_void_p]),
    "ada_protocol_fit_fwd": (c_int, [c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int64, c_void_p]),
    "ada_protocol_eval_fwd": (c_int, [c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int32, c_int32, c_int32, c_void_p, c_void_p,
                                      c_int64, c_void_p]),
    "ada_minmax_fwd": (c_int, [c_void_p, c_int32, c_int64, c_void_p, c_void_p]),
    "ada_normalize_fwd": (c_int, [c_void_p, c_void_p, c_int32, c_int64, c_void_p, c_void_p, c_void_p]),
    "ada_blend_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "ada_blend_ex": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "ada_depth_stats_fwd": (c_int, [c_void_p, c_int32, c_int64, c_int32, c_int32, c_void_p, c_void_p]),
    "ada_token_diversity_fwd": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "ada_ladder_select_fwd": (c_int, [c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_int32, c_double, c_double, c_double, c_double, c_int32, c_int32,
                                      c_int32, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ada_image_prep_fwd": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int64, c_int64, c_int32, c_int32, POINTER(c_float), POINTER(c_float), c_void_p,
                                   c_void_p]),
    "ada_depth_resize_fwd": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "ada_photo_prep_fwd": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "ada_mask_prep_fwd": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int64, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "ada_nearest_resize_fwd": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "ada_depth_render_fwd": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_float, c_float, c_void_p, c_void_p, c_int32, c_uint32, c_double, c_int32,
                                     c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "ada_quantile_fwd": (c_int, [c_void_p, c_void_p, c_int32, c_int64, POINTER(c_double), c_int32, c_int32, c_int32, c_double, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_int64, c_void_p]),
    "ada_range_map_fwd": (c_int, [c_void_p, c_void_p, c_int32, c_int64, c_float, c_float, c_int32, c_float, c_float, c_void_p, c_void_p]),
    "ada_depth_colorize_fwd": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_double, c_double, c_void_p, c_void_p, c_double, c_uint32, c_void_p,
                                       c_void_p]),
    "ada_pil_resize_u8_fwd": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int64, c_int64, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32,
                                      c_void_p, c_void_p, c_int32, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ada_label_combine_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                      c_void_p]),
    "ada_mask_label_fwd": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int64, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "ada_mask_stats_fwd": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "ada_mask_keep_area_fwd": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "ada_mask_grid_points_fwd": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "ada_depth_points_fwd": (c_int, [c_void_p, c_int32, c_int32, c_int32, POINTER(c_double), c_int32, c_double, c_double, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ada_mesh_triangles_fwd": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int32, c_double, c_double, c_double, c_int32, c_int32, c_int32, c_void_p, c_int32,
                                       c_void_p, c_void_p, c_int64, c_void_p]),
    "ada_mesh_compact_fwd": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_void_p,
                                     c_void_p, c_int64, c_void_p]),
    "ada_mesh_project_fwd": (c_int, [c_void_p, c_int32, c_int32, POINTER(c_double), c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ada_mesh_raster_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_int32, c_int32, c_int32, c_double, c_double, c_float,
                                    c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "ada_mesh_adaptive_workspace_bytes": (c_int, [c_int32, c_int32, POINTER(c_int64)]),
    "ada_mesh_adaptive_fwd": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int32, c_double, c_double, c_double, c_double, c_int32, c_int32, c_int32, c_int32,
                                      c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_int64, c_void_p]),
    "ada_canny_fwd": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                              c_void_p]),
    "ada_canny_hysteresis_fwd": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_float, c_void_p, c_void_p, c_int64, c_void_p]),
    "ada_edt_fwd": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int64, c_void_p]),
    "ada_edge_metric_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_double, c_void_p, c_void_p, c_int64, c_void_p]),
    "ada_soft_edge_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int64, c_void_p]),
    "ada_rank_filter_fwd": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_double, c_void_p, c_void_p, c_void_p]),
    "ada_extreme_filter_fwd": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_double, c_void_p, c_void_p, c_void_p,
                                       c_int64, c_void_p]),
    "ada_nearest_valid_workspace_bytes": (c_int, [c_int32, c_int32, c_int32, POINTER(c_int64)]),
    "ada_nearest_valid_fwd": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "ada_fill_gather_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_float, c_void_p, c_void_p]),
    "ada_push_pull_workspace_bytes": (c_int, [c_int32, c_int32, c_int32, c_int32, POINTER(c_int64)]),
    "ada_push_pull_fwd": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_float, c_void_p, c_void_p, c_int64, c_void_p]),
    "ada_membrane_workspace_bytes": (c_int, [c_int32, c_int32, c_int32, c_int32, POINTER(c_int64)]),
    "ada_membrane_begin_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_double, c_void_p, c_int64, c_void_p]),
    "ada_membrane_iterate_fwd": (c_int, [c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int64, c_void_p]),
    "ada_membrane_end_fwd": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                     c_void_p]),
    "ada_tile_blend_fwd": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "ada_selftest": (c_int, [c_void_p, c_int64, c_void_p]),
    "ada_debug_set_tile": (None, [c_int]),
    "ada_debug_set_variant": (None, [c_int]),
    "ada_debug_set_group": (None, [c_int]),
    "ada_debug_last_tile": (c_int, []),
    "ada_debug_set_timestamps": (None, [c_void_p]),
    "ada_debug_set_attention_variant": (None, [c_int]),
    "ada_debug_count_saturated": (c_int, [c_void_p, c_int64, c_void_p, c_void_p]),
    "ada_guided_workspace_bytes": (c_int, [c_int32, c_int32, c_int32, c_int32, POINTER(c_int64)]),
    "ada_guided_coeff_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_double, c_void_p,
                                     c_void_p, c_void_p, c_int64, c_void_p]),
    "ada_guided_apply_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_float, c_void_p, c_void_p]),
}
EXPORTS = tuple(PROTOTYPES)

# what hip_ext re-exports with `from ._abi import *`: every mirrored constant (the upper-case integers above) and the names listed here
__all__ = [k for k, v in list(globals().items()) if k.isupper() and isinstance(v, int)] + [
    "PROTOTYPES", "EXPORTS", "IgemmArgs", "LayerNormArgs", "HipExtError", "library_path", "load", "operand_dtype"]


class HipExtError(RuntimeError):
    pass


_lib = None
_lib_path = None


def library_path(bf16: bool = False) -> str:
    return os.path.join(_CSRC, "libada_hip_bf16.so" if bf16 else "libada_hip.so")


def load(path: Optional[str] = None):
    """Loads (once) and returns the ctypes handle.  Raises HipExtError when the library is absent."""
    global _lib, _lib_path
    if _lib is not None and (path is None or path == _lib_path):
        return _lib
    path = path or os.environ.get("ADA_HIP_LIB") or library_path()
    if not os.path.exists(path):
        raise HipExtError(
            f"libada_hip.so not found at {path}: build it with `python {os.path.join(_CSRC, 'build.py')}` "
            "(there is no CPU fallback for the HIP path)")
    try:
        lib = ctypes.CDLL(path)
    except OSError as e:  # pragma: no cover
        raise HipExtError(f"cannot load {path}: {e}") from e
    for name, (restype, argtypes) in PROTOTYPES.items():
        if not hasattr(lib, name):
            raise HipExtError(f"{path} does not export {name}")
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    if lib.ada_abi_version() != ABI_VERSION:
        raise HipExtError(f"{path}: ABI version {lib.ada_abi_version()} != binding version {ABI_VERSION}")
    _lib, _lib_path = lib, path
    return lib


def operand_dtype() -> torch.dtype:
    """torch dtype of the contraction operands the loaded library was built for."""
    return torch.float16 if load().ada_operand_dtype() == DT_F16 else torch.bfloat16


def _check(rc: int, what: str):
    if rc:      # ADA_OK is 0; a constant test, this runs after every launch
        msg = load().ada_last_error().decode(errors="replace")
        raise HipExtError(f"{what} failed (rc={rc}): {msg}")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream
