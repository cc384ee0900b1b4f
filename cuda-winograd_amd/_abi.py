"""The ctypes binding of libwinograd_mi355x.so.  ``SIGNATURES`` is the only place the Python side writes the C ABI
down: one row per function ``include/*.h`` declares, applied by ``lib()`` in one loop and checked against the headers,
like the two Structures, by tests/test_abi_signatures.py.  A new entry point: declare it in the header, add a row here.

Convention: tensor, workspace and stream parameters are ``c_void_p`` (callers pass ``data_ptr()`` ints and None);
host out-parameters are ``POINTER(<scalar>)`` / ``POINTER(<Structure>)``.
"""
from __future__ import annotations

import ctypes
import os
import sys
from ctypes import (POINTER, c_char_p, c_double, c_float, c_int, c_long, c_size_t, c_uint, c_uint64, c_ulonglong,
                    c_void_p)

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libwinograd_mi355x.so")


class WinoError(RuntimeError):
    pass


class DriverResult(ctypes.Structure):          # wino_driver_result
    _fields_ = [("mine_us", c_double), ("comparator_us", c_double), ("max_abs_err", c_double),
                ("max_rel_err", c_double), ("error_cnt", c_long), ("flops", c_double), ("N", c_int), ("gpus", c_int),
                ("steady_us", c_double)]


class CpuBaselineResult(ctypes.Structure):     # wino_cpu_baseline_result
    _fields_ = [("us", c_double), ("gflops", c_double), ("threads", c_int), ("reps", c_int),
                ("max_abs_diff", c_double), ("max_rel_diff", c_double)]


i, vp, sz = c_int, c_void_p, c_size_t
ip, fptr = POINTER(c_int), POINTER(c_float)

# name: (restype, [argtypes]), in the headers' order
SIGNATURES = {
    # ---- winograd_mi355x.h: runtime plumbing
    "wino_abi_version": (i, []),
    "wino_last_error_string": (c_char_p, []),
    "wino_last_status_name": (c_char_p, []),
    "wino_device_count": (i, [ip]),
    "wino_set_device": (i, [i]),
    "wino_device_name": (i, [i, c_char_p, sz]),
    "wino_malloc": (i, [POINTER(vp), sz]),
    "wino_free": (i, [vp]),
    "wino_memset": (i, [vp, i, sz]),
    "wino_memcpy_h2d": (i, [vp, vp, sz]),
    "wino_memcpy_d2h": (i, [vp, vp, sz]),
    "wino_memcpy_d2d": (i, [vp, vp, sz]),
    "wino_device_synchronize": (i, []),
    "wino_stream_create": (i, [POINTER(vp)]),
    "wino_stream_destroy": (i, [vp]),
    "wino_stream_synchronize": (i, [vp]),
    "wino_stream_check": (i, [vp]),
    "wino_stream_reset_scratch": (i, [vp]),
    "wino_event_create": (i, [POINTER(vp)]),
    "wino_event_destroy": (i, [vp]),
    "wino_event_record": (i, [vp, vp]),
    "wino_event_elapsed_ms": (i, [vp, vp, fptr]),
    # ---- 3x3 filters, layers and plans
    "wino_filter_f2_elems": (sz, [i, i]),
    "wino_filter_f2_index": (c_long, [i] * 5),
    "wino_filter_transform_f2": (i, [vp, vp, i, i, vp]),
    "wino_filter_import_f4": (i, [vp, vp, i, i, vp]),
    "wino_conv3x3_bn_relu": (i, [vp] * 5 + [i] * 4 + [vp]),
    "wino_conv3x3_prepare": (i, [i] * 3 + [vp]),
    "wino_conv3x3_bn_relu_hw": (i, [vp] * 5 + [i] * 6 + [vp]),
    "wino_conv3x3_prepare_hw": (i, [i] * 5 + [vp]),
    "wino_conv3x3_plan": (i, [i] * 6 + [ip, ip, POINTER(c_long), ip]),
    "wino_conv3x3_plan_groups": (i, [i] * 6 + [ip] * 4),
    "wino_conv3x3_small_plan": (i, [i] * 6 + [ip] * 4),
    "wino_conv3x3_small_plan2": (i, [i] * 6 + [ip] * 5),
    "wino_conv3x3_f4_workspace_bytes": (sz, [i] * 3),
    "wino_conv3x3_f4_bn_relu": (i, [vp] * 5 + [i] * 4 + [vp, sz, vp]),
    "wino_conv3x3_direct": (i, [vp] * 5 + [i] * 4 + [vp]),
    "wino_conv3x3_direct_hw": (i, [vp] * 5 + [i] * 6 + [vp]),
    # ---- 1x1 layers and plans
    "wino_conv1x1_bn": (i, [vp] * 5 + [c_long, i, i, i, vp]),
    "wino_conv1x1_bn_ex": (i, [vp] * 6 + [c_long, i, i, i, vp]),
    "wino_conv1x1_bn_ex_hw": (i, [vp] * 6 + [i] * 6 + [vp]),
    "wino_conv1x1_prepare": (i, [c_long, i, i, vp]),
    "wino_conv1x1_plan": (i, [c_long, i, i, i] + [ip] * 5),
    "wino_conv1x1_small_plan": (i, [c_long, i, i, i] + [ip] * 3),
    "wino_conv1x1_small_plan2": (i, [c_long, i, i, i] + [ip] * 5),
    "wino_debug_conv1x1_models": (i, [c_long, i, i, i, POINTER(c_double), POINTER(c_double)]),
    # ---- bottleneck and projection blocks
    "wino_residual_block_workspace_bytes": (sz, [i, i]),
    "wino_residual_block": (i, [vp] * 11 + [i] * 3 + [vp, sz, vp]),
    "wino_residual_block_workspace_bytes_hw": (sz, [i] * 4),
    "wino_residual_block_hw": (i, [vp] * 11 + [i] * 5 + [vp, sz, vp]),
    "wino_residual_block_prepare": (i, [i] * 3 + [vp]),
    "wino_residual_block_prepare_hw": (i, [i] * 5 + [vp]),
    "wino_proj_tail_elems": (sz, [i] * 3),
    "wino_proj_tail_pack": (i, [vp] * 7 + [i] * 3 + [vp]),
    "wino_proj_block_workspace_bytes_hw": (sz, [i] * 4),
    "wino_proj_block_hw": (i, [vp] * 9 + [i] * 7 + [vp, sz, vp]),
    "wino_proj_block_prepare_hw": (i, [i] * 7 + [vp]),
    "wino_proj_tail_plan": (i, [i] * 8 + [ip] * 2),
    "wino_conv3x3_s2_bn_relu_hw": (i, [vp] * 5 + [i] * 6 + [vp]),
    "wino_conv3x3_s2_prepare_hw": (i, [i] * 5 + [vp]),
    "wino_conv3x3_s2_plan": (i, [i] * 6 + [ip]),
    "wino_proj_block_v15_workspace_bytes_hw": (sz, [i] * 4),
    "wino_proj_block_v15_hw": (i, [vp] * 9 + [i] * 6 + [vp, sz, vp]),
    "wino_proj_block_v15_prepare_hw": (i, [i] * 6 + [vp]),
    "wino_conv1x1_direct": (i, [vp] * 5 + [c_long, i, i, i, vp]),
    # ---- driver configuration of the argument-less entry points
    "wino_driver_set_batch": (i, [i]),
    "wino_driver_set_gpus": (i, [i]),
    "wino_driver_set_quiet": (i, [i]),
    "wino_driver_get_batch": (i, []),
    "wino_driver_get_gpus": (i, []),
    "wino_driver_last_result": (i, [POINTER(DriverResult)]),
    "wino_driver_last_output": (fptr, [POINTER(sz)]),
    "wino_driver_pack_times": (i, [c_uint64, c_uint64]),
    "wino_driver_set_gpu_alias": (i, [i]),
    "wino_driver_set_stdout_compat": (i, [i]),
    "wino_driver_get_stdout_compat": (i, []),
    "wino_driver_cpu_baseline": (i, [POINTER(CpuBaselineResult)]),
    # ---- basic blocks
    "wino_conv3x3_bn_add_relu_hw": (i, [vp] * 6 + [i] * 6 + [vp]),
    "wino_basic_block_workspace_bytes_hw": (sz, [i] * 4),
    "wino_basic_block_hw": (i, [vp] * 8 + [i] * 4 + [vp, sz, vp]),
    "wino_basic_block_prepare_hw": (i, [i] * 4 + [vp]),
    "wino_s2_proj_elems": (sz, [i] * 2),
    "wino_s2_proj_pack": (i, [vp] * 7 + [i] * 2 + [vp]),
    "wino_conv3x3_s2_proj_bn_relu_hw": (i, [vp] * 4 + [i] * 5 + [vp]),
    "wino_basic_block_s2_workspace_bytes_hw": (sz, [i] * 4),
    "wino_basic_block_s2_hw": (i, [vp] * 6 + [i] * 5 + [vp, sz, vp]),
    "wino_basic_block_s2_prepare_hw": (i, [i] * 5 + [vp]),
    # ---- stem, head, VGG
    "wino_stem_filter_elems": (sz, [i]),
    "wino_stem_filter_pack": (i, [vp] * 4 + [i, vp]),
    "wino_stem_hw": (i, [vp] * 3 + [i] * 5 + [vp]),
    "wino_stem_plan": (i, [i] * 5 + [ip]),
    "wino_head_elems": (sz, [i] * 2),
    "wino_head_pack": (i, [vp] * 3 + [i] * 2 + [vp]),
    "wino_head_workspace_bytes": (sz, [i] * 3),
    "wino_head_prepare": (i, [i] * 3 + [vp]),
    "wino_avgpool_fc_hw": (i, [vp] * 3 + [i] * 6 + [vp, sz, vp]),
    "wino_conv3x3_bn_relu_pool_hw": (i, [vp] * 5 + [i] * 6 + [vp]),
    "wino_image_pack_hw": (i, [vp] * 2 + [i] * 5 + [vp]),
    "wino_avgpool7_flatten_hw": (i, [vp] * 2 + [i] * 5 + [vp]),
    # ---- grouped 3x3 and the ResNeXt blocks
    "wino_conv3x3_grouped_filter_elems": (sz, [i] * 2),
    "wino_conv3x3_grouped_filter_pack": (i, [vp] * 2 + [i] * 2 + [vp]),
    "wino_conv3x3_grouped_bn_relu_hw": (i, [vp] * 5 + [i] * 7 + [vp]),
    "wino_conv3x3_grouped_plan": (i, [i] * 6 + [ip] * 4),
    "wino_grouped_residual_block_hw": (i, [vp] * 11 + [i] * 6 + [vp, sz, vp]),
    "wino_grouped_residual_block_prepare_hw": (i, [i] * 6 + [vp]),
    "wino_grouped_proj_block_hw": (i, [vp] * 9 + [i] * 8 + [vp, sz, vp]),
    "wino_grouped_proj_block_prepare_hw": (i, [i] * 8 + [vp]),
    # ---- Feature Pyramid Network
    "wino_fpn_level_hw": (i, [vp] * 10 + [i] * 6 + [vp]),
    "wino_fpn_level_prepare_hw": (i, [i] * 5 + [vp]),
    # ---- dilated 3x3 and the dilated bottleneck blocks
    "wino_conv3x3_dilated_bn_relu_hw": (i, [vp] * 5 + [i] * 7 + [vp]),
    "wino_conv3x3_dilated_prepare_hw": (i, [i] * 6 + [vp]),
    "wino_conv3x3_dilated_plan": (i, [i] * 7 + [ip]),
    "wino_dilated_residual_block_hw": (i, [vp] * 11 + [i] * 6 + [vp, sz, vp]),
    "wino_dilated_residual_block_prepare_hw": (i, [i] * 6 + [vp]),
    "wino_dilated_proj_block_hw": (i, [vp] * 9 + [i] * 7 + [vp, sz, vp]),
    "wino_dilated_proj_block_prepare_hw": (i, [i] * 7 + [vp]),
    # ---- the concat projection and the ASPP module
    "wino_conv1x1_cat_bn_hw": (i, [vp, c_long] + [vp] * 4 + [i] * 7 + [vp]),
    "wino_conv1x1_cat_prepare_hw": (i, [i] * 6 + [vp]),
    "wino_conv1x1_cat_plan": (i, [i] * 7 + [ip]),
    "wino_aspp_hw": (i, [vp] * 20 + [i] * 9 + [vp, sz, vp]),
    "wino_aspp_prepare_hw": (i, [i] * 9 + [vp]),
    # ---- bilinear resize and label map
    "wino_resize_bilinear_hw": (i, [vp] * 3 + [i] * 8 + [vp]),
    "wino_resize_bilinear_plan": (i, [i] * 8 + [ip]),
    # ---- multi-scale RoIAlign
    "wino_roi_align_hw": (i, [vp] * 4 + [ip, fptr] + [i] * 4 + [vp] + [i] * 3 + [c_float, i, vp, i, vp]),
    "wino_roi_align_launches": (i, [i] * 3 + [POINTER(c_long)]),
    # ---- box decoding and batched NMS
    "wino_box_decode_hw": (i, [vp] + [i] * 6 + [vp] + [i] * 4 + [vp] + [c_float] * 5 + [vp, c_long, c_long] * 2 + [vp]),
    "wino_batched_nms_hw": (i, [vp] * 3 + [i] * 2 + [c_float] * 3 + [i] + [vp] * 4 + [sz, vp]),
    # ---- mask selection and paste
    "wino_mask_paste_hw": (i, [vp, i] + [vp] * 3 + [i] * 7 + [c_float] + [vp] * 3),
    # ---- heatmaps to keypoints
    "wino_keypoints_hw": (i, [vp, i, vp, vp] + [i] * 5 + [vp] * 3),
    # ---- image transform
    "wino_image_transform_hw": (i, [POINTER(vp), ip, ip, i, i, i, fptr, fptr, vp, i, i, vp]),
    "wino_transform_size": (i, [i] * 4 + [ip] * 2),
    # ---- segmented top-k and sort
    "wino_select_topk_hw": (i, [vp, i, c_long, i, POINTER(c_long), ip, ip, i, c_float] + [vp] * 3 + [c_long, vp, c_long]
                            + [vp] * 2 + [sz, vp]),
    "wino_select_topk_map_hw": (i, [vp] + [i] * 7 + [c_float] + [vp] * 3 + [c_long] * 2 + [vp, sz, vp]),
    # ---- RetinaNet: decode only the selected anchors
    "wino_retina_decode_hw": (i, [vp, i, i, c_long, c_long, vp] + [i] * 5 + [vp, i, i, vp, c_float, vp, vp, vp]),
    # ---- GroupNorm (+ ReLU) on a padded map
    "wino_groupnorm_plan": (i, [i] * 6 + [ip] * 2),
    "wino_groupnorm_relu_hw": (i, [vp] * 4 + [i] * 5 + [c_float, i, vp, sz, vp]),
    # ---- FCOS: score map and decode of the selected locations
    "wino_fcos_score_map_hw": (i, [vp] * 2 + [i] * 7 + [vp]),
    "wino_fcos_decode_hw": (i, [vp, i, i, c_long, c_long, vp] + [i] * 5 + [vp, i, i, vp, vp, vp, vp]),
    # ---- diagnostics
    "wino_debug_reload_knobs": (i, []),
    "wino_debug_tickets_in_use": (i, [vp, POINTER(c_long)]),
    "wino_debug_poison_ticket": (i, [vp, c_long, c_uint]),
    "wino_diag_last_clock": (i, [i, vp, POINTER(c_ulonglong)]),
    "wino_diag_conv3x3_clock": (i, [vp] * 5 + [i] * 3 + [vp, ip, vp]),
    # ---- Kernel*.h: the reference's argument-less entry points
    **{name: (i, []) for name in ("kernel_128", "kernel_256", "kernel_128_1_in", "kernel_128_1_out", "kernel_256_1_in",
                                  "kernel_256_1_out")},
    # ---- util.h
    "get_parameter": (fptr, [c_char_p, i]),
    "transpose": (fptr, [fptr, i, i]),
    "getTimeMicroseconds64": (c_uint64, []),
    "output_checker": (c_float, [vp, vp, i, i, i]),
    "output_checker_accumulate": (c_float, [vp, vp, i, i, i, fptr, POINTER(c_long)]),
}
ABI_SYMBOLS = list(SIGNATURES)
del i, vp, sz, ip, fptr   # (the table's shorthand, not names of this module)

_lib = None


def lib() -> ctypes.CDLL:
    """Load libwinograd_mi355x.so (built in-tree by `make` / __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    # the package re-exports LIB_PATH, and a tool may point that at another build before the first call
    path = getattr(sys.modules.get(__package__), "LIB_PATH", LIB_PATH)
    if not os.path.exists(path):
        raise WinoError(
            f"{path} not found: build it with `make` (or __graft_entry__.build()). "
            "There is no fallback path.")
    L = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise WinoError(f"{what} failed (rc={rc}): {lib().wino_last_error_string().decode()}")
