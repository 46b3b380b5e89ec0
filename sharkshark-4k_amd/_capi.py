"""ctypes binding of libss4k_hip.so (C ABI declared in include/ss4k.h).

PyTorch is used only as the owner of device memory and streams: every function here takes
``torch`` CUDA(HIP) tensors, passes their ``data_ptr()`` and the current stream to the library and
returns tensors.  There is no CPU fallback: a missing library or a failing call raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SS4K_LIB") or os.path.join(_HERE, "libss4k_hip.so")  # override = A/B builds

FSRCNN, RRDBNET, SRVGG, BSVD = 1, 2, 3, 4
F32, F16 = 0, 1

# every symbol include/ss4k.h declares (tests check the library exports all of them)
SYMBOLS = [
    "ss4k_abi_version", "ss4k_last_error", "ss4k_ctx_create", "ss4k_ctx_destroy", "ss4k_ctx_device",
    "ss4k_model_param_count", "ss4k_model_create", "ss4k_model_destroy", "ss4k_model_out_shape",
    "ss4k_model_in_channels", "ss4k_model_forward", "ss4k_model_check", "ss4k_upscaler_create", "ss4k_upscaler_destroy",
    "ss4k_upscaler_reset", "ss4k_upscaler_out_shape", "ss4k_upscaler_last_enqueue_ms", "ss4k_model_workspace_bytes", "ss4k_upscale_frames", "ss4k_upscaler_enable_taps",
    "ss4k_upscaler_read_tap", "ss4k_op_u8nhwc_to_f32nchw", "ss4k_op_area_resize", "ss4k_op_bicubic_resize",
    "ss4k_op_bilinear_resize", "ss4k_op_depthwise_reflect", "ss4k_op_plane_stats", "ss4k_op_f32nchw_to_u8nhwc",
    "ss4k_prof_enable", "ss4k_prof_reset", "ss4k_prof_read", "ss4k_prof_read_kind", "ss4k_prof_read_family", "ss4k_prof_read_section_ms",
    "ss4k_stream_pair_check", "ss4k_op_cv_area_shape", "ss4k_op_cv_area_resize_u8",
    "ss4k_frvsr_param_count", "ss4k_frvsr_create", "ss4k_frvsr_destroy", "ss4k_frvsr_step", "ss4k_frvsr_workspace_bytes",
    "ss4k_frvsr_prof_enable", "ss4k_frvsr_prof_read", "ss4k_frvsr_upscaler_create", "ss4k_frvsr_upscaler_destroy",
    "ss4k_frvsr_upscaler_reset", "ss4k_frvsr_upscaler_out_shape", "ss4k_frvsr_upscale_frames", "ss4k_frvsr_upscaler_enable_taps",
    "ss4k_frvsr_upscaler_read_tap", "ss4k_op_backward_warp", "ss4k_op_bicubic_upsample4",
    "ss4k_frvsr_upscaler_create_streams", "ss4k_frvsr_upscale_streams", "ss4k_frvsr_upscaler_reset_stream", "ss4k_frvsr_upscaler_state_bytes",
    "ss4k_frvsr_upscale_streams_at",
    "ss4k_frvsr_param_count_as", "ss4k_frvsr_create_as", "ss4k_frvsr_generator",
    "ss4k_frvsr_param_count_ex", "ss4k_frvsr_create_ex", "ss4k_frvsr_degradation",
    "ss4k_frvsr_upscaler_set_scene_cut", "ss4k_frvsr_upscaler_scene_cut", "ss4k_frvsr_upscaler_scene_cut_stats", "ss4k_frvsr_upscaler_scene_cut_total",
    "ss4k_op_frame_sad_u8",
    "ss4k_bsvd_online_create", "ss4k_bsvd_online_destroy", "ss4k_bsvd_online_lag", "ss4k_bsvd_online_push", "ss4k_bsvd_online_flush",
    "ss4k_bsvd_online_reset", "ss4k_bsvd_online_pending", "ss4k_bsvd_online_state_bytes",
    "ss4k_upscaler_temporal_create", "ss4k_upscaler_temporal_destroy", "ss4k_upscale_frames_temporal", "ss4k_upscaler_temporal_flush",
    "ss4k_upscaler_temporal_reset", "ss4k_upscaler_temporal_out_shape", "ss4k_upscaler_temporal_pending", "ss4k_upscaler_temporal_state_bytes",
    "ss4k_bsvd_online_push_cuts",
    "ss4k_upscaler_temporal_set_scene_cut", "ss4k_upscaler_temporal_scene_cut", "ss4k_upscaler_temporal_scene_cut_stats",
    "ss4k_upscaler_temporal_scene_cut_total",
    # several streams on one temporal upscaler: slots and rounds
    "ss4k_upscaler_temporal_create_streams", "ss4k_upscale_round_temporal", "ss4k_upscaler_temporal_flush_stream",
    "ss4k_upscaler_temporal_reset_stream", "ss4k_upscaler_temporal_pending_stream", "ss4k_upscaler_temporal_scene_cut_stats_stream",
    "ss4k_upscaler_temporal_stream_state_bytes_for", "ss4k_upscaler_temporal_release_idle",
    # a denoise rate per slot
    "ss4k_upscaler_temporal_set_denoise_rate_stream",
    # the frame-recurrent chain with the online denoiser in front
    "ss4k_frvsr_temporal_create", "ss4k_frvsr_temporal_destroy", "ss4k_frvsr_temporal_round", "ss4k_frvsr_temporal_flush_stream",
    "ss4k_frvsr_temporal_reset_stream", "ss4k_frvsr_temporal_pending_stream", "ss4k_frvsr_temporal_set_denoise_rate_stream",
    "ss4k_frvsr_temporal_out_shape", "ss4k_frvsr_temporal_state_bytes", "ss4k_frvsr_temporal_stream_state_bytes_for",
    "ss4k_frvsr_temporal_release_idle",
    # ... and its scene cuts
    "ss4k_frvsr_temporal_set_scene_cut", "ss4k_frvsr_temporal_scene_cut", "ss4k_frvsr_temporal_scene_cut_stats_stream",
    "ss4k_frvsr_temporal_scene_cut_total",
    # ... and an lr_shape that 4 does not divide: reflect-pad in front of the denoiser, crop behind it
    "ss4k_frvsr_temporal_create_padded",
    # the motion-adaptive noise map of both temporal chains
    "ss4k_upscaler_temporal_set_noise_map", "ss4k_upscaler_temporal_noise_map", "ss4k_frvsr_temporal_set_noise_map",
    "ss4k_frvsr_temporal_noise_map",
]
NOISE_MAPS = {"constant": 0, "motion": 1}   # SS4K_NOISE_MAP_*


def noise_map_mode(word) -> int:
    """``'constant'`` / ``'motion'`` -> SS4K_NOISE_MAP_*; anything else raises ``ValueError``."""
    if not isinstance(word, str) or word not in NOISE_MAPS:
        raise ValueError(f"noise_map is 'constant' or 'motion', not {word!r}")
    return NOISE_MAPS[word]


# include/ss4k_dev.h: libss4k_hip_dev.so only (SS4K_LIB=.../libss4k_hip_dev.so, or load(build.LIB_DEV))
DEV_SYMBOLS = [
    "ss4k_bench_conv",
    # the internal glue launchers and their route report (tests/test_gpu_glue_budget.py)
    "ss4k_dev_op_area_normalized", "ss4k_dev_op_tail_fused", "ss4k_dev_op_bicubic_u8", "ss4k_dev_op_bicubic", "ss4k_dev_op_bilinear",
    "ss4k_dev_gauss17_taps", "ss4k_dev_op_gauss17_reflect", "ss4k_dev_op_depthwise_reflect", "ss4k_dev_op_normalize", "ss4k_dev_op_sub",
    "ss4k_dev_op_clamp01", "ss4k_dev_op_plane_stats", "ss4k_dev_op_plane_stats_u8nhwc", "ss4k_dev_op_plane_stats_partial",
    "ss4k_dev_op_plane_stats_u8nhwc_partial", "ss4k_dev_op_plane_stats_finish", "ss4k_dev_op_plane_stats_finish2",
    "ss4k_dev_op_ps_nchw_addbase", "ss4k_dev_op_pack_input", "ss4k_dev_op_temporal_shift",
    "ss4k_dev_glue_routes_reset", "ss4k_dev_glue_routes_read",
    # the launchers of csrc/frvsr.hip (tests/test_gpu_frvsr_glue_budget.py)
    "ss4k_dev_op_frvsr_maxpool2_planes", "ss4k_dev_op_frvsr_bilinear2_planes", "ss4k_dev_op_frvsr_flow_finish",
    "ss4k_dev_op_frvsr_warp_s2d_planes", "ss4k_dev_op_frvsr_warp_s2d_planes_items", "ss4k_dev_op_frvsr_ps4_conv_tail",
    "ss4k_dev_op_frvsr_ps4_conv_tail_items", "ss4k_dev_op_frvsr_planes_to_nchw", "ss4k_dev_op_frvsr_clamp01_to",
    "ss4k_dev_op_frvsr_frames_in_items", "ss4k_dev_op_frvsr_pack_lr_items", "ss4k_dev_op_frvsr_frames_out_items",
    # the launchers of csrc/frvsr_bi.hip, degradation 'BI' (tests/test_gpu_frvsr_bi_glue_budget.py)
    "ss4k_dev_op_frvsrbi_bilinear_upsample4", "ss4k_dev_op_frvsrbi_warp_s2d_planes", "ss4k_dev_op_frvsrbi_warp_s2d_planes_items",
    "ss4k_dev_op_frvsrbi_bilinear4_add", "ss4k_dev_op_frvsrbi_bilinear4_add_items",
    # a whole step with every item's flow and warped space-to-depth tensor copied out (tests/test_gpu_frvsr_budget.py)
    "ss4k_dev_frvsr_step_taps",
    # the tail of a TecoGAN generator alone, and the host-side embedding of its transposed layers (tests/test_gpu_tecogan_tail.py)
    "ss4k_dev_frvsr_tail_taps", "ss4k_dev_frvsr_embed_convt", "ss4k_dev_frvsr_pack_convt",
    # guard mode: red zones and 0xFF poison for every device buffer of the library (tests/test_gpu_memory_hygiene.py)
    "ss4k_dev_guard_enable", "ss4k_dev_guard_check", "ss4k_dev_guard_poison", "ss4k_dev_guard_selftest", "ss4k_dev_guard_poison_frvsr", "ss4k_dev_guard_poison_temporal",
    # stream ordering: a bounded delay on any stream; the frame lanes' handicap, counters and dropped-join control (tests/test_gpu_lane_order.py)
    "ss4k_dev_op_spin", "ss4k_dev_lane_handicap", "ss4k_dev_lane_counts", "ss4k_dev_lane_counts_reset", "ss4k_dev_lane_drop_join",
    # the kernels of csrc/bsvd_online.hip on caller buffers (tests/test_gpu_bsvd_online.py)
    "ss4k_dev_op_bsvd_online_shift", "ss4k_dev_op_bsvd_online_carry",
    # ... and the scene-cut builds (tests/test_gpu_bsvd_cuts.py)
    "ss4k_dev_op_bsvd_online_shift_cuts", "ss4k_dev_op_bsvd_noise_planes",
    # the kernel of a temporal round (tests/test_gpu_temporal_streams_kernel.py)
    "ss4k_dev_op_temporal_gather", "ss4k_dev_op_temporal_gather_levels",
    # the glue kernel of the frame-recurrent chain with the denoiser in front, and the poison of its job buffers
    # (tests/test_gpu_frvsr_temporal_kernel.py, tests/test_gpu_frvsr_temporal_hygiene.py)
    "ss4k_dev_op_frvsrt_denoised_in", "ss4k_dev_guard_poison_frvsr_temporal",
    # the late reset of a scene cut in that chain (tests/test_gpu_frvsr_temporal_cuts_kernel.py)
    "ss4k_dev_op_frvsrt_clear_flagged",
    # the two kernels of the padded form of that chain (tests/test_gpu_frvsr_temporal_pad_kernel.py)
    "ss4k_dev_op_temporal_gather_pad", "ss4k_dev_op_frvsrt_denoised_in_crop",
    # the gathers with the motion-adaptive noise map, their tile and their taps (tests/test_gpu_temporal_motion_kernel.py)
    "ss4k_dev_op_temporal_gather_motion", "ss4k_dev_op_temporal_gather_motion_pad", "ss4k_dev_temporal_motion_tile",
    "ss4k_dev_temporal_motion_taps",
]


class ModelDesc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("dtype", C.c_int32), ("scale", C.c_int32), ("num_feat", C.c_int32),
                ("num_block", C.c_int32), ("num_grow_ch", C.c_int32), ("bsvd_chns", C.c_int32 * 3),
                ("bsvd_mid_ch", C.c_int32), ("bsvd_interm_ch", C.c_int32), ("bsvd_stream", C.c_int32),
                ("flags", C.c_int32), ("reserved", C.c_int32 * 3)]


# ss4k_model_desc.flags (include/ss4k.h)
MODEL_FS_EXACT, MODEL_ONE_CHAIN, MODEL_TWO_CHAINS, MODEL_TILE_ROWS_16, MODEL_TILE_ROWS_20 = 1, 2, 4, 16, 32
MODEL_NO_PAIR, MODEL_HR_F32, MODEL_NO_DENSE, MODEL_NO_WIDE, MODEL_NO_UPS_PRESUM, MODEL_NO_W16 = 256, 512, 1024, 4096, 8192, 32768
MODEL_FLAGS_ALL = 1 | 2 | 4 | 16 | 32 | 256 | 512 | 1024 | 4096 | 8192 | 32768


class UpscaleCfg(C.Structure):
    _fields_ = [("lr_h", C.c_int32), ("lr_w", C.c_int32), ("out_h", C.c_int32), ("out_w", C.c_int32),
                ("lr_hr_resize", C.c_int32), ("single_mode", C.c_int32), ("sr_is_realesrgan", C.c_int32),
                ("denoising", C.c_int32), ("reserved0", C.c_int32), ("denoise_rate", C.c_double),
                ("reserved", C.c_int32 * 6)]


class FrvsrDesc(C.Structure):
    _fields_ = [("dtype", C.c_int32), ("num_feat", C.c_int32), ("num_block", C.c_int32), ("flags", C.c_int32),
                ("reserved", C.c_int32 * 4)]


class SceneCutStats(C.Structure):
    """ss4k_scene_cut_stats: a slot's counters and the values of its last frame (include/ss4k.h)."""
    _fields_ = [("compared", C.c_uint64), ("cuts", C.c_uint64), ("last_sad", C.c_uint64), ("last_score", C.c_uint64),
                ("last_was_cut", C.c_int32), ("reserved", C.c_int32)]


class Ss4kError(RuntimeError):
    pass


_lib = None
#: set once this process has created a library context = initialised the HIP runtime (BaseService.start_method reads it: a child forked
#: from such a process cannot use the GPU)
GPU_TOUCHED = False


def lib() -> C.CDLL:
    """Load the HIP library; fail loudly if it has not been built (no fallback path exists)."""
    global _lib
    if _lib is None:
        _lib = load(LIB_PATH)
    return _lib


def load(path: str) -> C.CDLL:
    """Bind one build of the library (the product library, or libss4k_hip_dev.so for a test that needs its hooks)."""
    if not os.path.exists(path):
        raise Ss4kError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
    L = C.CDLL(path)
    vp, i, sz = C.c_void_p, C.c_int, C.c_size_t
    L.ss4k_last_error.restype = C.c_char_p
    L.ss4k_ctx_create.argtypes = [i, C.POINTER(vp)]
    L.ss4k_ctx_destroy.argtypes = [vp]; L.ss4k_ctx_destroy.restype = None
    L.ss4k_ctx_device.argtypes = [vp]
    L.ss4k_model_param_count.argtypes = [C.POINTER(ModelDesc)]; L.ss4k_model_param_count.restype = sz
    L.ss4k_model_create.argtypes = [vp, C.POINTER(ModelDesc), vp, sz, C.POINTER(vp)]
    L.ss4k_model_destroy.argtypes = [vp]; L.ss4k_model_destroy.restype = None
    L.ss4k_model_out_shape.argtypes = [vp, i, i, i, C.POINTER(i), C.POINTER(i), C.POINTER(i)]
    L.ss4k_model_in_channels.argtypes = [vp]
    L.ss4k_model_forward.argtypes = [vp, vp, vp, i, i, i, vp]
    if hasattr(L, "ss4k_model_check"):   # (absent from ABI-1 builds, which tools/lib_ab.py loads for A/B timing)
        L.ss4k_model_check.argtypes = [vp, i]
    L.ss4k_upscaler_create.argtypes = [vp, C.POINTER(UpscaleCfg), vp, vp, C.POINTER(vp)]
    L.ss4k_upscaler_destroy.argtypes = [vp]; L.ss4k_upscaler_destroy.restype = None
    L.ss4k_upscaler_reset.argtypes = [vp]
    L.ss4k_model_workspace_bytes.argtypes = [vp, i, i, i, C.POINTER(C.c_size_t)]
    L.ss4k_upscaler_last_enqueue_ms.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.ss4k_upscaler_out_shape.argtypes = [vp, i, i, i, C.POINTER(i), C.POINTER(i)]
    L.ss4k_upscale_frames.argtypes = [vp, vp, i, i, i, vp, sz, vp]
    L.ss4k_upscaler_enable_taps.argtypes = [vp, i]
    L.ss4k_upscaler_read_tap.argtypes = [vp, i, vp, sz, C.POINTER(i * 4), vp]
    L.ss4k_op_u8nhwc_to_f32nchw.argtypes = [vp, vp, vp, i, i, i, i, vp]
    for name in ("ss4k_op_area_resize", "ss4k_op_bicubic_resize", "ss4k_op_bilinear_resize"):
        getattr(L, name).argtypes = [vp, vp, vp, i, i, i, i, i, vp]
    L.ss4k_op_depthwise_reflect.argtypes = [vp, vp, vp, i, i, i, vp, i, vp]
    L.ss4k_op_plane_stats.argtypes = [vp, vp, vp, i, i, vp]
    L.ss4k_op_f32nchw_to_u8nhwc.argtypes = [vp, vp, vp, i, i, i, i, vp]
    if hasattr(L, "ss4k_bench_conv"):  # dev library only
        L.ss4k_bench_conv.argtypes = [vp, i, i, i, i, i, i, i, i, i, C.POINTER(C.c_double), vp]
    if hasattr(L, "ss4k_dev_glue_routes_read"):  # dev library only: the glue launchers (include/ss4k_dev.h)
        f = C.c_float
        L.ss4k_dev_op_area_normalized.argtypes = [vp, vp, i, vp, i, i, i, i, i, vp, vp, vp]
        L.ss4k_dev_op_tail_fused.argtypes = [vp, vp, i, vp, vp, i, i, i, i, i, i, vp, vp, vp]
        L.ss4k_dev_op_bicubic_u8.argtypes = [vp, vp, i, vp, i, i, i, i, i, i, vp]
        L.ss4k_dev_op_bicubic.argtypes = [vp, vp, vp, i, i, i, i, i, i, vp]
        L.ss4k_dev_op_bilinear.argtypes = [vp, vp, vp, i, i, i, i, i, i, i, vp]
        L.ss4k_dev_gauss17_taps.argtypes = [vp]
        L.ss4k_dev_op_gauss17_reflect.argtypes = [vp, vp, vp, vp, vp, i, i, i, vp]
        L.ss4k_dev_op_depthwise_reflect.argtypes = [vp, vp, vp, vp, i, i, i, i, i, vp, f, f, vp]
        L.ss4k_dev_op_normalize.argtypes = [vp, vp, vp, vp, i, i, vp]
        L.ss4k_dev_op_sub.argtypes = [vp, vp, vp, vp, sz, vp]
        L.ss4k_dev_op_clamp01.argtypes = [vp, vp, sz, vp]
        L.ss4k_dev_op_plane_stats.argtypes = [vp, vp, vp, i, vp, i, i, vp]
        L.ss4k_dev_op_plane_stats_u8nhwc.argtypes = [vp, vp, vp, vp, i, i, vp]
        L.ss4k_dev_op_plane_stats_partial.argtypes = [vp, vp, vp, i, i, i, i, i, vp]
        L.ss4k_dev_op_plane_stats_u8nhwc_partial.argtypes = [vp, vp, vp, i, i, i, i, vp]
        L.ss4k_dev_op_plane_stats_finish.argtypes = [vp, vp, vp, i, i, vp]
        L.ss4k_dev_op_plane_stats_finish2.argtypes = [vp, vp, vp, vp, i, i, i, i, vp]
        L.ss4k_dev_op_ps_nchw_addbase.argtypes = [vp, vp, i, vp, i, vp, i, i, i, i, i, vp, vp]
        L.ss4k_dev_op_pack_input.argtypes = [vp, vp, vp, i, i, i, i, i, i, i, vp]
        L.ss4k_dev_op_temporal_shift.argtypes = [vp, vp, vp, i, i, sz, i, i, i, vp]
        L.ss4k_dev_glue_routes_reset.argtypes = []
        # csrc/frvsr.hip; the _items forms take host arrays of device pointers ((C.c_void_p * n)(...))
        L.ss4k_dev_op_frvsr_maxpool2_planes.argtypes = [vp, vp, vp, i, i, i, i, i, vp]
        L.ss4k_dev_op_frvsr_bilinear2_planes.argtypes = [vp, vp, vp, i, i, i, i, i, vp]
        L.ss4k_dev_op_frvsr_flow_finish.argtypes = [vp, vp, vp, i, i, i, i, i, vp]
        L.ss4k_dev_op_frvsr_warp_s2d_planes.argtypes = [vp, vp, vp, vp, i, i, i, i, vp]
        L.ss4k_dev_op_frvsr_warp_s2d_planes_items.argtypes = [vp, vp, vp, vp, i, i, i, i, vp]
        L.ss4k_dev_op_frvsr_ps4_conv_tail.argtypes = [vp, vp, i, vp, vp, i, i, i, vp]
        L.ss4k_dev_op_frvsr_ps4_conv_tail_items.argtypes = [vp, vp, i, vp, vp, i, i, i, vp]
        L.ss4k_dev_op_frvsr_planes_to_nchw.argtypes = [vp, vp, i, vp, i, i, i, i, vp]
        L.ss4k_dev_op_frvsr_clamp01_to.argtypes = [vp, vp, vp, sz, vp]
        L.ss4k_dev_op_frvsr_frames_in_items.argtypes = [vp, vp, vp, i, i, i, i, i, vp]
        L.ss4k_dev_op_frvsr_pack_lr_items.argtypes = [vp, vp, vp, vp, vp, i, i, i, i, vp]
        L.ss4k_dev_op_frvsr_frames_out_items.argtypes = [vp, vp, vp, i, i, i, i, i, vp]
        L.ss4k_dev_glue_routes_read.argtypes = [i, C.c_char_p, sz, C.POINTER(C.c_int64)]
    if hasattr(L, "ss4k_dev_op_frvsrbi_bilinear_upsample4"):   # csrc/frvsr_bi.hip
        L.ss4k_dev_op_frvsrbi_bilinear_upsample4.argtypes = [vp, vp, vp, i, i, i, vp]
        L.ss4k_dev_op_frvsrbi_warp_s2d_planes.argtypes = [vp, vp, vp, vp, i, i, i, i, vp]
        L.ss4k_dev_op_frvsrbi_warp_s2d_planes_items.argtypes = [vp, vp, vp, vp, i, i, i, i, vp]
        L.ss4k_dev_op_frvsrbi_bilinear4_add.argtypes = [vp, vp, vp, vp, i, i, i, vp]
        L.ss4k_dev_op_frvsrbi_bilinear4_add_items.argtypes = [vp, vp, vp, vp, i, i, i, vp]
    if hasattr(L, "ss4k_dev_frvsr_step_taps"):  # dev library only
        L.ss4k_dev_frvsr_step_taps.argtypes = [vp, vp, vp, vp, vp, vp, vp, i, i, i, vp]
    if hasattr(L, "ss4k_dev_guard_check"):  # dev library only: guard mode
        L.ss4k_dev_guard_enable.argtypes = [i]
        L.ss4k_dev_guard_check.argtypes = [C.POINTER(i), C.POINTER(i), C.POINTER(i), C.c_char_p, sz]
        L.ss4k_dev_guard_poison.argtypes = [vp, vp, vp, C.POINTER(i), C.POINTER(sz), C.POINTER(sz)]
        L.ss4k_dev_guard_selftest.argtypes = [vp]
        if hasattr(L, "ss4k_dev_guard_poison_frvsr"):
            L.ss4k_dev_guard_poison_frvsr.argtypes = [vp, vp, C.POINTER(i), C.POINTER(sz), C.POINTER(sz)]
        if hasattr(L, "ss4k_dev_guard_poison_temporal"):
            L.ss4k_dev_guard_poison_temporal.argtypes = [vp, C.POINTER(i), C.POINTER(sz), C.POINTER(sz)]
    if hasattr(L, "ss4k_dev_lane_counts"):  # dev library only: stream ordering
        i64p = C.POINTER(C.c_int64)
        L.ss4k_dev_op_spin.argtypes = [vp, C.c_uint, vp]
        L.ss4k_dev_lane_handicap.argtypes = [vp, i, C.c_uint]
        L.ss4k_dev_lane_counts.argtypes = [vp, i64p, i64p, i64p]
        L.ss4k_dev_lane_counts_reset.argtypes = [vp]
        L.ss4k_dev_lane_drop_join.argtypes = [vp, i]
    L.ss4k_prof_enable.argtypes = [vp, i]
    L.ss4k_prof_reset.argtypes = [vp]
    L.ss4k_prof_read.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    if hasattr(L, "ss4k_prof_read_kind"):
        L.ss4k_prof_read_kind.argtypes = [vp, i, C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    if hasattr(L, "ss4k_prof_read_family"):
        L.ss4k_prof_read_family.argtypes = [vp, i, C.c_char_p, sz, C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.ss4k_prof_read_section_ms.argtypes = [vp, C.POINTER(C.c_double)]
    L.ss4k_stream_pair_check.argtypes = [vp, vp, vp, C.POINTER(C.c_int)]
    L.ss4k_op_cv_area_shape.argtypes = [i, i, C.c_double, C.c_double, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.ss4k_op_cv_area_resize_u8.argtypes = [vp, vp, vp, sz, i, i, i, i, C.c_double, C.c_double, vp]
    if hasattr(L, "ss4k_frvsr_create"):   # (absent from older builds, which tools/lib_ab.py loads for A/B timing)
        L.ss4k_frvsr_param_count.argtypes = [C.POINTER(FrvsrDesc)]; L.ss4k_frvsr_param_count.restype = sz
        L.ss4k_frvsr_create.argtypes = [vp, C.POINTER(FrvsrDesc), vp, sz, C.POINTER(vp)]
        L.ss4k_frvsr_destroy.argtypes = [vp]; L.ss4k_frvsr_destroy.restype = None
        L.ss4k_frvsr_step.argtypes = [vp, vp, vp, vp, vp, i, i, i, vp]
        L.ss4k_frvsr_workspace_bytes.argtypes = [vp, i, i, i, C.POINTER(C.c_size_t)]
        L.ss4k_frvsr_prof_enable.argtypes = [vp, i]
        L.ss4k_frvsr_prof_read.argtypes = [vp, i, C.POINTER(C.c_double)]
        L.ss4k_frvsr_upscaler_create.argtypes = [vp, vp, i, i, i, i, C.POINTER(vp)]
        L.ss4k_frvsr_upscaler_destroy.argtypes = [vp]; L.ss4k_frvsr_upscaler_destroy.restype = None
        L.ss4k_frvsr_upscaler_reset.argtypes = [vp]
        L.ss4k_frvsr_upscaler_out_shape.argtypes = [vp, C.POINTER(i), C.POINTER(i)]
        L.ss4k_frvsr_upscale_frames.argtypes = [vp, vp, i, i, i, vp, sz, vp]
        L.ss4k_frvsr_upscaler_enable_taps.argtypes = [vp, i]
        L.ss4k_frvsr_upscaler_read_tap.argtypes = [vp, i, vp, sz, C.POINTER(i * 4), vp]
        L.ss4k_op_backward_warp.argtypes = [vp, vp, vp, vp, i, i, i, i, vp]
        L.ss4k_op_bicubic_upsample4.argtypes = [vp, vp, vp, i, i, i, vp]
    if hasattr(L, "ss4k_frvsr_upscale_streams"):   # (absent from builds before the stream slots)
        L.ss4k_frvsr_upscaler_create_streams.argtypes = [vp, vp, i, i, i, i, i, C.POINTER(vp)]
        L.ss4k_frvsr_upscale_streams.argtypes = [vp, C.POINTER(C.c_int32), i, vp, i, i, vp, sz, vp]
        L.ss4k_frvsr_upscaler_reset_stream.argtypes = [vp, i]
        L.ss4k_frvsr_upscaler_state_bytes.argtypes = [vp, C.POINTER(C.c_size_t)]
    if hasattr(L, "ss4k_frvsr_upscale_streams_at"):   # (absent from builds before the scattered rounds)
        L.ss4k_frvsr_upscale_streams_at.argtypes = [vp, C.POINTER(C.c_int32), i, C.POINTER(vp), i, i, C.POINTER(vp), sz, vp]
    if hasattr(L, "ss4k_frvsr_create_as"):   # (absent from builds before the second generator)
        L.ss4k_frvsr_param_count_as.argtypes = [C.POINTER(FrvsrDesc), i]; L.ss4k_frvsr_param_count_as.restype = sz
        L.ss4k_frvsr_create_as.argtypes = [vp, C.POINTER(FrvsrDesc), i, i, vp, sz, C.POINTER(vp)]
        L.ss4k_frvsr_generator.argtypes = [vp]
    if hasattr(L, "ss4k_frvsr_create_ex"):   # (absent from builds before degradation 'BI')
        L.ss4k_frvsr_param_count_ex.argtypes = [C.POINTER(FrvsrDesc), i, i]; L.ss4k_frvsr_param_count_ex.restype = sz
        L.ss4k_frvsr_create_ex.argtypes = [vp, C.POINTER(FrvsrDesc), i, i, i, vp, sz, C.POINTER(vp)]
        L.ss4k_frvsr_degradation.argtypes = [vp]
    if hasattr(L, "ss4k_frvsr_upscaler_set_scene_cut"):   # (absent from builds before the scene-cut detector)
        L.ss4k_frvsr_upscaler_set_scene_cut.argtypes = [vp, C.c_double]
        L.ss4k_frvsr_upscaler_scene_cut.argtypes = [vp, C.POINTER(C.c_double)]
        L.ss4k_frvsr_upscaler_scene_cut_stats.argtypes = [vp, i, C.POINTER(SceneCutStats), vp]
        L.ss4k_frvsr_upscaler_scene_cut_total.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.ss4k_op_frame_sad_u8.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), i, sz, vp, vp]
    if hasattr(L, "ss4k_bsvd_online_create"):   # (absent from builds before the online denoiser)
        L.ss4k_bsvd_online_create.argtypes = [vp, vp, i, C.POINTER(vp)]
        L.ss4k_bsvd_online_destroy.argtypes = [vp]; L.ss4k_bsvd_online_destroy.restype = None
        L.ss4k_bsvd_online_lag.argtypes = [vp]
        L.ss4k_bsvd_online_push.argtypes = [vp, vp, i, i, i, vp, sz, C.POINTER(i), vp]
        L.ss4k_bsvd_online_flush.argtypes = [vp, vp, sz, C.POINTER(i), vp]
        L.ss4k_bsvd_online_reset.argtypes = [vp]
        L.ss4k_bsvd_online_pending.argtypes = [vp, C.POINTER(i)]
        L.ss4k_bsvd_online_state_bytes.argtypes = [vp, C.POINTER(sz)]
    if hasattr(L, "ss4k_upscaler_temporal_create"):
        L.ss4k_upscaler_temporal_create.argtypes = [vp, C.POINTER(UpscaleCfg), vp, vp, i, C.POINTER(vp)]
        L.ss4k_upscaler_temporal_destroy.argtypes = [vp]; L.ss4k_upscaler_temporal_destroy.restype = None
        L.ss4k_upscale_frames_temporal.argtypes = [vp, vp, i, i, i, vp, sz, C.POINTER(i), vp]
        L.ss4k_upscaler_temporal_flush.argtypes = [vp, vp, sz, C.POINTER(i), vp]
        L.ss4k_upscaler_temporal_reset.argtypes = [vp]
        L.ss4k_upscaler_temporal_out_shape.argtypes = [vp, i, i, C.POINTER(i), C.POINTER(i)]
        L.ss4k_upscaler_temporal_pending.argtypes = [vp, C.POINTER(i)]
        L.ss4k_upscaler_temporal_state_bytes.argtypes = [vp, C.POINTER(sz)]
    if hasattr(L, "ss4k_bsvd_online_push_cuts"):   # (absent from builds before the temporal stream's scene cuts)
        L.ss4k_bsvd_online_push_cuts.argtypes = [vp, vp, vp, i, i, i, vp, sz, C.POINTER(i), vp]
        L.ss4k_upscaler_temporal_set_scene_cut.argtypes = [vp, C.c_double]
        L.ss4k_upscaler_temporal_scene_cut.argtypes = [vp, C.POINTER(C.c_double)]
        L.ss4k_upscaler_temporal_scene_cut_stats.argtypes = [vp, C.POINTER(SceneCutStats), vp]
        L.ss4k_upscaler_temporal_scene_cut_total.argtypes = [vp, C.POINTER(C.c_uint64)]
    if hasattr(L, "ss4k_upscale_round_temporal"):
        ip = C.POINTER(i)
        L.ss4k_upscaler_temporal_create_streams.argtypes = [vp, C.POINTER(UpscaleCfg), vp, vp, i, i, C.POINTER(vp)]
        L.ss4k_upscale_round_temporal.argtypes = [vp, C.POINTER(vp), ip, i, i, i, vp, sz, ip, ip, ip, vp]
        L.ss4k_upscaler_temporal_flush_stream.argtypes = [vp, i, vp, sz, ip, vp]
        L.ss4k_upscaler_temporal_reset_stream.argtypes = [vp, i]
        L.ss4k_upscaler_temporal_pending_stream.argtypes = [vp, i, ip]
        L.ss4k_upscaler_temporal_scene_cut_stats_stream.argtypes = [vp, i, C.POINTER(SceneCutStats), vp]
        L.ss4k_upscaler_temporal_stream_state_bytes_for.argtypes = [vp, C.POINTER(sz)]
        L.ss4k_upscaler_temporal_release_idle.argtypes = [vp]
    if hasattr(L, "ss4k_upscaler_temporal_set_denoise_rate_stream"):   # (absent from builds before the per-slot rate)
        L.ss4k_upscaler_temporal_set_denoise_rate_stream.argtypes = [vp, i, C.c_float]
    if hasattr(L, "ss4k_frvsr_temporal_create"):   # (absent from builds before the denoiser in front of the frame-recurrent chain)
        ip = C.POINTER(i)
        L.ss4k_frvsr_temporal_create.argtypes = [vp, vp, vp, i, i, i, i, C.c_double, i, i, C.POINTER(vp)]
        L.ss4k_frvsr_temporal_destroy.argtypes = [vp]; L.ss4k_frvsr_temporal_destroy.restype = None
        L.ss4k_frvsr_temporal_round.argtypes = [vp, C.POINTER(vp), ip, i, i, i, vp, sz, ip, ip, ip, vp]
        L.ss4k_frvsr_temporal_flush_stream.argtypes = [vp, i, vp, sz, ip, vp]
        L.ss4k_frvsr_temporal_reset_stream.argtypes = [vp, i]
        L.ss4k_frvsr_temporal_pending_stream.argtypes = [vp, i, ip]
        L.ss4k_frvsr_temporal_set_denoise_rate_stream.argtypes = [vp, i, C.c_float]
        L.ss4k_frvsr_temporal_out_shape.argtypes = [vp, ip, ip]
        L.ss4k_frvsr_temporal_state_bytes.argtypes = [vp, C.POINTER(sz)]
        L.ss4k_frvsr_temporal_stream_state_bytes_for.argtypes = [vp, C.POINTER(sz)]
        L.ss4k_frvsr_temporal_release_idle.argtypes = [vp]
    if hasattr(L, "ss4k_frvsr_temporal_set_scene_cut"):   # (absent from builds before that chain's scene cuts)
        L.ss4k_frvsr_temporal_set_scene_cut.argtypes = [vp, C.c_double]
        L.ss4k_frvsr_temporal_scene_cut.argtypes = [vp, C.POINTER(C.c_double)]
        L.ss4k_frvsr_temporal_scene_cut_stats_stream.argtypes = [vp, i, C.POINTER(SceneCutStats), vp]
        L.ss4k_frvsr_temporal_scene_cut_total.argtypes = [vp, C.POINTER(C.c_uint64)]
    if hasattr(L, "ss4k_frvsr_temporal_create_padded"):   # (absent from builds before the padded form)
        L.ss4k_frvsr_temporal_create_padded.argtypes = [vp, vp, vp, i, i, i, i, C.c_double, i, i, C.POINTER(vp)]
    if hasattr(L, "ss4k_upscaler_temporal_set_noise_map"):   # (absent from builds before the motion map)
        L.ss4k_upscaler_temporal_set_noise_map.argtypes = [vp, i]
        L.ss4k_upscaler_temporal_noise_map.argtypes = [vp, C.POINTER(i)]
        L.ss4k_frvsr_temporal_set_noise_map.argtypes = [vp, i]
        L.ss4k_frvsr_temporal_noise_map.argtypes = [vp, C.POINTER(i)]
    if hasattr(L, "ss4k_dev_op_temporal_gather_motion"):   # dev library only
        for f in (L.ss4k_dev_op_temporal_gather_motion, L.ss4k_dev_op_temporal_gather_motion_pad):
            f.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), i, i, i, C.c_uint64, C.c_float, C.POINTER(C.c_float), vp, vp]
        L.ss4k_dev_temporal_motion_tile.argtypes = [C.POINTER(i), C.POINTER(i)]
        L.ss4k_dev_temporal_motion_taps.argtypes = [C.POINTER(C.c_float)]
    if hasattr(L, "ss4k_dev_op_temporal_gather_pad"):   # dev library only
        L.ss4k_dev_op_temporal_gather_pad.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), i, i, i, C.c_uint64, C.c_float, C.POINTER(C.c_float), vp, vp]
        L.ss4k_dev_op_frvsrt_denoised_in_crop.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), i, i, i, i, i, vp, vp]
    if hasattr(L, "ss4k_dev_op_frvsrt_clear_flagged"):   # dev library only
        L.ss4k_dev_op_frvsrt_clear_flagged.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), i, sz, sz, vp]
    if hasattr(L, "ss4k_dev_op_frvsrt_denoised_in"):   # dev library only
        L.ss4k_dev_op_frvsrt_denoised_in.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), i, i, i, vp, vp]
        L.ss4k_dev_guard_poison_frvsr_temporal.argtypes = [vp, C.POINTER(i), C.POINTER(sz), C.POINTER(sz)]
    if hasattr(L, "ss4k_dev_op_temporal_gather"):   # dev library only
        L.ss4k_dev_op_temporal_gather.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), i, sz, i, C.c_uint64, C.c_float, C.c_float, vp, vp]
    if hasattr(L, "ss4k_dev_op_temporal_gather_levels"):   # dev library only
        L.ss4k_dev_op_temporal_gather_levels.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), i, sz, i, C.c_uint64, C.c_float, C.POINTER(C.c_float), vp, vp]
    if hasattr(L, "ss4k_dev_op_bsvd_online_shift_cuts"):   # dev library only
        L.ss4k_dev_op_bsvd_online_shift_cuts.argtypes = [vp, vp, vp, i, i, i, i, sz, i, i, i, i, i, vp, C.c_uint, i, vp]
        L.ss4k_dev_op_bsvd_noise_planes.argtypes = [vp, vp, i, sz, vp, i, C.c_float, C.c_float, vp]
    if hasattr(L, "ss4k_dev_op_bsvd_online_shift"):   # dev library only
        ip, szp = C.POINTER(i), C.POINTER(sz)
        L.ss4k_dev_op_bsvd_online_shift.argtypes = [vp, vp, vp, i, i, i, i, sz, i, i, i, i, i, vp]
        L.ss4k_dev_op_bsvd_online_carry.argtypes = [vp, i, C.POINTER(vp), C.POINTER(vp), ip, ip, ip, ip, ip, szp, vp]
    if hasattr(L, "ss4k_dev_frvsr_tail_taps"):
        L.ss4k_dev_frvsr_tail_taps.argtypes = [vp, vp, vp, vp, vp, vp, i, i, i, i, i, vp]
        L.ss4k_dev_frvsr_embed_convt.argtypes = [vp, i, vp, sz]
        L.ss4k_dev_frvsr_pack_convt.argtypes = [vp, i, vp, sz]
    return L


def glue_routes(L: C.CDLL) -> dict:
    """{route name: launches} of the dev library's glue launchers since the last ``L.ss4k_dev_glue_routes_reset()``."""
    out, idx = {}, 0
    while True:
        name, n = C.create_string_buffer(256), C.c_int64()
        if L.ss4k_dev_glue_routes_read(idx, name, 256, C.byref(n)) != 0:
            return out
        out[name.value.decode()] = n.value
        idx += 1


def _guard_lib(L: Optional[C.CDLL]) -> C.CDLL:
    L = L or lib()
    if not hasattr(L, "ss4k_dev_guard_check"):
        raise Ss4kError("guard mode lives in libss4k_hip_dev.so: run with SS4K_LIB=<package>/libss4k_hip_dev.so")
    return L


def _guard_rc(L: C.CDLL, rc: int) -> None:
    if rc != 0:
        raise Ss4kError(f"libss4k_hip_dev error {rc}: {L.ss4k_last_error().decode()}")


def guard_enable(on: bool = True, L: Optional[C.CDLL] = None) -> None:
    """Guard mode of the dev library (include/ss4k_dev.h): red zones and 0xFF poison for every LATER device allocation of the library."""
    L = _guard_lib(L)
    _guard_rc(L, L.ss4k_dev_guard_enable(int(on)))


def guard_check(L: Optional[C.CDLL] = None) -> Tuple[int, int, int, str]:
    """(guarded live buffers, unguarded live buffers, damaged red zones, text of the first damage); synchronises the device."""
    L = _guard_lib(L)
    g, u, d, text = C.c_int(), C.c_int(), C.c_int(), C.create_string_buffer(512)
    _guard_rc(L, L.ss4k_dev_guard_check(C.byref(g), C.byref(u), C.byref(d), text, 512))
    return g.value, u.value, d.value, text.value.decode()


def guard_poison(ctx=None, model=None, upscaler=None, L: Optional[C.CDLL] = None) -> Tuple[int, int, int]:
    """0xFF into the transient buffers of the objects given (handles or the wrappers of this module): (buffers, bytes, bytes rounded
    up to 256 per buffer)."""
    L = _guard_lib(L)
    h = [getattr(o, "_h", o) for o in (ctx, model, upscaler)]
    n, b, b256 = C.c_int(), C.c_size_t(), C.c_size_t()
    _guard_rc(L, L.ss4k_dev_guard_poison(*h, C.byref(n), C.byref(b), C.byref(b256)))
    return n.value, int(b.value), int(b256.value)


def guard_poison_frvsr(model=None, upscaler=None, L: Optional[C.CDLL] = None) -> Tuple[int, int, int]:
    """``guard_poison`` for a ``Frvsr`` and / or a ``FrvsrUpscaler``; the recurrent state is left alone."""
    L = _guard_lib(L)
    h = [getattr(o, "_h", o) for o in (model, upscaler)]
    n, b, b256 = C.c_int(), C.c_size_t(), C.c_size_t()
    _guard_rc(L, L.ss4k_dev_guard_poison_frvsr(*h, C.byref(n), C.byref(b), C.byref(b256)))
    return n.value, int(b.value), int(b256.value)


def guard_poison_temporal(upscaler, L: Optional[C.CDLL] = None) -> Tuple[int, int, int]:
    """``guard_poison`` for a ``TemporalUpscaler``: the chain's intermediates and the job buffers its slots share; every slot's state is left alone."""
    L = _guard_lib(L)
    n, b, b256 = C.c_int(), C.c_size_t(), C.c_size_t()
    _guard_rc(L, L.ss4k_dev_guard_poison_temporal(getattr(upscaler, "_h", upscaler), C.byref(n), C.byref(b), C.byref(b256)))
    return n.value, int(b.value), int(b256.value)


def guard_poison_frvsr_temporal(upscaler, L: Optional[C.CDLL] = None) -> Tuple[int, int, int]:
    """``guard_poison`` for a ``TemporalFrvsrUpscaler``: the job buffers its slots share; every slot's state is left alone."""
    L = _guard_lib(L)
    n, b, b256 = C.c_int(), C.c_size_t(), C.c_size_t()
    _guard_rc(L, L.ss4k_dev_guard_poison_frvsr_temporal(getattr(upscaler, "_h", upscaler), C.byref(n), C.byref(b), C.byref(b256)))
    return n.value, int(b.value), int(b256.value)


def guard_selftest(ctx, L: Optional[C.CDLL] = None) -> None:
    """The guard's positive control (one legal byte written into each red zone of a buffer of its own must be reported); raises if not."""
    L = _guard_lib(L)
    _guard_rc(L, L.ss4k_dev_guard_selftest(getattr(ctx, "_h", ctx)))


def _check(rc: int) -> None:
    if rc != 0:
        raise Ss4kError(f"libss4k_hip error {rc}: {lib().ss4k_last_error().decode()}")


def _stream() -> int:
    return int(torch.cuda.current_stream().cuda_stream)


def _dev_index(device) -> int:
    d = torch.device(device if not isinstance(device, int) else f"cuda:{device}")
    return d.index if d.index is not None else torch.cuda.current_device()


class Context:
    """One per GPU (include/ss4k.h: ss4k_ctx)."""

    def __init__(self, device=0):
        self.device_index = _dev_index(device)
        self.device = torch.device("cuda", self.device_index)
        h = C.c_void_p()
        global GPU_TOUCHED
        rc = lib().ss4k_ctx_create(self.device_index, C.byref(h))
        # (a box without any GPU has no runtime to initialise: the failed attempt leaves the process as fork-safe as it was)
        GPU_TOUCHED = GPU_TOUCHED or rc == 0 or torch.cuda.device_count() > 0
        _check(rc)
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().ss4k_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- profiling hooks (bench.py roofline leg)
    def prof_enable(self, on: bool):
        _check(lib().ss4k_prof_enable(self._h, int(on)))

    def prof_reset(self):
        _check(lib().ss4k_prof_reset(self._h))

    def prof_read(self) -> Tuple[int, float, float]:
        n, ms, fl = C.c_int64(), C.c_double(), C.c_double()
        _check(lib().ss4k_prof_read(self._h, C.byref(n), C.byref(ms), C.byref(fl)))
        return n.value, ms.value, fl.value

    def prof_read_kind(self, kind: int) -> Tuple[int, float, float]:
        """(launches, total ms, algorithmic FLOPs) of one kernel family: 0 conv, 1 / 2 / 3 FSRCNN head / mapping / tail."""
        n, ms, fl = C.c_int64(), C.c_double(), C.c_double()
        _check(lib().ss4k_prof_read_kind(self._h, kind, C.byref(n), C.byref(ms), C.byref(fl)))
        return n.value, ms.value, fl.value

    def prof_read_families(self):
        """[(kernel build, launches, total ms, algorithmic FLOPs)] of the conv launches since the last reset."""
        out, idx = [], 0
        while True:
            name, n, ms, fl = C.create_string_buffer(256), C.c_int64(), C.c_double(), C.c_double()
            if lib().ss4k_prof_read_family(self._h, idx, name, 256, C.byref(n), C.byref(ms), C.byref(fl)) != 0:
                return out
            out.append((name.value.decode(), n.value, ms.value, fl.value))
            idx += 1

    def streams_side_by_side(self, a, b) -> bool:
        """Measured (~ 3 ms, synchronises both): do the torch streams `a` and `b` run beside each other at full launch rate?"""
        ok = C.c_int()
        _check(lib().ss4k_stream_pair_check(self._h, int(a.cuda_stream), int(b.cuda_stream), C.byref(ok)))
        return bool(ok.value)

    def prof_read_section_ms(self) -> float:
        """Wall time of the profiled forwards' conv sections (first conv launch to the end of the last, caller's stream)."""
        ms = C.c_double()
        _check(lib().ss4k_prof_read_section_ms(self._h, C.byref(ms)))
        return ms.value

    def bench_conv(self, dtype, cin0, cin1, cout, n, h, w, flags=0, iters=20) -> float:
        if not hasattr(lib(), "ss4k_bench_conv"):
            raise Ss4kError("ss4k_bench_conv lives in libss4k_hip_dev.so: run with SS4K_LIB=<package>/libss4k_hip_dev.so")
        us = C.c_double()
        _check(lib().ss4k_bench_conv(self._h, dtype, cin0, cin1, cout, n, h, w, flags, iters, C.byref(us), _stream()))
        return us.value

    # -- granular ops (tests)
    def _f32(self, t):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
        return t

    def u8nhwc_to_f32nchw(self, x: torch.Tensor) -> torch.Tensor:
        assert x.is_cuda and x.dtype == torch.uint8 and x.is_contiguous() and x.ndim == 4
        n, h, w, c = x.shape
        out = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
        _check(lib().ss4k_op_u8nhwc_to_f32nchw(self._h, x.data_ptr(), out.data_ptr(), n, h, w, c, _stream()))
        return out

    def _resize(self, fn, x, size):
        self._f32(x)
        n, c, h, w = x.shape
        out = torch.empty((n, c, size[0], size[1]), dtype=torch.float32, device=x.device)
        _check(fn(self._h, x.data_ptr(), out.data_ptr(), n * c, h, w, size[0], size[1], _stream()))
        return out

    def area_resize(self, x, size):
        return self._resize(lib().ss4k_op_area_resize, x, size)

    def bicubic_resize(self, x, size):
        return self._resize(lib().ss4k_op_bicubic_resize, x, size)

    def cv_area_resize(self, frames: torch.Tensor, fx: float, fy: Optional[float] = None) -> torch.Tensor:
        """``cv2.resize(frame, None, fx=fx, fy=fy, interpolation=cv2.INTER_AREA)`` of every frame of a uint8 NHWC device tensor (shrinking,
        non-integer 1 / f: the image server's pre / post scale, image_pipeline.py:272-273,347-348) -> uint8 NHWC."""
        assert frames.is_cuda and frames.dtype == torch.uint8 and frames.is_contiguous() and frames.ndim == 4
        fy = fx if fy is None else fy
        n, h, w, c = frames.shape
        oh, ow = C.c_int(), C.c_int()
        _check(lib().ss4k_op_cv_area_shape(h, w, fx, fy, C.byref(oh), C.byref(ow)))
        out = torch.empty((n, oh.value, ow.value, c), dtype=torch.uint8, device=frames.device)
        _check(lib().ss4k_op_cv_area_resize_u8(self._h, frames.data_ptr(), out.data_ptr(), out.numel(), n, h, w, c, fx, fy, _stream()))
        return out

    def bilinear_resize(self, x, size):
        return self._resize(lib().ss4k_op_bilinear_resize, x, size)

    def depthwise_reflect(self, x, k2d: np.ndarray):
        self._f32(x)
        n, c, h, w = x.shape
        k = np.ascontiguousarray(k2d, dtype=np.float32)
        out = torch.empty_like(x)
        _check(lib().ss4k_op_depthwise_reflect(self._h, x.data_ptr(), out.data_ptr(), n * c, h, w,
                                               k.ctypes.data_as(C.c_void_p), k.shape[0], _stream()))
        torch.cuda.current_stream().synchronize()  # k lives on the host until the copy is done
        return out

    def plane_stats(self, x):
        self._f32(x)
        n, c, h, w = x.shape
        out = torch.empty((n, c, 2), dtype=torch.float32, device=x.device)
        _check(lib().ss4k_op_plane_stats(self._h, x.data_ptr(), out.data_ptr(), n * c, h * w, _stream()))
        return out

    def backward_warp(self, x, flow):
        """``backward_warp(x, flow)`` (utils/net_utils.py:50-93): x (n, c, h, w), flow (n, 2, h, w)."""
        self._f32(x); self._f32(flow)
        n, c, h, w = x.shape
        assert tuple(flow.shape) == (n, 2, h, w)
        out = torch.empty_like(x)
        _check(lib().ss4k_op_backward_warp(self._h, x.data_ptr(), flow.data_ptr(), out.data_ptr(), n, c, h, w, _stream()))
        return out

    def bicubic_upsample4(self, x):
        """``BicubicUpsample(4)(x)`` (utils/net_utils.py:112-165)."""
        self._f32(x)
        n, c, h, w = x.shape
        out = torch.empty((n, c, 4 * h, 4 * w), dtype=torch.float32, device=x.device)
        _check(lib().ss4k_op_bicubic_upsample4(self._h, x.data_ptr(), out.data_ptr(), n * c, h, w, _stream()))
        return out

    def frame_sad(self, a_frames, b_frames) -> torch.Tensor:
        """``sum |a_frames[i] - b_frames[i]|`` over the bytes of each pair of uint8 device frames (1..64 pairs of one size, each contiguous, at
        any byte address): an int64 tensor of the exact sums on the device (ss4k_op_frame_sad_u8, the scene-cut detector's kernel)."""
        n = len(a_frames)
        assert n >= 1 and len(b_frames) == n, "one b frame per a frame"
        nbytes = int(a_frames[0].numel())
        for t in list(a_frames) + list(b_frames):
            assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and int(t.numel()) == nbytes, "frames: contiguous uint8 of one size"
        out = torch.empty((n,), dtype=torch.int64, device=a_frames[0].device)
        pa = (C.c_void_p * n)(*[t.data_ptr() for t in a_frames])
        pb = (C.c_void_p * n)(*[t.data_ptr() for t in b_frames])
        with torch.cuda.device(self.device):
            _check(lib().ss4k_op_frame_sad_u8(self._h, pa, pb, n, nbytes, out.data_ptr(), _stream()))
        return out

    def f32nchw_to_u8nhwc(self, x):
        self._f32(x)
        n, c, h, w = x.shape
        out = torch.empty((n, h, w, c), dtype=torch.uint8, device=x.device)
        _check(lib().ss4k_op_f32nchw_to_u8nhwc(self._h, x.data_ptr(), out.data_ptr(), n, c, h, w, _stream()))
        return out


def make_desc(kind: int, dtype: int = F32, scale: int = 2, num_feat: int = 64, num_block: int = 23,
              num_grow_ch: int = 32, bsvd_chns: Sequence[int] = (32, 64, 128), bsvd_mid_ch: int = 32,
              bsvd_interm_ch: int = 30, bsvd_stream: bool = False, flags: int = 0) -> ModelDesc:
    d = ModelDesc()
    d.kind, d.dtype, d.scale, d.num_feat, d.num_block, d.num_grow_ch = kind, dtype, scale, num_feat, num_block, num_grow_ch
    d.bsvd_chns = (C.c_int32 * 3)(*bsvd_chns)
    d.bsvd_mid_ch, d.bsvd_interm_ch = bsvd_mid_ch, bsvd_interm_ch
    d.bsvd_stream = 1 if bsvd_stream else 0
    d.flags = int(flags)
    return d


def param_count(desc: ModelDesc) -> int:
    return int(lib().ss4k_model_param_count(C.byref(desc)))


class Model:
    """A network resident on one GPU; callable like the reference's ``self.model`` (NCHW float in/out)."""

    def __init__(self, ctx: Context, desc: ModelDesc, flat_weights: np.ndarray):
        self.ctx, self.desc = ctx, desc
        w = np.ascontiguousarray(flat_weights, dtype=np.float32)
        h = C.c_void_p()
        with torch.cuda.device(ctx.device):
            _check(lib().ss4k_model_create(ctx._h, C.byref(desc), w.ctypes.data_as(C.c_void_p), w.size, C.byref(h)))
        self._h = h
        self.in_channels = lib().ss4k_model_in_channels(h)

    def close(self):
        if getattr(self, "_h", None):
            lib().ss4k_model_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, wait: bool = True) -> None:
        """Raise if an earlier forward of this model failed asynchronously (ss4k_model_check; no kernel can any more: always passes)."""
        _check(lib().ss4k_model_check(self._h, 1 if wait else 0))

    def workspace_bytes(self, n, h, w) -> int:
        b = C.c_size_t()
        _check(lib().ss4k_model_workspace_bytes(self._h, n, h, w, C.byref(b)))
        return int(b.value)

    def out_shape(self, n, h, w):
        oc, oh, ow = C.c_int(), C.c_int(), C.c_int()
        _check(lib().ss4k_model_out_shape(self._h, n, h, w, C.byref(oc), C.byref(oh), C.byref(ow)))
        return oc.value, oh.value, ow.value

    def __call__(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``out``: a caller-owned float32 device tensor of the output's shape to write into (tests place it between red zones)."""
        squeeze_f = False
        seq_shape = None
        if x.ndim == 5:  # BSVD's (N, F, C, H, W)
            if self.desc.bsvd_stream:  # BSVD.forward flattens N*F into one stream (bsvd/model.py:520-522)
                seq_shape = x.shape[:2]
                x = x.reshape((-1,) + tuple(x.shape[2:]))
            else:
                assert x.shape[1] == 1, "per-frame BSVD takes F = 1 (fsrcnn_upscaler.py:277); build it with stream=True for F > 1"
                x = x[:, 0]
                squeeze_f = True
        assert x.ndim == 4 and x.shape[1] == self.in_channels, f"expected (N,{self.in_channels},H,W), got {tuple(x.shape)}"
        x = x.to(device=self.ctx.device, dtype=torch.float32).contiguous()
        n, _, h, w = x.shape
        oc, oh, ow = self.out_shape(n, h, w)
        if out is None:
            out = torch.empty((n, oc, oh, ow), dtype=torch.float32, device=x.device)
        else:
            assert out.is_cuda and out.device == x.device and out.dtype == torch.float32 and out.is_contiguous() and \
                out.numel() == n * oc * oh * ow, f"out: expected {n * oc * oh * ow} contiguous float32 elements on {x.device}"
            out = out.view(n, oc, oh, ow)
        with torch.cuda.device(self.ctx.device):
            _check(lib().ss4k_model_forward(self._h, x.data_ptr(), out.data_ptr(), n, h, w, _stream()))
        if seq_shape is not None:
            return out.reshape(tuple(seq_shape) + tuple(out.shape[1:]))
        return out.unsqueeze(1) if squeeze_f else out

    forward = __call__

    def eval(self):
        return self


class Upscaler:
    """ss4k_upscaler: the frame-in/frame-out path (uint8 NHWC -> uint8 NHWC)."""

    def __init__(self, ctx: Context, sr: Model, lr_shape, output_shape=None, lr_hr_resize=True, single_mode=False,
                 denoise: Optional[Model] = None, denoise_rate: float = 1.0):
        self.ctx, self.sr, self.denoise = ctx, sr, denoise
        cfg = UpscaleCfg()
        cfg.lr_h, cfg.lr_w = int(lr_shape[0]), int(lr_shape[1])
        cfg.out_h, cfg.out_w = (0, 0) if output_shape is None else (int(output_shape[0]), int(output_shape[1]))
        cfg.lr_hr_resize, cfg.single_mode = int(bool(lr_hr_resize)), int(bool(single_mode))
        cfg.sr_is_realesrgan = int(sr.in_channels == 3)
        cfg.denoising, cfg.denoise_rate = int(denoise is not None), float(denoise_rate)
        h = C.c_void_p()
        _check(lib().ss4k_upscaler_create(ctx._h, C.byref(cfg), sr._h, denoise._h if denoise is not None else None,
                                          C.byref(h)))
        self._h, self.cfg = h, cfg

    def close(self):
        if getattr(self, "_h", None):
            lib().ss4k_upscaler_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        _check(lib().ss4k_upscaler_reset(self._h))

    def last_enqueue_ms(self):
        """(denoise_ms, model_ms): host time the last job spent enqueueing those stages."""
        d, m = C.c_double(), C.c_double()
        _check(lib().ss4k_upscaler_last_enqueue_ms(self._h, C.byref(d), C.byref(m)))
        return d.value, m.value

    def out_shape(self, n, h, w):
        oh, ow = C.c_int(), C.c_int()
        _check(lib().ss4k_upscaler_out_shape(self._h, n, h, w, C.byref(oh), C.byref(ow)))
        return oh.value, ow.value

    def enable_taps(self, on=True):
        _check(lib().ss4k_upscaler_enable_taps(self._h, int(on)))

    def read_tap(self, which: int) -> torch.Tensor:
        dims = (C.c_int * 4)()
        _check(lib().ss4k_upscaler_read_tap(self._h, which, None, 0, C.byref(dims), _stream()))
        out = torch.empty(tuple(dims), dtype=torch.float32, device=self.ctx.device)
        _check(lib().ss4k_upscaler_read_tap(self._h, which, out.data_ptr(), out.numel(), C.byref(dims), _stream()))
        return out

    def __call__(self, frames: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        assert frames.is_cuda and frames.dtype == torch.uint8 and frames.ndim == 4 and frames.shape[-1] == 3
        frames = frames.contiguous()
        n, h, w, _ = frames.shape
        oh, ow = self.out_shape(n, h, w)
        if out is None:
            out = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device=frames.device)
        with torch.cuda.device(self.ctx.device):
            _check(lib().ss4k_upscale_frames(self._h, frames.data_ptr(), n, h, w, out.data_ptr(), out.numel(), _stream()))
        return out


class BsvdOnline:
    """ss4k_bsvd_online: BSVD as the reference's online machine (``BSVD.feedin_one_element``, bsvd/model.py:510-513).  ``model`` is a BSVD
    ``Model`` built with ``bsvd_stream=True``; it is held, not owned.  The frames of a stream, however the pushes cut it, are bit for bit
    those of ``model`` on the whole stream as one clip."""

    def __init__(self, model: Model, max_push: int = 4, L: Optional[C.CDLL] = None):
        self.model, self.ctx, self.max_push, self._L = model, model.ctx, int(max_push), L or lib()
        self._shape = None
        h = C.c_void_p()
        self._rc(self._L.ss4k_bsvd_online_create(self.ctx._h, model._h, self.max_push, C.byref(h)))
        self._h = h
        self.lag = int(self._L.ss4k_bsvd_online_lag(h))

    def _rc(self, rc: int) -> None:   # (the error text lives in the library that made it: the product's, or a dev build given as L)
        if rc != 0:
            raise Ss4kError(f"libss4k_hip error {rc}: {self._L.ss4k_last_error().decode()}")

    def close(self):
        if getattr(self, "_h", None):
            self._L.ss4k_bsvd_online_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def pending(self) -> int:
        """Frames pushed and not yet returned."""
        k = C.c_int()
        self._rc(self._L.ss4k_bsvd_online_pending(self._h, C.byref(k)))
        return k.value

    def state_bytes(self) -> int:
        b = C.c_size_t()
        self._rc(self._L.ss4k_bsvd_online_state_bytes(self._h, C.byref(b)))
        return int(b.value)

    def push(self, x: torch.Tensor, out: Optional[torch.Tensor] = None, cuts: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``x`` (n, 4, h, w), 1 <= n <= max_push -> the (k, 3, h, w) frames that became ready, oldest first (k = 0 while the lag fills).
        ``out``: a caller-owned contiguous float32 device tensor to write into (its leading dimension is the capacity in frames).
        ``cuts``: an (n,) int32 / uint32 device tensor, element i != 0: frame i is the first of a new scene (ss4k_bsvd_online_push_cuts) -
        the stream is then the concatenation of its scenes run as streams of their own; k is what it is without cuts."""
        assert x.ndim == 4 and x.shape[1] == 4, f"expected (n, 4, h, w), got {tuple(x.shape)}"
        x = x.to(device=self.ctx.device, dtype=torch.float32).contiguous()
        n, _, h, w = x.shape
        if out is None:
            out = torch.empty((n, 3, h, w), dtype=torch.float32, device=x.device)
        k = C.c_int()
        if cuts is not None:
            if not (cuts.is_cuda and cuts.ndim == 1 and cuts.shape[0] == n and cuts.dtype in (torch.int32, getattr(torch, "uint32", torch.int32))):
                raise ValueError(f"cuts must be an ({n},) int32 / uint32 device tensor")
            cuts = cuts.contiguous()
        with torch.cuda.device(self.ctx.device):
            if cuts is not None:
                self._rc(self._L.ss4k_bsvd_online_push_cuts(self._h, x.data_ptr(), cuts.data_ptr(), n, h, w, out.data_ptr(), out.shape[0], C.byref(k), _stream()))
            else:
                self._rc(self._L.ss4k_bsvd_online_push(self._h, x.data_ptr(), n, h, w, out.data_ptr(), out.shape[0], C.byref(k), _stream()))
        self._shape = (h, w)
        return out[:k.value]

    def flush(self) -> torch.Tensor:
        """The frames still inside, oldest first; ends the stream (the next push starts a new one)."""
        left = self.pending
        h, w = self._shape if self._shape else (0, 0)
        out = torch.empty((left, 3, h, w), dtype=torch.float32, device=self.ctx.device)
        k = C.c_int()
        with torch.cuda.device(self.ctx.device):
            self._rc(self._L.ss4k_bsvd_online_flush(self._h, out.data_ptr() if left else None, left, C.byref(k), _stream()))
        self._shape = None
        return out[:k.value]

    def reset(self) -> None:
        self._rc(self._L.ss4k_bsvd_online_reset(self._h))
        self._shape = None


class TemporalUpscaler:
    """ss4k_upscaler_temporal: the per-frame service chain (uint8 NHWC -> uint8 NHWC) with the online BSVD denoiser.  ``denoise`` is a BSVD
    ``Model`` built with ``bsvd_stream=True`` (or a ``BsvdOnline``'s ``.model``).  A call returns the frames that became ready: none during
    the first 16 frames of a stream, as many as went in after."""

    def __init__(self, ctx: Context, sr: Model, denoise: Model, lr_shape, output_shape=None, denoise_rate: float = 1.0, max_push: int = 4,
                 scene_cut: Optional[float] = None, max_streams: int = 1, noise_map: str = "constant"):
        self.ctx, self.sr, self.denoise, self.max_push, self.max_streams = ctx, sr, denoise, int(max_push), int(max_streams)
        mode = noise_map_mode(noise_map)
        cfg = UpscaleCfg()
        cfg.lr_h, cfg.lr_w = int(lr_shape[0]), int(lr_shape[1])
        cfg.out_h, cfg.out_w = (0, 0) if output_shape is None else (int(output_shape[0]), int(output_shape[1]))
        cfg.lr_hr_resize, cfg.single_mode = 1, 1
        cfg.sr_is_realesrgan = int(sr.in_channels == 3)
        cfg.denoising, cfg.denoise_rate = 1, float(denoise_rate)
        h = C.c_void_p()
        if self.max_streams == 1:
            _check(lib().ss4k_upscaler_temporal_create(ctx._h, C.byref(cfg), sr._h, denoise._h, self.max_push, C.byref(h)))
        else:   # several streams on this object: slots, served in rounds (``round``)
            _check(lib().ss4k_upscaler_temporal_create_streams(ctx._h, C.byref(cfg), sr._h, denoise._h, self.max_push, self.max_streams, C.byref(h)))
        self._h, self.cfg, self.lag = h, cfg, 16
        try:
            if scene_cut is not None:
                self.set_scene_cut(scene_cut)
            if mode != 0:
                self.set_noise_map(noise_map)
        except Exception:
            self.close()
            raise

    def close(self):
        if getattr(self, "_h", None):
            lib().ss4k_upscaler_temporal_destroy(self._h)
            self._h = None

    def set_noise_map(self, noise_map: str) -> None:
        """The denoiser's fourth input plane (ss4k_upscaler_temporal_set_noise_map): ``'constant'`` - 0.05 for a stream's or scene's first frame,
        0.1 * rate after, the default - or ``'motion'``, the reference's motion-adaptive map from each frame and the one before it in its
        stream.  Refused (``RuntimeError``) while any slot has a running stream; ``ValueError`` for another word."""
        _check(lib().ss4k_upscaler_temporal_set_noise_map(self._h, noise_map_mode(noise_map)))

    def noise_map(self) -> str:
        m = C.c_int()
        _check(lib().ss4k_upscaler_temporal_noise_map(self._h, C.byref(m)))
        return {v: k for k, v in NOISE_MAPS.items()}[int(m.value)]

    def set_scene_cut(self, threshold: float) -> None:
        """Scene-cut detection in front of every job (include/ss4k.h): ``threshold`` is the mean absolute byte difference between consecutive
        input frames, in (0, 255]; 0 turns it off (the default).  A cut keeps the two scenes apart inside the denoiser, on the device: the
        output is that of the scenes run as separate streams, and every job still returns the frames it returns without the detector."""
        with torch.cuda.device(self.ctx.device):
            _check(lib().ss4k_upscaler_temporal_set_scene_cut(self._h, float(threshold)))

    def scene_cut(self) -> float:
        t = C.c_double()
        _check(lib().ss4k_upscaler_temporal_scene_cut(self._h, C.byref(t)))
        return float(t.value)

    def scene_cut_stats(self, slot: int = 0) -> dict:
        """The counters of a slot's stream and its last frame's values: compared, cuts, last_sad, last_score, last_was_cut.  Synchronises."""
        s = SceneCutStats()
        with torch.cuda.device(self.ctx.device):
            if slot == 0:
                _check(lib().ss4k_upscaler_temporal_scene_cut_stats(self._h, C.byref(s), _stream()))
            else:
                _check(lib().ss4k_upscaler_temporal_scene_cut_stats_stream(self._h, int(slot), C.byref(s), _stream()))
        return {"compared": int(s.compared), "cuts": int(s.cuts), "last_sad": int(s.last_sad), "last_score": int(s.last_score),
                "last_was_cut": int(s.last_was_cut)}

    def scene_cut_total(self) -> int:
        """Cuts in the jobs that have completed on the device; never synchronises."""
        n = C.c_uint64()
        _check(lib().ss4k_upscaler_temporal_scene_cut_total(self._h, C.byref(n)))
        return int(n.value)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def out_shape(self, h=None, w=None):
        oh, ow = C.c_int(), C.c_int()
        _check(lib().ss4k_upscaler_temporal_out_shape(self._h, h or self.cfg.lr_h, w or self.cfg.lr_w, C.byref(oh), C.byref(ow)))
        return oh.value, ow.value

    @property
    def pending(self) -> int:
        k = C.c_int()
        _check(lib().ss4k_upscaler_temporal_pending(self._h, C.byref(k)))
        return k.value

    def state_bytes(self) -> int:
        b = C.c_size_t()
        _check(lib().ss4k_upscaler_temporal_state_bytes(self._h, C.byref(b)))
        return int(b.value)

    def __call__(self, frames: torch.Tensor) -> torch.Tensor:
        assert frames.is_cuda and frames.dtype == torch.uint8 and frames.ndim == 4 and frames.shape[-1] == 3
        frames = frames.contiguous()
        n, h, w, _ = frames.shape
        oh, ow = self.out_shape(h, w)
        out = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device=frames.device)
        k = C.c_int()
        with torch.cuda.device(self.ctx.device):
            _check(lib().ss4k_upscale_frames_temporal(self._h, frames.data_ptr(), n, h, w, out.data_ptr(), out.numel(), C.byref(k), _stream()))
        return out[:k.value]

    def _out_view(self, out: torch.Tensor, oh: int, ow: int) -> torch.Tensor:
        """A caller-owned result buffer as (capacity, oh, ow, 3): any contiguous uint8 view on this device; bytes beyond whole frames are not used."""
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
                and out.device.index == torch.device(self.ctx.device).index):
            raise ValueError("out= is a contiguous uint8 tensor or view on the upscaler's device")
        frame = oh * ow * 3
        cap = out.numel() // frame
        return out.reshape(-1)[:cap * frame].view(cap, oh, ow, 3)

    def flush(self, slot: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The frames still inside a slot's stream, oldest first; the stream ends and the slot is free for another.  ``out``: a caller-owned
        contiguous uint8 device view to write them into (the result is a view of its first frames); one too small for the pending frames is the
        library's refusal, and the stream stays as it was."""
        left = self.pending if slot == 0 else self.pending_of(slot)
        oh, ow = self.out_shape()
        if out is None:
            out = torch.empty((left, oh, ow, 3), dtype=torch.uint8, device=self.ctx.device)
        else:
            out = self._out_view(out, oh, ow)
        k = C.c_int()
        with torch.cuda.device(self.ctx.device):
            if slot == 0:
                _check(lib().ss4k_upscaler_temporal_flush(self._h, out.data_ptr() if out.numel() else None, out.numel(), C.byref(k), _stream()))
            else:
                _check(lib().ss4k_upscaler_temporal_flush_stream(self._h, int(slot), out.data_ptr() if out.numel() else None, out.numel(), C.byref(k), _stream()))
        return out[:k.value]

    def set_denoise_rate(self, slot: int, rate: float) -> None:
        """The denoise rate of one slot's stream (ss4k_upscaler_temporal_set_denoise_rate_stream): its frames enter at the level 0.1 * rate from
        the next call or round on.  It ends with the stream: after ``flush`` / ``reset`` the slot is back at the object's ``denoise_rate``."""
        _check(lib().ss4k_upscaler_temporal_set_denoise_rate_stream(self._h, int(slot), float(rate)))

    def reset(self, slot: int = 0) -> None:
        if slot == 0:
            _check(lib().ss4k_upscaler_temporal_reset(self._h))
        else:
            _check(lib().ss4k_upscaler_temporal_reset_stream(self._h, int(slot)))

    def pending_of(self, slot: int) -> int:
        """Frames of a slot's stream that went in and have not come back."""
        k = C.c_int()
        _check(lib().ss4k_upscaler_temporal_pending_stream(self._h, int(slot), C.byref(k)))
        return k.value

    def stream_state_bytes_for(self) -> int:
        """Device bytes one slot holds while its stream runs (the denoiser's state and the ring of waiting LR planes): known before any push."""
        b = C.c_size_t()
        _check(lib().ss4k_upscaler_temporal_stream_state_bytes_for(self._h, C.byref(b)))
        return int(b.value)

    def release_idle(self) -> None:
        """Frees the state of every slot without a running stream; ``state_bytes`` drops by their share."""
        with torch.cuda.device(self.ctx.device):
            _check(lib().ss4k_upscaler_temporal_release_idle(self._h))

    def round(self, frames, slots, out: Optional[torch.Tensor] = None):
        """One round (ss4k_upscale_round_temporal): ``frames`` is a list of (h, w, 3) uint8 device tensors or views, each with contiguous bytes at
        any byte address; frame i belongs to slot ``slots[i]``.  Frames of a slot enter in list order, at most ``max_push`` per slot and 64 in all.
        Returns ``(out, [(slot, count), ...])``: the frames that became ready, contiguous, slot after slot in order of first appearance and oldest
        first within a slot.  The counts are known without a synchronisation.  ``out``: a caller-owned contiguous uint8 device view that the ready
        frames are written into (the result is a view of it); one too small for them is the library's refusal, and nothing changes."""
        k = len(frames)
        if k != len(slots):
            raise ValueError(f"{k} frames and {len(slots)} slots")
        for f in frames:
            if not (isinstance(f, torch.Tensor) and f.is_cuda and f.dtype == torch.uint8 and f.ndim == 3 and f.shape[-1] == 3 and f.is_contiguous()):
                raise ValueError("a round takes (h, w, 3) uint8 device tensors whose bytes are contiguous")
        h, w = (int(frames[0].shape[0]), int(frames[0].shape[1])) if k else (1, 1)
        if any(tuple(f.shape) != (h, w, 3) for f in frames):
            raise ValueError("the frames of a round have one size")
        oh, ow = self.out_shape(h, w)
        if out is None:
            out = torch.empty((max(k, 1), oh, ow, 3), dtype=torch.uint8, device=self.ctx.device)
        else:
            out = self._out_view(out, oh, ow)
        ptrs = (C.c_void_p * max(k, 1))(*[f.data_ptr() for f in frames])
        ids = (C.c_int * max(k, 1))(*[int(s) for s in slots])
        counts, item_slots, n_items = (C.c_int * max(k, 1))(), (C.c_int * max(k, 1))(), C.c_int()
        with torch.cuda.device(self.ctx.device):
            _check(lib().ss4k_upscale_round_temporal(self._h, ptrs, ids, k, h, w, out.data_ptr() if out.numel() else None, out.numel(), counts, item_slots,
                                                     C.byref(n_items), _stream()))
        items = [(int(item_slots[t]), int(counts[t])) for t in range(n_items.value)]
        return out[:sum(c for _, c in items)], items


FRVSR_MAX_STREAMS = 64   # SS4K_FRVSR_MAX_STREAMS (include/ss4k.h)
FRV_STAGES = ("fnet_conv", "srnet_conv", "pool_up", "flow_finish", "warp", "tail", "glue")
FRV_STAGES_TECOGAN = FRV_STAGES + ("convt", "conv_out", "skip")   # stages 7..9: a TecoGAN generator's tail ("tail" stays 0 there)
FRVSR_EGVSR, FRVSR_TECOGAN = 0, 1   # SS4K_FRVSR_EGVSR / SS4K_FRVSR_TECOGAN
FRVSR_BD, FRVSR_BI = 0, 1   # SS4K_FRVSR_BD / SS4K_FRVSR_BI: FRNet's `degradation`, the up-sampling function (bicubic | bilinear x4)
FRVSR_CONVT_EMBEDDED, FRVSR_CONVT_PHASE = 1, 4   # route_flags: SS4K_FRVSR_CONVT_* (0: the library's choice, today the embedded route)


def make_frvsr_desc(dtype: int = F32, num_feat: int = 64, num_block: int = 10, flags: int = 0) -> FrvsrDesc:
    d = FrvsrDesc()
    d.dtype, d.num_feat, d.num_block, d.flags = dtype, num_feat, num_block, int(flags)
    return d


def frvsr_degradation(degradation) -> int:
    """'BD' | 'BI' | 0 | 1 -> SS4K_FRVSR_BD | SS4K_FRVSR_BI; anything else raises ValueError (weights.frvsr_degradation)."""
    from . import weights as W
    return W.FRVSR_DEGRADATIONS[W.frvsr_degradation(degradation)]


def frvsr_param_count(desc: FrvsrDesc, generator: int = FRVSR_EGVSR, degradation: int = FRVSR_BD) -> int:
    if degradation != FRVSR_BD:
        return int(lib().ss4k_frvsr_param_count_ex(C.byref(desc), int(generator), int(degradation)))
    if generator == FRVSR_EGVSR:
        return int(lib().ss4k_frvsr_param_count(C.byref(desc)))
    return int(lib().ss4k_frvsr_param_count_as(C.byref(desc), int(generator)))


class Frvsr:
    """ss4k_frvsr: EGVSR's FRNet x4 (``generator=0``) or TecoGAN's (``generator=1``, tecogan_nets.py:101-202) resident on one GPU; callable like
    the reference's ``self.model(lr_curr, lr_prev, hr_prev)`` (egvsr_upscaler.py:204).  ``degradation``: FRVSR_BD (the entry points from before
    there was a choice) or FRVSR_BI (``ss4k_frvsr_create_ex``)."""

    def __init__(self, ctx: Context, desc: FrvsrDesc, flat_weights: np.ndarray, generator: int = FRVSR_EGVSR, route_flags: int = 0,
                 degradation: int = FRVSR_BD):
        self.ctx, self.desc, self.generator, self.degradation = ctx, desc, int(generator), int(degradation)
        w = np.ascontiguousarray(flat_weights, dtype=np.float32)
        h = C.c_void_p()
        with torch.cuda.device(ctx.device):
            if self.degradation != FRVSR_BD:
                _check(lib().ss4k_frvsr_create_ex(ctx._h, C.byref(desc), self.generator, self.degradation, int(route_flags),
                                                  w.ctypes.data_as(C.c_void_p), w.size, C.byref(h)))
            elif self.generator == FRVSR_EGVSR and not route_flags:
                _check(lib().ss4k_frvsr_create(ctx._h, C.byref(desc), w.ctypes.data_as(C.c_void_p), w.size, C.byref(h)))
            else:
                _check(lib().ss4k_frvsr_create_as(ctx._h, C.byref(desc), self.generator, int(route_flags), w.ctypes.data_as(C.c_void_p), w.size,
                                                  C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().ss4k_frvsr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def workspace_bytes(self, n, h, w) -> int:
        b = C.c_size_t()
        _check(lib().ss4k_frvsr_workspace_bytes(self._h, n, h, w, C.byref(b)))
        return int(b.value)

    def prof_enable(self, on: bool = True):
        _check(lib().ss4k_frvsr_prof_enable(self._h, int(on)))

    def prof_read(self) -> dict:
        """{stage: total ms since prof_enable(True)}; waits for the recorded events."""
        out = {}
        for k, name in enumerate(FRV_STAGES_TECOGAN if self.generator == FRVSR_TECOGAN else FRV_STAGES):
            ms = C.c_double()
            _check(lib().ss4k_frvsr_prof_read(self._h, k, C.byref(ms)))
            out[name] = ms.value
        return out

    def __call__(self, lr_curr: torch.Tensor, lr_prev: torch.Tensor, hr_prev: torch.Tensor) -> torch.Tensor:
        dev = self.ctx.device
        lr_curr, lr_prev, hr_prev = (t.to(device=dev, dtype=torch.float32).contiguous() for t in (lr_curr, lr_prev, hr_prev))
        n, c, h, w = lr_curr.shape
        assert c == 3 and tuple(lr_prev.shape) == (n, 3, h, w) and tuple(hr_prev.shape) == (n, 3, 4 * h, 4 * w), "FRNet.forward shapes"
        out = torch.empty((n, 3, 4 * h, 4 * w), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _check(lib().ss4k_frvsr_step(self._h, lr_curr.data_ptr(), lr_prev.data_ptr(), hr_prev.data_ptr(), out.data_ptr(), n, h, w, _stream()))
        return out

    forward = __call__

    def eval(self):
        return self


class FrvsrUpscaler:
    """ss4k_frvsr_upscaler: EgvsrUpscalerService.upscale (egvsr_upscaler.py:172-212), uint8 NHWC frames of ONE stream in order -> uint8 NHWC;
    with ``max_streams`` > 1 also rounds of one frame per stream slot (``upscale_streams``).  Calling the object drives slot 0."""

    def __init__(self, ctx: Context, model: Frvsr, lr_shape, output_shape=None, max_streams: int = 1, scene_cut: Optional[float] = None):
        self.ctx, self.model, self.max_streams = ctx, model, int(max_streams)
        oh, ow = (0, 0) if output_shape is None else (int(output_shape[0]), int(output_shape[1]))
        h = C.c_void_p()
        if self.max_streams == 1:   # (the entry point every build of the library has: tools/lib_ab.py loads older ones)
            _check(lib().ss4k_frvsr_upscaler_create(ctx._h, model._h, int(lr_shape[0]), int(lr_shape[1]), oh, ow, C.byref(h)))
        else:
            _check(lib().ss4k_frvsr_upscaler_create_streams(ctx._h, model._h, int(lr_shape[0]), int(lr_shape[1]), oh, ow, self.max_streams, C.byref(h)))
        self._h = h
        if scene_cut is not None:
            try:
                self.set_scene_cut(scene_cut)
            except Exception:
                self.close()
                raise

    def close(self):
        if getattr(self, "_h", None):
            lib().ss4k_frvsr_upscaler_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, slot: Optional[int] = None):
        """Forget the state of every slot, or of ``slot`` only."""
        if slot is None:
            _check(lib().ss4k_frvsr_upscaler_reset(self._h))
        else:
            _check(lib().ss4k_frvsr_upscaler_reset_stream(self._h, int(slot)))

    def set_scene_cut(self, threshold: float) -> None:
        """Scene-cut detection in front of every round (include/ss4k.h): ``threshold`` is the mean absolute byte difference between a
        stream's consecutive input frames, in (0, 255]; 0 turns it off (the default).  A cut resets that stream's state on the device."""
        _check(lib().ss4k_frvsr_upscaler_set_scene_cut(self._h, float(threshold)))

    def scene_cut(self) -> float:
        t = C.c_double()
        _check(lib().ss4k_frvsr_upscaler_scene_cut(self._h, C.byref(t)))
        return float(t.value)

    def scene_cut_stats(self, slot: int = 0) -> dict:
        """The slot's counters and its last frame's values: compared, cuts, last_sad, last_score, last_was_cut.  Synchronises."""
        s = SceneCutStats()
        with torch.cuda.device(self.ctx.device):
            _check(lib().ss4k_frvsr_upscaler_scene_cut_stats(self._h, int(slot), C.byref(s), _stream()))
        return {"compared": int(s.compared), "cuts": int(s.cuts), "last_sad": int(s.last_sad), "last_score": int(s.last_score),
                "last_was_cut": int(s.last_was_cut)}

    def scene_cut_total(self) -> int:
        """Cuts of all slots in the rounds that have completed on the device; never synchronises."""
        n = C.c_uint64()
        _check(lib().ss4k_frvsr_upscaler_scene_cut_total(self._h, C.byref(n)))
        return int(n.value)

    def state_bytes(self) -> int:
        """Device bytes of recurrent state held now (slots that never saw a frame hold none)."""
        b = C.c_size_t()
        _check(lib().ss4k_frvsr_upscaler_state_bytes(self._h, C.byref(b)))
        return int(b.value)

    def out_shape(self):
        oh, ow = C.c_int(), C.c_int()
        _check(lib().ss4k_frvsr_upscaler_out_shape(self._h, C.byref(oh), C.byref(ow)))
        return oh.value, ow.value

    def enable_taps(self, on=True):
        _check(lib().ss4k_frvsr_upscaler_enable_taps(self._h, int(on)))

    def read_tap(self, which: int) -> torch.Tensor:
        dims = (C.c_int * 4)()
        _check(lib().ss4k_frvsr_upscaler_read_tap(self._h, which, None, 0, C.byref(dims), _stream()))
        out = torch.empty(tuple(dims), dtype=torch.float32, device=self.ctx.device)
        _check(lib().ss4k_frvsr_upscaler_read_tap(self._h, which, out.data_ptr(), out.numel(), C.byref(dims), _stream()))
        return out

    def __call__(self, frames: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        assert frames.is_cuda and frames.dtype == torch.uint8 and frames.ndim == 4 and frames.shape[-1] == 3
        frames = frames.contiguous()
        n, h, w, _ = frames.shape
        oh, ow = self.out_shape()
        if out is None:
            out = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device=frames.device)
        with torch.cuda.device(self.ctx.device):
            _check(lib().ss4k_frvsr_upscale_frames(self._h, frames.data_ptr(), n, h, w, out.data_ptr(), out.numel(), _stream()))
        return out

    def upscale_streams(self, frames: torch.Tensor, slots: Sequence[int], out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One round: ``frames[i]`` is the next frame of the stream in slot ``slots[i]`` (distinct slots); returns ``(len(slots), oh, ow, 3)``
        in the same order.  The round runs as one batched step (ss4k_frvsr_upscale_streams)."""
        assert frames.is_cuda and frames.dtype == torch.uint8 and frames.ndim == 4 and frames.shape[-1] == 3
        frames = frames.contiguous()
        n, h, w, _ = frames.shape
        slots = [int(s) for s in slots]
        assert len(slots) == n, "one slot per frame"
        oh, ow = self.out_shape()
        if out is None:
            out = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device=frames.device)
        ids = (C.c_int32 * max(n, 1))(*slots)
        with torch.cuda.device(self.ctx.device):
            _check(lib().ss4k_frvsr_upscale_streams(self._h, ids, n, frames.data_ptr(), h, w, out.data_ptr(), out.numel(), _stream()))
        return out

    @staticmethod
    def has_streams_at() -> bool:
        """Whether the loaded library has the scattered round (an older build loaded through SS4K_LIB has not)."""
        return hasattr(lib(), "ss4k_frvsr_upscale_streams_at")

    def upscale_streams_at(self, frames: Sequence[torch.Tensor], slots: Sequence[int], outs: Sequence[torch.Tensor]) -> None:
        """One round like ``upscale_streams`` with the frames scattered: ``frames[i]`` is a contiguous ``(h, w, 3)`` uint8 device tensor - a
        row of a larger tensor will do - with the next frame of the stream in slot ``slots[i]``, and its result is written into ``outs[i]``,
        a contiguous ``(oh, ow, 3)`` one.  Nothing is gathered or scattered: the kernels read and write the frames where they lie
        (ss4k_frvsr_upscale_streams_at), bit for bit what ``upscale_streams`` gives."""
        n = len(frames)
        slots = [int(s) for s in slots]
        assert n >= 1 and len(slots) == n and len(outs) == n, "one slot and one output frame per frame"
        h, w = int(frames[0].shape[0]), int(frames[0].shape[1])
        oh, ow = self.out_shape()
        for f, o in zip(frames, outs):
            assert f.is_cuda and f.dtype == torch.uint8 and tuple(f.shape) == (h, w, 3) and f.is_contiguous(), "frames: contiguous (h, w, 3) uint8"
            assert o.is_cuda and o.dtype == torch.uint8 and tuple(o.shape) == (oh, ow, 3) and o.is_contiguous(), "outs: contiguous (oh, ow, 3) uint8"
            assert f.device == o.device == frames[0].device
        ids = (C.c_int32 * n)(*slots)
        fin = (C.c_void_p * n)(*[f.data_ptr() for f in frames])
        fout = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
        with torch.cuda.device(self.ctx.device):
            _check(lib().ss4k_frvsr_upscale_streams_at(self._h, ids, n, fin, h, w, fout, oh * ow * 3, _stream()))


class TemporalFrvsrUpscaler:
    """ss4k_frvsr_temporal: the frame-recurrent service chain (uint8 HWC frames -> uint8 NHWC) with the online BSVD denoiser in front of the
    generator, per stream.  ``model`` is a ``Frvsr`` (either generator, either degradation), ``denoise`` a BSVD ``Model`` built with
    ``bsvd_stream=True``; both are held, not owned.  A stream returns nothing for its first 16 frames and one frame per frame after; ``flush``
    returns the up to 16 frames still inside and ends it.  The methods mirror ``TemporalUpscaler``'s.  ``pad=True``
    (ss4k_frvsr_temporal_create_padded) accepts an ``lr_shape`` that 4 does not divide: the denoiser alone runs at the shape rounded up to
    multiples of 4, on reflect-padded planes, and its output is cropped (include/ss4k.h); at a divisible shape it changes nothing."""

    def __init__(self, ctx: Context, model: Frvsr, denoise: Model, lr_shape, output_shape=None, denoise_rate: float = 1.0, max_push: int = 4,
                 max_streams: int = 1, scene_cut: Optional[float] = None, pad: bool = False, noise_map: str = "constant"):
        self.ctx, self.model, self.denoise, self.max_push, self.max_streams = ctx, model, denoise, int(max_push), int(max_streams)
        mode = noise_map_mode(noise_map)
        self.lr_shape = (int(lr_shape[0]), int(lr_shape[1]))
        oh, ow = (0, 0) if output_shape is None else (int(output_shape[0]), int(output_shape[1]))
        h = C.c_void_p()
        if pad and not self.has_padded():
            raise RuntimeError("pad=True needs a library with ss4k_frvsr_temporal_create_padded")
        create = lib().ss4k_frvsr_temporal_create_padded if pad else lib().ss4k_frvsr_temporal_create
        self.padded_shape = tuple((v + 3) // 4 * 4 for v in self.lr_shape) if pad else self.lr_shape
        with torch.cuda.device(ctx.device):
            _check(create(ctx._h, model._h, denoise._h, self.lr_shape[0], self.lr_shape[1], oh, ow, float(denoise_rate),
                          self.max_push, self.max_streams, C.byref(h)))
        self._h, self.lag = h, 16
        try:
            if scene_cut is not None:
                self.set_scene_cut(scene_cut)
            if mode != 0:
                self.set_noise_map(noise_map)
        except Exception:
            self.close()
            raise

    @staticmethod
    def has_padded() -> bool:
        """Whether the loaded library has ``pad=True`` (an older build loaded through SS4K_LIB has not)."""
        return hasattr(lib(), "ss4k_frvsr_temporal_create_padded")

    def close(self):
        if getattr(self, "_h", None):
            lib().ss4k_frvsr_temporal_destroy(self._h)
            self._h = None

    def set_noise_map(self, noise_map: str) -> None:
        """``'constant'`` (default) or ``'motion'``: ``TemporalUpscaler.set_noise_map`` (ss4k_frvsr_temporal_set_noise_map).  With ``pad=True``
        the map is computed on the ``lr_shape`` frame and reflect-padded with the colour planes."""
        _check(lib().ss4k_frvsr_temporal_set_noise_map(self._h, noise_map_mode(noise_map)))

    def noise_map(self) -> str:
        m = C.c_int()
        _check(lib().ss4k_frvsr_temporal_noise_map(self._h, C.byref(m)))
        return {v: k for k, v in NOISE_MAPS.items()}[int(m.value)]

    def set_scene_cut(self, threshold: float) -> None:
        """Scene-cut detection in front of every round, every slot (include/ss4k.h): ``threshold`` is the mean absolute byte difference between
        a stream's consecutive input frames, in (0, 255]; 0 turns it off (the default).  A cut keeps the two scenes apart inside the denoiser
        and, when the scene's first frame leaves it 16 frames later, zeroes the stream's recurrent state: the output is that of the scenes run
        as separate streams, and every round still returns the frames it returns without the detector."""
        with torch.cuda.device(self.ctx.device):
            _check(lib().ss4k_frvsr_temporal_set_scene_cut(self._h, float(threshold)))

    def scene_cut(self) -> float:
        t = C.c_double()
        _check(lib().ss4k_frvsr_temporal_scene_cut(self._h, C.byref(t)))
        return float(t.value)

    def scene_cut_stats(self, slot: int = 0) -> dict:
        """The counters of a slot's stream and its last frame's values: compared, cuts, last_sad, last_score, last_was_cut.  Synchronises."""
        s = SceneCutStats()
        with torch.cuda.device(self.ctx.device):
            _check(lib().ss4k_frvsr_temporal_scene_cut_stats_stream(self._h, int(slot), C.byref(s), _stream()))
        return {"compared": int(s.compared), "cuts": int(s.cuts), "last_sad": int(s.last_sad), "last_score": int(s.last_score),
                "last_was_cut": int(s.last_was_cut)}

    def scene_cut_total(self) -> int:
        """Cuts in the rounds that have completed on the device, over all slots; never synchronises."""
        n = C.c_uint64()
        _check(lib().ss4k_frvsr_temporal_scene_cut_total(self._h, C.byref(n)))
        return int(n.value)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def out_shape(self):
        oh, ow = C.c_int(), C.c_int()
        _check(lib().ss4k_frvsr_temporal_out_shape(self._h, C.byref(oh), C.byref(ow)))
        return oh.value, ow.value

    def pending_of(self, slot: int) -> int:
        """Frames of a slot's stream that went in and have not come back."""
        k = C.c_int()
        _check(lib().ss4k_frvsr_temporal_pending_stream(self._h, int(slot), C.byref(k)))
        return k.value

    @property
    def pending(self) -> int:
        return self.pending_of(0)

    def state_bytes(self) -> int:
        b = C.c_size_t()
        _check(lib().ss4k_frvsr_temporal_state_bytes(self._h, C.byref(b)))
        return int(b.value)

    def stream_state_bytes_for(self) -> int:
        """Device bytes one slot holds while its stream runs (the denoiser's state, the ring of waiting LR planes, lr / hr twice): known before
        any push."""
        b = C.c_size_t()
        _check(lib().ss4k_frvsr_temporal_stream_state_bytes_for(self._h, C.byref(b)))
        return int(b.value)

    def release_idle(self) -> None:
        """Frees the state of every slot without a running stream; ``state_bytes`` drops by their share."""
        with torch.cuda.device(self.ctx.device):
            _check(lib().ss4k_frvsr_temporal_release_idle(self._h))

    def set_denoise_rate(self, slot: int, rate: float) -> None:
        """The denoise rate of one slot's stream: its frames enter at the level 0.1 * rate from the next round on.  It ends with the stream."""
        _check(lib().ss4k_frvsr_temporal_set_denoise_rate_stream(self._h, int(slot), float(rate)))

    def reset(self, slot: int = 0) -> None:
        _check(lib().ss4k_frvsr_temporal_reset_stream(self._h, int(slot)))

    _out_view = TemporalUpscaler._out_view

    def flush(self, slot: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The frames still inside a slot's stream, through the generator in order, oldest first; the stream ends and the slot is free."""
        left = self.pending_of(slot)
        oh, ow = self.out_shape()
        out = torch.empty((left, oh, ow, 3), dtype=torch.uint8, device=self.ctx.device) if out is None else self._out_view(out, oh, ow)
        k = C.c_int()
        with torch.cuda.device(self.ctx.device):
            _check(lib().ss4k_frvsr_temporal_flush_stream(self._h, int(slot), out.data_ptr() if out.numel() else None, out.numel(), C.byref(k), _stream()))
        return out[:k.value]

    def round(self, frames, slots, out: Optional[torch.Tensor] = None):
        """One round (ss4k_frvsr_temporal_round), as ``TemporalUpscaler.round``: ``frames`` is a list of (h, w, 3) uint8 device tensors or views
        with contiguous bytes at any byte address, frame i of slot ``slots[i]``; returns ``(out, [(slot, count), ...])``, the ready frames slot
        after slot in order of first appearance and oldest first within a slot."""
        k = len(frames)
        if k != len(slots):
            raise ValueError(f"{k} frames and {len(slots)} slots")
        for f in frames:
            if not (isinstance(f, torch.Tensor) and f.is_cuda and f.dtype == torch.uint8 and f.ndim == 3 and f.shape[-1] == 3 and f.is_contiguous()):
                raise ValueError("a round takes (h, w, 3) uint8 device tensors whose bytes are contiguous")
        h, w = (int(frames[0].shape[0]), int(frames[0].shape[1])) if k else (1, 1)
        if any(tuple(f.shape) != (h, w, 3) for f in frames):
            raise ValueError("the frames of a round have one size")
        oh, ow = self.out_shape()
        out = torch.empty((max(k, 1), oh, ow, 3), dtype=torch.uint8, device=self.ctx.device) if out is None else self._out_view(out, oh, ow)
        ptrs = (C.c_void_p * max(k, 1))(*[f.data_ptr() for f in frames])
        ids = (C.c_int * max(k, 1))(*[int(s) for s in slots])
        counts, item_slots, n_items = (C.c_int * max(k, 1))(), (C.c_int * max(k, 1))(), C.c_int()
        with torch.cuda.device(self.ctx.device):
            _check(lib().ss4k_frvsr_temporal_round(self._h, ptrs, ids, k, h, w, out.data_ptr() if out.numel() else None, out.numel(), counts, item_slots,
                                                   C.byref(n_items), _stream()))
        items = [(int(item_slots[t]), int(counts[t])) for t in range(n_items.value)]
        return out[:sum(c for _, c in items)], items

    def __call__(self, frames: torch.Tensor) -> torch.Tensor:
        """A round of slot 0: (n, h, w, 3) uint8, 1 <= n <= max_push -> the frames that became ready."""
        assert frames.is_cuda and frames.dtype == torch.uint8 and frames.ndim == 4 and frames.shape[-1] == 3
        frames = frames.contiguous()
        return self.round([frames[i] for i in range(frames.shape[0])], [0] * frames.shape[0])[0]
