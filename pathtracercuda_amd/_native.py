"""ctypes bindings of the native libraries (include/pt_hip.h, include/pt_host.h).

The libraries are built in-tree by `make` (or __graft_entry__.build()) into
pathtracercuda_amd/lib/.  There is no fallback: if they are missing the import fails loudly.
"""
from __future__ import annotations

import ctypes as C
import importlib.util
import os
import pathlib
import sys

LIB_DIR = pathlib.Path(__file__).resolve().parent / "lib"
HIP_LIB = LIB_DIR / "libpt_hip.so"
HOST_LIB = LIB_DIR / "libpt_host.so"
CLI = LIB_DIR / "pathtracer"

PT_OK, PT_ERR_HIP, PT_ERR_ARG, PT_ERR_STATE, PT_ERR_DEPTH, PT_ERR_NO_DEVICE = range(6)
PT_MAX_TEXTURES = 64


class PtCamera(C.Structure):
    """pt_camera (reference Camera.h:14-22)."""
    _fields_ = [("tan_half_fovy", C.c_float), ("aspect_ratio", C.c_float), ("origin", C.c_float * 3),
                ("lower_left_corner", C.c_float * 3), ("horizontal", C.c_float * 3), ("vertical", C.c_float * 3),
                ("right", C.c_float * 3), ("up", C.c_float * 3), ("backward", C.c_float * 3)]


class PtBvhNode(C.Structure):
    """pt_bvh_node (reference BVH.h:6-11)."""
    _fields_ = [("aabb_min", C.c_float * 3), ("aabb_max", C.c_float * 3), ("offset", C.c_uint32),
                ("primitive_count_axis", C.c_uint32)]


class PtHittable(C.Structure):
    """pt_hittable (reference Hittable.h:23-27 + Material.h:22-27)."""
    _fields_ = [("inv_transform_rows", (C.c_float * 4) * 3), ("base_color", C.c_float * 3), ("roughness", C.c_float),
                ("emissive", C.c_float * 3), ("metalness", C.c_float), ("texture_index", C.c_uint32),
                ("material_type", C.c_uint32), ("type", C.c_uint32), ("pad", C.c_uint32)]


class PtRenderStats(C.Structure):
    _fields_ = [("node_tests", C.c_uint64), ("prim_tests", C.c_uint64), ("hits", C.c_uint64),
                ("sky_lookups", C.c_uint64), ("segments", C.c_uint64), ("samples", C.c_uint64),
                ("wave_node_iters", C.c_uint64), ("wave_prim_iters", C.c_uint64), ("wave_hits", C.c_uint64),
                ("wave_sky", C.c_uint64), ("wave_segments", C.c_uint64), ("cycles_node_walk", C.c_uint64),
                ("cycles_leaf_tests", C.c_uint64), ("cycles_shading", C.c_uint64), ("cycles_total", C.c_uint64),
                ("cycles_lane_idle", C.c_uint64), ("leaf_rounds", C.c_uint64), ("family_execs", C.c_uint64),
                ("family_execs_compacted", C.c_uint64), ("leaf_round_lanes", C.c_uint64), ("leaf_pairs", C.c_uint64),
                ("family_execs_compacted_in_round", C.c_uint64), ("repairs", C.c_uint64)]


class PtAdaptiveParams(C.Structure):
    """pt_adaptive_params (pt_hip.h, adaptive sampling)."""
    _fields_ = [("spp", C.c_uint32), ("min_calls", C.c_uint32), ("max_calls", C.c_uint32), ("tolerance", C.c_float),
                ("floor", C.c_float), ("reset", C.c_int)]


class PtAdaptiveResult(C.Structure):
    _fields_ = [("rounds", C.c_uint32), ("samples", C.c_uint64), ("gpu_ms", C.c_float)]


class PtDenoiseParams(C.Structure):
    """pt_denoise_params (pt_hip.h, a-trous denoiser)."""
    _fields_ = [("iterations", C.c_uint32), ("sigma_color", C.c_float), ("sigma_plane", C.c_float),
                ("normal_power_log2", C.c_uint32), ("flags", C.c_uint32), ("staging", C.c_uint32)]


class PtTemporalParams(C.Structure):
    """pt_temporal_params (pt_hip.h, temporal reprojection)."""
    _fields_ = [("alpha_min", C.c_float), ("max_history", C.c_uint32), ("sigma_plane", C.c_float),
                ("normal_cos_min", C.c_float), ("flags", C.c_uint32)]


class PtVarianceParams(C.Structure):
    """pt_variance_params (pt_hip.h, the variance estimate of the temporal history)."""
    _fields_ = [("min_temporal", C.c_uint32)]


class PtVDenoiseParams(C.Structure):
    """pt_vdenoise_params (pt_hip.h, variance-guided a-trous filter)."""
    _fields_ = [("iterations", C.c_uint32), ("sigma_l", C.c_float), ("variance_floor", C.c_float),
                ("sigma_plane", C.c_float), ("normal_power_log2", C.c_uint32), ("flags", C.c_uint32),
                ("staging", C.c_uint32)]


class PtVFeedbackParams(C.Structure):
    """pt_vfeedback_params (pt_hip.h, the feedback of the filtered colour into the temporal history)."""
    _fields_ = [("level", C.c_uint32)]


class PtAdaptiveVarianceParams(C.Structure):
    """pt_adaptive_variance_params (pt_hip.h, the variance of an adaptive render's image)."""
    _fields_ = [("min_batches", C.c_uint32), ("sigma_plane", C.c_float), ("normal_cos_min", C.c_float),
                ("flags", C.c_uint32)]


class PtDespikeParams(C.Structure):
    """pt_despike_params (pt_hip.h, the same-surface firefly clamp)."""
    _fields_ = [("radius", C.c_uint32), ("rank", C.c_uint32), ("factor", C.c_float), ("floor", C.c_float),
                ("min_neighbors", C.c_uint32), ("sigma_plane", C.c_float), ("normal_cos_min", C.c_float),
                ("flags", C.c_uint32), ("staging", C.c_uint32)]


class PtUpsampleParams(C.Structure):
    """pt_upsample_params (pt_hip.h, the guided upsampling)."""
    _fields_ = [("sigma_plane", C.c_float), ("normal_power_log2", C.c_uint32), ("flags", C.c_uint32),
                ("staging", C.c_uint32)]


PT_UPSAMPLE_ACCUM, PT_UPSAMPLE_DENOISED, PT_UPSAMPLE_TEMPORAL, PT_UPSAMPLE_DESPIKED = 0, 1, 2, 3
PT_FEATURE_HIT, PT_FEATURE_EMISSIVE = 1, 2
PT_TEMPORAL_DEMODULATE, PT_TEMPORAL_SAME_PRIMITIVE = 1, 2
PT_DENOISE_DEMODULATE, PT_DENOISE_SAME_PRIMITIVE = 1, 2
PT_DENOISE_TILE_W, PT_DENOISE_TILE_H = 32, 8


# symbol -> (restype, argtypes); the CPU test suite checks that every declaration in include/*.h
# is exported and bound here.
P = C.POINTER
_HIP_SYMBOLS = {
    "pt_device_count": (C.c_int, [P(C.c_int)]),
    "pt_create": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, P(C.c_void_p)]),
    "pt_create_banded": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, P(C.c_void_p)]),
    "pt_band_rows": (C.c_uint32, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "pt_destroy": (None, [C.c_void_p]),
    "pt_set_scene": (C.c_int, [C.c_void_p, P(PtBvhNode), C.c_uint32, P(PtHittable), C.c_uint32]),
    "pt_set_texture": (C.c_int, [C.c_void_p, C.c_uint32, P(C.c_float), C.c_uint32, C.c_uint32]),
    "pt_set_skybox": (C.c_int, [C.c_void_p, C.c_uint32]),
    "pt_render": (C.c_int, [C.c_void_p, P(PtCamera), C.c_uint32, C.c_uint32, C.c_int, P(C.c_float)]),
    "pt_render_instrumented": (C.c_int, [C.c_void_p, P(PtCamera), C.c_uint32, C.c_uint32, C.c_int, P(C.c_float),
                                         P(PtRenderStats)]),
    "pt_render_adaptive": (C.c_int, [C.c_void_p, P(PtCamera), P(PtAdaptiveParams), P(PtAdaptiveResult)]),
    "pt_holds_adaptive": (C.c_int, [C.c_void_p]),
    "pt_read_moments": (C.c_int, [C.c_void_p, P(C.c_float)]),
    "pt_read_adaptive_hdr": (C.c_int, [C.c_void_p, P(C.c_float)]),
    "pt_tonemap_adaptive": (C.c_int, [C.c_void_p, P(C.c_uint8)]),
    "pt_read_accum": (C.c_int, [C.c_void_p, P(C.c_float)]),
    "pt_copy_accum_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "pt_tonemap": (C.c_int, [C.c_void_p, C.c_uint32, P(C.c_uint8)]),
    "pt_tonemap_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t]),
    "pt_read_rng": (C.c_int, [C.c_void_p, P(C.c_uint32)]),
    "pt_write_rng": (C.c_int, [C.c_void_p, P(C.c_uint32)]),
    "pt_local_rows": (C.c_uint32, [C.c_void_p]),
    "pt_read_tile_costs": (C.c_int, [C.c_void_p, P(C.c_uint32), C.c_uint32]),
    "pt_read_tile_idle": (C.c_int, [C.c_void_p, P(C.c_uint32), C.c_uint32]),
    "pt_set_strip_units": (C.c_int, [C.c_void_p, C.c_int]),
    "pt_set_rise_repair": (C.c_int, [C.c_void_p, C.c_int]),
    "pt_set_zero_quadric_consts": (C.c_int, [C.c_void_p, C.c_int]),
    "pt_set_run_ahead": (C.c_int, [C.c_void_p, C.c_int]),
    "pt_set_cold_start": (C.c_int, [C.c_void_p, C.c_uint32, C.c_int]),
    "pt_unpermute_bands": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                     C.c_uint32]),
    "pt_set_kernel_variant": (C.c_int, [C.c_void_p, C.c_int]),
    "pt_set_occupancy": (C.c_int, [C.c_void_p, C.c_uint32]),
    "pt_set_tile_trace": (C.c_int, [C.c_void_p, C.c_int]),
    "pt_read_tile_trace": (C.c_int, [C.c_void_p, P(C.c_uint32), C.c_uint32]),
    "pt_set_issue_priority": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32]),
    "pt_set_schedule": (C.c_int, [C.c_void_p, C.c_int]),
    "pt_set_sample_groups": (C.c_int, [C.c_void_p, C.c_int]),
    "pt_last_sample_groups": (C.c_int, [C.c_void_p]),
    "pt_last_variant": (C.c_int, [C.c_void_p]),
    "pt_last_launch": (C.c_int, [C.c_void_p, P(C.c_uint32)]),
    "pt_read_group_stats": (C.c_int, [C.c_void_p, P(C.c_uint32)]),
    "pt_set_patch_rounds": (C.c_int, [C.c_void_p, C.c_uint32]),
    "pt_set_group_lookback": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32]),
    "pt_read_group_fold": (C.c_int, [C.c_void_p, C.c_uint32, P(C.c_uint32)]),
    "pt_read_group_log_counts": (C.c_int, [C.c_void_p, P(C.c_uint32), C.c_size_t]),
    "pt_last_error": (C.c_char_p, [C.c_void_p]),
    "pt_render_features": (C.c_int, [C.c_void_p, P(PtCamera)]),
    "pt_read_features": (C.c_int, [C.c_void_p, C.c_uint32, P(C.c_float)]),
    "pt_read_features_timing": (C.c_int, [C.c_void_p, P(C.c_float)]),
    "pt_denoise": (C.c_int, [C.c_void_p, C.c_uint32, P(PtDenoiseParams)]),
    "pt_read_denoise_timing": (C.c_int, [C.c_void_p, P(C.c_float)]),
    "pt_read_denoised": (C.c_int, [C.c_void_p, P(C.c_float)]),
    "pt_tonemap_denoised": (C.c_int, [C.c_void_p, P(C.c_uint8)]),
    "pt_denoise_image": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, P(C.c_float), P(C.c_float), P(C.c_float),
                                   P(C.c_float), P(PtDenoiseParams), P(C.c_float)]),
    "pt_temporal": (C.c_int, [C.c_void_p, C.c_uint32, P(PtTemporalParams), C.c_int, P(C.c_int)]),
    "pt_read_temporal": (C.c_int, [C.c_void_p, P(C.c_float)]),
    "pt_tonemap_temporal": (C.c_int, [C.c_void_p, P(C.c_uint8)]),
    "pt_read_temporal_timing": (C.c_int, [C.c_void_p, P(C.c_float)]),
    "pt_denoise_temporal": (C.c_int, [C.c_void_p, P(PtDenoiseParams)]),
    "pt_temporal_image": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_float),
                                    P(PtCamera), P(C.c_float), P(C.c_float), P(C.c_float), P(PtCamera), P(PtTemporalParams),
                                    P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_float)]),
    "pt_temporal_moments": (C.c_int, [C.c_void_p, C.c_uint32, P(PtTemporalParams), P(PtVarianceParams), C.c_int, P(C.c_int)]),
    "pt_read_temporal_variance": (C.c_int, [C.c_void_p, P(C.c_float)]),
    "pt_read_temporal_moments_timing": (C.c_int, [C.c_void_p, P(C.c_float)]),
    "pt_denoise_variance": (C.c_int, [C.c_void_p, P(PtVDenoiseParams)]),
    "pt_temporal_moments_image": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32] + [P(C.c_float)] * 4 + [P(PtCamera)]
                                  + [P(C.c_float)] * 4 + [P(PtCamera), P(PtTemporalParams), P(PtVarianceParams)]
                                  + [P(C.c_float)] * 6),
    "pt_denoise_variance_image": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32] + [P(C.c_float)] * 5
                                  + [P(PtVDenoiseParams), P(C.c_float)]),
    "pt_denoise_variance_feedback": (C.c_int, [C.c_void_p, P(PtVDenoiseParams), P(PtVFeedbackParams)]),
    "pt_read_feedback_timing": (C.c_int, [C.c_void_p, P(C.c_float)]),
    "pt_read_temporal_history": (C.c_int, [C.c_void_p, C.c_uint32, P(C.c_float)]),
    "pt_denoise_variance_feedback_image": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32] + [P(C.c_float)] * 6
                                           + [P(PtVDenoiseParams), P(PtVFeedbackParams), P(C.c_float), P(C.c_float)]),
    "pt_denoise_adaptive": (C.c_int, [C.c_void_p, P(PtAdaptiveVarianceParams), P(PtVDenoiseParams)]),
    "pt_read_adaptive_variance": (C.c_int, [C.c_void_p, P(C.c_float)]),
    "pt_read_adaptive_variance_timing": (C.c_int, [C.c_void_p, P(C.c_float)]),
    "pt_adaptive_variance_image": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32] + [P(C.c_float)] * 5
                                   + [P(PtAdaptiveVarianceParams), C.c_uint32, P(C.c_float)]),
    "pt_despike": (C.c_int, [C.c_void_p, C.c_uint32, P(PtDespikeParams)]),
    "pt_holds_despiked": (C.c_int, [C.c_void_p]),
    "pt_read_despiked": (C.c_int, [C.c_void_p, P(C.c_float)]),
    "pt_tonemap_despiked": (C.c_int, [C.c_void_p, P(C.c_uint8)]),
    "pt_read_despike_count": (C.c_int, [C.c_void_p, P(C.c_uint32)]),
    "pt_read_despike_timing": (C.c_int, [C.c_void_p, P(C.c_float)]),
    "pt_denoise_despiked": (C.c_int, [C.c_void_p, P(PtDenoiseParams)]),
    "pt_despike_image": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32] + [P(C.c_float)] * 4
                         + [P(PtDespikeParams), P(C.c_float), P(C.c_uint32)]),
    "pt_upsample": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, P(PtUpsampleParams)]),
    "pt_holds_upsampled": (C.c_int, [C.c_void_p]),
    "pt_read_upsampled": (C.c_int, [C.c_void_p, P(C.c_float)]),
    "pt_tonemap_upsampled": (C.c_int, [C.c_void_p, P(C.c_uint8)]),
    "pt_read_upsample_counts": (C.c_int, [C.c_void_p, P(C.c_uint32)]),
    "pt_read_upsample_timing": (C.c_int, [C.c_void_p, P(C.c_float)]),
    "pt_upsample_image": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32] + [P(C.c_float)] * 4 + [C.c_uint32, C.c_uint32]
                          + [P(C.c_float)] * 3 + [P(PtUpsampleParams), P(C.c_float), P(C.c_uint32)]),
    "pt_upsample_resolve": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                      P(PtUpsampleParams)]),
    "pt_upsample_resolve_image": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32] + [P(C.c_float)] * 4 + [C.c_uint32, C.c_uint32]
                                  + [P(C.c_float)] * 3 + [C.c_uint32, P(PtUpsampleParams), P(C.c_float), P(C.c_uint32)]),
    "pt_set_scene_moved": (C.c_int, [C.c_void_p, P(PtBvhNode), C.c_uint32, P(PtHittable), C.c_uint32, P(C.c_float),
                                     P(C.c_uint32)]),
    "pt_holds_motion": (C.c_int, [C.c_void_p]),
    "pt_temporal_motion_image": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32] + [P(C.c_float)] * 4 + [P(PtCamera)]
                                 + [P(C.c_float)] * 3 + [P(PtCamera), P(PtTemporalParams)] + [P(C.c_float)] * 4
                                 + [C.c_uint32, P(C.c_float), P(C.c_uint32)]),
    "pt_temporal_moments_motion_image": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32] + [P(C.c_float)] * 4 + [P(PtCamera)]
                                         + [P(C.c_float)] * 4 + [P(PtCamera), P(PtTemporalParams), P(PtVarianceParams)]
                                         + [P(C.c_float)] * 6 + [C.c_uint32, P(C.c_float), P(C.c_uint32)]),
    "pt_set_primitive_boxes": (C.c_int, [C.c_void_p, P(C.c_float)]),
    "pt_holds_primitive_boxes": (C.c_int, [C.c_void_p]),
    "pt_move_primitives": (C.c_int, [C.c_void_p, C.c_uint32, P(C.c_uint32), P(PtHittable), P(C.c_float), P(C.c_float),
                                     P(C.c_uint32)]),
    "pt_read_bvh": (C.c_int, [C.c_void_p, P(PtBvhNode), P(C.c_float)]),
    "pt_read_primitive": (C.c_int, [C.c_void_p, C.c_uint32, P(C.c_float)]),
    "pt_read_refit_timing": (C.c_int, [C.c_void_p, P(C.c_float)]),
    "pt_group_create": (C.c_int, [C.c_int, P(C.c_int), C.c_uint32, C.c_uint32, C.c_uint32, P(C.c_void_p)]),
    "pt_group_destroy": (None, [C.c_void_p]),
    "pt_group_size": (C.c_int, [C.c_void_p]),
    "pt_group_context": (C.c_void_p, [C.c_void_p, C.c_int]),
    "pt_group_set_scene": (C.c_int, [C.c_void_p, P(PtBvhNode), C.c_uint32, P(PtHittable), C.c_uint32]),
    "pt_group_set_texture": (C.c_int, [C.c_void_p, C.c_uint32, P(C.c_float), C.c_uint32, C.c_uint32]),
    "pt_group_set_skybox": (C.c_int, [C.c_void_p, C.c_uint32]),
    "pt_group_render": (C.c_int, [C.c_void_p, P(PtCamera), C.c_uint32, C.c_uint32, C.c_int, P(C.c_float)]),
    "pt_group_gather": (C.c_int, [C.c_void_p, P(C.c_float)]),
    "pt_group_read_accum": (C.c_int, [C.c_void_p, P(C.c_float)]),
    "pt_group_tonemap": (C.c_int, [C.c_void_p, C.c_uint32, P(C.c_uint8)]),
    "pt_group_last_error": (C.c_char_p, [C.c_void_p]),
}

_HOST_SYMBOLS = {
    "pth_last_error": (C.c_char_p, []),
    "pth_scene_load": (C.c_int, [C.c_char_p, C.c_uint32, C.c_uint32, P(C.c_void_p)]),
    "pth_scene_free": (None, [C.c_void_p]),
    "pth_scene_timing": (C.c_int, [C.c_void_p, P(C.c_double), P(C.c_double)]),
    "pth_scene_object_count": (C.c_uint32, [C.c_void_p]),
    "pth_scene_node_count": (C.c_uint32, [C.c_void_p]),
    "pth_scene_bvh_depth": (C.c_uint32, [C.c_void_p]),
    "pth_scene_objects": (C.c_int, [C.c_void_p, P(PtHittable), P(C.c_float)]),
    "pth_scene_bvh": (C.c_int, [C.c_void_p, P(PtBvhNode), P(PtHittable)]),
    "pth_scene_camera": (C.c_int, [C.c_void_p, P(PtCamera)]),
    "pth_scene_skybox": (C.c_uint32, [C.c_void_p]),
    "pth_scene_texture_count": (C.c_uint32, [C.c_void_p]),
    "pth_scene_texture_info": (C.c_int, [C.c_void_p, C.c_uint32, P(C.c_uint32), P(C.c_uint32)]),
    "pth_scene_texture_data": (C.c_int, [C.c_void_p, C.c_uint32, P(C.c_float)]),
    "pth_camera_make": (C.c_int, [P(C.c_float), P(C.c_float), P(C.c_float), C.c_float, C.c_float, P(PtCamera)]),
    "pth_camera_rotate": (C.c_int, [P(PtCamera), C.c_float, C.c_float, C.c_float]),
    "pth_camera_translate": (C.c_int, [P(PtCamera), C.c_float, C.c_float, C.c_float]),
    "pth_radians": (C.c_float, [C.c_float]),
    "pth_renderer_create": (C.c_int, [C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, P(C.c_void_p)]),
    "pth_renderer_create_banded": (C.c_int, [C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32,
                                             P(C.c_void_p)]),
    "pth_renderer_create_group": (C.c_int, [C.c_uint32, C.c_uint32, C.c_int, P(C.c_int), C.c_uint32, P(C.c_void_p)]),
    "pth_renderer_gather_ms": (C.c_float, [C.c_void_p]),
    "pth_renderer_destroy": (None, [C.c_void_p]),
    "pth_renderer_load_scene": (C.c_int, [C.c_void_p, C.c_char_p, P(PtCamera)]),
    "pth_renderer_load_scene_moved": (C.c_int, [C.c_void_p, C.c_char_p, P(C.c_uint32), P(PtCamera)]),
    "pth_renderer_holds_motion": (C.c_int, [C.c_void_p]),
    "pth_renderer_motion_table": (C.c_uint32, [C.c_void_p, P(P(C.c_float)), P(P(C.c_uint32))]),
    "pth_renderer_move_objects": (C.c_int, [C.c_void_p, C.c_uint32, P(C.c_uint32), P(C.c_float), P(C.c_float), P(C.c_float)]),
    "pth_renderer_rebuild_scene": (C.c_int, [C.c_void_p]),
    "pth_renderer_object_transforms": (C.c_uint32, [C.c_void_p, P(C.c_float), P(C.c_float), P(C.c_float)]),
    "pth_renderer_refit_timing": (C.c_int, [C.c_void_p, P(C.c_float)]),
    "pth_renderer_bvh": (C.c_int, [C.c_void_p, P(PtBvhNode), P(PtHittable), P(C.c_uint32), P(C.c_uint32)]),
    "pth_refit_boxes": (C.c_int, [P(PtBvhNode), C.c_uint32, P(C.c_float), C.c_uint32]),
    "pth_motion_table": (C.c_int, [P(PtHittable), P(PtHittable), C.c_uint32, P(C.c_float), P(C.c_uint32)]),
    "pth_renderer_render": (C.c_int, [C.c_void_p, P(PtCamera), C.c_uint32, C.c_uint32, C.c_int]),
    "pth_renderer_render_adaptive": (C.c_int, [C.c_void_p, P(PtCamera), P(PtAdaptiveParams), P(PtAdaptiveResult)]),
    "pth_renderer_adaptive": (C.c_int, [C.c_void_p]),
    "pth_renderer_features": (C.c_int, [C.c_void_p, P(PtCamera)]),
    "pth_renderer_feature_plane": (P(C.c_float), [C.c_void_p, C.c_uint32]),
    "pth_renderer_denoise": (C.c_int, [C.c_void_p, P(PtDenoiseParams), C.c_int, P(C.c_float)]),
    "pth_renderer_denoised": (C.c_int, [C.c_void_p]),
    "pth_renderer_temporal": (C.c_int, [C.c_void_p, P(PtTemporalParams), C.c_int, P(C.c_int)]),
    "pth_renderer_temporal_hdr": (P(C.c_float), [C.c_void_p]),
    "pth_renderer_temporal_moments": (C.c_int, [C.c_void_p, P(PtTemporalParams), P(PtVarianceParams), C.c_int, P(C.c_int)]),
    "pth_renderer_temporal_variance": (P(C.c_float), [C.c_void_p]),
    "pth_renderer_denoise_variance": (C.c_int, [C.c_void_p, P(PtVDenoiseParams)]),
    "pth_renderer_denoise_variance_feedback": (C.c_int, [C.c_void_p, P(PtVDenoiseParams), P(PtVFeedbackParams)]),
    "pth_renderer_temporal_history": (P(C.c_float), [C.c_void_p, C.c_uint32]),
    "pth_renderer_denoise_adaptive": (C.c_int, [C.c_void_p, P(PtAdaptiveVarianceParams), P(PtVDenoiseParams)]),
    "pth_renderer_adaptive_variance": (P(C.c_float), [C.c_void_p]),
    "pth_renderer_despike": (C.c_int, [C.c_void_p, P(PtDespikeParams)]),
    "pth_renderer_despike_count": (C.c_int, [C.c_void_p, P(C.c_uint32)]),
    "pth_renderer_upsample": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, P(PtUpsampleParams)]),
    "pth_renderer_upsample_resolve": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, P(PtUpsampleParams)]),
    "pth_renderer_upsample_counts": (C.c_int, [C.c_void_p, P(C.c_uint32)]),
    "pth_renderer_timing": (C.c_float, [C.c_void_p]),
    "pth_renderer_frames": (C.c_uint32, [C.c_void_p]),
    "pth_renderer_local_rows": (C.c_uint32, [C.c_void_p]),
    "pth_renderer_hdr": (P(C.c_float), [C.c_void_p]),
    "pth_renderer_image": (P(C.c_uint8), [C.c_void_p]),
    "pth_renderer_context": (C.c_void_p, [C.c_void_p]),
    "pth_renderer_group": (C.c_void_p, [C.c_void_p]),
    "pth_write_png": (C.c_int, [C.c_char_p, C.c_uint32, C.c_uint32, P(C.c_uint8), C.c_int]),
    "pth_write_hdr": (C.c_int, [C.c_char_p, C.c_uint32, C.c_uint32, P(C.c_float), C.c_int]),
}

_hip = None
_host = None


def _bind(lib: C.CDLL, table: dict) -> C.CDLL:
    for name, (res, args) in table.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


def mapped_hip_runtimes() -> list:
    """Distinct HIP runtime files (libamdhip64*) mapped into this process, from /proc/self/maps."""
    seen = []
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                parts = line.split(None, 5)
                if len(parts) == 6 and "/libamdhip64" in parts[5]:
                    path = os.path.realpath(parts[5].strip())
                    if path not in seen:
                        seen.append(path)
    except OSError:
        pass
    return seen


def check_single_runtime() -> None:
    """Raise PathtracerError when two HIP runtimes are mapped: two copies of the runtime in one process
    corrupt the heap at exit ("double free or corruption", rc 134)."""
    paths = mapped_hip_runtimes()
    if len(paths) > 1:
        raise PathtracerError(PT_ERR_STATE, "two HIP runtimes are mapped into this process ("
                              + ", ".join(paths) + "); load libpt_hip.so through pathtracercuda_amd._native.hip() "
                              "before any other HIP user, or import torch first")


def _unify_runtime() -> None:
    """Load the HIP runtime stack the process will use before libpt_hip.so binds one.

    The torch wheel ships its own libamdhip64 / librccl / libhsa-runtime64 and resolves them by file
    name through RPATH $ORIGIN, so a torch imported after libpt_hip.so maps a second runtime next to
    /opt/rocm's.  Preloading the wheel's files is not enough: with the wheel's own librccl.so mapped
    before libtorch_hip.so, the process aborts at exit ("double free or corruption", measured in this
    container with nothing else loaded).  So when torch is importable it is imported first, which is
    the configuration every test runs; libpt_hip.so then binds the wheel's runtime by soname
    (libamdhip64.so.7, librccl.so.1).  Without torch the system runtime (/opt/rocm) is used.
    """
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is not None:
        import torch  # noqa: F401


def hip() -> C.CDLL:
    global _hip
    if _hip is None:
        if not HIP_LIB.exists():
            raise RuntimeError(f"{HIP_LIB} is missing: build it with `make` (or __graft_entry__.build())")
        _unify_runtime()
        lib = C.CDLL(str(HIP_LIB), mode=C.RTLD_GLOBAL)
        check_single_runtime()
        _hip = _bind(lib, _HIP_SYMBOLS)
    return _hip


def host() -> C.CDLL:
    global _host
    if _host is None:
        hip()
        if not HOST_LIB.exists():
            raise RuntimeError(f"{HOST_LIB} is missing: build it with `make` (or __graft_entry__.build())")
        _host = _bind(C.CDLL(str(HOST_LIB)), _HOST_SYMBOLS)
    return _host


class PathtracerError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"[{code}] {message}")
        self.code = code


def check_host(rc: int) -> None:
    if rc != PT_OK:
        raise PathtracerError(rc, (host().pth_last_error() or b"").decode(errors="replace"))


def check_ctx(rc: int, ctx) -> None:
    if rc != PT_OK:
        raise PathtracerError(rc, (hip().pt_last_error(ctx) or b"").decode(errors="replace"))


def check_group(rc: int, group) -> None:
    if rc != PT_OK:
        raise PathtracerError(rc, (hip().pt_group_last_error(group) or b"").decode(errors="replace"))


def device_count() -> int:
    n = C.c_int(0)
    hip().pt_device_count(C.byref(n))
    return int(n.value)
