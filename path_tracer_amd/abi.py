"""ctypes mirror of include/pt_render.h — the C-ABI drop-in boundary of render() — and of include/pt_post.h (POST_SIGNATURES) and
include/pt_spatial_variance.h (SPATIAL_VARIANCE_SIGNATURES), include/pt_metrics.h (METRICS_SIGNATURES) and include/pt_encode.h
(ENCODE_SIGNATURES).

The structs are declared field-for-field as in the header; `load_library()` opens the
in-tree `libpt_render.so` built by `__graft_entry__.build()` (hipcc, gfx950) and fails
loudly when it is missing: there is no CPU fallback in the product path.

Reference boundary being replaced: `render<W,H,S>(queue, frame_buf, hittables, cam)`
(/root/reference include/render.hpp:141-160).
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

PT_ABI_VERSION = 2  # (1: rounds 1-5; the table structs did not change: scene_io loads both)

# tags — same numbering as the reference's std::variant alternatives
PT_HIT_SPHERE, PT_HIT_XY_RECT, PT_HIT_TRIANGLE, PT_HIT_BOX, PT_HIT_CONSTANT_MEDIUM = 0, 1, 2, 3, 4
PT_HIT_XZ_RECT, PT_HIT_YZ_RECT = 5, 6  # extension (rectangle.hpp:54,92 exist but are not hittable_t members)
PT_HIT_KIND_COUNT = 7
PT_MAT_LAMBERTIAN, PT_MAT_METAL, PT_MAT_DIELECTRIC, PT_MAT_LIGHTSOURCE, PT_MAT_ISOTROPIC = 0, 1, 2, 3, 4
PT_TEX_CHECKER, PT_TEX_SOLID, PT_TEX_IMAGE = 0, 1, 2

PT_TILE = 8
PT_TILE_PIXELS = 64
PT_TRI_MOLLER_TRUMBORE, PT_TRI_BADOUEL = 0, 1  # PtHittable.strategy of a triangle (triangle.hpp:102-103)
PT_FLAG_NONE = 0
PT_FLAG_NO_LDS = 1
PT_FLAG_FORCE_STREAM = 2
PT_FLAG_NO_FASTDIV = 4
PT_FLAG_TILE_GRANULAR = 8
PT_FLAG_PIXEL_GRANULAR = 16
PT_FLAG_NO_LPT = 32
PT_FLAG_NO_COOP = 64
PT_FLAG_FORCE_COOP = 128
PT_FLAG_NO_SPLIT = 256
PT_FLAG_FAST_RNG = 512  # opt-in decorrelated RNG streams: NOT the reference's image (include/pt_render.h)
PT_FAST_CHUNK_SPP = 64
PT_FLAG_SINGLE_STREAM = 1024  # the reference's USE_SINGLE_TASK executor: one RNG stream for the whole frame (small frames)

PT_OK, PT_ERR_INVALID_ARG, PT_ERR_BAD_SCENE, PT_ERR_HIP, PT_ERR_NO_DEVICE, PT_ERR_TOO_LARGE = range(6)
PT_BOUNCE_MISS, PT_BOUNCE_SCATTERED, PT_BOUNCE_ABSORBED = 0, 1, 2


class PtHittable(C.Structure):
    _fields_ = [("kind", C.c_int32), ("material", C.c_int32), ("boundary_kind", C.c_int32),
                ("strategy", C.c_int32), ("f", C.c_float * 12)]


class PtMaterial(C.Structure):
    _fields_ = [("kind", C.c_int32), ("texture", C.c_int32), ("color", C.c_float * 3),
                ("param", C.c_float), ("reserved", C.c_int32 * 2)]


class PtTexture(C.Structure):
    _fields_ = [("kind", C.c_int32), ("color0", C.c_float * 3), ("color1", C.c_float * 3),
                ("width", C.c_uint32), ("height", C.c_uint32), ("offset", C.c_uint32),
                ("freq", C.c_float), ("reserved", C.c_int32)]


class PtSceneDesc(C.Structure):
    _fields_ = [("hittables", C.POINTER(PtHittable)), ("n_hittables", C.c_int32),
                ("materials", C.POINTER(PtMaterial)), ("n_materials", C.c_int32),
                ("textures", C.POINTER(PtTexture)), ("n_textures", C.c_int32),
                ("reserved", C.c_int32),
                ("atlas", C.POINTER(C.c_uint8)), ("atlas_bytes", C.c_uint64)]


class PtCamera(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("lower_left_corner", C.c_float * 3),
                ("horizontal", C.c_float * 3), ("vertical", C.c_float * 3),
                ("u", C.c_float * 3), ("v", C.c_float * 3), ("w", C.c_float * 3),
                ("lens_radius", C.c_float), ("time0", C.c_float), ("time1", C.c_float)]


class PtRenderParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("samples", C.c_int32), ("depth", C.c_int32),
                ("shard_index", C.c_int32), ("shard_count", C.c_int32), ("flags", C.c_uint32),
                ("reserved", C.c_int32)]


class PtTuning(C.Structure):
    """include/pt_render.h PtTuning: performance-only knobs (same image under all of them).  Zero = the library's default."""
    _fields_ = [("struct_size", C.c_int32), ("sphere_grid", C.c_int32), ("grid_margin", C.c_float), ("grid_cell", C.c_float),
                ("slab_pools", C.c_int32), ("tri_pool", C.c_int32), ("tri_min_run", C.c_int32),
                ("tri_M", C.c_float), ("tri_binned", C.c_int32), ("tri_cell", C.c_float), ("tri_res", C.c_int32 * 3),
                ("generic_materials", C.c_int32), ("blocks_per_cu", C.c_int32), ("cold_state", C.c_int32),
                ("wide_log2_group", C.c_int32), ("split_tiles_mode", C.c_int32), ("split_tiles", C.c_int32),
                ("lpt_by_max", C.c_int32), ("probe_spp_max", C.c_int32), ("grid_min_tiles", C.c_int32),
                ("model_fixed", C.c_float), ("model_chain", C.c_float), ("scatter_log", C.c_int32), ("scatter_mode", C.c_int32),
                ("lanes_cap", C.c_int32), ("grid_walk", C.c_int32), ("heavy_tiles", C.c_int32),
                ("tri_rho", C.c_float * 2), ("tri_budget_mb", C.c_int32), ("tri_rho2", C.c_float), ("probe_resume", C.c_int32), ("chain_priority", C.c_int32), ("tri_cache", C.c_int32), ("sphere_merge", C.c_int32)]


def tuning(**fields) -> "PtTuning":
    """A PtTuning with the library's defaults (pt_tuning_init) and the given fields set."""
    t = PtTuning()
    load_library().pt_tuning_init(C.byref(t))
    for k, v in fields.items():
        if k == "tri_res":
            t.tri_res[:] = list(v)
        elif k == "tri_rho":
            t.tri_rho[:] = list(v)
        else:
            setattr(t, k, v)
    return t


class PtBounceIn(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("dir", C.c_float * 3), ("time", C.c_float),
                ("rng_state", C.c_uint32), ("attenuation", C.c_float * 3)]


class PtBounceOut(C.Structure):
    _fields_ = [("status", C.c_int32), ("hittable", C.c_int32), ("material", C.c_int32), ("front_face", C.c_int32),
                ("t", C.c_float), ("p", C.c_float * 3), ("normal", C.c_float * 3), ("u", C.c_float), ("v", C.c_float),
                ("color", C.c_float * 3), ("sc_origin", C.c_float * 3), ("sc_dir", C.c_float * 3),
                ("sc_time", C.c_float), ("rng_state", C.c_uint32)]


class PtCameraRay(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("dir", C.c_float * 3), ("time", C.c_float), ("rng_state", C.c_uint32)]


class PtAovBuffers(C.Structure):
    """include/pt_render.h PtAovBuffers: device pointers of the planes pt_render_aov writes (NULL = plane not wanted)."""
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("albedo", C.c_void_p), ("normal", C.c_void_p),
                ("direct", C.c_void_p), ("depth", C.c_void_p), ("coverage", C.c_void_p), ("id", C.c_void_p)]


class PtDenoiseParams(C.Structure):
    """include/pt_render.h PtDenoiseParams: the a-trous denoiser's parameters (pt_denoise); a sigma <= 0 turns its term off."""
    _fields_ = [("struct_size", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("iterations", C.c_int32),
                ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float), ("sigma_albedo", C.c_float),
                ("flags", C.c_uint32), ("reserved", C.c_int32)]


class PtVarianceDenoiseParams(C.Structure):
    """include/pt_render.h PtVarianceDenoiseParams: the variance-guided denoiser's parameters (pt_variance_denoise); a sigma <= 0
    turns its term off."""
    _fields_ = [("struct_size", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("iterations", C.c_int32),
                ("sigma_variance", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float), ("sigma_albedo", C.c_float),
                ("flags", C.c_uint32), ("reserved", C.c_int32)]


class PtTemporalParams(C.Structure):
    """include/pt_render.h PtTemporalParams: the temporal reprojection's parameters (pt_temporal_push)."""
    _fields_ = [("struct_size", C.c_int32), ("alpha", C.c_float), ("tol_depth", C.c_float), ("tol_normal", C.c_float),
                ("flags", C.c_uint32), ("reserved", C.c_int32 * 3)]


class PtDisplayParams(C.Structure):
    """include/pt_render.h PtDisplayParams: the display stage's parameters (pt_display_meter, pt_display_apply)."""
    _fields_ = [("struct_size", C.c_int32), ("tone", C.c_int32), ("flags", C.c_uint32), ("ev_bias", C.c_float), ("ev_min", C.c_float),
                ("ev_max", C.c_float), ("lo_permille", C.c_int32), ("hi_permille", C.c_int32), ("adapt_up", C.c_float),
                ("adapt_down", C.c_float), ("white", C.c_float), ("rect_x0", C.c_int32), ("rect_y0", C.c_int32), ("rect_x1", C.c_int32),
                ("rect_y1", C.c_int32), ("reserved", C.c_int32)]


class PtFireflyParams(C.Structure):
    """include/pt_post.h PtFireflyParams: the firefly stage's parameters (pt_firefly)."""
    _fields_ = [("struct_size", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("rank", C.c_int32), ("k", C.c_float),
                ("flags", C.c_uint32), ("reserved", C.c_int32 * 2)]


class PtSpatialVarianceParams(C.Structure):
    """include/pt_spatial_variance.h PtSpatialVarianceParams: the spatial variance estimate's parameters (pt_spatial_variance)."""
    _fields_ = [("struct_size", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("radius", C.c_int32), ("min_pairs", C.c_int32),
                ("tol_depth", C.c_float), ("tol_normal", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_int32 * 2)]


class PtImageErrorParams(C.Structure):
    """include/pt_metrics.h PtImageErrorParams: the image error's parameters (pt_image_error)."""
    _fields_ = [("struct_size", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("rect_x0", C.c_int32), ("rect_y0", C.c_int32),
                ("rect_x1", C.c_int32), ("rect_y1", C.c_int32), ("flags", C.c_uint32), ("eps", C.c_double), ("scratch_bytes", C.c_int64),
                ("reserved", C.c_int32 * 2)]


class PtImageErrorResult(C.Structure):
    """include/pt_metrics.h PtImageErrorResult: what pt_image_error leaves on the device."""
    _fields_ = [("sum_sq", C.c_double * 3), ("sum_abs", C.c_double * 3), ("sum_rel", C.c_double * 3), ("pixels", C.c_uint64),
                ("skipped", C.c_uint64), ("max_abs", C.c_float * 3), ("reserved", C.c_uint32)]


class PtEncodeParams(C.Structure):
    """include/pt_encode.h PtEncodeParams: the encode stage's parameters (pt_encode, pt_display_encode)."""
    _fields_ = [("struct_size", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("transfer", C.c_int32), ("flags", C.c_uint32),
                ("phase_x", C.c_int32), ("phase_y", C.c_int32), ("reserved", C.c_int32)]


assert C.sizeof(PtHittable) == 64 and C.sizeof(PtMaterial) == 32 and C.sizeof(PtTexture) == 48
assert C.sizeof(PtCamera) == 96 and C.sizeof(PtRenderParams) == 32

_FP = C.POINTER(C.c_float)
_SCENE_P = C.c_void_p

# name -> (restype, argtypes): every entry point include/pt_render.h declares
SIGNATURES = {
    "pt_abi_version": (C.c_int, []),
    "pt_error_string": (C.c_char_p, [C.c_int]),
    "pt_last_error": (C.c_char_p, []),
    "pt_camera_init": (C.c_int, [C.POINTER(PtCamera), _FP, _FP, _FP, C.c_float, C.c_float, C.c_float, C.c_float,
                                 C.c_float, C.c_float]),
    "pt_scene_create": (C.c_int, [C.POINTER(PtSceneDesc), C.POINTER(_SCENE_P)]),
    "pt_scene_create_tuned": (C.c_int, [C.POINTER(PtSceneDesc), C.POINTER(PtTuning), C.POINTER(_SCENE_P)]),
    "pt_tuning_init": (None, [C.POINTER(PtTuning)]),
    "pt_tuning_from_env": (None, [C.POINTER(PtTuning)]),
    "pt_debug_flatten_tuned": (C.c_int, [C.POINTER(PtSceneDesc), C.POINTER(PtTuning), _FP, C.c_int64, C.POINTER(C.c_int32),
                                         C.POINTER(C.c_int32), _FP, C.c_int64, C.POINTER(C.c_int32)]),
    "pt_scene_destroy": (None, [_SCENE_P]),
    "pt_scene_device_bytes": (C.c_int64, [_SCENE_P]),
    "pt_build_id": (C.c_char_p, []),
    "pt_scene_reserve": (C.c_int, [_SCENE_P, C.POINTER(PtRenderParams)]),
    "pt_fast_seed": (C.c_uint32, [C.c_uint32, C.c_uint32]),
    "pt_framebuffer_floats": (C.c_int64, [C.POINTER(PtRenderParams)]),
    "pt_shard_tiles": (C.c_int32, [C.POINTER(PtRenderParams)]),
    "pt_render": (C.c_int, [_SCENE_P, C.POINTER(PtCamera), C.POINTER(PtRenderParams), C.c_void_p, C.c_void_p]),
    "pt_render_timed": (C.c_int, [_SCENE_P, C.POINTER(PtCamera), C.POINTER(PtRenderParams), C.c_void_p, C.c_void_p,
                                  C.POINTER(C.c_float)]),
    "pt_render_host": (C.c_int, [_SCENE_P, C.POINTER(PtCamera), C.POINTER(PtRenderParams), _FP]),
    "pt_unshard_tiles": (C.c_int, [C.c_void_p, C.POINTER(PtRenderParams), C.c_void_p, C.c_void_p]),
    "pt_tonemap_rgb8": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "pt_debug_bounce": (C.c_int, [_SCENE_P, C.POINTER(PtBounceIn), C.POINTER(PtBounceOut), C.c_int32]),
    "pt_debug_camera_rays": (C.c_int, [C.POINTER(PtCamera), C.c_int32, C.c_int32, C.POINTER(C.c_int32),
                                       C.POINTER(C.c_uint32), C.POINTER(PtCameraRay), C.c_int32]),
    "pt_debug_schedule": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "pt_debug_last_launch": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "pt_debug_last_kernels": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "pt_debug_flatten": (C.c_int, [C.POINTER(PtSceneDesc), _FP, C.c_int64, C.POINTER(C.c_int32),
                                   C.POINTER(C.c_int32), _FP, C.c_int64, C.POINTER(C.c_int32)]),
    "pt_debug_math": (C.c_int, [C.c_int32, _FP, _FP, _FP, C.c_int64]),
    "pt_debug_sphere_texel": (C.c_int, [_FP, C.c_int64, C.c_float, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                        C.POINTER(C.c_uint8), _FP]),
    "pt_debug_tri_pool": (C.c_int, [C.POINTER(PtSceneDesc), C.POINTER(C.c_int32)]),
    "pt_debug_flatten_pool": (C.c_int, [C.POINTER(PtSceneDesc), C.POINTER(PtTuning), C.POINTER(C.c_float), C.c_int64, C.POINTER(C.c_int64)]),
    # progressive rendering (PtAccum): added without an ABI version change, so loaded optionally (ACCUM_SYMBOLS)
    "pt_accum_create": (C.c_int, [_SCENE_P, C.POINTER(PtRenderParams), C.POINTER(C.c_void_p)]),
    "pt_accum_destroy": (None, [C.c_void_p]),
    "pt_accum_reset": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pt_accum_samples": (C.c_int32, [C.c_void_p]),
    "pt_render_accumulate": (C.c_int, [C.c_void_p, C.POINTER(PtCamera), C.c_int32, C.c_void_p]),
    "pt_accum_resolve": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "pt_accum_tonemap_rgb8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "pt_accum_state_bytes": (C.c_int64, [C.POINTER(PtRenderParams)]),
    "pt_accum_export": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "pt_accum_import": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    # adaptive sampling (a PtAccum with per-pixel counts): likewise optional (ADAPTIVE_SYMBOLS)
    "pt_adaptive_create": (C.c_int, [_SCENE_P, C.POINTER(PtRenderParams), C.POINTER(C.c_void_p)]),
    "pt_adaptive_window": (C.c_int, [C.c_void_p, C.POINTER(PtCamera), C.c_int32, C.c_void_p, C.c_void_p]),
    "pt_adaptive_counts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "pt_adaptive_error": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "pt_adaptive_select": (C.c_int, [C.c_void_p, C.c_float, C.c_int32, C.c_int32, C.c_uint32, C.c_void_p, C.POINTER(C.c_int64),
                                     C.c_void_p]),
    "pt_adaptive_state_bytes": (C.c_int64, [C.POINTER(PtRenderParams)]),
    "pt_adaptive_export": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "pt_adaptive_import": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    # first-hit feature buffers (AOVs): likewise optional (AOV_SYMBOLS)
    "pt_aov_plane_elems": (C.c_int64, [C.POINTER(PtRenderParams), C.c_int32]),
    "pt_debug_last_aov": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "pt_render_aov": (C.c_int, [_SCENE_P, C.POINTER(PtCamera), C.POINTER(PtRenderParams), C.POINTER(PtAovBuffers), C.c_void_p]),
    # the a-trous denoiser: likewise optional (DENOISE_SYMBOLS)
    "pt_denoise_params_init": (None, [C.POINTER(PtDenoiseParams), C.c_int32, C.c_int32]),
    "pt_denoise_scratch_floats": (C.c_int64, [C.c_int32, C.c_int32]),
    "pt_denoise": (C.c_int, [C.POINTER(PtDenoiseParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pt_debug_last_denoise": (C.c_int, [C.POINTER(C.c_int32)]),
    # the variance-guided denoiser and the estimate that feeds it: likewise optional (VARIANCE_SYMBOLS)
    "pt_variance_estimate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "pt_variance_denoise_params_init": (None, [C.POINTER(PtVarianceDenoiseParams), C.c_int32, C.c_int32]),
    "pt_variance_denoise_scratch_floats": (C.c_int64, [C.c_int32, C.c_int32]),
    "pt_variance_denoise": (C.c_int, [C.POINTER(PtVarianceDenoiseParams)] + [C.c_void_p] * 9),
    "pt_debug_last_variance_denoise": (C.c_int, [C.POINTER(C.c_int32)]),
    # temporal reprojection and the frame that continues every pixel's stream: likewise optional (TEMPORAL_SYMBOLS)
    "pt_adaptive_next_frame": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pt_temporal_params_init": (None, [C.POINTER(PtTemporalParams)]),
    "pt_temporal_state_bytes": (C.c_int64, [C.c_int32, C.c_int32]),
    "pt_temporal_create": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "pt_temporal_destroy": (None, [C.c_void_p]),
    "pt_temporal_reset": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pt_temporal_frames": (C.c_int32, [C.c_void_p]),
    "pt_temporal_push": (C.c_int, [C.c_void_p, C.POINTER(PtTemporalParams), C.POINTER(PtCamera)] + [C.c_void_p] * 9),
    # the display stage (histogram auto-exposure, tone curves): likewise optional (DISPLAY_SYMBOLS)
    "pt_display_params_init": (None, [C.POINTER(PtDisplayParams)]),
    "pt_display_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "pt_display_destroy": (None, [C.c_void_p]),
    "pt_display_reset": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pt_display_frames": (C.c_int32, [C.c_void_p]),
    "pt_display_meter": (C.c_int, [C.c_void_p, C.POINTER(PtDisplayParams), C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "pt_display_set_exposure": (C.c_int, [C.c_void_p, C.c_float, C.c_void_p]),
    "pt_display_apply": (C.c_int, [C.c_void_p, C.POINTER(PtDisplayParams), C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pt_display_exposure": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_void_p]),
    "pt_display_histogram": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p]),
    "pt_debug_last_display": (C.c_int, [C.POINTER(C.c_int32)]),
    # the launcher's geometry rules for one pass, host-only: likewise optional (PLAN_SYMBOLS)
    "pt_debug_plan_pass": (C.c_int, [C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    # the one-pool plan of rect / box-only scenes, as the last frame pass got it and as derived without a device: likewise optional (POOL_PLAN_SYMBOLS)
    "pt_debug_last_pool_plan": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "pt_debug_last_pool_word": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "pt_debug_pool_plan": (C.c_int, [C.POINTER(PtSceneDesc), C.POINTER(PtTuning), C.POINTER(PtRenderParams), C.POINTER(C.c_int32)]),
    # the shade table of a small rect / box-only scene, host-only (csrc/pt_flatten.hpp: Flat::shade)
    "pt_debug_shade_table": (C.c_int, [C.POINTER(PtSceneDesc), C.POINTER(PtTuning), _FP, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
}

# name -> (restype, argtypes): every entry point include/pt_post.h declares — the image-space stages added since pt_render.h's table was
# closed.  A table of its own: SIGNATURES stays exactly what pt_render.h declares.  Optional, like DISPLAY_SYMBOLS: load_library() applies a
# row where the library exports the symbol; has_firefly() tells whether the loaded one has the stage.
POST_SIGNATURES = {
    "pt_firefly_params_init": (None, [C.POINTER(PtFireflyParams), C.c_int32, C.c_int32]),
    "pt_firefly": (C.c_int, [C.POINTER(PtFireflyParams)] + [C.c_void_p] * 6),
    "pt_debug_last_firefly": (C.c_int, [C.POINTER(C.c_int32)]),
}
FIREFLY_SYMBOLS = frozenset({"pt_firefly_params_init", "pt_firefly", "pt_debug_last_firefly"})
PT_FIREFLY_REPAIR = 1
PT_FIREFLY_NO_LDS = 2  # A/B switch, same bits: every neighbour from global memory
PT_FIREFLY_TILE_W, PT_FIREFLY_TILE_H = 32, 8
# the header's PT_FIREFLY_DEFAULT_* (pt_firefly_params_init)
PT_FIREFLY_DEFAULT_RANK, PT_FIREFLY_DEFAULT_K, PT_FIREFLY_DEFAULT_FLAGS = 1, 1.0, PT_FIREFLY_REPAIR

# name -> (restype, argtypes): every entry point include/pt_spatial_variance.h declares.  A table of its own, like POST_SIGNATURES and for
# its reason: SIGNATURES and POST_SIGNATURES stay exactly what their headers declare.  load_library() applies a row where the library
# exports the symbol; has_spatial_variance() tells whether the loaded one has the stage.
SPATIAL_VARIANCE_SIGNATURES = {
    "pt_spatial_variance_params_init": (None, [C.POINTER(PtSpatialVarianceParams), C.c_int32, C.c_int32]),
    "pt_spatial_variance": (C.c_int, [C.POINTER(PtSpatialVarianceParams)] + [C.c_void_p] * 9),
    "pt_debug_last_spatial_variance": (C.c_int, [C.POINTER(C.c_int32)]),
}
SPATIAL_VARIANCE_SYMBOLS = frozenset(SPATIAL_VARIANCE_SIGNATURES)
PT_SVAR_DEMODULATE = 1
PT_SVAR_NO_LDS = 2  # A/B switch, same bits: the window from global memory
PT_SVAR_MAX_RADIUS = 3
PT_SVAR_TILE_W, PT_SVAR_TILE_H = 32, 8
# the header's PT_SVAR_DEFAULT_* (pt_spatial_variance_params_init)
PT_SVAR_DEFAULT_RADIUS, PT_SVAR_DEFAULT_MIN_PAIRS, PT_SVAR_DEFAULT_TOL_DEPTH, PT_SVAR_DEFAULT_TOL_NORMAL = 2, 4, 0.1, 0.5
PT_SVAR_DEFAULT_FLAGS = PT_SVAR_DEMODULATE

# name -> (restype, argtypes): every entry point include/pt_metrics.h declares.  A table of its own, like SPATIAL_VARIANCE_SIGNATURES and
# for its reason.  load_library() applies a row where the library exports the symbol; has_metrics() tells whether the loaded one has the
# stage.
METRICS_SIGNATURES = {
    "pt_image_error_params_init": (None, [C.POINTER(PtImageErrorParams), C.c_int32, C.c_int32]),
    "pt_image_error_scratch_bytes": (C.c_int64, []),
    "pt_image_error": (C.c_int, [C.POINTER(PtImageErrorParams)] + [C.c_void_p] * 6),
    "pt_debug_last_image_error": (C.c_int, [C.POINTER(C.c_int32)]),
}
METRICS_SYMBOLS = frozenset(METRICS_SIGNATURES)
PT_IMAGE_ERROR_NO_LDS = 1  # A/B switch, same bits: global atomics only
PT_IMAGE_ERROR_WORDS, PT_IMAGE_ERROR_SUMS = 68, 9
PT_IMAGE_ERROR_DEFAULT_EPS = 1e-4  # the header's (pt_image_error_params_init)

# name -> (restype, argtypes): every entry point include/pt_encode.h declares.  A table of its own, like METRICS_SIGNATURES and for its
# reason.  load_library() applies a row where the library exports the symbol; has_encode() tells whether the loaded one has the stage.
ENCODE_SIGNATURES = {
    "pt_encode_params_init": (None, [C.POINTER(PtEncodeParams), C.c_int32, C.c_int32]),
    "pt_encode": (C.c_int, [C.POINTER(PtEncodeParams), C.c_void_p, C.c_void_p, C.c_void_p]),
    "pt_display_encode": (C.c_int, [C.c_void_p, C.POINTER(PtDisplayParams), C.POINTER(PtEncodeParams), C.c_void_p, C.c_void_p, C.c_void_p]),
    "pt_debug_last_encode": (C.c_int, [C.POINTER(C.c_int32)]),
}
ENCODE_SYMBOLS = frozenset(ENCODE_SIGNATURES)
PT_TRANSFER_REFERENCE, PT_TRANSFER_SRGB = 0, 1
TRANSFERS = {"reference": PT_TRANSFER_REFERENCE, "srgb": PT_TRANSFER_SRGB}
PT_ENCODE_DITHER = 1
PT_ENCODE_NO_VEC = 2  # A/B switch, same bits: one value per lane
# the header's PT_ENCODE_DEFAULT_* (pt_encode_params_init)
PT_ENCODE_DEFAULT_TRANSFER, PT_ENCODE_DEFAULT_FLAGS = PT_TRANSFER_SRGB, 0

# Entry points a library may lack and still load for everything else (include/pt_render.h: the feature is detected by their presence);
# has_accumulator() tells whether the loaded one has them.
ACCUM_SYMBOLS = frozenset(n for n in SIGNATURES if n.startswith("pt_accum_") or n == "pt_render_accumulate")
PT_ACCUM_MAGIC = 0x43415450
PT_ACCUM_FORMAT = 1
PT_ACCUM_HEADER_BYTES = 160
# adaptive sampling (include/pt_render.h: pt_adaptive_*); has_adaptive() tells whether the loaded library has them
# (pt_adaptive_next_frame came later and is detected with temporal reprojection: TEMPORAL_SYMBOLS)
ADAPTIVE_SYMBOLS = frozenset(n for n in SIGNATURES if n.startswith("pt_adaptive_") and n != "pt_adaptive_next_frame")
PT_ADAPTIVE_FORMAT = 2
PT_ADAPTIVE_DILATE = 1
# first-hit feature buffers (include/pt_render.h: pt_render_aov); has_aov() tells whether the loaded library has them
AOV_SYMBOLS = frozenset({"pt_aov_plane_elems", "pt_render_aov", "pt_debug_last_aov"})
AOV_PLANES = ("albedo", "normal", "direct", "depth", "coverage", "id")  # PtAovBuffers' planes, in the struct's order
AOV_CHANNELS = {"albedo": 3, "normal": 3, "direct": 3, "depth": 1, "coverage": 1, "id": 1}
# the a-trous denoiser (include/pt_render.h: pt_denoise); has_denoise() tells whether the loaded library has it
DENOISE_SYMBOLS = frozenset({"pt_denoise_params_init", "pt_denoise_scratch_floats", "pt_denoise", "pt_debug_last_denoise"})
# the launcher's planner as an entry point (include/pt_render.h: pt_debug_plan_pass): the order of its facts and of its output words
PLAN_SYMBOLS = frozenset({"pt_debug_plan_pass"})
# the one-pool plan's read-backs (include/pt_render.h: pt_debug_last_pool_plan, pt_debug_pool_plan) and the order of the latter's words
POOL_PLAN_SYMBOLS = frozenset({"pt_debug_last_pool_plan", "pt_debug_pool_plan"})
POOL_PLAN_WORDS = ("one", "n", "x_off", "oct_off", "pool_off", "bmax_bits", "kind", "off", "count", "scene_allows", "lds", "mats")
PLAN_FACTS = ("num_cus", "per_cu", "block_threads", "chain_bound", "use_grid", "queued_walk", "flags", "blocks_per_cu", "lanes_cap", "heavy_tiles",
              "no_chain_prio", "launch_units", "n_local_pixels", "samples", "probe", "has_order", "has_split", "tile_granular", "scatter_p", "fast_chunks")
PLAN_WORDS = ("workgroups", "n_waves_resident", "lanes_cap", "tile_granular", "heavy_pixels", "heavy_lanes", "prio_onset", "prio_t1", "prio_t2",
              "prio_t3", "last_workgroups", "last_lanes_cap", "last_heavy_pixels", "last_queued_walk")
PT_DENOISE_DEMODULATE = 1
PT_DENOISE_NO_LDS = 2  # A/B switch, same bits: every iteration reads its taps from global memory
PT_DENOISE_MAX_ITERATIONS = 8
# the header's PT_DENOISE_DEFAULT_* (pt_denoise_params_init)
PT_DENOISE_DEFAULT_ITERATIONS = 5
PT_DENOISE_DEFAULT_SIGMA_COLOR, PT_DENOISE_DEFAULT_SIGMA_NORMAL, PT_DENOISE_DEFAULT_SIGMA_DEPTH, PT_DENOISE_DEFAULT_SIGMA_ALBEDO = 32.0, 0.5, 0.2, 0.0
# the variance-guided denoiser (include/pt_render.h: pt_variance_estimate, pt_variance_denoise); has_variance_denoise() tells whether the
# loaded library has it
VARIANCE_SYMBOLS = frozenset({"pt_variance_estimate", "pt_variance_denoise_params_init", "pt_variance_denoise_scratch_floats",
                              "pt_variance_denoise", "pt_debug_last_variance_denoise"})
PT_VDENOISE_DEMODULATE = 1
PT_VDENOISE_NO_LDS = 2  # A/B switch, same bits: every iteration reads from global memory
PT_VDENOISE_MAX_ITERATIONS = 8
# the header's PT_VDENOISE_DEFAULT_* (pt_variance_denoise_params_init)
PT_VDENOISE_DEFAULT_ITERATIONS = 5
PT_VDENOISE_DEFAULT_SIGMA_VARIANCE, PT_VDENOISE_DEFAULT_SIGMA_NORMAL, PT_VDENOISE_DEFAULT_SIGMA_DEPTH, PT_VDENOISE_DEFAULT_SIGMA_ALBEDO = 2.0, 0.5, 0.2, 0.0

# temporal reprojection (include/pt_render.h: pt_adaptive_next_frame, pt_temporal_*); has_temporal() tells whether the loaded library has it
TEMPORAL_SYMBOLS = frozenset({"pt_adaptive_next_frame", "pt_temporal_params_init", "pt_temporal_state_bytes", "pt_temporal_create",
                              "pt_temporal_destroy", "pt_temporal_reset", "pt_temporal_frames", "pt_temporal_push"})
# the header's PT_TEMPORAL_DEFAULT_* (pt_temporal_params_init)
PT_TEMPORAL_DEFAULT_ALPHA, PT_TEMPORAL_DEFAULT_TOL_DEPTH, PT_TEMPORAL_DEFAULT_TOL_NORMAL = 0.1, 0.1, 0.5

# the display stage (include/pt_render.h: pt_display_*); has_display() tells whether the loaded library has it
DISPLAY_SYMBOLS = frozenset({"pt_display_params_init", "pt_display_create", "pt_display_destroy", "pt_display_reset", "pt_display_frames",
                             "pt_display_meter", "pt_display_set_exposure", "pt_display_apply", "pt_display_exposure", "pt_display_histogram",
                             "pt_debug_last_display"})
PT_TONE_REFERENCE, PT_TONE_REINHARD, PT_TONE_ACES = 0, 1, 2
TONES = {"reference": PT_TONE_REFERENCE, "reinhard": PT_TONE_REINHARD, "aces": PT_TONE_ACES}
# the header's PT_DISPLAY_DEFAULT_* (pt_display_params_init)
PT_DISPLAY_DEFAULT_TONE = PT_TONE_ACES
PT_DISPLAY_DEFAULT_EV_BIAS, PT_DISPLAY_DEFAULT_EV_MIN, PT_DISPLAY_DEFAULT_EV_MAX = 0.0, -16.0, 16.0
PT_DISPLAY_DEFAULT_LO_PERMILLE, PT_DISPLAY_DEFAULT_HI_PERMILLE = 400, 950
PT_DISPLAY_DEFAULT_ADAPT_UP, PT_DISPLAY_DEFAULT_ADAPT_DOWN, PT_DISPLAY_DEFAULT_WHITE = 1.0, 1.0, 4.0

LIB_NAME = "libpt_render.so"
_lib = None


class PtError(RuntimeError):
    """A pt_* entry point returned a non-zero code (the reference's `void` + asserts, made explicit)."""

    def __init__(self, code: int, where: str, detail: str = ""):
        self.code = code
        super().__init__(f"{where}: error {code}" + (f" ({detail})" if detail else ""))


def library_path() -> Path:
    override = os.environ.get("PT_RENDER_LIB")
    return Path(override) if override else Path(__file__).resolve().parent / LIB_NAME


def override_is_older_build(path, lib, name) -> bool:
    """A/B tooling only (tools/abn.sh loads an OLDER build of the extension through PT_RENDER_LIB): entry points added since
    that build may be missing there.  The in-tree library must export everything include/pt_render.h declares."""
    return bool(os.environ.get("PT_RENDER_LIB")) and os.environ.get("PT_RENDER_LIB_ALLOW_OLDER") == "1" and not hasattr(lib, name)


def load_library() -> C.CDLL:
    """Open the HIP extension.  Fails loudly: the product has no CPU path."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not path.exists():
        raise ImportError(
            f"{path} is missing: the gfx950 HIP extension has not been built. "
            "Run `python -c 'import __graft_entry__ as g; g.build()'` (hipcc cross-compiles without a GPU).")
    # PyTorch ships its own copy of the HIP runtime (torch/lib/libamdhip64.so, SONAME libamdhip64.so.7).  Two
    # HIP runtimes in one process cannot both see the GPU, and torch asks for its copy by file name, so the
    # order matters: with torch loaded first the loader binds this library's libamdhip64.so.7 dependency to
    # torch's copy by SONAME; loaded the other way round the process would end up with two runtimes.
    try:
        import torch  # noqa: F401  (plumbing: device memory, streams, RCCL)
    except ImportError:
        pass  # torch-free hosts bind to /opt/rocm/lib through the library's RUNPATH
    lib = C.CDLL(str(path))
    for name, (res, args) in SIGNATURES.items():
        if override_is_older_build(path, lib, name) or (name in ACCUM_SYMBOLS | ADAPTIVE_SYMBOLS | AOV_SYMBOLS | DENOISE_SYMBOLS | PLAN_SYMBOLS | POOL_PLAN_SYMBOLS | VARIANCE_SYMBOLS | TEMPORAL_SYMBOLS | DISPLAY_SYMBOLS and not hasattr(lib, name)):
            continue
        fn = getattr(lib, name)  # AttributeError if the library does not export what the header declares
        fn.restype = res
        fn.argtypes = args
    for name, (res, args) in list(POST_SIGNATURES.items()) + list(SPATIAL_VARIANCE_SIGNATURES.items()) + list(METRICS_SIGNATURES.items()) + list(ENCODE_SIGNATURES.items()):  # include/pt_post.h, pt_spatial_variance.h, pt_metrics.h, pt_encode.h: applied where the library has the symbol
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
    older_ok = bool(os.environ.get("PT_RENDER_LIB")) and os.environ.get("PT_RENDER_LIB_ALLOW_OLDER") == "1"  # (A/B tooling: an older build beside this tree)
    if lib.pt_abi_version() != PT_ABI_VERSION and not (older_ok and lib.pt_abi_version() == 1):
        raise ImportError(f"{path}: ABI version {lib.pt_abi_version()} != {PT_ABI_VERSION}")
    _lib = lib
    return lib


def has_accumulator(lib=None) -> bool:
    """Does the loaded library offer progressive rendering (the PtAccum entry points)?"""
    lib = lib or load_library()
    return all(hasattr(lib, n) for n in ACCUM_SYMBOLS)


def has_adaptive(lib=None) -> bool:
    """Does the loaded library offer adaptive sampling (the pt_adaptive_* entry points)?"""
    lib = lib or load_library()
    return has_accumulator(lib) and all(hasattr(lib, n) for n in ADAPTIVE_SYMBOLS)


def has_aov(lib=None) -> bool:
    """Does the loaded library offer the first-hit feature buffers (pt_render_aov)?"""
    lib = lib or load_library()
    return all(hasattr(lib, n) for n in AOV_SYMBOLS)


def has_denoise(lib=None) -> bool:
    """Does the loaded library offer the a-trous denoiser (pt_denoise)?"""
    lib = lib or load_library()
    return all(hasattr(lib, n) for n in DENOISE_SYMBOLS)


def has_variance_denoise(lib=None) -> bool:
    """Does the loaded library offer the variance-guided denoiser (pt_variance_estimate, pt_variance_denoise)?"""
    lib = lib or load_library()
    return all(hasattr(lib, n) for n in VARIANCE_SYMBOLS)


def has_temporal(lib=None) -> bool:
    """Does the loaded library offer temporal reprojection (pt_adaptive_next_frame, pt_temporal_push)?"""
    lib = lib or load_library()
    return has_adaptive(lib) and all(hasattr(lib, n) for n in TEMPORAL_SYMBOLS)


def has_display(lib=None) -> bool:
    """Does the loaded library offer the display stage (pt_display_meter, pt_display_apply)?"""
    lib = lib or load_library()
    return all(hasattr(lib, n) for n in DISPLAY_SYMBOLS)


def has_firefly(lib=None) -> bool:
    """Does the loaded library offer the firefly stage (include/pt_post.h: pt_firefly)?"""
    lib = lib or load_library()
    return all(hasattr(lib, n) for n in FIREFLY_SYMBOLS)


def has_spatial_variance(lib=None) -> bool:
    """Does the loaded library offer the spatial variance estimate (include/pt_spatial_variance.h: pt_spatial_variance)?"""
    lib = lib or load_library()
    return all(hasattr(lib, n) for n in SPATIAL_VARIANCE_SYMBOLS)


def has_metrics(lib=None) -> bool:
    """Does the loaded library offer the image error (include/pt_metrics.h: pt_image_error)?"""
    lib = lib or load_library()
    return all(hasattr(lib, n) for n in METRICS_SYMBOLS)


def has_encode(lib=None) -> bool:
    """Does the loaded library offer the encode stage (include/pt_encode.h: pt_encode, pt_display_encode)?"""
    lib = lib or load_library()
    return has_display(lib) and all(hasattr(lib, n) for n in ENCODE_SYMBOLS)


def check(code: int, where: str) -> None:
    if code != PT_OK:
        lib = load_library()
        detail = lib.pt_last_error().decode() or lib.pt_error_string(code).decode()
        raise PtError(code, where, detail)
