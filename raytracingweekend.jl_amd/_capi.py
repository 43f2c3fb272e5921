"""ctypes binding of librtw_hip.so (C ABI: include/rtw_hip.h).  No fallback of any kind."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RTW_HIP_LIB") or os.path.join(_HERE, "lib", "librtw_hip.so")   # env: kernel A/B experiments only

#: every symbol include/rtw_hip.h declares
SYMBOLS = [
    "rtw_abi_version", "rtw_device_count", "rtw_last_error", "rtw_render_f32", "rtw_render_f64",
    "rtw_scene_upload_f32", "rtw_scene_upload_f64", "rtw_scene_free", "rtw_render_device_f32",
    "rtw_render_device_f64", "rtw_stats", "rtw_stats_devices", "rtw_unit_f32", "rtw_unit_f64", "rtw_shutdown",
    "rtw_render_batch_f32", "rtw_render_batch_f64", "rtw_render_batch_device_f32", "rtw_render_batch_device_f64",
    "rtw_accum_create", "rtw_accum_reset", "rtw_accum_free", "rtw_render_accum_f32", "rtw_render_accum_f64",
    "rtw_accum_resolve_f32", "rtw_accum_resolve_f64", "rtw_accum_resolve_host_f32", "rtw_accum_resolve_host_f64",
    "rtw_accum_merge", "rtw_accum_info", "rtw_accum_ranges", "rtw_accum_read_pixels", "rtw_accum_export", "rtw_accum_import",
    "rtw_render_adaptive_f32", "rtw_render_adaptive_f64", "rtw_accum_adaptive_info", "rtw_accum_tile_chunks",
    "rtw_render_accum_batch_f32", "rtw_render_accum_batch_f64", "rtw_render_adaptive_batch_f32", "rtw_render_adaptive_batch_f64",
    "rtw_render_features_device_f32", "rtw_render_features_device_f64", "rtw_render_features_f32", "rtw_render_features_f64",
    "rtw_denoise_work_bytes", "rtw_denoise_device_f32", "rtw_denoise_device_f64", "rtw_denoise_f32", "rtw_denoise_f64",
    "rtw_render_denoised_f32", "rtw_render_denoised_f64",
    "rtw_accum_features_f32", "rtw_accum_features_f64", "rtw_accum_noise_f32", "rtw_accum_noise_f64",
    "rtw_guided_filter_device_f32", "rtw_guided_filter_device_f64", "rtw_accum_filtered_f32", "rtw_accum_filtered_f64",
    "rtw_render_features_batch_device_f32", "rtw_render_features_batch_device_f64", "rtw_render_features_batch_f32", "rtw_render_features_batch_f64",
    "rtw_filter_batch_device_f32", "rtw_filter_batch_device_f64", "rtw_filter_batch_f32", "rtw_filter_batch_f64",
    "rtw_render_filtered_batch_f32", "rtw_render_filtered_batch_f64",
    "rtw_accum_resolve_batch_f32", "rtw_accum_resolve_batch_f64", "rtw_accum_features_batch_f32", "rtw_accum_features_batch_f64",
    "rtw_accum_noise_batch_f32", "rtw_accum_noise_batch_f64", "rtw_guided_filter_batch_device_f32", "rtw_guided_filter_batch_device_f64",
    "rtw_accum_filtered_batch_f32", "rtw_accum_filtered_batch_f64",
    "rtw_upsample_work_bytes", "rtw_upsample_device_f32", "rtw_upsample_device_f64", "rtw_upsample_f32", "rtw_upsample_f64",
    "rtw_upsample_batch_device_f32", "rtw_upsample_batch_device_f64", "rtw_upsample_batch_f32", "rtw_upsample_batch_f64",
    "rtw_render_upsampled_f32", "rtw_render_upsampled_f64", "rtw_render_upsampled_batch_f32", "rtw_render_upsampled_batch_f64",
    "rtw_temporal_state_bytes", "rtw_temporal_device_f32", "rtw_temporal_device_f64", "rtw_temporal_f32", "rtw_temporal_f64",
    "rtw_render_sequence_f32", "rtw_render_sequence_f64",
    "rtw_history_moment_bytes", "rtw_history_moments_device_f32", "rtw_history_moments_device_f64", "rtw_history_noise_device_f32", "rtw_history_noise_device_f64",
    "rtw_history_moments_f32", "rtw_history_moments_f64", "rtw_render_path_guided_f32", "rtw_render_path_guided_f64",
    "rtw_clamped_step_device_f32", "rtw_clamped_step_device_f64", "rtw_clamped_step_f32", "rtw_clamped_step_f64",
    "rtw_render_path_clamped_f32", "rtw_render_path_clamped_f64",
    "rtw_reproject_table_bytes", "rtw_reproject_table_f32", "rtw_reproject_table_f64", "rtw_reproject_batch_device_f32", "rtw_reproject_batch_device_f64",
    "rtw_reproject_noise_batch_device_f32", "rtw_reproject_noise_batch_device_f64", "rtw_render_paths_f32", "rtw_render_paths_f64",
    "rtw_motion_table_f32", "rtw_motion_table_f64", "rtw_first_hit_motion_device_f32", "rtw_first_hit_motion_device_f64", "rtw_first_hit_motion_f32",
    "rtw_first_hit_motion_f64", "rtw_animated_step_device_f32", "rtw_animated_step_device_f64", "rtw_animated_step_f32", "rtw_animated_step_f64",
    "rtw_render_animation_f32", "rtw_render_animation_f64",
    "rtw_velocity_blur_work_bytes", "rtw_velocity_blur_device_f32", "rtw_velocity_blur_device_f64", "rtw_velocity_blur_f32", "rtw_velocity_blur_f64",
    "rtw_render_blurred_f32", "rtw_render_blurred_f64",
    "rtw_defocus_work_bytes", "rtw_defocus_device_f32", "rtw_defocus_device_f64", "rtw_defocus_f32", "rtw_defocus_f64",
    "rtw_render_defocused_f32", "rtw_render_defocused_f64",
    "rtw_wide_aperture_work_bytes", "rtw_wide_aperture_device_f32", "rtw_wide_aperture_device_f64", "rtw_wide_aperture_f32", "rtw_wide_aperture_f64",
    "rtw_render_wide_aperture_f32", "rtw_render_wide_aperture_f64",
    "rtw_lens_table_bytes", "rtw_lens_table_f32", "rtw_lens_table_f64", "rtw_lens_batch_work_bytes", "rtw_lens_batch_device_f32",
    "rtw_lens_batch_device_f64", "rtw_lens_batch_f32", "rtw_lens_batch_f64", "rtw_render_lens_batch_f32",
    "rtw_render_lens_batch_f64",
    "rtw_present_bytes", "rtw_present_device_f32", "rtw_present_device_f64", "rtw_present_batch_device_f32", "rtw_present_batch_device_f64",
    "rtw_present_f32", "rtw_present_f64", "rtw_render_presented_f32", "rtw_render_presented_f64", "rtw_render_presented_batch_f32",
    "rtw_render_presented_batch_f64",
    "rtw_cast_rays_device_f32", "rtw_cast_rays_device_f64", "rtw_cast_rays_f32", "rtw_cast_rays_f64",
    "rtw_trace_rays_device_f32", "rtw_trace_rays_device_f64", "rtw_trace_rays_f32", "rtw_trace_rays_f64",
]


def _scene_struct(ct):
    class S(C.Structure):
        _fields_ = [("n", C.c_int32)] + [(k, C.POINTER(ct)) for k in ("cx", "cy", "cz", "r")] + \
                   [("kind", C.POINTER(C.c_int32))] + [(k, C.POINTER(ct)) for k in ("ar", "ag", "ab", "param")]
    return S


def _camera_struct(ct):
    class Cam(C.Structure):
        _fields_ = [(k, ct * 3) for k in ("origin", "lower_left_corner", "horizontal", "vertical", "u", "v", "w")] + \
                   [("lens_radius", ct)]
    return Cam


SceneF32, SceneF64 = _scene_struct(C.c_float), _scene_struct(C.c_double)
CameraF32, CameraF64 = _camera_struct(C.c_float), _camera_struct(C.c_double)


class Params(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("spp", C.c_int32), ("max_depth", C.c_int32),
                ("seed", C.c_uint64), ("n_chunks", C.c_int32), ("shard_index", C.c_int32),
                ("shard_count", C.c_int32), ("device", C.c_int32), ("gamma", C.c_int32), ("flags", C.c_int32),
                ("n_devices", C.c_int32), ("job_pixels", C.c_int32), ("device_ids", C.POINTER(C.c_int32))]


class Stats(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("segments", C.c_uint64), ("sphere_tests", C.c_uint64),
                ("kernel_ms", C.c_double), ("total_ms", C.c_double), ("n_chunks", C.c_int32),
                ("grid_blocks", C.c_int32), ("block_threads", C.c_int32), ("gather_path", C.c_int32)]


class AccumInfo(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("width", "height", "device", "bound", "precision", "spp", "chunk_spp", "n_chunks", "max_depth",
                                          "numerics_flags", "chunks_done", "samples_done", "complete")] + [("seed", C.c_uint64)]


class Adaptive(C.Structure):
    """rtw_adaptive_t"""
    _fields_ = [("tolerance", C.c_double), ("dark_floor", C.c_double), ("min_chunks", C.c_int32), ("check_chunks", C.c_int32),
                ("reserved", C.c_int32 * 2)]


class AdaptiveInfo(C.Structure):
    """rtw_adaptive_info_t"""
    _fields_ = [(k, C.c_int32) for k in ("n_tiles", "tiles_converged", "tiles_at_cap", "rounds", "min_chunks_held", "max_chunks_held")] + \
               [("samples", C.c_uint64), ("tolerance", C.c_double)]


class Denoise(C.Structure):
    """rtw_denoise_t"""
    _fields_ = [(k, C.c_int32) for k in ("levels", "normal_power_log2", "flags", "gamma", "device", "reserved")] + \
               [("sigma_color", C.c_double), ("sigma_depth", C.c_double)]


class Upsample(C.Structure):
    """rtw_upsample_t"""
    _fields_ = [(k, C.c_int32) for k in ("levels", "normal_power_log2", "flags", "gamma", "device", "hi_chunks")] + \
               [("sigma_color", C.c_double), ("sigma_depth", C.c_double), ("sigma_albedo", C.c_double)]


class Temporal(C.Structure):
    """rtw_temporal_t"""
    _fields_ = [(k, C.c_int32) for k in ("normal_power_log2", "flags", "gamma", "device")] + [("reserved", C.c_int32 * 2)] + \
               [("sigma_depth", C.c_double), ("min_weight", C.c_double), ("history_max", C.c_double)]


assert C.sizeof(Temporal) == 48


class TemporalNoise(C.Structure):
    """rtw_temporal_noise_t"""
    _fields_ = [(k, C.c_int32) for k in ("radius", "normal_power_log2", "device")] + [("reserved", C.c_int32 * 3)] + \
               [("sigma_depth", C.c_double), ("min_len", C.c_double)]


assert C.sizeof(TemporalNoise) == 40


class TemporalClamp(C.Structure):
    """rtw_temporal_clamp_t"""
    _fields_ = [("radius", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32 * 2), ("sigma", C.c_double), ("len_scale", C.c_double)]


assert C.sizeof(TemporalClamp) == 32


class VelocityBlur(C.Structure):
    """rtw_velocity_blur_t"""
    _fields_ = [(k, C.c_int32) for k in ("taps", "flags", "gamma", "device")] + [("reserved", C.c_int32 * 2), ("shutter", C.c_double), ("depth_extent", C.c_double)]


assert C.sizeof(VelocityBlur) == 40


class Defocus(C.Structure):
    """rtw_defocus_t"""
    _fields_ = [(k, C.c_int32) for k in ("max_radius", "flags", "gamma", "device")] + [("reserved", C.c_int32 * 2), ("lens_radius", C.c_double), ("focus_dist", C.c_double)]


assert C.sizeof(Defocus) == 40


class WideAperture(C.Structure):
    """rtw_wide_aperture_t"""
    _fields_ = list(Defocus._fields_)


assert C.sizeof(WideAperture) == 40


class Present(C.Structure):
    """rtw_present_t"""
    _fields_ = [(k, C.c_int32) for k in ("channels", "flags", "device")] + [("nan_rgb", C.c_uint8 * 3), ("reserved0", C.c_uint8), ("exposure", C.c_double),
                                                                            ("reserved", C.c_int32 * 2)]


assert C.sizeof(Present) == 32


class RaysParams(C.Structure):
    """rtw_rays_params"""
    _fields_ = [(k, C.c_int32) for k in ("flags", "device", "max_workgroups", "reserved")] + [("tmin", C.c_double)]


assert C.sizeof(RaysParams) == 24


class TraceParams(C.Structure):
    """rtw_trace_params"""
    _fields_ = ([(k, C.c_int32) for k in ("flags", "device", "max_workgroups", "spp", "max_depth", "reserved")]
                + [(k, C.c_uint64) for k in ("seed", "first_stream", "first_sample")])


assert C.sizeof(TraceParams) == 48

_lib = None


class RtwError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"librtw_hip error {code}: {msg}")
        self.code = code


def lib():
    """Load librtw_hip.so; raise loudly if it has not been built (no CPU fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C raytracingweekend.jl_amd/csrc`).  There is no CPU fallback for the render path.")
    L = C.CDLL(LIB_PATH)
    L.rtw_last_error.restype = C.c_char_p
    L.rtw_abi_version.restype = C.c_int
    for name in SYMBOLS:
        getattr(L, name)  # AttributeError if the ABI is incomplete
    L.rtw_scene_upload_f32.argtypes = [C.POINTER(SceneF32), C.c_int, C.POINTER(C.c_void_p)]
    L.rtw_scene_upload_f64.argtypes = [C.POINTER(SceneF64), C.c_int, C.POINTER(C.c_void_p)]
    L.rtw_scene_free.argtypes = [C.c_void_p]
    L.rtw_render_device_f32.argtypes = [C.c_void_p, C.POINTER(CameraF32), C.POINTER(Params), C.c_void_p, C.c_void_p]
    L.rtw_render_device_f64.argtypes = [C.c_void_p, C.POINTER(CameraF64), C.POINTER(Params), C.c_void_p, C.c_void_p]
    L.rtw_render_f32.argtypes = [C.POINTER(SceneF32), C.POINTER(CameraF32), C.POINTER(Params), C.c_void_p]
    L.rtw_render_f64.argtypes = [C.POINTER(SceneF64), C.POINTER(CameraF64), C.POINTER(Params), C.c_void_p]
    L.rtw_render_batch_f32.argtypes = [C.POINTER(SceneF32), C.POINTER(CameraF32), C.c_int32, C.POINTER(C.c_uint64), C.POINTER(Params), C.c_void_p]
    L.rtw_render_batch_f64.argtypes = [C.POINTER(SceneF64), C.POINTER(CameraF64), C.c_int32, C.POINTER(C.c_uint64), C.POINTER(Params), C.c_void_p]
    L.rtw_render_batch_device_f32.argtypes = [C.c_void_p, C.POINTER(CameraF32), C.c_int32, C.POINTER(C.c_uint64), C.POINTER(Params),
                                              C.c_void_p, C.c_void_p]
    L.rtw_render_batch_device_f64.argtypes = [C.c_void_p, C.POINTER(CameraF64), C.c_int32, C.POINTER(C.c_uint64), C.POINTER(Params),
                                              C.c_void_p, C.c_void_p]
    for name, CamT in (("rtw_render_accum_f32", CameraF32), ("rtw_render_accum_f64", CameraF64)):
        getattr(L, name).argtypes = [C.c_void_p, C.POINTER(CamT), C.POINTER(Params), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    for name, CamT in (("rtw_render_adaptive_f32", CameraF32), ("rtw_render_adaptive_f64", CameraF64)):
        getattr(L, name).argtypes = [C.c_void_p, C.POINTER(CamT), C.POINTER(Params), C.POINTER(Adaptive), C.c_void_p, C.c_void_p, C.c_void_p]
    for name, CamT in (("rtw_render_accum_batch_f32", CameraF32), ("rtw_render_accum_batch_f64", CameraF64)):
        getattr(L, name).argtypes = [C.c_void_p, C.POINTER(CamT), C.c_int32, C.POINTER(C.c_uint64), C.POINTER(Params), C.c_int32, C.c_int32,
                                     C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p]
    for name, CamT in (("rtw_render_adaptive_batch_f32", CameraF32), ("rtw_render_adaptive_batch_f64", CameraF64)):
        getattr(L, name).argtypes = [C.c_void_p, C.POINTER(CamT), C.c_int32, C.POINTER(C.c_uint64), C.POINTER(Params), C.POINTER(Adaptive),
                                     C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p]
    for sfx, SceneT, CamT in (("f32", SceneF32, CameraF32), ("f64", SceneF64, CameraF64)):
        getattr(L, "rtw_render_features_device_" + sfx).argtypes = [C.c_void_p, C.POINTER(CamT), C.POINTER(Params), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        getattr(L, "rtw_render_features_" + sfx).argtypes = [C.POINTER(SceneT), C.POINTER(CamT), C.POINTER(Params), C.c_int32, C.c_int32, C.c_void_p]
        getattr(L, "rtw_denoise_device_" + sfx).argtypes = [C.POINTER(Denoise), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        getattr(L, "rtw_denoise_" + sfx).argtypes = [C.POINTER(Denoise), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        getattr(L, "rtw_render_denoised_" + sfx).argtypes = [C.POINTER(SceneT), C.POINTER(CamT), C.POINTER(Params), C.POINTER(Denoise), C.c_void_p]
        getattr(L, "rtw_accum_features_" + sfx).argtypes = [C.c_void_p, C.POINTER(CamT), C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_void_p]
        getattr(L, "rtw_accum_noise_" + sfx).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        getattr(L, "rtw_guided_filter_device_" + sfx).argtypes = [C.POINTER(Denoise), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                                 C.c_void_p]
        getattr(L, "rtw_accum_filtered_" + sfx).argtypes = [C.c_void_p, C.POINTER(CamT), C.POINTER(Params), C.POINTER(Denoise), C.c_void_p, C.c_int32, C.c_void_p]
        seeds = C.POINTER(C.c_uint64)
        getattr(L, "rtw_render_features_batch_device_" + sfx).argtypes = [C.c_void_p, C.POINTER(CamT), C.c_int32, seeds, C.POINTER(Params), C.c_int32, C.c_int32, C.c_void_p,
                                                                         C.c_void_p]
        getattr(L, "rtw_render_features_batch_" + sfx).argtypes = [C.POINTER(SceneT), C.POINTER(CamT), C.c_int32, seeds, C.POINTER(Params), C.c_int32, C.c_int32, C.c_void_p]
        getattr(L, "rtw_filter_batch_device_" + sfx).argtypes = [C.POINTER(Denoise), C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        getattr(L, "rtw_filter_batch_" + sfx).argtypes = [C.POINTER(Denoise), C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        getattr(L, "rtw_render_filtered_batch_" + sfx).argtypes = [C.POINTER(SceneT), C.POINTER(CamT), C.c_int32, seeds, C.POINTER(Params), C.POINTER(Denoise), C.c_void_p]
        accums = C.POINTER(C.c_void_p)
        getattr(L, "rtw_accum_resolve_batch_" + sfx).argtypes = [accums, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        getattr(L, "rtw_accum_features_batch_" + sfx).argtypes = [C.c_void_p, C.POINTER(CamT), C.c_int32, seeds, C.POINTER(Params), accums, C.c_void_p, C.c_void_p]
        getattr(L, "rtw_accum_noise_batch_" + sfx).argtypes = [accums, C.c_int32, C.c_void_p, C.c_void_p]
        getattr(L, "rtw_guided_filter_batch_device_" + sfx).argtypes = [C.POINTER(Denoise), C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                                       C.c_void_p, C.c_void_p]
        getattr(L, "rtw_accum_filtered_batch_" + sfx).argtypes = [C.c_void_p, C.POINTER(CamT), C.c_int32, seeds, C.POINTER(Params), C.POINTER(Denoise), accums, C.c_int32,
                                                                 C.c_void_p]
        up, i32, ptr = C.POINTER(Upsample), C.c_int32, C.c_void_p
        getattr(L, "rtw_upsample_device_" + sfx).argtypes = [up, i32, i32, i32, i32, ptr, ptr, ptr, ptr, ptr, ptr]
        getattr(L, "rtw_upsample_" + sfx).argtypes = [up, i32, i32, i32, i32, ptr, ptr, ptr, ptr]
        getattr(L, "rtw_upsample_batch_device_" + sfx).argtypes = [up, i32, i32, i32, i32, i32, ptr, ptr, ptr, ptr, ptr, ptr]
        getattr(L, "rtw_upsample_batch_" + sfx).argtypes = [up, i32, i32, i32, i32, i32, ptr, ptr, ptr, ptr]
        getattr(L, "rtw_render_upsampled_" + sfx).argtypes = [C.POINTER(SceneT), C.POINTER(CamT), C.POINTER(Params), i32, i32, up, ptr]
        getattr(L, "rtw_render_upsampled_batch_" + sfx).argtypes = [C.POINTER(SceneT), C.POINTER(CamT), i32, seeds, C.POINTER(Params), i32, i32, up, ptr]
        tp = C.POINTER(Temporal)
        getattr(L, "rtw_temporal_device_" + sfx).argtypes = [tp, C.POINTER(CamT), C.POINTER(CamT), i32, i32, ptr, ptr, ptr, ptr, ptr, ptr]
        getattr(L, "rtw_temporal_" + sfx).argtypes = [tp, C.POINTER(CamT), C.POINTER(CamT), i32, i32, ptr, ptr, ptr, ptr, ptr]
        getattr(L, "rtw_render_sequence_" + sfx).argtypes = [C.POINTER(SceneT), C.POINTER(CamT), i32, seeds, C.POINTER(Params), tp, C.POINTER(Denoise), ptr]
        tn = C.POINTER(TemporalNoise)
        getattr(L, "rtw_history_moments_device_" + sfx).argtypes = [tp, C.POINTER(CamT), C.POINTER(CamT), i32, i32, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr]
        getattr(L, "rtw_history_noise_device_" + sfx).argtypes = [tn, i32, i32, ptr, ptr, ptr, ptr]
        getattr(L, "rtw_history_moments_" + sfx).argtypes = [tp, tn, C.POINTER(CamT), C.POINTER(CamT), i32, i32, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr]
        getattr(L, "rtw_render_path_guided_" + sfx).argtypes = [C.POINTER(SceneT), C.POINTER(CamT), i32, seeds, C.POINTER(Params), tp, tn, C.POINTER(Denoise), ptr]
        tc = C.POINTER(TemporalClamp)
        getattr(L, "rtw_clamped_step_device_" + sfx).argtypes = [tp, tc, C.POINTER(CamT), C.POINTER(CamT), i32, i32, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr]
        getattr(L, "rtw_clamped_step_" + sfx).argtypes = [tp, tc, C.POINTER(CamT), C.POINTER(CamT), i32, i32, ptr, ptr, ptr, ptr, ptr, ptr, ptr]
        getattr(L, "rtw_render_path_clamped_" + sfx).argtypes = [C.POINTER(SceneT), C.POINTER(CamT), i32, seeds, C.POINTER(Params), tp, tc, tn, C.POINTER(Denoise), ptr]
        getattr(L, "rtw_reproject_table_" + sfx).argtypes = [C.POINTER(CamT), C.POINTER(CamT), i32, ptr]
        getattr(L, "rtw_reproject_batch_device_" + sfx).argtypes = [tp, tc, i32, ptr, i32, i32, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr]
        getattr(L, "rtw_reproject_noise_batch_device_" + sfx).argtypes = [tn, i32, i32, i32, ptr, ptr, ptr, ptr]
        getattr(L, "rtw_render_paths_" + sfx).argtypes = [C.POINTER(SceneT), C.POINTER(CamT), i32, i32, seeds, C.POINTER(Params), tp, tc, tn, C.POINTER(Denoise), ptr]
        getattr(L, "rtw_motion_table_" + sfx).argtypes = [C.POINTER(SceneT), C.POINTER(SceneT), ptr]
        getattr(L, "rtw_first_hit_motion_device_" + sfx).argtypes = [ptr, C.POINTER(CamT), C.POINTER(Params), ptr, ptr, ptr]
        getattr(L, "rtw_first_hit_motion_" + sfx).argtypes = [C.POINTER(SceneT), C.POINTER(CamT), C.POINTER(Params), ptr, ptr]
        getattr(L, "rtw_animated_step_device_" + sfx).argtypes = [tp, tc, C.POINTER(CamT), C.POINTER(CamT), i32, i32, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr]
        getattr(L, "rtw_animated_step_" + sfx).argtypes = [tp, tc, C.POINTER(CamT), C.POINTER(CamT), i32, i32, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr]
        getattr(L, "rtw_render_animation_" + sfx).argtypes = [C.POINTER(SceneT), C.POINTER(CamT), i32, seeds, C.POINTER(Params), tp, tc, C.POINTER(Denoise), ptr]
        getattr(L, "rtw_velocity_blur_device_" + sfx).argtypes = [C.POINTER(VelocityBlur), C.POINTER(CamT), C.POINTER(CamT), i32, i32, ptr, ptr, ptr, ptr, ptr, ptr]
        getattr(L, "rtw_velocity_blur_" + sfx).argtypes = [C.POINTER(VelocityBlur), C.POINTER(CamT), C.POINTER(CamT), i32, i32, ptr, ptr, ptr, ptr]
        getattr(L, "rtw_render_blurred_" + sfx).argtypes = [C.POINTER(SceneT), C.POINTER(CamT), i32, seeds, C.POINTER(Params), tp, tc, C.POINTER(Denoise), C.POINTER(VelocityBlur), ptr]
        df = C.POINTER(Defocus)
        getattr(L, "rtw_defocus_device_" + sfx).argtypes = [df, C.POINTER(CamT), i32, i32, ptr, ptr, ptr, ptr, ptr]
        getattr(L, "rtw_defocus_" + sfx).argtypes = [df, C.POINTER(CamT), i32, i32, ptr, ptr, ptr]
        getattr(L, "rtw_render_defocused_" + sfx).argtypes = [C.POINTER(SceneT), C.POINTER(CamT), C.POINTER(Params), C.POINTER(Denoise), df, ptr]
        wa = C.POINTER(WideAperture)
        getattr(L, "rtw_wide_aperture_device_" + sfx).argtypes = [wa, C.POINTER(CamT), i32, i32, ptr, ptr, ptr, ptr, ptr]
        getattr(L, "rtw_wide_aperture_" + sfx).argtypes = [wa, C.POINTER(CamT), i32, i32, ptr, ptr, ptr]
        getattr(L, "rtw_render_wide_aperture_" + sfx).argtypes = [C.POINTER(SceneT), C.POINTER(CamT), C.POINTER(Params), C.POINTER(Denoise), wa, ptr]
        f64p = C.POINTER(C.c_double)
        getattr(L, "rtw_lens_table_" + sfx).argtypes = [wa, C.POINTER(CamT), i32, i32, i32, f64p, f64p, ptr]
        getattr(L, "rtw_lens_batch_device_" + sfx).argtypes = [wa, i32, i32, ptr, i32, i32, ptr, ptr, ptr, ptr, ptr]
        getattr(L, "rtw_lens_batch_" + sfx).argtypes = [wa, C.POINTER(CamT), i32, i32, f64p, f64p, i32, i32, ptr, ptr, ptr]
        getattr(L, "rtw_render_lens_batch_" + sfx).argtypes = [C.POINTER(SceneT), C.POINTER(CamT), i32, C.POINTER(C.c_uint64), C.POINTER(Params), C.POINTER(Denoise), wa,
                                                                          f64p, f64p, ptr]
        pr, dn = C.POINTER(Present), C.POINTER(Denoise)
        getattr(L, "rtw_present_device_" + sfx).argtypes = [pr, i32, i32, ptr, ptr, ptr]
        getattr(L, "rtw_present_batch_device_" + sfx).argtypes = [pr, i32, i32, i32, ptr, ptr, ptr]
        getattr(L, "rtw_present_" + sfx).argtypes = [pr, i32, i32, ptr, ptr]
        getattr(L, "rtw_render_presented_" + sfx).argtypes = [C.POINTER(SceneT), C.POINTER(CamT), C.POINTER(Params), dn, pr, ptr]
        getattr(L, "rtw_render_presented_batch_" + sfx).argtypes = [C.POINTER(SceneT), C.POINTER(CamT), i32, seeds, C.POINTER(Params), dn, pr, ptr]
        getattr(L, "rtw_cast_rays_device_" + sfx).argtypes = [ptr, ptr, C.c_int64, C.POINTER(RaysParams), ptr, ptr, ptr]
        getattr(L, "rtw_cast_rays_" + sfx).argtypes = [C.POINTER(SceneT), ptr, C.c_int64, C.POINTER(RaysParams), ptr, ptr]
        getattr(L, "rtw_trace_rays_device_" + sfx).argtypes = [ptr, ptr, C.c_int64, C.POINTER(TraceParams), ptr, ptr]
        getattr(L, "rtw_trace_rays_" + sfx).argtypes = [C.POINTER(SceneT), ptr, C.c_int64, C.POINTER(TraceParams), ptr]
    L.rtw_present_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    L.rtw_present_bytes.restype = C.c_int64
    L.rtw_temporal_state_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    L.rtw_temporal_state_bytes.restype = C.c_int64
    L.rtw_velocity_blur_work_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    L.rtw_velocity_blur_work_bytes.restype = C.c_int64
    L.rtw_defocus_work_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    L.rtw_defocus_work_bytes.restype = C.c_int64
    L.rtw_wide_aperture_work_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    L.rtw_wide_aperture_work_bytes.restype = C.c_int64
    L.rtw_lens_table_bytes.argtypes = [C.c_int32, C.c_int32]
    L.rtw_lens_table_bytes.restype = C.c_int64
    L.rtw_lens_batch_work_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    L.rtw_lens_batch_work_bytes.restype = C.c_int64
    L.rtw_history_moment_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    L.rtw_history_moment_bytes.restype = C.c_int64
    L.rtw_reproject_table_bytes.argtypes = [C.c_int32, C.c_int32]
    L.rtw_reproject_table_bytes.restype = C.c_int64
    L.rtw_upsample_work_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    L.rtw_upsample_work_bytes.restype = C.c_int64
    L.rtw_denoise_work_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    L.rtw_denoise_work_bytes.restype = C.c_int64
    L.rtw_accum_adaptive_info.argtypes = [C.c_void_p, C.POINTER(AdaptiveInfo)]
    L.rtw_accum_tile_chunks.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.rtw_accum_create.argtypes = [C.c_int, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    L.rtw_accum_reset.argtypes = [C.c_void_p, C.c_void_p]
    L.rtw_accum_free.argtypes = [C.c_void_p]
    L.rtw_accum_resolve_f32.argtypes = L.rtw_accum_resolve_f64.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.rtw_accum_resolve_host_f32.argtypes = L.rtw_accum_resolve_host_f64.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    L.rtw_accum_merge.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.rtw_accum_info.argtypes = [C.c_void_p, C.POINTER(AccumInfo)]
    L.rtw_accum_ranges.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.rtw_accum_read_pixels.argtypes = [C.c_void_p, C.c_void_p]
    L.rtw_accum_export.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.rtw_accum_import.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]
    L.rtw_stats.argtypes = [C.POINTER(Stats)]
    L.rtw_stats_devices.argtypes = [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double)]
    L.rtw_unit_f32.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(SceneF32), C.POINTER(CameraF32)]
    L.rtw_unit_f64.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(SceneF64), C.POINTER(CameraF64)]
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise RtwError(rc, lib().rtw_last_error().decode("utf-8", "replace"))


def is_f64(T):
    return np.dtype(T) == np.float64


def make_scene(flat, T):
    """dict from structs.flatten_scene -> (ctypes struct, keep-alive list)"""
    ct = C.c_double if is_f64(T) else C.c_float
    S = (SceneF64 if is_f64(T) else SceneF32)()
    keep = []
    S.n = int(flat["n"])
    for k in ("cx", "cy", "cz", "r", "ar", "ag", "ab", "param"):
        a = np.ascontiguousarray(flat[k], dtype=T)
        keep.append(a)
        setattr(S, k, a.ctypes.data_as(C.POINTER(ct)))
    kind = np.ascontiguousarray(flat["kind"], dtype=np.int32)
    keep.append(kind)
    S.kind = kind.ctypes.data_as(C.POINTER(C.c_int32))
    return S, keep


def make_camera(cam, T):
    ct = C.c_double if is_f64(T) else C.c_float
    Cm = (CameraF64 if is_f64(T) else CameraF32)()
    for k in ("origin", "lower_left_corner", "horizontal", "vertical", "u", "v", "w"):
        setattr(Cm, k, (ct * 3)(*[float(x) for x in np.asarray(getattr(cam, k), dtype=T)]))
    Cm.lens_radius = float(np.dtype(T).type(cam.lens_radius))
    return Cm


def make_cameras(cams, T):
    """sequence of Camera -> ctypes array of n camera structs (the ``cams`` of rtw_render_batch_*)"""
    arr = ((CameraF64 if is_f64(T) else CameraF32) * len(cams))()
    for k, cam in enumerate(cams):
        arr[k] = make_camera(cam, T)
    return arr


def make_seeds(seed, n):
    """int or sequence of n ints -> ctypes array of n uint64 seeds (the ``seeds`` of rtw_render_batch_*)"""
    if isinstance(seed, (int, np.integer)):
        seeds = [int(seed)] * n
    else:
        seeds = [int(s) for s in seed]
        if len(seeds) != n:
            raise ValueError(f"{len(seeds)} seeds for {n} views")
    return (C.c_uint64 * n)(*seeds)


def make_handles(handles):
    """sequence of accumulator handles (c_void_p or int) -> ctypes array (the ``accums`` of rtw_render_accum_batch_* / _adaptive_batch_*)"""
    return (C.c_void_p * len(handles))(*[h.value if isinstance(h, C.c_void_p) else h for h in handles])


FLAG_GROUP_CULL = 1      # include/rtw_hip.h RTW_FLAG_GROUP_CULL
FLAG_COMPACT_TILES = 2   # include/rtw_hip.h RTW_FLAG_COMPACT_TILES
FLAG_SCAN_VALU = 4       # include/rtw_hip.h RTW_FLAG_SCAN_VALU
FLAG_RAY_POOL = 8        # include/rtw_hip.h RTW_FLAG_RAY_POOL
FLAG_RCCL_REDUCE = 16    # include/rtw_hip.h RTW_FLAG_RCCL_REDUCE
FLAG_NUMERICS_CONTRACT = 32        # include/rtw_hip.h RTW_FLAG_NUMERICS_CONTRACT
FLAG_NUMERICS_REFERENCE_FMA2 = 128  # include/rtw_hip.h RTW_FLAG_NUMERICS_REFERENCE_FMA2
DENOISE_DEMODULATE = 1   # include/rtw_hip.h RTW_DENOISE_DEMODULATE
UPSAMPLE_DEMODULATE = 1  # include/rtw_hip.h RTW_UPSAMPLE_DEMODULATE
TEMPORAL_DEMODULATE = 1  # include/rtw_hip.h RTW_TEMPORAL_DEMODULATE
CLAMP_GUIDES = 1         # include/rtw_hip.h RTW_CLAMP_GUIDES
PRESENT_DITHER, PRESENT_BGR, PRESENT_SQRT = 1, 2, 4     # include/rtw_hip.h RTW_PRESENT_*
GATHER_PEER, GATHER_HOST_STAGED, GATHER_RCCL, GATHER_SAME_DEVICE = 1, 2, 4, 8    # rtw_stats_t.gather_path bits
ABI_VERSION = 4

# The deciding arithmetic of the ray-sphere test (src/hit.jl:16-18; include/rtw_hip.h RTW_FLAG_NUMERICS_*).
# name -> (rtw_params.flags bits, the mode code in bits 8-9 of a unit op)
NUMERICS = {"reference": (0, 0), "contract": (FLAG_NUMERICS_CONTRACT, 1), "reference_fma2": (FLAG_NUMERICS_REFERENCE_FMA2, 3)}
_default_numerics = "reference"


def set_default_numerics(name):
    """TEST HELPER (tests/conftest.py runs every parity module once per mode with it) -- process-wide, not for product code: name the mode
    per call instead.  The mode ``render`` / ``DeviceRenderer`` / ``make_params`` use when none is named.  Returns the previous default."""
    global _default_numerics
    if name not in NUMERICS:
        raise ValueError(f"numerics must be one of {sorted(NUMERICS)}")
    prev, _default_numerics = _default_numerics, name
    return prev


def numerics_name(numerics=None):
    name = _default_numerics if numerics is None else numerics
    if name not in NUMERICS:
        raise ValueError(f"numerics must be one of {sorted(NUMERICS)}")
    return name


def numerics_flags(numerics=None):
    return NUMERICS[numerics_name(numerics)][0]


def numerics_unit_bits(numerics=None):
    """what to OR into the ``op`` of rtw_unit_f32/_f64"""
    return NUMERICS[numerics_name(numerics)][1] << 8


def make_params(width, height, spp, max_depth=16, seed=1, n_chunks=0, shard_index=0, shard_count=1,
                device=-1, gamma=1, flags=0, devices=None, job_pixels=0, numerics=None):
    """``numerics``: "reference" (default) / "contract" / "reference_fma2", or None = the module default
    (``set_default_numerics``).  ``flags`` may name the mode instead (a NUMERICS bit); naming a DIFFERENT mode both ways is a ValueError
    (the mode changes the image: it is never overridden silently).
    ``devices``: None / int ordinal -> one device; "all" -> every visible device (n_devices = -1);
    a sequence of ordinals -> that device list (host-buffer entry points only)."""
    flags = int(flags)
    named = flags & (FLAG_NUMERICS_CONTRACT | FLAG_NUMERICS_REFERENCE_FMA2)
    if not named:
        flags |= numerics_flags(numerics)
    elif numerics is not None and numerics_flags(numerics) != named:
        raise ValueError(f"numerics={numerics!r} conflicts with the NUMERICS bit already in flags (0x{named:x})")
    P = Params(int(width), int(height), int(spp), int(max_depth), int(seed), int(n_chunks),
               int(shard_index), int(shard_count), int(device), int(gamma), flags, 0, int(job_pixels), None)
    if devices is None:
        return P
    if isinstance(devices, str):
        if devices != "all":
            raise ValueError("devices must be None, 'all', an ordinal or a sequence of ordinals")
        P.n_devices = -1
    elif isinstance(devices, (int, np.integer)):
        P.device = int(devices)
    else:
        ids = (C.c_int32 * len(devices))(*[int(d) for d in devices])
        P._keep_ids = ids                     # keep the array alive as long as the struct
        if len(devices) == 1:
            P.device = int(devices[0])
        P.n_devices = len(devices)            # (a list of one: the same device, named both ways)
        P.device_ids = C.cast(ids, C.POINTER(C.c_int32))
    return P
