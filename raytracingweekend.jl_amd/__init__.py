"""raytracingweekend.jl_amd -- MI355X (gfx950) implementation of ONE hot path of
claforte/RayTracingWeekend.jl: ``render -> ray_color -> hit/scatter``.

Host-side mirror of the reference's exported interface for that path
(/root/reference/src/RayTracingWeekend.jl:9-31): same names, argument meaning and defaults.
The compute is ``lib/librtw_hip.so`` (hand-written HIP, C ABI in include/rtw_hip.h); this
package only flattens the scene, calls it through ctypes and wraps the result.  There is no
CPU fallback: without the built library or without a GPU every render call raises.

The directory name contains a dot, so it is imported through the alias module ``rtw_amd``
at the repository root (``import rtw_amd``).
"""
from .rng import TRNG, Xoroshiro128Plus, reseed, trand, random_between  # noqa: F401
from .structs import (  # noqa: F401
    Camera, Dielectric, HittableList, Lambertian, Material, Metal, Sphere, default_camera,
    flatten_scene, image_height,
)
from .scenes import (  # noqa: F401
    scene_2_spheres, scene_4_spheres, scene_blue_red_spheres, scene_diel_spheres,
    scene_random_spheres, t_cam1, t_cam2, t_default_cam,
)
from .render import DeviceRenderer, render, render_batch, last_stats  # noqa: F401
from .progressive import ProgressiveBatchRenderer, ProgressiveRenderer, render_progressive, samples_in_chunks  # noqa: F401
from .adaptive import (  # noqa: F401
    AdaptiveBatchRenderer, AdaptiveRenderer, reference_decisions, render_adaptive, render_adaptive_batch, render_adaptive_denoised,
    render_adaptive_denoised_batch,
)
from .shard import compact_elems, compact_to_frame_index, local_tile_count, owned_pixel_mask, render_sharded  # noqa: F401
from .features import features_batch_into, features_into, render_features, render_features_batch  # noqa: F401
from .denoise import (  # noqa: F401
    denoise, denoise_batch, denoise_batch_into, denoise_guided_batch_into, denoise_guided_into, denoise_into, denoise_work_bytes, render_denoised,
    render_denoised_batch,
)
from .upsample import (  # noqa: F401
    make_upsample, render_upsampled, render_upsampled_batch, upsample, upsample_batch, upsample_batch_into, upsample_into, upsample_work_bytes,
)
from .temporal import (  # noqa: F401
    TemporalAccumulator, make_temporal, make_temporal_noise, render_sequence, temporal_moment_bytes, temporal_noise_into, temporal_state_bytes, temporal_step,
    temporal_step_into, temporal_step_moments, temporal_step_moments_into, make_temporal_clamp, temporal_step_clamped, temporal_step_clamped_into,
    temporal_path_table, temporal_step_batch_into, temporal_noise_batch_into, TemporalBatchAccumulator, render_sequences,
    motion_table, first_hit_motion, first_hit_motion_into, temporal_step_animated, temporal_step_animated_into, render_animation,
)
from .motion_blur import make_motion_blur, motion_blur, motion_blur_into, motion_blur_work_bytes  # noqa: F401
from .defocus import defocus, defocus_into, defocus_work_bytes, make_defocus, render_defocused  # noqa: F401
from .wide_aperture import (  # noqa: F401
    focus_bracket, lens_table, make_wide_aperture, render_wide_aperture, render_wide_aperture_batch, wide_aperture, wide_aperture_batch, wide_aperture_batch_into,
    wide_aperture_batch_work_bytes, wide_aperture_into, wide_aperture_work_bytes,
)
from .present import (  # noqa: F401
    make_present, present, present_batch_into, present_bytes, present_into, render_presented, render_presented_batch,
)
from .rays import cast_rays, cast_rays_into, make_rays_params  # noqa: F401
from .trace_rays import make_trace_params, trace_rays, trace_rays_into  # noqa: F401
from . import imageio  # noqa: F401

__all__ = [
    "TRNG", "Xoroshiro128Plus", "reseed", "trand", "random_between",
    "Camera", "Dielectric", "HittableList", "Lambertian", "Material", "Metal", "Sphere",
    "default_camera", "flatten_scene", "image_height",
    "scene_2_spheres", "scene_4_spheres", "scene_blue_red_spheres", "scene_diel_spheres",
    "scene_random_spheres", "t_cam1", "t_cam2", "t_default_cam",
    "DeviceRenderer", "render", "render_batch", "last_stats", "ProgressiveRenderer", "render_progressive", "samples_in_chunks",
    "AdaptiveRenderer", "render_adaptive", "reference_decisions", "owned_pixel_mask", "render_sharded", "compact_elems",
    "compact_to_frame_index", "local_tile_count", "ProgressiveBatchRenderer", "AdaptiveBatchRenderer", "render_adaptive_batch",
    "render_features", "features_into", "denoise", "denoise_into", "denoise_work_bytes", "render_denoised",
    "denoise_guided_into", "render_adaptive_denoised",
    "render_features_batch", "features_batch_into", "denoise_batch", "denoise_batch_into", "render_denoised_batch",
    "denoise_guided_batch_into", "render_adaptive_denoised_batch",
    "make_upsample", "upsample_work_bytes", "upsample", "upsample_into", "upsample_batch", "upsample_batch_into", "render_upsampled",
    "render_upsampled_batch",
    "make_temporal", "temporal_state_bytes", "temporal_step", "temporal_step_into", "TemporalAccumulator", "render_sequence",
    "make_temporal_noise", "temporal_moment_bytes", "temporal_step_moments", "temporal_step_moments_into", "temporal_noise_into",
    "make_temporal_clamp", "temporal_step_clamped", "temporal_step_clamped_into",
    "temporal_path_table", "temporal_step_batch_into", "temporal_noise_batch_into", "TemporalBatchAccumulator", "render_sequences",
    "motion_table", "first_hit_motion", "first_hit_motion_into", "temporal_step_animated", "temporal_step_animated_into", "render_animation",
    "make_motion_blur", "motion_blur_work_bytes", "motion_blur", "motion_blur_into",
    "make_defocus", "defocus_work_bytes", "defocus", "defocus_into", "render_defocused",
    "make_wide_aperture", "wide_aperture_work_bytes", "wide_aperture", "wide_aperture_into", "render_wide_aperture",
    "lens_table", "wide_aperture_batch_work_bytes", "wide_aperture_batch", "wide_aperture_batch_into", "focus_bracket", "render_wide_aperture_batch",
    "make_present", "present_bytes", "present", "present_into", "present_batch_into", "render_presented", "render_presented_batch",
    "cast_rays", "cast_rays_into", "make_rays_params",
    "trace_rays", "trace_rays_into", "make_trace_params",
]
