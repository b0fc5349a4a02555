"""Host-side mirror of the reference's Camera / Scene / integrate surface over the libptmi C-ABI (include/pt_api.h).

    Scene::new(models)                 src/scene.rs:21        -> Renderer(scene_desc, ...)
    Camera::new(...)                   src/camera.rs:17       -> Renderer.set_camera(CameraDesc)
    per-frame pixel loop + accumulate  src/main.rs:181-207    -> Renderer.render(first_sample, n_samples)
    TLAS::intersect / any_intersect    src/tlas.rs:66,111     -> Renderer.trace_closest / trace_any

All compute happens in libptmi.so (HIP, gfx950).  If the library is missing or no GPU is present the calls raise:
there is no CPU path in the product.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from . import build as _build
from .scene_desc import CameraDesc, SceneDesc

PT_OK = 0
FLAG_TIMING = 1
FLAG_NO_LDS_SCENE = 2
FLAG_TIMING_ALL = 4
FLAG_NO_PRIMARY_CULL = 8
FLAG_GENERAL_WALK = 16
FLAG_ADAPTIVE = 32
DEFAULT_SEED = 0x5EED5EED

# every symbol include/pt_api.h declares
EXPORTS = [
    "pt_create", "pt_destroy", "pt_last_error", "pt_set_config", "pt_add_material", "pt_add_model", "pt_add_model_obj", "pt_model_vertices", "pt_build", "pt_set_camera",
    "pt_camera_matrices", "pt_set_environment", "pt_create_ray", "pt_set_lens", "pt_primary_ray", "pt_render", "pt_render_device", "pt_reset_accumulation", "pt_accum_device_ptr",
    "pt_read_accumulation", "pt_read_frame", "pt_write_accumulation", "pt_render_samples", "pt_render_adaptive", "pt_adaptive_mask", "pt_read_moments", "pt_write_moments", "pt_active_pixels", "pt_local_rows", "pt_set_stream", "pt_synchronize", "pt_camera_input", "pt_camera_angles", "pt_frame", "pt_inv_projection", "pt_present", "pt_post_velocity", "pt_post_reproject", "pt_post_tonemap", "pt_post_rgb8", "pt_present_rgb8", "pt_write_image", "pt_trace_closest", "pt_trace_any",
    "pt_ss_sobol", "pt_math_batch", "pt_material_eval", "pt_volume_eval", "pt_bsdf_eval", "pt_blas_count", "pt_blas_dump", "pt_tlas_dump", "pt_tlas_instances", "pt_instance_materials", "pt_light_cdf",
    "pt_triangle_dump", "pt_get_stats", "pt_reset_stats", "pt_last_batch_counters", "pt_last_batch_shade_pids", "pt_last_batch_step_stats",
    "pt_variant_axes", "pt_variant_compiled", "pt_last_launches", "pt_trace_geometry",
    "pt_multi_create", "pt_multi_destroy", "pt_multi_last_error", "pt_multi_ctx", "pt_multi_render", "pt_multi_framebuffer_device_ptr",
    "pt_multi_reset_accumulation", "pt_multi_get_stats", "pt_multi_used_rccl", "pt_multi_write_image",
    "pt_render_guides", "pt_read_guides", "pt_denoise", "pt_write_denoised_image", "pt_post_denoise",
    "pt_integrate_rays", "pt_integrate_rays_device", "pt_bake_probes", "pt_probe_ray",
    "pt_set_instances", "pt_get_scene_info", "pt_read_guide_instances", "pt_frame_moving", "pt_post_motion",
    "pt_add_texture", "pt_set_material_texture", "pt_set_model_uvs", "pt_model_uvs", "pt_surface_colour", "pt_read_guide_albedo",
    "pt_set_material_emission_texture", "pt_set_material_normal_texture", "pt_shading_normal",
    "pt_set_material_roughness_texture", "pt_surface_roughness",
    "pt_accumulate_albedo", "pt_reset_albedo", "pt_read_albedo", "pt_denoise_albedo", "pt_post_denoise_albedo",
    "pt_set_projection", "pt_get_projection",
    "pt_bake_lightmap", "pt_lightmap_texels", "pt_lightmap_ray", "pt_lightmap_dilate",
    "pt_render_guides_followed", "pt_read_guide_hops", "pt_accumulate_albedo_followed", "pt_guide_follow_dir",
    "pt_frame_temporal", "pt_read_temporal", "pt_reset_temporal", "pt_post_temporal", "pt_frame_temporal_options", "pt_post_temporal_options",
    "pt_set_lightmap", "pt_get_lightmap_info", "pt_lightmap_lookup", "pt_render_baked", "pt_read_baked", "pt_reset_baked", "pt_write_baked_image",
    "pt_set_probe_grid", "pt_get_probe_grid_info", "pt_probe_grid_lookup", "pt_probe_backfaces",
    "pt_bake_lightmap_moments", "pt_lightmap_denoise",
    "pt_probe_depth_texel", "pt_bake_probe_depth", "pt_set_probe_grid_depth", "pt_get_probe_grid_depth_info",
    "pt_probe_radiance_dir", "pt_bake_probe_radiance", "pt_probe_radiance_prefilter", "pt_set_probe_grid_radiance", "pt_get_probe_grid_radiance_info",
    "pt_probe_grid_specular",
    "pt_bake_lightmap_directional", "pt_lightmap_gradient", "pt_set_lightmap_directional", "pt_get_lightmap_directional_info", "pt_lightmap_lookup_directional",
    "pt_bake_lightmap_adaptive", "pt_lightmap_adaptive_mask", "pt_lightmap_denoise_counts",
    "pt_bake_lightmap_direct", "pt_bake_lightmap_adaptive_direct", "pt_lightmap_light_sample",
    "pt_baked_rays", "pt_baked_rays_device", "pt_bake_lightmap_gather", "pt_bake_lightmap_adaptive_gather",
]


LAUNCHERS = ("shade", "terminal", "closest", "any", "fused", "generate", "guide_rays", "accumulate")   # pt_launcher
LAUNCHES_BATCH, LAUNCHES_HOOK = 0, 1   # pt_last_launches' which
PROBE_VIS_FACING = 1   # pt_probe_depth's flags
ALBEDO_GUIDE, ALBEDO_MEAN = 1, 2   # pt_denoise_albedo's albedo_source
PROJ_PERSPECTIVE, PROJ_PANORAMA, PROJ_ORTHOGRAPHIC = range(3)   # pt_projection_kind
EV_MOUSE_MOTION, EV_KEY_W, EV_KEY_S, EV_KEY_A, EV_KEY_D = range(5)


class MaterialDesc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("colour", C.c_float * 3), ("roughness", C.c_float), ("ior", C.c_float), ("has_volume", C.c_int32),
                ("vol_absorption", C.c_float * 3), ("vol_k", C.c_float), ("vol_c", C.c_float), ("vol_g", C.c_float)]


class Projection(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("span_x_deg", C.c_float), ("span_y_deg", C.c_float), ("ortho_height", C.c_float), ("reserved", C.c_uint32 * 4)]


class Config(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("max_bounces", C.c_uint32), ("n_sobol", C.c_uint32),
                ("enable_nee", C.c_uint32), ("seed", C.c_uint64), ("rank", C.c_uint32), ("world_size", C.c_uint32),
                ("strip_rows", C.c_uint32), ("batch_spp", C.c_uint32), ("device", C.c_int32), ("flags", C.c_uint32),
                ("stack_lds_levels", C.c_uint32), ("queue_slack", C.c_uint32), ("pipelines", C.c_uint32), ("reserved", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [("rays_closest", C.c_uint64), ("rays_any", C.c_uint64), ("rays_light_closest", C.c_uint64), ("paths", C.c_uint64),
                ("launches_trace_closest", C.c_uint64), ("ms_trace_closest", C.c_double), ("ms_trace_any", C.c_double),
                ("ms_trace_light", C.c_double), ("ms_shade", C.c_double), ("ms_generate", C.c_double), ("ms_accumulate", C.c_double),
                ("ms_total", C.c_double), ("scene_bytes", C.c_uint64), ("lds_scene", C.c_uint32), ("stack_entries", C.c_uint32),
                ("state_bytes", C.c_uint64), ("rays_light_closest_traced", C.c_uint64), ("rays_primary_culled", C.c_uint64),
                ("ident_tlas", C.c_uint32), ("reserved_stats", C.c_uint32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}

    @property
    def rays(self):
        return self.rays_closest + self.rays_any + self.rays_light_closest


class Adaptive(C.Structure):
    """pt_adaptive: the selection criterion of an adaptive render (include/pt_api.h)"""
    _fields_ = [("rel_error", C.c_float), ("abs_floor", C.c_float), ("min_samples", C.c_uint32), ("max_samples", C.c_uint32)]


class DenoiseParams(C.Structure):
    """pt_denoise_params: the a-trous filter's levels and edge-stopping widths (include/pt_api.h); 0 selects each default"""
    _fields_ = [("iterations", C.c_uint32), ("sigma_luminance", C.c_float), ("sigma_normal", C.c_uint32), ("sigma_plane", C.c_float)]


class TemporalParams(C.Structure):
    """pt_temporal_params: the temporal stage's blend floors, tap tests and feedback switch (include/pt_api.h); 0 selects each default"""
    _fields_ = [("alpha", C.c_float), ("alpha_moments", C.c_float), ("normal_min", C.c_float), ("plane_max", C.c_float), ("feedback", C.c_uint32),
                ("reserved", C.c_uint32 * 3)]


class TemporalOptions(C.Structure):
    """pt_temporal_options: the temporal stage's options, each 0 or 1 (include/pt_api.h): the 3 x 3 rescue search, the length rule, demodulation"""
    _fields_ = [("rescue", C.c_uint32), ("length_rule", C.c_uint32), ("demodulate", C.c_uint32), ("reserved", C.c_uint32)]


TEMPORAL_LENGTH_MIN, TEMPORAL_LENGTH_MEAN = 0, 1


class GuideParams(C.Structure):
    """pt_guide_params: how many mirror / glass surfaces the guide chains follow per pixel (include/pt_api.h)"""
    _fields_ = [("max_hops", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class BakedParams(C.Structure):
    """pt_baked_params: the hops the baked view's chains follow and the factor of a final surface without a usable map (include/pt_api.h)"""
    _fields_ = [("max_hops", C.c_uint32), ("unlit", C.c_float * 3), ("reserved", C.c_uint32 * 4)]


class RaysParams(C.Structure):
    """pt_rays_params: the draws a ray list's paths start with and the batch cut (include/pt_api.h)"""
    _fields_ = [("draws_consumed", C.c_uint32), ("batch_rays", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class ProbeParams(C.Structure):
    """pt_probe_params: the sample range and stream keys of a probe bake (include/pt_api.h)"""
    _fields_ = [("first_sample", C.c_uint32), ("n_samples", C.c_uint32), ("key_base", C.c_uint32), ("reserved", C.c_uint32)]


class ProbeGrid(C.Structure):
    """pt_probe_grid: where the nodes of the irradiance volume stand and the lookup's offset along the normal (include/pt_api.h)"""
    _fields_ = [("origin", C.c_float * 3), ("cell", C.c_float * 3), ("count", C.c_uint32 * 3), ("normal_bias", C.c_float),
                ("reserved", C.c_uint32 * 4)]


class ProbeDepthParams(C.Structure):
    """pt_probe_depth_params: the sample range and stream keys of a depth bake, the octahedral map's side and the distance clamp (include/pt_api.h)"""
    _fields_ = [("first_sample", C.c_uint32), ("n_samples", C.c_uint32), ("key_base", C.c_uint32), ("res", C.c_uint32), ("max_distance", C.c_float),
                ("reserved", C.c_uint32 * 3)]


class ProbeDepth(C.Structure):
    """pt_probe_depth: the side of the nodes' octahedral depth maps, PROBE_VIS_FACING and the visibility floor (include/pt_api.h)"""
    _fields_ = [("res", C.c_uint32), ("flags", C.c_uint32), ("vis_floor", C.c_float), ("reserved", C.c_uint32 * 5)]


class ProbeRadianceParams(C.Structure):
    """pt_probe_radiance_params: the sample range and stream keys of a radiance bake and the octahedral map's side (include/pt_api.h)"""
    _fields_ = [("first_sample", C.c_uint32), ("n_samples", C.c_uint32), ("key_base", C.c_uint32), ("res", C.c_uint32), ("reserved", C.c_uint32 * 4)]


class ProbeRadianceFilter(C.Structure):
    """pt_probe_radiance_filter: the maps' side, how many probes, and the GGX alphas of the levels the prefilter writes (include/pt_api.h)"""
    _fields_ = [("res", C.c_uint32), ("n_probes", C.c_uint32), ("n_levels", C.c_uint32), ("alpha", C.c_float * 8), ("reserved", C.c_uint32 * 5)]


class ProbeRadiance(C.Structure):
    """pt_probe_radiance: the side of the nodes' prefiltered radiance maps and their levels' GGX alphas (include/pt_api.h)"""
    _fields_ = [("res", C.c_uint32), ("n_levels", C.c_uint32), ("alpha", C.c_float * 8), ("reserved", C.c_uint32 * 6)]


class LightmapParams(C.Structure):
    """pt_lightmap_params: the placement, size, sample range, stream keys and ray bias of a lightmap bake (include/pt_api.h)"""
    _fields_ = [("model", C.c_int32), ("instance", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32), ("first_sample", C.c_uint32),
                ("n_samples", C.c_uint32), ("key_base", C.c_uint32), ("bias", C.c_float), ("reserved", C.c_uint32 * 4)]


class LightmapDirect(C.Structure):
    """pt_lightmap_direct: the stream keys of a direct bake's light samples (include/pt_api.h)"""
    _fields_ = [("light_key_base", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class BakedRaysParams(C.Structure):
    """pt_baked_rays_params"""
    _fields_ = [("baked", BakedParams), ("window_rays", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class LightmapGather(C.Structure):
    """pt_lightmap_gather"""
    _fields_ = [("baked", BakedParams), ("direct", C.c_uint32), ("light_key_base", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class LightmapDenoiseParams(C.Structure):
    """pt_lightmap_denoise_params: the placement and map, the samples in the sums, pt_denoise's filter parameters and the reach (include/pt_api.h)"""
    _fields_ = [("model", C.c_int32), ("instance", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32), ("n_samples", C.c_uint32),
                ("filter", DenoiseParams), ("reach", C.c_float), ("reserved", C.c_uint32 * 4)]


class SceneInfo(C.Structure):
    """pt_scene_info: which build and upload paths ran (include/pt_api.h)"""
    _fields_ = [("blas_builds", C.c_uint64), ("tlas_builds", C.c_uint64), ("uploads_full", C.c_uint64), ("uploads_patched", C.c_uint64),
                ("last_upload_bytes", C.c_uint64), ("scene_bytes", C.c_uint64), ("reserved", C.c_uint64 * 2)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}


class PtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libptmi error {code}: {msg}")
        self.code = code


_lib = None


def lib():
    """Load libptmi.so (building it in-tree if the sources are newer).  Raises if that is impossible."""
    global _lib
    if _lib is None:
        path = os.environ.get("PTMI_LIB")  # tuning builds only; the default is the in-tree library
        if not path:
            path = _build.LIB_PATH
            if _build.is_stale():
                path = _build.build()
        # One HIP runtime per process: torch ships its own libamdhip64 / libhsa-runtime64 / librccl, and a process that has already
        # opened the GPU through /opt/rocm's copies cannot open it again through torch's ("No HIP GPUs are available").  This module
        # hands device pointers to torch (framebuffer_tensor, dist.gather_framebuffer), so torch's copies go in first and libptmi binds
        # to them by soname.  A C/C++/Rust host that never loads torch uses /opt/rocm's runtime.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(path)
        vp, u32, f32p = C.c_void_p, C.c_uint32, C.c_void_p
        L.pt_create.restype = vp
        L.pt_create.argtypes = [C.POINTER(Config)]
        L.pt_destroy.argtypes = [vp]
        L.pt_last_error.restype = C.c_char_p
        L.pt_last_error.argtypes = [vp]
        L.pt_set_config.argtypes = [vp, C.POINTER(Config)]
        L.pt_add_material.argtypes = [vp, C.POINTER(MaterialDesc)]
        L.pt_add_model.argtypes = [vp, f32p, f32p, u32, C.c_int, f32p, u32]
        L.pt_add_model_obj.argtypes = [vp, C.c_char_p, C.c_int, f32p, u32]
        L.pt_model_vertices.argtypes = [vp, C.c_int, f32p, f32p, u32, C.POINTER(u32)]
        L.pt_build.argtypes = [vp]
        L.pt_set_camera.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, C.c_float]
        L.pt_camera_matrices.argtypes = [vp, vp, vp]
        L.pt_set_environment.argtypes = [vp, u32, u32, vp]
        L.pt_create_ray.argtypes = [vp, C.c_float, C.c_float, vp, vp]
        L.pt_set_lens.argtypes = [vp, C.c_float, C.c_float]
        L.pt_primary_ray.argtypes = [vp, u32, u32, vp, vp, C.POINTER(u32)]
        L.pt_set_projection.argtypes = [vp, C.POINTER(Projection)]
        L.pt_get_projection.argtypes = [vp, C.POINTER(Projection)]
        L.pt_render.argtypes = [vp, u32, u32, vp, vp, vp]
        L.pt_render_device.argtypes = [vp, u32, u32]
        L.pt_active_pixels.argtypes = [vp, vp, vp]
        L.pt_reset_accumulation.argtypes = [vp]
        L.pt_accum_device_ptr.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_uint64)]
        L.pt_read_accumulation.argtypes = [vp, vp]
        L.pt_write_accumulation.argtypes = [vp, vp, vp, vp]
        L.pt_read_frame.argtypes = [vp, vp, vp, vp]
        L.pt_render_samples.argtypes = [vp, u32, u32, vp]
        L.pt_render_adaptive.argtypes = [vp, C.POINTER(Adaptive), u32, C.POINTER(u32)]
        L.pt_adaptive_mask.argtypes = [vp, C.POINTER(Adaptive), vp, C.POINTER(u32)]
        L.pt_read_moments.argtypes = [vp, vp]
        L.pt_write_moments.argtypes = [vp, vp]
        L.pt_local_rows.argtypes = [vp, C.POINTER(u32), vp, u32]
        L.pt_set_stream.argtypes = [vp, vp]
        L.pt_synchronize.argtypes = [vp]
        L.pt_frame.argtypes = [vp, u32, vp, vp, vp, vp]
        L.pt_camera_input.argtypes = [vp, C.c_int, C.c_float, C.c_float, C.c_float]
        L.pt_camera_angles.argtypes = [vp, vp]
        L.pt_inv_projection.argtypes = [vp, vp]
        L.pt_present.argtypes = [vp, vp]
        L.pt_multi_create.restype = vp
        L.pt_multi_create.argtypes = [C.POINTER(Config), vp, u32]
        L.pt_multi_destroy.argtypes = [vp]
        L.pt_multi_last_error.restype = C.c_char_p
        L.pt_multi_last_error.argtypes = [vp]
        L.pt_multi_ctx.restype = vp
        L.pt_multi_ctx.argtypes = [vp, u32]
        L.pt_multi_render.argtypes = [vp, u32, u32, vp]
        L.pt_multi_framebuffer_device_ptr.argtypes = [vp, C.POINTER(vp)]
        L.pt_multi_reset_accumulation.argtypes = [vp]
        L.pt_multi_get_stats.argtypes = [vp, C.POINTER(Stats)]
        L.pt_multi_used_rccl.argtypes = [vp]
        L.pt_multi_write_image.argtypes = [vp, C.c_char_p]
        L.pt_post_velocity.argtypes = [vp, u32, u32, vp, vp, vp]
        L.pt_post_reproject.argtypes = [vp, u32, u32, vp, vp, vp, vp, vp]
        L.pt_post_tonemap.argtypes = [vp, u32, u32, vp, vp]
        L.pt_post_rgb8.argtypes = [vp, u32, u32, vp, vp]
        L.pt_present_rgb8.argtypes = [vp, vp]
        L.pt_write_image.argtypes = [vp, C.c_char_p]
        L.pt_trace_closest.argtypes = [vp, C.c_int, u32] + [vp] * 8
        L.pt_trace_any.argtypes = [vp, C.c_int, u32] + [vp] * 4
        L.pt_ss_sobol.argtypes = [vp, u32, u32, vp, vp, vp]
        L.pt_math_batch.argtypes = [vp, C.c_int, u32, vp, vp, vp, vp]
        L.pt_material_eval.argtypes = [vp, C.c_int, u32, vp, vp, vp, vp, vp, u32, vp]
        L.pt_volume_eval.argtypes = [vp, C.c_int, u32, vp, vp, vp, vp, vp, u32, vp]
        L.pt_bsdf_eval.argtypes = [vp, C.c_int, u32, vp, vp, vp, vp, vp]
        L.pt_blas_count.argtypes = [vp]
        L.pt_blas_dump.argtypes = [vp, C.c_int] + [vp] * 8 + [u32, u32]
        L.pt_tlas_dump.argtypes = [vp, C.c_int] + [vp] * 6 + [u32]
        L.pt_tlas_instances.argtypes = [vp, C.c_int, vp, vp, vp, u32]
        L.pt_instance_materials.argtypes = [vp, C.c_int, vp, vp, vp, u32]
        L.pt_light_cdf.argtypes = [vp] + [vp] * 6 + [u32]
        L.pt_triangle_dump.argtypes = [vp, C.c_int, u32, vp]
        L.pt_get_stats.argtypes = [vp, C.POINTER(Stats)]
        L.pt_reset_stats.argtypes = [vp]
        L.pt_last_batch_counters.argtypes = [vp, vp, u32, C.POINTER(u32)]
        L.pt_last_launches.argtypes = [vp, u32, vp, u32, C.POINTER(u32)]
        L.pt_trace_geometry.argtypes = [vp, vp]
        L.pt_variant_axes.argtypes = [u32, vp]
        L.pt_variant_compiled.argtypes = [u32, vp]
        L.pt_last_batch_shade_pids.argtypes = [vp, u32, u32, u32, vp]
        L.pt_render_guides.argtypes = [vp, u32]
        L.pt_read_guides.argtypes = [vp, vp, vp, vp]
        L.pt_denoise.argtypes = [vp, C.POINTER(DenoiseParams), vp]
        L.pt_write_denoised_image.argtypes = [vp, C.c_char_p]
        L.pt_post_denoise.argtypes = [vp, u32, u32, C.POINTER(DenoiseParams), vp, vp, vp, vp, vp, vp]
        L.pt_integrate_rays.argtypes = [vp, C.c_uint64, vp, vp, vp, vp, C.POINTER(RaysParams), vp, vp, vp]
        L.pt_integrate_rays_device.argtypes = [vp, C.c_uint64, vp, vp, vp, vp, C.POINTER(RaysParams), vp, vp, vp]
        L.pt_bake_probes.argtypes = [vp, u32, vp, C.POINTER(ProbeParams), vp]
        L.pt_probe_ray.argtypes = [vp, u32, u32, vp, vp]
        L.pt_set_instances.argtypes = [vp, C.c_int, f32p, u32]
        L.pt_get_scene_info.argtypes = [vp, C.POINTER(SceneInfo)]
        L.pt_read_guide_instances.argtypes = [vp, vp]
        L.pt_frame_moving.argtypes = [vp, u32, vp, vp, vp, vp]
        L.pt_post_motion.argtypes = [vp, u32, u32, vp, vp, u32, vp, vp, vp, vp, vp]
        L.pt_add_texture.argtypes = [vp, u32, u32, vp]
        L.pt_set_material_texture.argtypes = [vp, C.c_int, C.c_int]
        L.pt_set_material_emission_texture.argtypes = [vp, C.c_int, C.c_int]
        L.pt_set_material_normal_texture.argtypes = [vp, C.c_int, C.c_int]
        L.pt_shading_normal.argtypes = [vp, C.c_int, u32, vp, vp, vp, vp, vp, vp, vp]
        L.pt_set_material_roughness_texture.argtypes = [vp, C.c_int, C.c_int]
        L.pt_surface_roughness.argtypes = [vp, C.c_int, u32, vp, vp, vp, vp, vp]
        L.pt_set_model_uvs.argtypes = [vp, C.c_int, vp, u32]
        L.pt_model_uvs.argtypes = [vp, C.c_int, vp, u32, C.POINTER(u32)]
        L.pt_surface_colour.argtypes = [vp, C.c_int, u32, vp, vp, vp, vp, vp]
        L.pt_read_guide_albedo.argtypes = [vp, vp]
        L.pt_accumulate_albedo.argtypes = [vp, u32, u32]
        L.pt_reset_albedo.argtypes = [vp]
        L.pt_read_albedo.argtypes = [vp, vp]
        L.pt_denoise_albedo.argtypes = [vp, C.POINTER(DenoiseParams), u32, vp]
        L.pt_post_denoise_albedo.argtypes = [vp, u32, u32, C.POINTER(DenoiseParams), vp, vp, vp, vp, vp, vp, vp]
        L.pt_bake_lightmap.argtypes = [vp, C.POINTER(LightmapParams), vp, vp]
        L.pt_lightmap_texels.argtypes = [vp, C.c_int, u32, u32, u32, C.c_int, vp, vp, vp, vp]
        L.pt_lightmap_ray.argtypes = [vp, u32, u32, vp, vp]
        L.pt_lightmap_dilate.argtypes = [vp, u32, u32, u32, vp, vp]
        L.pt_bake_lightmap_moments.argtypes = [vp, C.POINTER(LightmapParams), vp, vp, vp]
        L.pt_lightmap_denoise.argtypes = [vp, C.c_int, C.POINTER(LightmapDenoiseParams), vp, vp, vp, vp]
        L.pt_bake_lightmap_adaptive.argtypes = [vp, C.POINTER(LightmapParams), C.POINTER(Adaptive), vp, vp, vp, vp, C.POINTER(u32)]
        L.pt_lightmap_adaptive_mask.argtypes = [vp, C.c_int, C.c_int, u32, u32, u32, C.POINTER(Adaptive), vp, vp, vp, vp, C.POINTER(u32)]
        L.pt_lightmap_denoise_counts.argtypes = [vp, C.c_int, C.POINTER(LightmapDenoiseParams), vp, vp, vp, vp, vp]
        L.pt_bake_lightmap_direct.argtypes = [vp, C.POINTER(LightmapParams), C.POINTER(LightmapDirect), vp, vp, vp]
        L.pt_bake_lightmap_adaptive_direct.argtypes = [vp, C.POINTER(LightmapParams), C.POINTER(LightmapDirect), C.POINTER(Adaptive), vp, vp, vp, vp, C.POINTER(u32)]
        L.pt_lightmap_light_sample.argtypes = [vp, C.c_int, u32, vp, vp, vp, vp, vp, vp, vp, vp]
        L.pt_baked_rays.argtypes = [vp, C.c_uint64, vp, vp, C.POINTER(BakedRaysParams), vp, vp]
        L.pt_baked_rays_device.argtypes = [vp, C.c_uint64, vp, vp, C.POINTER(BakedRaysParams), vp, vp]
        L.pt_bake_lightmap_gather.argtypes = [vp, C.POINTER(LightmapParams), C.POINTER(LightmapGather), vp, vp, vp]
        L.pt_bake_lightmap_adaptive_gather.argtypes = [vp, C.POINTER(LightmapParams), C.POINTER(LightmapGather), C.POINTER(Adaptive), vp, vp, vp, vp, C.POINTER(u32)]
        L.pt_set_lightmap.argtypes = [vp, C.c_int, u32, u32, u32, vp]
        L.pt_get_lightmap_info.argtypes = [vp, C.c_int, u32, vp, vp]
        L.pt_lightmap_lookup.argtypes = [vp, C.c_int, u32, vp, vp, vp, vp, vp, vp]
        L.pt_render_baked.argtypes = [vp, u32, u32, C.POINTER(BakedParams), vp]
        L.pt_bake_lightmap_directional.argtypes = [vp, C.POINTER(LightmapParams), vp, vp, vp]
        L.pt_lightmap_gradient.argtypes = [vp, C.c_int, C.c_int, u32, u32, u32, u32, vp, vp]
        L.pt_set_lightmap_directional.argtypes = [vp, C.c_int, u32, u32, u32, vp]
        L.pt_get_lightmap_directional_info.argtypes = [vp, C.c_int, u32, vp]
        L.pt_lightmap_lookup_directional.argtypes = [vp, C.c_int, u32, vp, vp, vp, vp, vp, vp, vp]
        L.pt_read_baked.argtypes = [vp, vp]
        L.pt_reset_baked.argtypes = [vp]
        L.pt_write_baked_image.argtypes = [vp, C.c_char_p]
        L.pt_set_probe_grid.argtypes = [vp, C.POINTER(ProbeGrid), vp, vp]
        L.pt_get_probe_grid_info.argtypes = [vp, C.POINTER(ProbeGrid), C.POINTER(u32)]
        L.pt_probe_grid_lookup.argtypes = [vp, C.c_int, u32, vp, vp, vp, vp]
        L.pt_probe_backfaces.argtypes = [vp, u32, vp, C.POINTER(ProbeParams), vp, vp]
        L.pt_probe_depth_texel.argtypes = [u32, u32, vp, vp]
        L.pt_bake_probe_depth.argtypes = [vp, u32, vp, C.POINTER(ProbeDepthParams), vp, vp]
        L.pt_set_probe_grid_depth.argtypes = [vp, C.POINTER(ProbeDepth), vp]
        L.pt_get_probe_grid_depth_info.argtypes = [vp, C.POINTER(ProbeDepth)]
        L.pt_probe_radiance_dir.argtypes = [u32, u32, vp, vp, vp]
        L.pt_bake_probe_radiance.argtypes = [vp, u32, vp, C.POINTER(ProbeRadianceParams), vp, vp]
        L.pt_probe_radiance_prefilter.argtypes = [vp, C.c_int, C.POINTER(ProbeRadianceFilter), vp, vp, vp]
        L.pt_set_probe_grid_radiance.argtypes = [vp, C.POINTER(ProbeRadiance), vp]
        L.pt_get_probe_grid_radiance_info.argtypes = [vp, C.POINTER(ProbeRadiance)]
        L.pt_probe_grid_specular.argtypes = [vp, C.c_int, u32, vp, vp, vp, vp, vp, vp]
        L.pt_render_guides_followed.argtypes = [vp, u32, C.POINTER(GuideParams)]
        L.pt_read_guide_hops.argtypes = [vp, vp]
        L.pt_accumulate_albedo_followed.argtypes = [vp, u32, u32, C.POINTER(GuideParams)]
        L.pt_guide_follow_dir.argtypes = [vp, C.c_int, C.c_int, u32, vp, vp, vp, vp]
        L.pt_frame_temporal.argtypes = [vp, u32, vp, C.POINTER(TemporalParams), C.POINTER(DenoiseParams), vp, vp, vp, vp]
        L.pt_read_temporal.argtypes = [vp, vp, vp, vp]
        L.pt_reset_temporal.argtypes = [vp]
        L.pt_post_temporal.argtypes = [vp, C.c_int, u32, u32, C.POINTER(TemporalParams), C.POINTER(DenoiseParams)] + [vp] * 15
        L.pt_frame_temporal_options.argtypes = [vp, u32, vp, C.POINTER(TemporalParams), C.POINTER(TemporalOptions), C.POINTER(DenoiseParams), vp, vp, vp, vp]
        L.pt_post_temporal_options.argtypes = [vp, C.c_int, u32, u32, C.POINTER(TemporalParams), C.POINTER(TemporalOptions), C.POINTER(DenoiseParams)] + [vp] * 15
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def variant_axes(launcher):
    """pt_variant_axes: the number of values of each axis of a keyed launcher (a name of LAUNCHERS), in order.  Needs no device."""
    b = np.zeros(6, np.uint32)
    n = lib().pt_variant_axes(LAUNCHERS.index(launcher), _p(b))
    if n <= 0:
        raise PtError(n, f"no launcher {launcher}")
    return tuple(int(v) for v in b[:n])


def variant_compiled(launcher, axes):
    """pt_variant_compiled: is this point of the launcher's axes a kernel of the library?  Needs no device."""
    a = np.zeros(6, np.uint32)
    a[: len(axes)] = axes
    return bool(lib().pt_variant_compiled(LAUNCHERS.index(launcher), _p(a)))


def compiled_variants(launcher):
    """every compiled point of a keyed launcher's axes as (launcher, axis values)"""
    import itertools
    return {(launcher, p) for p in itertools.product(*[range(n) for n in variant_axes(launcher)]) if variant_compiled(launcher, p)}


class Renderer:
    """Scene + Camera + integrator behind one pt_ctx."""

    def __init__(self, scene: SceneDesc, width: int, height: int, max_bounces: int = 8, n_sobol: int = 512, enable_nee: bool = True,
                 seed: int = DEFAULT_SEED, rank: int = 0, world_size: int = 1, strip_rows: int = 4, batch_spp: int = 0, device: int = -1,
                 flags: int = 0, stack_lds_levels: int = 0, queue_slack: int = 0, pipelines: int = 0):
        self.L = lib()
        self.cfg = Config(width, height, max_bounces, n_sobol, int(enable_nee), seed, rank, world_size, strip_rows, batch_spp, device, flags,
                          stack_lds_levels, queue_slack, pipelines, 0)
        self.ctx = C.c_void_p(self.L.pt_create(C.byref(self.cfg)))
        if not self.ctx:
            raise PtError(-1, "pt_create failed (bad configuration)")
        self.desc = scene
        self._materials = []
        self._textures = []
        for mod in scene.models:
            self.add_model(mod)
        self.rebuild()
        if scene.camera is not None:
            self.set_camera(scene.camera)

    def _material_index(self, m) -> int:
        """pt_add_material once per distinct material, in first-use order (SceneDesc.materials() gives the same indices)"""
        if m not in self._materials:
            d = MaterialDesc()
            d.kind = m.kind
            d.colour[:] = m.colour
            d.roughness, d.ior = m.roughness, m.ior
            if m.volume is not None:
                d.has_volume = 1
                d.vol_absorption[:] = m.volume.absorption
                d.vol_k, d.vol_c, d.vol_g = m.volume.k, m.volume.c, m.volume.g
            mi = self._chk(self.L.pt_add_material(self.ctx, C.byref(d)), allow_positive=True)
            self._materials.append(m)
            if getattr(m, "texture", None) is not None:
                self.set_material_texture(mi, self._texture_index(m.texture))
            if getattr(m, "emission_texture", None) is not None:
                self.set_material_emission_texture(mi, self._texture_index(m.emission_texture))
            if getattr(m, "normal_texture", None) is not None:
                self.set_material_normal_texture(mi, self._texture_index(m.normal_texture))
            if getattr(m, "roughness_texture", None) is not None:
                self.set_material_roughness_texture(mi, self._texture_index(m.roughness_texture))
        return self._materials.index(m)

    def _texture_index(self, t) -> int:
        """pt_add_texture once per distinct Texture object"""
        for i, have in enumerate(self._textures):
            if have is t:
                return i
        self.add_texture(t.data)
        self._textures[-1] = t
        return len(self._textures) - 1

    def add_model(self, mod) -> int:
        """Model::new + push onto the scene's model list; call rebuild() (Scene::new) before the next render"""
        mi = self._material_index(mod.material)
        if getattr(mod, "obj_path", None):
            r = self._chk(self.L.pt_add_model_obj(self.ctx, mod.obj_path.encode(), mi, _p(mod.matrices), mod.matrices.shape[0]), allow_positive=True)
        else:
            r = self._chk(self.L.pt_add_model(self.ctx, _p(mod.positions), _p(mod.normals), mod.positions.shape[0], mi, _p(mod.matrices),
                                              mod.matrices.shape[0]), allow_positive=True)
        if getattr(mod, "uvs", None) is not None:
            self.set_model_uvs(r, mod.uvs)
        return r

    # ---- textured surface colour (include/pt_api.h); the texture setters un-build the scene: rebuild() before the next render
    def add_texture(self, rgb) -> int:
        """[h, w, 3] linear RGB, finite and non-negative; returns the texture index"""
        a = np.ascontiguousarray(rgb, dtype=np.float32)
        assert a.ndim == 3 and a.shape[2] == 3
        r = self._chk(self.L.pt_add_texture(self.ctx, a.shape[1], a.shape[0], _p(a)), allow_positive=True)
        self._textures.append(None)
        return r

    def set_material_texture(self, material: int, texture: int):
        """texture -1 clears"""
        self._chk(self.L.pt_set_material_texture(self.ctx, material, texture))

    def set_material_emission_texture(self, material: int, texture: int):
        """the emission texture of an EMISSIVE material (textured area light; include/pt_api.h); texture -1 clears"""
        self._chk(self.L.pt_set_material_emission_texture(self.ctx, material, texture))

    def set_material_normal_texture(self, material: int, texture: int):
        """the tangent-space normal map of a material of any kind but EMISSIVE (include/pt_api.h); texture -1 clears"""
        self._chk(self.L.pt_set_material_normal_texture(self.ctx, material, texture))

    def set_material_roughness_texture(self, material: int, texture: int):
        """the roughness map of a GGX material: the texel's first component is the hit's linear roughness (include/pt_api.h); texture -1 clears"""
        self._chk(self.L.pt_set_material_roughness_texture(self.ctx, material, texture))

    def set_model_uvs(self, model: int, uvs):
        """[n_tris, 3, 2] in load order; None clears"""
        if uvs is None:
            self._chk(self.L.pt_set_model_uvs(self.ctx, model, None, 0))
            return
        a = np.ascontiguousarray(uvs, dtype=np.float32).reshape(-1, 3, 2)
        self._chk(self.L.pt_set_model_uvs(self.ctx, model, _p(a), a.shape[0]))

    def model_uvs(self, model):
        """[n_tris, 3, 2], or None for a model without UVs"""
        n = C.c_uint32()
        self._chk(self.L.pt_model_uvs(self.ctx, model, None, 0, C.byref(n)))
        if n.value == 0:
            return None
        uv = np.zeros((n.value, 3, 2), np.float32)
        self._chk(self.L.pt_model_uvs(self.ctx, model, _p(uv), n.value, C.byref(n)))
        return uv

    def surface_colour(self, instance, prim, u, v, on_device=False):
        """unit hook: the surface colour [n, 3] of hits (world-TLAS instance, load-order primitive, barycentrics) of the built scene;
        on the host (no GPU) unless on_device"""
        i = np.ascontiguousarray(instance, dtype=np.uint32); p = np.ascontiguousarray(prim, dtype=np.uint32)
        uu = np.ascontiguousarray(u, dtype=np.float32); vv = np.ascontiguousarray(v, dtype=np.float32)
        assert i.shape == p.shape == uu.shape == vv.shape and i.ndim == 1
        out = np.zeros((i.shape[0], 3), np.float32)
        self._chk(self.L.pt_surface_colour(self.ctx, int(bool(on_device)), i.shape[0], _p(i), _p(p), _p(uu), _p(vv), _p(out)))
        return out

    def surface_roughness(self, instance, prim, u, v, on_device=False):
        """unit hook: the GGX alpha [n] of hits (world-TLAS instance, load-order primitive, barycentrics) of the built scene, roughness maps
        applied; the stored alpha of an unmapped GGX material, 0 for a kind that is not GGX; on the host (no GPU) unless on_device"""
        i = np.ascontiguousarray(instance, dtype=np.uint32); p = np.ascontiguousarray(prim, dtype=np.uint32)
        uu = np.ascontiguousarray(u, dtype=np.float32); vv = np.ascontiguousarray(v, dtype=np.float32)
        assert i.shape == p.shape == uu.shape == vv.shape and i.ndim == 1
        out = np.zeros(i.shape[0], np.float32)
        self._chk(self.L.pt_surface_roughness(self.ctx, int(bool(on_device)), i.shape[0], _p(i), _p(p), _p(uu), _p(vv), _p(out)))
        return out

    def shading_normal(self, instance, prim, u, v, direction, on_device=False):
        """unit hook: the world shading normal [n, 3] and the front flag [n] (uint8) of hits (world-TLAS instance, load-order primitive,
        barycentrics, world ray direction [n, 3]) of the built scene, normal maps applied; on the host (no GPU) unless on_device"""
        i = np.ascontiguousarray(instance, dtype=np.uint32); p = np.ascontiguousarray(prim, dtype=np.uint32)
        uu = np.ascontiguousarray(u, dtype=np.float32); vv = np.ascontiguousarray(v, dtype=np.float32)
        d = np.ascontiguousarray(direction, dtype=np.float32)
        assert i.shape == p.shape == uu.shape == vv.shape and i.ndim == 1 and d.shape == (i.shape[0], 3)
        out = np.zeros((i.shape[0], 3), np.float32)
        front = np.zeros(i.shape[0], np.uint8)
        self._chk(self.L.pt_shading_normal(self.ctx, int(bool(on_device)), i.shape[0], _p(i), _p(p), _p(uu), _p(vv), _p(d), _p(out), _p(front)))
        return out, front

    def rebuild(self):
        self._chk(self.L.pt_build(self.ctx))

    def set_instances(self, model: int, matrices):
        """replace the instance matrices of a model ([n, 3, 4] row-major rigid transforms, n may be 0); call rebuild() before the next render"""
        m = np.ascontiguousarray(np.zeros((0, 3, 4), np.float32) if matrices is None else matrices, dtype=np.float32).reshape(-1, 3, 4)
        self._chk(self.L.pt_set_instances(self.ctx, model, _p(m) if m.shape[0] else None, m.shape[0]))

    def scene_info(self) -> SceneInfo:
        """which build and upload paths ran: BLAS / TLAS builds, full and patched scene uploads, bytes of the last upload"""
        out = SceneInfo()
        self._chk(self.L.pt_get_scene_info(self.ctx, C.byref(out)))
        return out

    # ---- plumbing
    def _chk(self, r, allow_positive=False):
        if r < 0 or (r != 0 and not allow_positive):
            raise PtError(r, self.L.pt_last_error(self.ctx).decode())
        return r

    @classmethod
    def attach(cls, ctx, cfg):
        """Wrap a context somebody else owns (a member of a MultiRenderer): same calls, close() leaves it alone."""
        self = cls.__new__(cls)
        self.L = lib()
        self.cfg = cfg
        self.ctx = C.c_void_p(ctx)
        self.desc = None
        self._materials = []
        self._textures = []
        self._borrowed = True
        return self

    def close(self):
        if getattr(self, "ctx", None):
            if not getattr(self, "_borrowed", False):
                self.L.pt_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_config(self, **kw):
        """pt_set_config with the given fields changed.  A refused call leaves the context AND self.cfg (which sizes every host buffer) as they were."""
        new = Config.from_buffer_copy(self.cfg)
        for k, v in kw.items():
            if not hasattr(Config, k):
                raise AttributeError(f"pt_config has no field {k!r}")
            setattr(new, k, v)
        self._chk(self.L.pt_set_config(self.ctx, C.byref(new)))
        self.cfg = new

    def set_camera(self, cam: CameraDesc):
        """Camera::new: the view and, with it, the description's thin lens (aperture 0 = pinhole)"""
        self._chk(self.L.pt_set_camera(self.ctx, _f3(cam.origin), _f3(cam.target), cam.fov, cam.aspect_ratio))
        self.set_lens(cam.aperture, cam.focus)

    def set_lens(self, aperture: float, focus: float):
        """thin lens (pt_set_lens): aperture = lens diameter in world units (0 = pinhole), focus = distance of the plane of focus"""
        self._chk(self.L.pt_set_lens(self.ctx, aperture, focus))

    def set_projection(self, kind: int, span_x: float = 0.0, span_y: float = 0.0, ortho_height: float = 0.0):
        """pt_set_projection: PROJ_PERSPECTIVE (the camera as it is), PROJ_PANORAMA (span_x x span_y degrees of azimuth / elevation, 0 = 360 / 180)
        or PROJ_ORTHOGRAPHIC (a view volume ortho_height world units high)"""
        p = Projection(int(kind), span_x, span_y, ortho_height)
        self._chk(self.L.pt_set_projection(self.ctx, C.byref(p)))

    def get_projection(self):
        """(kind, span_x, span_y, ortho_height) as pt_set_projection last accepted them"""
        p = Projection()
        self._chk(self.L.pt_get_projection(self.ctx, C.byref(p)))
        return int(p.kind), float(p.span_x_deg), float(p.span_y_deg), float(p.ortho_height)

    def camera_input(self, event, a=0.0, b=0.0, dt=0.0) -> bool:
        """Camera::input (camera.rs:56-92): event = EV_MOUSE_MOTION (a, b = delta) or EV_KEY_W/S/A/D; True if consumed"""
        return bool(self._chk(self.L.pt_camera_input(self.ctx, int(event), a, b, dt), allow_positive=True))

    def camera_angles(self):
        out = np.zeros(2, np.float32)
        self._chk(self.L.pt_camera_angles(self.ctx, _p(out)))
        return out

    def set_environment(self, rgb):
        """rgb: (h, w, 3) linear float32 equirect image, or None for the constant-ambient branch."""
        if rgb is None:
            self._chk(self.L.pt_set_environment(self.ctx, 0, 0, None))
        else:
            rgb = np.ascontiguousarray(rgb, np.float32)
            self._chk(self.L.pt_set_environment(self.ctx, rgb.shape[1], rgb.shape[0], _p(rgb)))

    def set_stream(self, hip_stream: Optional[int]):
        self._chk(self.L.pt_set_stream(self.ctx, C.c_void_p(hip_stream) if hip_stream else None))

    def synchronize(self):
        self._chk(self.L.pt_synchronize(self.ctx))

    # ---- geometry of the local framebuffer
    def local_rows(self) -> np.ndarray:
        n = C.c_uint32()
        self._chk(self.L.pt_local_rows(self.ctx, C.byref(n), None, 0))
        rows = np.zeros(n.value, np.uint32)
        self._chk(self.L.pt_local_rows(self.ctx, C.byref(n), _p(rows), n.value))
        return rows

    @property
    def width(self):
        return self.cfg.width

    # ---- Camera
    def camera_matrices(self):
        m = np.zeros(12, np.float32)
        ip = np.zeros(16, np.float32)
        self._chk(self.L.pt_camera_matrices(self.ctx, _p(m), _p(ip)))
        return m.reshape(3, 4), ip.reshape(4, 4).T.copy()

    def create_ray(self, s, t):
        o = np.zeros(3, np.float32)
        d = np.zeros(3, np.float32)
        self._chk(self.L.pt_create_ray(self.ctx, s, t, _p(o), _p(d)))
        return o, d

    def primary_ray(self, pixel: int, sample: int):
        """(origin, direction, stream draws consumed) of the camera ray of (global pixel, sample) under the lens or projection in force; host evaluation"""
        o = np.zeros(3, np.float32)
        d = np.zeros(3, np.float32)
        n = C.c_uint32()
        self._chk(self.L.pt_primary_ray(self.ctx, pixel, sample, _p(o), _p(d), C.byref(n)))
        return o, d, n.value

    # ---- integrate over the frame
    def render(self, first_sample: int, n_samples: int, ident: Optional[np.ndarray] = None, want_position=True):
        rows = len(self.local_rows())
        acc = np.zeros((rows, self.cfg.width, 4), np.float32)
        pos = np.zeros((rows, self.cfg.width, 4), np.float32) if want_position else None
        idb = np.zeros((rows, self.cfg.width), np.uint32) if ident is None else ident
        self._chk(self.L.pt_render(self.ctx, first_sample, n_samples, _p(acc), _p(pos), _p(idb)))
        return acc, pos, idb

    def active_pixels(self):
        """(x0, width, local row0, rows) of the rectangle camera rays are generated for, and the world root box (min xyz, max xyz)"""
        rect = np.zeros(4, np.uint32); box = np.zeros(6, np.float32)
        self._chk(self.L.pt_active_pixels(self.ctx, _p(rect), _p(box)))
        return tuple(int(v) for v in rect), box

    def render_device(self, first_sample: int, n_samples: int):
        self._chk(self.L.pt_render_device(self.ctx, first_sample, n_samples))

    def render_samples(self, first_sample: int, n_samples: int):
        rows = len(self.local_rows())
        out = np.zeros((n_samples, rows, self.cfg.width, 4), np.float32)
        self._chk(self.L.pt_render_samples(self.ctx, first_sample, n_samples, _p(out)))
        return out

    def reset_accumulation(self):
        self._chk(self.L.pt_reset_accumulation(self.ctx))

    # ---- adaptive sampling (FLAG_ADAPTIVE)
    @staticmethod
    def _adaptive(rel_error, abs_floor, min_samples, max_samples):
        return Adaptive(rel_error, abs_floor, min_samples, max_samples)

    def render_adaptive(self, n_samples: int, rel_error: float, abs_floor: float = 0.0, min_samples: int = 2, max_samples: int = 0) -> int:
        """Select the pixels whose mean luminance is not yet known to rel_error (pt_adaptive), then render n_samples more samples for each
        of them, continuing from each pixel's own count.  Returns the number of selected pixels; the frame stays on the device (read_frame)."""
        n = C.c_uint32(0)
        crit = self._adaptive(rel_error, abs_floor, min_samples, max_samples)
        self._chk(self.L.pt_render_adaptive(self.ctx, C.byref(crit), n_samples, C.byref(n)))
        return n.value

    def adaptive_mask(self, rel_error: float, abs_floor: float = 0.0, min_samples: int = 2, max_samples: int = 0) -> np.ndarray:
        """The selection alone: bool per local pixel (local rows x width), True = would be rendered"""
        mask = np.zeros((len(self.local_rows()), self.cfg.width), np.uint8)
        n = C.c_uint32(0)
        crit = self._adaptive(rel_error, abs_floor, min_samples, max_samples)
        self._chk(self.L.pt_adaptive_mask(self.ctx, C.byref(crit), _p(mask), C.byref(n)))
        assert int(mask.sum()) == n.value
        return mask.astype(bool)

    def read_moments(self) -> np.ndarray:
        """Q, the sum of the squared luminance of every accumulated sample, per local pixel (local rows x width, f32)"""
        q = np.zeros((len(self.local_rows()), self.cfg.width), np.float32)
        self._chk(self.L.pt_read_moments(self.ctx, _p(q)))
        return q

    def write_moments(self, sumsq):
        """Restore Q beside write_accumulation (checkpoint / resume of an adaptive render)"""
        q = np.ascontiguousarray(sumsq, np.float32)
        if q.size != len(self.local_rows()) * self.cfg.width:
            raise PtError(-1, f"write_moments: not one value per local pixel of a {self.cfg.width}-wide frame")
        self._chk(self.L.pt_write_moments(self.ctx, _p(q)))

    def read_accumulation(self):
        rows = len(self.local_rows())
        acc = np.zeros((rows, self.cfg.width, 4), np.float32)
        self._chk(self.L.pt_read_accumulation(self.ctx, _p(acc)))
        return acc

    def read_frame(self):
        """(accumulation, position, id history) as they lie on the device, e.g. after render_device()"""
        rows = len(self.local_rows())
        acc = np.zeros((rows, self.cfg.width, 4), np.float32); pos = np.zeros((rows, self.cfg.width, 4), np.float32); idb = np.zeros((rows, self.cfg.width), np.uint32)
        self._chk(self.L.pt_read_frame(self.ctx, _p(acc), _p(pos), _p(idb)))
        return acc, pos, idb

    def write_accumulation(self, data, position=None, ident=None):
        """Restore a frame's state (what render() returned) into this context: checkpoint / resume across contexts."""
        data = np.ascontiguousarray(data, np.float32)
        pos = None if position is None else np.ascontiguousarray(position, np.float32)
        idb = None if ident is None else np.ascontiguousarray(ident, np.uint32)
        px = self.cfg.width * self.cfg.height      # the library copies width * height texels from each pointer
        if data.size != px * 4 or (pos is not None and pos.size != px * 4) or (idb is not None and idb.size != px):
            raise PtError(-1, f"write_accumulation: arrays are not those of a {self.cfg.width}x{self.cfg.height} frame")
        self._chk(self.L.pt_write_accumulation(self.ctx, _p(data), None if pos is None else _p(pos), None if idb is None else _p(idb)))

    def accum_device_ptr(self):
        p = C.c_void_p()
        n = C.c_uint64()
        self._chk(self.L.pt_accum_device_ptr(self.ctx, C.byref(p), C.byref(n)))
        return p.value, n.value

    # ---- after the path: State::update / State::render
    def inv_projection(self):
        m = np.zeros(16, np.float32)
        self._chk(self.L.pt_inv_projection(self.ctx, _p(m)))
        return m

    def frame(self, frame_index, last_inv_projection=None, ident=None, download=True):
        """one event-loop iteration (main.rs:179-218): 1 spp pixel loop + State::update; returns data, position, id
        (download=False keeps everything on the device: the id history then lives in the library's own texture)"""
        m = None if last_inv_projection is None else np.ascontiguousarray(last_inv_projection, np.float32)
        if not download:
            self._chk(self.L.pt_frame(self.ctx, frame_index, _p(m), None, None, None))
            return None
        h, w = self.cfg.height, self.cfg.width
        data = np.zeros((h, w, 4), np.float32); pos = np.zeros((h, w, 4), np.float32)
        idb = np.zeros((h, w), np.uint32) if ident is None else ident
        self._chk(self.L.pt_frame(self.ctx, frame_index, _p(m), _p(data), _p(pos), _p(idb)))
        return data, pos, idb

    def frame_moving(self, frame_index, last_inv_projection=None, ident=None, download=True):
        """frame() with a world that may have moved since the previous frame_moving (set_instances + rebuild): the history is reprojected by
        the camera's AND the instances' motion; leaves the guides of this sample valid (frame_moving(k), denoise())"""
        m = None if last_inv_projection is None else np.ascontiguousarray(last_inv_projection, np.float32)
        if not download:
            self._chk(self.L.pt_frame_moving(self.ctx, frame_index, _p(m), None, None, None))
            return None
        h, w = self.cfg.height, self.cfg.width
        data = np.zeros((h, w, 4), np.float32); pos = np.zeros((h, w, 4), np.float32)
        idb = np.zeros((h, w), np.uint32) if ident is None else ident
        self._chk(self.L.pt_frame_moving(self.ctx, frame_index, _p(m), _p(data), _p(pos), _p(idb)))
        return data, pos, idb

    def present(self):
        out = np.zeros((self.cfg.height, self.cfg.width, 4), np.float32)
        self._chk(self.L.pt_present(self.ctx, _p(out)))
        return out

    def present_rgb8(self):
        out = np.zeros((self.cfg.height, self.cfg.width, 3), np.uint8)
        self._chk(self.L.pt_present_rgb8(self.ctx, _p(out)))
        return out

    def write_image(self, path):
        self._chk(self.L.pt_write_image(self.ctx, str(path).encode()))

    def post_rgb8(self, accum):
        accum = np.ascontiguousarray(accum, np.float32)
        h, w = accum.shape[:2]
        out = np.zeros((h, w, 3), np.uint8)
        self._chk(self.L.pt_post_rgb8(self.ctx, w, h, _p(accum), _p(out)))
        return out

    def post_velocity(self, position, last_inv_projection):
        position = np.ascontiguousarray(position, np.float32)
        h, w = position.shape[:2]
        v = np.zeros((h, w, 2), np.float32)
        self._chk(self.L.pt_post_velocity(self.ctx, w, h, _p(position), _p(np.ascontiguousarray(last_inv_projection, np.float32)), _p(v)))
        return v

    def post_motion(self, position, instance, matrix12, inv_matrix12, prev_matrix12, has_prev=None):
        """x_prev of frame_moving on caller images: where each pixel's first hit was under its instance's previous matrix"""
        position = np.ascontiguousarray(position, np.float32); instance = np.ascontiguousarray(instance, np.uint32)
        h, w = position.shape[:2]
        tabs = [np.ascontiguousarray(t, np.float32).reshape(-1, 12) for t in (matrix12, inv_matrix12, prev_matrix12)]
        n = tabs[0].shape[0]
        assert all(t.shape[0] == n for t in tabs)
        hp = None if has_prev is None else np.ascontiguousarray(has_prev, np.uint8)
        assert hp is None or hp.shape == (n,)
        out = np.zeros((h, w, 4), np.float32)
        self._chk(self.L.pt_post_motion(self.ctx, w, h, _p(position), _p(instance), n, *[_p(t) if n else None for t in tabs], _p(hp), _p(out)))
        return out

    def post_reproject(self, inp, accum, velocity, ident):
        inp = np.ascontiguousarray(inp, np.float32); accum = np.ascontiguousarray(accum, np.float32)
        velocity = np.ascontiguousarray(velocity, np.float32); ident = np.ascontiguousarray(ident, np.uint32)
        h, w = inp.shape[:2]
        out = np.zeros((h, w, 4), np.float32)
        self._chk(self.L.pt_post_reproject(self.ctx, w, h, _p(inp), _p(accum), _p(velocity), _p(ident), _p(out)))
        return out

    def post_tonemap(self, accum):
        accum = np.ascontiguousarray(accum, np.float32)
        h, w = accum.shape[:2]
        out = np.zeros((h, w, 4), np.float32)
        self._chk(self.L.pt_post_tonemap(self.ctx, w, h, _p(accum), _p(out)))
        return out

    # ---- denoising: first-hit guides + edge-aware a-trous filter
    def render_guides(self, sample: int, follow: int = 0):
        """trace the camera ray of `sample` of every local pixel: first-hit position, normal and model guides stay on the device.
        follow = K > 0 (pt_render_guides_followed): mirrors and glass are followed, up to K of them per pixel, and the guides are those
        of the surface the chain ends on (the model guide carries the hops in bits 31..28); after frame_moving, render these after it"""
        if follow:
            prm = GuideParams(follow)
            self._chk(self.L.pt_render_guides_followed(self.ctx, sample, C.byref(prm)))
        else:
            self._chk(self.L.pt_render_guides(self.ctx, sample))

    def read_guide_hops(self):
        """the hop guide of the last render_guides: how many mirror / glass surfaces every pixel's chain followed (zeros unless follow)"""
        hops = np.zeros((len(self.local_rows()), self.cfg.width), np.uint8)
        self._chk(self.L.pt_read_guide_hops(self.ctx, _p(hops)))
        return hops

    def read_guides(self):
        """(position xyzt, normal xyz, model u32; MISS = 0xffffffff) of the last render_guides, local rows x width"""
        rows, w = len(self.local_rows()), self.cfg.width
        pos = np.zeros((rows, w, 4), np.float32); nrm = np.zeros((rows, w, 3), np.float32); model = np.zeros((rows, w), np.uint32)
        self._chk(self.L.pt_read_guides(self.ctx, _p(pos), _p(nrm), _p(model)))
        return pos, nrm, model

    def read_guide_instances(self):
        """the instance guide of the last render_guides: world-TLAS leaf (tlas_instances(0) index) of every pixel's hit, MISS = 0xffffffff"""
        inst = np.zeros((len(self.local_rows()), self.cfg.width), np.uint32)
        self._chk(self.L.pt_read_guide_instances(self.ctx, _p(inst)))
        return inst

    def read_guide_albedo(self):
        """the albedo guide of the last render_guides: surface colour at the first hit (emitted colour of a light, 0 for a miss), rows x width x 3"""
        al = np.zeros((len(self.local_rows()), self.cfg.width, 3), np.float32)
        self._chk(self.L.pt_read_guide_albedo(self.ctx, _p(al)))
        return al

    def denoise(self, iterations=0, sigma_luminance=0.0, sigma_normal=0, sigma_plane=0.0, download=True):
        """filter the accumulation with the guides (and the moments where the context keeps valid ones); returns rgba (c, 1) per local pixel,
        or None with download=False (the result stays on the device for write_denoised_image)"""
        prm = DenoiseParams(iterations, sigma_luminance, sigma_normal, sigma_plane)
        out = np.zeros((len(self.local_rows()), self.cfg.width, 4), np.float32) if download else None
        self._chk(self.L.pt_denoise(self.ctx, C.byref(prm), _p(out)))
        return out

    def write_denoised_image(self, path):
        self._chk(self.L.pt_write_denoised_image(self.ctx, str(path).encode()))

    def post_denoise(self, accum, position, normal, model, sumsq=None, iterations=0, sigma_luminance=0.0, sigma_normal=0, sigma_plane=0.0):
        """the filter's kernels on caller images (h x w x 4 accumulation and position, h x w x 3 normal, h x w model; sumsq None = spatial variance)"""
        accum = np.ascontiguousarray(accum, np.float32)
        h, w = accum.shape[:2]
        position = np.ascontiguousarray(position, np.float32); normal = np.ascontiguousarray(normal, np.float32)
        model = np.ascontiguousarray(model, np.uint32)
        q = None if sumsq is None else np.ascontiguousarray(sumsq, np.float32)
        if position.size != h * w * 4 or normal.size != h * w * 3 or model.size != h * w or (q is not None and q.size != h * w):
            raise PtError(-1, f"post_denoise: guides are not those of a {w}x{h} image")
        out = np.zeros((h, w, 4), np.float32)
        prm = DenoiseParams(iterations, sigma_luminance, sigma_normal, sigma_plane)
        self._chk(self.L.pt_post_denoise(self.ctx, w, h, C.byref(prm), _p(accum), _p(position), _p(normal), _p(model), _p(q), _p(out)))
        return out

    # ---- the temporal stage: reprojected history, history length and luminance moments (pt_frame_temporal)
    def frame_temporal(self, frame_index, last_inv_projection=None, ident=None, download=True, alpha=0.0, alpha_moments=0.0, normal_min=0.0,
                       plane_max=0.0, feedback=0, iterations=0, sigma_luminance=0.0, sigma_normal=0, sigma_plane=0.0, rescue=0, length_rule=0, demodulate=0):
        """frame_moving's render, guides and velocity, then the temporal stage instead of State::update: the history is reprojected through
        geometry tests, blended by its length, and the a-trous levels run on it with the variance the pixels observed over time.  rescue=1: a
        pixel that lost every tap searches the 3 x 3 around its reprojected position; length_rule=1 (TEMPORAL_LENGTH_MEAN): the taps' mean
        history length, not their least; demodulate=1: the stage works on the sample divided by its albedo guide (any of the three set: the
        call goes through pt_frame_temporal_options, otherwise through pt_frame_temporal).  Returns
        data, position, id, result (download=False: None; the result stays on the device for write_denoised_image)"""
        m = None if last_inv_projection is None else np.ascontiguousarray(last_inv_projection, np.float32)
        tp = TemporalParams(alpha, alpha_moments, normal_min, plane_max, feedback)
        dp = DenoiseParams(iterations, sigma_luminance, sigma_normal, sigma_plane)
        if rescue or length_rule or demodulate:
            to = TemporalOptions(rescue, length_rule, demodulate)
            call = lambda *bufs: self.L.pt_frame_temporal_options(self.ctx, frame_index, _p(m), C.byref(tp), C.byref(to), C.byref(dp), *bufs)
        else:
            call = lambda *bufs: self.L.pt_frame_temporal(self.ctx, frame_index, _p(m), C.byref(tp), C.byref(dp), *bufs)
        if not download:
            self._chk(call(None, None, None, None))
            return None
        h, w = self.cfg.height, self.cfg.width
        data = np.zeros((h, w, 4), np.float32); pos = np.zeros((h, w, 4), np.float32); out = np.zeros((h, w, 4), np.float32)
        idb = np.zeros((h, w), np.uint32) if ident is None else ident
        self._chk(call(_p(data), _p(pos), _p(idb), _p(out)))
        return data, pos, idb, out

    def read_temporal(self):
        """the temporal stage's state after the last frame_temporal: history (rgb | N), moments (mu1, mu2), the variance handed to the levels"""
        h, w = self.cfg.height, self.cfg.width
        cn = np.zeros((h, w, 4), np.float32); mom = np.zeros((h, w, 2), np.float32); var = np.zeros((h, w), np.float32)
        self._chk(self.L.pt_read_temporal(self.ctx, _p(cn), _p(mom), _p(var)))
        return cn, mom, var

    def reset_temporal(self):
        self._chk(self.L.pt_reset_temporal(self.ctx))

    def post_temporal(self, prev, cur, xprev=None, nprev=None, velocity=None, on_device=False, alpha=0.0, alpha_moments=0.0, normal_min=0.0,
                      plane_max=0.0, sigma_normal=0, sigma_plane=0.0, rescue=0, length_rule=0, demodulate=0):
        """one temporal step (without the levels) on caller images.  prev = (history h x w x 4, moments h x w x 2, position h x w x 4, normal
        h x w x 3, model h x w) of the previous call, cur = (input h x w x 4, position, normal, model) of this frame; xprev / nprev None: the
        position / the normal; velocity None: at rest.  on_device False evaluates on the host and touches no GPU.  rescue and length_rule as
        frame_temporal's; the library refuses demodulate here (divide the input image yourself).  Returns history, moments, variance"""
        ph, pm, px, pn, pmod = (np.ascontiguousarray(a, t) for a, t in zip(prev, (np.float32,) * 4 + (np.uint32,)))
        ci, cx, cn, cmod = (np.ascontiguousarray(a, t) for a, t in zip(cur, (np.float32,) * 3 + (np.uint32,)))
        h, w = ci.shape[:2]
        opt = [None if a is None else np.ascontiguousarray(a, np.float32) for a in (xprev, nprev, velocity)]
        sizes = [(ph, 4), (pm, 2), (px, 4), (pn, 3), (pmod, 1), (ci, 4), (cx, 4), (cn, 3), (cmod, 1), (opt[0], 4), (opt[1], 3), (opt[2], 2)]
        if any(a is not None and a.size != h * w * k for a, k in sizes):
            raise PtError(-1, f"post_temporal: images are not those of a {w}x{h} frame")
        out_h = np.zeros((h, w, 4), np.float32); out_m = np.zeros((h, w, 2), np.float32); out_v = np.zeros((h, w), np.float32)
        tp = TemporalParams(alpha, alpha_moments, normal_min, plane_max, 0)
        dp = DenoiseParams(0, 0.0, sigma_normal, sigma_plane)
        images = [_p(a) for a in (ph, pm, px, pn, pmod, ci, cx, cn, cmod, opt[0], opt[1], opt[2], out_h, out_m, out_v)]
        if rescue or length_rule or demodulate:
            to = TemporalOptions(rescue, length_rule, demodulate)
            self._chk(self.L.pt_post_temporal_options(self.ctx, int(bool(on_device)), w, h, C.byref(tp), C.byref(to), C.byref(dp), *images))
        else:
            self._chk(self.L.pt_post_temporal(self.ctx, int(bool(on_device)), w, h, C.byref(tp), C.byref(dp), *images))
        return out_h, out_m, out_v

    # ---- mean albedo and the demodulated filter (pt_denoise_albedo)
    def accumulate_albedo(self, first_sample: int, n_samples: int, follow: int = 0):
        """add the albedo guide of samples [first_sample, first_sample + n_samples) of every local pixel to the mean-albedo sums, in sample
        order; a miss adds (1, 1, 1).  Calls continue the sums until they go stale (whatever makes the guides stale) or reset_albedo.
        follow = K > 0 (pt_accumulate_albedo_followed): the albedo product of render_guides(.., follow=K); sums made with another K restart"""
        if follow:
            prm = GuideParams(follow)
            self._chk(self.L.pt_accumulate_albedo_followed(self.ctx, first_sample, n_samples, C.byref(prm)))
        else:
            self._chk(self.L.pt_accumulate_albedo(self.ctx, first_sample, n_samples))

    def reset_albedo(self):
        self._chk(self.L.pt_reset_albedo(self.ctx))

    def read_albedo(self):
        """the mean-albedo sums (sum r, sum g, sum b, n), local rows x width x 4"""
        out = np.zeros((len(self.local_rows()), self.cfg.width, 4), np.float32)
        self._chk(self.L.pt_read_albedo(self.ctx, _p(out)))
        return out

    def denoise_albedo(self, source=ALBEDO_MEAN, iterations=0, sigma_luminance=0.0, sigma_normal=0, sigma_plane=0.0, download=True):
        """denoise() on the accumulation divided by the albedo (source: ALBEDO_GUIDE, the last render_guides' albedo guide, or ALBEDO_MEAN,
        the accumulate_albedo sums), the result multiplied by it again: texture detail survives the filter"""
        prm = DenoiseParams(iterations, sigma_luminance, sigma_normal, sigma_plane)
        out = np.zeros((len(self.local_rows()), self.cfg.width, 4), np.float32) if download else None
        self._chk(self.L.pt_denoise_albedo(self.ctx, C.byref(prm), source, _p(out)))
        return out

    def post_denoise_albedo(self, accum, position, normal, model, albedo, sumsq=None, iterations=0, sigma_luminance=0.0, sigma_normal=0,
                            sigma_plane=0.0):
        """the demodulated filter's kernels on caller images: post_denoise's, and an h x w x 3 albedo"""
        accum = np.ascontiguousarray(accum, np.float32)
        h, w = accum.shape[:2]
        position = np.ascontiguousarray(position, np.float32); normal = np.ascontiguousarray(normal, np.float32)
        model = np.ascontiguousarray(model, np.uint32); albedo = np.ascontiguousarray(albedo, np.float32)
        q = None if sumsq is None else np.ascontiguousarray(sumsq, np.float32)
        if (position.size != h * w * 4 or normal.size != h * w * 3 or model.size != h * w or albedo.size != h * w * 3
                or (q is not None and q.size != h * w)):
            raise PtError(-1, f"post_denoise_albedo: guides are not those of a {w}x{h} image")
        out = np.zeros((h, w, 4), np.float32)
        prm = DenoiseParams(iterations, sigma_luminance, sigma_normal, sigma_plane)
        self._chk(self.L.pt_post_denoise_albedo(self.ctx, w, h, C.byref(prm), _p(accum), _p(position), _p(normal), _p(model), _p(albedo), _p(q),
                                                _p(out)))
        return out

    # ---- caller-supplied rays and irradiance probes
    def integrate_rays(self, o, d, key, sample, draws_consumed=1, batch_rays=0):
        """The radiance arriving along caller-supplied rays (pt_integrate_rays): o, d (n, 3) float32 (d is used as given), key and sample (n,)
        uint32 naming each path's stream.  Returns (radiance (n, 4), first-hit position xyz|t (n, 4), id byte (n,)).  With torch tensors on the
        GPU for all four inputs the rays are read in place and the three results are GPU tensors (pt_integrate_rays_device)."""
        if type(o).__module__.startswith("torch"):
            return self._integrate_rays_device(o, d, key, sample, draws_consumed, batch_rays)
        o = np.ascontiguousarray(o, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
        key = np.ascontiguousarray(key, np.uint32).reshape(-1)
        sample = np.ascontiguousarray(sample, np.uint32).reshape(-1)
        n = o.shape[0]
        if d.shape[0] != n or key.size != n or sample.size != n:
            raise PtError(-1, "integrate_rays: o, d, key and sample do not describe the same number of rays")
        rad = np.zeros((n, 4), np.float32); pos = np.zeros((n, 4), np.float32); idb = np.zeros(n, np.uint8)
        prm = RaysParams(draws_consumed, batch_rays)
        self._chk(self.L.pt_integrate_rays(self.ctx, n, _p(o), _p(d), _p(key), _p(sample), C.byref(prm), _p(rad), _p(pos), _p(idb)))
        return rad, pos, idb

    def _integrate_rays_device(self, o, d, key, sample, draws_consumed, batch_rays):
        import torch
        n = o.shape[0]
        ts = (o, d, key, sample)
        if not all(t.is_cuda and t.is_contiguous() for t in ts) or o.dtype != torch.float32 or d.dtype != torch.float32 or \
                key.dtype not in (torch.int32, torch.uint32) or sample.dtype not in (torch.int32, torch.uint32):
            raise PtError(-1, "integrate_rays: device rays are contiguous GPU tensors, o and d float32, key and sample 32-bit integers")
        if o.numel() != 3 * n or d.numel() != 3 * n or key.numel() != n or sample.numel() != n:
            raise PtError(-1, "integrate_rays: o, d, key and sample do not describe the same number of rays")
        rad = torch.zeros((n, 4), dtype=torch.float32, device=o.device); pos = torch.zeros((n, 4), dtype=torch.float32, device=o.device)
        idb = torch.zeros(n, dtype=torch.uint8, device=o.device)
        torch.cuda.synchronize(o.device)  # the library launches on its own stream
        prm = RaysParams(draws_consumed, batch_rays)
        ptr = lambda t: C.c_void_p(t.data_ptr())
        self._chk(self.L.pt_integrate_rays_device(self.ctx, n, ptr(o), ptr(d), ptr(key), ptr(sample), C.byref(prm), ptr(rad), ptr(pos), ptr(idb)))
        return rad, pos, idb

    def bake_probes(self, positions, n_samples, first_sample=0, key_base=0, sh=None):
        """Irradiance probes (pt_bake_probes): adds samples [first_sample, first_sample + n_samples) of every probe at positions (n, 3) to the raw
        spherical-harmonics sums sh (n, 9, 3) float32 (None: a fresh bake from zero) and returns them.  The factor 4 pi / samples and the
        cosine-lobe convolution are the caller's."""
        pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
        n = pos.shape[0]
        out = np.zeros((n, 9, 3), np.float32) if sh is None else np.ascontiguousarray(sh, np.float32)
        if out.size != n * 27:
            raise PtError(-1, "bake_probes: sh does not hold 27 values per probe")
        prm = ProbeParams(first_sample, n_samples, key_base, 0)
        self._chk(self.L.pt_bake_probes(self.ctx, n, _p(pos), C.byref(prm), _p(out)))
        return out.reshape(n, 9, 3)

    def probe_ray(self, key: int, sample: int):
        """(direction, y0..y8) of sample `sample` of the probe whose stream is pixel `key`, as bake_probes makes them; host evaluation"""
        d = np.zeros(3, np.float32); y = np.zeros(9, np.float32)
        self._chk(self.L.pt_probe_ray(self.ctx, key, sample, _p(d), _p(y)))
        return d, y

    # ---- lightmaps
    def bake_lightmap(self, model, instance, w, h, n_samples, first_sample=0, key_base=0, bias=0.0, sums=None):
        """A lightmap of one placement of a model over its UV layout (pt_bake_lightmap): adds samples [first_sample, first_sample + n_samples) of
        every covered texel to the raw sums (h, w, 3) float32 (None: a fresh bake from zero) and returns (sums, coverage (h, w) uint8).  With
        cosine-distributed directions the irradiance is pi * sums / samples; that factor is the caller's."""
        out = np.zeros((h, w, 3), np.float32) if sums is None else np.ascontiguousarray(sums, np.float32)
        if out.size != w * h * 3:
            raise PtError(-1, "bake_lightmap: sums does not hold 3 values per texel")
        cov = np.zeros((h, w), np.uint8)
        prm = LightmapParams(model, instance, w, h, first_sample, n_samples, key_base, bias)
        self._chk(self.L.pt_bake_lightmap(self.ctx, C.byref(prm), _p(out), _p(cov)))
        return out.reshape(h, w, 3), cov

    def lightmap_texels(self, model, instance, w, h, on_device=False):
        """unit hook: the texel table of a map, (prim (h, w) uint32 with 0xffffffff for an uncovered texel, uv (h, w, 2), position (h, w, 3),
        normal (h, w, 3)); on the host (no GPU) unless on_device"""
        prim = np.zeros((h, w), np.uint32); uv = np.zeros((h, w, 2), np.float32)
        pos = np.zeros((h, w, 3), np.float32); nrm = np.zeros((h, w, 3), np.float32)
        self._chk(self.L.pt_lightmap_texels(self.ctx, model, instance, w, h, int(bool(on_device)), _p(prim), _p(uv), _p(pos), _p(nrm)))
        return prim, uv, pos, nrm

    def lightmap_ray(self, key: int, sample: int, normal):
        """direction of sample `sample` of the texel whose stream is pixel `key` over `normal`, as bake_lightmap makes it; host evaluation"""
        n = np.ascontiguousarray(normal, np.float32).reshape(3)
        d = np.zeros(3, np.float32)
        self._chk(self.L.pt_lightmap_ray(self.ctx, key, sample, _p(n), _p(d)))
        return d

    def dilate_lightmap(self, rgb, coverage, passes=1):
        """`passes` dilation passes (pt_lightmap_dilate) of a map (h, w, 3) float32 with coverage bytes (h, w); returns new (rgb, coverage),
        filled texels carrying the byte 2"""
        a = np.array(rgb, np.float32, order="C"); cv = np.array(coverage, np.uint8, order="C")
        if a.ndim != 3 or a.shape[2] != 3 or cv.shape != a.shape[:2]:
            raise PtError(-1, "dilate_lightmap: rgb is (h, w, 3) and coverage (h, w)")
        self._chk(self.L.pt_lightmap_dilate(self.ctx, a.shape[1], a.shape[0], passes, _p(a), _p(cv)))
        return a, cv

    def bake_lightmap_moments(self, model, instance, w, h, n_samples, first_sample=0, key_base=0, bias=0.0, sums=None, sumsq=None):
        """bake_lightmap that also folds the second moment of every sample's luminance (pt_bake_lightmap_moments): returns (sums (h, w, 3),
        sumsq (h, w), coverage (h, w) uint8); sums and sumsq continue from what is passed in (None: zero)"""
        out = np.zeros((h, w, 3), np.float32) if sums is None else np.ascontiguousarray(sums, np.float32)
        sq = np.zeros((h, w), np.float32) if sumsq is None else np.ascontiguousarray(sumsq, np.float32)
        if out.size != w * h * 3 or sq.size != w * h:
            raise PtError(-1, "bake_lightmap_moments: sums holds 3 values per texel and sumsq one")
        cov = np.zeros((h, w), np.uint8)
        prm = LightmapParams(model, instance, w, h, first_sample, n_samples, key_base, bias)
        self._chk(self.L.pt_bake_lightmap_moments(self.ctx, C.byref(prm), _p(out), _p(sq), _p(cov)))
        return out.reshape(h, w, 3), sq.reshape(h, w), cov

    def denoise_lightmap(self, model, instance, sums, n_samples, sumsq=None, iterations=0, sigma_luminance=0.0, sigma_normal=0, sigma_plane=0.0, reach=0.0,
                         on_device=True, want_area=False, counts=None):
        """the texel-space filter (pt_lightmap_denoise) on a bake's raw sums (h, w, 3) over n_samples samples, with its second moments sumsq
        (h, w) or, None, the spatial variance: the texel means (h, w, 3), zeros where uncovered (dilate afterwards); with want_area
        (means, texel areas (h, w)).  0 selects each default; on the host (no GPU) unless on_device.  counts (h, w) uint32, an adaptive
        bake's samples per texel, routes to pt_lightmap_denoise_counts; n_samples must then be 0 (or None)"""
        a = np.ascontiguousarray(sums, np.float32)
        if a.ndim != 3 or a.shape[2] != 3:
            raise PtError(-1, "denoise_lightmap: sums is (h, w, 3)")
        h, w = a.shape[:2]
        sq = None if sumsq is None else np.ascontiguousarray(sumsq, np.float32)
        if sq is not None and sq.shape != (h, w):
            raise PtError(-1, "denoise_lightmap: sumsq is (h, w)")
        cn = None if counts is None else np.ascontiguousarray(counts, np.uint32)
        if cn is not None and cn.shape != (h, w):
            raise PtError(-1, "denoise_lightmap: counts is (h, w)")
        prm = LightmapDenoiseParams(model, instance, w, h, n_samples or 0, DenoiseParams(iterations, sigma_luminance, sigma_normal, sigma_plane), reach)
        out = np.zeros((h, w, 3), np.float32)
        area = np.zeros((h, w), np.float32) if want_area else None
        if cn is not None:
            self._chk(self.L.pt_lightmap_denoise_counts(self.ctx, int(bool(on_device)), C.byref(prm), _p(a), _p(sq), _p(cn), _p(out), _p(area)))
        else:
            self._chk(self.L.pt_lightmap_denoise(self.ctx, int(bool(on_device)), C.byref(prm), _p(a), _p(sq), _p(out), _p(area)))
        return (out, area) if want_area else out

    # ---- adaptive bakes
    @staticmethod
    def _lightmap_state(what, w, h, sums, sumsq, counts, copy):
        """the three arrays of an adaptive bake as C-contiguous (h, w, 3) float32, (h, w) float32, (h, w) uint32; None: zeros"""
        def one(a, shape, dt):
            if a is None:
                return np.zeros(shape, dt)
            a = np.array(a, dt, order="C") if copy else np.ascontiguousarray(a, dt)
            if a.shape != shape:
                raise PtError(-1, f"{what}: sums is (h, w, 3) float32, sumsq (h, w) float32 and counts (h, w) uint32 for a {w} x {h} map")
            return a
        return one(sums, (h, w, 3), np.float32), one(sumsq, (h, w), np.float32), one(counts, (h, w), np.uint32)

    def bake_lightmap_adaptive(self, model, instance, w, h, n_samples, rel_error, abs_floor=0.0, min_samples=2, max_samples=0, key_base=0, bias=0.0,
                               sums=None, sumsq=None, counts=None):
        """One round of an adaptive bake (pt_bake_lightmap_adaptive): selects the covered texels whose mean luminance is not yet known to
        rel_error (pt_adaptive's rule on sums, sumsq and counts as they come in) and gives each of them n_samples more samples, continuing from
        its own count.  Returns (sums (h, w, 3), sumsq (h, w), counts (h, w) uint32, coverage (h, w) uint8, n_active): new arrays, the ones
        passed in are not written (None: a fresh bake from zeros, where every covered texel is active).  Every texel's sums are bit for bit
        bake_lightmap_moments(0, counts[texel]) at that texel.  Call until n_active == 0."""
        out, sq, cn = self._lightmap_state("bake_lightmap_adaptive", w, h, sums, sumsq, counts, copy=True)
        cov = np.zeros((h, w), np.uint8)
        n = C.c_uint32(0)
        prm = LightmapParams(model, instance, w, h, 0, n_samples, key_base, bias)
        crit = self._adaptive(rel_error, abs_floor, min_samples, max_samples)
        self._chk(self.L.pt_bake_lightmap_adaptive(self.ctx, C.byref(prm), C.byref(crit), _p(out), _p(sq), _p(cn), _p(cov), C.byref(n)))
        return out, sq, cn, cov, n.value

    def lightmap_adaptive_mask(self, model, instance, sums, sumsq, counts, rel_error, abs_floor=0.0, min_samples=2, max_samples=0, on_device=False):
        """unit hook: the selection of bake_lightmap_adaptive alone, bool (h, w), True = the texel would get samples; on the host (no GPU)
        unless on_device, which runs the bake's selection kernels and builds the mask from their list"""
        a = np.ascontiguousarray(sums, np.float32)
        if a.ndim != 3 or a.shape[2] != 3:
            raise PtError(-1, "lightmap_adaptive_mask: sums is (h, w, 3)")
        h, w = a.shape[:2]
        a, sq, cn = self._lightmap_state("lightmap_adaptive_mask", w, h, a, sumsq, counts, copy=False)
        if sumsq is None or counts is None:
            raise PtError(-1, "lightmap_adaptive_mask: sumsq and counts are needed")
        mask = np.zeros((h, w), np.uint8)
        n = C.c_uint32(0)
        crit = self._adaptive(rel_error, abs_floor, min_samples, max_samples)
        self._chk(self.L.pt_lightmap_adaptive_mask(self.ctx, int(bool(on_device)), model, instance, w, h, C.byref(crit), _p(a), _p(sq), _p(cn), _p(mask), C.byref(n)))
        assert int(mask.sum()) == n.value
        return mask.astype(bool)

    # ---- direct light sampled at the texel
    def bake_lightmap_direct(self, model, instance, w, h, n_samples, first_sample=0, key_base=0, bias=0.0, sums=None, sumsq=None, light_key_base=None,
                             moments=False):
        """bake_lightmap whose sample is X = G + D (pt_bake_lightmap_direct): the gather radiance, zero when the gather ray's first hit is a
        lamp, plus one light sample taken at the texel with a shadow ray.  light_key_base (None: key_base + w * h) keys the light samples'
        streams.  Returns (sums (h, w, 3), coverage (h, w) uint8) as bake_lightmap does; with sumsq given (or moments=True, from zero) the
        second moments are folded too and (sums, sumsq (h, w), coverage) come back, as bake_lightmap_moments"""
        out = np.zeros((h, w, 3), np.float32) if sums is None else np.ascontiguousarray(sums, np.float32)
        with_sq = moments or sumsq is not None
        sq = None if not with_sq else np.zeros((h, w), np.float32) if sumsq is None else np.ascontiguousarray(sumsq, np.float32)
        if out.size != w * h * 3 or (sq is not None and sq.size != w * h):
            raise PtError(-1, "bake_lightmap_direct: sums holds 3 values per texel and sumsq one")
        cov = np.zeros((h, w), np.uint8)
        prm = LightmapParams(model, instance, w, h, first_sample, n_samples, key_base, bias)
        dp = LightmapDirect(key_base + w * h if light_key_base is None else light_key_base)
        self._chk(self.L.pt_bake_lightmap_direct(self.ctx, C.byref(prm), C.byref(dp), _p(out), _p(sq), _p(cov)))
        return (out.reshape(h, w, 3), sq.reshape(h, w), cov) if with_sq else (out.reshape(h, w, 3), cov)

    def bake_lightmap_adaptive_direct(self, model, instance, w, h, n_samples, rel_error, abs_floor=0.0, min_samples=2, max_samples=0, key_base=0, bias=0.0,
                                      sums=None, sumsq=None, counts=None, light_key_base=None):
        """One round of bake_lightmap_adaptive over bake_lightmap_direct's samples (pt_bake_lightmap_adaptive_direct); arguments and the five
        return values as bake_lightmap_adaptive, light_key_base as bake_lightmap_direct"""
        out, sq, cn = self._lightmap_state("bake_lightmap_adaptive_direct", w, h, sums, sumsq, counts, copy=True)
        cov = np.zeros((h, w), np.uint8)
        n = C.c_uint32(0)
        prm = LightmapParams(model, instance, w, h, 0, n_samples, key_base, bias)
        dp = LightmapDirect(key_base + w * h if light_key_base is None else light_key_base)
        crit = self._adaptive(rel_error, abs_floor, min_samples, max_samples)
        self._chk(self.L.pt_bake_lightmap_adaptive_direct(self.ctx, C.byref(prm), C.byref(dp), C.byref(crit), _p(out), _p(sq), _p(cn), _p(cov), C.byref(n)))
        return out, sq, cn, cov, n.value

    def lightmap_light_sample(self, key, sample, origin, normal, on_device=False):
        """unit hook: the light sample bake_lightmap_direct takes for (key = light_key_base + texel, sample) at `origin` under `normal`
        (pt_lightmap_light_sample): (light (n,) uint32, dir (n, 3), t_max (n,), ce (n, 3) before the shadow ray); on the host (no GPU)
        unless on_device"""
        key = np.ascontiguousarray(key, np.uint32).reshape(-1); smp = np.ascontiguousarray(sample, np.uint32).reshape(-1)
        n = key.size
        o = np.ascontiguousarray(origin, np.float32).reshape(n, 3); nr = np.ascontiguousarray(normal, np.float32).reshape(n, 3)
        if smp.size != n:
            raise PtError(-1, "lightmap_light_sample: key and sample have one entry per sample")
        light = np.zeros(n, np.uint32); d = np.zeros((n, 3), np.float32); t = np.zeros(n, np.float32); ce = np.zeros((n, 3), np.float32)
        self._chk(self.L.pt_lightmap_light_sample(self.ctx, int(bool(on_device)), n, _p(key), _p(smp), _p(o), _p(nr), _p(light), _p(d), _p(t), _p(ce)))
        return light, d, t, ce

    # ---- lightmaps kept by the context, and the baked view
    def set_lightmap(self, model, instance, rgb):
        """the finished map of placement (model, instance) (pt_set_lightmap): rgb (h, w, 3), every texel the MEAN of the bake's radiance
        samples (sums / n_samples after dilation); None clears the map"""
        if rgb is None:
            self._chk(self.L.pt_set_lightmap(self.ctx, model, instance, 0, 0, None))
            return
        a = np.ascontiguousarray(rgb, np.float32)
        if a.ndim != 3 or a.shape[2] != 3:
            raise PtError(-1, "set_lightmap: rgb is (h, w, 3)")
        self._chk(self.L.pt_set_lightmap(self.ctx, model, instance, a.shape[1], a.shape[0], _p(a)))

    def set_lightmap_sums(self, model, instance, sums, n_samples):
        """set_lightmap of a bake's raw sums (bake_lightmap, dilate_lightmap) over n_samples samples: the division is done here"""
        if not n_samples > 0:
            raise PtError(-1, "set_lightmap_sums: n_samples must be positive")
        self.set_lightmap(model, instance, np.asarray(sums, np.float32) / np.float32(n_samples))

    def set_lightmap_counts(self, model, instance, sums, counts, coverage, passes=0):
        """set_lightmap of an adaptive bake: sums (h, w, 3), counts (h, w), coverage (h, w) as bake_lightmap_adaptive returns them.  Every
        texel is divided by ITS OWN count FIRST (zero where the count is 0), THEN the means are dilated `passes` times, then set.  The order
        matters: with per-texel counts a dilated raw sum is a mix of neighbours with different denominators, and there is no count left to
        divide it by; a mean of means is what dilation is meant to produce.  Returns the (means, coverage) that were set."""
        a = np.ascontiguousarray(sums, np.float32)
        cn = np.ascontiguousarray(counts, np.uint32)
        cv = np.ascontiguousarray(coverage, np.uint8)
        if a.ndim != 3 or a.shape[2] != 3 or cn.shape != a.shape[:2] or cv.shape != a.shape[:2]:
            raise PtError(-1, "set_lightmap_counts: sums is (h, w, 3), counts and coverage (h, w)")
        mean = np.zeros_like(a)
        have = cn > 0
        mean[have] = a[have] / cn[have].astype(np.float32)[:, None]
        if passes:
            mean, cv = self.dilate_lightmap(mean, cv, passes)
        self.set_lightmap(model, instance, mean)
        return mean, cv

    def lightmap_info(self, model, instance):
        """(w, h) of the map of placement (model, instance); (0, 0): none"""
        w = C.c_uint32(); h = C.c_uint32()
        self._chk(self.L.pt_get_lightmap_info(self.ctx, model, instance, C.byref(w), C.byref(h)))
        return w.value, h.value

    def lightmap_lookup(self, instance, prim, u, v, on_device=False):
        """unit hook: (rgb [n, 3], mapped [n] uint8) of the lightmap at hits (world-TLAS instance, load-order primitive, barycentrics) of the
        built scene, zeros where the leaf has no map; on the host (no GPU) unless on_device"""
        i = np.ascontiguousarray(instance, dtype=np.uint32); p = np.ascontiguousarray(prim, dtype=np.uint32)
        uu = np.ascontiguousarray(u, dtype=np.float32); vv = np.ascontiguousarray(v, dtype=np.float32)
        assert i.shape == p.shape == uu.shape == vv.shape and i.ndim == 1
        out = np.zeros((i.shape[0], 3), np.float32); mapped = np.zeros(i.shape[0], np.uint8)
        self._chk(self.L.pt_lightmap_lookup(self.ctx, int(bool(on_device)), i.shape[0], _p(i), _p(p), _p(uu), _p(vv), _p(out), _p(mapped)))
        return out, mapped

    # ---- directional lightmaps: a direction baked beside the irradiance, for normal-mapped surfaces in the baked view
    def bake_lightmap_directional(self, model, instance, w, h, n_samples, first_sample=0, key_base=0, bias=0.0, sums=None, dir_sums=None):
        """bake_lightmap that also folds every sample's radiance times its direction (pt_bake_lightmap_directional): returns (sums (h, w, 3),
        dir_sums (h, w, 3, 3) as [axis][channel], coverage (h, w) uint8); both sums continue from what is passed in (None: zero)"""
        out = np.zeros((h, w, 3), np.float32) if sums is None else np.ascontiguousarray(sums, np.float32)
        dirs = np.zeros((h, w, 3, 3), np.float32) if dir_sums is None else np.ascontiguousarray(dir_sums, np.float32)
        if out.size != w * h * 3 or dirs.size != w * h * 9:
            raise PtError(-1, "bake_lightmap_directional: sums holds 3 values per texel and dir_sums 9")
        cov = np.zeros((h, w), np.uint8)
        prm = LightmapParams(model, instance, w, h, first_sample, n_samples, key_base, bias)
        self._chk(self.L.pt_bake_lightmap_directional(self.ctx, C.byref(prm), _p(out), _p(dirs), _p(cov)))
        return out.reshape(h, w, 3), dirs.reshape(h, w, 3, 3), cov

    def lightmap_gradient(self, model, instance, dir_sums, n_samples, on_device=False):
        """the tangential gradient (pt_lightmap_gradient) of a directional bake's raw first moments (h, w, 3, 3) over n_samples samples:
        (h, w, 3, 3) as [axis][channel], zeros where uncovered; on the host (no GPU) unless on_device"""
        a = np.ascontiguousarray(dir_sums, np.float32)
        if a.ndim != 4 or a.shape[2:] != (3, 3):
            raise PtError(-1, "lightmap_gradient: dir_sums is (h, w, 3, 3)")
        out = np.zeros_like(a)
        self._chk(self.L.pt_lightmap_gradient(self.ctx, int(bool(on_device)), model, instance, a.shape[1], a.shape[0], n_samples, _p(a), _p(out)))
        return out

    def dilate_lightmap_directional(self, grad, coverage, passes=1):
        """dilate_lightmap on the three axis planes of a gradient (h, w, 3, 3), each with a fresh copy of the coverage; returns (grad, coverage)"""
        g = np.array(grad, np.float32, order="C")
        if g.ndim != 4 or g.shape[2:] != (3, 3):
            raise PtError(-1, "dilate_lightmap_directional: grad is (h, w, 3, 3)")
        cov = np.asarray(coverage, np.uint8)
        for a in range(3):
            g[:, :, a, :], cov_out = self.dilate_lightmap(g[:, :, a, :], cov, passes)
        return g, cov_out

    def set_lightmap_directional(self, model, instance, grad):
        """the gradient of placement (model, instance) (pt_set_lightmap_directional): grad (h, w, 3, 3) of the size of the placement's map; None
        clears it"""
        if grad is None:
            self._chk(self.L.pt_set_lightmap_directional(self.ctx, model, instance, 0, 0, None))
            return
        a = np.ascontiguousarray(grad, np.float32)
        if a.ndim != 4 or a.shape[2:] != (3, 3):
            raise PtError(-1, "set_lightmap_directional: grad is (h, w, 3, 3)")
        self._chk(self.L.pt_set_lightmap_directional(self.ctx, model, instance, a.shape[1], a.shape[0], _p(a)))

    def lightmap_directional_info(self, model, instance):
        """whether placement (model, instance) has a gradient"""
        has = C.c_uint32()
        self._chk(self.L.pt_get_lightmap_directional_info(self.ctx, model, instance, C.byref(has)))
        return bool(has.value)

    def lightmap_lookup_directional(self, instance, prim, u, v, direction, on_device=False):
        """unit hook: lightmap_lookup under the perturbed normal of hits made by rays of world direction `direction` [n, 3]"""
        i = np.ascontiguousarray(instance, dtype=np.uint32); p = np.ascontiguousarray(prim, dtype=np.uint32)
        uu = np.ascontiguousarray(u, dtype=np.float32); vv = np.ascontiguousarray(v, dtype=np.float32)
        d = np.ascontiguousarray(direction, dtype=np.float32)
        assert i.shape == p.shape == uu.shape == vv.shape and i.ndim == 1 and d.shape == (i.shape[0], 3)
        out = np.zeros((i.shape[0], 3), np.float32); mapped = np.zeros(i.shape[0], np.uint8)
        self._chk(self.L.pt_lightmap_lookup_directional(self.ctx, int(bool(on_device)), i.shape[0], _p(i), _p(p), _p(uu), _p(vv), _p(d), _p(out), _p(mapped)))
        return out, mapped

    def render_baked(self, first_sample: int, n_samples: int, follow: int = 0, unlit=(0.0, 0.0, 0.0), download=True):
        """the baked view (pt_render_baked): adds samples [first_sample, first_sample + n_samples) of every local pixel to the baked sums:
        the chain of render_guides(.., follow=K), its final surface's colour times the lightmap at the hit (`unlit` where the surface has no
        usable map).  Returns the sums (sum r, sum g, sum b, n), local rows x width x 4"""
        prm = BakedParams(follow, (C.c_float * 3)(*[float(x) for x in unlit]))
        out = np.zeros((len(self.local_rows()), self.cfg.width, 4), np.float32) if download else None
        self._chk(self.L.pt_render_baked(self.ctx, first_sample, n_samples, C.byref(prm), _p(out) if download else None))
        return out

    # ---- baked rays and the final-gather bake
    @staticmethod
    def _baked_params(follow, unlit):
        return BakedParams(follow, (C.c_float * 3)(*[float(x) for x in unlit]))

    def baked_rays(self, o, d, follow: int = 0, unlit=(0.0, 0.0, 0.0), window_rays: int = 0):
        """The baked view's chain for caller-supplied rays (pt_baked_rays): o, d (n, 3) float32 (d is used as given).  Returns (rgb (n, 3) the
        baked sample B of every ray, hops (n,) uint32 the hop its chain ended at, id (n,) uint8 the first hit's id byte as integrate_rays
        reports it).  With torch tensors on the GPU for o and d the rays are read in place and the results are GPU tensors: (rgbh (n, 4)
        float32 with the hop in .w, id) (pt_baked_rays_device)."""
        prm = BakedRaysParams(self._baked_params(follow, unlit), window_rays)
        if type(o).__module__.startswith("torch"):
            import torch
            n = o.shape[0]
            if not (o.is_cuda and d.is_cuda and o.is_contiguous() and d.is_contiguous()) or o.dtype != torch.float32 or d.dtype != torch.float32 or \
                    o.numel() != 3 * n or d.numel() != 3 * n:
                raise PtError(-1, "baked_rays: device rays are contiguous float32 GPU tensors of 3 values per ray")
            rgbh = torch.zeros((n, 4), dtype=torch.float32, device=o.device); idb = torch.zeros(n, dtype=torch.uint8, device=o.device)
            torch.cuda.synchronize(o.device)  # the library launches on its own stream
            ptr = lambda t: C.c_void_p(t.data_ptr())
            self._chk(self.L.pt_baked_rays_device(self.ctx, n, ptr(o), ptr(d), C.byref(prm), ptr(rgbh), ptr(idb)))
            return rgbh, idb
        o = np.ascontiguousarray(o, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
        n = o.shape[0]
        if d.shape[0] != n:
            raise PtError(-1, "baked_rays: o and d do not describe the same number of rays")
        rgbh = np.zeros((n, 4), np.float32); idb = np.zeros(n, np.uint8)
        self._chk(self.L.pt_baked_rays(self.ctx, n, _p(o), _p(d), C.byref(prm), _p(rgbh), _p(idb)))
        return np.ascontiguousarray(rgbh[:, :3]), rgbh[:, 3].astype(np.uint32), idb

    def _gather(self, w, h, key_base, follow, unlit, direct, light_key_base):
        lkb = 0 if not direct else key_base + w * h if light_key_base is None else light_key_base
        return LightmapGather(self._baked_params(follow, unlit), int(bool(direct)), lkb)

    def bake_lightmap_gather(self, model, instance, w, h, n_samples, first_sample=0, key_base=0, bias=0.0, sums=None, sumsq=None, follow=0,
                             unlit=(0.0, 0.0, 0.0), direct=True, light_key_base=None, moments=False):
        """The final-gather bake (pt_bake_lightmap_gather): bake_lightmap whose gather ray is one baked chain, baked_rays(.., follow, unlit) of
        the texel's ray, ended in the maps, grid and probes set on this renderer; with direct the texel's light sample is added and a gather
        ray whose first hit is a lamp counts zero, as bake_lightmap_direct (light_key_base likewise).  Sets nothing.  Returns (sums, coverage),
        or with sumsq given (or moments=True) (sums, sumsq, coverage)."""
        out = np.zeros((h, w, 3), np.float32) if sums is None else np.ascontiguousarray(sums, np.float32)
        with_sq = moments or sumsq is not None
        sq = None if not with_sq else np.zeros((h, w), np.float32) if sumsq is None else np.ascontiguousarray(sumsq, np.float32)
        if out.size != w * h * 3 or (sq is not None and sq.size != w * h):
            raise PtError(-1, "bake_lightmap_gather: sums holds 3 values per texel and sumsq one")
        cov = np.zeros((h, w), np.uint8)
        prm = LightmapParams(model, instance, w, h, first_sample, n_samples, key_base, bias)
        g = self._gather(w, h, key_base, follow, unlit, direct, light_key_base)
        self._chk(self.L.pt_bake_lightmap_gather(self.ctx, C.byref(prm), C.byref(g), _p(out), _p(sq), _p(cov)))
        return (out.reshape(h, w, 3), sq.reshape(h, w), cov) if with_sq else (out.reshape(h, w, 3), cov)

    def bake_lightmap_adaptive_gather(self, model, instance, w, h, n_samples, rel_error, abs_floor=0.0, min_samples=2, max_samples=0, key_base=0, bias=0.0,
                                      sums=None, sumsq=None, counts=None, follow=0, unlit=(0.0, 0.0, 0.0), direct=True, light_key_base=None):
        """One round of bake_lightmap_adaptive over bake_lightmap_gather's samples (pt_bake_lightmap_adaptive_gather); arguments and the five
        return values as bake_lightmap_adaptive, the gather's as bake_lightmap_gather"""
        out, sq, cn = self._lightmap_state("bake_lightmap_adaptive_gather", w, h, sums, sumsq, counts, copy=True)
        cov = np.zeros((h, w), np.uint8)
        n = C.c_uint32(0)
        prm = LightmapParams(model, instance, w, h, 0, n_samples, key_base, bias)
        g = self._gather(w, h, key_base, follow, unlit, direct, light_key_base)
        crit = self._adaptive(rel_error, abs_floor, min_samples, max_samples)
        self._chk(self.L.pt_bake_lightmap_adaptive_gather(self.ctx, C.byref(prm), C.byref(g), C.byref(crit), _p(out), _p(sq), _p(cn), _p(cov), C.byref(n)))
        return out, sq, cn, cov, n.value

    def bake_lightmaps_gather(self, placements, sizes, n_samples, iterations, key_bases=None, bias=0.0, follow=0, unlit=(0.0, 0.0, 0.0), direct=True,
                              dilate=1):
        """The Jacobi loop of the final gather over several placements: placements [(model, instance), ..], sizes [(w, h), ..], key_bases one
        per placement (None: disjoint ranges of 2 * w * h keys from 0 on, the second half the light samples').  Each of `iterations` passes
        bakes EVERY placement with bake_lightmap_gather from the maps currently set (pass 0: whatever is set), then divides by n_samples,
        dilates `dilate` times and sets all of them.  The same keys every pass.  Returns one list per pass of (sums, coverage) per placement."""
        if len(placements) != len(sizes):
            raise PtError(-1, "bake_lightmaps_gather: one size per placement")
        if key_bases is None:
            key_bases, k = [], 0
            for (w, h) in sizes:
                key_bases.append(k)
                k += 2 * w * h
        passes = []
        for _ in range(iterations):
            baked = [self.bake_lightmap_gather(m, i, w, h, n_samples, key_base=kb, bias=bias, follow=follow, unlit=unlit, direct=direct)
                     for (m, i), (w, h), kb in zip(placements, sizes, key_bases)]
            for (m, i), (sums, cov) in zip(placements, baked):
                mean = sums / np.float32(n_samples)
                self.set_lightmap(m, i, self.dilate_lightmap(mean, cov, dilate)[0] if dilate else mean)
            passes.append(baked)
        return passes

    def read_baked(self):
        """the baked sums (sum r, sum g, sum b, n), local rows x width x 4"""
        out = np.zeros((len(self.local_rows()), self.cfg.width, 4), np.float32)
        self._chk(self.L.pt_read_baked(self.ctx, _p(out)))
        return out

    def reset_baked(self):
        self._chk(self.L.pt_reset_baked(self.ctx))

    def write_baked_image(self, path):
        self._chk(self.L.pt_write_baked_image(self.ctx, str(path).encode()))

    # ---- the irradiance volume: a grid of SH9 probes that lights what no lightmap lights
    def set_probe_grid(self, origin, cell, sh, valid=None, normal_bias=0.0):
        """the probe grid (pt_set_probe_grid): node (ix, iy, iz) at origin + (ix, iy, iz) * cell; sh (nz, ny, nx, 9, 3) float32 the RADIANCE SH
        coefficients of every node (a bake's raw sums times 4 pi / n_samples: set_probe_grid_sums does that); valid (nz, ny, nx), None: all
        valid.  sh None clears the grid."""
        if sh is None:
            self._chk(self.L.pt_set_probe_grid(self.ctx, C.byref(ProbeGrid()), None, None))
            return
        a = np.ascontiguousarray(sh, np.float32)
        if a.ndim != 5 or a.shape[3:] != (9, 3):
            raise PtError(-1, "set_probe_grid: sh is (nz, ny, nx, 9, 3)")
        nz, ny, nx = a.shape[:3]
        v = None if valid is None else np.ascontiguousarray(np.asarray(valid) != 0, np.uint8)
        if v is not None and v.shape != (nz, ny, nx):
            raise PtError(-1, "set_probe_grid: valid is (nz, ny, nx)")
        g = ProbeGrid(_f3(origin), _f3(cell), (C.c_uint32 * 3)(nx, ny, nz), float(normal_bias))
        self._chk(self.L.pt_set_probe_grid(self.ctx, C.byref(g), _p(a), _p(v)))

    def set_probe_grid_sums(self, origin, cell, sums, n_samples, valid=None, normal_bias=0.0):
        """set_probe_grid of bake_probes' raw sums (nz, ny, nx, 9, 3) over n_samples samples: the factor 4 pi / n_samples is applied here"""
        if not n_samples > 0:
            raise PtError(-1, "set_probe_grid_sums: n_samples must be positive")
        scale = np.float32(4.0 * np.pi) / np.float32(n_samples)
        self.set_probe_grid(origin, cell, np.asarray(sums, np.float32) * scale, valid, normal_bias)

    def probe_grid_info(self):
        """(origin, cell, (nx, ny, nz), normal_bias, valid nodes) of the grid; counts of 0: none"""
        g = ProbeGrid(); n = C.c_uint32()
        self._chk(self.L.pt_get_probe_grid_info(self.ctx, C.byref(g), C.byref(n)))
        return np.array(g.origin, np.float32), np.array(g.cell, np.float32), tuple(g.count), float(g.normal_bias), n.value

    def probe_grid_lookup(self, position, normal, on_device=False):
        """unit hook: (rgb [n, 3], lit [n] uint8) of the grid's lookup at world positions and normals [n, 3]; on the host (no GPU) unless
        on_device"""
        p = np.ascontiguousarray(position, np.float32).reshape(-1, 3); nn = np.ascontiguousarray(normal, np.float32).reshape(-1, 3)
        assert p.shape == nn.shape
        out = np.zeros((p.shape[0], 3), np.float32); lit = np.zeros(p.shape[0], np.uint8)
        self._chk(self.L.pt_probe_grid_lookup(self.ctx, int(bool(on_device)), p.shape[0], _p(p), _p(nn), _p(out), _p(lit)))
        return out, lit

    def probe_backfaces(self, positions, n_samples, first_sample=0, key_base=0):
        """the census of probes inside geometry (pt_probe_backfaces): (hits [n], back [n]) uint32 over bake_probes' rays of samples
        [first_sample, first_sample + n_samples), each traced once: the rays that hit, and those that hit a back face"""
        pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
        n = pos.shape[0]
        hits = np.zeros(n, np.uint32); back = np.zeros(n, np.uint32)
        prm = ProbeParams(first_sample, n_samples, key_base, 0)
        self._chk(self.L.pt_probe_backfaces(self.ctx, n, _p(pos), C.byref(prm), _p(hits), _p(back)))
        return hits, back

    def probe_validity(self, positions, n_samples, max_back_fraction=0.25):
        """the usual policy over probe_backfaces: a probe is usable while at most max_back_fraction of its rays see a back face"""
        _, back = self.probe_backfaces(positions, n_samples)
        return back <= max_back_fraction * n_samples

    @staticmethod
    def probe_grid_positions(origin, cell, count):
        """the node positions (nz, ny, nx, 3) float32 of a grid: origin + index * cell, one binary32 product and sum per component"""
        nx, ny, nz = (int(k) for k in count)
        o = np.asarray(origin, np.float32); c = np.asarray(cell, np.float32)
        idx = np.stack(np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")[::-1], axis=-1).astype(np.float32)
        return (o + idx * c).astype(np.float32)

    def bake_probe_grid(self, origin, cell, count, n_samples, max_back_fraction=0.25, normal_bias=0.0, depth_res=0, max_distance=None, vis_floor=0.0,
                        facing=False, radiance_res=0, radiance_alphas=(0.1, 0.2, 0.4, 0.7, 1.0)):
        """bakes and sets a grid of count = (nx, ny, nz) probes: the node positions, bake_probes, probe_validity and set_probe_grid_sums.
        Returns (sums (nz, ny, nx, 9, 3), valid (nz, ny, nx)).  depth_res > 0 also bakes the nodes' depth moments from the same rays
        (bake_probe_depth) and sets them (set_probe_grid_depth_sums); max_distance None: the cell's diagonal times 1.5.  radiance_res > 0
        also bakes the nodes' radiance maps from the same rays (bake_probe_radiance), prefilters them at radiance_alphas on the device and sets
        them (set_probe_grid_radiance_sums)."""
        nx, ny, nz = (int(k) for k in count)
        pos = self.probe_grid_positions(origin, cell, count).reshape(-1, 3)
        sums = self.bake_probes(pos, n_samples).reshape(nz, ny, nx, 9, 3)
        valid = self.probe_validity(pos, n_samples, max_back_fraction).reshape(nz, ny, nx)
        self.set_probe_grid_sums(origin, cell, sums, n_samples, valid, normal_bias)
        if depth_res:
            if max_distance is None:
                max_distance = 1.5 * float(np.linalg.norm(np.asarray(cell, np.float64)))
            dsums, dcounts = self.bake_probe_depth(pos, n_samples, depth_res, max_distance)
            self.set_probe_grid_depth_sums(dsums, dcounts, max_distance, vis_floor, facing)
        if radiance_res:
            rsums, rcounts = self.bake_probe_radiance(pos, n_samples, radiance_res)
            self.set_probe_grid_radiance_sums(rsums, rcounts, radiance_alphas)
        return sums, valid

    # ---- probe visibility: depth moments on the nodes' octahedral maps
    def probe_depth_texel(self, directions, res):
        """the texel of every direction [n, 3] (any values, not normalised) in an octahedral map of side res (pt_probe_depth_texel; no GPU)"""
        d = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
        out = np.zeros(d.shape[0], np.uint32)
        self._chk(self.L.pt_probe_depth_texel(int(res), d.shape[0], _p(d), _p(out)))
        return out

    def bake_probe_depth(self, positions, n_samples, res, max_distance, first_sample=0, key_base=0, sums=None, counts=None):
        """depth moments (pt_bake_probe_depth): adds the distances seen by bake_probes' rays of samples [first_sample, first_sample + n_samples),
        clamped to max_distance, to the raw sums (n, res * res, 2) float32 and counts (n, res * res) uint32 per octahedral texel (None: zeros),
        in sample order per texel.  Returns (sums, counts)."""
        pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
        n, rr = pos.shape[0], int(res) * int(res)
        s = np.zeros((n, rr, 2), np.float32) if sums is None else np.ascontiguousarray(sums, np.float32).copy()
        k = np.zeros((n, rr), np.uint32) if counts is None else np.ascontiguousarray(counts, np.uint32).copy()
        if 2 <= int(res) <= 16 and (s.size != n * rr * 2 or k.size != n * rr):
            raise PtError(-1, "bake_probe_depth: sums hold res * res * 2 values and counts res * res per probe")
        prm = ProbeDepthParams(first_sample, n_samples, key_base, int(res), float(max_distance))
        self._chk(self.L.pt_bake_probe_depth(self.ctx, n, _p(pos), C.byref(prm), _p(s), _p(k)))
        return s, k

    def set_probe_grid_depth(self, moments, vis_floor=0.0, facing=False):
        """depth on the grid in force (pt_set_probe_grid_depth): moments (nodes, res * res, 2) float32, per texel the mean distance and the
        mean squared distance.  moments None clears depth."""
        if moments is None:
            self._chk(self.L.pt_set_probe_grid_depth(self.ctx, C.byref(ProbeDepth()), None))
            return
        m = np.ascontiguousarray(moments, np.float32)
        res = int(round(np.sqrt(m.shape[-2]))) if m.ndim >= 2 else 0
        nodes = int(np.prod(self.probe_grid_info()[2]))
        if m.ndim < 2 or m.shape[-1] != 2 or res * res != m.shape[-2] or m.size != nodes * res * res * 2:
            raise PtError(-1, "set_probe_grid_depth: moments is (nodes, res * res, 2)")
        v = ProbeDepth(res, PROBE_VIS_FACING if facing else 0, float(vis_floor))
        self._chk(self.L.pt_set_probe_grid_depth(self.ctx, C.byref(v), _p(m)))

    def set_probe_grid_depth_sums(self, sums, counts, max_distance, vis_floor=0.0, facing=False):
        """set_probe_grid_depth of bake_probe_depth's raw sums and counts: the means are taken here, one binary32 division each, and a texel
        without a sample gets (max_distance, max_distance * max_distance): nothing was seen nearer"""
        self.set_probe_grid_depth(self.probe_depth_means(sums, counts, max_distance), vis_floor, facing)

    @staticmethod
    def probe_depth_means(sums, counts, max_distance):
        """the moments (.., res * res, 2) float32 of raw depth sums and counts, as set_probe_grid_depth_sums sets them"""
        s = np.asarray(sums, np.float32); k = np.asarray(counts, np.uint32)
        far = np.float32(max_distance)
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = (s / k.astype(np.float32)[..., None]).astype(np.float32)
        return np.where((k > 0)[..., None], mean, np.array([far, far * far], np.float32)).astype(np.float32)

    def probe_grid_depth_info(self):
        """(res, flags, vis_floor) of the grid's depth; res 0: none"""
        v = ProbeDepth()
        self._chk(self.L.pt_get_probe_grid_depth_info(self.ctx, C.byref(v)))
        return int(v.res), int(v.flags), float(v.vis_floor)

    # ---- reflection probes: GGX-prefiltered radiance on the nodes' octahedral maps
    def probe_radiance_dir(self, res, texels=None):
        """(dir [n, 3], omega [n]) float32 of texel centres in an octahedral map of side res (pt_probe_radiance_dir; no GPU); texels None:
        every texel in order"""
        t = np.arange(int(res) * int(res), dtype=np.uint32) if texels is None else np.ascontiguousarray(texels, np.uint32).reshape(-1)
        d = np.zeros((t.shape[0], 3), np.float32); om = np.zeros(t.shape[0], np.float32)
        self._chk(self.L.pt_probe_radiance_dir(int(res), t.shape[0], _p(t), _p(d), _p(om)))
        return d, om

    def bake_probe_radiance(self, positions, n_samples, res, first_sample=0, key_base=0, sums=None, counts=None):
        """radiance maps (pt_bake_probe_radiance): adds the radiance of bake_probes' rays of samples [first_sample, first_sample + n_samples),
        the full path each, to the raw sums (n, res * res, 3) float32 and counts (n, res * res) uint32 per octahedral texel (None: zeros), in
        sample order per texel.  Returns (sums, counts)."""
        pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
        n, rr = pos.shape[0], int(res) * int(res)
        s = np.zeros((n, rr, 3), np.float32) if sums is None else np.ascontiguousarray(sums, np.float32).copy()
        k = np.zeros((n, rr), np.uint32) if counts is None else np.ascontiguousarray(counts, np.uint32).copy()
        if 2 <= int(res) <= 16 and (s.size != n * rr * 3 or k.size != n * rr):
            raise PtError(-1, "bake_probe_radiance: sums hold res * res * 3 values and counts res * res per probe")
        prm = ProbeRadianceParams(first_sample, n_samples, key_base, int(res))
        self._chk(self.L.pt_bake_probe_radiance(self.ctx, n, _p(pos), C.byref(prm), _p(s), _p(k)))
        return s, k

    def probe_radiance_prefilter(self, sums, counts, alphas, on_device=True):
        """the GGX prefilter of raw radiance maps (pt_probe_radiance_prefilter): sums (n, res * res, 3) and counts (n, res * res) to the table
        (n, levels, res * res, 4) float32 that set_probe_grid_radiance takes, one level per alpha; on the host (no GPU) unless on_device"""
        s = np.ascontiguousarray(sums, np.float32); k = np.ascontiguousarray(counts, np.uint32)
        if s.ndim != 3 or s.shape[2] != 3 or k.shape != s.shape[:2]:
            raise PtError(-1, "probe_radiance_prefilter: sums is (n, res * res, 3) and counts (n, res * res)")
        n, rr = k.shape
        res = int(round(np.sqrt(rr)))
        al = [float(a) for a in alphas]
        if res * res != rr or not 1 <= len(al) <= 8:
            raise PtError(-1, "probe_radiance_prefilter: res * res texels per probe and 1..8 alphas")
        f = ProbeRadianceFilter(res, n, len(al), (C.c_float * 8)(*al))
        table = np.zeros((n, len(al), rr, 4), np.float32)
        self._chk(self.L.pt_probe_radiance_prefilter(self.ctx, int(bool(on_device)), C.byref(f), _p(s), _p(k), _p(table)))
        return table

    def set_probe_grid_radiance(self, table, alphas=None):
        """radiance on the grid in force (pt_set_probe_grid_radiance): table (nodes, levels, res * res, 4) float32 as probe_radiance_prefilter
        returns it, alphas the levels' GGX alphas.  table None clears radiance."""
        if table is None:
            self._chk(self.L.pt_set_probe_grid_radiance(self.ctx, None, None))
            return
        if alphas is None:
            raise PtError(-1, "set_probe_grid_radiance: a table needs its levels' alphas")
        t = np.ascontiguousarray(table, np.float32)
        al = [float(a) for a in alphas]
        nodes = int(np.prod(self.probe_grid_info()[2]))
        res = int(round(np.sqrt(t.shape[2]))) if t.ndim == 4 else 0
        if t.ndim != 4 or t.shape[3] != 4 or t.shape[0] != nodes or t.shape[1] != len(al) or res * res != t.shape[2] or not 1 <= len(al) <= 8:
            raise PtError(-1, "set_probe_grid_radiance: table is (nodes, levels, res * res, 4) with one alpha per level")
        v = ProbeRadiance(res, len(al), (C.c_float * 8)(*al))
        self._chk(self.L.pt_set_probe_grid_radiance(self.ctx, C.byref(v), _p(t)))

    def set_probe_grid_radiance_sums(self, sums, counts, alphas, on_device=True):
        """set_probe_grid_radiance of bake_probe_radiance's raw sums and counts: the prefilter, then the setter.  Returns the table."""
        table = self.probe_radiance_prefilter(sums, counts, alphas, on_device)
        self.set_probe_grid_radiance(table, alphas)
        return table

    def probe_grid_radiance_info(self):
        """(res, alphas) of the grid's radiance; res 0: none"""
        v = ProbeRadiance()
        self._chk(self.L.pt_get_probe_grid_radiance_info(self.ctx, C.byref(v)))
        return int(v.res), tuple(float(v.alpha[l]) for l in range(int(v.n_levels)))

    def probe_grid_specular(self, position, normal, incoming, alpha, on_device=False):
        """unit hook: (rgb [n, 3], lit [n] uint8) of the reflection probes' lookup at world positions, normals and incoming directions [n, 3]
        and GGX alphas [n] (a scalar: the same for all); on the host (no GPU) unless on_device"""
        p = np.ascontiguousarray(position, np.float32).reshape(-1, 3); nn = np.ascontiguousarray(normal, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(incoming, np.float32).reshape(-1, 3)
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(alpha, np.float32), (p.shape[0],)))
        assert p.shape == nn.shape == d.shape
        out = np.zeros((p.shape[0], 3), np.float32); lit = np.zeros(p.shape[0], np.uint8)
        self._chk(self.L.pt_probe_grid_specular(self.ctx, int(bool(on_device)), p.shape[0], _p(p), _p(nn), _p(d), _p(a), _p(out), _p(lit)))
        return out, lit

    # ---- unit hooks
    def trace_closest(self, o, d, tmax=None, which=0):
        o = np.ascontiguousarray(o, np.float32)
        d = np.ascontiguousarray(d, np.float32)
        n = o.shape[0]
        tm = None if tmax is None else np.ascontiguousarray(tmax, np.float32)
        t = np.zeros(n, np.float32); u = np.zeros(n, np.float32); v = np.zeros(n, np.float32)
        inst = np.zeros(n, np.uint32); prim = np.zeros(n, np.uint32)
        self._chk(self.L.pt_trace_closest(self.ctx, which, n, _p(o), _p(d), _p(tm), _p(t), _p(u), _p(v), _p(inst), _p(prim)))
        return dict(t=t, u=u, v=v, inst=inst, prim=prim)

    def trace_any(self, o, d, tmax, which=0):
        o = np.ascontiguousarray(o, np.float32)
        d = np.ascontiguousarray(d, np.float32)
        tm = np.ascontiguousarray(tmax, np.float32)
        hit = np.zeros(o.shape[0], np.uint8)
        self._chk(self.L.pt_trace_any(self.ctx, which, o.shape[0], _p(o), _p(d), _p(tm), _p(hit)))
        return hit

    def ss_sobol(self, n_points, index, seed):
        index = np.ascontiguousarray(index, np.uint32)
        seed = np.ascontiguousarray(seed, np.uint32)
        out = np.zeros((index.size, 2), np.float32)
        self._chk(self.L.pt_ss_sobol(self.ctx, n_points, index.size, _p(index), _p(seed), _p(out)))
        return out

    def math_batch(self, fn, a, b=None):
        a = np.ascontiguousarray(a, np.float32)
        b = None if b is None else np.ascontiguousarray(b, np.float32)
        o0 = np.zeros_like(a)
        o1 = np.zeros_like(a)
        self._chk(self.L.pt_math_batch(self.ctx, fn, a.size, _p(a), _p(b), _p(o0), _p(o1)))
        return o0, o1

    def material_eval(self, material, incoming, normal, front, pixel, sample, draws_consumed=0):
        i = np.ascontiguousarray(incoming, np.float32); n = np.ascontiguousarray(normal, np.float32)
        f = np.ascontiguousarray(front, np.uint8); px = np.ascontiguousarray(pixel, np.uint32); sm = np.ascontiguousarray(sample, np.uint32)
        out = np.zeros((i.shape[0], 9), np.float32)
        self._chk(self.L.pt_material_eval(self.ctx, material, i.shape[0], _p(i), _p(n), _p(f), _p(px), _p(sm), draws_consumed, _p(out)))
        return out

    def volume_eval(self, material, incoming, t_max, dist, pixel, sample, draws_consumed=0):
        """[n, 9]: scattered, t, direction xyz, transmission over dist rgb, draws (pt_volume_eval)"""
        i = np.ascontiguousarray(incoming, np.float32); tm = np.ascontiguousarray(t_max, np.float32); d = np.ascontiguousarray(dist, np.float32)
        px = np.ascontiguousarray(pixel, np.uint32); sm = np.ascontiguousarray(sample, np.uint32)
        out = np.zeros((i.shape[0], 9), np.float32)
        self._chk(self.L.pt_volume_eval(self.ctx, material, i.shape[0], _p(i), _p(tm), _p(d), _p(px), _p(sm), draws_consumed, _p(out)))
        return out

    def bsdf_eval(self, material, incoming, outgoing, normal, front):
        """[n, 4]: bsdf rgb, pdf of the material at caller-chosen outgoing directions, as next-event estimation asks (pt_bsdf_eval)"""
        i = np.ascontiguousarray(incoming, np.float32); w = np.ascontiguousarray(outgoing, np.float32)
        n = np.ascontiguousarray(normal, np.float32); f = np.ascontiguousarray(front, np.uint8)
        out = np.zeros((i.shape[0], 4), np.float32)
        self._chk(self.L.pt_bsdf_eval(self.ctx, material, i.shape[0], _p(i), _p(w), _p(n), _p(f), _p(out)))
        return out

    def guide_follow_dir(self, material, incoming, normal, front, on_device=False):
        """[n, 4]: the direction the guide chain goes on in at hits of the material (xyz) and whether it is followed at all (1 / 0);
        on the host (no GPU) unless on_device (pt_guide_follow_dir)"""
        i = np.ascontiguousarray(incoming, np.float32); n = np.ascontiguousarray(normal, np.float32); f = np.ascontiguousarray(front, np.uint8)
        out = np.zeros((i.shape[0], 4), np.float32)
        self._chk(self.L.pt_guide_follow_dir(self.ctx, int(bool(on_device)), material, i.shape[0], _p(i), _p(n), _p(f), _p(out)))
        return out

    def model_vertices(self, model):
        n = C.c_uint32()
        self._chk(self.L.pt_model_vertices(self.ctx, model, None, None, 0, C.byref(n)))
        p = np.zeros((n.value, 3, 3), np.float32)
        nr = np.zeros((n.value, 3, 3), np.float32)
        self._chk(self.L.pt_model_vertices(self.ctx, model, _p(p), _p(nr), n.value, C.byref(n)))
        return p, nr

    # ---- host-builder introspection (CPU)
    def blas_count(self):
        return self._chk(self.L.pt_blas_count(self.ctx), allow_positive=True)

    def blas_dump(self, blas, cap=1 << 20):
        nn = C.c_uint32(); root = C.c_uint32(); nids = C.c_uint32()
        boxes = np.zeros((cap, 6), np.float32); kind = np.zeros(cap, np.uint32); a = np.zeros(cap, np.uint32); b = np.zeros(cap, np.uint32)
        ids = np.zeros(cap, np.uint32)
        self._chk(self.L.pt_blas_dump(self.ctx, blas, C.byref(nn), C.byref(root), _p(boxes), _p(kind), _p(a), _p(b), C.byref(nids), _p(ids), cap, cap))
        n = nn.value
        return dict(root=root.value, boxes=boxes[:n].copy(), kind=kind[:n].copy(), a=a[:n].copy(), b=b[:n].copy(), prim_ids=ids[:nids.value].copy())

    def tlas_dump(self, which=0, cap=1 << 16):
        nn = C.c_uint32(); root = C.c_uint32()
        boxes = np.zeros((cap, 6), np.float32); kind = np.zeros(cap, np.uint32); a = np.zeros(cap, np.uint32); b = np.zeros(cap, np.uint32)
        self._chk(self.L.pt_tlas_dump(self.ctx, which, C.byref(nn), C.byref(root), _p(boxes), _p(kind), _p(a), _p(b), cap))
        n = nn.value
        return dict(root=root.value, boxes=boxes[:n].copy(), kind=kind[:n].copy(), a=a[:n].copy(), b=b[:n].copy())

    def tlas_instances(self, which=0, cap=1 << 16):
        """matrix / inv_matrix of every TLAS leaf (leaf allocation order), [n, 3, 4] each"""
        n = C.c_uint32()
        m = np.zeros((cap, 3, 4), np.float32); inv = np.zeros((cap, 3, 4), np.float32)
        self._chk(self.L.pt_tlas_instances(self.ctx, which, C.byref(n), _p(m), _p(inv), cap))
        return dict(matrix=m[:n.value].copy(), inv_matrix=inv[:n.value].copy())

    def instance_materials(self, which=0, cap=1 << 16):
        """material index every TLAS leaf is shaded with and the model it instantiates (leaf allocation order)"""
        n = C.c_uint32()
        mat = np.zeros(cap, np.uint32); bl = np.zeros(cap, np.uint32)
        self._chk(self.L.pt_instance_materials(self.ctx, which, C.byref(n), _p(mat), _p(bl), cap))
        return dict(material=mat[:n.value].copy(), blas=bl[:n.value].copy())

    def light_cdf(self, cap=1 << 20):
        n = C.c_uint32(); mx = C.c_float()
        pdf = np.zeros(cap, np.float32); cdf = np.zeros(cap, np.float32); bl = np.zeros(cap, np.uint32); pr = np.zeros(cap, np.uint32)
        self._chk(self.L.pt_light_cdf(self.ctx, C.byref(n), _p(pdf), _p(cdf), _p(bl), _p(pr), C.byref(mx), cap))
        k = n.value
        return dict(pdf=pdf[:k].copy(), cdf=cdf[:k].copy(), blas=bl[:k].copy(), prim=pr[:k].copy(), max=mx.value)

    def triangle(self, blas, prim):
        out = np.zeros(36, np.float32)
        self._chk(self.L.pt_triangle_dump(self.ctx, blas, prim, _p(out)))
        return out

    # ---- measurement
    def stats(self) -> Stats:
        s = Stats()
        self._chk(self.L.pt_get_stats(self.ctx, C.byref(s)))
        return s

    def last_batch_counters(self):
        rows = np.zeros((self.cfg.max_bounces + 2, 16), np.uint32)
        n = C.c_uint32()
        self._chk(self.L.pt_last_batch_counters(self.ctx, _p(rows), rows.shape[0], C.byref(n)))
        return rows[: n.value]

    def last_launches(self, which=LAUNCHES_BATCH):
        """pt_last_launches: the keyed launches of the last batch (or hook request) as (launcher name, counter row, axis values) tuples"""
        n = C.c_uint32()
        self._chk(self.L.pt_last_launches(self.ctx, which, None, 0, C.byref(n)))
        rows = np.zeros((max(n.value, 1), 8), np.uint32)
        self._chk(self.L.pt_last_launches(self.ctx, which, _p(rows), rows.shape[0], C.byref(n)))
        return [(LAUNCHERS[int(r[0])], int(r[1]), tuple(int(v) for v in r[2:2 + len(variant_axes(LAUNCHERS[int(r[0])]))])) for r in rows[: n.value]]

    def trace_geometry(self):
        """pt_trace_geometry: {block_threads, trace_blocks, stack_lds, shade_traces_shadow} of the uploaded scene (uploads it if need be)"""
        z = np.zeros((0, 3), np.float32)
        self.trace_closest(z, z)   # no rays: uploads the scene and launches nothing
        out = np.zeros(4, np.uint32)
        self._chk(self.L.pt_trace_geometry(self.ctx, _p(out)))
        return {"block_threads": int(out[0]), "trace_blocks": int(out[1]), "stack_lds": int(out[2]), "shade_traces_shadow": bool(out[3])}

    def last_batch_shade_pids(self, qclass, first, count):
        out = np.zeros(count, np.uint32)
        self._chk(self.L.pt_last_batch_shade_pids(self.ctx, qclass, first, count, _p(out)))
        return out

    def last_batch_step_stats(self):
        rows = np.zeros((self.cfg.max_bounces + 2, 8), np.uint32)
        n = C.c_uint32()
        self._chk(self.L.pt_last_batch_step_stats(self.ctx, _p(rows), rows.shape[0], C.byref(n)))
        return rows[: n.value]

    def reset_stats(self):
        self._chk(self.L.pt_reset_stats(self.ctx))


class MultiRenderer:
    """One process, several devices (pt_multi): rows dealt to the devices in strips, one host thread per device while rendering, one
    RCCL gather of the strip framebuffers to devices[0].  `devices` may list a device more than once (contexts then share it and the
    gather is device-to-device copies): that is how the assembly is tested on a one-GPU box."""

    def __init__(self, scene: SceneDesc, width: int, height: int, devices, **kw):
        self.L = lib()
        devices = [int(d) for d in devices]
        kw.setdefault("strip_rows", 4)
        cfg = Config(width, height, kw.get("max_bounces", 8), kw.get("n_sobol", 512), int(kw.get("enable_nee", True)), kw.get("seed", DEFAULT_SEED), 0, 1,
                     kw["strip_rows"], kw.get("batch_spp", 0), -1, kw.get("flags", 0), 0, 0, kw.get("pipelines", 0), 0)
        arr = (C.c_int32 * len(devices))(*devices)
        self.m = C.c_void_p(self.L.pt_multi_create(C.byref(cfg), arr, len(devices)))
        if not self.m:
            raise PtError(-1, "pt_multi_create failed")
        self.width, self.height, self.n = width, height, len(devices)
        self.rank0 = Renderer.attach(self.L.pt_multi_ctx(self.m, 0), cfg)
        for mod in scene.models:
            self.rank0.add_model(mod)
        self.rank0.rebuild()
        if scene.camera is not None:
            self.rank0.set_camera(scene.camera)

    def _chk(self, r):
        if r != 0:
            raise PtError(r, self.L.pt_multi_last_error(self.m).decode())

    def render(self, first_sample: int, n_samples: int, download=True):
        out = np.zeros((self.height, self.width, 4), np.float32) if download else None
        self._chk(self.L.pt_multi_render(self.m, first_sample, n_samples, _p(out)))
        return out

    def reset_accumulation(self):
        self._chk(self.L.pt_multi_reset_accumulation(self.m))

    def write_image(self, path):
        self._chk(self.L.pt_multi_write_image(self.m, str(path).encode()))

    def used_rccl(self) -> bool:
        return bool(self.L.pt_multi_used_rccl(self.m))

    def stats(self) -> Stats:
        s = Stats()
        self._chk(self.L.pt_multi_get_stats(self.m, C.byref(s)))
        return s

    def close(self):
        if getattr(self, "m", None):
            self.rank0.close()
            self.L.pt_multi_destroy(self.m)
            self.m = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
