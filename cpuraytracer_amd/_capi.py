"""ctypes binding of cpuraytracer_amd/lib/librt_hip.so (the C ABI of include/rt_api.h).

The library is hand-written HIP for gfx950; there is no CPU fallback.  Loading succeeds without a
GPU (so the symbol table can be checked on a CPU-only host) but rt_create fails loudly there.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "librt_hip.so")


class RtSphere(C.Structure):
    _fields_ = [("cx", C.c_float), ("cy", C.c_float), ("cz", C.c_float), ("r", C.c_float)]


class RtMaterial(C.Structure):
    _fields_ = [("type", C.c_uint32), ("tex_type", C.c_uint32), ("smoothness", C.c_float), ("ior", C.c_float),
                ("tiling", C.c_float), ("rgb0", C.c_float * 3), ("rgb1", C.c_float * 3), ("luminance", C.c_float)]


class RtCamera(C.Structure):
    _fields_ = [("origin", C.c_float * 4), ("x", C.c_float * 4), ("y", C.c_float * 4),
                ("origin_image_plane", C.c_float * 4), ("aperture", C.c_float), ("focal_length", C.c_float)]


class RtLight(C.Structure):
    _fields_ = [("direction", C.c_float * 3), ("color", C.c_float * 3), ("luminance", C.c_float)]


class RtRowset(C.Structure):
    _fields_ = [("first_row", C.c_uint32), ("num_rows", C.c_uint32), ("block_rows", C.c_uint32),
                ("shard", C.c_uint32), ("nshards", C.c_uint32)]


class RtStats(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("traversals", C.c_uint64), ("segments", C.c_uint64),
                ("ms_render", C.c_double), ("ms_accumulate", C.c_double), ("ms_resolve", C.c_double),
                ("local_rows", C.c_uint32), ("passes", C.c_uint32)]


class RtDenoiseParams(C.Structure):
    _fields_ = [("levels", C.c_uint32), ("k_normal", C.c_float), ("k_depth", C.c_float), ("k_albedo", C.c_float),
                ("k_coverage", C.c_float), ("k_colour", C.c_float), ("var_floor", C.c_float)]


class RtTemporalParams(C.Structure):
    _fields_ = [("max_history", C.c_uint32), ("use_id", C.c_uint32), ("depth_tol", C.c_float), ("normal_tol", C.c_float),
                ("coverage_tol", C.c_float)]


class RtVarianceParams(C.Structure):
    """rt_variance_params: where the filter's v0 comes from (source 0 the second moments, 1 the spatial estimate) and the window's radius."""
    _fields_ = [("source", C.c_uint32), ("radius", C.c_uint32)]


class RtShardParts(C.Structure):
    """rt_shard_parts: the gathered parts of a row-sharded picture (device pointers) and their shape."""
    _fields_ = [("hdr", C.c_void_p), ("sq", C.c_void_p), ("feat", C.c_void_p), ("W", C.c_uint32), ("rows_max", C.c_uint32),
                ("rs", RtRowset), ("n", C.c_uint32), ("m", C.c_uint32)]


class RtShardFrame(C.Structure):
    """rt_shard_frame: the parts, the shards' ids in the same layout (a device pointer), the image's height and the shards' camera."""
    _fields_ = [("parts", RtShardParts), ("ids", C.c_void_p), ("H", C.c_uint32), ("camera", RtCamera)]


SPHERE_DTYPE = np.dtype([("cx", "<f4"), ("cy", "<f4"), ("cz", "<f4"), ("r", "<f4")])
MATERIAL_DTYPE = np.dtype([("type", "<u4"), ("tex_type", "<u4"), ("smoothness", "<f4"), ("ior", "<f4"),
                           ("tiling", "<f4"), ("rgb0", "<f4", (3,)), ("rgb1", "<f4", (3,)), ("luminance", "<f4")])

RT_OK = 0
RT_ERR_NO_DEVICE = 1
RT_ERR_SEQUENCE = 6
RT_SAMPLER_COSINE_HEMISPHERE, RT_SAMPLER_SQRT_DISK = 1, 2
RT_TEMPORAL_FETCH_NEAREST, RT_TEMPORAL_FETCH_BILINEAR = 1, 4
RT_VARIANCE_MOMENTS, RT_VARIANCE_SPATIAL = 0, 1

# every symbol include/rt_api.h declares
EXPORTS = [
    "rt_last_error", "rt_api_version", "rt_create", "rt_destroy", "rt_set_stream", "rt_set_workspace_limit", "rt_set_sampler", "rt_set_frame_pipelining", "rt_set_frame_batch", "rt_set_frame_lookahead", "rt_committed_samples",
    "rt_scene_upload", "rt_render", "rt_clear", "rt_resolve", "rt_last_resolve_ms", "rt_download", "rt_copy_to_device",
    "rt_synchronize", "rt_rowset_local_rows", "rt_rowset_global_row", "rt_unit_halton", "rt_unit_math", "rt_unit_math_host",
    "rt_unit_primary_rays", "rt_unit_closest_hit", "rt_unit_trace", "rt_unit_camera_rays", "rt_unit_scatter", "rt_unit_tonemap", "rt_unit_layout", "rt_unit_layout_info", "rt_unit_grid_rows", "rt_unit_grid_info",
    "rt_unit_tile_masks", "rt_unit_tile_masks_host", "rt_unit_tile_cone", "rt_unit_tile_spheres", "rt_unit_tile_spheres_host", "rt_unit_sky_planes", "rt_unit_sky_excluded",
    "rt_set_noise_estimate", "rt_download_moments", "rt_noise_map", "rt_noise_summary", "rt_unit_noise_estimate_host",
    "rt_render_features", "rt_feature_samples", "rt_download_features", "rt_copy_features_to_device", "rt_clear_features",
    "rt_unit_features_host",
    "rt_unit_shadow_index_host", "rt_unit_shadow_query_host", "rt_unit_shadow",
    "rt_unit_launch_plan", "rt_unit_last_trace_launch", "rt_unit_trace_variants",
    "rt_unit_trace_lean_variants", "rt_unit_last_trace_far_state", "rt_unit_far_state_plan",
    "rt_unit_shadow_index_host_tier", "rt_unit_shadow_query_host_tier", "rt_unit_shadow_tier",
    "rt_denoise_default_params", "rt_denoise", "rt_download_denoised", "rt_copy_denoised_to_device", "rt_unit_denoise_host", "rt_unit_denoise_forms",
    "rt_copy_moments_to_device", "rt_rowset_locate", "rt_denoise_shards", "rt_unit_denoise_shards_host",
    "rt_temporal_default_params", "rt_denoise_temporal", "rt_temporal_reset", "rt_download_temporal", "rt_unit_temporal_host",
    "rt_temporal_default_params_fetch", "rt_denoise_temporal_fetch", "rt_unit_temporal_host_fetch",
    "rt_denoise_shards_temporal", "rt_unit_temporal_shards_host",
    "rt_variance_default_params", "rt_denoise_variance", "rt_denoise_temporal_variance", "rt_unit_denoise_variance_host", "rt_unit_temporal_variance_host",
    "rt_denoise_shards_variance", "rt_denoise_shards_temporal_variance", "rt_unit_denoise_shards_variance_host", "rt_unit_temporal_shards_variance_host",
    "rt_set_camera", "rt_get_camera",
    "rt_set_materials", "rt_set_lights", "rt_set_exposure", "rt_temporal_forget", "rt_unit_temporal_forget_host",
    "rt_unit_tile_order", "rt_unit_tile_order_sort",
    "rt_turn_lights", "rt_get_lights",
]

_lib = None


class RtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("librt_hip: [%d] %s" % (code, msg))
        self.code = code


def load():
    """dlopen librt_hip.so; raises if the library has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("librt_hip.so is missing (%s): run `python -c 'import __graft_entry__ as g; g.build()'`; "
                           "there is no CPU fallback for the render path" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    L.rt_last_error.restype = C.c_char_p
    L.rt_api_version.restype = C.c_int
    L.rt_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.rt_destroy.argtypes = [C.c_void_p]
    L.rt_destroy.restype = None
    L.rt_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    L.rt_set_workspace_limit.argtypes = [C.c_void_p, C.c_uint64]
    L.rt_set_sampler.argtypes = [C.c_void_p, C.c_uint32]
    L.rt_set_frame_pipelining.argtypes = [C.c_void_p, C.c_uint32]
    L.rt_set_frame_batch.argtypes = [C.c_void_p, C.c_uint32]
    L.rt_committed_samples.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    L.rt_set_frame_lookahead.argtypes = [C.c_void_p, C.c_uint32]
    L.rt_scene_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(RtCamera), C.POINTER(RtLight), C.c_uint32,
                                  C.POINTER(RtMaterial), C.c_float]
    L.rt_set_camera.argtypes = [C.c_void_p, C.POINTER(RtCamera)]
    L.rt_get_camera.argtypes = [C.c_void_p, C.POINTER(RtCamera)]
    if hasattr(L, "rt_set_materials"):
        L.rt_set_materials.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(RtMaterial)]
        L.rt_set_lights.argtypes = [C.c_void_p, C.POINTER(RtLight), C.c_uint32]
        L.rt_set_exposure.argtypes = [C.c_void_p, C.c_float]
        L.rt_temporal_forget.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.rt_unit_temporal_forget_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32]
    if hasattr(L, "rt_turn_lights"):
        L.rt_turn_lights.argtypes = [C.c_void_p, C.POINTER(RtLight), C.c_uint32]
        L.rt_get_lights.argtypes = [C.c_void_p, C.POINTER(RtLight), C.c_uint32, C.POINTER(C.c_uint32)]
    L.rt_render.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, RtRowset, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                            C.POINTER(RtStats)]
    L.rt_clear.argtypes = [C.c_void_p]
    L.rt_resolve.argtypes = [C.c_void_p, C.c_uint32]
    L.rt_last_resolve_ms.argtypes = [C.c_void_p]
    L.rt_last_resolve_ms.restype = C.c_double
    L.rt_download.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.rt_copy_to_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.rt_synchronize.argtypes = [C.c_void_p]
    L.rt_rowset_local_rows.argtypes = [RtRowset]
    L.rt_rowset_local_rows.restype = C.c_uint32
    L.rt_rowset_global_row.argtypes = [RtRowset, C.c_uint32]
    L.rt_rowset_global_row.restype = C.c_uint32
    L.rt_unit_halton.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    L.rt_unit_math.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    if hasattr(L, "rt_unit_math_host"):  # (older builds of the library in A/B runs: tools/ab_run.sh)
        L.rt_unit_math_host.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.rt_unit_primary_rays.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
    L.rt_unit_closest_hit.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.rt_unit_trace.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64,
                                C.c_void_p, C.c_void_p]
    L.rt_unit_camera_rays.argtypes = [C.c_void_p, C.POINTER(RtCamera), C.c_void_p, C.c_uint32, C.c_void_p]
    L.rt_unit_scatter.argtypes = [C.c_void_p, C.POINTER(RtMaterial), C.POINTER(RtLight), C.POINTER(C.c_float), C.c_void_p, C.c_uint32,
                                  C.c_void_p]
    L.rt_unit_tonemap.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    L.rt_unit_layout.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p]
    L.rt_unit_layout_info.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    if hasattr(L, "rt_unit_grid_info"):
        L.rt_unit_grid_info.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.c_void_p]
    # the tile-mask entries are bound only where the library has them: A/B tools load older builds of the library through this module
    if hasattr(L, "rt_unit_tile_masks"):
        L.rt_unit_tile_masks.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, RtRowset, C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p,
                                         C.c_uint32, C.c_void_p, C.c_void_p]
        L.rt_unit_tile_masks_host.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(RtCamera), C.c_uint32, C.c_uint32, RtRowset, C.c_uint32,
                                              C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p]
        L.rt_unit_tile_cone.argtypes = [C.POINTER(RtCamera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    if hasattr(L, "rt_unit_sky_planes"):
        L.rt_unit_sky_planes.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    if hasattr(L, "rt_unit_sky_excluded"):
        L.rt_unit_sky_excluded.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    if hasattr(L, "rt_unit_tile_spheres"):
        L.rt_unit_tile_spheres.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, RtRowset, C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p]
        L.rt_unit_tile_spheres_host.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(RtCamera), C.c_uint32, C.c_uint32, RtRowset, C.c_uint32, C.c_uint32,
                                                C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p]
    if hasattr(L, "rt_unit_tile_order"):
        L.rt_unit_tile_order.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, RtRowset, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p]
        L.rt_unit_tile_order_sort.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    if hasattr(L, "rt_set_noise_estimate"):
        L.rt_set_noise_estimate.argtypes = [C.c_void_p, C.c_int]
        L.rt_download_moments.argtypes = [C.c_void_p, C.c_void_p]
        L.rt_noise_map.argtypes = [C.c_void_p, C.c_float, C.c_void_p]
        L.rt_noise_summary.argtypes = [C.c_void_p, C.c_float, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_float)]
        L.rt_unit_noise_estimate_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p]
    if hasattr(L, "rt_render_features"):
        L.rt_render_features.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, RtRowset, C.c_uint32, C.c_uint32, C.POINTER(C.c_double)]
        L.rt_feature_samples.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        L.rt_download_features.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.rt_copy_features_to_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.rt_clear_features.argtypes = [C.c_void_p]
        L.rt_unit_features_host.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(RtMaterial), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    if hasattr(L, "rt_unit_shadow"):
        L.rt_unit_shadow_index_host.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(RtLight), C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_float),
                                                C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
        L.rt_unit_shadow_query_host.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(RtLight), C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
        L.rt_unit_shadow.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    if hasattr(L, "rt_unit_launch_plan"):
        L.rt_unit_launch_plan.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    if hasattr(L, "rt_unit_last_trace_launch"):
        L.rt_unit_last_trace_launch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
        L.rt_unit_trace_variants.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    if hasattr(L, "rt_unit_last_trace_far_state"):
        L.rt_unit_trace_lean_variants.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        L.rt_unit_last_trace_far_state.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        L.rt_unit_far_state_plan.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
        L.rt_unit_shadow_index_host_tier.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(RtLight), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32),
                                                     C.POINTER(C.c_float), C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                                     C.c_void_p]
        L.rt_unit_shadow_query_host_tier.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(RtLight), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32,
                                                     C.c_void_p]
        L.rt_unit_shadow_tier.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    if hasattr(L, "rt_denoise"):
        L.rt_denoise_default_params.argtypes = [C.POINTER(RtDenoiseParams)]
        L.rt_denoise.argtypes = [C.c_void_p, C.POINTER(RtDenoiseParams), C.POINTER(C.c_double)]
        L.rt_download_denoised.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rt_copy_denoised_to_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rt_unit_denoise_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(RtDenoiseParams),
                                           C.c_void_p, C.c_void_p]
        L.rt_unit_denoise_forms.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    if hasattr(L, "rt_denoise_shards"):
        L.rt_copy_moments_to_device.argtypes = [C.c_void_p, C.c_void_p]
        L.rt_rowset_locate.argtypes = [RtRowset, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.rt_denoise_shards.argtypes = [C.c_void_p, C.POINTER(RtShardParts), C.POINTER(RtDenoiseParams), C.POINTER(C.c_double)]
        L.rt_unit_denoise_shards_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(RtShardParts), C.POINTER(RtDenoiseParams),
                                                  C.c_void_p, C.c_void_p]
    if hasattr(L, "rt_denoise_temporal"):
        L.rt_temporal_default_params.argtypes = [C.POINTER(RtTemporalParams)]
        L.rt_denoise_temporal.argtypes = [C.c_void_p, C.POINTER(RtDenoiseParams), C.POINTER(RtTemporalParams), C.POINTER(C.c_double)]
        L.rt_temporal_reset.argtypes = [C.c_void_p]
        L.rt_download_temporal.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rt_unit_temporal_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                            C.c_uint32, C.POINTER(RtCamera), C.POINTER(RtCamera), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.POINTER(RtDenoiseParams), C.POINTER(RtTemporalParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p]
    if hasattr(L, "rt_denoise_temporal_fetch"):
        L.rt_temporal_default_params_fetch.argtypes = [C.c_uint32, C.POINTER(RtTemporalParams)]
        L.rt_denoise_temporal_fetch.argtypes = [C.c_void_p, C.POINTER(RtDenoiseParams), C.POINTER(RtTemporalParams), C.c_uint32, C.POINTER(C.c_double)]
        L.rt_unit_temporal_host_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                                  C.c_uint32, C.POINTER(RtCamera), C.POINTER(RtCamera), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.POINTER(RtDenoiseParams), C.POINTER(RtTemporalParams), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(L, "rt_denoise_shards_temporal"):
        L.rt_denoise_shards_temporal.argtypes = [C.c_void_p, C.POINTER(RtShardFrame), C.POINTER(RtDenoiseParams), C.POINTER(RtTemporalParams), C.c_uint32,
                                                 C.POINTER(C.c_double)]
        L.rt_unit_temporal_shards_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(RtShardFrame), C.POINTER(RtCamera), C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(RtDenoiseParams), C.POINTER(RtTemporalParams), C.c_uint32,
                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(L, "rt_denoise_variance"):
        L.rt_variance_default_params.argtypes = [C.POINTER(RtVarianceParams)]
        L.rt_denoise_variance.argtypes = [C.c_void_p, C.POINTER(RtDenoiseParams), C.POINTER(RtVarianceParams), C.POINTER(C.c_double)]
        L.rt_denoise_temporal_variance.argtypes = [C.c_void_p, C.POINTER(RtDenoiseParams), C.POINTER(RtTemporalParams), C.c_uint32,
                                                   C.POINTER(RtVarianceParams), C.POINTER(C.c_double)]
        L.rt_unit_denoise_variance_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                                    C.POINTER(RtDenoiseParams), C.POINTER(RtVarianceParams), C.c_void_p, C.c_void_p, C.c_void_p]
        L.rt_unit_temporal_variance_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                                     C.c_uint32, C.POINTER(RtCamera), C.POINTER(RtCamera), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.POINTER(RtDenoiseParams), C.POINTER(RtTemporalParams), C.c_uint32, C.POINTER(RtVarianceParams),
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(L, "rt_denoise_shards_variance"):
        L.rt_denoise_shards_variance.argtypes = [C.c_void_p, C.POINTER(RtShardParts), C.POINTER(RtDenoiseParams), C.POINTER(RtVarianceParams), C.POINTER(C.c_double)]
        L.rt_denoise_shards_temporal_variance.argtypes = [C.c_void_p, C.POINTER(RtShardFrame), C.POINTER(RtDenoiseParams), C.POINTER(RtTemporalParams), C.c_uint32,
                                                          C.POINTER(RtVarianceParams), C.POINTER(C.c_double)]
        L.rt_unit_denoise_shards_variance_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(RtShardParts), C.POINTER(RtDenoiseParams),
                                                           C.POINTER(RtVarianceParams), C.c_void_p, C.c_void_p, C.c_void_p]
        L.rt_unit_temporal_shards_variance_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(RtShardFrame), C.POINTER(RtCamera), C.c_void_p,
                                                            C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(RtDenoiseParams), C.POINTER(RtTemporalParams), C.c_uint32,
                                                            C.POINTER(RtVarianceParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    _lib = L
    return L


def check(rc):
    if rc != RT_OK:
        raise RtError(rc, load().rt_last_error().decode())


def denoise_params(**fields):
    """rt_denoise_default_params with the given fields replaced (levels, k_normal, k_depth, k_albedo, k_coverage, k_colour, var_floor)."""
    p = RtDenoiseParams()
    check(load().rt_denoise_default_params(C.byref(p)))
    for k, v in fields.items():
        if k not in dict(RtDenoiseParams._fields_):
            raise TypeError("rt_denoise_params has no field %r" % k)
        setattr(p, k, v)
    return p


def temporal_params(**fields):
    """rt_temporal_default_params with the given fields replaced (max_history, use_id, depth_tol, normal_tol, coverage_tol)."""
    p = RtTemporalParams()
    check(load().rt_temporal_default_params(C.byref(p)))
    for k, v in fields.items():
        if k not in dict(RtTemporalParams._fields_):
            raise TypeError("rt_temporal_params has no field %r" % k)
        setattr(p, k, v)
    return p


def temporal_params_fetch(fetch, **fields):
    """rt_temporal_default_params_fetch(fetch) with the given fields replaced."""
    p = RtTemporalParams()
    check(load().rt_temporal_default_params_fetch(fetch, C.byref(p)))
    for k, v in fields.items():
        if k not in dict(RtTemporalParams._fields_):
            raise TypeError("rt_temporal_params has no field %r" % k)
        setattr(p, k, v)
    return p


def variance_params(**fields):
    """rt_variance_default_params with the given fields replaced (source: RT_VARIANCE_MOMENTS 0 or RT_VARIANCE_SPATIAL 1; radius 1..3)."""
    p = RtVarianceParams()
    check(load().rt_variance_default_params(C.byref(p)))
    for k, v in fields.items():
        if k not in dict(RtVarianceParams._fields_):
            raise TypeError("rt_variance_params has no field %r" % k)
        setattr(p, k, v)
    return p


def unit_denoise_variance_host(hdr, sq, n, feat8, m, params=None, variance=None):
    """rt_unit_denoise_variance_host over numpy strips (hdr [rows, W, 3]; sq the same or None, which only the spatial source accepts;
    feat8 [rows, W, 8]).  Returns rgb, var (den and den_var) and state, the prepared (c0, v0) [rows, W, 4]."""
    hdr = np.ascontiguousarray(hdr, dtype=np.float32)
    feat8 = np.ascontiguousarray(feat8, dtype=np.float32)
    sq = None if sq is None else np.ascontiguousarray(sq, dtype=np.float32)
    rows, W = hdr.shape[:2]
    out = {"rgb": np.full((rows, W, 3), -1.0, np.float32), "var": np.full((rows, W), -1.0, np.float32), "state": np.full((rows, W, 4), -1.0, np.float32)}
    check(load().rt_unit_denoise_variance_host(hdr.ctypes.data, sq.ctypes.data if sq is not None else None, n, feat8.ctypes.data, m, W, rows,
                                               C.byref(params) if params is not None else None, C.byref(variance) if variance is not None else None,
                                               out["rgb"].ctypes.data, out["var"].ctypes.data, out["state"].ctypes.data))
    return out


FORGET_SKY = 0xffffffff  # the id rt_temporal_forget and its twin take for the sky


def unit_temporal_forget_host(length, ids, n_spheres, forget_ids):
    """rt_unit_temporal_forget_host over numpy arrays: a copy of `length` (any shape, uint32) with 0 wherever the pixel's id (ids, the
    same shape) is one of forget_ids; FORGET_SKY names the sky, ids at or above n_spheres match nothing."""
    out = np.array(length, dtype=np.uint32, copy=True, order="C")
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    assert ids.size == out.size
    f = np.ascontiguousarray(forget_ids, dtype=np.uint32).reshape(-1)
    check(load().rt_unit_temporal_forget_host(out.ctypes.data if out.size else None, ids.ctypes.data if ids.size else None, out.size, int(n_spheres),
                                              f.ctypes.data if f.size else None, f.size))
    return out


def unit_temporal_host(hdr, sq, n, feat8, m, ids, W, H, camera, history=None, params=None, tparams=None, first_row=0, fetch=1, variance=None):
    """rt_unit_temporal_host_fetch (fetch 1, nearest: rt_unit_temporal_host's bits; 4: bilinear; tparams None: that fetch's defaults) over numpy strips of rows [first_row, first_row + rows) of the W x H image.  history: None (empty) or a dict
    with camera, state (rows, W, 4), guides (rows, W, 8), ids and len (rows, W).  Returns a dict: rgb, var (den and den_var), target,
    and state, guides, len, ids, camera -- the last five are the next call's history."""
    hdr = np.ascontiguousarray(hdr, dtype=np.float32)
    sq = None if sq is None else np.ascontiguousarray(sq, dtype=np.float32)
    feat8 = np.ascontiguousarray(feat8, dtype=np.float32)
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    rows = hdr.size // (3 * W)
    assert hdr.size == rows * W * 3 and (sq is None or sq.size == hdr.size) and feat8.size == rows * W * 8 and ids.size == rows * W
    out = {"rgb": np.zeros((rows, W, 3), np.float32), "var": np.zeros((rows, W), np.float32), "state": np.zeros((rows, W, 4), np.float32),
           "guides": np.zeros((rows, W, 8), np.float32), "len": np.zeros((rows, W), np.uint32), "target": np.zeros((rows, W), np.uint32)}
    cam = RtCamera.from_buffer_copy(bytes(camera))
    if history is None:
        hc, hs, hg, hi, hl = None, None, None, None, None
    else:
        hc = C.byref(RtCamera.from_buffer_copy(bytes(history["camera"])))
        keep = [np.ascontiguousarray(history["state"], dtype=np.float32), np.ascontiguousarray(history["guides"], dtype=np.float32),
                np.ascontiguousarray(history["ids"], dtype=np.uint32), np.ascontiguousarray(history["len"], dtype=np.uint32)]
        assert keep[0].size == rows * W * 4 and keep[1].size == rows * W * 8 and keep[2].size == rows * W and keep[3].size == rows * W
        hs, hg, hi, hl = (a.ctypes.data for a in keep)
    tail = (out["rgb"].ctypes.data, out["var"].ctypes.data, out["state"].ctypes.data, out["guides"].ctypes.data, out["len"].ctypes.data,
            out["target"].ctypes.data)
    head = (hdr.ctypes.data, sq.ctypes.data if sq is not None else None, n, feat8.ctypes.data, m, ids.ctypes.data, W, H, first_row, rows, C.byref(cam),
            hc, hs, hg, hi, hl, C.byref(params) if params is not None else None, C.byref(tparams) if tparams is not None else None, int(fetch))
    if variance is None:
        check(load().rt_unit_temporal_host_fetch(*head, *tail))
    else:  # (rt_unit_temporal_variance_host: sq None is accepted under the spatial source only)
        check(load().rt_unit_temporal_variance_host(*head, C.byref(variance), *tail))
    out["ids"] = ids.reshape(rows, W).copy()
    out["camera"] = cam
    return out


def shard_parts(W, H, world, rows_max, n, m, hdr=None, sq=None, feat=None, block_rows=None, first_row=0):
    """An rt_shard_parts for a W x H picture cut cyclically into `world` shards of block_rows rows (default BLOCK_ROWS)."""
    rs = RtRowset(first_row, H, BLOCK_ROWS if block_rows is None else block_rows, 0, world)
    return RtShardParts(hdr or None, sq or None, feat or None, W, rows_max, rs, n, m)


def shard_frame(W, H, world, rows_max, n, m, camera, hdr=None, sq=None, feat=None, ids=None, block_rows=None, first_row=0, num_rows=None):
    """An rt_shard_frame: rows [first_row, first_row + num_rows) (default: all) of the W x H image, rendered with `camera` (an
    rt_camera record) and cut cyclically into `world` shards of block_rows rows (default BLOCK_ROWS)."""
    parts = shard_parts(W, H - first_row if num_rows is None else num_rows, world, rows_max, n, m, hdr, sq, feat, block_rows=block_rows, first_row=first_row)
    return RtShardFrame(parts, ids or None, H, RtCamera.from_buffer_copy(bytes(camera)))


def unit_denoise_shards_variance_host(hdr, sq, feat8, parts, params=None, variance=None):
    """rt_unit_denoise_shards_variance_host over numpy parts ([world, rows_max, W, c] each; sq None is accepted under the spatial source
    only) shaped by `parts` (shard_parts(...), its pointers unused).  Returns rgb, var and state, the prepared (c0, v0), in image order."""
    hdr = np.ascontiguousarray(hdr, dtype=np.float32)
    sq = None if sq is None else np.ascontiguousarray(sq, dtype=np.float32)
    feat8 = np.ascontiguousarray(feat8, dtype=np.float32)
    W, rows, px = parts.W, parts.rs.num_rows, parts.rs.nshards * parts.rows_max * parts.W
    assert hdr.size == px * 3 and (sq is None or sq.size == px * 3) and feat8.size == px * 8
    out = {"rgb": np.full((rows, W, 3), -1.0, np.float32), "var": np.full((rows, W), -1.0, np.float32), "state": np.full((rows, W, 4), -1.0, np.float32)}
    check(load().rt_unit_denoise_shards_variance_host(hdr.ctypes.data, sq.ctypes.data if sq is not None else None, feat8.ctypes.data, C.byref(parts),
                                                      C.byref(params) if params is not None else None, C.byref(variance) if variance is not None else None,
                                                      out["rgb"].ctypes.data, out["var"].ctypes.data, out["state"].ctypes.data))
    return out


def unit_temporal_shards_variance_host(hdr, sq, feat8, ids, frame, history=None, params=None, tparams=None, fetch=1, variance=None):
    """rt_unit_temporal_shards_variance_host: unit_temporal_shards_host with the variance source chosen; sq None is accepted under the
    spatial source only."""
    return unit_temporal_shards_host(hdr, sq, feat8, ids, frame, history, params, tparams, fetch, variance, _entry="rt_unit_temporal_shards_variance_host")


def unit_temporal_shards_host(hdr, sq, feat8, ids, frame, history=None, params=None, tparams=None, fetch=1, variance=None, _entry=None):
    """rt_unit_temporal_shards_host over numpy parts ([world, rows_max, W, c] each; ids uint32) shaped by `frame` (shard_frame(...), its
    pointers unused).  history and the returned dict as unit_temporal_host's: everything in image order, num_rows x W."""
    hdr = np.ascontiguousarray(hdr, dtype=np.float32)
    sq = None if sq is None else np.ascontiguousarray(sq, dtype=np.float32)
    feat8 = np.ascontiguousarray(feat8, dtype=np.float32)
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    W, rows, world, rows_max, block_rows = frame.parts.W, frame.parts.rs.num_rows, frame.parts.rs.nshards, frame.parts.rows_max, frame.parts.rs.block_rows
    px = world * rows_max * W
    assert hdr.size == px * 3 and (sq is None or sq.size == px * 3) and feat8.size == px * 8 and ids.size == px
    out = {"rgb": np.zeros((rows, W, 3), np.float32), "var": np.zeros((rows, W), np.float32), "state": np.zeros((rows, W, 4), np.float32),
           "guides": np.zeros((rows, W, 8), np.float32), "len": np.zeros((rows, W), np.uint32), "target": np.zeros((rows, W), np.uint32)}
    if history is None:
        hc, hs, hg, hi, hl = None, None, None, None, None
    else:
        hc = C.byref(RtCamera.from_buffer_copy(bytes(history["camera"])))
        keep = [np.ascontiguousarray(history["state"], dtype=np.float32), np.ascontiguousarray(history["guides"], dtype=np.float32),
                np.ascontiguousarray(history["ids"], dtype=np.uint32), np.ascontiguousarray(history["len"], dtype=np.uint32)]
        assert keep[0].size == rows * W * 4 and keep[1].size == rows * W * 8 and keep[2].size == rows * W and keep[3].size == rows * W
        hs, hg, hi, hl = (a.ctypes.data for a in keep)
    head = (hdr.ctypes.data, sq.ctypes.data if sq is not None else None, feat8.ctypes.data, ids.ctypes.data, C.byref(frame), hc, hs, hg, hi, hl,
            C.byref(params) if params is not None else None, C.byref(tparams) if tparams is not None else None, int(fetch))
    tail = (out["rgb"].ctypes.data, out["var"].ctypes.data, out["state"].ctypes.data, out["guides"].ctypes.data, out["len"].ctypes.data,
            out["target"].ctypes.data)
    if _entry is None:
        check(load().rt_unit_temporal_shards_host(*head, *tail))
    else:
        check(load().rt_unit_temporal_shards_variance_host(*head, C.byref(variance) if variance is not None else None, *tail))
    # the new history's ids: the parts' ids in image order (block b of the range is block b // world of part b % world)
    j = np.arange(rows)
    b = j // block_rows
    out["ids"] = ids.reshape(world, rows_max, W)[b % world, (b // world) * block_rows + j % block_rows].copy()
    out["camera"] = RtCamera.from_buffer_copy(bytes(frame.camera))
    return out


def whole_image(H):
    return RtRowset(0, H, H, 0, 1)


BLOCK_ROWS = 1  # rows per block of the cyclic partition (distributed.py says why single rows)


def cyclic_rows(H, rank, world, block_rows=BLOCK_ROWS):
    """Row blocks b = rank (mod world) of block_rows rows."""
    return RtRowset(0, H, block_rows, rank, world)
