"""ctypes binding of librmr.so (the C ABI in include/rmr.h).

librmr.so is built in-tree by raymarchrenderer_amd/csrc/Makefile (``__graft_entry__.build()``).
There is no fallback: if the library is missing, every entry point raises.
"""
import ctypes as C
import os

from . import abi

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "librmr.so")
# the diagnostic build (csrc/Makefile `diag`, -DRMR_DIAG=1): the same library plus the experiments'
# environment switches (RMR_GRID, RMR_JIT_OPTS, ...), for tools/ and the A/B tests
LIB_DIAG_PATH = os.path.join(HERE, "librmr_diag.so")
_libs = {}

EXPORTS = [
    "rmr_create", "rmr_destroy", "rmr_last_error", "rmr_build_info", "rmr_set_stream",
    "rmr_set_image_size", "rmr_get_image_size", "rmr_set_params", "rmr_get_params",
    "rmr_default_params", "rmr_set_view", "rmr_camera_view", "rmr_load_scene_json",
    "rmr_load_scene_tables", "rmr_load_builtin_scene", "rmr_reload", "rmr_render",
    "rmr_render_spp", "rmr_render_tiles", "rmr_read_accum", "rmr_write_accum",
    "rmr_accum_device_ptr", "rmr_bind_accum", "rmr_save_bmp", "rmr_encode_bmp",
    "rmr_save_accum", "rmr_load_accum", "rmr_sync", "rmr_get_stats", "rmr_reset_stats", "rmr_get_section_cycles", "rmr_get_counters", "rmr_get_counters_n", "rmr_set_culling",
    "rmr_set_kernel", "rmr_set_tuning", "rmr_set_grid_reserve", "rmr_set_trail_steps", "rmr_set_trail_tuning", "rmr_trace_samples", "rmr_abi_sizes", "rmr_set_jit", "rmr_set_instrument", "rmr_jit_compile_scene", "rmr_set_env_map",
    "rmr_scene_compile", "rmr_scene_view", "rmr_scene_free", "rmr_display", "rmr_display_device",
    "rmr_srgb_thresholds", "rmr_candidate_grid", "rmr_set_call_batching", "rmr_set_launch_streams", "rmr_get_launch_streams",
    "rmr_default_denoise_params", "rmr_render_guides", "rmr_read_guide", "rmr_guide_device_ptr", "rmr_denoise",
    "rmr_read_denoised", "rmr_denoised_device_ptr", "rmr_set_output_source", "rmr_encode_pfm",
    "rmr_set_error_estimate", "rmr_read_half_accum", "rmr_half_device_ptr", "rmr_tile_error", "rmr_tile_error_images",
    "rmr_default_adaptive_params", "rmr_check_adaptive_params", "rmr_render_adaptive", "rmr_read_sample_counts",
    "rmr_adaptive_select",
    "rmr_default_camera_model", "rmr_check_camera_model", "rmr_set_camera_model", "rmr_get_camera_model",
    "rmr_camera_frame", "rmr_check_rays", "rmr_trace_rays", "rmr_camera_rays", "rmr_jit_compile_scene_rays",
    "rmr_cast_rays", "rmr_eval_map", "rmr_trace_rays_device", "rmr_cast_rays_device", "rmr_eval_map_device",
    "rmr_query_rejects", "rmr_set_query_grid",
    "rmr_default_variance_params", "rmr_check_variance_params", "rmr_denoise_variance", "rmr_read_variance",
    "rmr_variance_device_ptr", "rmr_denoise_variance_images",
    "rmr_default_temporal_params", "rmr_check_temporal_params", "rmr_temporal_view_inverse", "rmr_temporal_accumulate",
    "rmr_temporal_reset", "rmr_read_temporal", "rmr_read_temporal_count", "rmr_temporal_device_ptr", "rmr_temporal_images",
    "rmr_default_tonemap_params", "rmr_check_tonemap_params", "rmr_tonemap", "rmr_read_tonemapped",
    "rmr_tonemapped_device_ptr", "rmr_read_exposure", "rmr_luminance_histogram", "rmr_tonemap_reset",
    "rmr_luminance_bins", "rmr_exposure_from_histogram", "rmr_tonemap_pixels",
    "rmr_default_bloom_params", "rmr_check_bloom_params", "rmr_bloom", "rmr_read_bloom", "rmr_bloom_device_ptr",
    "rmr_bloom_pixels",
    "rmr_render_aov", "rmr_aov_reset", "rmr_read_aov", "rmr_read_aov_resolved", "rmr_aov_device_ptr",
    "rmr_aov_resolved_device_ptr", "rmr_set_aov_launch_samples", "rmr_aov_init", "rmr_aov_fold", "rmr_aov_resolve",
    "rmr_check_volume", "rmr_sample_volume", "rmr_sample_volume_device", "rmr_extract_mesh", "rmr_read_mesh",
    "rmr_mesh_device_ptr", "rmr_mesh_free", "rmr_surface_nets", "rmr_encode_obj", "rmr_encode_ply",
    "rmr_default_bake_params", "rmr_check_bake_params", "rmr_bake_check_points", "rmr_bake_fold", "rmr_srgb8_pixels",
    "rmr_encode_ply_colors", "rmr_bake_points", "rmr_bake_points_device", "rmr_bake_rays_device", "rmr_bake_mesh",
    "rmr_read_mesh_bake", "rmr_mesh_bake_device_ptr",
    "rmr_default_probe_params", "rmr_check_probe_params", "rmr_sh_basis", "rmr_probe_fold", "rmr_probe_irradiance_host",
    "rmr_probe_rays_device", "rmr_bake_probes", "rmr_bake_probes_device", "rmr_bake_probe_field", "rmr_write_probe_field",
    "rmr_read_probe_field", "rmr_probe_field_device_ptr", "rmr_probe_field_free", "rmr_probe_irradiance",
    "rmr_probe_irradiance_device",
    "rmr_probe_vis_dirs", "rmr_probe_vis_fold", "rmr_probe_irradiance_vis_host", "rmr_bake_probe_visibility",
    "rmr_bake_probe_visibility_device", "rmr_bake_probe_field_visibility", "rmr_write_probe_field_visibility",
    "rmr_read_probe_field_visibility", "rmr_probe_field_visibility_device_ptr", "rmr_probe_irradiance_vis",
    "rmr_probe_irradiance_vis_device",
]


class RMRError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s (%d): %s" % (abi.ERRORS.get(code, "RMR_E?"), code, msg))
        self.code = code


def build():
    import subprocess
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "csrc"), "-j8"])


def lib(diag=None):
    """The ctypes handle of librmr.so, or of librmr_diag.so with diag=True, or of the library file
    diag names (a str: another build of the same ABI, for same-process A/B runs). diag=None: the release
    library unless the environment selects the diagnostic one with RMR_LIB=diag (tools/ scripts;
    the selection is made here, in Python: the release library itself reads no such switch)."""
    if diag is None:
        diag = os.environ.get("RMR_LIB", "") == "diag"
    if isinstance(diag, str):   # a library file (tools/abrun.py: another build of the same ABI)
        path = os.path.abspath(diag)
    else:
        path = LIB_DIAG_PATH if diag else LIB_PATH
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise RuntimeError("%s not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(expected at %s)" % (os.path.basename(path), path))
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64, and once librmr has brought
    # in /opt/rocm's, torch can no longer initialise the GPU ("No HIP GPUs are available", measured on
    # the MI355X box). Loading torch first makes librmr bind to the runtime already in the process, so
    # torch tensors and rmr contexts can share one device (FrameRenderer, rmr_bind_accum).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(path)
    vp, fp, ip = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int)
    dp = C.POINTER(C.c_double)
    sig = {
        "rmr_create": (C.c_int, [C.POINTER(vp), C.c_int]),
        "rmr_destroy": (None, [vp]),
        "rmr_last_error": (C.c_char_p, [vp]),
        "rmr_build_info": (C.c_char_p, []),
        "rmr_set_stream": (C.c_int, [vp, vp]),
        "rmr_set_image_size": (C.c_int, [vp, C.c_int, C.c_int]),
        "rmr_get_image_size": (C.c_int, [vp, ip, ip]),
        "rmr_set_params": (C.c_int, [vp, C.POINTER(abi.Params)]),
        "rmr_get_params": (C.c_int, [vp, C.POINTER(abi.Params)]),
        "rmr_default_params": (None, [C.POINTER(abi.Params)]),
        "rmr_set_view": (C.c_int, [vp, fp, fp, fp, fp, fp]),
        "rmr_camera_view": (None, [dp, dp, C.c_float, C.c_float, fp, fp, fp, fp, fp]),
        "rmr_load_scene_json": (C.c_int, [vp, C.c_int, C.c_char_p, C.c_size_t]),
        "rmr_load_scene_tables": (C.c_int, [vp, C.POINTER(abi.Scene)]),
        "rmr_load_builtin_scene": (C.c_int, [vp, C.c_int]),
        "rmr_reload": (C.c_int, [vp]),
        "rmr_render": (C.c_int, [vp, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_uint32]),
        "rmr_render_spp": (C.c_int, [vp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32]),
        "rmr_render_tiles": (C.c_int, [vp, fp, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_uint32, C.c_uint32]),
        "rmr_read_accum": (C.c_int, [vp, fp, C.c_size_t]),
        "rmr_write_accum": (C.c_int, [vp, fp, C.c_size_t]),
        "rmr_accum_device_ptr": (vp, [vp]),
        "rmr_bind_accum": (C.c_int, [vp, vp, C.c_size_t]),
        "rmr_save_bmp": (C.c_int, [vp, C.c_char_p]),
        "rmr_encode_bmp": (C.c_int, [fp, C.c_int, C.c_int, C.c_char_p]),
        "rmr_save_accum": (C.c_int, [vp, C.c_char_p, C.c_uint32]),
        "rmr_load_accum": (C.c_int, [vp, C.c_char_p, C.POINTER(C.c_uint32)]),
        "rmr_sync": (C.c_int, [vp]),
        "rmr_get_stats": (C.c_int, [vp, C.POINTER(abi.Stats)]),
        "rmr_reset_stats": (C.c_int, [vp]),
        "rmr_get_section_cycles": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
        "rmr_get_counters": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
        "rmr_get_counters_n": (C.c_int, [vp, C.POINTER(C.c_uint64), C.c_int]),
        "rmr_set_culling": (C.c_int, [vp, C.c_int]),
        "rmr_set_kernel": (C.c_int, [vp, C.c_int]),
        "rmr_set_tuning": (C.c_int, [vp, C.c_int, C.c_int, C.c_longlong]),
        "rmr_set_grid_reserve": (C.c_int, [vp, C.c_int]),
        "rmr_set_trail_steps": (C.c_int, [vp, C.c_int]),
        "rmr_set_trail_tuning": (C.c_int, [vp, C.c_int, C.c_int, C.c_int]),
        "rmr_set_call_batching": (C.c_int, [vp, C.c_int]),
        "rmr_set_launch_streams": (C.c_int, [vp, C.c_int]),
        "rmr_get_launch_streams": (C.c_int, [vp]),
        "rmr_set_jit": (C.c_int, [vp, C.c_int]),
        "rmr_set_instrument": (C.c_int, [vp, C.c_int]),
        "rmr_set_env_map": (C.c_int, [vp, C.c_void_p, C.c_int, C.c_int]),
        "rmr_jit_compile_scene": (C.c_int, [C.c_int, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]),
        "rmr_trace_samples": (C.c_int, [vp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, fp]),
        "rmr_abi_sizes": (C.c_int, [C.POINTER(C.c_int32), C.c_int]),
        "rmr_scene_compile": (C.c_int, [C.c_int, C.c_char_p, C.c_size_t, C.POINTER(vp), C.c_char_p, C.c_size_t]),
        "rmr_scene_view": (C.c_int, [vp, C.POINTER(abi.Scene)]),
        "rmr_scene_free": (None, [vp]),
        "rmr_display": (C.c_int, [vp] + [C.c_float] * 7 + [C.c_int, C.c_int, C.c_void_p, C.c_size_t]),
        "rmr_display_device": (C.c_int, [vp] + [C.c_float] * 7 + [C.c_int, C.c_int, C.c_void_p, C.c_size_t]),
        "rmr_srgb_thresholds": (C.c_int, [fp]),
        "rmr_candidate_grid": (C.c_int, [fp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double,
                                         C.POINTER(C.c_int32), fp, C.POINTER(C.c_uint32), C.c_size_t,
                                         C.POINTER(C.c_uint16), C.c_size_t]),
        "rmr_default_denoise_params": (None, [C.POINTER(abi.DenoiseParams)]),
        "rmr_render_guides": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int]),
        "rmr_read_guide": (C.c_int, [vp, C.c_int, fp, C.c_size_t]),
        "rmr_guide_device_ptr": (vp, [vp, C.c_int]),
        "rmr_denoise": (C.c_int, [vp, C.POINTER(abi.DenoiseParams)]),
        "rmr_read_denoised": (C.c_int, [vp, fp, C.c_size_t]),
        "rmr_denoised_device_ptr": (vp, [vp]),
        "rmr_set_output_source": (C.c_int, [vp, C.c_int]),
        "rmr_encode_pfm": (C.c_int, [fp, C.c_int, C.c_int, C.c_char_p]),
        "rmr_set_error_estimate": (C.c_int, [vp, C.c_int]),
        "rmr_read_half_accum": (C.c_int, [vp, fp, C.c_size_t]),
        "rmr_half_device_ptr": (vp, [vp]),
        "rmr_tile_error": (C.c_int, [vp, C.c_float, fp, C.c_size_t]),
        "rmr_tile_error_images": (C.c_int, [vp, fp, fp, C.c_int, C.c_int, C.c_float, fp]),
        "rmr_default_adaptive_params": (None, [C.POINTER(abi.AdaptiveParams)]),
        "rmr_check_adaptive_params": (C.c_int, [C.POINTER(abi.AdaptiveParams)]),
        "rmr_render_adaptive": (C.c_int, [vp, fp, C.POINTER(abi.AdaptiveParams), C.POINTER(abi.AdaptiveResult)]),
        "rmr_read_sample_counts": (C.c_int, [vp, C.POINTER(C.c_uint32), C.c_size_t]),
        "rmr_adaptive_select": (C.c_int, [fp, C.c_int, C.c_int, C.c_int, C.c_float, C.POINTER(C.c_uint8)]),
        "rmr_default_camera_model": (None, [C.POINTER(abi.CameraModel)]),
        "rmr_check_camera_model": (C.c_int, [C.POINTER(abi.CameraModel)]),
        "rmr_set_camera_model": (C.c_int, [vp, C.POINTER(abi.CameraModel)]),
        "rmr_get_camera_model": (C.c_int, [vp, C.POINTER(abi.CameraModel)]),
        "rmr_camera_frame": (C.c_int, [fp, fp]),
        "rmr_check_rays": (C.c_int, [C.c_void_p, C.c_size_t]),
        "rmr_trace_rays": (C.c_int, [vp, C.c_void_p, C.c_size_t, fp]),
        "rmr_camera_rays": (C.c_int, [vp, fp, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
        "rmr_jit_compile_scene_rays": (C.c_int, [C.c_int, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]),
        "rmr_cast_rays": (C.c_int, [vp, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
        "rmr_eval_map": (C.c_int, [vp, fp, C.c_size_t, fp]),
        "rmr_trace_rays_device": (C.c_int, [vp, C.c_void_p, C.c_size_t, C.c_float, C.c_void_p]),
        "rmr_cast_rays_device": (C.c_int, [vp, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
        "rmr_eval_map_device": (C.c_int, [vp, C.c_void_p, C.c_size_t, C.c_void_p]),
        "rmr_query_rejects": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
        "rmr_set_query_grid": (C.c_int, [vp, C.c_int]),
        "rmr_default_variance_params": (None, [C.POINTER(abi.VarianceParams)]),
        "rmr_check_variance_params": (C.c_int, [C.POINTER(abi.VarianceParams)]),
        "rmr_denoise_variance": (C.c_int, [vp, C.POINTER(abi.DenoiseParams), C.POINTER(abi.VarianceParams)]),
        "rmr_read_variance": (C.c_int, [vp, C.c_int, fp, C.c_size_t]),
        "rmr_variance_device_ptr": (vp, [vp, C.c_int]),
        "rmr_denoise_variance_images": (C.c_int, [vp, fp, fp, fp, fp, C.c_int, C.c_int, C.POINTER(abi.DenoiseParams),
                                                  C.POINTER(abi.VarianceParams), fp, fp, fp]),
        "rmr_default_temporal_params": (None, [C.POINTER(abi.TemporalParams)]),
        "rmr_check_temporal_params": (C.c_int, [C.POINTER(abi.TemporalParams)]),
        "rmr_temporal_view_inverse": (C.c_int, [fp, dp]),
        "rmr_temporal_accumulate": (C.c_int, [vp, C.c_int, C.c_float, C.POINTER(abi.TemporalParams)]),
        "rmr_temporal_reset": (C.c_int, [vp]),
        "rmr_read_temporal": (C.c_int, [vp, fp, C.c_size_t]),
        "rmr_read_temporal_count": (C.c_int, [vp, fp, C.c_size_t]),
        "rmr_temporal_device_ptr": (vp, [vp]),
        "rmr_temporal_images": (C.c_int, [vp, fp, fp, fp, fp, fp, fp, fp, fp, fp, C.c_int, C.c_int, C.c_float,
                                          C.POINTER(abi.TemporalParams), fp, fp, fp]),
        "rmr_default_tonemap_params": (None, [C.POINTER(abi.TonemapParams)]),
        "rmr_check_tonemap_params": (C.c_int, [C.POINTER(abi.TonemapParams)]),
        "rmr_tonemap": (C.c_int, [vp, C.c_int, C.POINTER(abi.TonemapParams)]),
        "rmr_read_tonemapped": (C.c_int, [vp, fp, C.c_size_t]),
        "rmr_tonemapped_device_ptr": (vp, [vp]),
        "rmr_read_exposure": (C.c_int, [vp, dp, fp]),
        "rmr_luminance_histogram": (C.c_int, [vp, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
        "rmr_tonemap_reset": (C.c_int, [vp]),
        "rmr_luminance_bins": (C.c_int, [fp, C.c_size_t, C.POINTER(C.c_int32)]),
        "rmr_exposure_from_histogram": (C.c_int, [C.POINTER(C.c_uint32), C.POINTER(abi.TonemapParams), C.c_double, dp]),
        "rmr_tonemap_pixels": (C.c_int, [C.POINTER(abi.TonemapParams), C.c_float, fp, C.c_size_t, fp]),
        "rmr_default_bloom_params": (None, [C.POINTER(abi.BloomParams)]),
        "rmr_check_bloom_params": (C.c_int, [C.POINTER(abi.BloomParams)]),
        "rmr_bloom": (C.c_int, [vp, C.c_int, C.POINTER(abi.BloomParams)]),
        "rmr_read_bloom": (C.c_int, [vp, fp, C.c_size_t]),
        "rmr_bloom_device_ptr": (vp, [vp]),
        "rmr_bloom_pixels": (C.c_int, [C.POINTER(abi.BloomParams), fp, C.c_int, C.c_int, fp]),
        "rmr_render_aov": (C.c_int, [vp, fp, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
        "rmr_aov_reset": (C.c_int, [vp]),
        "rmr_read_aov": (C.c_int, [vp, C.c_int, fp, C.c_size_t]),
        "rmr_read_aov_resolved": (C.c_int, [vp, C.c_int, fp, C.c_size_t]),
        "rmr_aov_device_ptr": (vp, [vp, C.c_int]),
        "rmr_aov_resolved_device_ptr": (vp, [vp, C.c_int]),
        "rmr_set_aov_launch_samples": (C.c_int, [vp, C.c_int]),
        "rmr_aov_init": (C.c_int, [fp, C.c_size_t]),
        "rmr_aov_fold": (C.c_int, [fp, C.c_void_p, C.c_size_t, C.c_uint32]),
        "rmr_aov_resolve": (C.c_int, [fp, C.c_size_t, C.c_float, fp]),
        "rmr_check_volume": (C.c_int, [C.POINTER(abi.VolumeDesc), C.POINTER(C.c_char_p)]),
        "rmr_sample_volume": (C.c_int, [vp, C.POINTER(abi.VolumeDesc), fp, fp]),
        "rmr_sample_volume_device": (C.c_int, [vp, C.POINTER(abi.VolumeDesc), C.c_void_p, C.c_void_p]),
        "rmr_extract_mesh": (C.c_int, [vp, C.POINTER(abi.VolumeDesc), C.POINTER(abi.MeshParams), C.POINTER(abi.MeshInfo)]),
        "rmr_read_mesh": (C.c_int, [vp, fp, fp, fp, C.POINTER(C.c_uint32)]),
        "rmr_mesh_device_ptr": (vp, [vp, C.c_int]),
        "rmr_mesh_free": (C.c_int, [vp]),
        "rmr_surface_nets": (C.c_int, [fp, C.POINTER(abi.VolumeDesc), C.c_float, fp, C.c_size_t, C.POINTER(C.c_uint32),
                                       C.c_size_t, C.POINTER(abi.MeshInfo)]),
        "rmr_encode_obj": (C.c_int, [C.c_char_p, fp, fp, C.c_size_t, C.POINTER(C.c_uint32), C.c_size_t]),
        "rmr_encode_ply": (C.c_int, [C.c_char_p, fp, fp, fp, C.c_size_t, C.POINTER(C.c_uint32), C.c_size_t]),
        "rmr_default_bake_params": (None, [C.POINTER(abi.BakeParams)]),
        "rmr_check_bake_params": (C.c_int, [C.POINTER(abi.BakeParams)]),
        "rmr_bake_check_points": (C.c_int, [fp, fp, C.c_size_t, C.POINTER(C.c_size_t)]),
        "rmr_bake_fold": (C.c_int, [fp, fp, fp, C.c_size_t, C.c_uint32, fp, fp]),
        "rmr_srgb8_pixels": (C.c_int, [fp, C.c_size_t, C.POINTER(C.c_uint8)]),
        "rmr_encode_ply_colors": (C.c_int, [C.c_char_p, fp, fp, fp, C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_uint32),
                                            C.c_size_t]),
        "rmr_bake_points": (C.c_int, [vp, fp, fp, C.c_size_t, fp, C.c_uint32, C.POINTER(abi.BakeParams), fp, fp]),
        "rmr_bake_points_device": (C.c_int, [vp, C.c_void_p, C.c_void_p, C.c_size_t, fp, C.c_uint32,
                                             C.POINTER(abi.BakeParams), C.c_void_p, C.c_void_p]),
        "rmr_bake_rays_device": (C.c_int, [vp, C.c_void_p, C.c_void_p, C.c_size_t, fp, C.c_uint32,
                                           C.POINTER(abi.BakeParams), C.c_void_p]),
        "rmr_bake_mesh": (C.c_int, [vp, fp, C.c_uint32, C.POINTER(abi.BakeParams)]),
        "rmr_read_mesh_bake": (C.c_int, [vp, fp, fp]),
        "rmr_mesh_bake_device_ptr": (vp, [vp, C.c_int]),
        "rmr_default_probe_params": (None, [C.POINTER(abi.ProbeParams)]),
        "rmr_check_probe_params": (C.c_int, [C.POINTER(abi.ProbeParams)]),
        "rmr_sh_basis": (C.c_int, [fp, C.c_size_t, fp]),
        "rmr_probe_fold": (C.c_int, [fp, fp, C.c_size_t, C.c_uint32, fp]),
        "rmr_probe_irradiance_host": (C.c_int, [C.POINTER(abi.VolumeDesc), fp, fp, fp, C.c_size_t, fp, C.POINTER(C.c_size_t)]),
        "rmr_probe_rays_device": (C.c_int, [vp, C.c_void_p, C.c_size_t, fp, C.c_uint32, C.POINTER(abi.ProbeParams), C.c_void_p]),
        "rmr_bake_probes": (C.c_int, [vp, fp, C.c_size_t, fp, C.c_uint32, C.POINTER(abi.ProbeParams), fp]),
        "rmr_bake_probes_device": (C.c_int, [vp, C.c_void_p, C.c_size_t, fp, C.c_uint32, C.POINTER(abi.ProbeParams),
                                             C.c_void_p]),
        "rmr_bake_probe_field": (C.c_int, [vp, C.POINTER(abi.VolumeDesc), fp, C.c_uint32, C.POINTER(abi.ProbeParams)]),
        "rmr_write_probe_field": (C.c_int, [vp, C.POINTER(abi.VolumeDesc), fp]),
        "rmr_read_probe_field": (C.c_int, [vp, C.POINTER(abi.VolumeDesc), fp]),
        "rmr_probe_field_device_ptr": (vp, [vp]),
        "rmr_probe_field_free": (C.c_int, [vp]),
        "rmr_probe_irradiance": (C.c_int, [vp, fp, fp, C.c_size_t, fp]),
        "rmr_probe_irradiance_device": (C.c_int, [vp, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
        "rmr_probe_vis_dirs": (C.c_int, [fp]),
        "rmr_probe_vis_fold": (C.c_int, [fp, C.c_size_t, C.c_uint32, C.c_float, fp]),
        "rmr_probe_irradiance_vis_host": (C.c_int, [C.POINTER(abi.VolumeDesc), fp, fp, fp, fp, C.c_size_t, C.c_float, fp,
                                                    C.POINTER(C.c_size_t)]),
        "rmr_bake_probe_visibility": (C.c_int, [vp, fp, C.c_size_t, fp, C.c_uint32, C.POINTER(abi.ProbeParams), C.c_float, fp]),
        "rmr_bake_probe_visibility_device": (C.c_int, [vp, C.c_void_p, C.c_size_t, fp, C.c_uint32, C.POINTER(abi.ProbeParams),
                                                       C.c_float, C.c_void_p]),
        "rmr_bake_probe_field_visibility": (C.c_int, [vp, fp, C.c_uint32, C.c_float]),
        "rmr_write_probe_field_visibility": (C.c_int, [vp, fp, C.c_float]),
        "rmr_read_probe_field_visibility": (C.c_int, [vp, fp, fp]),
        "rmr_probe_field_visibility_device_ptr": (vp, [vp]),
        "rmr_probe_irradiance_vis": (C.c_int, [vp, fp, fp, C.c_size_t, C.c_float, fp]),
        "rmr_probe_irradiance_vis_device": (C.c_int, [vp, C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_void_p]),
        "rmr_diag_probe_fold": (C.c_int, [vp, C.c_int]),
        "rmr_diag_bake_kernels": (C.c_int, [vp, C.c_void_p, C.c_void_p, C.c_size_t, fp, C.c_uint32,
                                            C.POINTER(abi.BakeParams), C.c_void_p]),
        "rmr_diag_bloom_tail": (C.c_int, [vp, C.c_int]),
        "rmr_diag_bloom_time": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, fp]),
        "rmr_diag_tonemap_fold": (C.c_int, [vp, C.c_int]),
        "rmr_diag_tonemap_time": (C.c_int, [vp, C.c_int, C.c_int, fp]),
        # diagnostic library only (rmr_api.cpp RMR_DIAG): ray_exit at given rays; the a-trous passes
        # that run the LDS-tiled form
        "rmr_diag_ray_exit": (C.c_int, [vp, fp, C.c_int, fp, fp, C.c_int, ip]),
        "rmr_diag_denoise_tiled": (C.c_int, [vp, C.c_int]),
        "rmr_diag_temporal_keep": (C.c_int, [vp, C.c_int]),
    }
    for name, (res, args) in sig.items():
        if not hasattr(L, name):   # (an older build given by path may lack a newer entry point)
            continue
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _libs[path] = L
    return L
