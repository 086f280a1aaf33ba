"""raymarchrenderer_amd — MI355X-native (gfx950) SDF ray-march path tracer.

The hot path of TheBinaryCodeX/RayMarchRenderer (RayMarch.glsl / RayMarch2.glsl / RayMarch3.glsl)
as HIP kernels behind a C ABI (include/rmr.h, librmr.so), with Python front-ends that mirror the
reference's Graphics / Camera / Screen host interfaces.
"""
from . import abi
from ._lib import RMRError, lib
from .renderer import (Camera, Graphics, Renderer, Screen, adaptive_select, aov_fold, aov_init, aov_resolve, bloom_pixels, camera_frame, camera_view,
                       check_bloom_params, check_volume, srgb8, check_bake_params, check_probe_params, sh_basis, probe_fold,
                       probe_irradiance_host, save_probes, load_probes, probe_vis_dirs, probe_vis_fold, probe_irradiance_vis_host, bake_check_points, bake_fold, encode_obj, encode_ply, quads_to_triangles, surface_nets,
                       check_camera_model, check_rays, check_temporal_params, check_tonemap_params, default_camera_view,
                       encode_bmp, encode_pfm, exposure_from_histogram, luminance_bins, parity_schedule, save_name,
                       temporal_view_inverse, tile_spiral, time_schedule, tonemap_pixels)

__all__ = ["abi", "lib", "RMRError", "Renderer", "Graphics", "Camera", "Screen", "camera_view",
           "default_camera_view", "encode_bmp", "encode_pfm", "tile_spiral", "time_schedule", "parity_schedule",
           "save_name", "adaptive_select", "camera_frame", "check_camera_model", "check_rays",
           "check_temporal_params", "temporal_view_inverse", "check_tonemap_params", "luminance_bins",
           "exposure_from_histogram", "tonemap_pixels", "check_bloom_params", "bloom_pixels", "aov_fold", "aov_resolve",
           "aov_init", "check_volume", "surface_nets", "encode_obj", "encode_ply", "quads_to_triangles",
           "srgb8", "check_bake_params", "bake_check_points", "bake_fold",
           "check_probe_params", "sh_basis", "probe_fold", "probe_irradiance_host", "save_probes", "load_probes",
           "probe_vis_dirs", "probe_vis_fold", "probe_irradiance_vis_host"]
