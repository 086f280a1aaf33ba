"""Python front-end of librmr.so: a Renderer context plus the reference's host interfaces.

`Renderer` owns one rmr_ctx (one GPU). `Graphics`, `Camera` and `Screen` mirror the reference's
static host classes (Graphics.h:15-134, Camera.h:4-32, Screen.h:4-15) with the same member names
and argument meaning, so driver code written against the reference reads the same here.
"""
import ctypes as C
import json
import math
import os
import time as _time

import numpy as np

from . import abi
from ._lib import RMRError, lib


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _check(ctx, code, L=None):
    if code != abi.RMR_OK:
        msg = (L or lib()).rmr_last_error(ctx) if ctx else b""
        raise RMRError(code, (msg or b"").decode(errors="replace"))


def time_schedule(nspp, frame=0, first_sample=0):
    """Seed schedule of SURVEY §8d: time(frame f, sample s) = 1000*f + 0.016*s (as float32)."""
    s = np.arange(first_sample, first_sample + nspp, dtype=np.float64)
    return (1000.0 * frame + 0.016 * s).astype(np.float32)


def parity_schedule(nspp):
    """Seed schedule for converged-parity checks: time(s) = s * 0.016 / 256 (float32).

    The reference hash rand() (RayMarch.glsl:43-57) feeds dot(co, (12.9898, 78.233)), co ~ pixel +
    time, through mod(., 3.14) in float32: once |dot| reaches ~1e4-1e5 the argument of sin() is
    quantised to a few hundred values and the stream's distribution starts to depend on the
    driver's sin() rounding (measured: +8.7% Cornell-5 mean between two implementations at
    time ~ 4000). Small, densely spaced seeds keep both implementations in the well-conditioned
    regime, so their converged images are comparable."""
    s = np.arange(nspp, dtype=np.float64)
    return (s * (0.016 / 256.0)).astype(np.float32)


def camera_view(eye, direction, aspect, fov):
    """Camera::calculateRays + setView swap (librmr's rmr_camera_view): 15 floats in shader order."""
    e = (C.c_double * 3)(*[float(x) for x in eye])
    d = (C.c_double * 3)(*[float(x) for x in direction])
    out = np.zeros(15, np.float32)
    p = out.ctypes.data
    fsz = 4
    lib().rmr_camera_view(e, d, C.c_float(aspect), C.c_float(fov),
                          *[C.cast(p + 3 * i * fsz, C.POINTER(C.c_float)) for i in range(5)])
    return out


def default_camera_view(W, H):
    """Program.cpp:102 camera for an image of W x H."""
    m = math.sqrt(0.0 + 9.0 + 36.0)
    pi = np.float32(3.141592653)
    return camera_view((0.0, 4.0, -6.0), (0.0, -3.0 / m, 6.0 / m), float(W) / float(H), float(pi / np.float32(4)))


class Renderer:
    """One rmr context on one GPU (device index `device`)."""

    def __init__(self, device=0, width=1024, height=1024, diag=None):
        """diag=True: the context lives in the diagnostic build librmr_diag.so, which also reads the
        experiments' environment switches (RMR_GRID, RMR_JIT_OPTS, ...; tools/, A/B tests); the
        release librmr.so reads none. None: the release library unless RMR_LIB=diag (tools/)."""
        self._L = lib(diag=diag)
        self._ctx = C.c_void_p()
        rc = self._L.rmr_create(C.byref(self._ctx), device)
        if rc != abi.RMR_OK:
            raise RMRError(rc, "rmr_create failed (no HIP device %d?)" % device)
        self._device = int(device)
        self._mesh_info = None   # (n_vertices, n_quads, normals, ids) of the last extract_mesh
        self.set_image_size(width, height)
        self.reload()
        self.variant = None

    # -- lifetime --
    def close(self):
        if self._ctx:
            self._L.rmr_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def ctx(self):
        return self._ctx

    @property
    def lib(self):
        """The ctypes library this context lives in (librmr.so, or librmr_diag.so with diag=True)."""
        return self._L

    def _chk(self, code):
        _check(self._ctx, code, self._L)

    # -- configuration --
    def set_image_size(self, w, h):
        self._chk(self._L.rmr_set_image_size(self._ctx, int(w), int(h)))

    def image_size(self):
        w, h = C.c_int(), C.c_int()
        self._chk(self._L.rmr_get_image_size(self._ctx, C.byref(w), C.byref(h)))
        return w.value, h.value

    def set_params(self, params=None, **kw):
        p = params if params is not None else abi.default_params()
        for k, v in kw.items():
            setattr(p, k, v)
        self._chk(self._L.rmr_set_params(self._ctx, C.byref(p)))

    def params(self):
        p = abi.Params()
        self._chk(self._L.rmr_get_params(self._ctx, C.byref(p)))
        return p

    def set_view(self, view15):
        v = np.ascontiguousarray(view15, np.float32).reshape(15)
        parts = [np.ascontiguousarray(v[3 * i:3 * i + 3]) for i in range(5)]
        self._chk(self._L.rmr_set_view(self._ctx, *[_fp(x) for x in parts]))
        self._view = v

    def load_scene(self, scene, variant):
        """scene: path, JSON text or dict in the reference's v1/v2 scene format."""
        if isinstance(variant, str):
            variant = abi.VARIANTS[variant]
        if isinstance(scene, dict):
            text = json.dumps(scene)
        elif isinstance(scene, str) and os.path.exists(scene):
            with open(scene, "r") as f:
                text = f.read()
        else:
            text = scene
        b = text.encode()
        self._chk(self._L.rmr_load_scene_json(self._ctx, variant, b, len(b)))
        self.variant = variant

    def load_builtin(self, variant):
        if isinstance(variant, str):
            variant = abi.VARIANTS[variant]
        self._chk(self._L.rmr_load_builtin_scene(self._ctx, variant))
        self.variant = variant

    def load_tables(self, tables):
        s = tables.to_ctypes()
        self._chk(self._L.rmr_load_scene_tables(self._ctx, C.byref(s)))
        self.variant = tables.variant

    def reload(self):
        self._chk(self._L.rmr_reload(self._ctx))

    def set_kernel(self, k):
        self._chk(self._L.rmr_set_kernel(self._ctx, int(k)))

    def set_tuning(self, shade_threshold=0, grid_per_cu=-1, samp_budget=0, park=None, slot_batch=None, lane_slots=None):
        """rmr_set_tuning. park / slot_batch / lane_slots: the lane-slot kernels' thresholds (0: the
        kernel class's) and the schedule's switch, carried in shade_threshold's upper bits (rmr.h);
        giving any of them sets all three (the others to their defaults)."""
        st = int(shade_threshold)
        if not (park is None and slot_batch is None and lane_slots is None):
            p = 127 if lane_slots is False else min(64, int(park or 0))
            st |= 1 << 23 | p << 16 | min(64, int(slot_batch or 0)) << 24
        self._chk(self._L.rmr_set_tuning(self._ctx, st, int(grid_per_cu), int(samp_budget)))

    def set_trail_steps(self, steps):
        """Trailing steps per map-loop iteration of the lane-slot kernels (rmr_set_trail_steps): a fixed 0..15,
        -1 the kernel class's own tuning; scheduling only."""
        self._chk(self._L.rmr_set_trail_steps(self._ctx, int(steps)))

    def set_trail_tuning(self, k_max, ratio_eighths=0, park_exit=False):
        """The trailing passes chosen per wave (rmr_set_trail_tuning): at most k_max (0..15) per map-loop
        iteration, another one only while the lanes taking part are ratio_eighths / 8 (0..8) of the active
        ones and, with park_exit, the finished lanes are fewer than the park threshold; scheduling only."""
        self._chk(self._L.rmr_set_trail_tuning(self._ctx, int(k_max), int(ratio_eighths), int(park_exit)))

    def set_grid_reserve(self, blocks):
        """Workgroups the persistent trace launch leaves free (rmr_set_grid_reserve; scheduling only)."""
        self._chk(self._L.rmr_set_grid_reserve(self._ctx, int(blocks)))
        self._grid_reserve = int(blocks)

    @property
    def grid_reserve(self):
        """The reserve last set through this object (0, the context's default, until then)."""
        return getattr(self, "_grid_reserve", 0)

    def set_env_map(self, rgba8):
        """envTex for skyColor (used with params use_env_tex=1): (h, w, 4) uint8, row 0 = up. None clears."""
        if rgba8 is None:
            self._chk(self._L.rmr_set_env_map(self._ctx, None, 0, 0))
            return
        a = np.ascontiguousarray(rgba8, np.uint8)
        self._env = a
        self._chk(self._L.rmr_set_env_map(self._ctx, a.ctypes.data, a.shape[1], a.shape[0]))

    def set_jit(self, mode):
        """hipRTC per-scene kernel specialisation: 0 off, 1 always, 2 auto (large launches)."""
        self._chk(self._L.rmr_set_jit(self._ctx, int(mode)))

    def set_instrument(self, flags):
        """Instrumented specialised kernels (abi.INSTR_*; rmr_set_instrument): the same images, extra
        counters (INSTR_COUNT_FLOPS: executed flops per map() in counters() [11..13])."""
        self._chk(self._L.rmr_set_instrument(self._ctx, int(flags)))

    def set_culling(self, flags):
        """Exact work-skipping switches (abi.CULL_*; results are bit-identical either way)."""
        self._chk(self._L.rmr_set_culling(self._ctx, int(flags)))

    def set_stream(self, hip_stream_handle):
        self._chk(self._L.rmr_set_stream(self._ctx, C.c_void_p(hip_stream_handle)))

    # -- rendering --
    def render(self, time, vmin, vmax, current_sample):
        """Graphics::Render(currentTime, min, max, currentSample)."""
        self._chk(self._L.rmr_render(self._ctx, float(time), float(vmin[0]), float(vmin[1]),
                                           float(vmax[0]), float(vmax[1]), int(current_sample)))

    def set_call_batching(self, mode):
        """rmr_set_call_batching: 1 on, 0 off, -1 auto (the default: on while the context owns its stream
        and accumulator). Batched render() calls go to the GPU together at the next other call."""
        self._chk(self._L.rmr_set_call_batching(self._ctx, int(mode)))

    def set_launch_streams(self, n):
        """rmr_set_launch_streams: n >= 2 (the library's default: 2, or 4 with 8 or more hardware queues)
        overlaps consecutive trace launches on n private streams (one sample-plane buffer each); 0 runs
        them on the context's stream. Same bits."""
        self._chk(self._L.rmr_set_launch_streams(self._ctx, int(n)))

    @property
    def launch_streams(self):
        """rmr_get_launch_streams: the context's launch streams (default 2, or 4 with 8 or more hardware
        queues per process)."""
        return int(self._L.rmr_get_launch_streams(self._ctx))

    def render_spp(self, times, rect=None, first_sample=0):
        times = np.ascontiguousarray(times, np.float32)
        if rect is None:
            w, h = self.image_size()
            rect = (0, 0, w, h)
        x0, y0, x1, y1 = rect
        self._chk(self._L.rmr_render_spp(self._ctx, _fp(times), x0, y0, x1, y1, int(first_sample), len(times)))

    def render_tiles(self, times, tiles_xy, tile_size, first_sample=0):
        times = np.ascontiguousarray(times, np.float32)
        t = np.ascontiguousarray(tiles_xy, np.int32).reshape(-1, 2)
        self._chk(self._L.rmr_render_tiles(self._ctx, _fp(times), t.ctypes.data_as(C.POINTER(C.c_int32)),
                                                 len(t), int(tile_size), int(first_sample), len(times)))

    def trace_samples(self, times, rect):
        times = np.ascontiguousarray(times, np.float32)
        x0, y0, x1, y1 = rect
        out = np.zeros((len(times), y1 - y0, x1 - x0, 4), np.float32)
        self._chk(self._L.rmr_trace_samples(self._ctx, _fp(times), x0, y0, x1, y1, len(times), _fp(out)))
        return out

    # -- camera models and caller-supplied rays --
    def set_camera_model(self, model=abi.CAMERA_VIEW, **fields):
        """rmr_set_camera_model: model abi.CAMERA_* or 'view' / 'thinlens' / 'equirect' / 'ortho';
        fields aperture, focus (thin lens), width, height (ortho). Survives reload()."""
        m = model if isinstance(model, abi.CameraModel) else abi.default_camera_model(model, **fields)
        self._chk(self._L.rmr_set_camera_model(self._ctx, C.byref(m)))

    def camera_model(self):
        m = abi.CameraModel()
        self._chk(self._L.rmr_get_camera_model(self._ctx, C.byref(m)))
        return m

    def camera_rays(self, times, rect=None):
        """rmr_camera_rays: the current model's rays of samples seeded `times` over the rect, a
        (len(times), h, w) structured array of abi.RAY_DTYPE (o, time, d, rc, gx, gy)."""
        times = np.ascontiguousarray(times, np.float32)
        w, h = self.image_size()
        x0, y0, x1, y1 = (int(v) for v in (rect if rect is not None else (0, 0, w, h)))
        x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, w), min(y1, h)
        out = np.zeros((len(times), max(y1 - y0, 0), max(x1 - x0, 0)), np.dtype(abi.RAY_DTYPE))
        self._chk(self._L.rmr_camera_rays(self._ctx, _fp(times), len(times), x0, y0, x1, y1, out.ctypes.data))
        return out

    def trace_rays(self, rays):
        """rmr_trace_rays: the radiance along each ray of a structured array of abi.RAY_DTYPE (any
        shape; taken in C order), (n, 4) float32 with alpha 1. The accumulator is not touched."""
        r = np.ascontiguousarray(rays, np.dtype(abi.RAY_DTYPE)).reshape(-1)
        out = np.zeros((len(r), 4), np.float32)
        self._chk(self._L.rmr_trace_rays(self._ctx, r.ctypes.data, len(r), _fp(out)))
        return out

    # -- first-hit and distance queries, device-resident lists (rmr.h) --
    def cast_rays(self, rays, normals=True):
        """rmr_cast_rays: the first hit of each ray of a structured array of abi.RAY_DTYPE (any shape;
        taken in C order), a structured array of abi.HIT_DTYPE (pos, t, n, id); id -1 marks a miss.
        normals=False: n stays zero and no probe is evaluated (visibility queries)."""
        r = np.ascontiguousarray(rays, np.dtype(abi.RAY_DTYPE)).reshape(-1)
        out = np.zeros(len(r), np.dtype(abi.HIT_DTYPE))
        self._chk(self._L.rmr_cast_rays(self._ctx, r.ctypes.data, len(r), abi.CAST_NORMALS if normals else 0,
                                        out.ctypes.data))
        return out

    def eval_map(self, points):
        """rmr_eval_map: map(p) of each point of an (..., 3) array as (n, 2) float32 (distance, id)."""
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        out = np.zeros((len(p), 2), np.float32)
        self._chk(self._L.rmr_eval_map(self._ctx, _fp(p), len(p), _fp(out)))
        return out

    @staticmethod
    def _device_rays(rays):
        """A torch CUDA tensor of rays, (n, 40) uint8 or (n, 10) float32 (views of abi.RAY_DTYPE): n."""
        import torch
        ok = (rays.is_cuda and rays.dim() == 2 and rays.is_contiguous() and
              ((rays.dtype == torch.uint8 and rays.shape[1] == 40) or (rays.dtype == torch.float32 and rays.shape[1] == 10)))
        if not ok:
            raise ValueError("device rays: a contiguous CUDA tensor, (n, 40) uint8 or (n, 10) float32 (abi.RAY_DTYPE)")
        return rays.shape[0]

    @staticmethod
    def _device_out(out, n, cols, like):
        import torch
        if out is None:
            return torch.empty((n, cols), dtype=torch.float32, device=like.device)
        if not (out.is_cuda and out.device == like.device and out.dtype == torch.float32 and out.is_contiguous() and
                tuple(out.shape) == (n, cols)):
            raise ValueError("out: a contiguous float32 CUDA tensor of shape (%d, %d) on %s" % (n, cols, like.device))
        return out

    def trace_rays_device(self, rays, origin_extent, out=None):
        """rmr_trace_rays_device: the radiance along each ray of a torch CUDA tensor (see _device_rays), an
        (n, 4) float32 tensor on the same device; queued on the context's stream (set_stream), no copy to
        the host and no sync. origin_extent: a bound on |origin coordinate| over the list. A ray the
        GPU's check rejects gives (0, 0, 0, 0) and counts in query_rejects()."""
        n = self._device_rays(rays)
        out = self._device_out(out, n, 4, rays)
        self._chk(self._L.rmr_trace_rays_device(self._ctx, rays.data_ptr(), n, float(origin_extent), out.data_ptr()))
        return out

    def cast_rays_device(self, rays, normals=True, out=None):
        """rmr_cast_rays_device: (n, 8) float32 (pos, t, n, id: abi.HIT_DTYPE) on the rays' device; a
        rejected ray gives (0, 0, 0, -1, 0, 0, 0, -2). Queued on the context's stream, no sync."""
        n = self._device_rays(rays)
        out = self._device_out(out, n, 8, rays)
        self._chk(self._L.rmr_cast_rays_device(self._ctx, rays.data_ptr(), n, abi.CAST_NORMALS if normals else 0,
                                               out.data_ptr()))
        return out

    def eval_map_device(self, points, out=None):
        """rmr_eval_map_device: map(p) of an (n, 3) float32 CUDA tensor as (n, 2) float32 (distance, id)."""
        import torch
        if not (points.is_cuda and points.dtype == torch.float32 and points.dim() == 2 and points.shape[1] == 3 and
                points.is_contiguous()):
            raise ValueError("points: a contiguous (n, 3) float32 CUDA tensor")
        n = points.shape[0]
        out = self._device_out(out, n, 2, points)
        self._chk(self._L.rmr_eval_map_device(self._ctx, points.data_ptr(), n, out.data_ptr()))
        return out

    def query_rejects(self):
        """rmr_query_rejects: rays the device forms rejected since the last call (synchronises)."""
        v = C.c_uint64(0)
        self._chk(self._L.rmr_query_rejects(self._ctx, C.byref(v)))
        return int(v.value)

    def set_query_grid(self, blocks):
        """rmr_set_query_grid: cap the cast / eval kernels' grid (0: automatic). Scheduling only."""
        self._chk(self._L.rmr_set_query_grid(self._ctx, int(blocks)))

    # -- sampled AOVs: coverage, depth, normal, position and id mattes (rmr.h) --
    def render_aov(self, times, rect=None, restart=False):
        """rmr_render_aov: fold the first hits of the samples seeded `times` (the beauty render's own
        primary rays under the current camera model) into the rect's pixels; restart=True starts the rect
        from the initial state. Queued on the context's stream, no sync."""
        times = np.ascontiguousarray(times if times is not None else [], np.float32).reshape(-1)
        if rect is None:
            w, h = self.image_size()
            rect = (0, 0, w, h)
        x0, y0, x1, y1 = (int(v) for v in rect)
        self._chk(self._L.rmr_render_aov(self._ctx, _fp(times) if len(times) else None, len(times), x0, y0, x1, y1,
                                         1 if restart else 0))

    def aov_reset(self):
        """rmr_aov_reset: the initial state everywhere."""
        self._chk(self._L.rmr_aov_reset(self._ctx))

    def set_aov_launch_samples(self, n):
        """rmr_set_aov_launch_samples: most samples per kernel launch of render_aov. Scheduling only."""
        self._chk(self._L.rmr_set_aov_launch_samples(self._ctx, int(n)))

    @staticmethod
    def _aov_plane(who, plane, names):
        if isinstance(plane, str):
            if plane not in names:
                raise ValueError("%s: unknown plane %r (%s)" % (who, plane, ", ".join(names)))
            plane = names[plane]
        return int(plane)

    def read_aov_raw(self, plane):
        """One raw state plane as (H, W, 4) float32; plane: abi.AOV_* or 'stats' / 'normal' / 'position' /
        'ids01' / 'ids23'."""
        plane = self._aov_plane("read_aov_raw", plane, abi.AOV_PLANES)
        w, h = self.image_size()
        out = np.zeros((h, w, 4), np.float32)
        self._chk(self._L.rmr_read_aov(self._ctx, plane, _fp(out), out.nbytes))
        return out

    def read_aov_resolved(self, which):
        """One resolved plane as (H, W, 4) float32; which: abi.AOV_R_* or 'depth' / 'normal' / 'position' /
        'ids01' / 'ids23'."""
        which = self._aov_plane("read_aov_resolved", which, abi.AOV_RESOLVED)
        w, h = self.image_size()
        out = np.zeros((h, w, 4), np.float32)
        self._chk(self._L.rmr_read_aov_resolved(self._ctx, which, _fp(out), out.nbytes))
        return out

    def read_aov(self):
        """The resolved AOVs as a dict of float32 arrays: alpha, depth (mean t), min_depth, samples, hits,
        other (H, W); normal, position (H, W, 3); ids and coverage (H, W, 4), the four id slots sorted by
        coverage (-1: empty)."""
        depth = self.read_aov_resolved(abi.AOV_R_DEPTH)
        nrm = self.read_aov_resolved(abi.AOV_R_NORMAL)
        pos = self.read_aov_resolved(abi.AOV_R_POSITION)
        s01, s23 = self.read_aov_resolved(abi.AOV_R_IDS01), self.read_aov_resolved(abi.AOV_R_IDS23)
        slots = np.concatenate([s01, s23], axis=2)
        return {"alpha": depth[..., 2].copy(), "depth": depth[..., 0].copy(), "min_depth": depth[..., 1].copy(),
                "normal": nrm[..., :3].copy(), "position": pos[..., :3].copy(), "samples": depth[..., 3].copy(),
                "hits": pos[..., 3].copy(), "ids": slots[..., 0::2].copy(), "coverage": slots[..., 1::2].copy(),
                "other": self.read_aov_raw(abi.AOV_NORMAL)[..., 3].copy()}

    def aov_device(self):
        """rmr_aov_resolved_device_ptr: the resolved planes as torch tensors on the context's device, a dict
        'depth' / 'normal' / 'position' / 'ids01' / 'ids23' of (H, W, 4) float32 views of the library's
        memory: no copy, no sync (the resolve is queued on the context's stream). Valid until the next
        render_aov, aov_reset, reload or scene load."""
        import torch
        w, h = self.image_size()
        out = {}
        for name, which in abi.AOV_RESOLVED.items():
            ptr = self._L.rmr_aov_resolved_device_ptr(self._ctx, which)
            if not ptr:
                raise RMRError(-5, (self._L.rmr_last_error(self._ctx) or b"").decode(errors="replace"))
            out[name] = torch.as_tensor(_DeviceArray(ptr, (h, w, 4), self), device="cuda:%d" % self._device)
        return out

    # -- SDF volume sampling and surface-nets mesh extraction (rmr.h) --
    def sample_volume(self, origin, spacing, shape, ids=False):
        """rmr_sample_volume: map() at the lattice's points origin + i * spacing, shape = (nx, ny, nz) points,
        as a float32 array indexed [iz, iy, ix]; with ids=True the pair (distances, ids)."""
        d = _volume_desc(origin, spacing, shape)
        nx, ny, nz = d.n[0], d.n[1], d.n[2]
        dist = np.zeros((nz, ny, nx), np.float32)
        idv = np.zeros((nz, ny, nx), np.float32) if ids else None
        self._chk(self._L.rmr_sample_volume(self._ctx, C.byref(d), _fp(dist), _fp(idv) if ids else None))
        return (dist, idv) if ids else dist

    def sample_volume_device(self, origin, spacing, shape, ids=False):
        """rmr_sample_volume_device: the same as torch float32 tensors [iz, iy, ix] on the context's device,
        written by the kernel (no copy); queued on the context's stream, no sync."""
        import torch
        d = _volume_desc(origin, spacing, shape)
        nx, ny, nz = d.n[0], d.n[1], d.n[2]
        dev = "cuda:%d" % self._device
        dist = torch.empty((nz, ny, nx), dtype=torch.float32, device=dev)
        idv = torch.empty((nz, ny, nx), dtype=torch.float32, device=dev) if ids else None
        self._chk(self._L.rmr_sample_volume_device(self._ctx, C.byref(d), dist.data_ptr(),
                                                   idv.data_ptr() if ids else None))
        return (dist, idv) if ids else dist

    def extract_mesh(self, origin, spacing, shape, iso=0.0, normals=True, ids=True):
        """rmr_extract_mesh + rmr_read_mesh: the surface-nets mesh of the level iso over the lattice, a dict of
        'vertices' (V, 3) float32, 'quads' (Q, 4) uint32, 'normals' (V, 3) float32 or None and 'ids' (V,)
        float32 or None. quads_to_triangles() splits the quads."""
        d = _volume_desc(origin, spacing, shape)
        mp = abi.MeshParams(float(iso), (abi.MESH_NORMALS if normals else 0) | (abi.MESH_IDS if ids else 0))
        info = abi.MeshInfo()
        self._mesh_info = None
        self._chk(self._L.rmr_extract_mesh(self._ctx, C.byref(d), C.byref(mp), C.byref(info)))
        self._mesh_info = (int(info.n_vertices), int(info.n_quads), bool(normals), bool(ids))
        return self.read_mesh(normals=normals, ids=ids)

    def read_mesh(self, normals=True, ids=True):
        """rmr_read_mesh: the last extraction's mesh (see extract_mesh)."""
        nv, nq = (self._mesh_info or (0, 0))[:2]
        v = np.zeros((nv, 3), np.float32)
        q = np.zeros((nq, 4), np.uint32)
        n = np.zeros((nv, 3), np.float32) if normals else None
        i = np.zeros((nv,), np.float32) if ids else None
        self._chk(self._L.rmr_read_mesh(self._ctx, _fp(v), _fp(n) if normals else None, _fp(i) if ids else None,
                                        q.ctypes.data_as(C.POINTER(C.c_uint32))))
        return {"vertices": v, "quads": q, "normals": n, "ids": i}

    def mesh_device(self):
        """rmr_mesh_device_ptr: the mesh as torch tensors on the context's device, views of the library's memory
        (no copy, no sync; written by work queued on the context's stream): 'vertices' (V, 3) float32, 'quads'
        (Q, 4) int32 (the uint32 indices' bits), 'normals' and 'ids' or None. Valid until the next extraction,
        mesh_free or reload."""
        import torch
        if not self._mesh_info or (self._mesh_info[0] and not self._L.rmr_mesh_device_ptr(self._ctx, abi.MESH_BUF_VERTICES)):
            raise RMRError(-5, "no mesh (call extract_mesh)")
        nv, nq, has_n, has_i = self._mesh_info
        dev = "cuda:%d" % self._device

        def view(which, shape, typestr):
            ptr = self._L.rmr_mesh_device_ptr(self._ctx, which)
            if not ptr or not shape[0]:
                return torch.empty(shape, dtype=torch.float32 if typestr == "<f4" else torch.int32, device=dev)
            a = _DeviceArray(ptr, shape, self)
            a.__cuda_array_interface__["typestr"] = typestr
            return torch.as_tensor(a, device=dev)
        return {"vertices": view(abi.MESH_BUF_VERTICES, (nv, 3), "<f4"), "quads": view(abi.MESH_BUF_QUADS, (nq, 4), "<i4"),
                "normals": view(abi.MESH_BUF_NORMALS, (nv, 3), "<f4") if has_n else None,
                "ids": view(abi.MESH_BUF_IDS, (nv,), "<f4") if has_i else None}

    def mesh_free(self):
        """rmr_mesh_free: release the mesh and the extraction's working memory."""
        self._mesh_info = None
        self._chk(self._L.rmr_mesh_free(self._ctx))

    # -- light baking at surface points and mesh vertices (rmr.h) --
    @staticmethod
    def _bake_params(params, fields):
        if params is not None and fields:
            raise ValueError("params or its fields as keywords, not both (got params and %s)" % ", ".join(sorted(fields)))
        q = abi.bake_params(**fields) if params is None else params
        if not isinstance(q, abi.BakeParams):
            raise ValueError("params: an abi.BakeParams (abi.bake_params(...))")
        return q

    def bake_points(self, points, normals, times, params=None, **fields):
        """rmr_bake_points: the light at n surface points with unit normals ((n, 3) float32 each) from the
        samples seeded `times`: a dict of 'rgba' ((n, 4) float32: irradiance / pi and the samples used) with
        the radiance flag and 'ao' ((n,) float32) with the occlusion flag, None for what was not asked for.
        params: an abi.BakeParams, or its fields as keywords (abi.bake_params: radiance, ao, bias,
        ao_distance, first_index). A rejected point (rmr.h) gives zeros and counts in query_rejects()."""
        q = self._bake_params(params, fields)
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        nn = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        if len(p) != len(nn):
            raise ValueError("one normal per point")
        t = np.ascontiguousarray(times, np.float32).reshape(-1)
        rgba = np.zeros((len(p), 4), np.float32) if q.flags & abi.BAKE_RADIANCE else None
        ao = np.zeros((len(p),), np.float32) if q.flags & abi.BAKE_AO else None
        self._chk(self._L.rmr_bake_points(self._ctx, _fp(p), _fp(nn), len(p), _fp(t) if len(t) else None, len(t), C.byref(q),
                                          _fp(rgba) if rgba is not None else None, _fp(ao) if ao is not None else None))
        return {"rgba": rgba, "ao": ao}

    @staticmethod
    def _device_points(points, normals):
        import torch
        for a in (points, normals):
            if not (a.is_cuda and a.dtype == torch.float32 and a.dim() == 2 and a.shape[1] == 3 and a.is_contiguous()):
                raise ValueError("points, normals: contiguous (n, 3) float32 CUDA tensors")
        if points.shape[0] != normals.shape[0] or points.device != normals.device:
            raise ValueError("one normal per point, on the points' device")
        return points.shape[0]

    def bake_points_device(self, points, normals, times, origin_extent, params=None, **fields):
        """rmr_bake_points_device: bake_points on torch CUDA tensors ((n, 3) float32 each), the results as
        torch tensors on the same device; queued on the context's stream (set_stream), no copy to the host
        and no sync. origin_extent: a bound on |coordinate| of every ray origin p + bias n."""
        import torch
        q = self._bake_params(params, fields)
        q = abi.BakeParams(q.flags, q.bias, q.ao_distance, float(origin_extent), q.first_index)
        n = self._device_points(points, normals)
        t = np.ascontiguousarray(times, np.float32).reshape(-1)
        rgba = torch.empty((n, 4), dtype=torch.float32, device=points.device) if q.flags & abi.BAKE_RADIANCE else None
        ao = torch.empty((n,), dtype=torch.float32, device=points.device) if q.flags & abi.BAKE_AO else None
        self._chk(self._L.rmr_bake_points_device(self._ctx, points.data_ptr(), normals.data_ptr(), n,
                                                 _fp(t) if len(t) else None, len(t), C.byref(q),
                                                 rgba.data_ptr() if rgba is not None else None,
                                                 ao.data_ptr() if ao is not None else None))
        return {"rgba": rgba, "ao": ao}

    def bake_rays_device(self, points, normals, times, params=None, **fields):
        """rmr_bake_rays_device: the rays the bake generates, a (len(times) * n, 10) float32 CUDA tensor (views
        of abi.RAY_DTYPE, ray [k * n + i] = sample k of point i) for trace_rays_device / cast_rays_device; a
        rejected point's rays carry gx = -1. Queued on the context's stream, no sync."""
        import torch
        q = self._bake_params(params, fields)
        n = self._device_points(points, normals)
        t = np.ascontiguousarray(times, np.float32).reshape(-1)
        out = torch.empty((len(t) * n, 10), dtype=torch.float32, device=points.device)
        self._chk(self._L.rmr_bake_rays_device(self._ctx, points.data_ptr(), normals.data_ptr(), n,
                                               _fp(t) if len(t) else None, len(t), C.byref(q), out.data_ptr()))
        return out

    def bake_mesh(self, times, params=None, **fields):
        """rmr_bake_mesh: bake at the last extraction's vertices and normals into buffers that live with the
        mesh (read_mesh_bake, mesh_bake_device). Queued on the context's stream, no sync."""
        q = self._bake_params(params, fields)
        t = np.ascontiguousarray(times, np.float32).reshape(-1)
        self._chk(self._L.rmr_bake_mesh(self._ctx, _fp(t) if len(t) else None, len(t), C.byref(q)))

    def read_mesh_bake(self, rgba=True, ao=False):
        """rmr_read_mesh_bake: the mesh's baked 'rgba' (V, 4) and / or 'ao' (V,) as a dict (None: not asked for)."""
        nv = (self._mesh_info or (0,))[0]
        c = np.zeros((nv, 4), np.float32) if rgba else None
        a = np.zeros((nv,), np.float32) if ao else None
        self._chk(self._L.rmr_read_mesh_bake(self._ctx, _fp(c) if rgba else None, _fp(a) if ao else None))
        return {"rgba": c, "ao": a}

    def mesh_bake_device(self):
        """rmr_mesh_bake_device_ptr: the mesh's bake as torch tensors on the context's device, views of the
        library's memory (no copy, no sync): 'rgba' (V, 4) and 'ao' (V,), None for what was not baked. Valid
        until the next extraction, mesh_free or reload."""
        import torch
        nv = (self._mesh_info or (0,))[0]
        out = {}
        for name, which, shape in (("rgba", abi.MESH_BAKE_RGBA, (nv, 4)), ("ao", abi.MESH_BAKE_AO, (nv,))):
            ptr = self._L.rmr_mesh_bake_device_ptr(self._ctx, which) if nv else None
            out[name] = torch.as_tensor(_DeviceArray(ptr, shape, self), device="cuda:%d" % self._device) if ptr else None
        return out

    # -- irradiance probes: SH light baking on a lattice and its lookup (rmr.h) --
    @staticmethod
    def _probe_params(params, fields):
        if params is not None and fields:
            raise ValueError("params or its fields as keywords, not both (got params and %s)" % ", ".join(sorted(fields)))
        q = abi.probe_params(**fields) if params is None else params
        if not isinstance(q, abi.ProbeParams):
            raise ValueError("params: an abi.ProbeParams (abi.probe_params(...))")
        return q

    def bake_probes(self, points, times, params=None, **fields):
        """rmr_bake_probes: the radiance over the whole sphere at n probe points ((n, 3) float32) from the samples
        seeded `times`, projected onto nine spherical harmonics per channel: (n, 28) float32, sh[9][3] then the
        samples used. params: an abi.ProbeParams, or its fields as keywords (abi.probe_params: clearance,
        first_index). A rejected or buried probe (rmr.h) gives zeros; rejected ones count in query_rejects()."""
        q = self._probe_params(params, fields)
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        t = np.ascontiguousarray(times, np.float32).reshape(-1)
        out = np.zeros((len(p), abi.PROBE_FLOATS), np.float32)
        self._chk(self._L.rmr_bake_probes(self._ctx, _fp(p), len(p), _fp(t) if len(t) else None, len(t), C.byref(q), _fp(out)))
        return out

    @staticmethod
    def _device_probes(points):
        import torch
        if not (points.is_cuda and points.dtype == torch.float32 and points.dim() == 2 and points.shape[1] == 3
                and points.is_contiguous()):
            raise ValueError("points: a contiguous (n, 3) float32 CUDA tensor")
        return points.shape[0]

    def bake_probes_device(self, points, times, origin_extent, params=None, **fields):
        """rmr_bake_probes_device: bake_probes on a torch CUDA tensor ((n, 3) float32), the (n, 28) result a torch
        tensor on the same device; queued on the context's stream (set_stream), no copy to the host and no sync.
        origin_extent: a bound on |coordinate| of every probe."""
        import torch
        q = self._probe_params(params, fields)
        q = abi.ProbeParams(q.clearance, float(origin_extent), q.first_index)
        n = self._device_probes(points)
        t = np.ascontiguousarray(times, np.float32).reshape(-1)
        out = torch.empty((n, abi.PROBE_FLOATS), dtype=torch.float32, device=points.device)
        self._chk(self._L.rmr_bake_probes_device(self._ctx, points.data_ptr(), n, _fp(t) if len(t) else None, len(t),
                                                 C.byref(q), out.data_ptr()))
        return out

    def probe_rays_device(self, points, times, params=None, **fields):
        """rmr_probe_rays_device: the rays the probe bake generates, a (len(times) * n, 10) float32 CUDA tensor
        (views of abi.RAY_DTYPE, ray [k * n + i] = sample k of probe i) for trace_rays_device; a rejected or
        buried probe's rays carry gx = -1. Queued on the context's stream, no sync."""
        import torch
        q = self._probe_params(params, fields)
        n = self._device_probes(points)
        t = np.ascontiguousarray(times, np.float32).reshape(-1)
        out = torch.empty((len(t) * n, 10), dtype=torch.float32, device=points.device)
        self._chk(self._L.rmr_probe_rays_device(self._ctx, points.data_ptr(), n, _fp(t) if len(t) else None, len(t),
                                                C.byref(q), out.data_ptr()))
        return out

    def bake_probe_field(self, origin, spacing=None, shape=None, *, times, params=None, **fields):
        """rmr_bake_probe_field: bake the probes at the lattice's points (an abi.VolumeDesc or origin, spacing,
        shape) into the context's field (read_probe_field, probe_field_device, probe_irradiance). Queued on the
        context's stream, no sync."""
        q = self._probe_params(params, fields)
        d = _volume_desc(origin, spacing, shape)
        t = np.ascontiguousarray(times, np.float32).reshape(-1)
        self._chk(self._L.rmr_bake_probe_field(self._ctx, C.byref(d), _fp(t) if len(t) else None, len(t), C.byref(q)))

    def write_probe_field(self, desc, sh):
        """rmr_write_probe_field: load a saved or synthetic field, sh (points, 28) float32 over the lattice desc
        (an abi.VolumeDesc or (origin, spacing, shape))."""
        d = desc if isinstance(desc, abi.VolumeDesc) else abi.volume_desc(*desc)
        a = np.ascontiguousarray(sh, np.float32)
        if a.size != d.n[0] * d.n[1] * d.n[2] * abi.PROBE_FLOATS:
            raise ValueError("sh: 28 floats per lattice point")
        self._chk(self._L.rmr_write_probe_field(self._ctx, C.byref(d), _fp(a)))

    def read_probe_field(self):
        """rmr_read_probe_field: (desc, sh): the field's abi.VolumeDesc and its (points, 28) float32 array."""
        d = abi.VolumeDesc()
        self._chk(self._L.rmr_read_probe_field(self._ctx, C.byref(d), None))
        sh = np.zeros((d.n[0] * d.n[1] * d.n[2], abi.PROBE_FLOATS), np.float32)
        self._chk(self._L.rmr_read_probe_field(self._ctx, None, _fp(sh)))
        return d, sh

    def probe_field_device(self):
        """rmr_probe_field_device_ptr: the field as a (points, 28) torch tensor on the context's device, a view of
        the library's memory (no copy, no sync), or None before a field exists. Valid until the next field,
        probe_field_free or reload."""
        import torch
        ptr = self._L.rmr_probe_field_device_ptr(self._ctx)
        if not ptr:
            return None
        d = abi.VolumeDesc()
        self._chk(self._L.rmr_read_probe_field(self._ctx, C.byref(d), None))
        shape = (d.n[0] * d.n[1] * d.n[2], abi.PROBE_FLOATS)
        return torch.as_tensor(_DeviceArray(ptr, shape, self), device="cuda:%d" % self._device)

    def probe_field_free(self):
        """rmr_probe_field_free: release the field and the probe bakes' working memory."""
        self._chk(self._L.rmr_probe_field_free(self._ctx))

    def probe_irradiance(self, points, normals, visibility=False, bias=0.0):
        """rmr_probe_irradiance: irradiance / pi at n points with unit normals ((n, 3) float32 each) from the
        context's field: (n, 4) float32, rgb and the valid corners' weight. A rejected query gives zeros and
        counts in query_rejects(). visibility=True: rmr_probe_irradiance_vis, each corner weighted by the field's
        visibility maps (bake_probe_field_visibility) and a back-face term, the point moved bias along its normal;
        it raises without baked maps."""
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        nn = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        if len(p) != len(nn):
            raise ValueError("one normal per point")
        out = np.zeros((len(p), 4), np.float32)
        if visibility:
            self._chk(self._L.rmr_probe_irradiance_vis(self._ctx, _fp(p), _fp(nn), len(p), float(bias), _fp(out)))
        else:
            self._chk(self._L.rmr_probe_irradiance(self._ctx, _fp(p), _fp(nn), len(p), _fp(out)))
        return out

    def probe_irradiance_device(self, points, normals, visibility=False, bias=0.0):
        """rmr_probe_irradiance_device: probe_irradiance on torch CUDA tensors, the (n, 4) result a torch tensor on
        the same device; queued on the context's stream, no sync."""
        import torch
        n = self._device_points(points, normals)
        out = torch.empty((n, 4), dtype=torch.float32, device=points.device)
        if visibility:
            self._chk(self._L.rmr_probe_irradiance_vis_device(self._ctx, points.data_ptr(), normals.data_ptr(), n, float(bias),
                                                              out.data_ptr()))
        else:
            self._chk(self._L.rmr_probe_irradiance_device(self._ctx, points.data_ptr(), normals.data_ptr(), n, out.data_ptr()))
        return out

    # -- the probes' visibility: octahedral depth moments per probe (rmr.h) --
    def bake_probe_visibility(self, points, times, range, clearance=0.0, first_index=0):
        """rmr_bake_probe_visibility: the visibility maps of n probe points ((n, 3) float32) from the samples
        seeded `times`: (n, 64, 2) float32, the first two moments of the distance min(t, range) each of the 8 x 8
        octahedral texels sees. A rejected or buried probe gives zeros; rejected ones count in query_rejects()."""
        q = abi.probe_params(clearance=clearance, first_index=first_index)
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        t = np.ascontiguousarray(times, np.float32).reshape(-1)
        out = np.zeros((len(p), abi.PROBE_VIS_TEXELS, 2), np.float32)
        self._chk(self._L.rmr_bake_probe_visibility(self._ctx, _fp(p), len(p), _fp(t) if len(t) else None, len(t), C.byref(q),
                                                    float(range), _fp(out)))
        return out

    def bake_probe_visibility_device(self, points, times, origin_extent, range, clearance=0.0, first_index=0):
        """rmr_bake_probe_visibility_device: bake_probe_visibility on a torch CUDA tensor ((n, 3) float32), the
        (n, 64, 2) result a torch tensor on the same device; queued on the context's stream, no sync.
        origin_extent: a bound on |coordinate| of every probe."""
        import torch
        q = abi.ProbeParams(float(clearance), float(origin_extent), int(first_index))
        n = self._device_probes(points)
        t = np.ascontiguousarray(times, np.float32).reshape(-1)
        out = torch.empty((n, abi.PROBE_VIS_TEXELS, 2), dtype=torch.float32, device=points.device)
        self._chk(self._L.rmr_bake_probe_visibility_device(self._ctx, points.data_ptr(), n, _fp(t) if len(t) else None, len(t),
                                                           C.byref(q), float(range), out.data_ptr()))
        return out

    def bake_probe_field_visibility(self, times, range=None):
        """rmr_bake_probe_field_visibility: the maps of the context's field, stored with it for
        probe_irradiance(..., visibility=True). range=None: np.float32(2.6) * spacing, about 1.5 cell diagonals.
        Queued on the context's stream, no sync."""
        if range is None:
            d = abi.VolumeDesc()
            self._chk(self._L.rmr_read_probe_field(self._ctx, C.byref(d), None))
            range = np.float32(2.6) * np.float32(d.spacing)
        t = np.ascontiguousarray(times, np.float32).reshape(-1)
        self._chk(self._L.rmr_bake_probe_field_visibility(self._ctx, _fp(t) if len(t) else None, len(t), float(range)))

    def _probe_field_points(self):
        d = abi.VolumeDesc()
        self._chk(self._L.rmr_read_probe_field(self._ctx, C.byref(d), None))
        return d.n[0] * d.n[1] * d.n[2]

    def write_probe_field_visibility(self, vis, range):
        """rmr_write_probe_field_visibility: load saved or synthetic maps, vis (points, 64, 2) float32, for the
        context's field."""
        a = np.ascontiguousarray(vis, np.float32)
        if a.size != self._probe_field_points() * abi.PROBE_VIS_FLOATS:
            raise ValueError("vis: 128 floats per lattice point")
        self._chk(self._L.rmr_write_probe_field_visibility(self._ctx, _fp(a), float(range)))

    def read_probe_field_visibility(self):
        """rmr_read_probe_field_visibility: (vis (points, 64, 2) float32, range)."""
        rng = C.c_float(0.0)
        self._chk(self._L.rmr_read_probe_field_visibility(self._ctx, None, C.byref(rng)))
        vis = np.zeros((self._probe_field_points(), abi.PROBE_VIS_TEXELS, 2), np.float32)
        self._chk(self._L.rmr_read_probe_field_visibility(self._ctx, _fp(vis), None))
        return vis, np.float32(rng.value)

    def probe_field_visibility_device(self):
        """rmr_probe_field_visibility_device_ptr: the maps as a (points, 64, 2) torch tensor on the context's
        device, a view of the library's memory (no copy, no sync), or None without them."""
        import torch
        ptr = self._L.rmr_probe_field_visibility_device_ptr(self._ctx)
        if not ptr:
            return None
        shape = (self._probe_field_points(), abi.PROBE_VIS_TEXELS, 2)
        return torch.as_tensor(_DeviceArray(ptr, shape, self), device="cuda:%d" % self._device)

    def sync(self):
        self._chk(self._L.rmr_sync(self._ctx))

    def read_accum(self):
        w, h = self.image_size()
        out = np.zeros((h, w, 4), np.float32)
        self._chk(self._L.rmr_read_accum(self._ctx, _fp(out), out.nbytes))
        return out

    def write_accum(self, a):
        a = np.ascontiguousarray(a, np.float32)
        self._chk(self._L.rmr_write_accum(self._ctx, _fp(a), a.nbytes))

    def accum_device_ptr(self):
        return self._L.rmr_accum_device_ptr(self._ctx)

    def bind_accum(self, dev_ptr, nbytes):
        self._chk(self._L.rmr_bind_accum(self._ctx, C.c_void_p(dev_ptr), int(nbytes)))

    def save_bmp(self, path):
        self._chk(self._L.rmr_save_bmp(self._ctx, path.encode()))

    def save_accum(self, path, samples_done):
        self._chk(self._L.rmr_save_accum(self._ctx, path.encode(), int(samples_done)))

    def load_accum(self, path):
        n = C.c_uint32()
        self._chk(self._L.rmr_load_accum(self._ctx, path.encode(), C.byref(n)))
        return n.value

    def display(self, centre, zoom, vmin, vmax, screen=None, screen_size=None):
        """Graphics::Display(centre, zoom, min, max) headless (rmr_display): the accumulator drawn into
        an RGBA8 screen image (h, w, 4) uint8, row 0 = top. `screen` is the image behind it (kept
        where the quad draws alpha 0); without it a zeroed image of `screen_size` (w, h)."""
        if screen is None:
            w, h = screen_size
            screen = np.zeros((int(h), int(w), 4), np.uint8)
        screen = np.ascontiguousarray(screen, np.uint8)
        if screen.ndim != 3 or screen.shape[2] != 4:
            raise ValueError("display: screen must be an (h, w, 4) RGBA8 image, got shape %s" % (screen.shape,))
        h, w = screen.shape[:2]
        self._chk(self._L.rmr_display(self._ctx, float(centre[0]), float(centre[1]), float(zoom),
                                            float(vmin[0]), float(vmin[1]), float(vmax[0]), float(vmax[1]),
                                            w, h, screen.ctypes.data, screen.nbytes))
        return screen

    def display_device(self, centre, zoom, vmin, vmax, dev, screen_w, screen_h, nbytes=None):
        """rmr_display_device: the same into a device RGBA8 buffer on the renderer's stream. `dev` is a
        torch tensor on the GPU (its size is numel * element_size) or a raw device pointer, which needs
        `nbytes`, the buffer's size in bytes (the library checks it against screen_w * screen_h * 4)."""
        if hasattr(dev, "data_ptr"):
            if not dev.is_contiguous():
                raise ValueError("display_device: the tensor must be contiguous")
            size = dev.numel() * dev.element_size()
            if nbytes is not None and int(nbytes) > size:
                raise ValueError("display_device: nbytes %d exceeds the tensor's %d bytes" % (nbytes, size))
            nbytes = size if nbytes is None else int(nbytes)
            dev_ptr = dev.data_ptr()
        else:
            if nbytes is None:
                raise ValueError("display_device: a raw device pointer needs nbytes (the buffer's size in bytes)")
            dev_ptr = int(dev)
        self._chk(self._L.rmr_display_device(self._ctx, float(centre[0]), float(centre[1]), float(zoom),
                                                   float(vmin[0]), float(vmin[1]), float(vmax[0]), float(vmax[1]),
                                                   int(screen_w), int(screen_h), C.c_void_p(dev_ptr), int(nbytes)))

    # -- first-hit guides and the preview denoiser --
    def render_guides(self, rect=None):
        """rmr_render_guides: the first-hit guide planes of the integer rect (the whole image without
        one). The guides are valid once a call covers the whole image."""
        if rect is None:
            w, h = self.image_size()
            rect = (0, 0, w, h)
        x0, y0, x1, y1 = (int(v) for v in rect)
        self._chk(self._L.rmr_render_guides(self._ctx, x0, y0, x1, y1))

    def read_guide(self, plane):
        """One guide plane as an (H, W, 4) float32 array; plane: abi.GUIDE_* or 'ray' / 'hit' / 'normal'."""
        if isinstance(plane, str):
            if plane not in abi.GUIDE_PLANES:
                raise ValueError("read_guide: unknown plane %r (ray, hit, normal)" % plane)
            plane = abi.GUIDE_PLANES[plane]
        w, h = self.image_size()
        out = np.zeros((h, w, 4), np.float32)
        self._chk(self._L.rmr_read_guide(self._ctx, int(plane), _fp(out), out.nbytes))
        return out

    def read_guides(self):
        """The three guide planes: {'ray': (dir, 0), 'hit': (pos, t), 'normal': (normal, id) or
        (0, 0, 0, -1) for a miss}, each (H, W, 4) float32."""
        return {name: self.read_guide(plane) for name, plane in abi.GUIDE_PLANES.items()}

    def guide_device_ptr(self, plane):
        if isinstance(plane, str):
            if plane not in abi.GUIDE_PLANES:
                raise ValueError("guide_device_ptr: unknown plane %r (ray, hit, normal)" % plane)
            plane = abi.GUIDE_PLANES[plane]
        return self._L.rmr_guide_device_ptr(self._ctx, int(plane))

    def denoise(self, params=None, **kw):
        """rmr_denoise: filter the accumulator (left unchanged) and return the denoised image (H, W, 4).
        Keywords: iterations (5; 0..8), normal_pow2 (5; 0..7), sigma_z (0.02; > 0), sigma_c (0 = off)."""
        if params is not None and not isinstance(params, abi.DenoiseParams):
            raise TypeError("denoise: params must be an abi.DenoiseParams")
        p = abi.default_denoise_params() if params is None else abi.DenoiseParams.from_buffer_copy(params)
        for k, v in kw.items():
            if k not in ("iterations", "normal_pow2", "sigma_z", "sigma_c"):
                raise TypeError("denoise: unknown parameter %r" % k)
            setattr(p, k, v)
        self._chk(self._L.rmr_denoise(self._ctx, C.byref(p)))
        return self.read_denoised()

    def read_denoised(self):
        w, h = self.image_size()
        out = np.zeros((h, w, 4), np.float32)
        self._chk(self._L.rmr_read_denoised(self._ctx, _fp(out), out.nbytes))
        return out

    def denoised_device_ptr(self):
        """Device pointer of the valid denoised image (W x H float4), None without one."""
        return self._L.rmr_denoised_device_ptr(self._ctx)

    def set_output_source(self, source):
        """What save_bmp / display / display_device read: abi.OUTPUT_ACCUM (default), abi.OUTPUT_DENOISED
        abi.OUTPUT_TEMPORAL, abi.OUTPUT_TONEMAPPED or abi.OUTPUT_BLOOM (also 'accum' / 'denoised' / 'temporal' /
        'tonemapped' / 'bloom'; the last three need a temporal / tonemapped / bloom image)."""
        if isinstance(source, str):
            names = abi.OUTPUT_SOURCES
            if source not in names:
                raise ValueError("set_output_source: unknown source %r (accum, denoised, temporal, tonemapped, bloom)" % source)
            source = names[source]
        self._chk(self._L.rmr_set_output_source(self._ctx, int(source)))

    # -- temporal reprojection of the preview across camera moves --
    @staticmethod
    def _temporal_params(who, params, kw):
        if params is not None and not isinstance(params, abi.TemporalParams):
            raise TypeError("%s: params must be an abi.TemporalParams" % who)
        p = abi.default_temporal_params() if params is None else abi.TemporalParams.from_buffer_copy(params)
        for k, v in kw.items():
            if k not in abi.TEMPORAL_FIELDS:
                raise TypeError("%s: unknown parameter %r" % (who, k))
            setattr(p, k, v)
        return p

    def temporal_accumulate(self, source="accum", samples=1.0, params=None, **kw):
        """rmr_temporal_accumulate: re-project the history into the current view and blend it with the
        source image ('accum' or 'denoised', or abi.OUTPUT_*) of `samples` samples per pixel; the result,
        returned as (H, W, 4), is the new history. The loop: set_view, reload, render_spp(k), denoise(),
        temporal_accumulate('denoised', k). Keywords: max_history (64; >= 1), sigma_z (0.02; > 0),
        normal_pow2 (5; 0..7)."""
        if isinstance(source, str):
            if source not in ("accum", "denoised"):
                raise ValueError("temporal_accumulate: unknown source %r (accum, denoised)" % source)
            source = abi.OUTPUT_SOURCES[source]
        p = self._temporal_params("temporal_accumulate", params, kw)
        self._chk(self._L.rmr_temporal_accumulate(self._ctx, int(source), C.c_float(samples), C.byref(p)))
        return self.read_temporal()

    def read_temporal(self):
        w, h = self.image_size()
        out = np.zeros((h, w, 4), np.float32)
        self._chk(self._L.rmr_read_temporal(self._ctx, _fp(out), out.nbytes))
        return out

    def read_temporal_count(self):
        """The temporal image's effective sample counts as an (H, W) float32 array (0: not live)."""
        w, h = self.image_size()
        out = np.zeros((h, w), np.float32)
        self._chk(self._L.rmr_read_temporal_count(self._ctx, _fp(out), out.nbytes))
        return out

    def temporal_device_ptr(self):
        """Device pointer of the valid temporal image (W x H float4), None without one."""
        return self._L.rmr_temporal_device_ptr(self._ctx)

    def temporal_reset(self):
        """rmr_temporal_reset: drop the history."""
        self._chk(self._L.rmr_temporal_reset(self._ctx))

    # -- tone mapping and histogram auto-exposure --
    @staticmethod
    def _stage_source(who, source, names=("accum", "denoised", "temporal")):
        if isinstance(source, str):
            if source not in names:
                raise ValueError("%s: unknown source %r (%s)" % (who, source, ", ".join(names)))
            source = abi.OUTPUT_SOURCES[source]
        return int(source)

    _BLOOM_TOO = ("accum", "denoised", "temporal", "bloom")

    def tonemap(self, source="accum", curve="aces", exposure=0.0, params=None, **kw):
        """rmr_tonemap: scale the source image ('accum', 'denoised', 'temporal' or 'bloom', or abi.OUTPUT_*) by an
        exposure and apply a curve ('linear', 'reinhard', 'aces', or abi.TONE_*); the result, values in
        [0, 1] returned as (H, W, 4), is what set_output_source('tonemapped') shows. exposure: a number of
        stops (scale 2^ev), or 'auto': metered on the GPU from the image's luminance histogram (then
        exposure_ev, if given, is added to the metered value). Keywords: key (0.18), low_pct / high_pct
        (0.10 / 0.90: the metered part of the histogram), adapt (1; the share of the way from the previous
        exposure to the metered one, for a loop), white (4; reinhard's white point), exposure_ev."""
        if params is not None and not isinstance(params, abi.TonemapParams):
            raise TypeError("tonemap: params must be an abi.TonemapParams")
        p = abi.default_tonemap_params() if params is None else abi.TonemapParams.from_buffer_copy(params)
        if params is None:
            if isinstance(curve, str):
                if curve not in abi.TONE_CURVES:
                    raise ValueError("tonemap: unknown curve %r (linear, reinhard, aces)" % curve)
                curve = abi.TONE_CURVES[curve]
            p.curve = int(curve)
            if isinstance(exposure, str):
                if exposure != "auto":
                    raise ValueError("tonemap: exposure is a number of stops or 'auto', got %r" % exposure)
                p.auto_exposure = 1
            else:
                p.exposure_ev = float(exposure)
        for k, v in kw.items():
            if k not in abi.TONEMAP_FIELDS:
                raise TypeError("tonemap: unknown parameter %r" % k)
            setattr(p, k, v)
        self._chk(self._L.rmr_tonemap(self._ctx, self._stage_source("tonemap", source, self._BLOOM_TOO), C.byref(p)))
        return self.read_tonemapped()

    def read_tonemapped(self):
        w, h = self.image_size()
        out = np.zeros((h, w, 4), np.float32)
        self._chk(self._L.rmr_read_tonemapped(self._ctx, _fp(out), out.nbytes))
        return out

    def tonemapped_device_ptr(self):
        """Device pointer of the valid tonemapped image (W x H float4), None without one."""
        return self._L.rmr_tonemapped_device_ptr(self._ctx)

    def read_exposure(self):
        """(log2_scale, scale) the last tonemap used."""
        l, s = C.c_double(0.0), C.c_float(0.0)
        self._chk(self._L.rmr_read_exposure(self._ctx, C.byref(l), C.byref(s)))
        return l.value, np.float32(s.value)

    def luminance_histogram(self, source="accum"):
        """rmr_luminance_histogram: (hist (256,) uint32, skipped) of a source image, by the stage's kernels."""
        hist = np.zeros(256, np.uint32)
        skipped = C.c_uint64(0)
        self._chk(self._L.rmr_luminance_histogram(self._ctx, self._stage_source("luminance_histogram", source, self._BLOOM_TOO),
                                                  hist.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(skipped)))
        return hist, int(skipped.value)

    def tonemap_reset(self):
        """rmr_tonemap_reset: drop the auto-exposure's adaptation state."""
        self._chk(self._L.rmr_tonemap_reset(self._ctx))

    # -- HDR bloom ahead of tone mapping --
    def bloom(self, source="accum", levels=5, threshold=1.0, clamp=0.0, scatter=0.7, intensity=0.2, params=None):
        """rmr_bloom: spread the part of the source image ('accum', 'denoised' or 'temporal', or abi.OUTPUT_*)
        above `threshold` (scene units) over a pyramid of `levels` levels and add it back, `intensity` of it in
        all; scatter: the weight of each coarser level against the finer one; clamp (0 = off): the most a
        pixel's excess over the threshold counts (fireflies). The sum, returned as (H, W, 4), is what
        tonemap('bloom') and set_output_source('bloom') read. params: an abi.BloomParams instead of the
        keywords."""
        if params is not None and not isinstance(params, abi.BloomParams):
            raise TypeError("bloom: params must be an abi.BloomParams")
        if params is None:
            p = abi.default_bloom_params(levels=int(levels), threshold=threshold, clamp=clamp, scatter=scatter,
                                         intensity=intensity)
        else:
            p = abi.BloomParams.from_buffer_copy(params)
        self._chk(self._L.rmr_bloom(self._ctx, self._stage_source("bloom", source), C.byref(p)))
        return self.read_bloom()

    def read_bloom(self):
        w, h = self.image_size()
        out = np.zeros((h, w, 4), np.float32)
        self._chk(self._L.rmr_read_bloom(self._ctx, _fp(out), out.nbytes))
        return out

    def bloom_device_ptr(self):
        """Device pointer of the valid bloom image (W x H float4), None without one."""
        return self._L.rmr_bloom_device_ptr(self._ctx)

    def temporal_images(self, S, hit, normal, view, h_rgba, h_n, h_hit, h_normal, h_view, samples=1.0, params=None,
                        **kw):
        """rmr_temporal_images (test hook): the stage's kernel on host images, (h, w, 4) each and h_n
        (h, w). Returns (image (h, w, 4), counts (h, w), projected coordinates (h, w, 2))."""
        p = self._temporal_params("temporal_images", params, kw)
        imgs = [np.ascontiguousarray(x, np.float32) for x in (S, hit, normal, h_rgba, h_hit, h_normal)]
        if imgs[0].ndim != 3 or imgs[0].shape[2] != 4 or any(x.shape != imgs[0].shape for x in imgs):
            raise ValueError("temporal_images: the six images must be (h, w, 4) of one shape, got %s"
                             % ", ".join(str(x.shape) for x in imgs))
        h, w = imgs[0].shape[:2]
        hn = np.ascontiguousarray(h_n, np.float32)
        if hn.shape != (h, w):
            raise ValueError("temporal_images: h_n must be (%d, %d), got %s" % (h, w, hn.shape))
        v = np.ascontiguousarray(view, np.float32).reshape(15)
        hv = np.ascontiguousarray(h_view, np.float32).reshape(15)
        out = np.zeros((h, w, 4), np.float32)
        n = np.zeros((h, w), np.float32)
        xy = np.zeros((h, w, 2), np.float32)
        self._chk(self._L.rmr_temporal_images(self._ctx, _fp(imgs[0]), _fp(imgs[1]), _fp(imgs[2]), _fp(v), _fp(imgs[3]),
                                               _fp(hn), _fp(imgs[4]), _fp(imgs[5]), _fp(hv), w, h, C.c_float(samples),
                                               C.byref(p), _fp(out), _fp(n), _fp(xy)))
        return out, n, xy

    # -- variance-guided mode of the preview denoiser --
    @staticmethod
    def _guided_params(who, params, variance, kw):
        if params is not None and not isinstance(params, abi.DenoiseParams):
            raise TypeError("%s: params must be an abi.DenoiseParams" % who)
        if variance is not None and not isinstance(variance, abi.VarianceParams):
            raise TypeError("%s: variance must be an abi.VarianceParams" % who)
        p = abi.default_denoise_params() if params is None else abi.DenoiseParams.from_buffer_copy(params)
        v = abi.default_variance_params() if variance is None else abi.VarianceParams.from_buffer_copy(variance)
        for k, val in kw.items():
            if k in abi.DENOISE_FIELDS:
                setattr(p, k, val)
            elif k in abi.VARIANCE_FIELDS:
                setattr(v, k, val)
            else:
                raise TypeError("%s: unknown parameter %r" % (who, k))
        return p, v

    @staticmethod
    def _variance_plane(who, which):
        if isinstance(which, str):
            if which not in abi.VARIANCE_PLANES:
                raise ValueError("%s: unknown plane %r (seed, filtered)" % (who, which))
            return abi.VARIANCE_PLANES[which]
        if isinstance(which, bool) or not isinstance(which, (int, np.integer)) or int(which) not in abi.VARIANCE_PLANES.values():
            raise ValueError("%s: unknown plane %r (seed, filtered)" % (who, which))
        return int(which)

    def denoise_variance(self, params=None, variance=None, **kw):
        """rmr_denoise_variance: the variance-guided filter over the accumulator (left unchanged); needs a
        valid error estimate (set_error_estimate before the first render, or render_adaptive). Returns
        the denoised image (H, W, 4). Keywords: denoise's, and sigma_l (4; > 0), var_radius (3; 0..4)."""
        p, v = self._guided_params("denoise_variance", params, variance, kw)
        self._chk(self._L.rmr_denoise_variance(self._ctx, C.byref(p), C.byref(v)))
        return self.read_denoised()

    def read_variance(self, which="filtered"):
        """One variance plane of the last denoise_variance as an (H, W) float32 array: 'seed' or
        'filtered' (abi.VARIANCE_*); -1 where the pixel is not v-live."""
        which = self._variance_plane("read_variance", which)
        w, h = self.image_size()
        out = np.zeros((h, w), np.float32)
        self._chk(self._L.rmr_read_variance(self._ctx, which, _fp(out), out.nbytes))
        return out

    def variance_device_ptr(self, which="filtered"):
        """Device pointer of a valid variance plane (W x H floats), None without one."""
        which = self._variance_plane("variance_device_ptr", which)
        return self._L.rmr_variance_device_ptr(self._ctx, which)

    def denoise_variance_images(self, A, B, hit, normal, params=None, variance=None, **kw):
        """rmr_denoise_variance_images (test hook): the seed and the guided passes on four host (h, w, 4)
        images. Returns (image (h, w, 4), seed (h, w), filtered variance (h, w))."""
        p, v = self._guided_params("denoise_variance_images", params, variance, kw)
        imgs = [np.ascontiguousarray(x, np.float32) for x in (A, B, hit, normal)]
        if imgs[0].ndim != 3 or imgs[0].shape[2] != 4 or any(x.shape != imgs[0].shape for x in imgs):
            raise ValueError("denoise_variance_images: A, B, hit and normal must be (h, w, 4) images of one shape, got %s"
                             % ", ".join(str(x.shape) for x in imgs))
        h, w = imgs[0].shape[:2]
        out = np.zeros((h, w, 4), np.float32)
        seed = np.zeros((h, w), np.float32)
        var = np.zeros((h, w), np.float32)
        self._chk(self._L.rmr_denoise_variance_images(self._ctx, _fp(imgs[0]), _fp(imgs[1]), _fp(imgs[2]), _fp(imgs[3]),
                                                       w, h, C.byref(p), C.byref(v), _fp(out), _fp(seed), _fp(var)))
        return out, seed, var

    # -- per-tile error estimate and adaptive sampling --
    def set_error_estimate(self, on=True):
        """rmr_set_error_estimate: while on, every fold also keeps the half image (the mean of the
        odd-indexed samples). Valid when enabled before the first render after a reload."""
        self._chk(self._L.rmr_set_error_estimate(self._ctx, 1 if on else 0))

    def read_half(self):
        """The half image as an (H, W, 4) float32 array (rmr_read_half_accum)."""
        w, h = self.image_size()
        out = np.zeros((h, w, 4), np.float32)
        self._chk(self._L.rmr_read_half_accum(self._ctx, _fp(out), out.nbytes))
        return out

    def half_device_ptr(self):
        return self._L.rmr_half_device_ptr(self._ctx)

    def tile_error(self, offset=1e-4):
        """rmr_tile_error: the (ceil(H / 8), ceil(W / 8)) float32 map of tile errors of the accumulator
        against the half image; +inf where a tile has a pixel with fewer than two samples."""
        w, h = self.image_size()
        out = np.zeros(((h + 7) // 8, (w + 7) // 8), np.float32)
        self._chk(self._L.rmr_tile_error(self._ctx, float(offset), _fp(out), out.nbytes))
        return out

    def tile_error_images(self, A, B, offset=1e-4):
        """rmr_tile_error_images (test hook): the tile-error kernel on two host (h, w, 4) images."""
        A = np.ascontiguousarray(A, np.float32)
        B = np.ascontiguousarray(B, np.float32)
        if A.ndim != 3 or A.shape[2] != 4 or A.shape != B.shape:
            raise ValueError("tile_error_images: A and B must be (h, w, 4) images of one shape, got %s and %s"
                             % (A.shape, B.shape))
        h, w = A.shape[:2]
        out = np.zeros(((h + 7) // 8, (w + 7) // 8), np.float32)
        self._chk(self._L.rmr_tile_error_images(self._ctx, _fp(A), _fp(B), w, h, float(offset), _fp(out)))
        return out

    def render_adaptive(self, times, params=None, **kw):
        """rmr_render_adaptive: samples 0 .. min_samples-1 everywhere, then pass_samples at a time on the
        decision blocks whose tile error is still > threshold, at most len(times) (or max_samples) per
        pixel. Keywords: threshold (0.1), offset (1e-4), min_samples (16), pass_samples (16),
        max_samples (len(times)), block_tiles (2). Returns the abi.AdaptiveResult."""
        times = np.ascontiguousarray(times, np.float32)
        if params is not None and not isinstance(params, abi.AdaptiveParams):
            raise TypeError("render_adaptive: params must be an abi.AdaptiveParams")
        p = abi.default_adaptive_params() if params is None else abi.AdaptiveParams.from_buffer_copy(params)
        for k, v in kw.items():
            if k not in abi.ADAPTIVE_FIELDS:
                raise TypeError("render_adaptive: unknown parameter %r" % k)
            setattr(p, k, v)
        if p.max_samples == 0:
            p.max_samples = len(times)
        if p.max_samples > len(times):
            raise ValueError("render_adaptive: max_samples %d exceeds the %d seeds given" % (p.max_samples, len(times)))
        res = abi.AdaptiveResult()
        self._chk(self._L.rmr_render_adaptive(self._ctx, _fp(times), C.byref(p), C.byref(res)))
        return res

    def sample_counts(self):
        """Samples per 8x8 tile of the last render_adaptive: (ceil(H / 8), ceil(W / 8)) uint32."""
        w, h = self.image_size()
        out = np.zeros(((h + 7) // 8, (w + 7) // 8), np.uint32)
        self._chk(self._L.rmr_read_sample_counts(self._ctx, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.nbytes))
        return out

    def stats(self):
        s = abi.Stats()
        self._chk(self._L.rmr_get_stats(self._ctx, C.byref(s)))
        return s

    def reset_stats(self):
        self._chk(self._L.rmr_reset_stats(self._ctx))

    def counters(self, n=32):
        """The kernels' first n raw device counters (rmr_get_counters_n; rmr.h and rmr_internal.h document
        the slots: 0-15 as ever, 16 the overflow deposits, 17-30 the profiling build's own, 31-33 the
        trailing steps')."""
        raw = (C.c_uint64 * n)()
        self._chk(self._L.rmr_get_counters_n(self._ctx, raw, n))
        return [int(v) for v in raw]


def jit_compile_scene(scene, variant, diag=None):
    """Compile the hipRTC-specialised trace kernel of a scene (no GPU needed). Returns the
    code-object key; raises RMRError with the compiler log on failure. diag: through the
    diagnostic build (which reads the experiments' RMR_JIT_* environment switches)."""
    if isinstance(variant, str):
        variant = abi.VARIANTS[variant]
    if scene is None:
        text = b""
    elif isinstance(scene, dict):
        text = json.dumps(scene).encode()
    elif os.path.exists(scene):
        text = open(scene, "rb").read()
    else:
        text = scene.encode()
    log = C.create_string_buffer(65536)
    rc = lib(diag=diag).rmr_jit_compile_scene(int(variant), text or None, len(text), log, len(log))
    if rc != abi.RMR_OK:
        raise RMRError(rc, log.value.decode(errors="replace"))
    return log.value.decode()


def camera_frame(view):
    """rmr_camera_frame (no GPU): U, V, FWD of a 15-float view as a (3, 3) float32 array (rows)."""
    v = np.ascontiguousarray(view, np.float32).reshape(15)
    out = np.zeros(9, np.float32)
    rc = lib().rmr_camera_frame(_fp(v), _fp(out))
    if rc != abi.RMR_OK:
        raise RMRError(rc, "rmr_camera_frame: degenerate view")
    return out.reshape(3, 3)


def check_camera_model(model, **fields):
    """rmr_check_camera_model (no GPU): True iff the model is known and its fields are in range."""
    m = model if isinstance(model, abi.CameraModel) else abi.default_camera_model(model, **fields)
    return lib().rmr_check_camera_model(C.byref(m)) == abi.RMR_OK


def check_rays(rays):
    """rmr_check_rays (no GPU): True iff rmr_trace_rays would accept the structured array."""
    r = np.ascontiguousarray(rays, np.dtype(abi.RAY_DTYPE)).reshape(-1)
    return lib().rmr_check_rays(r.ctypes.data, len(r)) == abi.RMR_OK


def check_temporal_params(params=None, **fields):
    """rmr_check_temporal_params (no GPU): True iff every field is in its range."""
    p = params if isinstance(params, abi.TemporalParams) else abi.default_temporal_params(**fields)
    return lib().rmr_check_temporal_params(C.byref(p)) == abi.RMR_OK


def check_bloom_params(params=None, **fields):
    """rmr_check_bloom_params (no GPU): True iff every field is in its range."""
    p = params if isinstance(params, abi.BloomParams) else abi.default_bloom_params(**fields)
    return lib().rmr_check_bloom_params(C.byref(p)) == abi.RMR_OK


def bloom_pixels(rgba, params=None, **fields):
    """rmr_bloom_pixels (no GPU): the whole bloom rule on an (H, W, 4) image."""
    p = params if isinstance(params, abi.BloomParams) else abi.default_bloom_params(**fields)
    a = np.ascontiguousarray(rgba, np.float32)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError("bloom_pixels: an (H, W, 4) image, got shape %r" % (a.shape,))
    out = np.zeros_like(a)
    rc = lib().rmr_bloom_pixels(C.byref(p), _fp(a), a.shape[1], a.shape[0], _fp(out))
    if rc != abi.RMR_OK:
        raise RMRError(rc, "rmr_bloom_pixels: bad params or image")
    return out


def _volume_desc(origin, spacing, shape):
    d = origin if isinstance(origin, abi.VolumeDesc) else abi.volume_desc(origin, spacing, shape)
    bad = check_volume(d)
    if bad:
        raise RMRError(-1, "bad volume descriptor field '%s'" % bad)
    return d


def check_volume(origin, spacing=None, shape=None):
    """rmr_check_volume (no GPU): None for a lattice in range (finite numbers, spacing > 0, 2 <= n <= 4096,
    at most 2^30 points), else the name of the first failing field: 'origin', 'spacing', 'n' or 'points'.
    Takes an abi.VolumeDesc or (origin, spacing, shape)."""
    d = origin if isinstance(origin, abi.VolumeDesc) else abi.volume_desc(origin, spacing, shape)
    bad = C.c_char_p()
    rc = lib().rmr_check_volume(C.byref(d), C.byref(bad))
    return None if rc == abi.RMR_OK else (bad.value or b"desc").decode()


def surface_nets(dist, origin, spacing, iso=0.0):
    """rmr_surface_nets (no GPU): the surface-nets mesh of a host volume dist[iz, iy, ix] (its shape gives the
    lattice), count then fill: (vertices (V, 3) float32, quads (Q, 4) uint32)."""
    a = np.ascontiguousarray(dist, np.float32)
    if a.ndim != 3:
        raise ValueError("surface_nets: a volume indexed [iz, iy, ix], got shape %r" % (a.shape,))
    d = _volume_desc(origin, spacing, a.shape[::-1])
    info = abi.MeshInfo()
    rc = lib().rmr_surface_nets(_fp(a), C.byref(d), C.c_float(iso), None, 0, None, 0, C.byref(info))
    if rc != abi.RMR_OK:
        raise RMRError(rc, "rmr_surface_nets: bad lattice or iso")
    v = np.zeros((int(info.n_vertices), 3), np.float32)
    q = np.zeros((int(info.n_quads), 4), np.uint32)
    if len(v):
        qp = (q if len(q) else np.zeros((1, 4), np.uint32)).ctypes.data_as(C.POINTER(C.c_uint32))
        rc = lib().rmr_surface_nets(_fp(a), C.byref(d), C.c_float(iso), _fp(v), len(v), qp, len(q), C.byref(info))
        if rc != abi.RMR_OK:
            raise RMRError(rc, "rmr_surface_nets")
    return v, q


def quads_to_triangles(quads):
    """Each quad (a, b, c, d) as the triangles (a, b, c), (a, c, d): (2 Q, 3)."""
    return np.asarray(quads)[:, [0, 1, 2, 0, 2, 3]].reshape(-1, 3)


def _mesh_arrays(vertices, quads, normals, ids):
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    q = np.ascontiguousarray(quads, np.uint32).reshape(-1, 4)
    n = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    i = None if ids is None else np.ascontiguousarray(ids, np.float32).reshape(-1)
    if (n is not None and len(n) != len(v)) or (i is not None and len(i) != len(v)):
        raise ValueError("one normal and one id per vertex")
    return v, q, n, i


def encode_obj(path, vertices, quads, normals=None):
    """rmr_encode_obj: 'v', optional 'vn', quad faces 'f a//a b//b c//c d//d' (1-based)."""
    v, q, n, _ = _mesh_arrays(vertices, quads, normals, None)
    rc = lib().rmr_encode_obj(os.fsencode(path), _fp(v), _fp(n) if n is not None else None, len(v),
                              q.ctypes.data_as(C.POINTER(C.c_uint32)), len(q))
    if rc != abi.RMR_OK:
        raise RMRError(rc, "rmr_encode_obj: %s" % path)


def encode_ply(path, vertices, quads, normals=None, ids=None, *, colors=None):
    """rmr_encode_ply: binary little-endian PLY, x y z, optional nx ny nz, optional float material, faces
    as lists of 4. colors: (V, 3) uint8 (srgb8 of a bake), written as uchar red green blue
    (rmr_encode_ply_colors)."""
    v, q, n, i = _mesh_arrays(vertices, quads, normals, ids)
    qp = q.ctypes.data_as(C.POINTER(C.c_uint32))
    if colors is None:
        rc = lib().rmr_encode_ply(os.fsencode(path), _fp(v), _fp(n) if n is not None else None,
                                  _fp(i) if i is not None else None, len(v), qp, len(q))
    else:
        c = np.ascontiguousarray(colors, np.uint8).reshape(-1, 3)
        if len(c) != len(v):
            raise ValueError("one colour per vertex")
        rc = lib().rmr_encode_ply_colors(os.fsencode(path), _fp(v), _fp(n) if n is not None else None,
                                         _fp(i) if i is not None else None, c.ctypes.data_as(C.POINTER(C.c_uint8)),
                                         len(v), qp, len(q))
    if rc != abi.RMR_OK:
        raise RMRError(rc, "rmr_encode_ply: %s" % path)


def srgb8(rgb):
    """rmr_srgb8_pixels (no GPU): the display's exact sRGB encode of an (..., 3) float array, uint8 of the same
    shape."""
    a = np.ascontiguousarray(rgb, np.float32)
    if a.ndim < 1 or a.shape[-1] != 3:
        raise ValueError("srgb8: an (..., 3) array")
    out = np.zeros(a.shape, np.uint8)
    rc = lib().rmr_srgb8_pixels(_fp(a), a.size // 3, out.ctypes.data_as(C.POINTER(C.c_uint8)))
    if rc != abi.RMR_OK:
        raise RMRError(rc, "rmr_srgb8_pixels")
    return out


def check_bake_params(params=None, **fields):
    """rmr_check_bake_params (no GPU): True iff the params are in range."""
    q = abi.bake_params(**fields) if params is None else params
    return lib().rmr_check_bake_params(C.byref(q)) == abi.RMR_OK


def bake_check_points(points, normals):
    """rmr_bake_check_points (no GPU): the first index the bake's reject rule refuses, or None."""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    n = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    if len(p) != len(n):
        raise ValueError("one normal per point")
    bad = C.c_size_t(0)
    rc = lib().rmr_bake_check_points(_fp(p), _fp(n), len(p), C.byref(bad))
    return None if rc == abi.RMR_OK else int(bad.value)


def bake_fold(L_rgb, c, cv=None):
    """rmr_bake_fold (no GPU): the bake's fold of host arrays laid out [k][i]: L_rgb (N, n, 3) or None, c (N, n),
    cv (N, n) or None; (rgba (n, 4) or None, ao (n,) or None)."""
    cc = np.ascontiguousarray(c, np.float32)
    nspp, n = cc.shape
    L = None if L_rgb is None else np.ascontiguousarray(L_rgb, np.float32).reshape(nspp, n, 3)
    v = None if cv is None else np.ascontiguousarray(cv, np.float32).reshape(nspp, n)
    rgba = np.zeros((n, 4), np.float32) if L is not None else None
    ao = np.zeros((n,), np.float32) if v is not None else None
    rc = lib().rmr_bake_fold(_fp(L) if L is not None else None, _fp(cc), _fp(v) if v is not None else None, n, nspp,
                             _fp(rgba) if rgba is not None else None, _fp(ao) if ao is not None else None)
    if rc != abi.RMR_OK:
        raise RMRError(rc, "rmr_bake_fold")
    return rgba, ao


def check_probe_params(params=None, **fields):
    """rmr_check_probe_params (no GPU): True iff the params are in range."""
    q = abi.probe_params(**fields) if params is None else params
    return lib().rmr_check_probe_params(C.byref(q)) == abi.RMR_OK


def sh_basis(dirs):
    """rmr_sh_basis (no GPU): Y_0 .. Y_8 of (..., 3) float32 unit vectors, (..., 9) float32."""
    d = np.ascontiguousarray(dirs, np.float32)
    if d.ndim < 1 or d.shape[-1] != 3:
        raise ValueError("sh_basis: an (..., 3) array")
    out = np.zeros(d.shape[:-1] + (9,), np.float32)
    rc = lib().rmr_sh_basis(_fp(d), d.size // 3, _fp(out))
    if rc != abi.RMR_OK:
        raise RMRError(rc, "rmr_sh_basis")
    return out


def probe_fold(L_rgb, dirs):
    """rmr_probe_fold (no GPU): the probes' fold and resolve of host arrays laid out [k][i], L_rgb and dirs
    (N, n, 3) float32: (n, 28) float32."""
    L = np.ascontiguousarray(L_rgb, np.float32)
    d = np.ascontiguousarray(dirs, np.float32)
    if L.ndim != 3 or L.shape[2] != 3 or d.shape != L.shape:
        raise ValueError("probe_fold: L_rgb and dirs of one shape (N, n, 3)")
    nspp, n = L.shape[:2]
    out = np.zeros((n, abi.PROBE_FLOATS), np.float32)
    rc = lib().rmr_probe_fold(_fp(L), _fp(d), n, nspp, _fp(out))
    if rc != abi.RMR_OK:
        raise RMRError(rc, "rmr_probe_fold")
    return out


def probe_irradiance_host(desc, sh, points, normals):
    """rmr_probe_irradiance_host (no GPU): the lookup over a host field, (rgba (n, 4) float32, the first
    rejected query's index or None)."""
    d = _volume_desc(desc, None, None) if isinstance(desc, abi.VolumeDesc) else _volume_desc(*desc)
    a = np.ascontiguousarray(sh, np.float32)
    if a.size != d.n[0] * d.n[1] * d.n[2] * abi.PROBE_FLOATS:
        raise ValueError("sh: 28 floats per lattice point")
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    n = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    if len(p) != len(n):
        raise ValueError("one normal per point")
    out = np.zeros((len(p), 4), np.float32)
    bad = C.c_size_t(0)
    rc = lib().rmr_probe_irradiance_host(C.byref(d), _fp(a), _fp(p), _fp(n), len(p), _fp(out), C.byref(bad))
    return out, (None if rc == abi.RMR_OK else int(bad.value))


def probe_vis_dirs():
    """rmr_probe_vis_dirs (no GPU): the 64 texel directions of a probe's visibility map, (64, 3) float32."""
    out = np.zeros((abi.PROBE_VIS_TEXELS, 3), np.float32)
    rc = lib().rmr_probe_vis_dirs(_fp(out))
    if rc != abi.RMR_OK:
        raise RMRError(rc, "rmr_probe_vis_dirs")
    return out


def probe_vis_fold(d_and_t, range):
    """rmr_probe_vis_fold (no GPU): the visibility's fold and resolve of host samples laid out [k][i], d_and_t
    (N, n, 4) float32 = (d.xyz, t): (n, 64, 2) float32."""
    a = np.ascontiguousarray(d_and_t, np.float32)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError("probe_vis_fold: d_and_t of shape (N, n, 4)")
    nspp, n = a.shape[:2]
    out = np.zeros((n, abi.PROBE_VIS_TEXELS, 2), np.float32)
    rc = lib().rmr_probe_vis_fold(_fp(a), n, nspp, float(range), _fp(out))
    if rc != abi.RMR_OK:
        raise RMRError(rc, "rmr_probe_vis_fold")
    return out


def probe_irradiance_vis_host(desc, sh, vis, points, normals, bias=0.0):
    """rmr_probe_irradiance_vis_host (no GPU): the visibility-weighted lookup over a host field and its maps,
    (rgba (n, 4) float32, the first rejected query's index or None)."""
    d = _volume_desc(desc, None, None) if isinstance(desc, abi.VolumeDesc) else _volume_desc(*desc)
    a = np.ascontiguousarray(sh, np.float32)
    npnt = d.n[0] * d.n[1] * d.n[2]
    if a.size != npnt * abi.PROBE_FLOATS:
        raise ValueError("sh: 28 floats per lattice point")
    v = np.ascontiguousarray(vis, np.float32)
    if v.size != npnt * abi.PROBE_VIS_FLOATS:
        raise ValueError("vis: 128 floats per lattice point")
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    n = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    if len(p) != len(n):
        raise ValueError("one normal per point")
    if not (np.isfinite(bias) and bias >= 0):
        raise RMRError(-1, "rmr_probe_irradiance_vis_host: bias must be finite and >= 0")
    out = np.zeros((len(p), 4), np.float32)
    bad = C.c_size_t(0)
    rc = lib().rmr_probe_irradiance_vis_host(C.byref(d), _fp(a), _fp(v), _fp(p), _fp(n), len(p), float(bias), _fp(out), C.byref(bad))
    return out, (None if rc == abi.RMR_OK else int(bad.value))


def save_probes(path, desc, sh, vis=None, vis_range=None):
    """A probe field as a file: the line 'RMRPROBES 1 nx ny nz ox oy oz spacing' (floats as %.9g), then the
    points * 28 little-endian float32 of sh. With vis ((points, 64, 2) float32) and vis_range: the line 'RMRPROBES
    2 nx ny nz ox oy oz spacing 8 range', then sh, then the points * 128 little-endian float32 of vis."""
    d = _volume_desc(desc, None, None) if isinstance(desc, abi.VolumeDesc) else _volume_desc(*desc)
    a = np.ascontiguousarray(sh, "<f4")
    npnt = d.n[0] * d.n[1] * d.n[2]
    if a.size != npnt * abi.PROBE_FLOATS:
        raise ValueError("sh: 28 floats per lattice point")
    if (vis is None) != (vis_range is None):
        raise ValueError("vis and vis_range go together")
    floats = [d.origin[0], d.origin[1], d.origin[2], d.spacing]
    tail = b""
    if vis is not None:
        v = np.ascontiguousarray(vis, "<f4")
        if v.size != npnt * abi.PROBE_VIS_FLOATS:
            raise ValueError("vis: 128 floats per lattice point")
        rng = float(np.float32(vis_range))
        if not (np.isfinite(rng) and rng > 0):
            raise ValueError("vis_range: finite and > 0")
        tail = v.tobytes()
    head = "RMRPROBES %d %d %d %d %s" % (1 if vis is None else 2, d.n[0], d.n[1], d.n[2], " ".join("%.9g" % x for x in floats))
    if vis is not None:
        head += " %d %.9g" % (abi.PROBE_VIS_RES, rng)
    with open(path, "wb") as f:
        f.write((head + "\n").encode("ascii"))
        f.write(a.tobytes())
        f.write(tail)


def load_probes(path, visibility=False):
    """(desc, sh) of a file save_probes or rmr_cli --probes wrote: an abi.VolumeDesc and (points, 28) float32.
    visibility=True: (desc, sh, vis, range), vis (points, 64, 2) float32, or None, None for a file without it."""
    with open(path, "rb") as f:
        w = f.readline().decode("ascii", "replace").split()
        v1 = len(w) == 9 and w[:2] == ["RMRPROBES", "1"]
        v2 = len(w) == 11 and w[:2] == ["RMRPROBES", "2"] and w[9] == str(abi.PROBE_VIS_RES)
        if not (v1 or v2):
            raise ValueError("%s: not a probe file (RMRPROBES 1 ... or RMRPROBES 2 ... 8 range)" % path)
        d = _volume_desc([float(v) for v in w[5:8]], float(w[8]), [int(v) for v in w[2:5]])
        npnt = d.n[0] * d.n[1] * d.n[2]
        n = npnt * abi.PROBE_FLOATS
        nv = npnt * abi.PROBE_VIS_FLOATS if v2 else 0
        raw = f.read()
    if len(raw) != 4 * (n + nv):
        raise ValueError("%s: %d payload bytes, the lattice needs %d" % (path, len(raw), 4 * (n + nv)))
    sh = np.frombuffer(raw[:4 * n], "<f4").astype(np.float32).reshape(-1, abi.PROBE_FLOATS)
    if not visibility:
        return d, sh
    if not v2:
        return d, sh, None, None
    rng = np.float32(float(w[10]))
    if not (np.isfinite(rng) and rng > 0):
        raise ValueError("%s: the visibility's range must be finite and > 0" % path)
    return d, sh, np.frombuffer(raw[4 * n:], "<f4").astype(np.float32).reshape(-1, abi.PROBE_VIS_TEXELS, 2), rng


class _DeviceArray:
    """A float32 array in the library's device memory, for torch.as_tensor (no copy); keeps its owner alive."""

    def __init__(self, ptr, shape, owner):
        self.owner = owner
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<f4", "data": (int(ptr), False),
                                         "strides": None, "version": 2}


def aov_init(n_px):
    """rmr_aov_init (no GPU): the sampled AOVs' initial state of n_px pixels, (5, n_px, 4) float32."""
    state = np.zeros((5, int(n_px), 4), np.float32)
    rc = lib().rmr_aov_init(_fp(state), int(n_px))
    if rc != abi.RMR_OK:
        raise RMRError(rc, "rmr_aov_init")
    return state


def aov_fold(state, hits):
    """rmr_aov_fold (no GPU): fold hits[k][pixel], a (nspp, n_px) structured array of abi.HIT_DTYPE (any
    shape (nspp, ...) with n_px values per sample), into a copy of the (5, n_px, 4) state, sample 0 first."""
    st = np.array(state, np.float32, order="C")
    if st.ndim != 3 or st.shape[0] != 5 or st.shape[2] != 4:
        raise ValueError("aov_fold: a (5, n_px, 4) state, got shape %r" % (st.shape,))
    n_px = st.shape[1]
    h = np.ascontiguousarray(hits, np.dtype(abi.HIT_DTYPE))
    h = h.reshape(-1, n_px) if n_px else h.reshape(0, 0)
    rc = lib().rmr_aov_fold(_fp(st), h.ctypes.data, n_px, len(h))
    if rc != abi.RMR_OK:
        raise RMRError(rc, "rmr_aov_fold: a pixel's sample count would pass 2^24")
    return st


def aov_resolve(state, max_dist):
    """rmr_aov_resolve (no GPU): the five resolved planes (5, n_px, 4) of a (5, n_px, 4) state."""
    st = np.ascontiguousarray(state, np.float32)
    if st.ndim != 3 or st.shape[0] != 5 or st.shape[2] != 4:
        raise ValueError("aov_resolve: a (5, n_px, 4) state, got shape %r" % (st.shape,))
    out = np.zeros_like(st)
    rc = lib().rmr_aov_resolve(_fp(st), st.shape[1], C.c_float(max_dist), _fp(out))
    if rc != abi.RMR_OK:
        raise RMRError(rc, "rmr_aov_resolve")
    return out


def check_tonemap_params(params=None, **fields):
    """rmr_check_tonemap_params (no GPU): True iff every field is in its range."""
    p = params if isinstance(params, abi.TonemapParams) else abi.default_tonemap_params(**fields)
    return lib().rmr_check_tonemap_params(C.byref(p)) == abi.RMR_OK


def luminance_bins(rgba):
    """rmr_luminance_bins (no GPU): the luminance bin (0..255, -1: skipped) of each RGBA pixel, (n,) int32."""
    a = np.ascontiguousarray(rgba, np.float32).reshape(-1, 4)
    out = np.zeros(len(a), np.int32)
    rc = lib().rmr_luminance_bins(_fp(a), len(a), out.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != abi.RMR_OK:
        raise RMRError(rc, "rmr_luminance_bins")
    return out


def exposure_from_histogram(hist, l_prev=None, params=None, **fields):
    """rmr_exposure_from_histogram (no GPU): l (log2 of the scale) the meter gives for a 256-bin histogram;
    l_prev: the previous state, None for none."""
    p = params if isinstance(params, abi.TonemapParams) else abi.default_tonemap_params(**fields)
    h = np.ascontiguousarray(hist, np.uint32).reshape(256)
    out = C.c_double(0.0)
    rc = lib().rmr_exposure_from_histogram(h.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(p),
                                           C.c_double(float("nan") if l_prev is None else l_prev), C.byref(out))
    if rc != abi.RMR_OK:
        raise RMRError(rc, "rmr_exposure_from_histogram: bad params")
    return out.value


def tonemap_pixels(rgba, scale, params=None, **fields):
    """rmr_tonemap_pixels (no GPU): the curve of RGBA pixels at `scale`, in the shape given."""
    p = params if isinstance(params, abi.TonemapParams) else abi.default_tonemap_params(**fields)
    a = np.ascontiguousarray(rgba, np.float32)
    out = np.zeros_like(a)
    rc = lib().rmr_tonemap_pixels(C.byref(p), C.c_float(scale), _fp(a), a.size // 4, _fp(out))
    if rc != abi.RMR_OK:
        raise RMRError(rc, "rmr_tonemap_pixels: bad params")
    return out


def temporal_view_inverse(view):
    """rmr_temporal_view_inverse (no GPU): (Minv (3, 3), k (3,)) in float64 of a 15-float history view,
    the host's part of the temporal stage's projection."""
    v = np.ascontiguousarray(view, np.float32).reshape(15)
    out = np.zeros(12, np.float64)
    rc = lib().rmr_temporal_view_inverse(_fp(v), out.ctypes.data_as(C.POINTER(C.c_double)))
    if rc != abi.RMR_OK:
        raise RMRError(rc, "rmr_temporal_view_inverse: degenerate view")
    return out[:9].reshape(3, 3), out[9:].copy()


def encode_bmp(rgba, path):
    """Graphics::SaveImage encoding of a host RGBA32F image (h, w, 4)."""
    a = np.ascontiguousarray(rgba, np.float32)
    h, w = a.shape[:2]
    rc = lib().rmr_encode_bmp(_fp(a), w, h, path.encode())
    if rc != abi.RMR_OK:
        raise RMRError(rc, "rmr_encode_bmp(%s)" % path)


def encode_pfm(rgba, path):
    """rmr_encode_pfm: a host RGBA32F image (h, w, 4) as a colour PFM (RGB float32, little-endian,
    rows bottom to top; alpha dropped). No GPU needed."""
    a = np.ascontiguousarray(rgba, np.float32)
    if a.ndim != 3 or a.shape[2] != 4 or a.shape[0] == 0 or a.shape[1] == 0:
        raise ValueError("encode_pfm: rgba must be a non-empty (h, w, 4) image, got shape %s" % (a.shape,))
    h, w = a.shape[:2]
    rc = lib().rmr_encode_pfm(_fp(a), w, h, path.encode())
    if rc != abi.RMR_OK:
        raise RMRError(rc, "rmr_encode_pfm(%s)" % path)


def adaptive_select(err, block_tiles, threshold, open_blocks=None):
    """rmr_adaptive_select (no GPU): the adaptive loop's decision rule on a (TY, TX) tile-error map.
    open_blocks: (ceil(TY / bt), ceil(TX / bt)) bools, all open without one. Returns the blocks still
    open: an open block stays open iff one of its tiles has an error > threshold."""
    err = np.ascontiguousarray(err, np.float32)
    if err.ndim != 2:
        raise ValueError("adaptive_select: err must be a (TY, TX) map, got shape %s" % (err.shape,))
    ty, tx = err.shape
    bt = int(block_tiles)
    shape = (-(-ty // max(bt, 1)), -(-tx // max(bt, 1)))
    o = np.ones(shape, np.uint8) if open_blocks is None else np.ascontiguousarray(open_blocks).astype(np.uint8).reshape(shape)
    rc = lib().rmr_adaptive_select(_fp(err), tx, ty, bt, float(threshold), o.ctypes.data_as(C.POINTER(C.c_uint8)))
    if rc < 0:
        raise RMRError(rc, "rmr_adaptive_select")
    return o.astype(bool)


# ------------------------------------------------------------------------------------------
# Reference-shaped facades
# ------------------------------------------------------------------------------------------
class Screen:
    """Screen.h:4-15 — static screen size / window position / delta time."""
    _size = (0.0, 0.0)
    _pos = (0.0, 0.0)
    _dt = 0.0

    @staticmethod
    def setScreenSize(size):
        Screen._size = tuple(size)

    @staticmethod
    def getScreenSize():
        return Screen._size

    @staticmethod
    def setWindowPos(pos):
        Screen._pos = tuple(pos)

    @staticmethod
    def getWindowPos():
        return Screen._pos

    @staticmethod
    def getDeltaTime():
        return Screen._dt

    @staticmethod
    def setDeltaTime(t):
        if t != 0:  # Screen.cpp:35-40
            Screen._dt = t


class Graphics:
    """Graphics.h:118-133 static interface over one Renderer (variant selectable; the reference
    hard-wires RayMarch3, Graphics.cpp:272)."""
    _r = None
    _materials = []
    _objects = []
    _size = (1024, 1024)
    variant = abi.RMR_VARIANT_RM3
    device = 0

    @staticmethod
    def Init():
        Graphics._r = Renderer(Graphics.device, *Graphics._size)
        Graphics.Reload()

    @staticmethod
    def _scene_dict():
        return {"materials": list(Graphics._materials), "objects": list(Graphics._objects)}

    @staticmethod
    def Reload():
        r = Graphics._r
        if Graphics.variant == abi.RMR_VARIANT_RM3:
            r.load_builtin(abi.RMR_VARIANT_RM3)
        else:
            r.load_scene(Graphics._scene_dict(), Graphics.variant)
        r.set_image_size(*Graphics._size)
        r.reload()

    @staticmethod
    def Render(currentTime, vmin, vmax, currentSample):
        Graphics._r.render(currentTime, vmin, vmax, currentSample)

    @staticmethod
    def SaveImage(path):
        Graphics._r.save_bmp(path)

    @staticmethod
    def Display(centre, zoom, vmin, vmax, screen=None):
        """Graphics::Display (Graphics.cpp:356-390) into a screen image of Screen.getScreenSize()."""
        size = tuple(int(v) for v in Screen.getScreenSize())
        return Graphics._r.display(centre, zoom, vmin, vmax, screen=screen, screen_size=size)

    @staticmethod
    def addMaterial(material):
        Graphics._materials.append(material)

    @staticmethod
    def addObject(obj):
        Graphics._objects.append(obj)

    @staticmethod
    def clearScene():
        Graphics._materials = []
        Graphics._objects = []

    @staticmethod
    def setImageSize(size):
        Graphics._size = (int(size[0]), int(size[1]))
        if Graphics._r is not None:
            Graphics._r.set_image_size(*Graphics._size)

    @staticmethod
    def getImageSize():
        return Graphics._size

    @staticmethod
    def setView(eye, ray00, ray01, ray10, ray11):
        """Same argument order as the reference (Graphics.cpp:827): uniform ray10 <- 3rd arg... note
        the reference binds the 3rd parameter (named ray01) to the uniform "ray01"."""
        v = np.array(list(eye) + list(ray00) + list(ray01) + list(ray10) + list(ray11), np.float32)
        Graphics._r.set_view(v)


class Camera:
    """Camera.h:4-32 — corner-ray camera; calculateRays() pushes the view to Graphics."""

    def __init__(self, eyePos=(0.0, 4.0, -6.0), lookDir=None, aspect=1.0, fov=None):
        if lookDir is None:
            m = math.sqrt(45.0)
            lookDir = (0.0, -3.0 / m, 6.0 / m)
        self.eye = tuple(float(x) for x in eyePos)
        self.dir = tuple(float(x) for x in lookDir)
        self.aspect = float(aspect)
        self.fov = float(np.float32(3.141592653) / np.float32(4)) if fov is None else float(fov)
        self.calculateRays()

    def setAspect(self, a):
        self.aspect = float(a)

    def calculateRays(self):
        v = camera_view(self.eye, self.dir, self.aspect, self.fov)
        # v is already in uniform order; Graphics.setView(eye, ray00, ray10, ray01, ray11) as
        # Camera.cpp:101 calls it maps to the same uniforms.
        if Graphics._r is not None:
            Graphics._r.set_view(v)
        self.view = v
        return v


def tile_spiral(gridW, gridH):
    """The outward spiral tile order of Program.cpp:113-115 / 203-222."""
    x = int(math.ceil(gridW / 2.0)) - 1
    y = int(math.ceil(gridH / 2.0)) - 1
    d = (-1, 0)
    passed, last, dist = 0, 0, 0
    order = []
    while passed < gridW * gridH:
        order.append((x, y))
        x -= gridW // 2
        y -= gridH // 2
        if dist * 2 == passed - last:
            dist += 1
            last = passed
            d = (d[1], -d[0])
        elif dist == passed - last:
            d = (d[1], -d[0])
        passed += 1
        x += d[0]
        y += d[1]
        x += gridW // 2
        y += gridH // 2
    return order


def save_name(now=None):
    """Program.cpp:71-84 file name: output\\%Y-%m-%d_%H-%M-%S.bmp."""
    t = _time.localtime(now)
    return _time.strftime("%Y-%m-%d_%H-%M-%S", t) + ".bmp"


def srgb_thresholds():
    """rmr_srgb_thresholds: the 256 linear-space decision points of the display's sRGB encode."""
    out = np.zeros(256, np.float32)
    rc = lib().rmr_srgb_thresholds(_fp(out))
    if rc != abi.RMR_OK:
        raise RMRError(rc, "rmr_srgb_thresholds")
    return out


def candidate_grid(prims, n_large, E, target=0.0, pad=0.0):
    """rmr_candidate_grid (test hook, no GPU): the nearest-primitive cache's candidate grid for
    `prims` (n x 8 float32 rows in leaf order: c.xyz, r.xyz, type, mat_id; the first n_large
    evaluated everywhere). Returns a dict with dim, lo, inv, sbox, eps, margin, cells (n_cells x 2
    uint32) and list (uint16), or None when no grid applies."""
    prims = np.ascontiguousarray(prims, np.float32)
    n = prims.shape[0]
    idims = (C.c_int32 * 5)()
    geom = np.zeros(12, np.float32)
    rc = lib().rmr_candidate_grid(_fp(prims), n, int(n_large), float(E), float(target), float(pad), idims, _fp(geom),
                                  None, 0, None, 0)
    if rc not in (abi.RMR_OK, -1):   # -1 RMR_E_INVALID: buffers not given yet (sizes returned)
        raise RMRError(rc, "rmr_candidate_grid")
    if not idims[4]:
        return None
    ncell = idims[0] * idims[1] * idims[2]
    cells = np.zeros(2 * ncell, np.uint32)
    lst = np.zeros(max(1, idims[3]), np.uint16)
    rc = lib().rmr_candidate_grid(_fp(prims), n, int(n_large), float(E), float(target), float(pad), idims, _fp(geom),
                                  cells.ctypes.data_as(C.POINTER(C.c_uint32)), cells.size,
                                  lst.ctypes.data_as(C.POINTER(C.c_uint16)), lst.size)
    if rc != abi.RMR_OK:
        raise RMRError(rc, "rmr_candidate_grid")
    return {"dim": (idims[0], idims[1], idims[2]), "lo": geom[0:3].copy(), "inv": geom[3], "sbox": geom[4:10].copy(),
            "eps": float(geom[10]), "margin": float(geom[11]), "cells": cells.reshape(-1, 2), "list": lst[:idims[3]]}
