"""rays_time.py — what the ray-source trace kernels cost.

One process, the release library, the hipRTC kernels (rmr_set_jit 1). After a warm-up the configurations
alternate round by round and the median over the rounds is reported, one JSON line per measurement
(--out FILE also writes them there):

  * price: C2's frame (Cornell-5, 1920x1080, 16 spp, 4 bounces) with RMR_CAMERA_VIEW (lane slots, the
    eye step, batch probes) and with a thin lens of aperture 0 (the same image through the generator and the
    ray-source kernel): the frame's wall time between two rmr_sync, the trace kernel's event time
    (rmr_stats.trace_ms; the generator runs before the first event), the fold's, and the rest of the
    wall time (under the model: the generator and the launch gaps), beside the ray buffer's bytes;
    --models adds frames of the other models (another image each);
  * trace_rays: one rmr_trace_rays call of 2^20 rays (a 1024x1024 image's primary rays, from
    rmr_camera_rays) on C2's scene and on csg256: the call's wall time, the kernel's event time, the rest
    (packing the records, the upload, the readback), and rays per second on both.

--kernels-only renders one frame of each kind and one trace_rays call and exits: the run to put under a
kernel trace, whose per-kernel times (k_camera_rays, rmr_jit_trace, rmr_jit_trace_rays) are the
kernel-side figures.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from raymarchrenderer_amd import Renderer, abi, default_camera_view, time_schedule  # noqa: E402

SCENES = os.path.join(ROOT, "scenes")
MODELS = {"view": ("view", {}), "thinlens0": ("thinlens", dict(aperture=0.0, focus=6.0)),
          "thinlens": ("thinlens", dict(aperture=0.15, focus=6.0)), "equirect": ("equirect", {}),
          "ortho": ("ortho", dict(width=8.0, height=4.5))}


def setup(W, H, scene="cornell5.scene"):
    r = Renderer(0, W, H)
    r.set_jit(1)
    r.load_scene(os.path.join(SCENES, scene), "rm1")
    r.set_params(abi.default_params(max_bounces=4))
    r.set_view(default_camera_view(W, H))
    return r


def frame(r, times, model):
    """One frame under a model; (wall ms, trace ms, fold ms)."""
    name, fields = MODELS[model]
    r.set_camera_model(name, **fields)
    r.reload()
    r.reset_stats()
    r.sync()
    t0 = time.perf_counter()
    r.render_spp(times)
    r.sync()
    wall = (time.perf_counter() - t0) * 1e3
    s = r.stats()
    return wall, s.trace_ms, s.fold_ms


def traced(r, rays):
    r.reset_stats()
    r.sync()
    t0 = time.perf_counter()
    r.trace_rays(rays)
    wall = (time.perf_counter() - t0) * 1e3
    return wall, r.stats().trace_ms


def med(v):
    return round(statistics.median(v), 4)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--models", default="view,thinlens0", help="frames to alternate (view, thinlens0, thinlens, equirect, ortho)")
    ap.add_argument("--out", default="")
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    models = a.models.split(",")
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    W, H = 1920, 1080
    times = time_schedule(a.spp)
    r = setup(W, H)
    if a.kernels_only:
        for m in models:
            frame(r, times, m)
            frame(r, times, m)
        r.close()
        r = setup(1024, 1024)
        rays = r.camera_rays(time_schedule(1))
        r.trace_rays(rays)
        r.trace_rays(rays)
        r.close()
        return
    runs = {m: [] for m in models}
    for rnd in range(a.rounds + 1):
        for m in models:
            v = frame(r, times, m)
            if rnd:   # round 0 is the warm-up (hipRTC compiles, first allocations)
                runs[m].append(v)
    units = ((W + 7) // 8) * ((H + 7) // 8) * 64 * a.spp
    for m in models:
        v = runs[m]
        emit({"what": "price", "model": m, "W": W, "H": H, "spp": a.spp, "wall_ms": med([x[0] for x in v]),
              "wall_ms_all": [round(x[0], 3) for x in v], "trace_ms": med([x[1] for x in v]), "fold_ms": med([x[2] for x in v]),
              "rest_ms": med([x[0] - x[1] - x[2] for x in v]), "ray_buffer_bytes": 0 if m == "view" else units * 48,
              "sample_plane_bytes": units * 16})
    r.close()
    for scene in ("cornell5.scene", "csg256.scene"):
        r = setup(1024, 1024, scene)
        rays = r.camera_rays(time_schedule(1))
        v = [traced(r, rays) for _ in range(a.rounds + 1)][1:]
        n = rays.size
        wall, kern = med([x[0] for x in v]), med([x[1] for x in v])
        emit({"what": "trace_rays", "scene": scene, "rays": n, "call_ms": wall, "call_ms_all": [round(x[0], 3) for x in v],
              "kernel_ms": kern, "pack_upload_readback_ms": round(wall - kern, 4), "upload_bytes": n * 48, "readback_bytes": n * 16,
              "mrays_per_s_call": round(n / wall / 1e3, 2), "mrays_per_s_kernel": round(n / kern / 1e3, 2)})
        r.close()
    if a.out:
        with open(a.out, "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
