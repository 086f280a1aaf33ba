"""bake_time.py — what a light bake costs beside the route there was before it.

One process, the diagnostic library (the same kernels as the release one, plus rmr_diag_bake_kernels), torch
tensors on a context bound to torch's stream. The workload: the vertices and normals of a scene's surface-nets
mesh at --mesh-grid cells (csg_nodes and Cornell-5 at 256), --seeds seeds, the radiance flag only, the rays'
origins lifted by 0.002 + spacing / 8 as rmr_cli --mesh-bake does. Everything is warmed up, then the three
configurations alternate round by round; a configuration queues its call and synchronises once (a host clock
around the bracket); medians and the spread (min .. max) over the rounds are reported, one JSON line per
measurement (--out FILE also writes them there):

  * bake:     rmr_bake_points_device (k_bake_rays, the ray-source trace kernel, k_bake_fold per launch);
  * trace:    rmr_trace_rays_device on the same rays as an rmr_ray list, produced once beforehand by
              rmr_bake_rays_device, outside the clock: what there was before the bake, once someone had built the
              rays (k_pack_rays, the same trace kernel, k_unpack_rgba; the fold over k is still to do);
  * kernels:  k_bake_rays and k_bake_fold alone over the bake's launches (rmr_diag_bake_kernels).

The bake's result is checked against the fold (in torch, float32, in ascending k) of the trace's samples with the
rays' own cosines before anything is timed. --kernels-only runs each configuration twice and exits: the run to
put under a kernel trace.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from raymarchrenderer_amd import Renderer, abi, time_schedule  # noqa: E402

SCENES = os.path.join(ROOT, "scenes")
BOXES = {"csg_nodes.scene": ((-4.0, -1.2, -4.0), 8.0), "cornell5.scene": ((-4.0, -1.2, -4.0), 8.0)}


def stat(v):
    return {"ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seeds", type=int, default=16)
    ap.add_argument("--mesh-grid", type=int, default=256)
    ap.add_argument("--scenes", default="csg_nodes.scene,cornell5.scene")
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--out", default="")
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    import torch
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    times = np.ascontiguousarray(time_schedule(a.seeds, frame=1), np.float32)
    tp = times.ctypes.data_as(C.POINTER(C.c_float))
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for scene in a.scenes.split(","):
            r = Renderer(0, 64, 64, diag=True)
            r.load_scene(os.path.join(SCENES, scene), "rm1")
            r.set_params(abi.default_params(max_bounces=a.bounces))
            r.set_stream(stream.cuda_stream)
            L, ctx = r.lib, r.ctx
            lo, side = BOXES.get(scene, ((-4.0, -1.2, -4.0), 8.0))
            spacing = side / a.mesh_grid
            size = a.mesh_grid + 1
            r.extract_mesh(lo, spacing, (size, size, size), ids=False)
            mesh = r.mesh_device()
            v, nrm = mesh["vertices"].clone(), mesh["normals"].clone()
            r.sync()
            r.mesh_free()
            n = v.shape[0]
            bias = 0.002 + spacing / 8
            extent = float(v.abs().max().item()) + 2 * bias
            q = abi.bake_params(bias=bias, origin_extent=extent)
            rays = r.bake_rays_device(v, nrm, times, params=q)                  # (seeds * n, 10)
            rgba = torch.empty((n, 4), dtype=torch.float32, device="cuda")
            samples = torch.empty((a.seeds * n, 4), dtype=torch.float32, device="cuda")
            scratch = torch.empty((n, 4), dtype=torch.float32, device="cuda")

            def ok(rc):
                if rc != abi.RMR_OK:
                    raise RuntimeError(L.rmr_last_error(ctx).decode())

            runs = {
                "bake": lambda: ok(L.rmr_bake_points_device(ctx, v.data_ptr(), nrm.data_ptr(), n, tp, a.seeds, C.byref(q),
                                                            rgba.data_ptr(), None)),
                "trace": lambda: ok(L.rmr_trace_rays_device(ctx, rays.data_ptr(), a.seeds * n, extent, samples.data_ptr())),
                "kernels": lambda: ok(L.rmr_diag_bake_kernels(ctx, v.data_ptr(), nrm.data_ptr(), n, tp, a.seeds, C.byref(q),
                                                              scratch.data_ptr())),
            }
            # the two routes give the same bytes: the trace's samples folded with the rays' cosines, in ascending k
            runs["bake"]()
            runs["trace"]()
            r.sync()
            rejects = r.query_rejects()
            d = rays.view(a.seeds, n, 10)[:, :, 4:7]
            c = torch.addcmul(torch.addcmul(nrm[None, :, 0] * d[:, :, 0], nrm[None, :, 1], d[:, :, 1]), nrm[None, :, 2], d[:, :, 2])
            s4 = samples.view(a.seeds, n, 4)
            used = (rays.view(a.seeds, n, 10).view(torch.int32)[:, :, 8] >= 0) & torch.isfinite(s4[:, :, :3]).all(dim=2)
            # (addcmul may or may not fuse as the kernel's fma does: the check is to a relative 1e-5, not to the bit;
            # tests/test_gpu_bake.py has the bit-for-bit comparison)
            S = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
            cnt = torch.zeros(n, dtype=torch.float32, device="cuda")
            for k in range(a.seeds):
                S = torch.where(used[k][:, None], S + s4[k, :, :3] * c[k].clamp(min=0)[:, None], S)
                cnt = cnt + used[k].float()
            want = torch.where(cnt[:, None] > 0, (S + S) / cnt.clamp(min=1)[:, None], torch.zeros_like(S))
            err = float(((rgba[:, :3] - want).abs() / (want.abs() + 1e-3)).max().item())
            assert err < 1e-4 and torch.equal(rgba[:, 3], cnt), "the routes differ: %g" % err
            if a.kernels_only:
                for fn in runs.values():
                    fn()
                    fn()
                r.sync()
                r.close()
                continue
            res = {key: [] for key in runs}
            for rnd in range(a.rounds + 1):
                for key, fn in runs.items():
                    r.sync()
                    t0 = time.perf_counter()
                    fn()
                    r.sync()
                    if rnd:   # round 0 is the warm-up (first allocations, the hipRTC kernel)
                        res[key].append((time.perf_counter() - t0) * 1e3)
            out = {"what": "bake_time", "scene": scene, "mesh_grid": a.mesh_grid, "vertices": n, "seeds": a.seeds,
                   "rays": a.seeds * n, "rejected_points": rejects, "rounds": a.rounds, "max_rel_diff_of_the_routes": err}
            for key, val in res.items():
                s = stat(val)
                out[key + "_ms"], out[key + "_min_ms"], out[key + "_max_ms"] = s["ms"], s["min_ms"], s["max_ms"]
            out["bake_over_trace"] = round(out["bake_ms"] / out["trace_ms"], 4)
            out["bake_over_trace_plus_kernels"] = round(out["bake_ms"] / (out["trace_ms"] + out["kernels_ms"]), 4)
            out["mrays_per_s"] = round(a.seeds * n / out["bake_ms"] / 1e3, 2)
            emit(out)
            del v, nrm, rays, rgba, samples, scratch
            r.close()
    if a.out:
        with open(a.out, "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
