"""query_time.py — what the first-hit / distance queries and the device-resident ray list cost
(DESIGN.md §4.10).

One process, the release library, the hipRTC trace kernels (rmr_set_jit 1), torch tensors for the device
forms on a context bound to torch's stream. Every shape is warmed up, then the configurations alternate
round by round; medians and the spread (min .. max) over the rounds are reported, one JSON line per
measurement (--out FILE also writes them there). Every timing is a host clock around work that ends in a
synchronise of the context's stream. Scenes: C2's (Cornell-5) and csg256; lists of 2^20 rays.

  * trace: rmr_trace_rays (host list: pack on one thread, two staged copies) against
    rmr_trace_rays_device (k_pack_rays, the same trace kernel, k_unpack_rgba) on the same list;
  * cast: rmr_cast_rays_device on an incoherent list (random origins in and around the scene, random
    directions) and a coherent one (rmr_camera_rays of a 1024x1024 view), with and without normals, in
    rays per second; beside it the cast of the view's pixel-centre rays against rmr_render_guides of the
    same image;
  * eval: rmr_eval_map_device in points per second, and its bytes (20 per point) over its time.

--kernels-only runs each device call twice and exits: the run to put under a kernel trace, which splits
the device trace call into k_pack_rays, the trace kernel and k_unpack_rgba.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from raymarchrenderer_amd import Renderer, abi, default_camera_view, time_schedule  # noqa: E402

SCENES = os.path.join(ROOT, "scenes")
W = H = 1024
N = W * H
FOLD_TBPS = 5.4   # the running-mean fold's measured rate, the yardstick for a streaming kernel


def setup(scene, torch, stream):
    r = Renderer(0, W, H)
    r.set_jit(1)
    r.load_scene(os.path.join(SCENES, scene), "rm1")
    r.set_params(abi.default_params(max_bounces=4))
    r.set_view(default_camera_view(W, H))
    r.set_stream(stream.cuda_stream)
    return r


def incoherent(r, coherent, seed=7):
    """2^20 rays in the style of the tests' list: origins in and around the box of the view's first hits,
    every fourth far outside (3 to 300 extents away, every eighth of them aimed at the scene); random
    directions; fresh chains with varied invocations and seeds."""
    rng = np.random.default_rng(seed)
    hits = r.cast_rays(coherent[::16], normals=False)
    pos = hits["pos"][hits["id"] >= 0]
    lo, hi = pos.min(axis=0).astype(np.float64), pos.max(axis=0).astype(np.float64)
    ext = float(np.abs([lo, hi]).max())
    o = rng.uniform(lo - 0.5, hi + 0.5, (N, 3))
    d = rng.normal(size=(N, 3))
    far = np.arange(N) % 4 == 3
    u = rng.normal(size=(N, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    o[far] = (u * ext * 10.0 ** rng.uniform(0.5, 2.5, (N, 1)))[far]
    aimed = np.arange(N) % 8 == 3
    d[aimed] = (rng.uniform(lo, hi, (N, 3)) - o)[aimed]
    d /= np.linalg.norm(d, axis=1)[:, None]
    rays = np.zeros(N, np.dtype(abi.RAY_DTYPE))
    rays["o"], rays["d"] = o.astype(np.float32), d.astype(np.float32)
    rays["gx"], rays["gy"] = rng.integers(0, 2000, N), rng.integers(0, 1200, N)
    rays["time"] = rng.uniform(0, 2000, N).astype(np.float32)
    return rays


def pixel_centre_rays(r):
    r.render_guides()
    rays = np.zeros(N, np.dtype(abi.RAY_DTYPE))
    rays["o"] = default_camera_view(W, H)[:3]
    rays["d"] = r.read_guide("ray")[..., :3].reshape(-1, 3)
    return rays


def timed(r, fn):
    r.sync()
    t0 = time.perf_counter()
    fn()
    r.sync()
    return (time.perf_counter() - t0) * 1e3


def stat(v):
    return {"ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--scenes", default="cornell5.scene,csg256.scene")
    a = ap.parse_args()
    import torch
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for scene in a.scenes.split(","):
            r = setup(scene, torch, stream)
            coh = r.camera_rays(time_schedule(1)).reshape(-1)
            lists = {"coherent": coh, "incoherent": incoherent(r, coh)}
            dev = {k: torch.from_numpy(v.view(np.uint8).reshape(N, 40).copy()).cuda() for k, v in lists.items()}
            ext = {k: float(np.abs(v["o"]).max()) for k, v in lists.items()}
            rgba = torch.empty((N, 4), dtype=torch.float32, device="cuda")
            hit = torch.empty((N, 8), dtype=torch.float32, device="cuda")
            pts = torch.from_numpy(np.ascontiguousarray(lists["incoherent"]["o"])).cuda()
            dist = torch.empty((N, 2), dtype=torch.float32, device="cuda")
            centre = pixel_centre_rays(r)
            d_centre = torch.from_numpy(centre.view(np.uint8).reshape(N, 40).copy()).cuda()

            runs = {}
            for k in lists:
                runs[("trace", "host", k)] = lambda k=k: r.trace_rays(lists[k])
                runs[("trace", "device", k)] = lambda k=k: r.trace_rays_device(dev[k], ext[k], out=rgba)
                for normals in (True, False):
                    runs[("cast", "normals" if normals else "visibility", k)] = \
                        lambda k=k, normals=normals: r.cast_rays_device(dev[k], normals=normals, out=hit)
            runs[("cast", "normals", "pixel_centres")] = lambda: r.cast_rays_device(d_centre, out=hit)
            runs[("guides", "render_guides", "pixel_centres")] = lambda: r.render_guides()
            runs[("eval", "device", "incoherent_origins")] = lambda: r.eval_map_device(pts, out=dist)
            if a.kernels_only:
                for key, fn in runs.items():
                    if key[1] != "host":
                        timed(r, fn)
                        timed(r, fn)
                r.close()
                continue
            res = {key: [] for key in runs}
            for rnd in range(a.rounds + 1):
                for key, fn in runs.items():
                    t = timed(r, fn)
                    if rnd:   # round 0 is the warm-up (hipRTC compiles, first allocations)
                        res[key].append(t)
            assert r.query_rejects() == 0
            for (what, form, lst), v in res.items():
                d = {"what": what, "form": form, "list": lst, "scene": scene, "n": N, "rounds": a.rounds}
                d.update(stat(v))
                d["all_ms"] = [round(x, 3) for x in v]
                d["m_per_s"] = round(N / d["ms"] / 1e3, 2)
                if what == "eval":
                    d["bytes"] = N * 20
                    d["tb_per_s"] = round(N * 20 / d["ms"] / 1e9, 4)
                    d["share_of_fold_rate"] = round(d["tb_per_s"] / FOLD_TBPS, 4)
                emit(d)
            # the acceptance of the device list: below the host form by more than the host form's spread
            for k in lists:
                h, dv = stat(res[("trace", "host", k)]), stat(res[("trace", "device", k)])
                emit({"what": "trace_accept", "scene": scene, "list": k, "host_ms": h["ms"], "host_spread_ms": round(h["max_ms"] - h["min_ms"], 4),
                      "device_ms": dv["ms"], "accepted": bool(h["ms"] - dv["ms"] > h["max_ms"] - h["min_ms"])})
            r.close()
    if a.out:
        with open(a.out, "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
