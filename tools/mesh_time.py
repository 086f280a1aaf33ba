"""mesh_time.py — what the volume sampling and the surface-nets extraction cost.

One process, the release library, torch tensors for the device forms on a context bound to torch's stream.
Every shape is warmed up, then the configurations alternate round by round; in a round a configuration queues
--calls calls and synchronises once (a host clock around the bracket, divided by the calls); medians and the
spread (min .. max) over the rounds are reported, one JSON line per measurement (--out FILE also writes them
there). Scenes: Cornell-5 and csg256; lattices of 256^3 and 512^3 points over the box (-4, -1.2, -4) .. (4, 6.8, 4).

  * volume: rmr_sample_volume_device (the lattice kernel: nothing read, 4 bytes written per point) against the
    route there was before it, rmr_eval_map_device over an explicit list of the same points (12 bytes read, 8
    written per point; the list is built once, outside the clock), and against the write floor, 4 bytes per
    point at the running-mean fold's 5.4 TB/s;
  * extract: rmr_extract_mesh as a whole (its sampling, count, scan, the synchronisation for the counts, the
    exact allocations, vertices, quads and attributes), without and with normals and ids; one call per bracket.

--kernels-only runs each device call twice and exits: the run to put under a kernel trace, which gives each
extraction kernel's own time.
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

from raymarchrenderer_amd import Renderer, abi  # noqa: E402

SCENES = os.path.join(ROOT, "scenes")
FOLD_TBPS = 5.4   # the running-mean fold's measured rate, the yardstick for a streaming kernel
LO, SIDE = (-4.0, -1.2, -4.0), 8.0


def point_list(torch, desc):
    """The lattice's points as an (n, 3) float32 tensor, x fastest: origin + float32(i) * spacing in float32
    (torch rounds the product, then the sum, as the kernel does)."""
    ax = [torch.tensor(desc.origin[a], dtype=torch.float32, device="cuda") +
          torch.arange(desc.n[a], dtype=torch.float32, device="cuda") * torch.tensor(desc.spacing, dtype=torch.float32, device="cuda")
          for a in range(3)]
    z, y, x = torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return torch.stack([x, y, z], dim=-1).reshape(-1, 3).contiguous()


def stat(v):
    return {"ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--scenes", default="cornell5.scene,csg256.scene")
    ap.add_argument("--out", default="")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--lib", default="", help="another build of the library (csrc/Makefile: make lib BUILD=.. OUT=.. EXTRA=..)")
    a = ap.parse_args()
    import torch
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for scene in a.scenes.split(","):
            r = Renderer(0, 64, 64, diag=a.lib or None)
            r.load_scene(os.path.join(SCENES, scene), "rm1")
            r.set_stream(stream.cuda_stream)
            L, ctx = r.lib, r.ctx
            for size in [int(s) for s in a.sizes.split(",")]:
                desc = abi.volume_desc(LO, SIDE / (size - 1), (size, size, size))
                n = size ** 3
                pts = point_list(torch, desc)
                dist = torch.empty(n, dtype=torch.float32, device="cuda")
                pair = torch.empty((n, 2), dtype=torch.float32, device="cuda")
                info = abi.MeshInfo()
                bare, full = abi.MeshParams(0.0, 0), abi.MeshParams(0.0, abi.MESH_NORMALS | abi.MESH_IDS)

                def ok(rc):
                    if rc != abi.RMR_OK:
                        raise RuntimeError(L.rmr_last_error(ctx).decode())

                runs = {
                    ("volume", "lattice"): (a.calls, lambda: ok(L.rmr_sample_volume_device(ctx, C.byref(desc), dist.data_ptr(), None))),
                    ("volume", "point_list"): (a.calls, lambda: ok(L.rmr_eval_map_device(ctx, pts.data_ptr(), n, pair.data_ptr()))),
                    ("extract", "bare"): (1, lambda: ok(L.rmr_extract_mesh(ctx, C.byref(desc), C.byref(bare), C.byref(info)))),
                    ("extract", "normals_ids"): (1, lambda: ok(L.rmr_extract_mesh(ctx, C.byref(desc), C.byref(full), C.byref(info)))),
                }
                # the two routes give the same distances
                runs[("volume", "lattice")][1]()
                runs[("volume", "point_list")][1]()
                r.sync()
                assert torch.equal(dist.view(torch.int32), pair[:, 0].contiguous().view(torch.int32)), "the routes differ"
                if a.kernels_only:
                    for calls, fn in runs.values():
                        fn()
                        fn()
                    r.sync()
                    continue
                res = {key: [] for key in runs}
                for rnd in range(a.rounds + 1):
                    for key, (calls, fn) in runs.items():
                        r.sync()
                        t0 = time.perf_counter()
                        for _ in range(calls):
                            fn()
                        r.sync()
                        if rnd:   # round 0 is the warm-up (first allocations)
                            res[key].append((time.perf_counter() - t0) * 1e3 / calls)
                for (what, form), v in res.items():
                    d = {"what": what, "form": form, "scene": scene, "size": size, "points": n, "rounds": a.rounds,
                         "calls_per_sync": runs[(what, form)][0]}
                    d.update(stat(v))
                    d["all_ms"] = [round(x, 3) for x in v]
                    d["gpoints_per_s"] = round(n / d["ms"] / 1e6, 3)
                    if what == "volume":
                        d["write_floor_ms"] = round(n * 4 / (FOLD_TBPS * 1e9), 4)
                        d["bytes_moved"] = n * (4 if form == "lattice" else 20)
                    else:
                        d["vertices"], d["quads"] = int(info.n_vertices), int(info.n_quads)
                    emit(d)
                lat, lst = stat(res[("volume", "lattice")]), stat(res[("volume", "point_list")])
                emit({"what": "volume_compare", "scene": scene, "size": size, "lattice_ms": lat["ms"], "point_list_ms": lst["ms"],
                      "lattice_over_point_list": round(lat["ms"] / lst["ms"], 4),
                      "lattice_spread_ms": round(lat["max_ms"] - lat["min_ms"], 4),
                      "point_list_spread_ms": round(lst["max_ms"] - lst["min_ms"], 4)})
                del pts, dist, pair
                r.mesh_free()
            r.close()
    if a.out:
        with open(a.out, "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
