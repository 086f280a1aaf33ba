"""probe_vis_time.py — what the probes' visibility costs and what it gives.

One process, Cornell-5 at 4 bounces, tools/probe_time.py's --grid^3 field over the room at --seeds seeds. One JSON
line per measurement (--out FILE also writes them there):

  * bake:     rmr_bake_probe_field_visibility over the field at --seeds seeds (a host clock around the queued call
              and one synchronisation); median and the spread;
  * lookup:   rmr_probe_irradiance_vis_device beside rmr_probe_irradiance_device at --queries queries (uniform in
              the box, random unit normals), alternating round by round in this process, and their ratio;
  * quality:  probe_time.py's experiment (the first hits of 64 rays from (0, 1.5, 0) against bake_points at 1024
              seeds) with the plain lookup and with visibility=True at each --bias (in spacings): the relative RMS
              difference over all points and over those off the emitter, and the values on the emitter's underside.

--kernels-only bakes the visibility three times and exits: the run to put under a kernel trace (the cast and the
fold appear under their own names).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from raymarchrenderer_amd import Renderer, abi, time_schedule  # noqa: E402

BOX_LO, BOX_SIDE = (-2.8, -0.8, -2.8), 5.6


def stat(v):
    return {"ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seeds", type=int, default=256)
    ap.add_argument("--grid", type=int, default=16)
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--bias", type=float, nargs="*", default=[0.0, 0.25], help="in spacings")
    ap.add_argument("--out", default="")
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    import torch
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    times = np.ascontiguousarray(time_schedule(a.seeds, frame=1), np.float32)
    r = Renderer(0, 64, 64)
    r.load_scene(os.path.join(ROOT, "scenes", "cornell5.scene"), "rm1")
    r.set_params(abi.default_params(max_bounces=a.bounces))
    spacing = BOX_SIDE / (a.grid - 1)
    desc = abi.volume_desc(BOX_LO, spacing, (a.grid,) * 3)
    r.bake_probe_field(desc, times=times)
    r.bake_probe_field_visibility(times)          # warm-up (first allocations)
    r.sync()
    if a.kernels_only:
        for _ in range(3):
            r.bake_probe_field_visibility(times)
        r.sync()
        r.close()
        return
    t = []
    for _ in range(a.rounds):
        r.sync()
        t0 = time.perf_counter()
        r.bake_probe_field_visibility(times)
        r.sync()
        t.append((time.perf_counter() - t0) * 1e3)
    vis, rng = r.read_probe_field_visibility()
    valid = r.read_probe_field()[1][:, 27] > 0
    emit({"what": "probe_vis_bake", "grid": a.grid, "probes": a.grid ** 3, "valid_probes": int(valid.sum()), "seeds": a.seeds,
          "casts": int(valid.sum()) * a.seeds, "rounds": a.rounds, "range": float(rng), **stat(t),
          "texels_at_range": int((vis[valid, :, 0] == rng).sum()), "mean_m1": round(float(vis[valid, :, 0].mean()), 4)})

    # the lookups' rates, alternating
    rs = np.random.default_rng(1)
    q = rs.uniform(np.array(BOX_LO), np.array(BOX_LO) + BOX_SIDE, (a.queries, 3)).astype(np.float32)
    v = rs.normal(size=(a.queries, 3))
    nr = (v / np.linalg.norm(v, axis=1)[:, None]).astype(np.float32)
    dq, dn = torch.from_numpy(q).cuda(), torch.from_numpy(nr).cuda()
    torch.cuda.synchronize()
    res = {"plain": [], "visibility": []}
    for rnd in range(a.rounds + 1):
        for name in res:
            r.sync()
            t0 = time.perf_counter()
            r.probe_irradiance_device(dq, dn, visibility=name == "visibility")
            r.sync()
            if rnd:
                res[name].append((time.perf_counter() - t0) * 1e3)
    sp, sv = stat(res["plain"]), stat(res["visibility"])
    emit({"what": "probe_vis_lookup", "queries": a.queries, "plain": sp, "visibility": sv,
          "visibility_over_plain": round(sv["ms"] / sp["ms"], 3), "gqueries_per_s": round(a.queries / sv["ms"] / 1e6, 3),
          "plain_gqueries_per_s": round(a.queries / sp["ms"] / 1e6, 3), "rejected": r.query_rejects()})

    # the quality experiment of probe_time.py, with and without the weights
    j = np.arange(64) + 0.5
    y, phi = 1 - 2 * j / 64, j * np.pi * (3 - np.sqrt(5))
    d = np.stack([np.sqrt(1 - y * y) * np.cos(phi), y, np.sqrt(1 - y * y) * np.sin(phi)], axis=1)
    rays = np.zeros(64, np.dtype(abi.RAY_DTYPE))
    rays["o"], rays["d"] = (0.0, 1.5, 0.0), d.astype(np.float32)
    hits = r.cast_rays(rays)
    keep = hits["id"] >= 0
    p, n = hits["pos"][keep], hits["n"][keep]
    want = r.bake_points(p, n, time_schedule(1024, frame=1))["rgba"][:, :3].astype(np.float64)
    lit = hits["id"][keep] != 3          # (material 3 is the emissive panel: its underside sees only the dim room)
    every = np.ones(len(p), bool)

    def rel_rms(x, sel):
        return round(float(np.sqrt(((x[sel] - want[sel]) ** 2).mean() / (want[sel] ** 2).mean())), 4)

    def report(name, got, bias):
        got = got[:, :3].astype(np.float64)
        emit({"what": "probe_vis_quality", "lookup": name, "bias_spacings": bias, "bias": round(bias * spacing, 5),
              "points": int(keep.sum()), "points_off_the_emitter": int(lit.sum()), "bake_seeds": 1024, "field_seeds": a.seeds,
              "grid": a.grid, "relative_rms_difference": rel_rms(got, every),
              "relative_rms_difference_off_the_emitter": rel_rms(got, lit),
              "underside": [round(float(x), 3) for x in got[~lit].mean(axis=1)],
              "underside_bake": [round(float(x), 3) for x in want[~lit].mean(axis=1)]})

    report("plain", r.probe_irradiance(p, n), 0.0)
    for b in a.bias:
        report("visibility", r.probe_irradiance(p, n, visibility=True, bias=b * spacing), b)
    r.close()
    if a.out:
        with open(a.out, "w") as f:
            for dline in lines:
                f.write(json.dumps(dline) + "\n")


if __name__ == "__main__":
    main()
