"""probe_time.py — what an irradiance probe field costs and what it gives.

One process, the diagnostic library (the same kernels as the release one, plus rmr_diag_probe_fold), Cornell-5 at
4 bounces, a --grid^3 field over the room at --seeds seeds. One JSON line per measurement (--out FILE also writes
them there):

  * fold:     rmr_bake_probe_field with the fold mapped one thread per (probe, basis function) and one thread per
              probe, alternating round by round in this process (a host clock around the queued call and one
              synchronisation); medians and the spread; the two fields are compared bytewise first;
  * lookup:   rmr_probe_irradiance_device at --queries queries (uniform in the box, random unit normals), queries
              per second and the bytes a query must move (24 in, 16 out; the eight corners' 896 are cache hits
              where queries share cells);
  * quality:  at 64 surface points (the first hits of 64 rays from (0, 1.5, 0)), probe_irradiance from the field
              against bake_points at the same points and normals with 1024 seeds, as a relative RMS difference.

--kernels-only bakes the field twice per mapping and exits: the run to put under a kernel trace (the ray source,
the trace kernel and the two fold kernels appear under their own names).
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

from raymarchrenderer_amd import Renderer, abi, sh_basis, time_schedule  # noqa: E402

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
    ap.add_argument("--out", default="")
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    import torch
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    times = np.ascontiguousarray(time_schedule(a.seeds, frame=1), np.float32)
    r = Renderer(0, 64, 64, diag=True)
    r.load_scene(os.path.join(ROOT, "scenes", "cornell5.scene"), "rm1")
    r.set_params(abi.default_params(max_bounces=a.bounces))
    desc = abi.volume_desc(BOX_LO, BOX_SIDE / (a.grid - 1), (a.grid,) * 3)
    mappings = {"per_pair": 1, "per_probe": 2}

    def bake(mapping):
        if r.lib.rmr_diag_probe_fold(r.ctx, mapping) != abi.RMR_OK:
            raise RuntimeError("rmr_diag_probe_fold")
        r.bake_probe_field(desc, times=times)

    fields = {}
    for name, m in mappings.items():       # warm-up (first allocations, the hipRTC kernel) and the comparison
        bake(m)
        fields[name] = r.read_probe_field()[1]
    assert fields["per_pair"].tobytes() == fields["per_probe"].tobytes(), "the two mappings' fields differ"
    if a.kernels_only:
        for m in mappings.values():
            bake(m)
            bake(m)
        r.sync()
        r.close()
        return
    res = {name: [] for name in mappings}
    for _ in range(a.rounds):
        for name, m in mappings.items():
            r.sync()
            t0 = time.perf_counter()
            bake(m)
            r.sync()
            res[name].append((time.perf_counter() - t0) * 1e3)
    out = {"what": "probe_fold", "grid": a.grid, "probes": a.grid ** 3, "seeds": a.seeds, "rays": a.grid ** 3 * a.seeds,
           "rounds": a.rounds, "valid_probes": int((fields["per_pair"][:, 27] > 0).sum())}
    for name, v in res.items():
        s = stat(v)
        out[name + "_ms"], out[name + "_min_ms"], out[name + "_max_ms"] = s["ms"], s["min_ms"], s["max_ms"]
    out["per_probe_over_per_pair"] = round(out["per_probe_ms"] / out["per_pair_ms"], 4)
    emit(out)

    # the lookup's rate
    bake(0)
    rng = np.random.default_rng(1)
    q = rng.uniform(np.array(BOX_LO), np.array(BOX_LO) + BOX_SIDE, (a.queries, 3)).astype(np.float32)
    v = rng.normal(size=(a.queries, 3))
    nr = (v / np.linalg.norm(v, axis=1)[:, None]).astype(np.float32)
    dq, dn = torch.from_numpy(q).cuda(), torch.from_numpy(nr).cuda()
    torch.cuda.synchronize()
    t = []
    for rnd in range(a.rounds + 1):
        r.sync()
        t0 = time.perf_counter()
        res_q = r.probe_irradiance_device(dq, dn)
        r.sync()
        if rnd:
            t.append((time.perf_counter() - t0) * 1e3)
    s = stat(t)
    emit({"what": "probe_lookup", "queries": a.queries, **s, "gqueries_per_s": round(a.queries / s["ms"] / 1e6, 3),
          "in_out_bytes_per_query": 40, "gathered_bytes_per_query": 8 * 112,
          "in_out_gb_per_s": round(a.queries * 40 / s["ms"] / 1e6, 1), "rejected": r.query_rejects(),
          "mean_weight": round(float(res_q[:, 3].mean().item()), 4)})

    # one quality number
    j = np.arange(64) + 0.5
    y, phi = 1 - 2 * j / 64, j * np.pi * (3 - np.sqrt(5))
    d = np.stack([np.sqrt(1 - y * y) * np.cos(phi), y, np.sqrt(1 - y * y) * np.sin(phi)], axis=1)
    rays = np.zeros(64, np.dtype(abi.RAY_DTYPE))
    rays["o"], rays["d"] = (0.0, 1.5, 0.0), d.astype(np.float32)
    hits = r.cast_rays(rays)
    keep = hits["id"] >= 0
    p, n = hits["pos"][keep], hits["n"][keep]
    want = r.bake_points(p, n, time_schedule(1024, frame=1))["rgba"][:, :3].astype(np.float64)
    got = r.probe_irradiance(p, n)[:, :3].astype(np.float64)
    # the same without the interpolation: a probe of its own at each point (lifted by the bake's bias), 1024 seeds,
    # resolved with the lookup's band factors in float64: Monte-Carlo noise and the SH band limit alone
    own = r.bake_probes(p + np.float32(0.002) * n, time_schedule(1024, frame=1))[:, :27].astype(np.float64).reshape(-1, 9, 3)
    band = np.array([1, 2 / 3, 2 / 3, 2 / 3, 0.25, 0.25, 0.25, 0.25, 0.25])
    same = np.maximum((own * (sh_basis(n).astype(np.float64) * band)[:, :, None]).sum(axis=1), 0)

    def rel_rms(x, sel):
        return round(float(np.sqrt(((x[sel] - want[sel]) ** 2).mean() / (want[sel] ** 2).mean())), 4)

    lit = hits["id"][keep] != 3          # (material 3 is the emissive panel: its underside sees only the dim room)
    every = np.ones(len(p), bool)
    emit({"what": "probe_quality", "points": int(keep.sum()), "points_off_the_emitter": int(lit.sum()), "bake_seeds": 1024,
          "field_seeds": a.seeds, "grid": a.grid, "relative_rms_difference": rel_rms(got, every),
          "relative_rms_difference_off_the_emitter": rel_rms(got, lit),
          "relative_rms_difference_probe_at_the_point": rel_rms(same, every),
          "relative_rms_difference_probe_at_the_point_off_the_emitter": rel_rms(same, lit),
          "mean_bake": round(float(want.mean()), 4), "mean_probe": round(float(got.mean()), 4),
          "mean_probe_at_the_point": round(float(same.mean()), 4)})
    r.close()
    if a.out:
        with open(a.out, "w") as f:
            for dline in lines:
                f.write(json.dumps(dline) + "\n")


if __name__ == "__main__":
    main()
