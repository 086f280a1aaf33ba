"""aov_time.py — what the sampled AOVs cost (rmr_render_aov).

Per section one process of its own, started from here under a time limit (a section that fails or runs out of
time ends the run: nothing more is started on the GPU). In a section, after a warm-up, every configuration is
timed in rmr_sync-bracketed repetitions of queued calls, the configurations alternating round by round; the
median over the rounds is reported with the minimum and maximum.

  * c2: C2's scene (Cornell-5) at 1920x1080. rmr_render_aov of 8 samples per call, cut into launches of 1, 2,
    4 and 8 samples (ms per sample; a launch reads and writes the pixel's 80-byte state once, 160 B per pixel
    per launch), beside the guide pass (rmr_render_guides: the same march and probes once per pixel from the
    pixel centre, no RNG and no fold) in the same process; the same under each camera model; and the route that
    existed before for 4 samples: rmr_camera_rays to the host, the upload, rmr_cast_rays_device and a fold in
    torch, each part timed.
  * c4: csg256 at 3840x2160: the same launch cuts beside the guide pass.

Prints one JSON line per measurement; --out FILE also writes them there.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = os.path.join(ROOT, "scenes")
FOLD_RATE = 5.4e12   # B/s, k_fold's measured rate
SECTIONS = {"c2": ("cornell5.scene", 1920, 1080, 300), "c4": ("csg256.scene", 3840, 2160, 420)}
SMALL = {"c2": (256, 144), "c4": (512, 288)}
MODELS = (("view", {}), ("thinlens", {"aperture": 0.15, "focus": 6.0}), ("equirect", {}), ("ortho", {"width": 6.0, "height": 5.0}))


def bracket(r, fn, reps):
    """ms per call of `reps` queued calls between two rmr_sync."""
    r.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    r.sync()
    return (time.perf_counter() - t0) * 1e3 / reps


def alternate(r, configs, reps, rounds):
    """configs: name -> callable. Median, minimum and maximum ms per call over `rounds` alternating rounds."""
    for f in configs.values():   # warm-up: every kernel once, more than one bracket
        bracket(r, f, 2)
    ms = {k: [] for k in configs}
    for _ in range(rounds):
        for k, f in configs.items():
            ms[k].append(bracket(r, f, reps))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


def torch_fold(torch, hits, n_px):
    """The rule's fold of (nspp, n_px, 8) device hit records (pos, t, n, id) in torch, sample by sample."""
    dev = hits.device
    n = torch.zeros(n_px, device=dev)
    h = torch.zeros(n_px, device=dev)
    sum_t = torch.zeros(n_px, device=dev)
    min_t = torch.full((n_px,), float("inf"), device=dev)
    sn = torch.zeros((n_px, 3), device=dev)
    sp = torch.zeros((n_px, 3), device=dev)
    ids = torch.full((n_px, 4), -1.0, device=dev)
    cnt = torch.zeros((n_px, 4), device=dev)
    other = torch.zeros(n_px, device=dev)
    for k in range(hits.shape[0]):
        rec = hits[k]
        ident, t = rec[:, 7], rec[:, 3]
        hit = ident >= 0
        n += 1
        h += hit
        sum_t = torch.where(hit, sum_t + t, sum_t)
        min_t = torch.where(hit & (t < min_t), t, min_t)
        sn = torch.where(hit[:, None], sn + rec[:, 4:7], sn)
        sp = torch.where(hit[:, None], sp + rec[:, 0:3], sp)
        todo = hit.clone()
        for j in range(4):
            m = todo & (ids[:, j] == ident)
            cnt[:, j] += m
            todo &= ~m
        for j in range(4):
            m = todo & (ids[:, j] == -1.0)
            ids[:, j] = torch.where(m, ident, ids[:, j])
            cnt[:, j] = torch.where(m, torch.ones_like(n), cnt[:, j])
            todo &= ~m
        other += todo
    return n, h, sum_t, min_t, sn, sp, ids, cnt, other


def section(name, small, reps, rounds, emit):
    import numpy as np
    import torch
    from raymarchrenderer_amd import Renderer, abi, default_camera_view, time_schedule
    scene, W, H, _ = SECTIONS[name]
    if small:
        W, H = SMALL[name]
    S = 8
    times = time_schedule(S)
    r = Renderer(0, W, H)
    try:
        r.load_scene(os.path.join(SCENES, scene), "rm1")
        r.set_params(abi.default_params(max_bounces=4))
        r.set_view(default_camera_view(W, H))
        state_ms = 160 * W * H / FOLD_RATE * 1e3

        def aov(per):
            def call():
                r.set_aov_launch_samples(per)
                r.render_aov(times)
            return call
        cuts = (1, 2, 4, 8)
        configs = {"guides": r.render_guides}
        configs.update({"aov_%d" % per: aov(per) for per in cuts})
        res = alternate(r, configs, reps, rounds)
        g = res["guides"]
        for per in cuts:
            a = res["aov_%d" % per]
            emit({"what": "aov_per_sample", "scene": scene, "W": W, "H": H, "camera": "view", "launch_samples": per,
                  "ms_per_sample": round(a[0] / S, 4), "ms_per_sample_min_max": [round(a[1] / S, 4), round(a[2] / S, 4)],
                  "ms_per_launch": round(a[0] / S * per, 4), "guides_ms": round(g[0], 4),
                  "guides_ms_min_max": [round(g[1], 4), round(g[2], 4)], "ratio_to_guides": round(a[0] / S / g[0], 3),
                  "state_traffic_floor_ms_per_launch": round(state_ms, 4), "samples_per_call": S, "reps": reps,
                  "rounds": rounds})
        if name != "c2":
            return
        # each camera model (the guide pass has none under equirect and ortho)
        for model, fields in MODELS[1:]:
            r.set_camera_model(model, **fields)
            a = alternate(r, {"aov": aov(8)}, reps, rounds)["aov"]
            emit({"what": "aov_per_sample", "scene": scene, "W": W, "H": H, "camera": model, "launch_samples": 8,
                  "ms_per_sample": round(a[0] / S, 4), "ms_per_sample_min_max": [round(a[1] / S, 4), round(a[2] / S, 4)],
                  "samples_per_call": S, "reps": reps, "rounds": rounds})
        r.set_camera_model("view")
        # the route that existed before, 4 samples, part by part (host clock, each part ends in a sync)
        t4 = times[:4]
        parts = {"camera_rays_host": [], "upload": [], "cast_rays_device": [], "torch_fold": []}
        for i in range(3 + 1):   # the first round is the warm-up
            t0 = time.perf_counter()
            rays = r.camera_rays(t4)
            t1 = time.perf_counter()
            d_rays = torch.from_numpy(rays.reshape(-1).view(np.uint8).reshape(-1, 40)).cuda()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            hits = r.cast_rays_device(d_rays)
            r.sync()
            t3 = time.perf_counter()
            torch_fold(torch, hits.reshape(4, W * H, 8), W * H)
            torch.cuda.synchronize()
            t4_ = time.perf_counter()
            if i:
                for k, v in zip(parts, (t1 - t0, t2 - t1, t3 - t2, t4_ - t3)):
                    parts[k].append(v * 1e3 / 4)
        row = {"what": "existing_route_per_sample", "scene": scene, "W": W, "H": H, "samples": 4, "rounds": 3}
        total = 0.0
        for k, v in parts.items():
            row[k + "_ms"] = round(statistics.median(v), 3)
            total += statistics.median(v)
        row["total_ms"] = round(total, 3)
        row["aov_ms_per_sample"] = round(res["aov_8"][0] / S, 4)
        row["ratio_to_aov"] = round(total / (res["aov_8"][0] / S), 1)
        emit(row)
    finally:
        r.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=3, help="queued calls (of 8 samples each) per bracket")
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds (the median is reported)")
    ap.add_argument("--out", help="also write the JSON lines to this file")
    ap.add_argument("--small", action="store_true", help="256x144 / 512x288 instead of 1080p / 4K (a rehearsal)")
    ap.add_argument("--section", choices=sorted(SECTIONS), help="run this section in this process (what the tool starts)")
    a = ap.parse_args()
    if a.section:
        section(a.section, a.small, a.reps, a.rounds, lambda row: print(json.dumps(row), flush=True))
        return 0
    lines = []
    for name in sorted(SECTIONS):
        cmd = [sys.executable, os.path.abspath(__file__), "--section", name, "--reps", str(a.reps), "--rounds", str(a.rounds)]
        if a.small:
            cmd.append("--small")
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=SECTIONS[name][3])
        except subprocess.TimeoutExpired:
            print("section %s ran out of time: stopping" % name, file=sys.stderr)
            return 124
        rows = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        lines += rows
        print("\n".join(rows), flush=True)
        if p.returncode != 0:
            print("section %s failed (%d): stopping" % (name, p.returncode), file=sys.stderr)
            return p.returncode if p.returncode > 0 else 1
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
