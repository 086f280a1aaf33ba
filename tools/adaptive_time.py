"""adaptive_time.py — what the error estimate and the adaptive loop cost.

One process, the release library. After a warm-up the configurations alternate round by round and the
median over the rounds is reported, one JSON line per measurement (--out FILE also writes them there):

  * fold: a C2 frame (Cornell-5, 1920x1080, 64 spp, 4 bounces) with the estimate off and on: the frame's
    wall time between two rmr_sync and the fold kernel's event time (rmr_stats.fold_ms: k_fold against
    k_fold_half), beside the HBM bytes each moves per pixel (64 sample planes of 16 B, + 32 B for the
    accumulator read and written, + 32 B more for the half image);
  * tile_error: rmr_tile_error (kernel, TX x TY floats back to the host, one sync) at 1920x1080 and
    3840x2160 on a 4-spp frame, beside the kernel's floor of 32 B per pixel at 5.4 TB/s (§4.6);
  * adaptive: rmr_render_adaptive on C2's scene (min 16, pass 16, max 64, block_tiles 2), once per
    threshold of --thresholds, against the uniform 64-spp frame: wall time, mean spp, passes, and the
    part of the wall time that no trace or fold kernel covers, per pass (the readback, the host decision,
    the tile list upload and the launch gaps).

--kernels-only renders one frame of each kind and exits: the run to put under a kernel trace, whose
per-kernel times (k_fold, k_fold_half, k_tile_error) are the kernel-side figures.
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
FOLD_RATE = 5.4e12   # B/s, k_fold's measured rate


def setup(W, H):
    r = Renderer(0, W, H)
    r.set_jit(1)
    r.load_scene(os.path.join(SCENES, "cornell5.scene"), "rm1")
    r.set_params(abi.default_params(max_bounces=4))
    r.set_view(default_camera_view(W, H))
    return r


def frame(r, times, estimate):
    """One uniform frame; (wall ms, trace ms, fold ms)."""
    r.set_error_estimate(estimate)
    r.reload()
    r.reset_stats()
    r.sync()
    t0 = time.perf_counter()
    r.render_spp(times)
    r.sync()
    wall = (time.perf_counter() - t0) * 1e3
    s = r.stats()
    return wall, s.trace_ms, s.fold_ms


def adaptive(r, times, threshold):
    r.set_error_estimate(False)
    r.reload()
    r.reset_stats()
    r.sync()
    t0 = time.perf_counter()
    res = r.render_adaptive(times, threshold=threshold, min_samples=16, pass_samples=16, block_tiles=2)
    r.sync()
    wall = (time.perf_counter() - t0) * 1e3
    s = r.stats()
    return wall, s.trace_ms, s.fold_ms, res


def med(v):
    return round(statistics.median(v), 4)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--thresholds", default="0.1,0.3,0.6", help="tile-error thresholds of the adaptive runs")
    ap.add_argument("--out", default="")
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    thresholds = [float(t) for t in a.thresholds.split(",")]
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    W, H, spp = 1920, 1080, 64
    times = time_schedule(spp)
    r = setup(W, H)
    if a.kernels_only:
        frame(r, times, False)
        frame(r, times, True)
        r.tile_error()
        adaptive(r, times, thresholds[0])
        r.close()
        r = setup(3840, 2160)
        r.set_error_estimate(True)
        r.render_spp(time_schedule(4))
        r.tile_error()
        r.close()
        return
    # fold: estimate off / on, alternating; adaptive against uniform in the same rounds
    off, on, ads = [], [], [[] for _ in thresholds]
    for rnd in range(a.rounds + 1):
        x, y = frame(r, times, False), frame(r, times, True)
        z = [adaptive(r, times, t) for t in thresholds]
        if rnd:   # round 0 is the warm-up (hipRTC compile, first allocations)
            off.append(x)
            on.append(y)
            for i, v in enumerate(z):
                ads[i].append(v)
    planes = spp * 16
    emit({"what": "fold", "W": W, "H": H, "spp": spp,
          "off": {"wall_ms": med([v[0] for v in off]), "trace_ms": med([v[1] for v in off]), "fold_ms": med([v[2] for v in off]),
                  "bytes_per_pixel": planes + 32},
          "on": {"wall_ms": med([v[0] for v in on]), "trace_ms": med([v[1] for v in on]), "fold_ms": med([v[2] for v in on]),
                 "bytes_per_pixel": planes + 64},
          "expected_fold_ratio": round((planes + 64) / (planes + 32), 4)})
    for thr, ad in zip(thresholds, ads):
        res = ad[-1][3]
        walls = [v[0] for v in ad]
        uncovered = [(v[0] - v[1] - v[2]) / v[3].passes for v in ad]
        emit({"what": "adaptive", "W": W, "H": H, "max_spp": spp, "threshold": thr, "min": 16, "pass": 16,
              "block_tiles": 2, "wall_ms": med(walls), "wall_ms_all": [round(v, 3) for v in walls],
              "uniform_wall_ms": med([v[0] for v in off]), "uniform_wall_ms_all": [round(v[0], 3) for v in off],
              "mean_spp": round(res.samples / float(W * H), 3), "passes": res.passes, "tiles_open": res.tiles_open,
              "max_error": res.max_error, "trace_ms": med([v[1] for v in ad]), "fold_ms": med([v[2] for v in ad]),
              "uncovered_ms_per_pass": med(uncovered),
              "uniform_uncovered_ms": med([v[0] - v[1] - v[2] for v in off])})
    r.close()
    # tile_error at two sizes
    for w, h in ((1920, 1080), (3840, 2160)):
        r = setup(w, h)
        r.set_error_estimate(True)
        r.render_spp(time_schedule(4))
        r.tile_error()
        t = []
        for _ in range(a.rounds * 4):
            r.sync()
            t0 = time.perf_counter()
            r.tile_error()
            t.append((time.perf_counter() - t0) * 1e3)
        emit({"what": "tile_error", "W": w, "H": h, "call_ms": med(t), "call_ms_min": round(min(t), 4),
              "kernel_floor_ms": round(w * h * 32 / FOLD_RATE * 1e3, 4), "readback_bytes": ((w + 7) // 8) * ((h + 7) // 8) * 4})
        r.close()
    if a.out:
        with open(a.out, "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
