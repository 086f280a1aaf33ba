"""temporal_time.py — what the temporal reprojection stage costs.

One process, the diagnostic library (its rmr_diag_temporal_keep makes rmr_temporal_accumulate run its
kernel against the history it has and leave that history in place, so that repeated calls time k_temporal
alone on one view pair; its rmr_diag_denoise_tiled picks the plain a-trous form). After a warm-up every
configuration is timed in rmr_sync-bracketed repetitions of queued calls, the configurations alternating
round by round, and the median over the rounds is reported, on C2's scene (Cornell-5, 4 spp) at
1920x1080 and 3840x2160:

  * k_temporal for two view pairs: the history made at a view 0.2 along x and 2 degrees of yaw away from
    the current one (rmr_camera_view's corner rays), and at that view with r11 scaled by 1.05 (a twist);
  * one step-4 pass of the plain a-trous filter, t(3 iterations) - t(2 iterations): the nearest existing
    kernel with a comparable gather;
  * a whole step as the loop runs it (the kernel and the device copy of the two guide planes), the
    history at the current view.

The kernel's HBM floor: 48 B of current planes, 52 B of history (colour, count, two guide planes: every
history pixel once) and 20 B written per pixel, at 5.4 TB/s (DESIGN.md §4.6's k_fold rate); the a-trous
pass's: four float4 planes.

Prints one JSON line per measurement; --out FILE also writes them there.
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from raymarchrenderer_amd import Renderer, abi, camera_view, default_camera_view, time_schedule  # noqa: E402

SCENES = os.path.join(ROOT, "scenes")
FOLD_RATE = 5.4e12   # B/s, k_fold's measured rate


def moved_view(W, H):
    m = math.sqrt(45.0)
    fov = float(np.float32(3.141592653) / np.float32(4))
    yaw = math.radians(2.0)
    d = (0.0, -3.0 / m, 6.0 / m)
    d2 = (d[0] * math.cos(yaw) + d[2] * math.sin(yaw), d[1], -d[0] * math.sin(yaw) + d[2] * math.cos(yaw))
    return camera_view((0.2, 4.0, -6.0), d2, float(W) / float(H), fov)


def bracket(r, fn, reps):
    """ms per call of `reps` queued calls between two rmr_sync."""
    r.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    r.sync()
    return (time.perf_counter() - t0) * 1e3 / reps


def primed(W, H, h_view, keep):
    """A context whose history was made at h_view and whose accumulator and guides are of the default view."""
    r = Renderer(0, W, H, diag=True)
    r.load_scene(os.path.join(SCENES, "cornell5.scene"), "rm1")
    r.set_params(abi.default_params(max_bounces=4))
    r.set_view(h_view)
    r.render_spp(time_schedule(4))
    r.temporal_accumulate("accum", 4)
    r.set_view(default_camera_view(W, H))
    r.render_spp(time_schedule(4, first_sample=4), first_sample=0)
    r.render_guides()
    if r.lib.rmr_diag_temporal_keep(r.ctx, int(keep)) != 0 or r.lib.rmr_diag_denoise_tiled(r.ctx, 0) != 0:
        raise RuntimeError("diagnostic switches failed")
    return r


def time_temporal(W, H, reps, rounds, emit):
    A = moved_view(W, H)
    twisted = A.copy()
    twisted[12:15] *= np.float32(1.05)
    ctx = {"camera_view": primed(W, H, A, True), "twisted": primed(W, H, twisted, True),
           "step": primed(W, H, default_camera_view(W, H), False)}
    try:
        tp = abi.default_temporal_params()

        def temporal(name):
            r = ctx[name]

            def call():
                rc = r.lib.rmr_temporal_accumulate(r.ctx, abi.OUTPUT_ACCUM, C.c_float(4.0), C.byref(tp))
                if rc != 0:
                    raise RuntimeError("rmr_temporal_accumulate failed: %d" % rc)
            return bracket(r, call, reps)

        def atrous(k):
            r = ctx["camera_view"]
            p = abi.default_denoise_params(iterations=k)

            def call():
                rc = r.lib.rmr_denoise(r.ctx, C.byref(p))
                if rc != 0:
                    raise RuntimeError("rmr_denoise failed: %d" % rc)
            return bracket(r, call, reps)

        configs = [(temporal, "camera_view"), (temporal, "twisted"), (temporal, "step"), (atrous, 2), (atrous, 3)]
        for f, a in configs:   # warm-up: every kernel once, more than one bracket
            f(a)
        ms = {c: [] for c in configs}
        for _ in range(rounds):
            for c in configs:
                ms[c].append(c[0](c[1]))
        med = {c: statistics.median(v) for c, v in ms.items()}
        spread = {c: [round(min(v), 4), round(max(v), 4)] for c, v in ms.items()}
        floor = (48 + 52 + 20) * W * H / FOLD_RATE * 1e3
        a4 = med[(atrous, 3)] - med[(atrous, 2)]
        for name in ("camera_view", "twisted"):
            k = med[(temporal, name)]
            emit({"what": "k_temporal", "W": W, "H": H, "view_pair": name, "kernel_ms": round(k, 4),
                  "kernel_ms_min_max": spread[(temporal, name)], "hbm_floor_ms": round(floor, 4),
                  "share_of_floor": round(k / floor, 3), "atrous_step4_ms": round(a4, 4),
                  "atrous_floor_ms": round(4 * 16 * W * H / FOLD_RATE * 1e3, 4),
                  "atrous_3it_ms_min_max": spread[(atrous, 3)], "atrous_2it_ms_min_max": spread[(atrous, 2)],
                  "reps": reps, "rounds": rounds})
        emit({"what": "temporal_step", "W": W, "H": H, "step_ms": round(med[(temporal, "step")], 4),
              "step_ms_min_max": spread[(temporal, "step")], "reps": reps, "rounds": rounds})
    finally:
        for r in ctx.values():
            r.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20, help="queued calls per bracket")
    ap.add_argument("--rounds", type=int, default=7, help="alternating rounds (the median is reported)")
    ap.add_argument("--out", help="also write the JSON lines to this file")
    ap.add_argument("--small", action="store_true", help="256x144 / 512x288 instead of 1080p / 4K (a rehearsal)")
    a = ap.parse_args()
    lines = []

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    for W, H in ([(256, 144), (512, 288)] if a.small else [(1920, 1080), (3840, 2160)]):
        time_temporal(W, H, a.reps, a.rounds, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
