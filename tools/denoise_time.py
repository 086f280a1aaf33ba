"""denoise_time.py — what the preview denoiser and the guide pass cost.

One process, the diagnostic library (its rmr_diag_denoise_tiled picks the a-trous form per step; the
release library's choice is a constant). After a warm-up every configuration is timed in
rmr_sync-bracketed repetitions, the configurations alternating round by round, and the median over
the rounds is reported:

  * filter: rmr_denoise with k = 1 .. 5 iterations on a 4-spp Cornell-5 frame at 1920x1080 and
    3840x2160, all passes plain, and k = 1, 2 with the LDS-tiled form. Pass i (step 2^i) costs
    t(i + 1) - t(i) (t(0) = 0: the calls are queued back to back, so launch gaps are hidden), beside
    the pass's HBM floor of four W x H float4 planes at 5.4 TB/s (DESIGN.md §4.6's k_fold rate);
  * guides: rmr_render_guides of the whole image on C2's scene (Cornell-5, 1080p) and C4's (csg256,
    4K), beside one 1-spp rmr_render_spp launch of the same scene at the same size.

With --variance the variance-guided mode instead, by the same protocol and in the
same process as the plain filter's kernels it is compared with: per pass the guided plain and tiled
forms beside k_atrous / k_atrous_lds, the seed kernel at var_radius 0, 1, 3, 4 (rmr_denoise_variance
with no iteration, less rmr_denoise's with none: both copy the accumulator), and the whole default call
of either filter. Floors: a guided pass moves four float4 planes and two float planes, (4 x 16 + 8) B
per pixel, the seed 52 B per pixel, at the same 5.4 TB/s.

Prints one JSON line per measurement; --out FILE also writes them there.
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

from raymarchrenderer_amd import Renderer, abi, default_camera_view, time_schedule  # noqa: E402

SCENES = os.path.join(ROOT, "scenes")
FOLD_RATE = 5.4e12   # B/s, k_fold's measured rate


def setup(scene, W, H, bounces):
    r = Renderer(0, W, H, diag=True)
    r.load_scene(os.path.join(SCENES, scene), "rm1")
    r.set_params(abi.default_params(max_bounces=bounces))
    r.set_view(default_camera_view(W, H))
    return r


def bracket(r, fn, reps):
    """ms per call of `reps` queued calls between two rmr_sync."""
    r.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    r.sync()
    return (time.perf_counter() - t0) * 1e3 / reps


def time_filter(W, H, reps, rounds, emit):
    r = setup("cornell5.scene", W, H, 4)
    try:
        r.render_spp(time_schedule(4))
        r.render_guides()

        def run(mask, k):
            p = abi.default_denoise_params(iterations=k)

            def call():
                rc = r.lib.rmr_denoise(r.ctx, C.byref(p))
                if rc != 0:
                    raise RuntimeError("rmr_denoise failed: %d" % rc)
            if r.lib.rmr_diag_denoise_tiled(r.ctx, mask) != 0:
                raise RuntimeError("rmr_diag_denoise_tiled failed")
            return bracket(r, call, reps)

        configs = [(0, k) for k in range(1, 6)] + [(3, 1), (3, 2)]
        for c in configs:   # warm-up: every kernel once, more than one bracket
            run(*c)
        ms = {c: [] for c in configs}
        for _ in range(rounds):
            for c in configs:
                ms[c].append(run(*c))
        med = {c: statistics.median(v) for c, v in ms.items()}
        spread = {c: (min(v), max(v)) for c, v in ms.items()}
        floor_ms = 4 * 16 * W * H / FOLD_RATE * 1e3
        for i in range(5):
            plain = med[(0, i + 1)] - (med[(0, i)] if i else 0.0)
            row = {"what": "atrous_pass", "W": W, "H": H, "step": 1 << i, "plain_ms": round(plain, 4),
                   "hbm_floor_ms": round(floor_ms, 4), "reps": reps, "rounds": rounds,
                   "plain_total_ms_min_max": [round(v, 4) for v in spread[(0, i + 1)]]}
            if i < 2:
                tiled = med[(3, i + 1)] - (med[(3, i)] if i else 0.0)
                row["tiled_ms"] = round(tiled, 4)
                row["tiled_total_ms_min_max"] = [round(v, 4) for v in spread[(3, i + 1)]]
            emit(row)
    finally:
        r.close()


def time_guided(W, H, reps, rounds, emit):
    r = setup("cornell5.scene", W, H, 4)
    try:
        r.set_error_estimate(True)
        r.render_spp(time_schedule(4))
        r.render_guides()

        def run(kind, mask, k, radius=3):
            p = abi.default_denoise_params(iterations=k)
            v = abi.default_variance_params(var_radius=radius)

            def call():
                if kind == "guided":
                    rc = r.lib.rmr_denoise_variance(r.ctx, C.byref(p), C.byref(v))
                else:
                    rc = r.lib.rmr_denoise(r.ctx, C.byref(p))
                if rc != 0:
                    raise RuntimeError("%s denoise failed: %d" % (kind, rc))
            if r.lib.rmr_diag_denoise_tiled(r.ctx, mask) != 0:
                raise RuntimeError("rmr_diag_denoise_tiled failed")
            return bracket(r, call, reps)

        configs = []
        for kind in ("guided", "plain"):
            configs += [(kind, 0, k) for k in range(0, 6)] + [(kind, 3, 1), (kind, 3, 2), (kind, 3, 5)]
        configs += [("guided", 0, 0, rad) for rad in (0, 1, 4)]
        for c in configs:   # warm-up: every kernel once, more than one bracket
            run(*c)
        ms = {c: [] for c in configs}
        for _ in range(rounds):
            for c in configs:
                ms[c].append(run(*c))
        med = {c: statistics.median(v) for c, v in ms.items()}
        spread = {c: [round(min(v), 4), round(max(v), 4)] for c, v in ms.items()}
        pass_floor = (4 * 16 + 8) * W * H / FOLD_RATE * 1e3
        plain_floor = 4 * 16 * W * H / FOLD_RATE * 1e3
        # what a call of k >= 1 iterations runs before its passes: the seed kernel (guided; the call with
        # no iteration also copies the accumulator, as rmr_denoise's does), nothing (plain)
        copy = med[("plain", 0, 0)]
        base = {"guided": med[("guided", 0, 0)] - copy, "plain": 0.0}

        def before(kind, mask, i):
            return med[(kind, mask, i)] if i else base[kind]
        for i in range(5):
            row = {"what": "guided_pass", "W": W, "H": H, "step": 1 << i, "reps": reps, "rounds": rounds,
                   "guided_plain_ms": round(med[("guided", 0, i + 1)] - before("guided", 0, i), 4),
                   "guided_plain_total_ms_min_max": spread[("guided", 0, i + 1)],
                   "k_atrous_ms": round(med[("plain", 0, i + 1)] - before("plain", 0, i), 4),
                   "k_atrous_total_ms_min_max": spread[("plain", 0, i + 1)],
                   "guided_floor_ms": round(pass_floor, 4), "k_atrous_floor_ms": round(plain_floor, 4)}
            if i < 2:
                for kind, key in (("guided", "guided_tiled"), ("plain", "k_atrous_lds")):
                    row[key + "_ms"] = round(med[(kind, 3, i + 1)] - before(kind, 3, i), 4)
                    row[key + "_total_ms_min_max"] = spread[(kind, 3, i + 1)]
            emit(row)
        for rad in (0, 1, 3, 4):
            c = ("guided", 0, 0) if rad == 3 else ("guided", 0, 0, rad)
            emit({"what": "variance_seed", "W": W, "H": H, "var_radius": rad, "seed_ms": round(med[c] - copy, 4),
                  "seed_and_copy_ms_min_max": spread[c], "copy_ms": round(copy, 4), "copy_ms_min_max": spread[("plain", 0, 0)],
                  "floor_ms": round(52 * W * H / FOLD_RATE * 1e3, 4), "reps": reps, "rounds": rounds})
        emit({"what": "default_call", "W": W, "H": H, "reps": reps, "rounds": rounds,
              "guided_tiled12_ms": round(med[("guided", 3, 5)], 4), "guided_tiled12_ms_min_max": spread[("guided", 3, 5)],
              "guided_all_plain_ms": round(med[("guided", 0, 5)], 4), "guided_all_plain_ms_min_max": spread[("guided", 0, 5)],
              "rmr_denoise_ms": round(med[("plain", 3, 5)], 4), "rmr_denoise_ms_min_max": spread[("plain", 3, 5)]})
    finally:
        r.close()


def trace_guided(W, H, reps):
    """For a `rocprofv3 --kernel-trace --stats` run of its own (one size per run, so that the per-kernel
    averages are of one size): every guided kernel `reps` times, the plain filter's beside them."""
    r = setup("cornell5.scene", W, H, 4)
    try:
        r.set_error_estimate(True)
        r.render_spp(time_schedule(4))
        r.render_guides()
        for mask in (0, 3):
            r.lib.rmr_diag_denoise_tiled(r.ctx, mask)
            for _ in range(reps):
                r.denoise_variance()
                r.denoise()
        r.sync()
    finally:
        r.close()


def time_guides(scene, W, H, bounces, reps, rounds, emit):
    r = setup(scene, W, H, bounces)
    try:
        t1 = time_schedule(1)

        def guides():
            r.render_guides()

        def one_spp():
            r.render_spp(t1)
        for f in (guides, one_spp, guides, one_spp):   # warm-up (the 1-spp launch compiles its kernel)
            bracket(r, f, 2)
        g, s = [], []
        for _ in range(rounds):
            g.append(bracket(r, guides, reps))
            s.append(bracket(r, one_spp, reps))
        emit({"what": "guide_pass", "scene": scene, "W": W, "H": H, "guides_ms": round(statistics.median(g), 4),
              "one_spp_launch_ms": round(statistics.median(s), 4), "guides_ms_min_max": [round(min(g), 4), round(max(g), 4)],
              "one_spp_ms_min_max": [round(min(s), 4), round(max(s), 4)], "reps": reps, "rounds": rounds})
    finally:
        r.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20, help="queued calls per bracket")
    ap.add_argument("--rounds", type=int, default=7, help="alternating rounds (the median is reported)")
    ap.add_argument("--out", help="also write the JSON lines to this file")
    ap.add_argument("--small", action="store_true", help="256x144 / 512x288 instead of 1080p / 4K (a rehearsal)")
    ap.add_argument("--variance", action="store_true", help="the variance-guided mode (DESIGN.md §4.11) instead")
    ap.add_argument("--trace", metavar="WxH", help="with --variance: no timing, run every guided kernel --reps times "
                    "at this size (for a rocprofv3 --kernel-trace --stats run of its own)")
    a = ap.parse_args()
    lines = []

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    sizes = [(256, 144), (512, 288)] if a.small else [(1920, 1080), (3840, 2160)]
    if a.variance and a.trace:
        trace_guided(*(int(v) for v in a.trace.split("x")), a.reps)
    elif a.variance:
        for W, H in sizes:
            time_guided(W, H, a.reps, a.rounds, emit)
    else:
        for W, H in sizes:
            time_filter(W, H, a.reps, a.rounds, emit)
        time_guides("cornell5.scene", *sizes[0], 4, a.reps, a.rounds, emit)
        time_guides("csg256.scene", *sizes[1], 4, a.reps, a.rounds, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
