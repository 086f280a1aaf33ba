"""bloom_time.py — what the bloom stage costs, by §4.13's method.

One process, the diagnostic library. Its rmr_diag_bloom_time times n back-to-back rounds of one thing on the
accumulator between two HIP events, all queued from C behind a stream it has made busy first, so the figure
is the GPU's time and not the host's enqueue rate; its rmr_diag_bloom_tail sets how many pixels the
single-workgroup tail kernel's levels may hold together (0: per-level launches only). At 1920x1080 on C2's
scene, Cornell-5, rendered at 4 spp, after a warm-up the configurations alternate round by round and the
median over the rounds is reported:

  * k_bloom_down0 and k_bloom_compose, per launch, and a device-to-device copy of one plane (W x H float4,
    33 MB at 1080p) queued the same way, the yardstick;
  * the whole stage at N = 5 and N = 8 with per-level launches only and with the tail kernel at each cap that
    changes which levels it takes;
  * the same on a 16x16 context: what the launches cost when the kernels have nothing to do (the dispatch
    floor, to be read beside every figure);
  * the two kernels, the copy and the stage at several launch counts: a time per launch that does not move
    with n is the GPU's;
  * the 4-spp preview loop's other stages (render_spp, denoise, temporal_accumulate, the auto-exposed tonemap)
    for the stage's share of that loop.

Prints one JSON line per measurement; --out FILE also appends them there.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from raymarchrenderer_amd import Renderer, abi, time_schedule  # noqa: E402
sys.path.insert(0, os.path.join(ROOT, "tools"))
from tonemap_time import Hip  # noqa: E402  (the few HIP runtime calls the loop's measurement needs)

SCENES = os.path.join(ROOT, "scenes")
WHICH = {"stage": 0, "k_bloom_down0": 1, "k_bloom_compose": 2, "copy_d2d": 3}
STAGE_REPS = 8   # a round of the stage is up to ten launches: fewer rounds keep the host ahead of the GPU


def timed(r, which, n, levels=5, tail=-1):
    """ms per round of n back-to-back rounds (rmr_diag_bloom_time); tail: the tail kernel's cap, -1 the default."""
    if r.lib.rmr_diag_bloom_tail(r.ctx, tail) != 0:
        raise RuntimeError("rmr_diag_bloom_tail failed")
    ms = C.c_float(0.0)
    if r.lib.rmr_diag_bloom_time(r.ctx, WHICH[which], levels, n, C.byref(ms)) != 0:
        raise RuntimeError("rmr_diag_bloom_time failed")
    return ms.value


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=32, help="back-to-back launches per event pair (1..64)")
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds (the median is reported)")
    ap.add_argument("--out", help="also append the JSON lines to this file")
    ap.add_argument("--small", action="store_true", help="256x144 instead of 1920x1080 (a rehearsal)")
    a = ap.parse_args()
    lines = []

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    hip = Hip()
    W, H = (256, 144) if a.small else (1920, 1080)
    r = Renderer(0, W, H, diag=True)
    tiny = Renderer(0, 16, 16, diag=True)
    stream = hip.handle(hip.lib.hipStreamCreate, "hipStreamCreate")
    try:
        r.set_stream(stream.value)
        r.load_scene(os.path.join(SCENES, "cornell5.scene"), "rm1")
        r.set_params(abi.default_params(max_bounces=4))
        r.render_spp(time_schedule(4))
        import numpy as np
        tiny.write_accum(np.full((16, 16, 4), 2.0, np.float32))
        kernels = {"k_bloom_down0": ("k_bloom_down0", a.reps, 5, -1), "k_bloom_compose": ("k_bloom_compose", a.reps, 5, -1),
                   "copy_d2d": ("copy_d2d", a.reps, 5, -1)}
        stages = {}
        for N in (5, 8):
            for name, cap in (("per_level", 0), ("tail_4096", 4096), ("tail_12288", 12288)):
                stages["stage_N%d_%s" % (N, name)] = ("stage", STAGE_REPS, N, cap)
        configs = {**kernels, **stages}
        for ctx in (r, tiny):   # warm-up: every kernel once, more than one bracket
            for which, n, N, cap in configs.values():
                timed(ctx, which, n, N, cap)
        ms = {k: [] for k in configs}
        floor = {k: [] for k in configs}
        for _ in range(a.rounds):
            for k, (which, n, N, cap) in configs.items():
                ms[k].append(timed(r, which, n, N, cap))
                floor[k].append(timed(tiny, which, n, N, cap))
        med = {k: statistics.median(v) for k, v in ms.items()}
        px = W * H
        row = {"what": "bloom", "W": W, "H": H, "plane_MB": round(px * 16 / 1e6, 2), "reps": a.reps, "stage_reps": STAGE_REPS,
               "rounds": a.rounds}
        for k, v in med.items():
            row[k + "_ms"] = round(v, 5)
            row[k + "_ms_min_max"] = [round(min(ms[k]), 5), round(max(ms[k]), 5)]
        for k in ("k_bloom_down0", "k_bloom_compose"):
            row[k + "_over_copy"] = round(med[k] / med["copy_d2d"], 3)
        # the traffic floors: bytes per source pixel over the copy's own rate (32 B per pixel in its time)
        rate = px * 32 / med["copy_d2d"]
        row["k_bloom_down0_floor_ms"] = round(px * (16 + 4) / rate, 5)
        row["k_bloom_compose_floor_ms"] = round(px * (16 + 16) / rate, 5)
        emit(row)
        emit({"what": "dispatch_floor_16x16", "reps": a.reps, "stage_reps": STAGE_REPS, "rounds": a.rounds,
              **{k + "_ms": round(statistics.median(v), 5) for k, v in floor.items()}})
        sweep = {"what": "launch_count_sweep", "W": W, "H": H, "rounds": a.rounds}
        for k in ("k_bloom_down0", "k_bloom_compose", "copy_d2d"):
            for n in (4, 16, 64):
                sweep["%s_n%d_ms" % (k, n)] = round(statistics.median(timed(r, k, n) for _ in range(a.rounds)), 5)
        for k in ("stage_N5_per_level", "stage_N5_tail_12288"):
            which, _, N, cap = configs[k]
            for n in (2, 4, 8, 16):
                sweep["%s_n%d_ms" % (k, n)] = round(statistics.median(timed(r, which, n, N, cap) for _ in range(a.rounds)), 5)
        emit(sweep)
        # the stage's share of the 4-spp preview loop
        times = time_schedule(4)
        parts = {"render_spp_4": lambda: r.render_spp(times, first_sample=0), "denoise": lambda: r.lib.rmr_denoise(r.ctx, None),
                 "temporal_accumulate": lambda: r.lib.rmr_temporal_accumulate(r.ctx, abi.OUTPUT_DENOISED, C.c_float(4.0), None)}
        loop = {}
        for name, fn in parts.items():
            fn()
            loop[name] = statistics.median(hip.timed(stream, fn, 3) for _ in range(a.rounds))
        tm = C.c_float(0.0)
        tone = []
        for _ in range(a.rounds):
            if r.lib.rmr_diag_tonemap_time(r.ctx, 4, a.reps, C.byref(tm)) != 0:
                raise RuntimeError("rmr_diag_tonemap_time failed")
            tone.append(tm.value)
        loop["tonemap_auto"] = statistics.median(tone)
        for k in ("stage_N5_per_level", "stage_N5_tail_12288"):
            total = sum(loop.values()) + med[k]
            emit({"what": "preview_loop_share", "stage": k, "W": W, "H": H, **{n + "_ms": round(v, 4) for n, v in loop.items()},
                  "bloom_ms": round(med[k], 5), "bloom_share": round(med[k] / total, 5)})
    finally:
        r.sync()
        r.close()
        tiny.close()
        hip.lib.hipStreamDestroy(stream)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
