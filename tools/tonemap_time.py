"""tonemap_time.py — what the tone-mapping stage costs.

One process, the diagnostic library. Its rmr_diag_tonemap_time times n back-to-back launches of one of the
stage's kernels on the accumulator between two HIP events, all queued from C behind a stream it has made
busy first, so the figure is the GPU's time per launch and not the host's enqueue rate; its
rmr_diag_tonemap_fold switches k_lum_hist's in-wave folding of equal bins. At 1920x1080, on three images
(log-uniform noise over 2^-20 .. 2^18, a flat 0.18 image, and C2's scene, Cornell-5, rendered at 4 spp),
after a warm-up the configurations alternate round by round and the median over the rounds is reported:

  * k_lum_hist with and without the folding, k_meter, k_tonemap;
  * a device-to-device copy of one plane (W x H float4, 33 MB at 1080p) queued the same way, the yardstick:
    it moves the bytes k_tonemap moves (16 B read and 16 B written per pixel) and twice k_lum_hist's;
  * the three kernels as an auto-exposed rmr_tonemap queues them;
  * the same five on a 16x16 context: what one back-to-back launch costs when the kernel has nothing to do
    (the dispatch floor, to be read beside every per-launch figure);
  * k_lum_hist, k_tonemap and the copy at n = 4, 16 and 64 launches: a per-launch time that does not move
    with n is the GPU's;
  * on the render, the 4-spp preview loop's other stages (render_spp, denoise, temporal_accumulate) between
    events on the context's stream, for the stage's share of that loop.

Prints one JSON line per measurement; --out FILE also appends them there. --image picks one image.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from raymarchrenderer_amd import Renderer, abi, time_schedule  # noqa: E402

SCENES = os.path.join(ROOT, "scenes")


class Hip:
    """The few runtime calls the loop's measurement needs: a stream and events on it."""

    def __init__(self):
        self.lib = C.CDLL("libamdhip64.so")
        vp = C.c_void_p
        self.lib.hipStreamCreate.argtypes = [C.POINTER(vp)]
        self.lib.hipEventCreate.argtypes = [C.POINTER(vp)]
        self.lib.hipEventRecord.argtypes = [vp, vp]
        self.lib.hipEventSynchronize.argtypes = [vp]
        self.lib.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), vp, vp]
        self.lib.hipStreamDestroy.argtypes = [vp]
        self.lib.hipEventDestroy.argtypes = [vp]

    def chk(self, rc, what):
        if rc != 0:
            raise RuntimeError("%s failed: hipError %d" % (what, rc))

    def handle(self, make, what):
        h = C.c_void_p()
        self.chk(make(C.byref(h)), what)
        return h

    def timed(self, stream, fn, reps):
        """ms per call of `reps` queued calls between two events on `stream`."""
        a, b = self.handle(self.lib.hipEventCreate, "hipEventCreate"), self.handle(self.lib.hipEventCreate, "hipEventCreate")
        try:
            self.chk(self.lib.hipEventRecord(a, stream), "hipEventRecord")
            for _ in range(reps):
                fn()
            self.chk(self.lib.hipEventRecord(b, stream), "hipEventRecord")
            self.chk(self.lib.hipEventSynchronize(b), "hipEventSynchronize")
            ms = C.c_float(0.0)
            self.chk(self.lib.hipEventElapsedTime(C.byref(ms), a, b), "hipEventElapsedTime")
            return ms.value / reps
        finally:
            self.lib.hipEventDestroy(a)
            self.lib.hipEventDestroy(b)


def make_image(kind, r, W, H):
    if kind == "noise":
        img = np.exp2(np.random.default_rng(5).uniform(-20.0, 18.0, (H, W, 4))).astype(np.float32)
        img[..., 3] = 1.0
        r.write_accum(img)
    elif kind == "flat":
        img = np.full((H, W, 4), 0.18, np.float32)
        img[..., 3] = 1.0
        r.write_accum(img)
    else:
        r.load_scene(os.path.join(SCENES, "cornell5.scene"), "rm1")
        r.set_params(abi.default_params(max_bounces=4))
        r.render_spp(time_schedule(4))


WHICH = {"k_lum_hist": 0, "k_meter": 1, "k_tonemap": 2, "copy_d2d": 3, "tonemap_auto": 4}


def timed_launches(r, which, n, fold=0):
    """ms per launch of n back-to-back launches (rmr_diag_tonemap_time)."""
    if r.lib.rmr_diag_tonemap_fold(r.ctx, fold) != 0:
        raise RuntimeError("rmr_diag_tonemap_fold failed")
    ms = C.c_float(0.0)
    if r.lib.rmr_diag_tonemap_time(r.ctx, WHICH[which], n, C.byref(ms)) != 0:
        raise RuntimeError("rmr_diag_tonemap_time failed")
    return ms.value


def time_image(hip, kind, W, H, reps, rounds, emit):
    r = Renderer(0, W, H, diag=True)
    tiny = Renderer(0, 16, 16, diag=True)
    stream = hip.handle(hip.lib.hipStreamCreate, "hipStreamCreate")
    try:
        r.set_stream(stream.value)
        make_image(kind, r, W, H)
        tiny.write_accum(np.full((16, 16, 4), 0.18, np.float32))
        nbytes = W * H * 16
        hist, skipped = r.luminance_histogram("accum")
        configs = {"k_lum_hist_fold": ("k_lum_hist", 1), "k_lum_hist_plain": ("k_lum_hist", 0), "k_meter": ("k_meter", 0),
                   "k_tonemap": ("k_tonemap", 0), "copy_d2d": ("copy_d2d", 0), "tonemap_auto": ("tonemap_auto", 0)}
        for ctx in (r, tiny):   # warm-up: every kernel once, more than one bracket
            for which, fold in configs.values():
                timed_launches(ctx, which, reps, fold)
        ms = {k: [] for k in configs}
        floor = {k: [] for k in configs}
        for _ in range(rounds):
            for k, (which, fold) in configs.items():
                ms[k].append(timed_launches(r, which, reps, fold))
                floor[k].append(timed_launches(tiny, which, reps, fold))
        med = {k: statistics.median(v) for k, v in ms.items()}
        row = {"what": "tonemap_kernels", "image": kind, "W": W, "H": H, "plane_MB": round(nbytes / 1e6, 2),
               "bins_used": int((hist > 0).sum()), "skipped": skipped, "reps": reps, "rounds": rounds}
        for k, v in med.items():
            row[k + "_ms"] = round(v, 5)
            row[k + "_ms_min_max"] = [round(min(ms[k]), 5), round(max(ms[k]), 5)]
        for k in ("k_lum_hist_fold", "k_lum_hist_plain", "k_tonemap"):
            row[k + "_over_copy"] = round(med[k] / med["copy_d2d"], 3)
        emit(row)
        emit({"what": "dispatch_floor_16x16", "image": kind, "reps": reps, "rounds": rounds,
              **{k + "_ms": round(statistics.median(v), 5) for k, v in floor.items()}})
        sweep = {"what": "launch_count_sweep", "image": kind, "W": W, "H": H, "rounds": rounds}
        for k in ("k_lum_hist_plain", "k_tonemap", "copy_d2d"):
            which, fold = configs[k]
            for n in (4, 16, 64):
                sweep["%s_n%d_ms" % (k, n)] = round(statistics.median(timed_launches(r, which, n, fold) for _ in range(rounds)), 5)
        emit(sweep)
        if kind == "render":   # the stage's share of the 4-spp preview loop
            times = time_schedule(4)
            parts = {"render_spp_4": lambda: r.render_spp(times, first_sample=0), "denoise": lambda: r.lib.rmr_denoise(r.ctx, None),
                     "temporal_accumulate": lambda: r.lib.rmr_temporal_accumulate(r.ctx, abi.OUTPUT_DENOISED, C.c_float(4.0), None)}
            loop = {}
            for name, fn in parts.items():
                fn()
                loop[name] = statistics.median(hip.timed(stream, fn, 3) for _ in range(rounds))
            total = sum(loop.values()) + med["tonemap_auto"]
            emit({"what": "preview_loop_share", "W": W, "H": H, **{k + "_ms": round(v, 4) for k, v in loop.items()},
                  "tonemap_auto_ms": round(med["tonemap_auto"], 5), "tonemap_share": round(med["tonemap_auto"] / total, 5)})
    finally:
        r.sync()
        r.close()
        tiny.close()
        hip.lib.hipStreamDestroy(stream)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=32, help="back-to-back launches per event pair (1..64)")
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds (the median is reported)")
    ap.add_argument("--image", choices=["noise", "flat", "render"], action="append", help="default: all three")
    ap.add_argument("--out", help="also append the JSON lines to this file")
    ap.add_argument("--small", action="store_true", help="256x144 instead of 1920x1080 (a rehearsal)")
    a = ap.parse_args()
    lines = []

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    hip = Hip()
    W, H = (256, 144) if a.small else (1920, 1080)
    for kind in a.image or ["noise", "flat", "render"]:
        time_image(hip, kind, W, H, a.reps, a.rounds, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
