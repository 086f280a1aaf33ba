"""Same-process A/B runner: every measured experiment of rounds 1-4 (library builds, compile-time
switches, environment switches, culling flags, tuning) in one tool with one config table.

    python tools/abrun.py [--cases c2,rm3] [--spp N] [--rounds R] VARIANT [VARIANT ...]

VARIANT = [LABEL=]SPEC[;SPEC...], SPEC one of
    lib:PATH        the context lives in that librmr build (default: the diagnostic library, which
                    reads the RMR_* switches; e.g. tools/build_rev.sh HEAD tools/librmr_base.so)
    opts:WORDS      RMR_JIT_OPTS (hipRTC compiler options, e.g. -DRMR_PROG_WAVES=6)
    env:K=V         any other RMR_* switch read at scene load / specialisation time (repeatable)
    cull:N          rmr_set_culling flags
    shade:T         rmr_set_tuning shading threshold (T + 256 R: refill threshold R)
    slots:off | slots:P,T2   lane-slot kernels: the schedule off, or its park / batch thresholds
    overflow:on | overflow:off   lane-slot kernels: the park step's overflow deposit (RMR_JIT_OVERFLOW)
    trail:K | trail:K,global     lane-slot kernels: K trailing steps per map-loop iteration (RMR_JIT_TRAIL=1 and
                    rmr_set_trail_steps; K = 0: compiled in, none taken); global: the primitive table
                    read from global memory (RMR_JIT_TRAIL=2) instead of the LDS copy
    tune:K,R,X      lane-slot kernels: the trailing passes chosen per wave (RMR_JIT_TRAIL=1 and
                    rmr_set_trail_tuning): at most K passes, ratio R eighths, park exit X (0 or 1)
e.g.  python tools/abrun.py --cases c2,c4 base="lib:tools/librmr_base.so" new="lib:raymarchrenderer_amd/librmr_diag.so"
      python tools/abrun.py --cases glass,default w6="opts:-DRMR_PROG_WAVES=6" w7="opts:-DRMR_PROG_WAVES=7" def=""

Each variant has its own context; rounds alternate between the variants (MI355X_MICROARCH rule 24:
compare in one process, interleaved), round 0 is warm-up (hipRTC compile). Per case one JSON line:
median / min trace-kernel ms per variant, the ratio to the first variant, the kernel counters, and
whether the accumulator is bitwise equal to the first variant's.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("RMR_LIB", "diag")   # tools run against the diagnostic build (env switches)
import numpy as np  # noqa: E402
from raymarchrenderer_amd import Renderer, abi, time_schedule  # noqa: E402

S, G = os.path.join(ROOT, "scenes"), os.path.join(ROOT, "tests", "golden", "scenes")
# name: scene file (None: the built-in RM3 scene), variant, bounces, W, H, default spp
CASES = {
    "c1": (os.path.join(S, "sphere1.scene"), "rm1", 1, 256, 256, 1),
    "c2": (os.path.join(S, "cornell5.scene"), "rm1", 4, 1920, 1080, 16),
    "c3": (os.path.join(S, "mandelbulb.scene"), "rm1", 2, 1920, 1080, 16),
    "c4": (os.path.join(S, "csg256.scene"), "rm1", 4, 1920, 1080, 8),
    "rm2": (os.path.join(G, "simple.scene"), "rm2", 16, 1920, 1080, 16),
    "rm3": (None, "rm3", 16, 1920, 1080, 16),
    "glass": (os.path.join(G, "glass_test.scene"), "rm1", 16, 1920, 1080, 16),
    "default": (os.path.join(G, "default.scene"), "rm1", 16, 1920, 1080, 16),
    "multilight": (os.path.join(G, "multilight.scene"), "rm1", 16, 1920, 1080, 16),
    "csg64": (os.path.join(S, "csg64.scene"), "rm1", 4, 1920, 1080, 8),
    "csg_nodes": (os.path.join(S, "csg_nodes.scene"), "rm1", 4, 1920, 1080, 8),
    # one tile of the reference's 4x4 grid at 1080p, one sample: a Graphics::Render call's launch
    "c2t": (os.path.join(S, "cornell5.scene"), "rm1", 4, 480, 270, 1),
    "rm3t": (None, "rm3", 16, 480, 270, 1),
    "c3t": (os.path.join(S, "mandelbulb.scene"), "rm1", 2, 480, 270, 1),
}


def parse_variant(text):
    label, _, spec = text.partition("=") if ("=" in text.split(":")[0]) else ("", "", text)
    v = {"label": label or text or "default", "lib": None, "env": {}, "cull": None, "shade": None, "trail": None, "tune": None}
    for item in filter(None, spec.split(";")):
        kind, _, val = item.partition(":")
        if kind == "lib":
            v["lib"] = val
        elif kind == "opts":
            v["env"]["RMR_JIT_OPTS"] = val
        elif kind == "env":
            k, _, x = val.partition("=")
            v["env"][k] = x
        elif kind == "cull":
            v["cull"] = int(val)
        elif kind == "shade":
            v["shade"] = (v["shade"] or 0) | int(val)
        elif kind == "slots":   # rmr_set_tuning's upper bits (rmr.h)
            p, _, t2 = val.partition(",")
            v["shade"] = (v["shade"] or 0) | 1 << 23 | ((127 << 16) if val == "off" else (int(p) << 16 | int(t2 or 0) << 24))
        elif kind == "overflow":   # rmr_jit.cpp: part of the generated source
            if val not in ("on", "off"):
                raise SystemExit("overflow:on or overflow:off, not %r" % item)
            v["env"]["RMR_JIT_OVERFLOW"] = "1" if val == "on" else "0"
        elif kind == "trail":   # rmr_jit.cpp: part of the generated source; K: a launch parameter
            k, _, tab = val.partition(",")
            if tab not in ("", "global") or not k.isdigit() or int(k) > 15:
                raise SystemExit("trail:K or trail:K,global with K in 0..15, not %r" % item)
            v["env"]["RMR_JIT_TRAIL"] = "2" if tab else "1"
            v["trail"] = int(k)
        elif kind == "tune":   # a launch parameter (rmr_set_trail_tuning)
            w = val.split(",")
            if len(w) != 3 or not all(x.isdigit() for x in w):
                raise SystemExit("tune:K,R,X with K in 0..15, R in 0..8, X 0 or 1, not %r" % item)
            v["env"]["RMR_JIT_TRAIL"] = "1"
            v["tune"] = tuple(int(x) for x in w)
        else:
            raise SystemExit("unknown variant spec %r" % item)
    return v


def ncnt(v):
    """Counters to read: the trailing steps' own from 31, the profiling build's pass counts from 34 (this
    tree's library; rmr_internal.h kCntProfTrail)."""
    if v["trail"] is None and v["tune"] is None:
        return 32
    return 74 if "-DRMR_PROFILE" in v["env"].get("RMR_JIT_OPTS", "") and not v["lib"] else 34


def apply_env(v, keys, saved):
    for k in keys:
        if k in v["env"]:
            os.environ[k] = v["env"][k]
        elif saved.get(k) is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = saved[k]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("variants", nargs="+")
    ap.add_argument("--cases", default="c2")
    ap.add_argument("--spp", type=int, default=0, help="samples per pixel (0: the case's default)")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--W", type=int, default=0)
    ap.add_argument("--H", type=int, default=0)
    ap.add_argument("--raw", action="store_true", help="also print the 32 raw kernel counters (diagnostic builds)")
    a = ap.parse_args()
    vs = [parse_variant(t) for t in a.variants]
    keys = sorted({k for v in vs for k in v["env"]})
    saved = {k: os.environ.get(k) for k in keys}
    ctx = [Renderer(0, 64, 64, diag=(v["lib"] if v["lib"] else True)) for v in vs]
    for name in a.cases.split(","):
        path, variant, bounces, W, H, spp = CASES[name]
        W, H, spp = a.W or W, a.H or H, a.spp or spp
        times = time_schedule(spp)
        ms = [[] for _ in vs]
        img, st, cnt = [None] * len(vs), [None] * len(vs), [None] * len(vs)
        for rnd in range(a.rounds + 1):
            for i, (v, r) in enumerate(zip(vs, ctx)):
                apply_env(v, keys, saved)
                r.set_image_size(W, H)
                r.set_jit(1)
                if path is None:
                    r.load_builtin(variant)
                else:
                    r.load_scene(path, variant)
                r.set_params(abi.default_params(max_bounces=bounces))
                if v["cull"] is not None:
                    r.set_culling(v["cull"])
                if v["shade"] is not None:
                    r.set_tuning(v["shade"], -1, 0)
                if v["trail"] is not None:
                    r.set_trail_steps(v["trail"])
                if v["tune"] is not None:
                    r.set_trail_tuning(*v["tune"])
                r.reload()
                r.reset_stats()
                r.render_spp(times)
                s = r.stats()
                if rnd:
                    ms[i].append(s.trace_ms)
                if rnd == a.rounds:
                    img[i], st[i], cnt[i] = r.read_accum(), s, r.counters(ncnt(v))
        apply_env({"env": {}}, keys, saved)
        t0 = float(np.median(ms[0]))
        out = {"case": name, "W": W, "H": H, "spp": spp, "bounces": bounces}
        for i, v in enumerate(vs):
            t = np.array(ms[i])
            out[v["label"]] = {
                "median_ms": round(float(np.median(t)), 3), "min_ms": round(float(t.min()), 3),
                "vs_first": round(float(np.median(t)) / t0, 4),
                "Msamples_s": round(W * H * spp / float(np.median(t)) / 1e3, 1),
                "map_evals": int(st[i].map_evals), "map_iters": int(st[i].map_iters),
                "shade_batches": int(st[i].shade_batches),
                "lanes_per_batch": round(cnt[i][8] / max(1, st[i].shade_batches), 2),
                "overflow_deposits": cnt[i][16],
                "bitwise_equal_to_first": bool(np.array_equal(img[i].view(np.uint32), img[0].view(np.uint32))),
            }
            if v["trail"] is not None or v["tune"] is not None:   # rmr_internal.h kCntTrail*: steps taken, passes, lanes evaluated in them
                c = cnt[i]
                out[v["label"]]["trail"] = {
                    "steps": c[31], "passes": c[32], "lanes": c[33],
                    "steps_share_of_march_evals": round(c[31] / max(1, c[0] - c[14]), 4),
                    "accepted_share": round(c[31] / max(1, c[33]), 4),
                    "lanes_per_pass": round(c[33] / max(1, c[32]), 2), "passes_per_iter": round(c[32] / max(1, c[1]), 3)}
            if a.raw:
                out[v["label"]]["raw"] = cnt[i]
            if "-DRMR_PROFILE" in v["env"].get("RMR_JIT_OPTS", ""):
                # section cycles of the profiling build (rmr_trace.h RMR_PROFILE: counters 4-7, 9, and its
                # own slots from 17 up, rmr_internal.h kCntProf*),
                # as fractions of the waves' cycles (the s_memtime stamps themselves cost ~10%)
                c, tot = cnt[i], max(1, cnt[i][7])
                out[v["label"]]["sections"] = {"refill": round(c[4] / tot, 4), "map_loop": round(c[5] / tot, 4),
                                               "shade": round(c[6] / tot, 4), "cache_full_maps": round(c[9] / tot, 4),
                                               # parts of refill: work-queue claims, the chunk's primary rays
                                               "refill_claims": round(c[17] / tot, 4), "refill_rays": round(c[18] / tot, 4)}
                if len(c) >= 74 and c[32]:   # trailing passes by pass index (the last: that index and later)
                    rows = {}
                    for e, tag in enumerate(("queue_has_work", "queue_used_up")):
                        for k in range(4):
                            n, qm, um, act, fin = c[34 + (4 * e + k) * 5:39 + (4 * e + k) * 5]
                            if n:
                                rows["%s_pass%d" % (tag, k)] = {
                                    "passes": n, "lanes_taking_part": round(qm / n, 2), "lanes_accepted": round(um / n, 2),
                                    "active_lanes": round(act / n, 2), "finished_lanes_sitting": round(fin / n, 2)}
                    out[v["label"]]["trail_passes"] = rows
                if c[3]:   # cache kernels: lanes per full map() batch
                    out[v["label"]]["lanes_per_full_batch"] = round(c[21] / c[3], 2)
                if c[22]:   # lane-slot kernels: the schedule's own counts, per map-loop iteration / per batch
                    it, nb = max(1, c[1]), max(1, c[2])
                    out[v["label"]]["schedule"] = {
                        "outer_passes": c[22], "park_steps": c[23], "park_steps_overflow": c[24], "batches": c[2],
                        "events_per_batch": round(c[27] / nb, 2),
                        "lanes_per_map_iter": round((c[0] - c[14]) / it, 2),
                        "lanes_awaiting_park_per_iter": round(c[25] / it, 3),
                        "lanes_waiting_full_slot_per_iter": round(c[26] / it, 3),
                        "lanes_idle_per_iter": round(c[28] / it, 3), "lanes_idle_drain_per_iter": round(c[29] / it, 3),
                        "ready_rays_waiting_per_iter": round(c[30] / it, 3)}
        print(json.dumps(out), flush=True)
    for r in ctx:
        r.close()


if __name__ == "__main__":
    main()
