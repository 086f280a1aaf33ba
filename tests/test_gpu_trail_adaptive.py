"""The trailing passes chosen per wave (rmr_set_trail_tuning; rmr_trace.h, the pass rule; rmr_trail_rule.h
trail_word) on the GPU. After each pass a wave takes another one iff fewer than k_max have run, the lanes
still taking part are at least ratio / 8 of its active lanes and, with the park exit, its finished lanes are
still fewer than the park threshold. The rule chooses how many passes run and nothing else, so every tuning
renders the oracle's bits, makes the same map() calls, and keeps the kernel's own counts consistent.

Scenes: Cornell-5 at 96 x 54, 4 samples, 4 bounces (12 x 7 tiles of 8 x 8 a sample, the last row clipped: work
for several waves); the same at 8 x 8, 1 sample (one tile: less than one wave's first claim, so every wave
drains from the start);
and three generated scenes at 64 x 48, 2 samples, built as tests/test_gpu_trail_lean.py builds its own — eight
primitives (the largest table the LDS copy holds), the scene family's ground sphere of radius 10^4, and the
overlay slab 0.0005 above the floor (near ties, where the acceptance rule has to refuse) — which are also
compared with their own render without any pass.

map_evals: DESIGN.md §4.2 has it equal between schedules up to the last two of eleven digits, which the
refill order leaves free; the bound here is a millionth of the count (exact equality below 10^6 calls)."""
import os

import numpy as np
import pytest

from oracle import camera, oracle, scene_compile
from raymarchrenderer_amd import Renderer, abi, time_schedule
from raymarchrenderer_amd._lib import RMRError

from . import scene_family as sf
from .conftest import SCENES
from .test_gpu_batch_probes import _same, overlay_scene

pytestmark = pytest.mark.gpu

CORNELL = os.path.join(SCENES, "cornell5.scene")
TRAIL_STEPS, TRAIL_PASSES, TRAIL_LANES = 31, 32, 33   # rmr_internal.h kCntTrail*
WG, HG, RECTG = 64, 48, (3, 5, 61, 44)   # generated scenes: the clip rect cuts 8x8 tiles on every side

# (k_max, ratio in eighths, park exit)
TUNINGS = [(0, 0, False), (1, 0, False), (3, 0, False), (15, 0, False), (15, 8, True), (15, 3, True), (15, 1, True)]


def _dict_scene(layout):
    mats = [sf._diffuse(0, [0.8, 0.8, 0.8]), sf._diffuse(1, [0.8, 0.1, 0.1]), sf._diffuse(2, [0.1, 0.8, 0.1]),
            sf._diffuse(3, [0.2, 0.3, 0.8]), sf._diffuse(4, [0.8, 0.7, 0.2]), sf._diffuse(5, [0.6, 0.2, 0.7]), sf._emission(6)]
    objs = [sf._sphere(m, list(c), r) if kind == "s" else sf._box(m, list(c), list(r)) for kind, m, c, r in layout]
    return {"materials": mats, "objects": objs}


def _family_view():
    m = float(np.linalg.norm(sf.LOOK))
    return camera.view_uniforms(sf.EYE, tuple(x / m for x in sf.LOOK), float(WG) / float(HG), sf.PI32 / np.float32(4))


# name: scene, W, H, rect, samples, view, params, compared with its own (0, 0, off) render
CASES = {
    "cornell5_96x54": (CORNELL, 96, 54, (0, 0, 96, 54), 4, lambda: camera.default_view(96, 54), {}, False),
    "cornell5_8x8": (CORNELL, 8, 8, (0, 0, 8, 8), 1, lambda: camera.default_view(8, 8), {}, False),
    "prims8": (_dict_scene(sf._room5() + sf._clutter(3, 8)), WG, HG, RECTG, 2, _family_view, {}, True),
    "ground_1e4": (sf.scene("ground_1e4"), WG, HG, RECTG, 2, lambda: sf.view("ground_1e4", WG, HG),
                   {"max_dist": sf.max_dist("ground_1e4")}, True),
    "overlay4": (overlay_scene(4), WG, HG, RECTG, 2, lambda: camera.default_view(WG, HG), {}, True),
}


def _tables(scene):
    return scene_compile.load_scene_file(scene, "rm1") if isinstance(scene, str) else scene_compile.compile_scene(scene, "rm1")


def test_the_generated_scenes_are_what_they_are_here_for():
    assert len(CASES["prims8"][0]["objects"]) == 8
    assert any(o["nodes"][0]["name"] == "map_sphere" and o["nodes"][0]["inputs"][2][0] >= 9999.0
               for o in CASES["ground_1e4"][0]["objects"])
    floor, slab = (o["nodes"][0]["inputs"][1][1] for o in CASES["overlay4"][0]["objects"][:2])
    assert abs((slab - floor) - 0.0005) < 1e-9


@pytest.fixture(scope="module")
def ctx():
    """One context of the diagnostic library (it reads RMR_JIT_TRAIL at specialisation time) with the steps
    compiled in, whatever the class's default is."""
    saved = os.environ.get("RMR_JIT_TRAIL")
    os.environ["RMR_JIT_TRAIL"] = "1"
    r = Renderer(0, 64, 64, diag=True)
    r.set_jit(1)
    try:
        yield r
    finally:
        r.close()
        if saved is None:
            os.environ.pop("RMR_JIT_TRAIL", None)
        else:
            os.environ["RMR_JIT_TRAIL"] = saved


_oracles, _renders = {}, {}   # per scene / per scene and tuning, computed once and read-only


def _times(name):
    return time_schedule(CASES[name][4], frame=1)


def _oracle(name):
    if name not in _oracles:
        scene, W, H, rect, _, view, kw, _ = CASES[name]
        cpu = oracle.Oracle(_tables(scene), abi.default_params(max_bounces=4, **kw), view(), W, H).trace_samples(_times(name), rect)
        cpu.setflags(write=False)
        _oracles[name] = cpu
    return _oracles[name]


def _load(r, name):
    scene, W, H, _, _, view, kw, _ = CASES[name]
    os.environ["RMR_JIT_TRAIL"] = "1"
    r.set_image_size(W, H)
    r.reload()
    r.load_scene(scene, "rm1")
    r.set_params(abi.default_params(max_bounces=4, **kw))
    r.set_view(view())
    r.set_tuning(lane_slots=True)


def _render(r, name, tuning):
    if (name, tuning) not in _renders:
        _load(r, name)
        r.set_trail_tuning(*tuning)
        r.reset_stats()
        gpu = r.trace_samples(_times(name), CASES[name][3])
        st = r.stats()
        cnt = r.counters(34)
        r.set_trail_steps(-1)
        assert st.jit_launches > 0 and st.jit_launches == st.trace_launches
        gpu.setflags(write=False)
        _renders[name, tuning] = gpu, st, cnt
    return _renders[name, tuning]


@pytest.mark.parametrize("tuning", TUNINGS, ids=["k%d_r%d_%s" % (k, q, "px" if x else "nopx") for k, q, x in TUNINGS])
@pytest.mark.parametrize("name", list(CASES))
def test_every_tuning_renders_the_same_bits(ctx, name, tuning):
    k_max = tuning[0]
    gpu, st, cnt = _render(ctx, name, tuning)
    cpu = _oracle(name)
    eq = _same(gpu[..., :3], cpu[..., :3])
    assert eq.all(), "%s %s vs oracle: %d samples differ" % (name, tuning, (~eq.all(axis=-1)).sum())
    base, st0, cnt0 = _render(ctx, name, TUNINGS[0])
    if CASES[name][7]:
        eq = _same(gpu, base)
        assert eq.all(), "%s %s vs no pass: %d values differ" % (name, tuning, (~eq).sum())
    print("%s %s: map_evals %d (no pass: %d), iterations %d, trailing steps %d, passes %d, lanes evaluated %d"
          % (name, tuning, st.map_evals, st0.map_evals, st.map_iters, cnt[TRAIL_STEPS], cnt[TRAIL_PASSES], cnt[TRAIL_LANES]))
    assert abs(int(st.map_evals) - int(st0.map_evals)) <= int(st0.map_evals) // 10**6, (name, tuning, st.map_evals, st0.map_evals)
    assert cnt[TRAIL_STEPS] <= cnt[TRAIL_LANES] <= 64 * cnt[TRAIL_PASSES], (name, tuning, cnt[31:34])
    assert cnt[TRAIL_PASSES] <= k_max * st.map_iters, (name, tuning, cnt[TRAIL_PASSES], st.map_iters)
    if k_max == 0:
        assert cnt[TRAIL_PASSES] == 0 and cnt[TRAIL_STEPS] == 0 and cnt[TRAIL_LANES] == 0, (name, cnt[31:34])
    elif name.startswith("cornell5"):
        assert cnt[TRAIL_STEPS] > 0, (name, tuning)


def test_the_rule_changes_the_schedule(ctx):
    """The tunings are not one schedule under seven names: on Cornell-5 the cap alone runs the most passes and
    the fewest whole maps, the rule's tunings run fewer passes than the cap alone, and a ratio of 8 / 8, which
    takes a second pass only while every active lane takes part, runs the fewest of them. (Which wave claims
    which unit varies from run to run, so only differences of the schedule's own size are asserted.)"""
    name = "cornell5_96x54"
    passes = {t: _render(ctx, name, t)[2][TRAIL_PASSES] for t in TUNINGS}
    iters = {t: _render(ctx, name, t)[1].map_iters for t in TUNINGS}
    print(passes, iters)
    assert passes[(15, 0, False)] > passes[(3, 0, False)] > passes[(1, 0, False)] > 0
    assert passes[(15, 0, False)] > passes[(15, 3, True)] > passes[(15, 8, True)] > 0
    assert iters[(15, 0, False)] < iters[(3, 0, False)] < iters[(1, 0, False)] < iters[(0, 0, False)]


BAD = [((-1, 0, 0), "k_max"), ((16, 0, 0), "k_max"), ((3, -1, 0), "ratio_eighths"), ((3, 9, 0), "ratio_eighths"),
       ((3, 3, 2), "park_exit"), ((3, 3, -1), "park_exit")]


@pytest.mark.parametrize("args,word", BAD, ids=["%d_%d_%d" % a for a, _ in BAD])
def test_out_of_range_tunings_are_refused(ctx, args, word):
    code = ctx._L.rmr_set_trail_tuning(ctx._ctx, *args)
    assert code == -1   # RMR_E_INVALID
    msg = ctx._L.rmr_last_error(ctx._ctx).decode()
    assert "rmr_set_trail_tuning" in msg and word in msg and str(args[("k_max", "ratio_eighths", "park_exit").index(word)]) in msg, msg
    with pytest.raises(RMRError) as e:
        ctx.set_trail_tuning(*args)
    assert e.value.code == -1 and word in str(e.value)


def test_set_trail_steps_restores_the_fixed_schedule(ctx):
    """rmr_set_trail_steps(k) after a tuning: k passes behind every iteration that has a lane to take one, no
    rule — the counts of rmr_set_trail_tuning(k, 0, off), and not the tuning's that came before. On the 8 x 8
    frame: one unit, so one wave runs the whole launch and the counts repeat from run to run."""
    name = "cornell5_8x8"
    want = _render(ctx, name, (3, 0, False))
    ruled = _render(ctx, name, (15, 3, True))
    _load(ctx, name)
    ctx.set_trail_tuning(15, 3, True)
    ctx.set_trail_steps(3)
    ctx.reset_stats()
    gpu = ctx.trace_samples(_times(name), CASES[name][3])
    st, cnt = ctx.stats(), ctx.counters(34)
    ctx.set_trail_steps(-1)
    assert _same(gpu, want[0]).all()
    assert cnt[31:34] == want[2][31:34] and st.map_iters == want[1].map_iters, (cnt[31:34], want[2][31:34])
    assert cnt[TRAIL_PASSES] != ruled[2][TRAIL_PASSES]
    # an out-of-range count is refused and leaves the schedule as it was
    assert ctx._L.rmr_set_trail_steps(ctx._ctx, 16) == -1 and ctx._L.rmr_set_trail_steps(ctx._ctx, -2) == -1
