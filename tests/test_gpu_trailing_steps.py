"""Trailing steps (rmr_trace.h RMR_TRAIL_STEPS, rmr_trail_rule.h): behind each map-loop iteration's whole map
the lane-slot kernels take up to K march steps that evaluate the map's minimiser alone, wherever the
rule proves that the whole map would return the same pair. Scheduling only: every sample must keep its
bits — against the CPU oracle, against the kernel without the steps (the parent's instruction stream),
against the same kernel told to take none, and against the class's kernel without lane slots — and
map_evals, the number of map() calls the paths make, must not move.

Scenes: Cornell-5; the overlay scenes of test_gpu_batch_probes (near ties over the overlay: the rule has
to refuse there); the glass scene (node-program materials, marches from inside: another kernel class,
which takes no trailing step); a scene whose camera looks up at a diffuse face with normal (0, -1, 0),
whose bounce directions are NaN (randHemisphere's cross product with (0, 1, 0) vanishes).
Boundary cases put a march's ending on a trailing step: a step budget of 1-7, stepMultiply above 1 and
small, and maxDist inside the scene. The animated Cornell-5 runs the live-primitive kernel, whose sphere
a trailing step reads from the same table as the whole map."""
import json
import math
import os

import numpy as np
import pytest

from oracle import camera, oracle, scene_compile
from raymarchrenderer_amd import Renderer, abi, time_schedule

from .conftest import GOLDEN, SCENES
from .test_gpu_batch_probes import H0, RECT0, TUNINGS, W0, _box, _diffuse, _same, _sphere, overlay_scene

pytestmark = pytest.mark.gpu

CORNELL = os.path.join(SCENES, "cornell5.scene")
GLASS = os.path.join(GOLDEN, "scenes", "glass_test.scene")
TRAIL_STEPS, TRAIL_PASSES, TRAIL_LANES = 31, 32, 33   # rmr_internal.h kCntTrail*


def underface_scene():
    """A diffuse slab above the eye line: its bottom face, normal (0, -1, 0), fills the upper frame."""
    mats = [_diffuse(0, [0.8, 0.8, 0.8]), _diffuse(1, [0.8, 0.1, 0.1]), _diffuse(2, [0.2, 0.3, 0.8]),
            {"id": 3, "total_vars": 1, "nodes": [{"name": "shader_emission", "inputs": [[1.0, 1.0, 1.0], [16, 16, 16]],
                                                  "outputs": [0]}], "color": 0, "dir": -1}]
    objs = [_box(0, [0, -1.025, 0], [4, 0.05, 4]),
            _box(1, [0, 2.0, 0], [2.5, 0.05, 2.5]),
            _sphere(2, [0.6, -0.475, 0.3], 0.5),
            _box(3, [-1.5, -0.6, 0.5], [0.4, 0.4, 0.4]),
            _box(0, [3, 1, 0], [0.05, 3, 4])]
    return {"materials": mats, "objects": objs}


def underface_view():
    d = np.array([0.0, 0.3, 1.0])
    d = d / np.linalg.norm(d)
    return camera.view_uniforms((0.0, 0.0, -5.0), tuple(float(x) for x in d), float(W0) / float(H0),
                                np.float32(3.141592653) / np.float32(4))


# name: scene, view (None: the default camera), whether the class runs the lane slots
CORE = {
    "cornell5": (CORNELL, None, True),
    "overlay2": (overlay_scene(2), None, True),
    "overlay4": (overlay_scene(4), None, True),
    "glass": (GLASS, None, False),
    "underface": (underface_scene(), underface_view, True),
}


def _tables(scene):
    return scene_compile.load_scene_file(scene, "rm1") if isinstance(scene, str) else scene_compile.compile_scene(scene, "rm1")


def _view(name):
    v = CORE[name][1]
    return camera.default_view(W0, H0) if v is None else v()


@pytest.fixture(scope="module")
def times():
    return time_schedule(3, frame=1)


@pytest.fixture(scope="module")
def oracles(times):
    """Per scene and max_bounces: the oracle's samples, computed once and read-only."""
    out = {}
    for name, (scene, _, _) in CORE.items():
        for mb in (1, 4):
            cpu = oracle.Oracle(_tables(scene), abi.default_params(max_bounces=mb), _view(name), W0, H0).trace_samples(times, RECT0)
            cpu.setflags(write=False)
            out[name, mb] = cpu
    return out


def test_underface_scene_has_downward_hits():
    """The scene does what it is here for: primary rays end on the slab's bottom face (y = 1.95)."""
    tables = _tables(underface_scene())
    view = underface_view()
    eye = np.asarray(view[:3], np.float32)
    v = np.asarray(view, np.float64)
    n = 0
    for px, py in [(x, y) for x in range(8, W0, 8) for y in (8, H0 - 8)]:
        u, w = px / W0, py / H0
        top, bot = v[3:6] + (v[6:9] - v[3:6]) * u, v[9:12] + (v[12:15] - v[9:12]) * u
        d = top + (bot - top) * w
        d = (d / np.linalg.norm(d)).astype(np.float32)
        t, _ = oracle.march(tables, eye, d)
        n += bool(t < 1000.0 and abs(float(eye[1] + np.float32(t) * d[1]) - 1.95) < 0.01)
    assert n >= 4, n


@pytest.fixture(scope="module")
def ctxs():
    """Two contexts of the diagnostic library (it reads RMR_JIT_TRAIL at specialisation time): the steps
    compiled in, and the source without them. Separate JIT cache keys: the switch is in the source."""
    saved = os.environ.get("RMR_JIT_TRAIL")
    rs = {}
    try:
        for tag in ("trail", "off"):
            r = Renderer(0, W0, H0, diag=True)
            r.set_jit(1)
            rs[tag] = r
        yield rs
    finally:
        for r in rs.values():
            r.close()
        if saved is None:
            os.environ.pop("RMR_JIT_TRAIL", None)
        else:
            os.environ["RMR_JIT_TRAIL"] = saved


def _render(rs, tag, scene, times, k=None, tuning=None, lane_slots=True, view=None, prime=None, **kw):
    """trace_samples of `scene` in context `tag` with k trailing steps; (samples, stats, counters).
    prime: a scene rendered first with the same layout, so that `scene` runs the live-primitive kernel."""
    r = rs[tag]
    os.environ["RMR_JIT_TRAIL"] = "1" if tag == "trail" else "0"   # (whatever the class's default is)
    r.set_image_size(W0, H0)
    r.reload()
    r.load_scene(scene if prime is None else prime, "rm1")
    r.set_params(abi.default_params(**kw))
    r.set_view(camera.default_view(W0, H0) if view is None else view)
    if not lane_slots:
        r.set_tuning(lane_slots=False)
    elif tuning is not None:
        r.set_tuning(park=tuning[0], slot_batch=tuning[1])
    else:
        r.set_tuning(lane_slots=True)
    r.set_trail_steps(-1 if k is None else k)
    if prime is not None:
        r.render_spp(time_schedule(1, frame=0))
        r.load_scene(scene, "rm1")
    r.reset_stats()
    gpu = r.trace_samples(times, RECT0)
    st = r.stats()
    cnt = r.counters(34)
    assert st.jit_launches > 0 and st.jit_launches == st.trace_launches
    r.set_tuning(lane_slots=True)
    r.set_trail_steps(-1)
    return gpu, st, cnt


_refs = {}   # renders without the steps, shared by the K cases (read-only)


def _ref(rs, times, name, what, tuning, mb):
    key = (name, what, tuning if what != "noslots" else None, mb)
    if key not in _refs:
        scene = CORE[name][0]
        if what == "off":
            got = _render(rs, "off", scene, times, tuning=tuning, view=_view(name), max_bounces=mb)
        elif what == "k0":
            got = _render(rs, "trail", scene, times, k=0, tuning=tuning, view=_view(name), max_bounces=mb)
        else:
            got = _render(rs, "off", scene, times, lane_slots=False, view=_view(name), max_bounces=mb)
        got[0].setflags(write=False)
        _refs[key] = got
    return _refs[key]


@pytest.mark.parametrize("mb", [1, 4])
@pytest.mark.parametrize("park,batch", TUNINGS)
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("name", sorted(CORE))
def test_core_bitexact(ctxs, times, oracles, name, k, park, batch, mb):
    scene, _, slots = CORE[name]
    tag = "%s K %d (P, T2) = (%d, %d) b%d" % (name, k, park, batch, mb)
    on, st, cnt = _render(ctxs, "trail", scene, times, k=k, tuning=(park, batch), view=_view(name), max_bounces=mb)
    cpu = oracles[name, mb]
    eq = _same(on[..., :3], cpu[..., :3])
    assert eq.all(), "%s vs oracle: %d samples differ" % (tag, (~eq.all(axis=-1)).sum())
    off, st_off, cnt_off = _ref(ctxs, times, name, "off", (park, batch), mb)
    eq = _same(on, off)
    assert eq.all(), "%s vs the source without the steps: %d values differ" % (tag, (~eq).sum())
    k0, st_k0, cnt_k0 = _ref(ctxs, times, name, "k0", (park, batch), mb)
    eq = _same(on, k0)
    assert eq.all(), "%s vs K = 0: %d values differ" % (tag, (~eq).sum())
    noslots, _, _ = _ref(ctxs, times, name, "noslots", None, mb)
    eq = _same(on, noslots)
    assert eq.all(), "%s vs lane slots off: %d values differ" % (tag, (~eq).sum())
    # counter 0 stays the number of map() calls the paths make, whoever evaluates them
    assert st.map_evals == st_k0.map_evals == st_off.map_evals, (tag, st.map_evals, st_k0.map_evals, st_off.map_evals)
    assert cnt_off[TRAIL_STEPS] == 0 and cnt_k0[TRAIL_STEPS] == 0 and cnt_k0[TRAIL_PASSES] == 0
    march = cnt[0] - cnt[14]   # map() calls of the marches (without the batches' getNormal probes)
    print("%s: trailing steps %d of %d march evaluations (%.1f %%), %d passes, %.1f %% of %d evaluated lanes accepted, "
          "map-loop iterations %d (K = 0: %d)"
          % (tag, cnt[TRAIL_STEPS], march, 100.0 * cnt[TRAIL_STEPS] / max(1, march), cnt[TRAIL_PASSES],
             100.0 * cnt[TRAIL_STEPS] / max(1, cnt[TRAIL_LANES]), cnt[TRAIL_LANES], st.map_iters, st_k0.map_iters))
    assert cnt[TRAIL_STEPS] <= cnt[TRAIL_LANES] <= 64 * cnt[TRAIL_PASSES] and cnt[TRAIL_PASSES] <= k * st.map_iters
    if not slots:
        assert cnt[TRAIL_PASSES] == 0, tag   # another kernel class: its source has no trailing step
    if name == "cornell5":
        assert cnt[TRAIL_STEPS] > 0, tag
        assert st.map_iters < st_k0.map_iters, tag   # the steps replace whole-map iterations


BOUNDARY = [("max_steps_%d" % n, {"max_steps": n}) for n in (1, 2, 3, 4, 7)] + [
    ("step_mult_1.7", {"step_multiply": 1.7}), ("step_mult_0.25", {"step_multiply": 0.25}),
    # am_dmax, the past-maxDist rule and the escape bound all trigger inside the scene
    ("max_dist_6", {"max_dist": 6.0}),
]


@pytest.mark.parametrize("case,kw", BOUNDARY, ids=[c[0] for c in BOUNDARY])
def test_boundary_cases_bitexact(ctxs, times, case, kw):
    kw = dict(kw, max_bounces=4)
    view = camera.default_view(W0, H0)
    cpu = oracle.Oracle(_tables(CORNELL), abi.default_params(**kw), view, W0, H0).trace_samples(times, RECT0)
    for k in (1, 3):
        on, st, cnt = _render(ctxs, "trail", CORNELL, times, k=k, **kw)
        eq = _same(on[..., :3], cpu[..., :3])
        assert eq.all(), "%s K %d vs oracle: %d samples differ" % (case, k, (~eq.all(axis=-1)).sum())
        print("%s K %d: trailing steps %d, passes %d" % (case, k, cnt[TRAIL_STEPS], cnt[TRAIL_PASSES]))
        if kw.get("max_steps", 512) > 2:
            assert cnt[TRAIL_STEPS] > 0, case   # (the eye step and one map use up a budget of 1 or 2)


def _c5_scene(frame):
    """bench.py's C5: Cornell-5 with the sphere centre y = 0.5 sin(2 pi f / 120)."""
    with open(CORNELL) as f:
        sc = json.load(f)
    sc["objects"][3]["nodes"][0]["inputs"][1][1] = 0.5 * math.sin(2.0 * math.pi * frame / 120.0)
    return sc


@pytest.mark.parametrize("frame", [1, 37])
def test_animated_cornell5_live_primitive(ctxs, frame):
    """Frame 0 bakes the layout's kernel; a later frame makes the sphere a loaded primitive. The table a
    trailing step reads has to hold that frame's sphere."""
    times = time_schedule(3, frame=frame)
    sc = _c5_scene(frame)
    prm = abi.default_params(max_bounces=4)
    cpu = oracle.Oracle(_tables(sc), prm, camera.default_view(W0, H0), W0, H0).trace_samples(times, RECT0)
    on, st, cnt = _render(ctxs, "trail", sc, times, k=3, prime=_c5_scene(0), max_bounces=4)
    eq = _same(on[..., :3], cpu[..., :3])
    assert eq.all(), "frame %d vs oracle: %d samples differ" % (frame, (~eq.all(axis=-1)).sum())
    assert cnt[TRAIL_STEPS] > 0
    off, st_off, _ = _render(ctxs, "off", sc, times, prime=_c5_scene(0), max_bounces=4)
    assert _same(on, off).all() and st.map_evals == st_off.map_evals
