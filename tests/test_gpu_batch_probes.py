"""Batch probes (rmr_trace.h RMR_BATCH_PROBES): in the lane-slot kernels a hit that am_normal_cert does
not certify parks like a certified one, and getNormal's six probes run on the whole map in the shading
batch, spread over the wave (probe_normals), instead of as six map-loop iterations of the hit's lane.
Every sample must keep its bits: against the CPU oracle, against the same launch with the switch off
(the in-loop probes), and against the class's kernel without lane slots.

The Cornell scenes hardly reach the new path (a fraction of a percent of their hits is uncertified), so
the scenes here lay an overlay slab on the floor whose top face is 0.0005 above the floor's: inside the
certificate's margin over the whole overlay. Each scene first has to show, on the CPU oracle alone, that
at least 10 % of the frame's primary hits have their two smallest primitive distances within 0.002.

Also here: the eye step with the chunk's rays (RMR_EYE_CHUNK) where a launch has no uniform "march on"
(an eye on a surface, max_steps = 1) and keeps the per-refill step."""
import os

import numpy as np
import pytest

from oracle import camera, oracle, scene_compile
from raymarchrenderer_amd import Renderer, abi, time_schedule

from .conftest import SCENES
from .scene_family import H0, RECT0, W0, _box, _diffuse, _primary_dirs, _sphere   # noqa: F401 (other tests import them from here)

pytestmark = pytest.mark.gpu

CORNELL = os.path.join(SCENES, "cornell5.scene")
TUNINGS = [(1, 1), (8, 32), (20, 64)]


def overlay_scene(overlay_r):
    """Floor, overlay slab 0.0005 above it, wall, sphere, emissive box (scene order matters: opU)."""
    mats = [_diffuse(0, [0.8, 0.8, 0.8]), _diffuse(1, [0.8, 0.1, 0.1]), _diffuse(2, [0.1, 0.8, 0.1]),
            _diffuse(3, [0.2, 0.3, 0.8]),
            {"id": 4, "total_vars": 1, "nodes": [{"name": "shader_emission", "inputs": [[1.0, 1.0, 1.0], [16, 16, 16]],
                                                  "outputs": [0]}], "color": 0, "dir": -1}]
    objs = [_box(0, [0, -1.025, 0], [4, 0.05, 4]),
            _box(1, [0, -1.0245, 0], [overlay_r, 0.05, overlay_r]),
            _box(2, [-3, 1, 0], [0.05, 3, 4]),
            _sphere(3, [0.8, -0.475, 0.5], 0.5),
            _box(4, [-0.8, -0.475, 0.5], [0.5, 0.5, 0.5])]
    return {"materials": mats, "objects": objs}


SCENE_DICTS = {"overlay2": overlay_scene(2), "overlay4": overlay_scene(4)}


def _same(a, b):
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def near_tie_share(scene):
    """Share of the frame's primary hits whose two smallest primitive distances are within 0.002."""
    tables = scene_compile.compile_scene(scene, "rm1")
    singles = [scene_compile.compile_scene({"materials": scene["materials"], "objects": [o]}, "rm1")
               for o in scene["objects"]]
    view = camera.default_view(W0, H0)
    eye = np.asarray(view[:3], np.float32)
    hits = ties = 0
    for d in _primary_dirs(view, W0, H0, RECT0):
        t, _ = oracle.march(tables, eye, d)
        if not t < 1000.0:
            continue
        p = eye + np.float32(t) * d
        ds = sorted(float(oracle.map_p(s, p)[0]) for s in singles)
        hits += 1
        ties += ds[1] - ds[0] <= 0.002
    return ties / max(1, hits), hits


@pytest.fixture(scope="module")
def scenes():
    """Per scene and max_bounces: the oracle's samples (computed once, read-only), after the condition
    that the scene exercises the uncertified path at all."""
    out = {}
    times = time_schedule(3, frame=1)
    view = camera.default_view(W0, H0)
    for name, sc in SCENE_DICTS.items():
        share, hits = near_tie_share(sc)
        assert hits > 500 and share >= 0.10, "%s: %.1f %% of %d primary hits are near ties" % (name, 100 * share, hits)
        tables = scene_compile.compile_scene(sc, "rm1")
        for mb in (1, 4):
            cpu = oracle.Oracle(tables, abi.default_params(max_bounces=mb), view, W0, H0).trace_samples(times, RECT0)
            cpu.setflags(write=False)
            out[name, mb] = cpu
    return times, out


@pytest.fixture(scope="module")
def diag_renderers():
    """Two contexts of the diagnostic library (it reads RMR_JIT_BPROBES at specialisation time): the
    switch at its default and forced off. Separate JIT cache keys: the switch is in the source."""
    saved = os.environ.get("RMR_JIT_BPROBES")
    rs = {}
    try:
        for tag in ("on", "off"):
            r = Renderer(0, W0, H0, diag=True)
            r.set_jit(1)
            rs[tag] = r
        yield rs
    finally:
        for r in rs.values():
            r.close()
        if saved is None:
            os.environ.pop("RMR_JIT_BPROBES", None)
        else:
            os.environ["RMR_JIT_BPROBES"] = saved


def _render(rs, tag, scene, times, rect=RECT0, tuning=None, lane_slots=True, view=None, **kw):
    """trace_samples of `scene` in context `tag`; the kernel is specialised under that tag's switch."""
    r = rs[tag]
    if tag == "off":
        os.environ["RMR_JIT_BPROBES"] = "0"
    else:
        os.environ.pop("RMR_JIT_BPROBES", None)
    r.set_image_size(W0, H0)
    r.reload()
    r.load_scene(scene, "rm1")
    r.set_params(abi.default_params(**kw))
    r.set_view(camera.default_view(W0, H0) if view is None else view)
    if not lane_slots:
        r.set_tuning(lane_slots=False)
    elif tuning is not None:
        r.set_tuning(park=tuning[0], slot_batch=tuning[1])
    else:
        r.set_tuning(lane_slots=True)
    r.reset_stats()
    gpu = r.trace_samples(times, rect)
    st = r.stats()
    assert st.jit_launches > 0 and st.jit_launches == st.trace_launches
    r.set_tuning(lane_slots=True)
    return gpu, st


@pytest.mark.parametrize("mb", [1, 4])
@pytest.mark.parametrize("park,batch", TUNINGS)
@pytest.mark.parametrize("name", sorted(SCENE_DICTS))
def test_overlay_bitexact(diag_renderers, scenes, name, park, batch, mb):
    times, cpus = scenes
    cpu = cpus[name, mb]
    sc = SCENE_DICTS[name]
    on, st_on = _render(diag_renderers, "on", sc, times, tuning=(park, batch), max_bounces=mb)
    eq = _same(on[..., :3], cpu[..., :3])
    assert eq.all(), "%s (P, T2) = (%d, %d) b%d vs oracle: %d samples differ" % (name, park, batch, mb, (~eq.all(axis=-1)).sum())
    off, st_off = _render(diag_renderers, "off", sc, times, tuning=(park, batch), max_bounces=mb)
    eq = _same(on, off)
    assert eq.all(), "%s (P, T2) = (%d, %d) b%d vs switch off: %d values differ" % (name, park, batch, mb, (~eq).sum())
    # the switch did something: the park step skips the probes of uncertified hits that end their path
    # (every hit at max_bounces = 1; emission and last-bounce hits at 4), so fewer map() evaluations
    assert st_on.map_evals < st_off.map_evals
    noslots, _ = _render(diag_renderers, "on", sc, times, lane_slots=False, max_bounces=mb)
    eq = _same(on, noslots)
    assert eq.all(), "%s (P, T2) = (%d, %d) b%d vs lane slots off: %d values differ" % (name, park, batch, mb, (~eq).sum())


def _eye_on_surface_view():
    """The default camera moved so that the eye lies on the unit sphere's surface (map(eye) < 0.001)."""
    d = np.array([0.0, -3.0, 6.0])
    d = d / np.linalg.norm(d)
    # on the sphere of radius 1 about the origin, looking through it (x = +0: a -0 eye coordinate
    # turns the eye step off altogether, rmr_api.cpp view_params)
    eye = (0.0, float(-d[1]), float(-d[2]))
    return camera.view_uniforms(eye, tuple(float(x) for x in d), float(W0) / float(H0), np.float32(3.141592653) / np.float32(4))


@pytest.mark.parametrize("case", ["eye_on_surface", "max_steps_1"])
def test_eye_step_fallback(diag_renderers, case):
    """Launches without a uniform first step (the eye within 0.001 of a surface: the step is a hit;
    max_steps = 1: the step is the last) keep the per-refill march_update, batch probes included."""
    times = time_schedule(3, frame=1)
    kw = {"max_bounces": 4}
    view = camera.default_view(W0, H0)
    if case == "eye_on_surface":
        view = _eye_on_surface_view()
        tables = scene_compile.load_scene_file(CORNELL, "rm1")
        assert abs(float(oracle.map_p(tables, view[:3])[0])) < 0.001
    else:
        kw["max_steps"] = 1
    prm = abi.default_params(**kw)
    cpu = oracle.Oracle(scene_compile.load_scene_file(CORNELL, "rm1"), prm, view, W0, H0).trace_samples(times, RECT0)
    on, _ = _render(diag_renderers, "on", CORNELL, times, view=view, **kw)
    eq = _same(on[..., :3], cpu[..., :3])
    assert eq.all(), "%s vs oracle: %d samples differ" % (case, (~eq.all(axis=-1)).sum())
    off, _ = _render(diag_renderers, "off", CORNELL, times, view=view, **kw)
    assert _same(on, off).all()
    noslots, _ = _render(diag_renderers, "on", CORNELL, times, lane_slots=False, view=view, **kw)
    assert _same(on, noslots).all()
