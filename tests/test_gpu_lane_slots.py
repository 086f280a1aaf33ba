"""Lane slots (rmr_trace.h RMR_LANE_SLOTS): each lane of RM1's certified sphere/box kernels owns a second
path in an LDS slot. The schedule moves work between a lane's registers and its slot only, so every
sample must keep its bits: against the CPU oracle, and against the same kernel class with the schedule off.

Why no (P, T2) can hang the persistent loop, (20, 64) included, where the batch threshold is out of
reach (a wave has 64 slots, and a slot holding an event makes its lane wait rather than add another):
every pass of the outer loop either runs the map loop, which ends after at most max_steps steps per
active lane, or has no active lane. With no active lane the batch fires whenever a slot holds an event
(the "no active lane" trigger), and a batch empties every event slot; the lanes that waited in registers
then park, which at most fires one more batch. With no active lane and no event, every lane that is not
idle would be waiting on an event slot, so every lane is idle: those with a ready ray take it, the others
refill (the refill's own "no active lane" trigger) until the queue is used up, and the loop ends once
no lane, no slot and no unit is left."""
import json
import math
import os

import numpy as np
import pytest

from oracle import camera, oracle, scene_compile
from oracle.envmap import synthetic_env
from raymarchrenderer_amd import abi, time_schedule

from .conftest import SCENES

pytestmark = pytest.mark.gpu

CORNELL = os.path.join(SCENES, "cornell5.scene")
SPHERE1 = os.path.join(SCENES, "sphere1.scene")


def _same(a, b):
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def _setup(r, scene, W, H, **kw):
    r.set_image_size(W, H)
    r.reload()
    r.load_scene(scene, "rm1")
    prm = abi.default_params(**kw)
    r.set_params(prm)
    view = camera.default_view(W, H)
    r.set_view(view)
    r.set_env_map(synthetic_env() if prm.use_env_tex else None)
    return prm, view


@pytest.fixture
def jit_renderer(renderer):
    """The specialised kernels at every size; tuning and grid back to their defaults afterwards."""
    renderer.set_jit(1)
    try:
        yield renderer
    finally:
        renderer.set_jit(2)
        renderer.set_grid_reserve(0)
        renderer.set_tuning(lane_slots=True)   # on where the class has it, its own thresholds
        renderer.set_env_map(None)


W0, H0, RECT0 = 72, 40, (3, 5, 67, 38)   # the clip rect cuts 8x8 tiles on every side


@pytest.fixture(scope="module")
def cornell_oracle():
    prm = abi.default_params(max_bounces=4)
    view = camera.default_view(W0, H0)
    times = time_schedule(3, frame=1)
    cpu = oracle.Oracle(scene_compile.load_scene_file(CORNELL, "rm1"), prm, view, W0, H0).trace_samples(times, RECT0)
    cpu.setflags(write=False)
    return times, cpu


@pytest.mark.parametrize("park,batch", [(1, 1), (8, 24), (16, 48), (20, 64)])
def test_cornell5_slots_bitexact_vs_oracle(jit_renderer, cornell_oracle, park, batch):
    r = jit_renderer
    times, cpu = cornell_oracle
    _setup(r, CORNELL, W0, H0, max_bounces=4)
    r.set_tuning(park=park, slot_batch=batch)
    r.reset_stats()
    gpu = r.trace_samples(times, RECT0)
    assert r.stats().jit_launches > 0
    eq = _same(gpu[..., :3], cpu[..., :3])
    assert eq.all(), "(P, T2) = (%d, %d): %d samples differ" % (park, batch, (~eq.all(axis=-1)).sum())


def _c5_scene(frame):
    """bench.py's C5: Cornell-5 with the sphere centre y = 0.5 sin(2 pi f / 120)."""
    with open(CORNELL) as f:
        sc = json.load(f)
    sc["objects"][3]["nodes"][0]["inputs"][1][1] = 0.5 * math.sin(2.0 * math.pi * frame / 120.0)
    return sc


ON_OFF = [
    ("cornell5_b1", CORNELL, {"max_bounces": 1}),
    ("cornell5_b2", CORNELL, {"max_bounces": 2}),
    ("cornell5_b4", CORNELL, {"max_bounces": 4}),
    ("sphere1_b1", SPHERE1, {"max_bounces": 1}),   # every event ends its path
    ("cornell5_sepch", CORNELL, {"max_bounces": 4, "separate_channels": 1}),
    ("sphere1_env", SPHERE1, {"max_bounces": 4, "use_env_tex": 1}),
    ("c5_frame37_live", None, {"max_bounces": 4}),   # the live-primitive kernel
]


@pytest.mark.parametrize("name,scene,kw", ON_OFF, ids=[c[0] for c in ON_OFF])
def test_slots_on_equals_off(jit_renderer, name, scene, kw):
    r = jit_renderer
    W, H, spp = 64, 48, 3
    times = time_schedule(spp, frame=37)
    img, evals = {}, {}
    for on in (True, False):
        if scene is None:   # frame 0 bakes the layout's kernel, frame 37 makes the sphere a loaded primitive
            _setup(r, _c5_scene(0), W, H, **kw)
            r.set_tuning(lane_slots=on)
            r.render_spp(time_schedule(1, frame=0))
            _setup(r, _c5_scene(37), W, H, **kw)
        else:
            _setup(r, scene, W, H, **kw)
        r.set_tuning(lane_slots=on)
        r.reset_stats()
        r.render_spp(times)
        st = r.stats()
        assert st.jit_launches > 0
        img[on], evals[on] = r.read_accum(), st.map_evals
    eq = _same(img[True], img[False])
    assert eq.all(), "%s: %d values differ" % (name, (~eq).sum())
    if name == "cornell5_b4":
        # the schedule ran: hits that end their path (emission, last bounce) skip getNormal's probes
        assert evals[True] < evals[False]
    if "sepch" in name or "env" in name:
        # launches the schedule does not cover run the class's kernel without it
        assert evals[True] == evals[False]


@pytest.mark.parametrize("park,batch", [(8, 48), (2, 6)])
def test_slot_reuse_and_drain_one_block(jit_renderer, park, batch):
    """One workgroup for 16,384 units: every wave runs tens of chunks, ready rays compete with fresh
    units at each refill, and the last slots flush after the queue is empty. Then a launch of fewer
    units than a wave has lanes."""
    r = jit_renderer
    W, H, spp = 64, 64, 4
    prm, view = _setup(r, CORNELL, W, H, max_bounces=4)
    times = time_schedule(spp, frame=2)
    r.set_tuning(park=park, slot_batch=batch)
    r.set_grid_reserve(1 << 20)
    r.render_spp(times)
    gpu = r.read_accum()
    cpu = oracle.Oracle(scene_compile.load_scene_file(CORNELL, "rm1"), prm, view, W, H).render(times)
    eq = _same(gpu, cpu)
    assert eq.all(), "%d values differ" % (~eq).sum()
    r.set_grid_reserve(0)
    rect = (29, 30, 34, 33)   # 5 x 3 pixels of the 8x8 tile at (24, 24)
    t1 = time_schedule(1, frame=3)
    g1 = r.trace_samples(t1, rect)
    c1 = oracle.Oracle(scene_compile.load_scene_file(CORNELL, "rm1"), prm, view, W, H).trace_samples(t1, rect)
    assert _same(g1[..., :3], c1[..., :3]).all()
