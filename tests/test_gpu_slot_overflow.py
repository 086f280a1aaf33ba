"""Overflow deposit (rmr_trace.h RMR_SLOT_OVERFLOW): in the lane-slot kernels a lane whose march ended in a
continuing hit while its own slot still holds an event puts the event into an empty slot of the wave
(csrc/rmr_slot_rule.h) and goes idle, instead of waiting in registers for the next batch. The batch shades
slot i in lane i, whoever produced the event, and the ready ray stays in that slot: a path may change
lanes, and nothing in a sample depends on its lane. So every sample keeps its bits: against the CPU oracle,
and against the same kernel with the switch off.

Why no (P, T2) can hang the persistent loop with the deposit in it (the argument of
tests/test_gpu_lane_slots.py, which this one extends): a deposit only turns an empty slot into an event
slot and frees a lane. It never creates a waiting lane, and it never removes an event without a batch. The
map loop's exit (at most max_steps steps per active lane), the two "no active lane" triggers (of the batch
and of the refill) and the end condition (no live lane, the queue used up, no slot in use) are untouched.
The lane-slot argument therefore holds with "a lane waits only when its own slot holds an event and no slot
is empty" in the place of "a lane waits when its own slot holds an event": every pass of the outer loop
either runs the map loop or has no active lane; with no active lane the batch fires whenever a slot holds
an event, and a batch empties every event slot, after which the waiting lanes park (own slot first, then
any empty one), which fires at most one more batch; with no active lane and no event no lane can be
waiting, since a waiting lane's own slot holds an event, so every lane is idle: those with a ready ray take
it, the others refill until the queue is used up, and the loop ends once no lane, no slot and no unit is
left. csrc/slot_rule_test.cpp runs this schedule on the host for P in {1, 8, 20, 255} and T2 in {1, 24, 32,
48, 56, 64, 255} through the queue's exhaustion (tests/test_slot_rule_cpu.py).

The contexts are the diagnostic library's (it reads RMR_JIT_OVERFLOW at specialisation time), so the tests
hold whatever the switch's default is."""
import json
import math
import os

import numpy as np
import pytest

from oracle import camera, oracle, scene_compile
from oracle.envmap import synthetic_env
from raymarchrenderer_amd import Renderer, abi, time_schedule

from .conftest import SCENES

pytestmark = pytest.mark.gpu

CORNELL = os.path.join(SCENES, "cornell5.scene")
SPHERE1 = os.path.join(SCENES, "sphere1.scene")
OVERFLOW_COUNTER = 16   # rmr_internal.h kCntOverflow: events deposited into another lane's slot
ENV = ("RMR_JIT_OVERFLOW", "RMR_SMALL_CHUNK")


def _same(a, b):
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


@pytest.fixture(scope="module")
def diag_renderers():
    """Two contexts of the diagnostic library: the switch forced on and forced off (separate code-object
    keys: the switch is part of the generated source)."""
    saved = {k: os.environ.get(k) for k in ENV}
    rs = {}
    try:
        for tag in ("on", "off"):
            r = Renderer(0, 64, 64, diag=True)
            r.set_jit(1)
            rs[tag] = r
        yield rs
    finally:
        for r in rs.values():
            r.close()
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _load(rs, tag, scene, W, H, small_chunk=None, **kw):
    """`scene` in context `tag`, its kernel specialised under that tag's switch."""
    r = rs[tag]
    os.environ["RMR_JIT_OVERFLOW"] = "1" if tag == "on" else "0"
    if small_chunk is None:
        os.environ.pop("RMR_SMALL_CHUNK", None)
    else:
        os.environ["RMR_SMALL_CHUNK"] = str(small_chunk)
    r.set_image_size(W, H)
    r.reload()
    r.load_scene(scene, "rm1")
    prm = abi.default_params(**kw)
    r.set_params(prm)
    view = camera.default_view(W, H)
    r.set_view(view)
    r.set_env_map(synthetic_env() if prm.use_env_tex else None)
    r.set_tuning(lane_slots=True)
    return r, prm, view


W0, H0, RECT0 = 72, 40, (3, 5, 67, 38)   # the clip rect cuts 8x8 tiles on every side


@pytest.fixture(scope="module")
def cornell_oracle():
    prm = abi.default_params(max_bounces=4)
    view = camera.default_view(W0, H0)
    times = time_schedule(3, frame=1)
    cpu = oracle.Oracle(scene_compile.load_scene_file(CORNELL, "rm1"), prm, view, W0, H0).trace_samples(times, RECT0)
    cpu.setflags(write=False)
    return times, cpu


@pytest.mark.parametrize("park,batch", [(1, 1), (8, 48), (8, 56), (2, 64), (20, 64), (20, 255)])
def test_cornell5_overflow_bitexact_vs_oracle(diag_renderers, cornell_oracle, park, batch):
    """The launch's 8,640 units on the whole chip, then in one workgroup. On the whole chip the launch is
    135 waves of one 64-unit claim each: every lane marches one fresh unit, a lane whose event waits in its
    slot has nothing else to march, and the deposit counter stays 0 at every (P, T2) (measured; no rect
    or sample count of a test's size changes that, a wave gets a second claim only beyond 393,216 units).
    In one workgroup the four waves run some 34 claims each, lanes march while their slot holds an event,
    and the counter must show the new path where T2 >= 48. Same rect, samples and oracle for both."""
    times, cpu = cornell_oracle
    r, _, _ = _load(diag_renderers, "on", CORNELL, W0, H0, max_bounces=4)
    r.set_tuning(park=park, slot_batch=batch)
    dep = {}
    try:
        for reserve in (0, 1 << 20):
            r.set_grid_reserve(reserve)
            r.reset_stats()
            gpu = r.trace_samples(times, RECT0)
            st, dep[reserve] = r.stats(), r.counters()[OVERFLOW_COUNTER]
            print("(P, T2) = (%d, %d) reserve %d: %d overflow deposits, %d batches" % (park, batch, reserve, dep[reserve], st.shade_batches))
            assert st.jit_launches > 0 and st.jit_launches == st.trace_launches
            eq = _same(gpu[..., :3], cpu[..., :3])
            assert eq.all(), "(P, T2) = (%d, %d) reserve %d: %d samples differ" % (park, batch, reserve, (~eq.all(axis=-1)).sum())
    finally:
        r.set_grid_reserve(0)
        r.set_tuning(lane_slots=True)
    if batch >= 48:   # the new path ran
        assert dep[1 << 20] > 0


def _c5_scene(frame):
    """bench.py's C5: Cornell-5 with the sphere centre y = 0.5 sin(2 pi f / 120)."""
    with open(CORNELL) as f:
        sc = json.load(f)
    sc["objects"][3]["nodes"][0]["inputs"][1][1] = 0.5 * math.sin(2.0 * math.pi * frame / 120.0)
    return sc


ON_OFF = [   # tests/test_gpu_lane_slots.py ON_OFF; slots: the launch runs the lane-slot schedule
    ("cornell5_b1", CORNELL, {"max_bounces": 1}, True),
    ("cornell5_b2", CORNELL, {"max_bounces": 2}, True),
    ("cornell5_b4", CORNELL, {"max_bounces": 4}, True),
    ("sphere1_b1", SPHERE1, {"max_bounces": 1}, True),   # every event ends its path: no slot event at all
    ("cornell5_sepch", CORNELL, {"max_bounces": 4, "separate_channels": 1}, False),
    ("sphere1_env", SPHERE1, {"max_bounces": 4, "use_env_tex": 1}, False),
    ("c5_frame37_live", None, {"max_bounces": 4}, True),   # the live-primitive kernel
]


@pytest.mark.parametrize("name,scene,kw,slots", ON_OFF, ids=[c[0] for c in ON_OFF])
def test_overflow_on_equals_off(diag_renderers, name, scene, kw, slots):
    W, H, spp = 64, 48, 3
    times = time_schedule(spp, frame=37)
    img, dep, evals = {}, {}, {}
    for tag in ("on", "off"):
        if scene is None:   # frame 0 bakes the layout's kernel, frame 37 makes the sphere a loaded primitive
            r, _, _ = _load(diag_renderers, tag, _c5_scene(0), W, H, **kw)
            r.render_spp(time_schedule(1, frame=0))
            r, _, _ = _load(diag_renderers, tag, _c5_scene(37), W, H, **kw)
        else:
            r, _, _ = _load(diag_renderers, tag, scene, W, H, **kw)
        r.reset_stats()
        r.render_spp(times)
        st = r.stats()
        assert st.jit_launches > 0
        img[tag], dep[tag], evals[tag] = r.read_accum(), r.counters()[OVERFLOW_COUNTER], st.map_evals
        r.set_env_map(None)
    print("%s: overflow deposits on %d, off %d" % (name, dep["on"], dep["off"]))
    eq = _same(img["on"], img["off"])
    assert eq.all(), "%s: %d values differ" % (name, (~eq).sum())
    assert dep["off"] == 0
    assert evals["on"] == evals["off"]   # the schedule moves events, it adds and removes no map()
    if not slots or name == "sphere1_b1":
        assert dep["on"] == 0


def test_overflow_drain(diag_renderers):
    """The drain with the queue used up while slots still hold events and rays: one 8x8 tile at one sample
    (a single wave's 64 units, no refill after the first), and a 64x48 launch whose waves claim 8 units at
    a time (chunk_units small), in one workgroup so that its four waves run the whole launch."""
    W, H = 64, 48
    r, prm, view = _load(diag_renderers, "on", CORNELL, W, H, small_chunk=8, max_bounces=4)
    tables = scene_compile.load_scene_file(CORNELL, "rm1")
    rect = (24, 24, 32, 32)
    t1 = time_schedule(1, frame=3)
    r.set_tuning(park=8, slot_batch=48)
    g1 = r.trace_samples(t1, rect)
    c1 = oracle.Oracle(tables, prm, view, W, H).trace_samples(t1, rect)
    assert _same(g1[..., :3], c1[..., :3]).all()
    times = time_schedule(3, frame=2)
    cpu = oracle.Oracle(tables, prm, view, W, H).render(times)
    for reserve in (0, 1 << 20):   # every CU (8-unit claims), then one workgroup
        r.set_grid_reserve(reserve)
        r.reset_stats()
        r.render_spp(times)
        gpu, dep = r.read_accum(), r.counters()[OVERFLOW_COUNTER]
        print("reserve %d: %d overflow deposits" % (reserve, dep))
        eq = _same(gpu, cpu)
        assert eq.all(), "reserve %d: %d values differ" % (reserve, (~eq).sum())
    r.set_grid_reserve(0)
    r.set_tuning(lane_slots=True)
    assert dep > 0   # (one workgroup: each wave runs tens of claims)
