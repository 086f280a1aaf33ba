"""The trailing steps with the box-form table and the launch-constant eps (rmr_trail_rule.h trail_row,
trail_anchor_hi, trail_rule_hi; KParams::trail_eps_hi) on the GPU: scheduling only, so every sample keeps its
bits — against the CPU oracle and against the source without the steps — and map_evals does not move. The
diagnostic guard (-DRMR_TRAIL_CHECK) counts the lanes a pass evaluates at a point whose eps(p) exceeds the
launch's bound: none.

64 x 48, 2 samples, 4 bounces, K = 3. Scenes: Cornell-5; spheres only (every table row a sphere's); one
primitive (the runner-up is +inf); generated scenes of exactly 8 and of 9 primitives (the largest the LDS
table holds, and the first that reads the global table); a scene-family case 1000 away from the origin (eps
two orders larger); an eye far outside the scene (the bound's |eye| term); and a launch without the escape
bound, which has no bound of eps either: it must take no trailing step."""
import os

import numpy as np
import pytest

from oracle import camera, oracle, scene_compile
from raymarchrenderer_amd import Renderer, abi, time_schedule

from . import scene_family as sf
from .conftest import SCENES
from .test_gpu_batch_probes import _same

pytestmark = pytest.mark.gpu

W, H, RECT = 64, 48, (3, 5, 61, 44)   # the clip rect cuts 8x8 tiles on every side
CORNELL = os.path.join(SCENES, "cornell5.scene")
TRAIL_STEPS, TRAIL_PASSES, TRAIL_LANES, TRAIL_CHECK = 31, 32, 33, 12   # rmr_internal.h kCntTrail*
K = 3


def _dict_scene(layout):
    mats = [sf._diffuse(0, [0.8, 0.8, 0.8]), sf._diffuse(1, [0.8, 0.1, 0.1]), sf._diffuse(2, [0.1, 0.8, 0.1]),
            sf._diffuse(3, [0.2, 0.3, 0.8]), sf._diffuse(4, [0.8, 0.7, 0.2]), sf._diffuse(5, [0.6, 0.2, 0.7]), sf._emission(6)]
    objs = [sf._sphere(m, list(c), r) if kind == "s" else sf._box(m, list(c), list(r)) for kind, m, c, r in layout]
    return {"materials": mats, "objects": objs}


def _family_view():
    m = float(np.linalg.norm(sf.LOOK))
    return camera.view_uniforms(sf.EYE, tuple(x / m for x in sf.LOOK), float(W) / float(H), sf.PI32 / np.float32(4))


def _far_view():
    """Cornell-5 from ten times the default camera's distance through a narrow lens: |eye| sets the bound."""
    d = np.array([0.0, -4.0, 6.0])
    d = d / np.linalg.norm(d)
    return camera.view_uniforms((0.0, 40.0, -60.0), tuple(float(x) for x in d), float(W) / float(H), sf.PI32 / np.float32(32))


SPHERES = [("s", 0, (0.0, -101.0, 0.0), 100.0), ("s", 1, (-1.5, -0.4, 1.0), 0.6), ("s", 3, (0.75, -0.5, 0.5), 0.5),
           ("s", 2, (0.5, 0.2, 3.0), 1.2), ("s", 6, (0.0, 3.0, 1.0), 0.8)]
# name: scene, view, params, culling flags, whether passes must run (None: either)
CASES = {
    "cornell5": (CORNELL, lambda: camera.default_view(W, H), {}, abi.CULL_ALL, True),
    "spheres": (_dict_scene(SPHERES), _family_view, {}, abi.CULL_ALL, True),
    # (one primitive is another kernel class where the generator gives it no certifying map: no count is asked)
    "one_primitive": (_dict_scene([("s", 3, (0.0, 0.0, 2.0), 1.5)]), _family_view, {}, abi.CULL_ALL, None),
    "prims8": (_dict_scene(sf._room5() + sf._clutter(3, 8)), _family_view, {}, abi.CULL_ALL, True),
    "prims9": (_dict_scene(sf._room5() + sf._clutter(4, 9)), _family_view, {}, abi.CULL_ALL, True),
    "offset_1000": (sf.scene("offset_1000"), lambda: sf.view("offset_1000", W, H), {"max_dist": sf.max_dist("offset_1000")},
                    abi.CULL_ALL, True),
    "far_eye": (CORNELL, _far_view, {}, abi.CULL_ALL, True),
    "escape_off": (CORNELL, lambda: camera.default_view(W, H), {}, abi.CULL_ALL & ~abi.CULL_ESCAPE, False),
}


def _tables(scene):
    return scene_compile.load_scene_file(scene, "rm1") if isinstance(scene, str) else scene_compile.compile_scene(scene, "rm1")


def test_the_generated_scenes_sit_on_the_table_edge():
    assert len(CASES["prims8"][0]["objects"]) == 8 and len(CASES["prims9"][0]["objects"]) == 9
    assert len(CASES["one_primitive"][0]["objects"]) == 1
    assert all(o["nodes"][0]["name"] == "map_sphere" for o in CASES["spheres"][0]["objects"])


@pytest.fixture(scope="module")
def ctxs():
    """Three contexts of the diagnostic library (it reads RMR_JIT_TRAIL and RMR_JIT_OPTS at specialisation
    time): the steps compiled in, the same with the guard, and the source without the steps."""
    saved = {k: os.environ.get(k) for k in ("RMR_JIT_TRAIL", "RMR_JIT_OPTS")}
    rs = {}
    try:
        for tag in ("trail", "guard", "off"):
            r = Renderer(0, W, H, diag=True)
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


def _render(rs, tag, name, times):
    scene, view, kw, cull, _ = CASES[name]
    r = rs[tag]
    os.environ["RMR_JIT_TRAIL"] = "0" if tag == "off" else "1"
    if tag == "guard":
        os.environ["RMR_JIT_OPTS"] = "-DRMR_TRAIL_CHECK"
    else:
        os.environ.pop("RMR_JIT_OPTS", None)
    r.set_image_size(W, H)
    r.reload()
    r.load_scene(scene, "rm1")
    r.set_params(abi.default_params(max_bounces=4, **kw))
    r.set_view(view())
    r.set_culling(cull)
    r.set_tuning(lane_slots=True)
    r.set_trail_steps(K)
    r.reset_stats()
    gpu = r.trace_samples(times, RECT)
    st = r.stats()
    cnt = r.counters(34)
    assert st.jit_launches > 0 and st.jit_launches == st.trace_launches
    r.set_trail_steps(-1)
    r.set_culling(abi.CULL_ALL)
    return gpu, st, cnt


@pytest.mark.parametrize("name", list(CASES))
def test_bitexact_and_within_the_bound(ctxs, name):
    scene, view, kw, _, passes = CASES[name]
    times = time_schedule(2, frame=1)
    cpu = oracle.Oracle(_tables(scene), abi.default_params(max_bounces=4, **kw), view(), W, H).trace_samples(times, RECT)
    on, st, cnt = _render(ctxs, "trail", name, times)
    eq = _same(on[..., :3], cpu[..., :3])
    assert eq.all(), "%s vs oracle: %d samples differ" % (name, (~eq.all(axis=-1)).sum())
    off, st_off, cnt_off = _render(ctxs, "off", name, times)
    eq = _same(on, off)
    assert eq.all(), "%s vs the source without the steps: %d values differ" % (name, (~eq).sum())
    assert st.map_evals == st_off.map_evals, (name, st.map_evals, st_off.map_evals)
    assert cnt_off[TRAIL_STEPS] == 0 and cnt_off[TRAIL_PASSES] == 0
    gd, st_gd, cnt_gd = _render(ctxs, "guard", name, times)
    assert _same(gd, on).all() and st_gd.map_evals == st.map_evals, name
    print("%s: trailing steps %d of %d march evaluations, %d passes, %d lanes evaluated, guard %d"
          % (name, cnt[TRAIL_STEPS], cnt[0] - cnt[14], cnt[TRAIL_PASSES], cnt[TRAIL_LANES], cnt_gd[TRAIL_CHECK]))
    assert cnt_gd[TRAIL_CHECK] == 0, name
    assert cnt_gd[TRAIL_STEPS] == cnt[TRAIL_STEPS] and cnt_gd[TRAIL_LANES] == cnt[TRAIL_LANES]
    assert cnt[TRAIL_STEPS] <= cnt[TRAIL_LANES] <= 64 * cnt[TRAIL_PASSES] and cnt[TRAIL_PASSES] <= K * st.map_iters
    if passes:
        assert cnt[TRAIL_PASSES] > 0 and cnt[TRAIL_STEPS] > 0, name
    elif passes is not None:
        assert cnt[TRAIL_PASSES] == 0 and cnt[TRAIL_STEPS] == 0, name
