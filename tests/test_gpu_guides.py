"""First-hit guide planes (rmr_render_guides) against the CPU oracle's march / getNormal, bit for bit.

The pass takes the pixel-centre ray of main() (no rand()), so its direction is checked against the
float64 evaluation of the formula, and everything after it against the oracle fed with the GPU's own
direction: (t, id) bitwise oracle.march with the far-hit rule (a hit at t >= max_dist is a miss), the
position within 1 ulp of eye + dir t, the normal bitwise oracle.normal at the GPU's position."""
import os

import numpy as np
import pytest

from oracle import camera
from raymarchrenderer_amd import Renderer, abi, time_schedule

from .conftest import GOLDEN, SCENES
from .denoise_ref import far_hit_rule, oracle_march, oracle_normals, pixel_centre_dirs
from .test_gpu_parity import _setup, _tables, same_bits

pytestmark = pytest.mark.gpu

W, H = 44, 36                      # ragged: not a multiple of the 8x8 tile
RECT = (3, 2, 41, 35)
CORNELL = os.path.join(SCENES, "cornell5.scene")
DEFAULT = os.path.join(GOLDEN, "scenes", "default.scene")

CASES = [
    ("rm1_cornell5", CORNELL, "rm1"),
    ("rm1_default", DEFAULT, "rm1"),
    ("rm1_csg_nodes", os.path.join(SCENES, "csg_nodes.scene"), "rm1"),
    ("rm1_csg64", os.path.join(SCENES, "csg64.scene"), "rm1"),
    ("rm1_mandelbulb", os.path.join(SCENES, "mandelbulb.scene"), "rm1"),
    ("rm2_simple", os.path.join(GOLDEN, "scenes", "simple.scene"), "rm2"),
    ("rm3_builtin", None, "rm3"),
]


def _inside(rect):
    x0, y0, x1, y1 = rect
    return (slice(y0, y1), slice(x0, x1))


def _check_planes(g, tables, prm, view, rect, name):
    """The three planes inside `rect` against the formula and the oracle. Returns the oracle's raw
    (t, id) there, for the callers that assert what the case contains."""
    sl = _inside(rect)
    ray, hit, nrm = g["ray"][sl], g["hit"][sl], g["normal"][sl]
    eye = np.asarray(view, np.float32).reshape(5, 3)[0]
    # RAY: about eight float32 roundings on values of magnitude <= 2, with roughly 4x margin
    want = pixel_centre_dirs(view, W, H)[sl]
    assert np.abs(ray[..., :3].astype(np.float64) - want).max() <= 2e-6, name
    assert (ray[..., 3] == 0).all()
    # (t, id): the oracle's march from the GPU's direction
    dirs = np.ascontiguousarray(ray[..., :3])
    t, ident = oracle_march(tables, prm, eye, dirs)
    want_id = far_hit_rule(t, ident, prm.max_dist)
    assert same_bits(hit[..., 3], t).all(), "%s: t differs at %s" % (name, np.argwhere(~same_bits(hit[..., 3], t))[:3])
    assert same_bits(nrm[..., 3], want_id).all(), "%s: id differs" % name
    # pos = fma(dir, t, eye): one rounding of the exact value, so within 1 ulp of the float64 evaluation
    p64 = eye.astype(np.float64) + dirs.astype(np.float64) * t[..., None].astype(np.float64)
    ulp = np.spacing(np.abs(p64.astype(np.float32))).astype(np.float64)
    assert (np.abs(hit[..., :3].astype(np.float64) - p64) <= ulp).all(), name
    # normal: getNormal at the GPU's position on hits, zero on misses
    is_hit = want_id >= 0
    want_n = oracle_normals(tables, prm.max_dist, np.ascontiguousarray(hit[..., :3]), is_hit)
    eq = same_bits(nrm[..., :3], want_n).all(axis=-1)
    assert eq.all(), "%s: %d normals differ, first %s gpu %s cpu %s" % (
        name, (~eq).sum(), np.argwhere(~eq)[0], nrm[tuple(np.argwhere(~eq)[0])], want_n[tuple(np.argwhere(~eq)[0])])
    assert (nrm[~is_hit] == np.array([0, 0, 0, -1], np.float32)).all()
    return t, ident


@pytest.mark.parametrize("name,path,variant", CASES, ids=[c[0] for c in CASES])
def test_guides_bitexact(renderer, name, path, variant):
    prm, view = _setup(renderer, path, variant, W, H, {})
    renderer.render_guides(RECT)
    g = renderer.read_guides()
    t, ident = _check_planes(g, _tables(path, variant), prm, view, RECT, name)
    assert (far_hit_rule(t, ident, prm.max_dist) >= 0).any(), "%s: no hit in the rect" % name
    # nothing outside the rect was written (the planes start as zeros after a reload)
    outside = np.ones((H, W), bool)
    outside[_inside(RECT)] = False
    for plane in g.values():
        assert (plane[outside] == 0).all()


@pytest.mark.parametrize("path", [CORNELL, DEFAULT], ids=["cornell5", "default"])
def test_guides_zero_steps_all_miss(renderer, path):
    prm, view = _setup(renderer, path, "rm1", W, H, {"max_steps": 0})
    renderer.render_guides(RECT)
    g = renderer.read_guides()
    t, ident = _check_planes(g, _tables(path, "rm1"), prm, view, RECT, "steps0")
    assert (t == prm.max_dist).all() and (ident == -1).all()
    assert (g["normal"][_inside(RECT)] == np.array([0, 0, 0, -1], np.float32)).all()


def _far_hit_case(tables):
    """An eye and a max_dist for which march with step_multiply 1.7 gives far hits (an id at
    t >= max_dist), hits and misses among the rect's pixel-centre rays; found on the CPU."""
    for eye_z in (-6.0, -4.5, -8.0):
        view = camera.default_view(W, H).copy()
        view[:3] = (0.0, 4.0, eye_z)
        dirs = pixel_centre_dirs(view, W, H).astype(np.float32)[_inside(RECT)]
        far = abi.default_params(step_multiply=1.7)
        t0, id0 = oracle_march(tables, far, view[:3], dirs)
        hits = np.sort(t0[(id0 >= 0) & (t0 < far.max_dist)])
        if len(hits) < 8:
            continue
        for q in (0.5, 0.35, 0.65, 0.2, 0.8):
            md = float(np.float32(hits[int(q * (len(hits) - 1))]))
            prm = abi.default_params(step_multiply=1.7, max_dist=md)
            t, ident = oracle_march(tables, prm, view[:3], dirs)
            n_far = ((ident >= 0) & (t >= prm.max_dist)).sum()
            n_hit = ((ident >= 0) & (t < prm.max_dist)).sum()
            n_miss = (ident < 0).sum()
            if min(n_far, n_hit, n_miss) >= 3:
                return view, prm
    raise AssertionError("no eye / max_dist with far hits, hits and misses found")


@pytest.mark.parametrize("path", [CORNELL, DEFAULT], ids=["cornell5", "default"])
def test_guides_far_hits(renderer, path):
    """step_multiply 1.7 overshoots into objects beyond a reduced max_dist: march returns those as
    hits at t >= max_dist, the guides show them as misses with march's t."""
    tables = _tables(path, "rm1")
    view, prm = _far_hit_case(tables)
    _setup(renderer, path, "rm1", W, H, {})
    renderer.set_params(prm)
    renderer.set_view(view)
    renderer.render_guides(RECT)
    g = renderer.read_guides()
    t, ident = _check_planes(g, tables, prm, view, RECT, "far")
    n_far = ((ident >= 0) & (t >= prm.max_dist)).sum()
    n_hit = ((ident >= 0) & (t < prm.max_dist)).sum()
    n_miss = (ident < 0).sum()
    print("far hits %d, hits %d, misses %d at max_dist %g" % (n_far, n_hit, n_miss, prm.max_dist))
    assert n_far >= 1 and n_hit >= 1 and n_miss >= 1
    far = (ident >= 0) & (t >= prm.max_dist)
    assert (g["normal"][_inside(RECT)][far] == np.array([0, 0, 0, -1], np.float32)).all()
    assert (g["hit"][_inside(RECT)][far][:, 3] >= prm.max_dist).all()


def test_sub_rect_rewrites_only_its_rect(renderer):
    prm, view = _setup(renderer, CORNELL, "rm1", W, H, {})
    renderer.render_guides()
    before = renderer.read_guides()
    view2 = view.copy()
    view2[:3] += np.array([0.4, -0.3, 0.5], np.float32)
    renderer.set_view(view2)
    sub = (9, 6, 30, 21)
    renderer.render_guides(sub)
    after = renderer.read_guides()
    renderer.render_guides()
    full2 = renderer.read_guides()
    inside = np.zeros((H, W), bool)
    inside[_inside(sub)] = True
    for k in before:
        assert same_bits(after[k][~inside], before[k][~inside]).all(), k
        assert same_bits(after[k][inside], full2[k][inside]).all(), k
    # the eye moved: the directions stay, the hits do not
    assert same_bits(full2["ray"], before["ray"]).all()
    assert not same_bits(full2["hit"][inside], before["hit"][inside]).all()


@pytest.mark.parametrize("streams0", [False, True], ids=["default_ctx", "launch_streams_0"])
def test_guides_and_denoise_leave_rendering_unchanged(streams0):
    """2 spp through rmr_render (call batching on by default), then guides + denoise + reads, then 2
    more: bitwise one 4-spp render."""
    w, h = 40, 24
    times = time_schedule(4, frame=2)
    r = Renderer(0, w, h)
    try:
        if streams0:
            r.set_launch_streams(0)
        r.load_scene(CORNELL, "rm1")
        r.set_params(abi.default_params(max_bounces=3))
        r.set_view(camera.default_view(w, h))
        for s in range(2):
            r.render(float(times[s]), (0, 0), (w, h), s)
        r.render_guides((5, 3, 20, 11))
        r.render_guides()
        g = r.read_guides()
        d = r.denoise(iterations=3)
        assert r.guide_device_ptr("hit") and r.denoised_device_ptr()
        mid = r.read_accum()
        for s in range(2, 4):
            r.render(float(times[s]), (0, 0), (w, h), s)
        got = r.read_accum()
        r.reload()
        r.render_spp(times)
        want = r.read_accum()
    finally:
        r.close()
    assert same_bits(got, want).all()
    assert (g["normal"][..., 3] >= 0).any() and d.shape == mid.shape
    assert same_bits(d[..., 3], mid[..., 3]).all()   # alpha unchanged
    assert not same_bits(d[..., :3], mid[..., :3]).all()   # and something was filtered
