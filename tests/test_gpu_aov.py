"""The sampled AOVs on the GPU (rmr_render_aov; include/rmr.h): the five raw state planes bit
for bit against the host fold of the oracle's march / getNormal over the context's own camera rays, and against
the route that existed before (aov_fold(cast_rays(camera_rays))), on every table-driven map class and camera
model; that cutting a frame into calls, launches and rects is invisible; the resolved planes; the slot
overflow; that nothing else moved; the state rules and errors; and rmr_cli --sampled-aov.
"""
import subprocess

import numpy as np
import pytest

from oracle import camera, scene_compile
from raymarchrenderer_amd import (Renderer, RMRError, abi, aov_fold, aov_init, aov_resolve, default_camera_view,
                                  time_schedule)

from . import aov_ref as ref
from . import camera_ref
from .test_gpu_denoise import _read_pfm
from .test_gpu_guides import _far_hit_case
from .test_gpu_parity import _tables, same_bits
from .test_gpu_query import CAST_SCENES
from .test_gpu_rays import CLI, CORNELL, H, SCENE_CASES, VIEW, W, _context

pytestmark = pytest.mark.gpu

TIMES = time_schedule(4, frame=1)
N_PX = W * H
E = 2.0 ** -24
MODELS = {"view": {}, "thinlens": {"aperture": 0.15, "focus": 6.0}, "equirect": {}, "ortho": {"width": 6.0, "height": 5.0}}
CASES = [(name, "view") for name in CAST_SCENES] + [("cornell5", m) for m in ("thinlens", "equirect", "ortho")]
IDS = ["%s-%s" % c for c in CASES]


def _aov_context(name, model):
    r = _context(*SCENE_CASES[name])
    r.set_camera_model(model, **MODELS[model])
    return r


def _raw(r):
    """The five raw planes as the host functions' (5, n_px, 4) state."""
    return np.stack([r.read_aov_raw(p).reshape(-1, 4) for p in range(5)])


_want = {}


def _expected(name, model, rays):
    """The host fold of the oracle's first hits of the context's rays, once per case and read-only."""
    if (name, model) not in _want:
        path, variant, params = SCENE_CASES[name]
        hits = ref.oracle_hits(_tables(path, variant), abi.default_params(**params), rays).reshape(len(TIMES), N_PX)
        state = aov_fold(aov_init(N_PX), hits)
        state.setflags(write=False)
        _want[(name, model)] = (rays.copy(), state, hits)
    kept, state, hits = _want[(name, model)]
    assert kept.tobytes() == rays.tobytes()   # (the rays are a function of the case)
    return state, hits


# ---- 1. the raw planes, bit for bit ---------------------------------------------------------------------
@pytest.mark.parametrize("name,model", CASES, ids=IDS)
def test_raw_planes_against_the_oracle(name, model):
    r = _aov_context(name, model)
    try:
        rays = r.camera_rays(TIMES)
        r.render_aov(TIMES)
        got = _raw(r)
    finally:
        r.close()
    want, hits = _expected(name, model, rays)
    is_hit = hits["id"] >= 0
    print("%s %s: %d hits, %d misses, %d pixels with both" % (name, model, is_hit.sum(), (~is_hit).sum(),
                                                             (is_hit.any(axis=0) & ~is_hit.all(axis=0)).sum()))
    assert is_hit.sum() >= 200 and (~is_hit).sum() >= 50   # (the oracle alone decides this)
    for p in range(5):
        eq = same_bits(got[p], want[p]).all(axis=-1)
        assert eq.all(), "%s %s: plane %d differs at %d pixels, first %d gpu %s cpu %s" % (
            name, model, p, (~eq).sum(), np.argmin(eq), got[p][np.argmin(eq)], want[p][np.argmin(eq)])
    assert (got[0, :, 0] == len(TIMES)).all()


@pytest.mark.parametrize("name,model", CASES, ids=IDS)
def test_raw_planes_against_the_existing_route(name, model):
    """The fused kernel against cast_rays(camera_rays) folded on the host: GPU against GPU."""
    r = _aov_context(name, model)
    try:
        hits = r.cast_rays(r.camera_rays(TIMES)).reshape(len(TIMES), N_PX)
        r.render_aov(TIMES)
        got = _raw(r)
    finally:
        r.close()
    assert (hits["id"] >= -1).all()   # no ray was rejected
    assert same_bits(got, aov_fold(aov_init(N_PX), hits)).all()


# ---- 2. cutting is invisible ----------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["thinlens", "equirect"])
def test_cutting_is_invisible(model):
    r = _aov_context("cornell5", model)
    try:
        r.render_aov(TIMES)
        one = _raw(r)
        r.aov_reset()
        assert same_bits(_raw(r), aov_init(N_PX)).all()
        for k in range(len(TIMES)):
            r.render_aov(TIMES[k:k + 1])
        assert same_bits(_raw(r), one).all(), "four calls of one sample"
        for n in (1, 3):
            r.set_aov_launch_samples(n)
            r.render_aov(TIMES, restart=True)
            assert same_bits(_raw(r), one).all(), "launches of %d samples" % n
        r.set_aov_launch_samples(8)
        r.aov_reset()
        r.render_aov(TIMES, rect=(0, 0, 13, H))
        left = _raw(r).reshape(5, H, W, 4)
        assert same_bits(left[:, :, :13], one.reshape(5, H, W, 4)[:, :, :13]).all()
        assert same_bits(left[:, :, 13:], aov_init(N_PX).reshape(5, H, W, 4)[:, :, 13:]).all()   # untouched
        r.render_aov(TIMES, rect=(13, 0, W, H))
        assert same_bits(_raw(r), one).all(), "two rects split at x = 13"
        # a rect beyond the image is clamped; restart on a sub-rect re-initialises that rect only
        sub = (5, 3, 29, 22)
        r.render_aov(TIMES[:2], rect=(sub[0], sub[1], sub[2], sub[3]), restart=True)
        got = _raw(r).reshape(5, H, W, 4)
        r.render_aov(TIMES[:2], rect=(-4, -4, W + 9, H + 9), restart=True)
        two = _raw(r).reshape(5, H, W, 4)
        inside = np.zeros((H, W), bool)
        inside[sub[1]:sub[3], sub[0]:sub[2]] = True
        assert same_bits(got[:, inside], two[:, inside]).all()
        assert same_bits(got[:, ~inside], one.reshape(5, H, W, 4)[:, ~inside]).all()
        assert (two[0, :, :, 0] == 2).all() and (got[0, ~inside, 0] == 4).all()
        # a bare restart: the rect back to the initial state, nothing folded
        r.render_aov(None, rect=sub, restart=True)
        bare = _raw(r).reshape(5, H, W, 4)
        assert same_bits(bare[:, inside], aov_init(N_PX).reshape(5, H, W, 4)[:, inside]).all()
        assert same_bits(bare[:, ~inside], two[:, ~inside]).all()
    finally:
        r.close()


# ---- 3. the resolved planes -----------------------------------------------------------------------------
def test_resolved_planes_and_device_tensors():
    import torch
    r = _aov_context("cornell5", "view")
    try:
        r.render_aov(TIMES)
        raw = _raw(r)
        got = np.stack([r.read_aov_resolved(p).reshape(-1, 4) for p in range(5)])
        dev = r.aov_device()
        r.sync()
        for name, which in abi.AOV_RESOLVED.items():
            t = dev[name]
            assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (H, W, 4)
            assert t.data_ptr() == r.lib.rmr_aov_resolved_device_ptr(r.ctx, which)   # no copy
            assert same_bits(t.cpu().numpy().reshape(-1, 4), got[which]).all(), name
        a = r.read_aov()
    finally:
        r.close()
    md = abi.default_params().max_dist
    host, w = aov_resolve(raw, md), ref.resolve64(raw, md)
    print("resolved planes equal to the host function bit for bit: %s" % same_bits(got, host).all())
    worst_q = 0.0
    for p, k in [(0, 0), (0, 2), (2, 0), (2, 1), (2, 2), (3, 1), (3, 3), (4, 1), (4, 3)]:
        want = w[p, :, k].astype(np.float32)
        worst_q = max(worst_q, float((np.abs(got[p, :, k].astype(np.float64) - want) /
                                      np.spacing(np.abs(want)).astype(np.float64)).max()))
    worst_n = float(np.abs(got[1, :, :3] - w[1, :, :3]).max())
    print("worst quotient distance %.3g ulp, worst normal component error %.2f x 2^-24" % (worst_q, worst_n / E))
    assert worst_q <= 1.0 and worst_n <= 4 * E
    for p, k in [(0, 1), (0, 3), (2, 3), (3, 0), (3, 2), (4, 0), (4, 2)]:
        assert (got[p, :, k] == w[p, :, k]).all(), (p, k)
    # the dictionary form
    assert set(a) == {"alpha", "depth", "min_depth", "normal", "position", "samples", "hits", "ids", "coverage", "other"}
    assert a["ids"].shape == (H, W, 4) and a["coverage"].shape == (H, W, 4) and a["normal"].shape == (H, W, 3)
    assert same_bits(a["alpha"].reshape(-1), got[0, :, 2]).all() and same_bits(a["depth"].reshape(-1), got[0, :, 0]).all()
    assert same_bits(a["ids"].reshape(-1, 4)[:, 2], got[4, :, 0]).all()
    assert same_bits(a["coverage"].reshape(-1, 4)[:, 1], got[3, :, 3]).all()
    assert same_bits(a["other"].reshape(-1), raw[1, :, 3]).all() and (a["samples"] == 4).all()
    assert ((a["alpha"] > 0) & (a["alpha"] < 1)).any() and (a["alpha"] == 1).any() and (a["alpha"] == 0).any()


# ---- 4. slot overflow -----------------------------------------------------------------------------------
def test_slot_overflow():
    """Eight materials around the eye at 4 x 2 under equirect, 16 samples: pixels that see more than four."""
    w, h, times = 4, 2, time_schedule(16)
    scene = ref.overflow_scene()
    tables = scene_compile.compile_scene(scene, "rm1")
    prm = abi.default_params()
    view = camera.view_uniforms((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), float(w) / h, np.float32(3.141592653) / np.float32(4))
    # on the oracle's side first, from the float64 statement of the generator: the case is not vacuous
    o, d, _ = camera_ref.rays(camera_ref.EQUIRECT, view, w, h, times, (0, 0, w, h))
    rays = np.zeros(o.shape[:3], np.dtype(abi.RAY_DTYPE))
    rays["o"], rays["d"] = o, d
    est = aov_fold(aov_init(w * h), ref.oracle_hits(tables, prm, rays).reshape(len(times), w * h))
    assert (est[1, :, 3] > 0).any() and ((est[1, :, 3] == 0) & (est[3, :, 2] >= 0)).any()
    r = Renderer(0, w, h)
    try:
        r.load_scene(scene, "rm1")
        r.set_params(prm)
        r.set_view(view)
        r.set_camera_model("equirect")
        grays = r.camera_rays(times)
        r.render_aov(times)
        got = _raw(r)
        res = r.read_aov()
    finally:
        r.close()
    want = aov_fold(aov_init(w * h), ref.oracle_hits(tables, prm, grays).reshape(len(times), w * h))
    assert (want[1, :, 3] > 0).any() and ((want[1, :, 3] == 0) & (want[3, :, 2] >= 0)).any()
    assert same_bits(got, want).all()
    over = want[1, :, 3] > 0
    assert (want[4, over, 2] >= 0).all()   # every slot is used where a hit found none
    cov = res["coverage"].reshape(-1, 4).astype(np.float64).sum(axis=1) + want[1, :, 3] / 16.0
    assert np.abs(cov - res["alpha"].reshape(-1)).max() <= 8 * E   # the slots and `other` account for every hit


# ---- 5. nothing else moved ------------------------------------------------------------------------------
def test_render_aov_leaves_the_images_alone():
    rect = (3, 2, 41, 35)
    r = _context(*SCENE_CASES["cornell5"])
    fresh = _context(*SCENE_CASES["cornell5"])
    try:
        r.set_error_estimate(True)
        r.render_spp(TIMES, rect)
        r.render_guides()
        dn = r.denoise(iterations=2)
        state = (r.read_accum(), r.read_half(), r.tile_error(), r.read_guides())

        def unchanged(what):
            assert same_bits(r.read_accum(), state[0]).all() and same_bits(r.read_half(), state[1]).all(), what
            assert same_bits(r.tile_error(), state[2]).all(), what
            assert same_bits(r.read_denoised(), dn).all(), what   # still valid: the call raises otherwise
            for k, g in r.read_guides().items():
                assert same_bits(g, state[3][k]).all(), (what, k)

        r.render_aov(TIMES)
        unchanged("render_aov")
        r.read_aov()
        unchanged("read_aov")
        r.aov_reset()
        r.render_aov(TIMES[:2], rect=rect, restart=True)
        unchanged("aov_reset, restart")
        # the next launch finds a clean work queue: the same bits as a context that never called the stage
        r.render_spp(TIMES[:1], rect, first_sample=4)
        got = r.read_accum()
        fresh.set_error_estimate(True)
        fresh.render_spp(TIMES, rect)
        fresh.render_spp(TIMES[:1], rect, first_sample=4)
        assert same_bits(got, fresh.read_accum()).all() and not same_bits(got, state[0]).all()
    finally:
        r.close()
        fresh.close()


def test_far_hits_count_as_misses():
    """step_multiply 1.7 overshoots into objects beyond a reduced max_dist: march returns those as hits at
    t >= max_dist; the fold counts them as misses."""
    path, variant, params = SCENE_CASES["cornell5"]
    tables = _tables(path, variant)
    view, prm = _far_hit_case(tables)
    r = _context(path, variant, params)
    try:
        r.set_params(prm)
        r.set_view(view)
        rays = r.camera_rays(TIMES)
        r.render_aov(TIMES)
        got = _raw(r)
        depth = r.read_aov_resolved("depth").reshape(-1, 4)
    finally:
        r.close()
    hits = ref.oracle_hits(tables, prm, rays).reshape(len(TIMES), N_PX)
    far = (hits["id"] < 0) & (hits["t"] >= prm.max_dist) & (hits["t"] != prm.max_dist)
    far_only = far.any(axis=0) & ~(hits["id"] >= 0).any(axis=0)
    print("far hits %d, pixels with far hits and no hit %d" % (far.sum(), far_only.sum()))
    assert far.sum() >= 3 and far_only.sum() >= 1
    assert same_bits(got, aov_fold(aov_init(N_PX), hits)).all()
    assert (got[0, far_only, 1] == 0).all() and (depth[far_only, 2] == 0).all()
    assert (depth[far_only, 0] == prm.max_dist).all() and (depth[far_only, 1] == prm.max_dist).all()


# ---- 6. state and errors --------------------------------------------------------------------------------
def test_state_and_errors():
    r = Renderer(0, W, H)
    try:
        def code(call):
            with pytest.raises(RMRError) as e:
                call()
            return e.value.code

        assert code(lambda: r.render_aov(TIMES)) == -5            # no scene
        assert code(lambda: r.read_aov_raw(0)) == -5
        r.load_scene(CORNELL, "rm1")
        r.set_view(VIEW)
        assert code(lambda: r.read_aov_raw(0)) == -5              # nothing rendered yet
        assert code(lambda: r.read_aov_resolved(0)) == -5
        assert code(r.aov_device) == -5
        r.aov_reset()                                             # nothing to do, nothing allocated
        assert code(lambda: r.read_aov_raw(0)) == -5
        r.render_aov(TIMES)
        before = _raw(r)
        for bad in (-1, 5):
            assert code(lambda: r.read_aov_raw(bad)) == -1
            assert code(lambda: r.read_aov_resolved(bad)) == -1
            assert not r.lib.rmr_aov_device_ptr(r.ctx, bad) and not r.lib.rmr_aov_resolved_device_ptr(r.ctx, bad)
        buf = np.zeros((H, W, 4), np.float32)
        fp = buf.ctypes.data_as(r.lib.rmr_read_aov.argtypes[2])
        for nbytes in (buf.nbytes - 16, buf.nbytes + 16, 0):
            assert r.lib.rmr_read_aov(r.ctx, 0, fp, nbytes) == -1
            assert r.lib.rmr_read_aov_resolved(r.ctx, 0, fp, nbytes) == -1
        assert r.lib.rmr_read_aov(r.ctx, 0, fp, buf.nbytes) == 0 and same_bits(buf.reshape(-1, 4), before[0]).all()
        # nspp and times must agree
        assert r.lib.rmr_render_aov(r.ctx, TIMES.ctypes.data_as(r.lib.rmr_render_aov.argtypes[1]), 0, 0, 0, W, H, 0) == -1
        assert r.lib.rmr_render_aov(r.ctx, None, 2, 0, 0, W, H, 0) == -1
        assert code(lambda: r.set_aov_launch_samples(0)) == -1
        # the 2^24 limit is checked before anything is queued
        many = np.zeros(2 ** 24 - 3, np.float32)
        assert code(lambda: r.render_aov(many)) == -1
        assert same_bits(_raw(r), before).all()
        # set_view, set_params and a camera-model change keep the planes
        r.set_view(VIEW)
        r.set_params(abi.default_params(max_bounces=2))
        r.set_camera_model("equirect")
        assert same_bits(_raw(r), before).all()
        r.set_camera_model("view")
        # reload, a scene load and set_image_size free them
        r.reload()
        assert code(lambda: r.read_aov_raw(0)) == -5
        r.render_aov(TIMES)
        assert same_bits(_raw(r), before).all()
        r.load_scene(CORNELL, "rm1")
        assert code(lambda: r.read_aov_raw(0)) == -5 and code(lambda: r.read_aov_resolved(0)) == -5
        r.render_aov(TIMES)
        assert same_bits(_raw(r), before).all()
        r.set_image_size(W, H)
        assert code(lambda: r.read_aov_raw(0)) == -5
        r.reload()
        r.render_aov(TIMES[:1])
        assert (_raw(r)[0, :, 0] == 1).all()
    finally:
        r.close()


# ---- 7. rmr_cli -----------------------------------------------------------------------------------------
def test_cli_sampled_aov(tmp_path):
    """rmr_cli --sampled-aov P at 44x36 and 4 samples under --camera equirect writes the five PFMs; they equal
    the Python route's arrays."""
    out, prefix = str(tmp_path / "cli.bmp"), str(tmp_path / "saov")
    p = subprocess.run([CLI, "--scene", CORNELL, "--variant", "rm1", "--size", "%dx%d" % (W, H), "--samples", "4",
                        "--bounces", "3", "--camera", "equirect", "--sampled-aov", prefix, "--out", out, "--quiet"],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    r = Renderer(0, W, H)
    try:
        r.load_scene(CORNELL, "rm1")
        r.set_params(abi.default_params(max_bounces=3))
        r.set_view(default_camera_view(W, H))   # the driver's camera (Camera.cpp through rmr_camera_view)
        r.set_camera_model("equirect")
        r.render_aov(time_schedule(4))
        a = r.read_aov()
    finally:
        r.close()
    alpha, depth, ids = (_read_pfm(prefix + s) for s in ("_alpha.pfm", "_depth.pfm", "_ids.pfm"))
    assert same_bits(alpha[..., 0], a["alpha"]).all() and same_bits(alpha[..., 1], a["samples"]).all()
    assert same_bits(alpha[..., 2], a["hits"]).all()
    assert same_bits(depth[..., 0], a["depth"]).all() and same_bits(depth[..., 1], a["min_depth"]).all()
    assert (depth[..., 2] == 0).all()
    assert same_bits(_read_pfm(prefix + "_normal.pfm"), a["normal"]).all()
    assert same_bits(_read_pfm(prefix + "_position.pfm"), a["position"]).all()
    assert same_bits(ids[..., 0], a["ids"][..., 0]).all() and same_bits(ids[..., 1], a["coverage"][..., 0]).all()
    assert same_bits(ids[..., 2], a["ids"][..., 1]).all()
    assert ((a["alpha"] > 0) & (a["alpha"] < 1)).any()
