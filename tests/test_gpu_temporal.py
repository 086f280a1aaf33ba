"""The temporal reprojection stage (rmr_temporal_accumulate) on the GPU: the kernel on
synthetic two-view images through the test hook against the float64 statement tests/temporal_ref.py, the
bit-exact pass-through rules, the real pipeline through both doors, and the state rules.

Bounds, over every pixel (none is excluded):
  projected coordinates: |gpu - ref| <= (bx, by), rmr.h's counted bound (temporal_ref.coordinate_bound);
  image: |gpu - ref| <= (bx + by) spread + 1e-5 (|ref| + M): the coordinate bound times the spread of the
    colours the pixel mixes (the taps that are on the image with Hn > 0, and S(p), which takes the weight a
    tap loses), plus the weights' own rounding; M the largest finite |rgb| over the live pixels of S
    (tests/denoise_ref.py tolerance_scale, the denoiser tests' scale);
  count: |gpu - ref| <= (bx + by) max Hn over those taps + 1e-5 (ref + max_history).
A pixel that is not live: the image bit for bit S, count 0, coordinates NaN.

Measured share of the bounds (MI355X), the largest over every case of test_hook_matches_reference:
coordinates 0.103 (8.7e-6 px), image 0.067, count 0.044."""
import os

import numpy as np
import pytest

from raymarchrenderer_amd import Renderer, RMRError, abi, encode_bmp, temporal_view_inverse, time_schedule

from .conftest import SCENES
from .denoise_ref import tolerance_scale
from .temporal_ref import coordinate_bound, synthetic_case, temporal_ref, twisted
from .test_gpu_parity import same_bits
from .test_temporal_cpu import view_pair

pytestmark = pytest.mark.gpu

CORNELL = os.path.join(SCENES, "cornell5.scene")
CSG64 = os.path.join(SCENES, "csg64.scene")
SIZES = [(44, 36), (33, 9), (1, 1)]
PARAMS = [dict(), dict(max_history=8.0, sigma_z=0.5, normal_pow2=0)]


@pytest.fixture(scope="module")
def hook():
    r = Renderer(0, 8, 8)
    yield r
    r.close()


@pytest.fixture(scope="module")
def cases():
    """The synthetic inputs per (W, H, twist), made once."""
    out = {}
    for W, H in SIZES:
        view, h_view = view_pair(W, H)
        for tw in (False, True):
            out[W, H, tw] = synthetic_case(W, H, view, twisted(h_view) if tw else h_view)
    return out


def _run_hook(r, c, samples, **kw):
    return r.temporal_images(c["S"], c["hit"], c["nrm"], c["view"], c["h_rgba"], c["h_n"], c["h_hit"], c["h_nrm"],
                             c["h_view"], samples, **kw)


def _ref(c, samples, **kw):
    return temporal_ref(c["S"], c["hit"], c["nrm"], c["h_rgba"], c["h_n"], c["h_hit"], c["h_nrm"], c["h_view"], samples, **kw)


# ---- case 1: the hook against the reference ---------------------------------------------------------
@pytest.mark.parametrize("twist", [False, True], ids=["camera_view", "twisted"])
@pytest.mark.parametrize("W,H", SIZES, ids=lambda v: str(v))
def test_hook_matches_reference(hook, cases, W, H, twist):
    c = cases[W, H, twist]
    Mi, k = temporal_view_inverse(c["h_view"])
    bx, by = coordinate_bound(c["hit"][..., :3].astype(np.float64), c["h_view"], Mi, k, W, H)
    M = tolerance_scale(c["S"], c["nrm"])
    worst = np.zeros(3)
    for kw in PARAMS:
        n_cur = 4.0
        ref = _ref(c, n_cur, **kw)
        img, cnt, xy = _run_hook(hook, c, n_cur, **kw)
        live, proj = ref["live"], ref["projected"]
        what = "%dx%d twist %d %s" % (W, H, twist, kw)
        # the same pixels have a projection, and it is within the counted bound
        assert (np.isnan(xy).any(-1) == ~proj).all(), what
        assert np.isfinite(bx[proj]).all() and np.isfinite(by[proj]).all(), what
        ex = np.abs(xy[..., 0].astype(np.float64) - ref["xy"][..., 0])
        ey = np.abs(xy[..., 1].astype(np.float64) - ref["xy"][..., 1])
        if proj.any():
            share = max(float((ex[proj] / bx[proj]).max()), float((ey[proj] / by[proj]).max()))
            print("%s: coordinates: largest error %.3g px, largest share of the bound %.3g"
                  % (what, max(ex[proj].max(), ey[proj].max()), share))
            worst[0] = max(worst[0], share)
            assert (ex[proj] <= bx[proj]).all() and (ey[proj] <= by[proj]).all(), (what, share)
        cb = np.where(proj, bx + by, 0.0)
        # image and count
        assert np.isfinite(img[live][:, :3]).all(), what
        with np.errstate(invalid="ignore"):
            err = np.abs(img[..., :3].astype(np.float64) - ref["out"][..., :3])
            bound = (cb * ref["spread"])[..., None] + 1e-5 * (np.abs(ref["out"][..., :3]) + M)
            nerr = np.abs(cnt.astype(np.float64) - ref["n"])
            nbound = cb * ref["spread_n"] + 1e-5 * (ref["n"] + float(np.float32(kw.get("max_history", 64.0))))
        if live.any():
            s_img, s_n = float((err[live] / bound[live]).max()), float((nerr[live] / nbound[live]).max())
            print("%s: largest share of the bound: image %.3g, count %.3g; history used at %d of %d live pixels"
                  % (what, s_img, s_n, ref["used"].sum(), live.sum()))
            worst[1:] = np.maximum(worst[1:], (s_img, s_n))
            assert (err[live] <= bound[live]).all(), (what, s_img)
            assert (nerr[live] <= nbound[live]).all(), (what, s_n)
        # pass-through, bit for bit
        assert same_bits(img[~live], c["S"][~live]).all() and (cnt[~live] == 0).all(), what
        assert same_bits(img[..., 3], c["S"][..., 3]).all(), what
        none = live & ~ref["used"]
        assert same_bits(img[none], c["S"][none]).all(), what
        assert (cnt[none] == np.float32(min(n_cur, kw.get("max_history", 64.0)))).all(), what
        if (W, H) == (44, 36):
            assert ref["used"].sum() > 0.5 * live.sum() and none.sum() >= 8 and (~live).sum() >= 5
            assert not same_bits(img[ref["used"]], c["S"][ref["used"]]).all()
        if (W, H) == (1, 1):
            assert ref["used"].all() and not same_bits(img[..., :3], c["S"][..., :3]).all()
    print("%dx%d twist %d: worst shares: coordinates %.3g, image %.3g, count %.3g" % ((W, H, twist) + tuple(worst)))


# ---- case 2: pass-through --------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", SIZES, ids=lambda v: str(v))
def test_empty_history_returns_the_source(hook, cases, W, H):
    c = dict(cases[W, H, False])
    c["h_n"] = np.zeros((H, W), np.float32)
    live = temporal_ref(c["S"], c["hit"], c["nrm"], c["h_rgba"], c["h_n"], c["h_hit"], c["h_nrm"], c["h_view"], 3.0)["live"]
    for samples, kw, want in ((3.0, {}, 3.0), (100.0, {}, 64.0), (0.25, {"max_history": 2.0}, 0.25)):
        img, cnt, xy = _run_hook(hook, c, samples, **kw)
        assert same_bits(img, c["S"]).all()
        assert (cnt[live] == np.float32(want)).all() and (cnt[~live] == 0).all()
    # a history of NaN colours with counts: the mean is not finite, so the source passes through
    c = dict(cases[W, H, False])
    c["h_rgba"] = np.full((H, W, 4), np.nan, np.float32)
    img, cnt, _ = _run_hook(hook, c, 3.0)
    assert same_bits(img, c["S"]).all() and (cnt[live] == 3.0).all() and (cnt[~live] == 0).all()


def test_hook_argument_errors(hook, cases):
    c = cases[44, 36, False]
    for bad in ({"max_history": 0.5}, {"max_history": float("nan")}, {"sigma_z": 0.0}, {"normal_pow2": 8}, {"normal_pow2": -1}):
        with pytest.raises(RMRError) as e:
            _run_hook(hook, c, 4.0, **bad)
        assert e.value.code == -1, bad
    for samples in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(RMRError) as e:
            _run_hook(hook, c, samples)
        assert e.value.code == -1, samples
    flat = dict(c)
    hv = c["h_view"].copy().reshape(5, 3)
    hv[1:, 2] = 0.0
    flat["h_view"] = hv.reshape(15)
    with pytest.raises(RMRError) as e:
        _run_hook(hook, flat, 4.0)
    assert e.value.code == -1
    with pytest.raises(TypeError):
        _run_hook(hook, c, 4.0, sigma_c=1.0)


# ---- case 3: the real pipeline, through both doors -------------------------------------------------
W0, H0 = 44, 36


def _context(path, jit=None):
    r = Renderer(0, W0, H0)
    if jit is not None:
        r.set_jit(jit)
    r.load_scene(path, "rm1")
    r.set_params(abi.default_params(max_bounces=4))
    return r


def _move_and_render(r, view, first_seed):
    """A camera move the reference's way: the new view, then samples from running-mean index 0, which
    overwrite the accumulator (rmr_reload would drop the history with everything else)."""
    r.set_view(view)
    r.render_spp(time_schedule(4, first_sample=first_seed), first_sample=0)


@pytest.mark.parametrize("jit", [0, 1], ids=["aot", "hiprtc"])
@pytest.mark.parametrize("path", [CORNELL, CSG64], ids=["cornell5", "csg64"])
def test_pipeline_is_the_hook(path, jit):
    B, A = view_pair(W0, H0)
    zero4, zero1 = np.zeros((H0, W0, 4), np.float32), np.zeros((H0, W0), np.float32)
    r, plain = _context(path, jit), _context(path, jit)
    try:
        ptrs = [r.guide_device_ptr(p) for p in ("ray", "hit", "normal")]
        # 1. view A, 4 spp: no history yet, the source comes back with count 4
        _move_and_render(r, A, 0)
        t1 = r.temporal_accumulate("accum", 4)
        n1 = r.read_temporal_count()
        acc1, g1 = r.read_accum(), r.read_guides()
        live1 = (g1["normal"][..., 3] >= 0) & (acc1[..., 3] != 0) & np.isfinite(acc1[..., :3]).all(-1)
        assert same_bits(t1, acc1).all() and (n1[live1] == 4.0).all() and (n1[~live1] == 0).all() and live1.any()
        h1 = r.temporal_images(acc1, g1["hit"], g1["normal"], A, zero4, zero1, zero4, zero4, A, 4)
        assert same_bits(t1, h1[0]).all() and same_bits(n1, h1[1]).all()
        p1 = r.temporal_device_ptr()
        # 2. the camera moves to B: the history follows it
        _move_and_render(r, B, 4)
        t2 = r.temporal_accumulate("accum", 4)
        n2 = r.read_temporal_count()
        acc2, g2 = r.read_accum(), r.read_guides()
        h2 = r.temporal_images(acc2, g2["hit"], g2["normal"], B, t1, n1, g1["hit"], g1["normal"], A, 4)
        assert same_bits(t2, h2[0]).all() and same_bits(n2, h2[1]).all()
        assert same_bits(r.read_temporal(), t2).all()      # the hook left the context's images alone
        assert r.temporal_device_ptr() and r.temporal_device_ptr() != p1
        assert n2.max() > 7.0 and (n2 > 4.0).sum() > 0.5 * (n2 > 0).sum()
        assert not same_bits(t2[..., :3], acc2[..., :3]).all()
        # 3. the denoised image as the source, against the history of step 2 (same view)
        d = r.denoise()
        t3 = r.temporal_accumulate("denoised", 4)
        n3 = r.read_temporal_count()
        h3 = r.temporal_images(d, g2["hit"], g2["normal"], B, t2, n2, g2["hit"], g2["normal"], B, 4)
        assert same_bits(t3, h3[0]).all() and same_bits(n3, h3[1]).all()
        assert n3.max() > 11.0
        # additive: the accumulator, the guides and the denoised image are those of a context that never
        # ran the stage, and the guide planes are where they were
        _move_and_render(plain, A, 0)
        _move_and_render(plain, B, 4)
        assert same_bits(plain.read_accum(), r.read_accum()).all()
        assert same_bits(plain.denoise(), r.read_denoised()).all() and same_bits(d, r.read_denoised()).all()
        gp = plain.read_guides()
        assert all(same_bits(gp[k], g2[k]).all() for k in gp)
        assert ptrs == [r.guide_device_ptr(p) for p in ("ray", "hit", "normal")]
        assert plain.temporal_device_ptr() is None
    finally:
        r.close()
        plain.close()


# ---- case 4: state ---------------------------------------------------------------------------------
def _state_error(call, word=None):
    with pytest.raises(RMRError) as e:
        call()
    assert e.value.code == -5, str(e.value)
    if word:
        assert word in str(e.value)


def test_state_rules(tmp_path):
    B, A = view_pair(W0, H0)
    r = _context(CORNELL)
    try:
        got, want = str(tmp_path / "got.bmp"), str(tmp_path / "want.bmp")
        # before the first call
        _state_error(r.read_temporal, "rmr_temporal_accumulate")
        _state_error(r.read_temporal_count)
        _state_error(lambda: r.set_output_source("temporal"), "rmr_temporal_accumulate")
        assert r.temporal_device_ptr() is None
        _move_and_render(r, A, 0)
        r.save_bmp(got)                                     # (the refused source left the accumulator selected)
        encode_bmp(r.read_accum(), want)
        assert open(got, "rb").read() == open(want, "rb").read()
        _state_error(lambda: r.temporal_accumulate("denoised", 4), "rmr_denoise")
        for bad in ({"max_history": 0.0}, {"sigma_z": float("inf")}, {"normal_pow2": 9}):
            with pytest.raises(RMRError) as e:
                r.temporal_accumulate("accum", 4, **bad)
            assert e.value.code == -1, bad
        for samples in (0.0, -2.0, float("nan")):
            with pytest.raises(RMRError) as e:
                r.temporal_accumulate("accum", samples)
            assert e.value.code == -1
        with pytest.raises(RMRError) as e:
            r.temporal_accumulate(abi.OUTPUT_TEMPORAL, 4)
        assert e.value.code == -1
        with pytest.raises(ValueError):
            r.temporal_accumulate("temporal", 4)
        assert r.temporal_device_ptr() is None
        # a step, then the output source reads the temporal image
        t1 = r.temporal_accumulate("accum", 4)
        r.set_output_source("temporal")
        r.save_bmp(got)
        encode_bmp(t1, want)
        assert open(got, "rb").read() == open(want, "rb").read()
        scr = r.display((W0 / 2.0, H0 / 2.0), 1.0, (0, 0), (W0, H0), screen_size=(W0, H0))
        r.set_output_source("accum")
        assert np.array_equal(scr, r.display((W0 / 2.0, H0 / 2.0), 1.0, (0, 0), (W0, H0), screen_size=(W0, H0)))
        # set_view, set_params and a thin-lens model keep the history
        r.set_view(B)
        r.set_params(abi.default_params(max_bounces=3))
        r.set_camera_model("thinlens", aperture=0.0)
        r.render_spp(time_schedule(4, first_sample=4), first_sample=0)
        t2 = r.temporal_accumulate("accum", 4)
        assert r.read_temporal_count().max() > 7.0 and not same_bits(t2, r.read_accum()).all()
        # no guides under the equirect and ortho models; the history survives the refusal
        for model in ("equirect", "ortho"):
            r.set_camera_model(model)
            _state_error(lambda: r.temporal_accumulate("accum", 4), "equirect")
        r.set_camera_model("view")
        assert same_bits(r.read_temporal(), t2).all()
        # rmr_temporal_reset drops the history: the next step returns the source
        r.set_output_source("temporal")
        r.temporal_reset()
        _state_error(r.read_temporal)
        _state_error(lambda: r.save_bmp(got), "temporal")
        r.set_output_source("accum")
        assert r.temporal_device_ptr() is None
        t = r.temporal_accumulate("accum", 4)
        assert same_bits(t, r.read_accum()).all() and r.read_temporal_count().max() == 4.0
        # rmr_reload drops it (and frees the planes), and so does a scene load
        r.reload()
        _state_error(r.read_temporal)
        r.render_spp(time_schedule(4))
        t = r.temporal_accumulate("accum", 4)
        assert same_bits(t, r.read_accum()).all() and r.read_temporal_count().max() == 4.0
        r.render_spp(time_schedule(4, first_sample=8), first_sample=0)
        r.temporal_accumulate("accum", 4)                   # (the same view: every live pixel finds itself)
        # (4 + 4 up to the normal term's rounding: |n|^2 is 1 to float precision, raised to the 32nd power)
        assert 7.9 < r.read_temporal_count().max() < 8.001
        r.load_scene(CSG64, "rm1")
        _state_error(r.read_temporal)
        r.render_spp(time_schedule(4), first_sample=0)
        t = r.temporal_accumulate("accum", 4)
        assert same_bits(t, r.read_accum()).all() and r.read_temporal_count().max() == 4.0
    finally:
        r.close()


def test_caller_stream_and_bound_accumulator():
    import torch
    B, A = view_pair(W0, H0)
    r, own = _context(CORNELL), _context(CORNELL)
    try:
        s = torch.cuda.Stream()
        acc = torch.zeros((H0, W0, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        r.set_stream(s.cuda_stream)
        r.bind_accum(acc.data_ptr(), acc.numel() * 4)
        out = []
        for c in (r, own):
            _move_and_render(c, A, 0)
            c.temporal_accumulate("accum", 4)
            _move_and_render(c, B, 4)
            c.denoise(iterations=3)
            out.append((c.temporal_accumulate("denoised", 4), c.read_temporal_count()))
        s.synchronize()
        assert same_bits(acc.cpu().numpy(), own.read_accum()).all()
        assert same_bits(out[0][0], out[1][0]).all() and same_bits(out[0][1], out[1][1]).all()
        assert out[0][1].max() > 7.0
    finally:
        r.close()
        own.close()
