"""The variance-guided denoiser (rmr_denoise_variance) on the GPU against the float64
statement tests/denoise_variance_ref.py: the kernels on synthetic images through the test hook in both
forms, the real pipeline (uniform, adaptive, caller stream), one quality row, the state rules, the CLI.

Bound, over v-live pixels: image |gpu - ref| <= 1e-4 (|ref| + M), M the largest finite |rgb| over live
input pixels (tests/denoise_ref.py tolerance_scale, the plain filter's bound); both variance planes
|gpu - ref| <= 1e-4 (ref + M_v), M_v the largest reference seed variance. Every other pixel: the image
bit for bit the accumulator, the planes exactly -1. Alpha is never changed.

Measured share of the bound (MI355X): at most 0.0025 (image) and 0.0031 (variance planes) over every
case of this file, eight passes included; the two forms of the pass gave the same bits in all 200 runs
of case 1 (the tiled form adds a tap that is not v-live as exact zeros where the plain form skips it)."""
import os
import subprocess

import numpy as np
import pytest

from oracle import camera
from raymarchrenderer_amd import (Renderer, RMRError, abi, default_camera_view, encode_bmp, parity_schedule,
                                 time_schedule)

from .conftest import GOLDEN, ROOT, SCENES
from .denoise_ref import tolerance_scale
from .denoise_variance_ref import denoise_variance_ref, synthetic_case, vlive_mask
from .test_denoise_cpu import mse
from .test_gpu_denoise import _read_pfm
from .test_gpu_parity import same_bits

pytestmark = pytest.mark.gpu

CORNELL = os.path.join(SCENES, "cornell5.scene")
CSG64 = os.path.join(SCENES, "csg64.scene")
CLI = os.path.join(ROOT, "raymarchrenderer_amd", "rmr_cli")


def _assert_close(gpu, ref, a, b, nrm, what):
    """gpu, ref: (image, seed, filtered variance). The bound above; returns the worst shares of it."""
    vl = vlive_mask(np.asarray(a, np.float32), np.asarray(b, np.float32), np.asarray(nrm, np.float32))
    M = tolerance_scale(a, nrm)
    Mv = float(max(ref[1].max(), 0.0))
    img, seed, var = gpu
    with np.errstate(invalid="ignore"):   # (pixels that are not v-live may hold NaN or inf)
        err = np.abs(img[..., :3].astype(np.float64) - ref[0][..., :3])
    bound = 1e-4 * (np.abs(ref[0][..., :3]) + M)
    worst = [float((err[vl] / bound[vl]).max()) if vl.any() and M > 0 else 0.0]
    assert np.isfinite(img[vl][:, :3]).all(), what
    assert (err[vl] <= bound[vl]).all(), (what, worst)
    for plane, want in ((seed, ref[1]), (var, ref[2])):
        e = np.abs(plane.astype(np.float64) - want)
        bd = 1e-4 * (want + Mv)
        worst.append(float((e[vl] / bd[vl]).max()) if vl.any() and Mv > 0 else 0.0)
        assert (e[vl] <= bd[vl]).all(), (what, worst)
        assert (plane[~vl] == -1.0).all(), what
    assert same_bits(img[~vl], np.asarray(a, np.float32)[~vl]).all(), what
    assert same_bits(img[..., 3], np.asarray(a, np.float32)[..., 3]).all(), what
    return worst


# ---- case 1: the images hook against the reference, both forms -------------------------------------
@pytest.fixture(scope="module")
def diag():
    r = Renderer(0, 8, 8, diag=True)
    yield r
    r.lib.rmr_diag_denoise_tiled(r.ctx, 3)
    r.close()


@pytest.mark.parametrize("W,H", [(1, 1), (5, 1), (33, 9), (67, 29), (44, 36)], ids=lambda v: str(v))
def test_images_hook_matches_reference(diag, W, H):
    a, b, hit, nrm, dead = synthetic_case(W, H)
    worst, n, equal = np.zeros(3), 0, 0
    for iters in (0, 1, 2, 3, 8):
        for radius in (0, 1, 3, 4):
            for sc in (0.0, 0.5):
                kw = dict(iterations=iters, var_radius=radius, sigma_c=sc)
                ref = denoise_variance_ref(a, b, hit, nrm, **kw)
                out = {}
                for mask in (0, 3):   # plain; steps 1 and 2 tiled
                    assert diag.lib.rmr_diag_denoise_tiled(diag.ctx, mask) == 0
                    out[mask] = diag.denoise_variance_images(a, b, hit, nrm, **kw)
                    worst = np.maximum(worst, _assert_close(out[mask], ref, a, b, nrm, "%dx%d %s form %d" % (W, H, kw, mask)))
                if iters == 0:
                    assert same_bits(out[0][0], a).all() and same_bits(out[0][1], out[0][2]).all()
                n += 1
                equal += all(same_bits(x, y).all() for x, y in zip(out[0], out[3]))
    print("%dx%d: worst share of the bound: image %.3g, seed %.3g, variance %.3g; the two forms bitwise equal in %d of %d runs"
          % (W, H, worst[0], worst[1], worst[2], equal, n))


# ---- case 2: the real pipeline ---------------------------------------------------------------------
def _check_pipeline(r, what):
    gpu = (r.denoise_variance(), r.read_variance("seed"), r.read_variance("filtered"))
    assert r.variance_device_ptr("seed") and r.variance_device_ptr(abi.VARIANCE_FILTERED)
    assert r.variance_device_ptr("seed") != r.variance_device_ptr("filtered")
    acc, half, g = r.read_accum(), r.read_half(), r.read_guides()
    hook = r.denoise_variance_images(acc, half, g["hit"], g["normal"])
    for x, y in zip(gpu, hook):
        assert same_bits(x, y).all(), what
    # the hook left the context's images alone
    assert same_bits(r.read_denoised(), gpu[0]).all() and same_bits(r.read_variance("filtered"), gpu[2]).all()
    ref = denoise_variance_ref(acc, half, g["hit"], g["normal"])
    worst = _assert_close(gpu, ref, acc, half, g["normal"], what)
    print("%s: worst share of the bound: image %.3g, seed %.3g, variance %.3g" % ((what,) + tuple(worst)))
    assert not same_bits(gpu[0][..., :3], acc[..., :3]).all() and (gpu[2] >= 0).any()


def _pipeline_context(path, W=44, H=36):
    r = Renderer(0, W, H)
    r.load_scene(path, "rm1")
    r.set_params(abi.default_params(max_bounces=4))
    r.set_view(camera.default_view(W, H))
    return r


@pytest.mark.parametrize("path", [CORNELL, CSG64], ids=["cornell5", "csg64"])
@pytest.mark.parametrize("mode", ["uniform", "adaptive", "stream"])
def test_pipeline_matches_hook_and_reference(path, mode):
    r = _pipeline_context(path)
    try:
        if mode == "stream":
            import torch
            s = torch.cuda.Stream()
            r.set_stream(s.cuda_stream)
        if mode == "adaptive":   # §4.8's case: per-tile sample counts from 4 to 32
            r.render_adaptive(parity_schedule(32), threshold=np.float32(0.6), min_samples=4, pass_samples=4, block_tiles=2)
            if path == CORNELL:
                assert len(np.unique(r.sample_counts())) > 2
        else:
            r.set_error_estimate(True)
            r.render_spp(time_schedule(16))
        _check_pipeline(r, "%s %s" % (os.path.basename(path), mode))
    finally:
        r.close()


# ---- case 3: one quality row -----------------------------------------------------------------------
def test_quality_row_on_gpu():
    """csg64 at the golden's 64x48 view, 64 spp: the guided image's MSE against the converged golden is
    at most the better of the plain filter's (3 and 5 iterations) and at most half the noisy image's."""
    gold = np.load(os.path.join(GOLDEN, "img_rm1_csg64_b4.npz"))
    conv, view = gold["conv"], gold["view"]
    H, W = conv.shape[:2]
    r = Renderer(0, W, H)
    try:
        r.load_scene(CSG64, "rm1")
        r.set_params(abi.default_params(max_bounces=4))
        r.set_view(view)
        r.set_error_estimate(True)
        r.render_spp(parity_schedule(64))
        acc = r.read_accum()
        p3, p5 = r.denoise(iterations=3), r.denoise(iterations=5)
        guided = r.denoise_variance(iterations=5)
    finally:
        r.close()
    e = [mse(x, conv) for x in (acc, p3, p5, guided)]
    print("csg64 @64 spp: noisy %.3e, plain 3 it %.3e, plain 5 it %.3e, guided %.3e" % tuple(e))
    assert e[3] <= min(e[1], e[2]) and e[3] <= 0.5 * e[0]


# ---- case 4: state ---------------------------------------------------------------------------------
def test_state_rules(tmp_path):
    W, H = 44, 36
    r = _pipeline_context(CORNELL, W, H)
    try:
        def state_error(call, word=None):
            with pytest.raises(RMRError) as e:
                call()
            assert e.value.code == -5, str(e.value)
            if word:
                assert word in str(e.value)
        # the estimate is off
        state_error(r.denoise_variance, "rmr_set_error_estimate")
        state_error(lambda: r.read_variance("seed"))         # before any call
        assert r.variance_device_ptr("seed") is None and r.variance_device_ptr("filtered") is None
        r.render_spp(time_schedule(2))
        state_error(r.denoise_variance, "rmr_set_error_estimate")
        r.set_error_estimate(True)                           # enabled after a render: not valid
        state_error(r.denoise_variance, "rmr_render_adaptive")
        # adaptive render: valid, with sample counts and tile errors to leave alone
        r.reload()
        r.render_adaptive(parity_schedule(32), threshold=np.float32(0.6), min_samples=4, pass_samples=4, block_tiles=2)
        for bad in ({"sigma_l": 0.0}, {"sigma_l": -1.0}, {"sigma_l": float("nan")}, {"sigma_l": float("inf")},
                    {"var_radius": -1}, {"var_radius": 5}, {"iterations": 9}, {"iterations": -1}, {"normal_pow2": 8},
                    {"sigma_z": 0.0}, {"sigma_c": -1.0}):
            with pytest.raises(RMRError) as e:
                r.denoise_variance(**bad)
            assert e.value.code == -1, bad
        plain_before = r.denoise(iterations=4, sigma_c=1.0)
        state_error(lambda: r.read_variance("filtered"))     # a plain denoise gives no planes
        before = (r.read_accum(), r.read_half(), r.read_guides(), r.tile_error(), r.sample_counts())
        guided = r.denoise_variance()
        seed = r.read_variance(abi.VARIANCE_SEED)
        after = (r.read_accum(), r.read_half(), r.read_guides(), r.tile_error(), r.sample_counts())
        assert same_bits(before[0], after[0]).all() and same_bits(before[1], after[1]).all()
        assert all(same_bits(before[2][k], after[2][k]).all() for k in before[2])
        assert same_bits(before[3], after[3]).all() and np.array_equal(before[4], after[4])
        assert same_bits(r.read_denoised(), guided).all() and not same_bits(guided, plain_before).all()
        # the output source and save_bmp read the guided image
        got, want = str(tmp_path / "got.bmp"), str(tmp_path / "want.bmp")
        r.set_output_source("denoised")
        r.save_bmp(got)
        encode_bmp(guided, want)
        assert open(got, "rb").read() == open(want, "rb").read()
        r.set_output_source("accum")
        # iterations 0: the accumulator, and the filtered variance is the seed
        assert same_bits(r.denoise_variance(iterations=0), before[0]).all()
        assert same_bits(r.read_variance("filtered"), seed).all() and same_bits(r.read_variance("seed"), seed).all()
        # a plain denoise after it: the same bits as before it, and the planes are invalid again
        assert same_bits(r.denoise(iterations=4, sigma_c=1.0), plain_before).all()
        state_error(lambda: r.read_variance("seed"), "rmr_denoise_variance")
        assert r.variance_device_ptr("seed") is None
        # a write to the accumulator makes the estimate invalid; a render makes the planes invalid
        r.denoise_variance()
        r.write_accum(before[0])
        state_error(lambda: r.read_variance("seed"))
        state_error(r.denoise_variance)
        r.reload()
        r.render_spp(time_schedule(4))                       # (the setting survived the reload)
        r.denoise_variance(iterations=1)
        assert r.variance_device_ptr("filtered")
        r.render_spp(time_schedule(1, first_sample=4), first_sample=4)
        state_error(lambda: r.read_variance("filtered"))
        assert r.variance_device_ptr("filtered") is None and r.denoised_device_ptr() is None
        r.denoise_variance(iterations=1)
        # the guides' refusal under the equirect model stays
        r.reload()
        r.set_camera_model("equirect")
        r.render_spp(time_schedule(2))
        state_error(r.denoise_variance, "equirect")
    finally:
        r.close()


# ---- case 5: the CLI -------------------------------------------------------------------------------
def test_cli_variance_guided(tmp_path):
    """rmr_cli --samples 16 --denoise 5 --variance-guided --aov P at 44x36: the BMP of
    Renderer.denoise_variance byte for byte, and P_variance.pfm equal to read_variance('filtered')."""
    W, H = 44, 36
    out, prefix, want = str(tmp_path / "cli.bmp"), str(tmp_path / "aov"), str(tmp_path / "want.bmp")
    p = subprocess.run([CLI, "--scene", CORNELL, "--variant", "rm1", "--size", "%dx%d" % (W, H), "--samples", "16",
                        "--bounces", "3", "--denoise", "5", "--variance-guided", "--aov", prefix, "--out", out, "--quiet"],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    r = Renderer(0, W, H)
    try:
        r.load_scene(CORNELL, "rm1")
        r.set_params(abi.default_params(max_bounces=3))
        r.set_view(default_camera_view(W, H))
        r.set_error_estimate(True)
        r.render_spp(time_schedule(16))
        d = r.denoise_variance(iterations=5)
        var = r.read_variance("filtered")
        plain = r.denoise(iterations=5)
    finally:
        r.close()
    encode_bmp(d, want)
    assert open(out, "rb").read() == open(want, "rb").read()
    assert not same_bits(d, plain).all()
    vp = _read_pfm(prefix + "_variance.pfm")
    assert same_bits(vp[..., 0], var).all() and (vp[..., 1:] == 0).all()
    assert os.path.exists(prefix + "_normal.pfm")
