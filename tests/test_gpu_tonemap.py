"""The tone-mapping stage (rmr_tonemap) on the GPU against the NumPy statement
tests/tonemap_ref.py: the histogram with ==, the curves bit for bit, the meter within 2^-40 of the
reference run on the library's own histogram (255 double products and sums of magnitude <= 16 at 2^-52
each), the scale within one float32 ulp of float32(2^l), and the state rules and outputs."""
import os
import subprocess

import numpy as np
import pytest

from raymarchrenderer_amd import Renderer, RMRError, abi, default_camera_view, encode_bmp, time_schedule

from .conftest import ROOT, SCENES
from . import tonemap_ref as ref
from .test_gpu_parity import same_bits

pytestmark = pytest.mark.gpu

CORNELL = os.path.join(SCENES, "cornell5.scene")
CLI = os.path.join(ROOT, "raymarchrenderer_amd", "rmr_cli")
F = np.float32
L_BOUND = 2.0 ** -40
# a single pixel; odd tails on both axes; more than one block; many blocks; and more pixels than 512 blocks of
# 1024 take in one round (533027 > 524288: the block cap and a second, ragged round of the grid-stride loop)
SHAPES = [(1, 1), (37, 29), (200, 120), (640, 360), (1031, 517)]
CURVES = [("linear", ref.LINEAR), ("reinhard", ref.REINHARD), ("aces", ref.ACES)]


def noise_image(W, H, seed, specials=True):
    """Log-uniform noise over 2^-20 .. 2^18 with about 5% specials and alpha-0 pixels sprinkled in."""
    rng = np.random.default_rng(seed)
    img = np.exp2(rng.uniform(-20.0, 18.0, (H, W, 4))).astype(F)
    img[..., 3] = 1.0
    if specials:
        pick = rng.uniform(size=(H, W))
        vals = np.array([np.nan, np.inf, -np.inf, -1.0, 0.0, -0.0, 1e-42], F)
        idx = pick < 0.04
        ch = rng.integers(0, 3, (H, W))
        v = vals[rng.integers(0, len(vals), (H, W))]
        for k in range(3):
            m = idx & (ch == k)
            img[..., k][m] = v[m]
        img[..., 3][(pick >= 0.04) & (pick < 0.05)] = 0.0
    return img


def images(W, H):
    flat = np.full((H, W, 4), 0.18, F)
    flat[..., 3] = 1.0
    skipped = noise_image(W, H, 3, specials=False)
    skipped[..., 3] = 0.0
    skipped[::2, :, 3] = 1.0
    skipped[::2, :, 1] = np.nan
    ends = np.zeros((H, W, 4), F)
    ends[..., 3] = 1.0
    ends[:, ::2, :3] = 1e6
    ends[:, 1::3, 1] = 1e-7
    return {"noise": noise_image(W, H, W * 1000 + H), "flat": flat, "skipped": skipped, "ends": ends}


@pytest.fixture(scope="module")
def contexts():
    made = {}

    def get(W, H):
        if (W, H) not in made:
            made[W, H] = Renderer(0, W, H)
        return made[W, H]
    yield get
    for r in made.values():
        r.close()


# ---- the histogram -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", SHAPES, ids=lambda v: str(v))
def test_histogram_equals_the_reference(contexts, W, H):
    r = contexts(W, H)
    for name, img in images(W, H).items():
        r.write_accum(img)
        hist, skipped = r.luminance_histogram("accum")
        want, want_skipped = ref.hist_ref(img)
        assert np.array_equal(hist, want), (name, np.flatnonzero(hist != want)[:8])
        assert skipped == want_skipped, name
        assert int(hist.sum()) + skipped == W * H, name
        if name == "flat":
            assert (hist > 0).sum() == 1 and skipped == 0
        if name == "skipped":
            assert hist.sum() == 0 and skipped == W * H
        if name == "ends":
            assert hist[0] + hist[255] == W * H and (W * H == 1 or (hist[0] > 0 and hist[255] > 0))
        assert same_bits(r.read_accum(), img).all(), name


def test_folded_histogram_form_counts_the_same():
    """The diagnostic library's k_lum_hist that folds equal bins inside the wave (the form measured and not
    kept): the same counts, on ragged tails too."""
    W, H = 200, 120
    r = Renderer(0, W, H, diag=True)
    try:
        assert r.lib.rmr_diag_tonemap_fold(r.ctx, 1) == 0
        for name, img in images(W, H).items():
            r.write_accum(img)
            hist, skipped = r.luminance_histogram("accum")
            want, want_skipped = ref.hist_ref(img)
            assert np.array_equal(hist, want) and skipped == want_skipped, name
    finally:
        r.close()


# ---- manual exposure ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(37, 29), (200, 120)], ids=lambda v: str(v))
def test_manual_exposure_is_the_reference_bit_for_bit(contexts, W, H):
    r = contexts(W, H)
    img = noise_image(W, H, 7)
    r.write_accum(img)
    before = r.read_accum().tobytes()
    for name, curve in CURVES:
        for ev in (-3.0, 0.0, 2.5):
            out = r.tonemap("accum", curve=name, exposure=ev, white=2.5)
            l, scale = r.read_exposure()
            assert l == ev and scale == F(np.exp2(ev)), (ev, l, scale)
            want = ref.curve_ref(curve, img, scale, white=2.5)
            assert same_bits(out, want).all(), (name, ev)
            assert same_bits(r.read_tonemapped(), out).all()
            assert r.tonemapped_device_ptr()
    assert r.read_accum().tobytes() == before == img.tobytes()


# ---- auto exposure -----------------------------------------------------------------------------------------
def _check_auto(r, img, curve_name, curve, l_prev, **kw):
    """One auto-exposed call on the accumulator's image; returns the reported l."""
    out = r.tonemap("accum", curve=curve_name, exposure="auto", **kw)
    l, scale = r.read_exposure()
    hist, _ = r.luminance_histogram("accum")
    assert np.array_equal(hist, ref.hist_ref(img)[0])
    want_l = ref.meter_ref(hist, l_prev, **kw)
    print("auto: l %.17g, reference %.17g, |d| %.3g (bound %.3g)" % (l, want_l, abs(l - want_l), L_BOUND))
    assert abs(l - want_l) <= L_BOUND
    s = F(2.0 ** l)
    assert np.nextafter(s, F(0)) <= scale <= np.nextafter(s, F(np.inf)), (scale, s)
    assert same_bits(out, ref.curve_ref(curve, img, scale)).all()
    assert r.read_exposure() == (l, scale)   # (the histogram call left the state alone)
    return l


@pytest.mark.parametrize("W,H", [(37, 29), (200, 120)], ids=lambda v: str(v))
def test_auto_exposure_and_adaptation(contexts, W, H):
    r = contexts(W, H)
    r.tonemap_reset()
    img1, img2 = noise_image(W, H, 11), noise_image(W, H, 12) * F(0.03125)
    img2[..., 3] = img1[..., 3]
    black = np.zeros((H, W, 4), F)
    black[..., 3] = 1.0
    # the first call has no state: its own target, whatever adapt is
    r.write_accum(img1)
    l1 = _check_auto(r, img1, "aces", ref.ACES, None, adapt=0.5)
    t1 = ref.meter_target(ref.hist_ref(img1)[0])
    assert abs(l1 - t1) <= L_BOUND
    # the second image: half the way from l1 to its own target
    r.write_accum(img2)
    l2 = _check_auto(r, img2, "reinhard", ref.REINHARD, l1, adapt=0.5)
    t2 = ref.meter_target(ref.hist_ref(img2)[0])
    assert abs(l2 - (l1 + 0.5 * (t2 - l1))) <= L_BOUND and abs(t2 - t1) > 3.0
    # a manual call in between leaves the state alone
    r.tonemap("accum", exposure=1.0)
    assert r.read_exposure() == (1.0, F(2.0))
    l3 = _check_auto(r, img2, "linear", ref.LINEAR, l2, adapt=0.5)
    assert abs(l3 - (l2 + 0.5 * (t2 - l2))) <= L_BOUND
    # an all-black image keeps the previous l
    r.write_accum(black)
    l4 = _check_auto(r, black, "aces", ref.ACES, l3, adapt=0.5)
    assert l4 == l3
    # after a reset the second image alone gives its target
    r.tonemap_reset()
    r.write_accum(img2)
    l5 = _check_auto(r, img2, "aces", ref.ACES, None, adapt=0.5, key=0.25, exposure_ev=-0.5, low_pct=0.2, high_pct=0.7)
    assert abs(l5 - ref.meter_target(ref.hist_ref(img2)[0], 0.25, 0.2, 0.7, -0.5)) <= L_BOUND
    # nothing metered and no state: exposure_ev
    r.tonemap_reset()
    r.write_accum(black)
    assert _check_auto(r, black, "aces", ref.ACES, None, exposure_ev=1.25) == 1.25


# ---- real sources and the state rules ---------------------------------------------------------------
W0, H0 = 44, 36


def _state_error(call, word=None):
    with pytest.raises(RMRError) as e:
        call()
    assert e.value.code == -5, str(e.value)
    if word:
        assert word in str(e.value)


def test_real_sources_state_rules_and_outputs(tmp_path):
    r, other = Renderer(0, W0, H0), Renderer(0, W0, H0)
    got, want, first = str(tmp_path / "got.bmp"), str(tmp_path / "want.bmp"), str(tmp_path / "first.bmp")
    centre, size = (W0 / 2.0, H0 / 2.0), (W0, H0)
    try:
        r.load_scene(CORNELL, "rm1")
        r.set_params(abi.default_params(max_bounces=4))
        # before any tonemap
        _state_error(lambda: r.set_output_source("tonemapped"), "rmr_tonemap")
        _state_error(r.read_tonemapped, "rmr_tonemap")
        _state_error(r.read_exposure)
        assert r.tonemapped_device_ptr() is None
        r.render_spp(time_schedule(4))
        acc = r.read_accum()
        r.save_bmp(first)                                   # (the refused source left the accumulator selected)
        encode_bmp(acc, want)
        assert open(first, "rb").read() == open(want, "rb").read()
        with pytest.raises(RMRError) as e:
            r.tonemap(source=7)
        assert e.value.code == -1
        with pytest.raises(RMRError) as e:
            r.tonemap(source=abi.OUTPUT_TONEMAPPED)
        assert e.value.code == -1
        with pytest.raises(RMRError) as e:
            r.tonemap("accum", white=0.0)
        assert e.value.code == -1
        with pytest.raises(ValueError):
            r.tonemap("tonemapped")
        _state_error(lambda: r.tonemap("denoised"), "rmr_denoise")
        _state_error(lambda: r.tonemap("temporal"), "rmr_temporal_accumulate")
        _state_error(lambda: r.luminance_histogram("denoised"), "rmr_denoise")
        assert r.tonemapped_device_ptr() is None
        # the three sources
        t_acc = r.tonemap("accum", exposure=1.0)
        assert same_bits(t_acc, ref.curve_ref(ref.ACES, acc, 2.0)).all()
        dn = r.denoise(iterations=3)
        _state_error(r.read_tonemapped)                     # (rmr_denoise: where a denoised image becomes invalid)
        tmp = r.temporal_accumulate("denoised", 4)
        t_dn = r.tonemap("denoised", curve="reinhard", exposure="auto")
        l, scale = r.read_exposure()
        assert same_bits(r.read_denoised(), dn).all()
        assert same_bits(t_dn, ref.curve_ref(ref.REINHARD, dn, scale)).all()
        assert abs(l - ref.meter_ref(ref.hist_ref(dn)[0])) <= L_BOUND
        assert np.array_equal(r.luminance_histogram("denoised")[0], ref.hist_ref(dn)[0])
        r.temporal_accumulate("denoised", 4)                # (a tonemapped image of the denoised image stays)
        assert same_bits(r.read_tonemapped(), t_dn).all()
        tmp = r.read_temporal()
        t_tmp = r.tonemap("temporal", curve="linear", exposure=-1.0)
        assert same_bits(r.read_temporal(), tmp).all()
        assert same_bits(t_tmp, ref.curve_ref(ref.LINEAR, tmp, 0.5)).all()
        assert np.array_equal(r.luminance_histogram("temporal")[0], ref.hist_ref(tmp)[0])
        # the outputs under the tonemapped source
        r.set_output_source("tonemapped")
        r.save_bmp(got)
        encode_bmp(r.read_tonemapped(), want)
        assert open(got, "rb").read() == open(want, "rb").read()
        scr = r.display(centre, 1.0, (0, 0), size, screen_size=size)
        other.write_accum(t_tmp)
        assert np.array_equal(scr, other.display(centre, 1.0, (0, 0), size, screen_size=size))
        import torch
        dev = torch.zeros((H0, W0, 4), dtype=torch.uint8, device="cuda")
        r.display_device(centre, 1.0, (0, 0), size, dev, W0, H0)
        r.sync()
        assert np.array_equal(dev.cpu().numpy(), scr)
        # the next temporal step replaces the image it was made from
        r.temporal_accumulate("denoised", 4)
        _state_error(r.read_tonemapped)
        _state_error(lambda: r.save_bmp(got), "tonemapped")
        _state_error(lambda: r.display(centre, 1.0, (0, 0), size, screen_size=size), "tonemapped")
        assert r.tonemapped_device_ptr() is None
        # back on the accumulator: the file written before any tonemap
        r.set_output_source("accum")
        r.save_bmp(got)
        assert open(got, "rb").read() == open(first, "rb").read()
        assert same_bits(r.read_accum(), acc).all()
        # a render invalidates it; the source stays selected and refuses to show a stale image
        r.tonemap("accum")
        r.set_output_source("tonemapped")
        r.render_spp(time_schedule(4, first_sample=4), first_sample=4)
        _state_error(r.read_tonemapped)
        assert r.tonemapped_device_ptr() is None
        _state_error(lambda: r.save_bmp(got), "tonemapped")
        r.set_output_source("accum")
        _state_error(lambda: r.set_output_source("tonemapped"))
        # rmr_reload drops the image, the exposure and the adaptation state
        r.tonemap("accum", exposure="auto")
        r.reload()
        _state_error(r.read_tonemapped)
        _state_error(r.read_exposure)
        r.render_spp(time_schedule(4))
        r.tonemap("accum", exposure="auto", adapt=0.25)
        assert abs(r.read_exposure()[0] - ref.meter_ref(ref.hist_ref(r.read_accum())[0])) <= L_BOUND
    finally:
        r.close()
        other.close()


# ---- rmr_cli ------------------------------------------------------------------------------------------------
def test_cli_writes_the_pipeline_image(tmp_path):
    """rmr_cli --samples 4 --denoise 3 --tonemap aces --exposure auto at 44x36: the BMP the Python pipeline
    writes for the same steps, byte for byte; bad values are usage errors."""
    out, want = str(tmp_path / "cli.bmp"), str(tmp_path / "want.bmp")
    base = [CLI, "--scene", CORNELL, "--variant", "rm1", "--size", "%dx%d" % (W0, H0), "--samples", "4", "--bounces", "3",
            "--out", out, "--quiet"]
    p = subprocess.run(base + ["--denoise", "3", "--tonemap", "aces", "--exposure", "auto"], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    for bad in (["--tonemap", "foo"], ["--exposure", "auto:-1"], ["--tonemap", "reinhard:0"]):
        q = subprocess.run(base + bad, capture_output=True, text=True, timeout=120)
        assert q.returncode == 2, (bad, q.stdout + q.stderr)
    cli_bytes = open(out, "rb").read()
    r = Renderer(0, W0, H0)
    try:
        r.load_scene(CORNELL, "rm1")
        r.set_params(abi.default_params(max_bounces=3))
        r.set_view(default_camera_view(W0, H0))   # the driver's camera (Camera.cpp through rmr_camera_view)
        r.render_spp(time_schedule(4))
        r.denoise(iterations=3)
        r.tonemap("denoised", curve="aces", exposure="auto")
        r.set_output_source("tonemapped")
        r.save_bmp(want)
        assert cli_bytes == open(want, "rb").read()
        r.set_output_source("denoised")
        r.save_bmp(want)
        assert cli_bytes != open(want, "rb").read()
    finally:
        r.close()
