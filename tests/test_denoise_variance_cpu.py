"""The variance-guided denoiser's definition (tests/denoise_variance_ref.py) and its host-side pieces,
without a GPU: the reference's own properties, the quality gate against the converged goldens, the C
ABI's defaults and parameter check, the Python argument errors, the CLI's rejections, and the new
kernels' resources compiled for gfx950 (not run).

Quality gate, measured with this reference (mse of tests/test_denoise_cpu.py, oracle renders at the
goldens' 64x48 views, five iterations, defaults): guided / noisy is at most 0.35 over the twelve rows,
and at 64 and 256 spp guided / min(plain 3 it, plain 5 it) is at most 0.70."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import oracle, scene_compile
from raymarchrenderer_amd import Renderer, abi, parity_schedule
from raymarchrenderer_amd._lib import lib

from .conftest import GOLDEN, ROOT
from .denoise_ref import denoise_ref, oracle_guides
from .denoise_variance_ref import (denoise_variance_ref, flat_guides, lum, synthetic_case, variance_seed_ref,
                                   vlive_mask)
from .test_denoise_cpu import ERR_CASES, mse

CSRC = os.path.join(ROOT, "raymarchrenderer_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CLI = os.path.join(ROOT, "raymarchrenderer_amd", "rmr_cli")
SPP = (4, 16, 64, 256)


# ---- the reference's own properties ----------------------------------------------------------------
def test_constant_image_stays_constant():
    H, W = 19, 23
    hit, nrm = flat_guides(H, W, 2.0)
    acc = np.empty((H, W, 4), np.float32)
    acc[...] = (0.3, 0.7, 1.9, 1.0)
    for sc in (0.0, 0.5):
        out, seed, var = denoise_variance_ref(acc, acc, hit, nrm, iterations=5, sigma_c=sc)
        assert np.abs(out - acc.astype(np.float64)).max() <= 1e-12
        assert (seed == 0).all() and (var == 0).all()


def test_two_ids_do_not_mix():
    H, W = 16, 24
    ids = np.where(np.arange(W)[None, :] < 11, 1.0, 4.0) * np.ones((H, 1))
    hit, nrm = flat_guides(H, W, ids)
    rng = np.random.default_rng(7)
    acc = np.ones((H, W, 4), np.float32)
    acc[..., :3] = np.where(ids[..., None] == 1.0, 0.2, 0.8) + rng.uniform(-0.05, 0.05, (H, W, 3))
    half = acc.copy()
    half[..., :3] += rng.uniform(-0.05, 0.05, (H, W, 3)).astype(np.float32)
    out, seed, var = denoise_variance_ref(acc, half, hit, nrm, iterations=4)
    left, right = out[:, :11, :3], out[:, 11:, :3]
    assert left.max() <= acc[:, :11, :3].max() + 1e-12 and right.min() >= acc[:, 11:, :3].min() - 1e-12
    assert left.max() < 0.3 and right.min() > 0.7
    assert left.std() < 0.5 * acc[:, :11, :3].std() and right.std() < 0.5 * acc[:, 11:, :3].std()
    # the seed's window stops at the id edge too: a side with A == B has variance 0 right up to it
    half2 = half.copy()
    half2[:, :11] = acc[:, :11]
    seed2 = variance_seed_ref(acc, half2, nrm, 3)
    assert (seed2[:, :11] == 0).all() and (seed2[:, 11:] > 0).all()
    # the variance shrinks where the filter averaged
    assert (var > 0).all() and var.mean() < 0.25 * seed.mean()


def test_pixels_that_are_not_vlive():
    """Sky, A.w = 0, B.w = 0, NaN / inf in A, NaN in B: bit for bit through every pass, variance -1 in
    both planes, and nothing of them reaches another pixel."""
    W, H = 24, 20
    a, b, hit, nrm, dead = synthetic_case(W, H)
    assert len(dead) == 6
    vl = vlive_mask(a, b, nrm)
    assert not vl[tuple(zip(*dead))].any() and vl.sum() == W * H - len(dead)
    out, seed, var = denoise_variance_ref(a, b, hit, nrm, iterations=3)
    for y, x in dead:
        assert np.array_equal(out[y, x].astype(np.float32), a[y, x], equal_nan=True)
        assert seed[y, x] == -1.0 and var[y, x] == -1.0
    assert np.isfinite(out[vl]).all() and (seed[vl] >= 0).all() and (var[vl] >= 0).all()
    assert np.array_equal(out[..., 3], a[..., 3].astype(np.float64))
    # what a dead pixel holds changes nothing elsewhere
    a2, b2 = a.copy(), b.copy()
    for y, x in dead:
        a2[y, x, :3] = np.where(np.isfinite(a[y, x, :3]), 1e6, a[y, x, :3])
        b2[y, x, :3] = np.where(np.isfinite(b[y, x, :3]), -1e6, b[y, x, :3])
    assert np.array_equal(vlive_mask(a2, b2, nrm), vl)
    out2, seed2, var2 = denoise_variance_ref(a2, b2, hit, nrm, iterations=3)
    assert np.array_equal(out2[vl], out[vl]) and np.array_equal(seed2[vl], seed[vl]) and np.array_equal(var2[vl], var[vl])


def test_zero_variance_region_keeps_its_values():
    """A == B over a region of distinct colours among noisy pixels: where the seed is 0 the luminance
    weight drops every differing tap, so the pixel keeps its value (to 1e-6) through five passes."""
    H, W = 30, 36
    hit, nrm = flat_guides(H, W, 2.0)
    rng = np.random.default_rng(5)
    a = np.ones((H, W, 4), np.float32)
    a[..., :3] = rng.uniform(0.1, 0.9, (H, W, 3))
    b = a.copy()
    b[..., :3] += rng.normal(0, 0.05, (H, W, 3)).astype(np.float32)
    region = (slice(8, 22), slice(10, 27))
    b[region] = a[region]
    # var_radius 0: the seed is 0 on every pixel of the region
    out, seed, var = denoise_variance_ref(a, b, hit, nrm, iterations=5, var_radius=0)
    assert (seed[region] == 0).all() and (var[region] == 0).all()
    assert np.abs(out[region] - a[region]).max() <= 1e-6
    outside = np.ones((H, W), bool)
    outside[region] = False
    assert np.abs(out[outside][:, :3] - a[outside][:, :3]).max() > 1e-3   # the rest was filtered
    # the default window: 0 where the whole window lies in the region
    out, seed, var = denoise_variance_ref(a, b, hit, nrm, iterations=5)
    inner = (slice(11, 19), slice(13, 24))
    assert (seed[inner] == 0).all() and (var[inner] == 0).all() and (seed[7, 9] > 0)
    assert np.abs(out[inner] - a[inner]).max() <= 1e-6


def test_radius_zero_seed_is_d_squared():
    W, H = 24, 20
    a, b, hit, nrm, dead = synthetic_case(W, H)
    vl = vlive_mask(a, b, nrm)
    seed = variance_seed_ref(a, b, nrm, 0)
    with np.errstate(all="ignore"):
        d = lum(a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64))
    assert np.array_equal(seed[vl], (d * d)[vl]) and (seed[~vl] == -1).all()
    # iterations = 0: the image is A, the filtered variance the seed
    out, s0, v0 = denoise_variance_ref(a, b, hit, nrm, iterations=0, var_radius=0)
    assert np.array_equal(out.astype(np.float32), a, equal_nan=True) and np.array_equal(s0, v0) and np.array_equal(s0, seed)


# ---- the quality gate ------------------------------------------------------------------------------
_rows = {}


def _quality_rows(name):
    """(noisy, plain 3 it, plain 5 it, guided) MSE per sample count of one scene, computed once."""
    if name in _rows:
        return _rows[name]
    path, kw = ERR_CASES[name]
    g = np.load(os.path.join(GOLDEN, "img_%s.npz" % name))
    conv, view = g["conv"], g["view"]
    H, W = conv.shape[:2]
    assert (W, H) == (64, 48)
    tables = scene_compile.load_scene_file(path, "rm1")
    prm = abi.default_params(**kw)
    hit, nrm = oracle_guides(tables, prm, view, W, H)
    times = parity_schedule(SPP[-1])
    orc = oracle.Oracle(tables, prm, view, W, H)
    rows, a, b, done = {}, None, None, 0
    for n in SPP:
        # A = render(times[:n]), B = render(times[1:n:2]), each continued from the previous count (the
        # running mean's bits do not depend on where a render is split)
        a = orc.render(times[done:n], first_sample=done, accum=a)
        b = orc.render(times[1:n:2][done // 2:], first_sample=done // 2, accum=b)
        done = n
        guided = denoise_variance_ref(a, b, hit, nrm, iterations=5)[0]
        rows[n] = (mse(a, conv), mse(denoise_ref(a, hit, nrm, iterations=3), conv),
                   mse(denoise_ref(a, hit, nrm, iterations=5), conv), mse(guided, conv))
    _rows[name] = rows
    return rows


@pytest.mark.parametrize("name", sorted(ERR_CASES))
def test_quality_gate(name):
    rows = _quality_rows(name)
    print("%-16s %5s %10s %10s %10s %10s" % ("scene", "spp", "noisy", "plain 3", "plain 5", "guided"))
    for n in SPP:
        print("%-16s %5d %10.3e %10.3e %10.3e %10.3e" % ((name, n) + rows[n]))
    for n in SPP:
        noisy, p3, p5, guided = rows[n]
        assert guided <= 0.5 * noisy, (name, n)
        if n >= 64:
            assert guided <= min(p3, p5), (name, n)


def test_split_renders_are_the_whole_renders():
    """The gate's continued renders are bitwise A = render(times[:n]) and B = render(times[1:n:2])."""
    name = "rm1_cornell5_b4"
    path, kw = ERR_CASES[name]
    g = np.load(os.path.join(GOLDEN, "img_%s.npz" % name))
    H, W = g["conv"].shape[:2]
    orc = oracle.Oracle(scene_compile.load_scene_file(path, "rm1"), abi.default_params(**kw), g["view"], W, H)
    times = parity_schedule(16)
    a = orc.render(times[4:16], first_sample=4, accum=orc.render(times[:4]))
    b = orc.render(times[1:16:2][2:], first_sample=2, accum=orc.render(times[1:4:2]))
    assert np.array_equal(a.view(np.uint32), orc.render(times[:16]).view(np.uint32))
    assert np.array_equal(b.view(np.uint32), orc.render(times[1:16:2]).view(np.uint32))


# ---- host-side pieces ------------------------------------------------------------------------------
def test_default_variance_params():
    p = abi.VarianceParams(-1.0, -1)
    lib().rmr_default_variance_params(C.byref(p))
    assert (p.sigma_l, p.var_radius) == (4.0, 3) and C.sizeof(abi.VarianceParams) == 8
    q = abi.default_variance_params()
    assert (q.sigma_l, q.var_radius) == (p.sigma_l, p.var_radius)
    assert (abi.VARIANCE_SEED, abi.VARIANCE_FILTERED) == (0, 1)
    q = abi.default_variance_params(sigma_l=2.5, var_radius=1)
    assert (q.sigma_l, q.var_radius) == (2.5, 1)


def test_check_variance_params():
    check = lib().rmr_check_variance_params
    ok = lambda s, r: check(C.byref(abi.VarianceParams(s, r)))   # noqa: E731
    assert check(None) == -1
    assert ok(4.0, 3) == 0
    for r in (0, 1, 4):
        assert ok(4.0, r) == 0, r
    for r in (-1, 5, 2 ** 31 - 1, -2 ** 31):
        assert ok(4.0, r) == -1, r
    tiny, big = float(np.finfo(np.float32).smallest_subnormal), float(np.finfo(np.float32).max)
    for s in (tiny, 1e-30, 1.0, big):
        assert ok(s, 3) == 0, s
    for s in (0.0, -0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert ok(s, 3) == -1, s


def test_library_exports_the_variance_calls():
    L = lib()
    for name in ("rmr_default_variance_params", "rmr_check_variance_params", "rmr_denoise_variance", "rmr_read_variance",
                 "rmr_variance_device_ptr", "rmr_denoise_variance_images"):
        assert hasattr(L, name), name
    # null contexts: RMR_E_INVALID / NULL before anything touches a GPU
    assert L.rmr_denoise_variance(None, None, None) == -1 and L.rmr_read_variance(None, 0, None, 0) == -1
    assert L.rmr_variance_device_ptr(None, 0) is None
    assert L.rmr_denoise_variance_images(None, None, None, None, None, 1, 1, None, None, None, None, None) == -1
    # rmr_denoise_params and rmr_abi_sizes are what they were
    out = (C.c_int32 * 16)(*([-7] * 16))
    assert L.rmr_abi_sizes(out, 16) == 8 and out[8] == 16 and out[9] == -7


def test_python_argument_errors():
    """The checks that happen before any call into the library (no context needed)."""
    r = Renderer.__new__(Renderer)   # no rmr_create: these raise before the library is reached
    with pytest.raises(TypeError):
        r.denoise_variance(passes=3)
    with pytest.raises(TypeError):
        r.denoise_variance(sigma=2.0)
    with pytest.raises(TypeError):
        r.denoise_variance(params={"iterations": 3})
    with pytest.raises(TypeError):
        r.denoise_variance(variance={"sigma_l": 3})
    with pytest.raises(TypeError):
        r.denoise_variance(variance=abi.default_denoise_params())
    for bad in ("variance", "", 2, -1, 0.5, None, True):
        with pytest.raises(ValueError):
            r.read_variance(bad)
        with pytest.raises(ValueError):
            r.variance_device_ptr(bad)
    with pytest.raises(TypeError):
        abi.default_variance_params(radius=2)
    img = np.zeros((4, 5, 4), np.float32)
    with pytest.raises(ValueError):
        r.denoise_variance_images(img, img, img, np.zeros((4, 6, 4), np.float32))
    with pytest.raises(ValueError):
        r.denoise_variance_images(img[..., :3], img[..., :3], img[..., :3], img[..., :3])
    with pytest.raises(TypeError):
        r.denoise_variance_images(img, img, img, img, window=2)


def test_cli_rejects_bad_variance_guided_arguments():
    """rmr_cli --variance-guided [SIGMA_L]: needs --denoise; not with the device group, --resume or
    --per-sample; SIGMA_L finite and > 0. All rejected with status 2 before any device is touched."""
    def rc(*args):
        return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=60).returncode
    assert rc("--variance-guided") == 2
    assert rc("--variance-guided", "2") == 2
    assert rc("--denoise", "--variance-guided", "--gpus", "2") == 2
    assert rc("--denoise", "--variance-guided", "--devices", "0,1") == 2
    assert rc("--denoise", "--variance-guided", "--resume", "x.acc") == 2
    assert rc("--denoise", "--variance-guided", "--per-sample") == 2
    for bad in ("0", "-1", "nan", "inf", "-inf", "1e60", "1e-60", "four", "2x", ""):
        assert rc("--denoise", "--variance-guided", bad) == 2, bad
    # valid forms parse: --print-tiles answers without a device
    assert rc("--denoise", "--variance-guided", "--print-tiles", "--grid", "1x1") == 0
    assert rc("--denoise", "3", "--variance-guided", "2.5", "--print-tiles", "--grid", "1x1") == 0
    assert rc("--variance-guided", "1e-3", "--denoise", "--adaptive", "0.5", "--samples", "16", "--print-tiles", "--grid", "1x1") == 0
    help_text = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--variance-guided [SIGMA_L]" in help_text and "_variance.pfm" in help_text


def test_variance_kernels_need_no_scratch(tmp_path):
    """rmr_denoise_var.hip for gfx950 with the compiler's resource remarks: the seed kernel, the plain
    pass and the two tiled passes have no scratch; the seed's LDS is its 40x16 tile of 8 bytes."""
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-slp-vectorize",
           "-Wno-pass-failed", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
           os.path.join(CSRC, "rmr_denoise_var.hip"), "-o", str(tmp_path / "rmr_denoise_var.o")]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-4000:]
    res, name = {}, None
    for line in p.stdout.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
        m = re.search(r"(ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|VGPRs|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            res[name][m.group(1).split(" [")[0]] = int(m.group(2))
    print(res)
    assert len(res) == 4, sorted(res)
    for key in ("k_variance_seed", "k_atrous_varE", "k_atrous_var_ldsILi1E", "k_atrous_var_ldsILi2E"):
        hits = [k for k in res if key in k]
        assert len(hits) == 1, (key, sorted(res))
        assert res[hits[0]]["ScratchSize"] == 0, hits[0]
    lds = {k: v["LDS Size"] for k, v in res.items()}
    assert sorted(lds.values()) == [0, 40 * 16 * 8, 36 * 12 * 48, 40 * 16 * 48]
