"""The bloom stage (rmr_bloom) without a GPU: the parameter ranges and sizes, the host
function rmr_bloom_pixels, which runs the header the kernels compile (csrc/rmr_bloom_rule.h), against the
NumPy statement tests/bloom_ref.py bit for bit and within a derived bound of its float64 form, the rule's
properties on the float64 form, the stand-alone program csrc/bloom_test.cpp plain and under the
sanitizers, and the resources of the kernels compiled for gfx950 (not run)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from raymarchrenderer_amd import abi, bloom_pixels, check_bloom_params, lib
from raymarchrenderer_amd._lib import RMRError

from .conftest import ROOT
from . import bloom_ref as ref

CSRC = os.path.join(ROOT, "raymarchrenderer_amd", "csrc")
CLI = os.path.join(ROOT, "raymarchrenderer_amd", "rmr_cli")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
F = np.float32
NAN, INF = float("nan"), float("inf")
SIZES = [(1, 1), (2, 3), (44, 36), (77, 131)]
LEVELS = [1, 2, 5, 8]


def same_bits(a, b):
    """Equal bit for bit; two NaNs count as equal (0 * inf is born with a different sign on the two
    machines, and an overflowed sum times scatter or intensity 0 is such a product)."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def bloom_image(W, H, seed, huge=False):
    """Log-uniform noise over 2^-12 .. 2^6 (about a third of the pixels above the default threshold) with
    the rule's special pixels sprinkled in, in this order while there is room: alpha 0, NaN, +inf and -inf
    channels, negative channels, a -0 pixel, a 1e4 firefly and 1e-40 values. huge: also channels of 1e38 and
    of FLT_MAX (their L stays finite, the weights summing to 1, so they pass the rule's test of L and make
    the pyramid's sums overflow instead)."""
    rng = np.random.default_rng(seed)
    img = np.exp2(rng.uniform(-12.0, 6.0, (H, W, 4))).astype(F)
    img[..., 3] = 1.0
    flat = img.reshape(-1, 4)
    n = len(flat)
    specials = [[3.0, 2.0, 1.0, 0.0], [NAN, 2.0, 1.0, 1.0], [2.0, INF, 1.0, 1.0], [2.0, 1.0, -INF, 1.0],
                [-5.0, 4.0, -0.5, 1.0], [-3.0, -2.0, -1.0, 1.0], [-0.0, -0.0, -0.0, 1.0], [1e4, 1e4, 1e4, 1.0],
                [1e-40, 2.0, 1e-40, 1.0], [1e-40, 1e-40, 1e-40, 0.5], [0.0, 3.0, -0.0, NAN]]
    if huge:
        fmax = float(np.finfo(F).max)
        specials = [[1e38, 1e38, 1e38, 1.0], [fmax, fmax, fmax, 1.0], [1e38, 0.0, 0.0, 1.0]] + specials
    if n >= 4:
        reps = max(1, n // 400)
        where = rng.permutation(n)[:min(n - 1, reps * len(specials))]
        for k, i in enumerate(where):
            flat[i] = specials[k % len(specials)]
    return img


def params_cases():
    """(levels, then the other fields): every level count with the defaults, and at N = 5 clamp on, scatter
    0 and 1, intensity 0, threshold 0."""
    cases = [dict(levels=n) for n in LEVELS]
    cases += [dict(levels=5, clamp=0.75), dict(levels=5, scatter=0.0), dict(levels=5, scatter=1.0),
              dict(levels=5, intensity=0.0), dict(levels=8, threshold=0.0, intensity=1.5, clamp=3.0)]
    return cases


# ---- defaults, ranges and sizes ------------------------------------------------------------------------
def test_default_and_checked_params():
    p = abi.BloomParams()
    lib().rmr_default_bloom_params(p)
    q = abi.default_bloom_params()
    for name in abi.BLOOM_FIELDS:
        assert getattr(p, name) == getattr(q, name), name
    assert (p.levels, p.threshold, p.clamp, p.scatter, p.intensity) == (5, 1.0, 0.0, F(0.7), F(0.2))
    assert list(p.reserved) == [0, 0, 0]
    assert check_bloom_params()
    for good in ({"levels": 1}, {"levels": 8}, {"threshold": 0.0}, {"threshold": 3e38}, {"clamp": 0.0}, {"clamp": 3e38},
                 {"scatter": 0.0}, {"scatter": 1.0}, {"intensity": 0.0}, {"intensity": 3e38}):
        assert check_bloom_params(**good), good
    bad = [{"levels": 0}, {"levels": 9}, {"levels": -1},
           {"threshold": -1e-6}, {"threshold": NAN}, {"threshold": INF}, {"threshold": -INF},
           {"clamp": -1e-6}, {"clamp": NAN}, {"clamp": INF},
           {"scatter": -1e-6}, {"scatter": 1.0001}, {"scatter": NAN}, {"scatter": INF},
           {"intensity": -1e-6}, {"intensity": NAN}, {"intensity": INF}]
    for fields in bad:
        assert not check_bloom_params(**fields), fields
    for k in range(3):
        p = abi.default_bloom_params()
        p.reserved[k] = 1
        assert not check_bloom_params(p), k
    assert lib().rmr_check_bloom_params(None) == -1
    with pytest.raises(TypeError):
        abi.default_bloom_params(radius=2.0)
    one = np.ones((1, 1, 4), F)
    with pytest.raises(RMRError):
        bloom_pixels(one, levels=9)
    with pytest.raises(RMRError):
        bloom_pixels(one, scatter=NAN)


def test_sizes():
    assert C.sizeof(abi.BloomParams) == 32
    assert [f[0] for f in abi.BloomParams._fields_][:5] == list(abi.BLOOM_FIELDS)
    assert abi.OUTPUT_BLOOM == 4 and abi.OUTPUT_SOURCES["bloom"] == 4
    sizes = (C.c_int32 * 16)()
    assert lib().rmr_abi_sizes(sizes, 16) == 8   # (unchanged: the new struct's size is a static_assert in the library)
    for name in ("rmr_bloom", "rmr_read_bloom", "rmr_bloom_device_ptr", "rmr_bloom_pixels"):
        assert hasattr(lib(), name), name
    assert ref.level_sizes(131, 77, 8) == [(131, 77), (66, 39), (33, 20), (17, 10), (9, 5), (5, 3), (3, 2), (2, 1), (1, 1)]


# ---- the host function against the float32 statement -----------------------------------------------------
@pytest.mark.parametrize("W,H", SIZES, ids=lambda v: str(v))
def test_host_function_is_the_float32_statement_bit_for_bit(W, H):
    for huge in (False, True):
        img = bloom_image(W, H, 100 * W + H, huge=huge)
        before = img.copy()
        for fields in params_cases():
            got = bloom_pixels(img, **fields)
            want = ref.bloom_f32(img, **fields)
            same = same_bits(got, want)
            assert same.all(), (huge, fields, np.argwhere(~same)[:4])
            if not huge:
                assert not np.isnan(got[~np.isnan(img)]).any()
            bad = ref.invalid(img)
            assert np.array_equal(got.view(np.uint32)[bad], img.view(np.uint32)[bad])            # copied bit for bit
            assert np.array_equal(got.view(np.uint32)[..., 3], img.view(np.uint32)[..., 3])
        assert img.tobytes() == before.tobytes()


def test_no_result_depends_on_a_zeros_sign():
    """max(c, 0) is `c > 0 ? c : +0`: an image and its copy with every zero's sign flipped give the same
    spread part (the copies and the final sum S + gain G keep S's own zero where G is 0)."""
    img = bloom_image(44, 36, 5)
    img[::3, ::2, 1] = 0.0
    flipped = img.copy()
    z = flipped[..., :3] == 0
    flipped[..., :3][z] = -flipped[..., :3][z]
    assert (np.signbit(flipped[..., :3][z]) != np.signbit(img[..., :3][z])).all()
    a, b = bloom_pixels(img, threshold=0.0), bloom_pixels(flipped, threshold=0.0)
    moved = (a[..., :3] != img[..., :3]) & ~np.isnan(a[..., :3])
    assert same_bits(a[..., :3][moved], b[..., :3][moved]).all() and moved.any()
    assert np.array_equal(a[..., :3] == 0, b[..., :3] == 0)
    assert same_bits(b, ref.bloom_f32(flipped, threshold=0.0)).all()


# ---- the float64 bound -----------------------------------------------------------------------------------
def f64_bound(img, out64, fields):
    """Per value: u ((12 N + 10) gain G_c + |out|) 1.001, u = 2^-24, G_c = the spread part of the image itself
    (threshold 0, no clamp). See test_host_function_stays_within_the_float64_bound."""
    N = fields.get("levels", 5)
    rest = {k: v for k, v in fields.items() if k not in ("threshold", "clamp")}
    full = ref.bloom_f64(img, threshold=0.0, clamp=0.0, **rest)
    gGc = full[..., :3] - img[..., :3].astype(np.float64)
    return 2.0 ** -24 * ((12 * N + 10) * gGc + np.abs(out64[..., :3])) * 1.001


@pytest.mark.parametrize("W,H", [(44, 36), (77, 131)], ids=lambda v: str(v))
def test_host_function_stays_within_the_float64_bound(W, H):
    """The float32 result against the float64 statement, on images without invalid pixels, denormals and
    overflow (normal floats: every rounding is relative, u = 2^-24).

    Every term of the pyramid is >= 0, so relative errors do not grow through the sums: a sum's error is the
    larger of its terms' plus u. Counting roundings along the longest path to one output value:
      P: L takes 3 products and 2 sums (<= 4 u relative, no cancellation); e = L - T cancels: its absolute
         error is <= 4 u L + u e; f = e / L and P = c f add u each: |dP| <= c (4 u + u f + 6 u f) <= 9 u c
         (f <= 1; the clamp and the test e > 0 are continuous in e). The error is relative to c, not to P,
         hence G_c, the spread part of c itself, in the bound.
      a down along one axis: a sum, the product by 3 and a sum (the product by 0.125 is exact): 3 u, 6 u in
         two dimensions, 6 N u for N levels;
      an up along one axis: the product by 3 and a sum: 2 u, 4 u in two dimensions; U_k = B_k + s up: 2 u more;
         N - 1 such steps: 6 (N - 1) u; the last up: 4 u;
      gain: its own rounding to float and the product gain G: 2 u;
      the final sum S + gain G: u |out|.
    In all (9 + 6 N + 6 (N - 1) + 4 + 2) u = (12 N + 9) u of gain G_c, taken as 12 N + 10, plus u |out|; the
    factor 1.001 covers the second-order terms ((1 + u)^106 - 1 = 106 u (1 + 3e-6))."""
    rng = np.random.default_rng(7 * W + H)
    img = np.exp2(rng.uniform(-12.0, 6.0, (H, W, 4))).astype(F)
    img[..., 3] = 1.0
    img[H // 2, W // 3, :3] = 1e4
    img[::5, ::7, 0] = -1.0
    worst = 0.0
    for fields in params_cases():
        got = bloom_pixels(img, **fields).astype(np.float64)
        want = ref.bloom_f64(img, **fields)
        bound = f64_bound(img, want, fields)
        err = np.abs(got[..., :3] - want[..., :3])
        ratio = float((err / bound).max())
        worst = max(worst, ratio)
        print(fields, "max error / bound = %.4f" % ratio)
        assert (err <= bound).all(), (fields, ratio)
        assert np.array_equal(got[..., 3], want[..., 3])
    print("worst error / bound: %.4f" % worst)


# ---- the rule's properties, on the float64 statement -------------------------------------------------------
def test_constant_image_gets_c_plus_intensity_c():
    for W, H in ((1, 1), (2, 3), (9, 7), (64, 96)):
        img = np.empty((H, W, 4), F)
        img[...] = [0.3, 1.7, 0.05, 1.0]
        for inten in (0.2, 1.0):
            out = ref.bloom_f64(img, levels=1, threshold=0.0, intensity=inten)
            c = img[..., :3].astype(np.float64)
            assert np.allclose(out[..., :3], c + float(F(inten)) * c, rtol=1e-14, atol=0.0)


def test_unit_impulse_keeps_its_sum():
    W, H = 64, 96
    img = np.zeros((H, W, 4), F)
    img[..., 3] = 1.0
    img[H // 2, W // 2, :3] = 1.0
    for N in (1, 3, 5):
        G = ref.spread(img, N, 0.0, 0.0, 0.7, np.float64)
        want = sum(float(F(0.7)) ** j for j in range(N))
        for k in range(3):
            assert abs(G[..., k].sum() - want) <= 1e-12, (N, k, G[..., k].sum(), want)


def test_image_at_or_below_the_threshold_comes_back():
    img = bloom_image(44, 36, 11)
    rgb = img[..., :3]
    rgb[np.isfinite(rgb) & (rgb > 0.5)] = 0.5
    img[3, 4] = [4.0, 0.0, 0.0, 1.0]    # L == T exactly (4 x 0.2126f, in float32 and in float64): e = 0 is not > 0
    T = float(F(4.0) * F(0.2126))
    assert T > 0.5
    assert float(ref.bright(img, T, 0.0, np.float64).max()) == 0.0
    for out in (ref.bloom_f64(img, threshold=T), bloom_pixels(img, threshold=T).astype(np.float64)):
        ok = ~np.isnan(img)
        assert (out[ok] == img[ok].astype(np.float64)).all()
    got = bloom_pixels(img, threshold=T)
    bad = ref.invalid(img)
    assert np.array_equal(got.view(np.uint32)[bad], img.view(np.uint32)[bad]) and bad.any()


def test_clamped_firefly_spreads_like_a_pixel_at_the_clamp():
    W, H, T, cl = 64, 96, 1.0, 2.0
    fire = np.zeros((H, W, 4), F)
    fire[..., 3] = 1.0
    fire[H // 2, W // 2, :3] = 1e4
    mild = fire.copy()
    mild[H // 2, W // 2, :3] = T + cl       # a grey pixel whose e is the clamp
    a = ref.spread(fire, 5, T, cl, 0.7, np.float64).sum()
    b = ref.spread(mild, 5, T, 0.0, 0.7, np.float64).sum()
    free = ref.spread(fire, 5, T, 0.0, 0.7, np.float64).sum()
    assert abs(a - b) <= 1e-6 * b and free > 1000 * a   # (L of a grey pixel is its value to 2^-24: the float32 weights)


def test_result_is_linear_in_intensity():
    img = bloom_image(44, 36, 13)
    ok = ~ref.invalid(img)
    S = np.where(ok[..., None], img[..., :3], 0.0).astype(np.float64)
    d1 = (ref.bloom_f64(img, intensity=0.25)[..., :3] - S)[ok]
    d2 = (ref.bloom_f64(img, intensity=0.5)[..., :3] - S)[ok]
    d4 = (ref.bloom_f64(img, intensity=1.0)[..., :3] - S)[ok]
    assert d1.max() > 0
    tol = 1e-14 * (np.abs(S[ok]) + d4)   # (the differences carry the sums' own roundings, 2^-53 of S + gain G each)
    assert (np.abs(d2 - 2 * d1) <= tol).all() and (np.abs(d4 - 4 * d1) <= tol).all()
    assert (ref.bloom_f64(img, intensity=0.0)[..., :3][ok] == S[ok]).all()


# ---- the stand-alone host program ----------------------------------------------------------------------
def _run_standalone(target):
    """csrc/bloom_test.cpp (its own main, bloom.cpp alone: no HIP, no Python in the program)."""
    subprocess.run(["make", "-s", "-C", CSRC, target], check=True, timeout=600)
    p = subprocess.run([os.path.join(CSRC, "build", target)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:]
    assert "bloom_test ok" in p.stdout, p.stdout[-4000:]
    for word in ("Sanitizer", "runtime error"):
        assert word not in p.stdout, p.stdout[-4000:]


def test_bloom_host_checks():
    _run_standalone("bloom_test")


def test_bloom_host_checks_sanitized(tmp_path):
    from .test_accel_cpu import _sanitizers_work
    if not _sanitizers_work(str(tmp_path)):
        pytest.skip("a one-line program does not build or start under -fsanitize=address,undefined")
    _run_standalone("bloom_test_san")


def test_bloom_cpp_has_no_hip():
    for name in ("bloom.cpp", "bloom.hpp", "bloom_test.cpp", "rmr_bloom_rule.h"):
        text = open(os.path.join(CSRC, name)).read()
        assert "#include <hip" not in text and "__global__" not in text, name


# ---- the kernels' resources ----------------------------------------------------------------------------
def test_bloom_kernels_need_no_scratch(tmp_path):
    """rmr_bloom.hip for gfx950 with the compiler's resource remarks: the five kernels have no scratch and no
    dynamic stack; the down kernels' LDS is the 18 staged rows of 32 float4, the tail's its 12288 pixels of
    12 B, and the up and compose kernels use none."""
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-slp-vectorize",
           "-Wno-pass-failed", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
           os.path.join(CSRC, "rmr_bloom.hip"), "-o", str(tmp_path / "rmr_bloom.o")]
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
        m = re.search(r"Dynamic Stack: (\w+)", line)
        if m and name:
            res[name]["Dynamic Stack"] = m.group(1)
    print(res)
    assert len(res) == 5, sorted(res)
    lds = {"k_bloom_down0": 18 * 32 * 16, "k_bloom_downE": 18 * 32 * 16, "k_bloom_up": 0, "k_bloom_compose": 0,
           "k_bloom_tail": 12288 * 12}
    for key, want in lds.items():
        hits = [k for k in res if key in k]
        assert len(hits) == 1, (key, sorted(res))
        assert res[hits[0]]["ScratchSize"] == 0, hits[0]
        assert res[hits[0]]["Dynamic Stack"] == "False", hits[0]
        assert res[hits[0]]["LDS Size"] == want, (hits[0], res[hits[0]])


# ---- rmr_cli ------------------------------------------------------------------------------------------------
def test_cli_help_and_usage_errors():
    help_text = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--bloom" in help_text

    def rc(*args):
        return subprocess.run([CLI, "--size", "8x8"] + list(args), capture_output=True, text=True,
                              timeout=60).returncode
    for bad in (("--bloom", "foo"), ("--bloom", "-1"), ("--bloom", "nan"), ("--bloom", "1:"), ("--bloom", "1:-0.5"),
                ("--bloom", "1:inf"), ("--bloom", "0.5:0.3:2"), ("--bloom", "1x")):
        assert rc(*bad) == 2, bad
    for good in (("--bloom",), ("--bloom", "0.5"), ("--bloom", "0.5:0.3", "--tonemap", "aces"),
                 ("--bloom", "--denoise", "3", "--exposure", "auto")):
        assert rc(*good, "--print-tiles", "--grid", "1x1") == 0, good
