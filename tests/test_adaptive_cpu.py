"""Adaptive sampling without a GPU: the decision rule of the C ABI against its numpy statement, the
parameter defaults and ranges, the two forms of the tile-error reference against each other, and the
whole loop on the oracle (tests/adaptive_ref.py simulate) as a quality gate."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle, scene_compile
from raymarchrenderer_amd import abi, adaptive_select, parity_schedule
from raymarchrenderer_amd._lib import lib

from .adaptive_ref import oracle_images, select_ref, simulate, tile_error_loop, tile_error_ref
from .conftest import GOLDEN, ROOT, SCENES
from .test_denoise_cpu import mse


@pytest.mark.parametrize("bt", [1, 2, 4])
def test_select_matches_numpy_rule(bt):
    """6 x 5 tiles (ragged block edges for 2 and 4), random errors with +inf, 0 and NaN entries, three
    successive calls with other maps: equal to the numpy rule, and a closed block never reopens."""
    TX, TY = 6, 5
    rng = np.random.default_rng(100 + bt)
    open_c = None
    open_n = None
    closed_ever = np.zeros((-(-TY // bt), -(-TX // bt)), bool)
    for call in range(3):
        err = rng.uniform(0.0, 0.4, (TY, TX)).astype(np.float32)
        err[rng.uniform(size=err.shape) < 0.15] = 0.0
        err[rng.uniform(size=err.shape) < 0.1] = np.inf
        if call == 1:
            err[2, 3] = np.nan
        thr = np.float32(0.25)
        open_c = adaptive_select(err, bt, thr, open_c)
        open_n = select_ref(err, bt, thr, open_n)
        assert open_c.shape == open_n.shape and np.array_equal(open_c, open_n), (bt, call)
        assert not (open_c & closed_ever).any()
        closed_ever |= ~open_c
    # every tile's error is the threshold itself: not above it, everything closes; all +inf: all open
    assert not adaptive_select(np.full((TY, TX), 0.25, np.float32), bt, np.float32(0.25)).any()
    assert adaptive_select(np.full((TY, TX), np.inf, np.float32), bt, np.float32(0.25)).all()


def test_select_returns_open_count_and_rejects_bad_arguments():
    L = lib()
    err = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 0.0]], np.float32)
    o = np.ones(3, np.uint8)
    fp, bp = err.ctypes.data_as(C.POINTER(C.c_float)), o.ctypes.data_as(C.POINTER(C.c_uint8))
    assert L.rmr_adaptive_select(fp, 3, 2, 1, 0.5, np.ones(6, np.uint8).ctypes.data_as(C.POINTER(C.c_uint8))) == 1
    assert L.rmr_adaptive_select(fp, 3, 2, 2, 0.5, bp) == 1 and list(o[:2]) == [1, 0]
    for args in ((None, 3, 2, 1, 0.5, bp), (fp, 0, 2, 1, 0.5, bp), (fp, 3, 2, 0, 0.5, bp), (fp, 3, 2, 9, 0.5, bp),
                 (fp, 3, 2, 1, float("nan"), bp), (fp, 3, 2, 1, -1.0, bp), (fp, 3, 2, 1, 0.5, None)):
        assert L.rmr_adaptive_select(*args) == -1, args


def test_default_adaptive_params_field_by_field():
    p = abi.AdaptiveParams(-1.0, -1.0, 99, 99, 99, -1)
    lib().rmr_default_adaptive_params(C.byref(p))
    assert p.threshold == np.float32(0.1) and p.offset == np.float32(1e-4)
    assert (p.min_samples, p.pass_samples, p.max_samples, p.block_tiles) == (16, 16, 0, 2)
    q = abi.default_adaptive_params()
    for name, _ in abi.AdaptiveParams._fields_:
        assert getattr(p, name) == getattr(q, name), name
    # the layout the header declares: 4-byte fields in order; the result's 64-bit count at offset 8
    assert C.sizeof(abi.AdaptiveParams) == 24 and abi.AdaptiveParams.block_tiles.offset == 20
    assert C.sizeof(abi.AdaptiveResult) == 24 and abi.AdaptiveResult.samples.offset == 8
    assert abi.AdaptiveResult.max_error.offset == 16


def test_adaptive_param_ranges():
    check = lib().rmr_check_adaptive_params
    good = abi.default_adaptive_params(max_samples=64)
    assert check(C.byref(good)) == 0
    assert check(C.byref(abi.default_adaptive_params())) == -1   # max_samples has no default
    assert check(None) == -1
    for bad in ({"threshold": float("nan")}, {"threshold": -0.5}, {"threshold": float("inf")}, {"offset": 0.0},
                {"offset": float("nan")}, {"offset": -1.0}, {"min_samples": 1}, {"min_samples": 0},
                {"pass_samples": 0}, {"max_samples": 15}, {"block_tiles": 0}, {"block_tiles": 9}):
        assert check(C.byref(abi.default_adaptive_params(**dict({"max_samples": 64}, **bad)))) == -1, bad
    for ok in ({"threshold": 0.0}, {"min_samples": 2}, {"max_samples": 16}, {"block_tiles": 1}, {"block_tiles": 8}):
        assert check(C.byref(abi.default_adaptive_params(**dict({"max_samples": 64}, **ok)))) == 0, ok
    with pytest.raises(TypeError):
        abi.default_adaptive_params(samples=3)


def test_cli_rejects_bad_adaptive_arguments():
    """rmr_cli: --adaptive needs a finite threshold >= 0 and --samples >= --min-samples >= 2, and is
    refused with the device group, --resume and --per-sample; all before any device is touched."""
    cli = os.path.join(ROOT, "raymarchrenderer_amd", "rmr_cli")

    def rc(*args):
        return subprocess.run([cli, *args], capture_output=True, text=True, timeout=60).returncode
    assert rc("--adaptive") == 2
    assert rc("--adaptive", "x") == 2
    assert rc("--adaptive", "-0.5") == 2
    assert rc("--adaptive", "nan") == 2
    assert rc("--adaptive", "0.1", "--samples", "8") == 2            # below the default --min-samples 16
    assert rc("--adaptive", "0.1", "--min-samples", "1") == 2
    assert rc("--adaptive", "0.1", "--pass-samples", "0") == 2
    assert rc("--adaptive", "0.1", "--gpus", "2") == 2
    assert rc("--adaptive", "0.1", "--devices", "0,1") == 2
    assert rc("--adaptive", "0.1", "--resume", "x.acc") == 2
    assert rc("--adaptive", "0.1", "--per-sample") == 2
    assert rc("--adaptive", "0.1", "--samples", "32", "--min-samples", "8", "--print-tiles", "--grid", "1x1") == 0
    help_text = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--adaptive T" in help_text and "--min-samples N" in help_text and "--pass-samples N" in help_text


CSRC = os.path.join(ROOT, "raymarchrenderer_amd", "csrc")


def _run_standalone(target):
    """csrc/adaptive_test.cpp (its own main, adaptive.cpp alone: no HIP, no Python in the program)."""
    subprocess.run(["make", "-s", "-C", CSRC, target], check=True, timeout=600)
    p = subprocess.run([os.path.join(CSRC, "build", target)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:]
    assert "adaptive_test ok" in p.stdout, p.stdout[-4000:]
    for word in ("Sanitizer", "runtime error"):
        assert word not in p.stdout, p.stdout[-4000:]


def test_adaptive_host_checks():
    _run_standalone("adaptive_test")


def test_adaptive_host_checks_sanitized(tmp_path):
    from .test_accel_cpu import _sanitizers_work
    if not _sanitizers_work(str(tmp_path)):
        pytest.skip("a one-line program does not build or start under -fsanitize=address,undefined")
    _run_standalone("adaptive_test_san")


def _random_pair(H, W, seed):
    rng = np.random.default_rng(seed)
    A = np.ones((H, W, 4), np.float32)
    A[..., :3] = rng.uniform(0, 2, (H, W, 3))
    B = A.copy()
    B[..., :3] += rng.normal(0, 0.2, (H, W, 3)).astype(np.float32)
    return A, B


def test_reference_forms_agree():
    """44 x 36: ragged tiles of 4 x 8 and 8 x 4 (and 4 x 4 in the corner), with an unsampled pixel, a NaN,
    an inf and a negative sum: the vectorised form is bitwise the per-lane loop."""
    A, B = _random_pair(36, 44, 5)
    A[3, 5, 3] = 0.0          # tile (0, 0): +inf
    B[20, 41, 3] = 0.0        # a ragged tile: +inf
    A[10, 10, 1] = np.nan     # counted, v = 0
    B[12, 30, 0] = np.inf
    A[34, 2, :3] = (-1.0, 0.25, 0.5)   # negative sum: sqrt(max(s, 0)) = 0
    v, l = tile_error_ref(A, B, 1e-4), tile_error_loop(A, B, 1e-4)
    assert v.shape == (5, 6) and v.dtype == np.float32
    assert np.array_equal(v.view(np.uint32), l.view(np.uint32))
    assert np.isinf(v[0, 0]) and np.isinf(v[2, 5]) and np.isfinite(v).sum() == 28
    # the NaN pixel's tile: the mean over 64 counted pixels of the 63 others' values
    A2, B2 = A.copy(), B.copy()
    A2[10, 10, :3] = B2[10, 10, :3] = 1.0   # a pixel with zero difference gives the same tile error
    assert tile_error_ref(A2, B2)[1, 1] == v[1, 1]
    assert (v[np.isfinite(v)] > 0).all()


def test_quality_gate_csg64():
    """The whole loop on the oracle: csg64 at the golden's 64 x 48, parity_schedule(64), min 8, pass 8,
    block_tiles 1, threshold = the median positive tile error after the first 8 samples. The adaptive
    image's MSE against the converged golden is below the uniform render's at the multiple of 8 at or
    above the adaptive mean spp."""
    gold = np.load(os.path.join(GOLDEN, "img_rm1_csg64_b4.npz"))
    conv, view = gold["conv"], gold["view"]
    H, W = conv.shape[:2]
    assert (W, H) == (64, 48)
    tables = scene_compile.load_scene_file(os.path.join(SCENES, "csg64.scene"), "rm1")
    orc = oracle.Oracle(tables, abi.default_params(max_bounces=4), view, W, H)
    times = parity_schedule(64)
    images = oracle_images(orc, times)
    e8 = tile_error_ref(*images(8))
    thr = np.float32(np.median(e8[e8 > 0]))
    sim = simulate(images, W, H, thr, min_samples=8, pass_samples=8, max_samples=64, block_tiles=1)
    mean_spp = sim["samples"] / float(W * H)
    uniform_at = int(-(-mean_spp // 8) * 8)
    for c in range(8, uniform_at + 1, 8):   # (in increasing order: the oracle renders incrementally)
        images(c)
    e_adaptive, e_uniform = mse(sim["image"], conv), mse(images(uniform_at)[0], conv)
    hist = {int(c): int((sim["counts"] == c).sum()) for c in np.unique(sim["counts"])}
    print("csg64: threshold %.4g, adaptive %.1f spp MSE %.4g, uniform %d spp MSE %.4g, counts %s, passes %d"
          % (thr, mean_spp, e_adaptive, uniform_at, e_uniform, hist, sim["passes"]))
    assert 8 < mean_spp < 64 and len(hist) >= 3
    assert e_adaptive < e_uniform
