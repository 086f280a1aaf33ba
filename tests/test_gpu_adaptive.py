"""The per-tile error estimate and adaptive sampling on the GPU (include/rmr.h): the
half image and the untouched accumulator bit for bit against the oracle on every launch path, the tile
errors bit for bit against tests/adaptive_ref.py, the adaptive loop's sample counts and pixels against
the CPU simulation (oracle plus reference), the state rules and the CLI."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import camera, oracle
from raymarchrenderer_amd import Renderer, RMRError, abi, default_camera_view, parity_schedule, time_schedule

from .adaptive_ref import oracle_images, simulate, tile_error_ref
from .conftest import ROOT, SCENES
from .test_gpu_denoise import _read_pfm
from .test_gpu_parity import _tables, same_bits

pytestmark = pytest.mark.gpu

CORNELL = os.path.join(SCENES, "cornell5.scene")
CLI = os.path.join(ROOT, "raymarchrenderer_amd", "rmr_cli")
W, H, RECT = 44, 36, (3, 2, 41, 35)
TIMES5 = time_schedule(5, frame=1)
PLANE_BYTES = 6 * 5 * 64 * 16   # the rect's 30 tiles, one sample

HALF_CASES = {   # name: (scene path, variant, params, set_jit mode)
    "cornell5_jit": (CORNELL, "rm1", {"max_bounces": 4}, 1),
    "cornell5_table": (CORNELL, "rm1", {"max_bounces": 4}, 0),
    "rm3_builtin": (None, "rm3", {}, 2),
}
_oracle_cache = {}


def _oracle_ab(name):
    """(A of the rect, B of the rect, A of the whole image, B of the whole image) from the oracle, once per scene."""
    key = name.split("_")[0]
    if key not in _oracle_cache:
        path, variant, kw, _ = HALF_CASES[name]
        orc = oracle.Oracle(_tables(path, variant), abi.default_params(**kw), camera.default_view(W, H), W, H)
        _oracle_cache[key] = (orc.render(TIMES5, rect=RECT), orc.render(TIMES5[1::2], rect=RECT),
                              orc.render(TIMES5), orc.render(TIMES5[1::2]))
    return _oracle_cache[key]


def _context(name):
    path, variant, kw, jit = HALF_CASES[name]
    r = Renderer(0, W, H)
    r.set_jit(jit)
    if path is None:
        r.load_builtin(variant)
    else:
        r.load_scene(path, variant)
    r.set_params(abi.default_params(**kw))
    r.set_view(camera.default_view(W, H))
    return r


def _one(r):
    r.render_spp(TIMES5, RECT)


def _split(r):
    r.render_spp(TIMES5[:3], RECT)
    r.render_spp(TIMES5[3:], RECT, first_sample=3)   # starts at an odd index


def _calls(r):
    r.set_call_batching(1)
    for s in range(5):
        r.render(TIMES5[s], RECT[:2], RECT[2:], s)
    r.sync()
    r.set_call_batching(-1)


def _tiles32(r):
    r.render_tiles(TIMES5, [(0, 0), (1, 0), (0, 1), (1, 1)], 32)   # the whole image


def _budget(r):
    r.set_tuning(samp_budget=3 * PLANE_BYTES)   # 5 samples: launches of 3 and 2
    try:
        before = r.stats().trace_launches
        r.render_spp(TIMES5, RECT)
        assert r.stats().trace_launches - before == 2
    finally:
        r.set_tuning(samp_budget=48 << 30)   # the default (rmr_api.cpp)


PATHS = {"one": _one, "split_3_2": _split, "batched_calls": _calls, "tiles32": _tiles32, "budget_3_2": _budget}


@pytest.mark.parametrize("name", sorted(HALF_CASES))
def test_half_image_and_untouched_accumulator(name):
    a_rect, b_rect, a_full, b_full = _oracle_ab(name)
    r = _context(name)
    try:
        for pname, path in PATHS.items():
            want_a, want_b = (a_full, b_full) if pname == "tiles32" else (a_rect, b_rect)
            r.set_error_estimate(False)
            r.reload()
            path(r)
            off = r.read_accum()
            r.set_error_estimate(True)
            r.reload()
            path(r)
            on, half = r.read_accum(), r.read_half()
            what = "%s %s" % (name, pname)
            assert same_bits(off, want_a).all(), what
            assert same_bits(on, off).all(), what
            assert same_bits(half, want_b).all(), what
            assert (half[..., 3] == want_a[..., 3]).all(), what   # alpha 1 exactly where samples landed
        if name == "cornell5_jit":
            st = r.stats()
            assert st.jit_launches == st.trace_launches > 0
    finally:
        r.close()


def test_tile_error_of_a_render():
    """The state of the first path: bitwise the reference on the GPU's own A and B (which are the
    oracle's), +inf exactly on the tiles that touch the unrendered border."""
    a_rect, b_rect, _, _ = _oracle_ab("cornell5_table")
    r = _context("cornell5_table")
    try:
        r.set_error_estimate(True)
        _one(r)
        A, B = r.read_accum(), r.read_half()
        assert same_bits(A, a_rect).all() and same_bits(B, b_rect).all()
        for offset in (1e-4, 0.5):
            gpu, ref = r.tile_error(offset), tile_error_ref(A, B, offset)
            assert gpu.shape == (5, 6) and same_bits(gpu, ref).all(), offset
        inner = np.zeros((5, 6), bool)
        inner[1:4, 1:5] = True
        assert np.isposinf(gpu[~inner]).all() and np.isfinite(gpu[inner]).all() and (gpu[inner] > 0).all()
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(RMRError) as e:
                r.tile_error(bad)
            assert e.value.code == -1, bad
    finally:
        r.close()


def test_tile_error_images_edge_cases(renderer):
    """20 x 12 (tiles of 8 x 8, 4 x 8, 8 x 4 and 4 x 4), one special pixel per tile."""
    rng = np.random.default_rng(11)
    A = np.ones((12, 20, 4), np.float32)
    A[..., :3] = rng.uniform(0, 2, (12, 20, 3))
    B = A.copy()
    B[..., :3] += rng.normal(0, 0.2, (12, 20, 3)).astype(np.float32)
    A[2, 3, 1] = np.nan                       # tile (0, 0): counted, v = 0
    B[5, 9, 2] = np.inf                       # tile (1, 0)
    B[1, 18, 3] = 0.0                         # tile (2, 0): +inf
    A[9, 4, :3] = (-2.0, 0.5, 0.25)           # tile (0, 1): negative sum
    B[8:, 8:16] = A[8:, 8:16]                 # tile (1, 1): nothing but a denormal difference
    A[10, 12, :3] = (1e-39, 0.0, 0.0)
    B[10, 12, :3] = (0.0, 0.0, 0.0)
    A[11, 17, 0], B[11, 17, 0] = 3e38, -3e38  # tile (2, 1): the difference overflows
    ref = tile_error_ref(A, B, 1e-4)
    gpu = renderer.tile_error_images(A, B, 1e-4)
    print("tile errors: gpu %s ref %s" % (gpu.ravel(), ref.ravel()))
    assert gpu.shape == (2, 3) and same_bits(gpu, ref).all()
    assert np.isposinf(ref[0, 2]) and np.isposinf(ref[1, 2]) and np.isfinite(ref[0, :2]).all()
    # the denormal difference survives: 1e-39 / (1e-4 + sqrt(1e-39)) over the tile's 32 pixels
    assert 2e-37 < ref[1, 1] < 4e-37
    with pytest.raises(RMRError) as e:
        renderer.tile_error_images(A, B, 0.0)
    assert e.value.code == -1
    with pytest.raises(ValueError):
        renderer.tile_error_images(A, B[:8])


_loop_cache = {}


def _loop_images():
    if not _loop_cache:
        prm, view = abi.default_params(max_bounces=4), camera.default_view(W, H)
        times = parity_schedule(32)
        orc = oracle.Oracle(_tables(CORNELL, "rm1"), prm, view, W, H)
        _loop_cache["x"] = (prm, view, times, oracle_images(orc, times))
    return _loop_cache["x"]


@pytest.mark.parametrize("bt", [1, 2])
def test_adaptive_loop_matches_simulation(bt):
    prm, view, times, images = _loop_images()
    thr = np.float32(0.6)
    sim = simulate(images, W, H, thr, min_samples=4, pass_samples=4, max_samples=32, block_tiles=bt)
    counts = sim["counts"]
    hist = {int(c): int((counts == c).sum()) for c in np.unique(counts)}
    print("block_tiles %d: counts %s, passes %d, open %d, max error %.4g" % (bt, hist, sim["passes"], sim["tiles_open"], sim["max_error"]))
    assert len(hist) >= 3 and hist.get(4, 0) >= 0.1 * counts.size and hist.get(32, 0) >= 0.1 * counts.size
    r = Renderer(0, W, H)
    try:
        r.load_scene(CORNELL, "rm1")
        r.set_params(prm)
        r.set_view(view)
        res = r.render_adaptive(times, threshold=thr, min_samples=4, pass_samples=4, block_tiles=bt)
        got, acc = r.sample_counts(), r.read_accum()
        err = r.tile_error()
    finally:
        r.close()
    assert got.dtype == np.uint32 and np.array_equal(got, counts)
    per_pixel = np.repeat(np.repeat(counts, 8, 0), 8, 1)[:H, :W]
    for c in hist:
        m = per_pixel == c
        assert same_bits(acc[m], images(c)[0][m]).all(), c
    assert same_bits(err, sim["errors"]).all()
    assert (res.samples, res.tiles_open, res.passes) == (sim["samples"], sim["tiles_open"], sim["passes"])
    assert same_bits(np.float32(res.max_error), sim["max_error"]).all()


def test_state_rules():
    r = Renderer(0, W, H)
    try:
        r.load_scene(CORNELL, "rm1")
        r.set_params(abi.default_params(max_bounces=2))
        r.set_view(camera.default_view(W, H))

        def state_error(call):
            with pytest.raises(RMRError) as e:
                call()
            assert e.value.code == -5
        state_error(r.tile_error)                    # before the estimate is enabled
        state_error(r.read_half)
        state_error(r.sample_counts)
        assert r.half_device_ptr() is None
        r.set_error_estimate(True)
        assert r.half_device_ptr()
        r.render_spp(TIMES5[:2])
        assert np.isfinite(r.tile_error()).all()
        a = r.read_accum()
        r.write_accum(a)                             # invalid after write_accum
        state_error(r.tile_error)
        r.reload()                                   # the setting survives, and B is zero again
        assert (r.read_half() == 0).all()
        r.render_spp(TIMES5[:2])
        assert np.isfinite(r.tile_error()).all() and (r.read_half()[..., 3] == 1).all()
        r.set_error_estimate(False)                  # switched off: invalid
        state_error(r.tile_error)
        r.set_error_estimate(True)                   # enabled after a render: not valid
        state_error(r.tile_error)
        # render_adaptive on a used accumulator, and with bad parameters
        state_error(lambda: r.render_adaptive(TIMES5, min_samples=2, pass_samples=1))
        r.reload()
        for bad in ({"threshold": float("nan")}, {"offset": 0.0}, {"min_samples": 1}, {"max_samples": 3, "min_samples": 4},
                    {"block_tiles": 0}, {"block_tiles": 9}):
            with pytest.raises(RMRError) as e:
                r.render_adaptive(TIMES5, **dict({"min_samples": 2, "pass_samples": 1}, **bad))
            assert e.value.code == -1, bad
        # threshold 0: only a block whose two means agree exactly closes, the rest run to the maximum
        res = r.render_adaptive(TIMES5, min_samples=2, pass_samples=1, threshold=0.0, block_tiles=1)
        counts = r.sample_counts()
        pixels = np.outer(np.minimum(8, H - 8 * np.arange(5)), np.minimum(8, W - 8 * np.arange(6)))
        assert res.passes == 4 and counts.max() == 5 and counts.min() >= 2
        assert res.samples == int((counts.astype(np.int64) * pixels).sum())
        assert res.tiles_open == int((r.tile_error() > 0).sum())
        state_error(lambda: r.render_adaptive(TIMES5, min_samples=2, pass_samples=1))   # no continuing
        r.reload()
        state_error(r.sample_counts)                 # a reload forgets the counts
    finally:
        r.close()


def test_adaptive_on_caller_stream_and_bound_accumulator():
    import torch
    prm, view, times, images = _loop_images()
    sim = simulate(images, W, H, np.float32(0.6), min_samples=4, pass_samples=4, max_samples=32, block_tiles=2)
    r = Renderer(0, W, H)
    try:
        r.load_scene(CORNELL, "rm1")
        r.set_params(prm)
        r.set_view(view)
        s = torch.cuda.Stream()
        acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        r.set_stream(s.cuda_stream)
        r.bind_accum(acc.data_ptr(), acc.numel() * 4)
        res = r.render_adaptive(times, threshold=np.float32(0.6), min_samples=4, pass_samples=4, block_tiles=2)
        counts = r.sample_counts()
        s.synchronize()
        host = acc.cpu().numpy()
    finally:
        r.close()
    assert np.array_equal(counts, sim["counts"]) and res.samples == sim["samples"]
    assert same_bits(host, sim["image"]).all()


def test_cli_adaptive(tmp_path):
    """rmr_cli --adaptive at 64 x 48: the BMP and the two PFMs, and the summary line of
    Renderer.render_adaptive on the same inputs."""
    w, h = 64, 48
    out, prefix = str(tmp_path / "cli.bmp"), str(tmp_path / "aov")
    p = subprocess.run([CLI, "--scene", CORNELL, "--variant", "rm1", "--size", "%dx%d" % (w, h), "--samples", "16",
                        "--bounces", "3", "--adaptive", "0.5", "--min-samples", "4", "--pass-samples", "4",
                        "--aov", prefix, "--out", out, "--quiet"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"adaptive: passes (\d+), mean spp ([0-9.]+), open tiles (\d+), max error (\S+)", p.stdout)
    assert m, p.stdout
    r = Renderer(0, w, h)
    try:
        r.load_scene(CORNELL, "rm1")
        r.set_params(abi.default_params(max_bounces=3))
        r.set_view(default_camera_view(w, h))
        res = r.render_adaptive(time_schedule(16), threshold=0.5, min_samples=4, pass_samples=4)
        counts, err = r.sample_counts(), r.tile_error()
        want = str(tmp_path / "want.bmp")
        r.save_bmp(want)
    finally:
        r.close()
    assert 1 < len(np.unique(counts))
    assert (int(m.group(1)), int(m.group(3))) == (res.passes, res.tiles_open)
    assert m.group(2) == "%.3f" % (res.samples / float(w * h)) and m.group(4) == "%.6g" % res.max_error
    assert open(out, "rb").read() == open(want, "rb").read()
    spp, ep = _read_pfm(prefix + "_spp.pfm"), _read_pfm(prefix + "_error.pfm")
    assert np.array_equal(spp[..., 0], np.repeat(np.repeat(counts, 8, 0), 8, 1)[:h, :w].astype(np.float32))
    assert same_bits(ep[..., 0], np.repeat(np.repeat(err, 8, 0), 8, 1)[:h, :w]).all()
    assert (spp[..., 1:] == 0).all() and (ep[..., 1:] == 0).all()
