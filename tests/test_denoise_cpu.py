"""The preview denoiser's definition (tests/denoise_ref.py) and its host-side pieces, without a GPU:
the reference filter reduces the error of few-sample oracle renders, keeps what it must keep, and the
C ABI's parameter defaults, PFM writer and Python argument checks behave as include/rmr.h says."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle import oracle, scene_compile
from raymarchrenderer_amd import Renderer, abi, encode_pfm, parity_schedule
from raymarchrenderer_amd._lib import lib

from .conftest import GOLDEN, ROOT, SCENES
from .denoise_ref import denoise_ref, live_mask, oracle_guides

ERR_CASES = {
    "rm1_cornell5_b4": (os.path.join(SCENES, "cornell5.scene"), {"max_bounces": 4}),
    "rm1_default": (os.path.join(GOLDEN, "scenes", "default.scene"), {}),
    "rm1_csg64_b4": (os.path.join(SCENES, "csg64.scene"), {"max_bounces": 4}),
}


def mse(a, b):
    """Mean squared error over linear RGB clamped to [0, 1] (test_gpu_reference_psnr.psnr's measure)."""
    a = np.clip(a[..., :3].astype(np.float64), 0, 1)
    b = np.clip(b[..., :3].astype(np.float64), 0, 1)
    return float(np.mean((a - b) ** 2))


@pytest.mark.parametrize("name", sorted(ERR_CASES))
def test_reference_filter_halves_error(name):
    """4 and 16 spp oracle renders at the goldens' 64x48 view, three iterations, colour term off: the
    filtered image's MSE against the converged golden is at most half the noisy image's."""
    path, kw = ERR_CASES[name]
    g = np.load(os.path.join(GOLDEN, "img_%s.npz" % name))
    conv, view = g["conv"], g["view"]
    H, W = conv.shape[:2]
    assert (W, H) == (64, 48)
    tables = scene_compile.load_scene_file(path, "rm1")
    prm = abi.default_params(**kw)
    hit, nrm = oracle_guides(tables, prm, view, W, H)
    times = parity_schedule(16)
    orc = oracle.Oracle(tables, prm, view, W, H)
    acc = orc.render(times[:4])
    for spp in (4, 16):
        if spp == 16:
            acc = orc.render(times[4:], first_sample=4, accum=acc)
        den = denoise_ref(acc, hit, nrm, iterations=3, sigma_c=0.0)
        e0, e1 = mse(acc, conv), mse(den, conv)
        print("%s @%d spp: MSE %.4g -> %.4g (%.1fx)" % (name, spp, e0, e1, e0 / max(e1, 1e-30)))
        assert e1 <= 0.5 * e0


def _flat_guides(H, W, ids):
    """A plane z = 5 facing the camera: constant normal, positions on the plane, t = 5."""
    hit = np.zeros((H, W, 4), np.float32)
    hit[..., 0] = np.arange(W)[None, :] * 0.01
    hit[..., 1] = np.arange(H)[:, None] * 0.01
    hit[..., 2] = 5.0
    hit[..., 3] = 5.0
    nrm = np.zeros((H, W, 4), np.float32)
    nrm[..., 2] = -1.0
    nrm[..., 3] = ids
    return hit, nrm


def test_constant_image_stays_constant():
    H, W = 19, 23
    hit, nrm = _flat_guides(H, W, 2.0)
    acc = np.empty((H, W, 4), np.float32)
    acc[...] = (0.3, 0.7, 1.9, 1.0)
    for sc in (0.0, 0.5):
        out = denoise_ref(acc, hit, nrm, iterations=5, sigma_c=sc)
        assert np.abs(out - acc.astype(np.float64)).max() <= 1e-12


def test_two_ids_do_not_mix():
    H, W = 16, 24
    ids = np.where(np.arange(W)[None, :] < 11, 1.0, 4.0) * np.ones((H, 1))
    hit, nrm = _flat_guides(H, W, ids)
    rng = np.random.default_rng(7)
    acc = np.ones((H, W, 4), np.float32)
    acc[..., :3] = np.where(ids[..., None] == 1.0, 0.2, 0.8) + rng.uniform(-0.05, 0.05, (H, W, 3))
    out = denoise_ref(acc, hit, nrm, iterations=4)
    left, right = out[:, :11, :3], out[:, 11:, :3]
    # each side stays within its own input range: nothing of the other side's level leaks in
    assert left.max() <= acc[:, :11, :3].max() + 1e-12 and right.min() >= acc[:, 11:, :3].min() - 1e-12
    assert left.max() < 0.3 and right.min() > 0.7
    # and each side was smoothed (its spread shrank)
    assert left.std() < 0.5 * acc[:, :11, :3].std() and right.std() < 0.5 * acc[:, 11:, :3].std()


def test_non_live_pixels_pass_through_and_do_not_contribute():
    H, W = 12, 14
    hit, nrm = _flat_guides(H, W, 3.0)
    rng = np.random.default_rng(3)
    acc = np.ones((H, W, 4), np.float32)
    acc[..., :3] = rng.uniform(0, 1, (H, W, 3))
    nrm[2, 3] = (0, 0, 0, -1)              # sky
    acc[5, 6] = (0.9, 0.9, 0.9, 0.0)        # not rendered yet
    acc[7, 2, 1] = np.nan                   # NaN pixel
    acc[9, 9, 0] = np.inf
    dead = [(2, 3), (5, 6), (7, 2), (9, 9)]
    assert not live_mask(acc, nrm)[tuple(zip(*dead))].any()
    out = denoise_ref(acc, hit, nrm, iterations=3)
    for y, x in dead:
        assert np.array_equal(out[y, x].astype(np.float32), acc[y, x], equal_nan=True)
    live = live_mask(acc, nrm)
    assert np.isfinite(out[live]).all()
    # a dead pixel's colour changes nothing elsewhere
    acc2 = acc.copy()
    acc2[5, 6, :3] = 1e6
    out2 = denoise_ref(acc2, hit, nrm, iterations=3)
    assert np.array_equal(out2[live], out[live])


def test_default_denoise_params():
    p = abi.DenoiseParams(-1, -1, -1.0, -1.0)
    lib().rmr_default_denoise_params(C.byref(p))
    assert (p.iterations, p.normal_pow2, p.sigma_c) == (5, 5, 0.0)
    assert p.sigma_z == np.float32(0.02)
    q = abi.default_denoise_params()
    assert (q.iterations, q.normal_pow2, q.sigma_z, q.sigma_c) == (p.iterations, p.normal_pow2, p.sigma_z, p.sigma_c)


def test_abi_sizes_ninth_entry_is_denoise_params():
    out = (C.c_int32 * 16)(*([-7] * 16))
    n = lib().rmr_abi_sizes(out, 16)
    assert n == 8 and out[8] == C.sizeof(abi.DenoiseParams) == 16 and out[9] == -7
    out8 = (C.c_int32 * 9)(*([-7] * 9))
    lib().rmr_abi_sizes(out8, 8)
    assert out8[8] == -7   # written only when n >= 9


def test_encode_pfm(tmp_path):
    H, W = 3, 5
    img = np.arange(H * W * 4, dtype=np.float32).reshape(H, W, 4) * np.float32(0.37) - np.float32(3.0)
    img[1, 2, 0] = np.float32(1e-40)   # a denormal survives
    img[0, 0, 3] = np.nan              # alpha is dropped
    path = str(tmp_path / "a.pfm")
    encode_pfm(img, path)
    raw = open(path, "rb").read()
    header = b"PF\n5 3\n-1.0\n"
    assert raw.startswith(header)
    body = raw[len(header):]
    assert len(body) == H * W * 3 * 4
    px = np.frombuffer(body, "<f4").reshape(H, W, 3)
    assert np.array_equal(px[::-1].view(np.uint32), np.ascontiguousarray(img[..., :3]).view(np.uint32))  # bottom row first
    assert struct.unpack("<f", body[:4])[0] == img[H - 1, 0, 0]
    assert lib().rmr_encode_pfm(None, 5, 3, path.encode()) == -1
    with pytest.raises(ValueError):
        encode_pfm(np.zeros((3, 5, 3), np.float32), path)
    with pytest.raises(Exception):
        encode_pfm(img, str(tmp_path / "no_such_dir" / "a.pfm"))


def test_python_argument_errors():
    """The checks that happen before any call into the library (no context needed)."""
    r = Renderer.__new__(Renderer)   # no rmr_create: these raise before the library is reached
    with pytest.raises(TypeError):
        r.denoise(passes=3)
    with pytest.raises(TypeError):
        r.denoise(params={"iterations": 3})
    with pytest.raises(ValueError):
        r.read_guide("albedo")
    with pytest.raises(ValueError):
        r.guide_device_ptr("depth")
    with pytest.raises(ValueError):
        r.set_output_source("filtered")
    with pytest.raises(TypeError):
        abi.default_denoise_params(sigma=1.0)


def test_cli_rejects_bad_denoise_arguments():
    """rmr_cli: --denoise takes 0..8 (the count is optional), --aov needs a prefix, and neither works
    with the device group; all rejected before any device is touched."""
    cli = os.path.join(ROOT, "raymarchrenderer_amd", "rmr_cli")

    def rc(*args):
        return subprocess.run([cli, *args], capture_output=True, text=True, timeout=60).returncode
    assert rc("--denoise", "9") == 2
    assert rc("--denoise", "123") == 2
    assert rc("--aov") == 2
    assert rc("--aov", "") == 2
    assert rc("--gpus", "2", "--denoise") == 2
    assert rc("--gpus", "2", "--aov", "p") == 2
    # a valid count, or none, parses: --print-tiles answers without a device
    assert rc("--denoise", "--print-tiles", "--grid", "1x1") == 0
    assert rc("--denoise", "8", "--print-tiles", "--grid", "1x1") == 0
    help_text = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--denoise [N]" in help_text and "--aov PREFIX" in help_text
