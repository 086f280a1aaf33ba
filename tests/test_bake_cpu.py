"""Light baking (include/rmr.h rmr_bake_points) without a GPU: the host fold bit for bit against
the NumPy statement tests/bake_ref.py (through the library and through the stand-alone program
csrc/bake_test.cpp), the reject rule at its bound, the parameter ranges, the sRGB bytes against the display's
thresholds, the coloured PLY read back, the estimator's directions and cosines from the oracle, the program's
own checks plain and under the sanitizers, the kernels' resources as compiled for gfx950 (not run) and
rmr_cli's argument handling."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from raymarchrenderer_amd import (RMRError, abi, bake_check_points, bake_fold, check_bake_params, encode_ply, lib, srgb8)

from . import bake_ref as ref
from .conftest import ROOT

CSRC = os.path.join(ROOT, "raymarchrenderer_amd", "csrc")
CLI = os.path.join(ROOT, "raymarchrenderer_amd", "rmr_cli")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
F = np.float32


def _build(target):
    subprocess.run(["make", "-s", "-C", CSRC, target], check=True, timeout=600)
    return os.path.join(CSRC, "build", target)


# ---- the fold -------------------------------------------------------------------------------------------------
def _fold_inputs():
    """7 samples of 41 points: ordinary values over several magnitudes; NaN, +inf and -inf radiance samples; a point
    whose every sample is skipped (n_used == 0); points whose cosines are all 0 (sum c == 0); a blocked-everywhere
    and a blocked-nowhere point."""
    rng = np.random.default_rng(17)
    N, n = 7, 41
    L = (rng.uniform(0, 4, (N, n, 3)) * 10.0 ** rng.integers(-3, 4, (N, n, 1))).astype(F)
    c = rng.uniform(0, 1, (N, n)).astype(F)
    c[rng.uniform(size=(N, n)) < 0.2] = 0
    v = rng.uniform(size=(N, n)) < 0.5
    L[1, 3, 0] = np.nan
    L[2, 3, 2] = np.inf
    L[0, 4, 1] = -np.inf
    L[:, 5, 1] = np.nan          # n_used == 0
    c[:, 6] = 0                  # sum c == 0
    c[:, 7] = 0
    L[3, 7] = np.nan
    v[:, 8], v[:, 9] = True, False
    cv = np.where(v, c, F(0.0)).astype(F)
    return L, c, cv


def test_fold_matches_statement(tmp_path):
    L, c, cv = _fold_inputs()
    want_rgba, want_ao = ref.fold(L, c, cv)
    assert want_rgba[5].tolist() == [0, 0, 0, 0] and want_rgba[3, 3] == 5 and want_rgba[4, 3] == 6
    assert want_ao[6] == 1 and want_ao[7] == 1 and want_ao[8] == 1 and want_ao[9] == 0
    assert np.isfinite(want_rgba).all() and ((want_ao >= 0) & (want_ao <= 1)).all()
    rgba, ao = bake_fold(L, c, cv)
    assert rgba.tobytes() == want_rgba.tobytes() and ao.tobytes() == want_ao.tobytes()
    # either output alone
    assert bake_fold(L, c)[0].tobytes() == want_rgba.tobytes() and bake_fold(L, c)[1] is None
    assert bake_fold(None, c, cv)[1].tobytes() == want_ao.tobytes()
    # the stand-alone program's copy of the same function
    src, dst = str(tmp_path / "fold.in"), str(tmp_path / "fold.out")
    with open(src, "wb") as f:
        f.write(struct.pack("<2I", c.shape[1], c.shape[0]))
        f.write(L.tobytes() + c.tobytes() + cv.tobytes())
    p = subprocess.run([_build("bake_test"), "fold", src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=600)
    assert p.returncode == 0 and "bake_test fold ok" in p.stdout, p.stdout[-4000:]
    raw = open(dst, "rb").read()
    assert raw == want_rgba.tobytes() + want_ao.tobytes()
    # the sums are sequential float32 sums: a float64 accumulation rounds to other bits at some of these points
    use = np.isfinite(L).all(axis=2)
    s64 = 2 * np.where(use[..., None], L.astype(np.float64) * c[..., None], 0).sum(axis=0) / np.maximum(use.sum(axis=0), 1)[:, None]
    differ = int((s64.astype(F) != want_rgba[:, :3]).any(axis=1).sum())
    print("%d of %d points: the float32 fold differs from a float64 one" % (differ, L.shape[1]))
    assert differ >= 5
    with pytest.raises(RMRError):
        bake_fold(np.zeros((0, 3, 3), F), np.zeros((0, 3), F))   # nspp == 0


# ---- the reject rule and the parameters -------------------------------------------------------------------------
def test_check_points():
    p = np.zeros((9, 3), F)
    n = np.tile(np.array([0, 1, 0], F), (9, 1))
    assert bake_check_points(p, n) is None and ref.point_ok(p, n).all()
    cases = {1: ("n", [0, np.nan, 0]), 2: ("n", [0, 0, 0]), 3: ("n", [1.000001, 0, 0]), 4: ("n", [0, 0, 0.999999]),
             5: ("p", [np.inf, 0, 0]), 6: ("p", [0, 0, np.nan]), 7: ("n", [np.inf, 0, 0])}
    for i, (what, v) in cases.items():
        q, m = p.copy(), n.copy()
        (q if what == "p" else m)[i] = v
        assert bake_check_points(q, m) == i, (i, what, v)
        assert (~ref.point_ok(q, m)).nonzero()[0].tolist() == [i]
    # 1 +- 2e-6 is outside, 1 +- 4e-7 inside: the bound is 1e-6 (rmr_check_rays' 1e-5 would take both)
    for s, ok in ((1.000001, False), (0.999999, False), (1.0000002, True), (0.9999998, True)):
        m = np.array([[F(s), 0, 0]], F)
        e = abs(float(m[0, 0]) ** 2 - 1.0)
        assert (e <= 1e-6) == ok and e < 1e-5
        assert (bake_check_points(p[:1], m) is None) == ok and bool(ref.point_ok(p[:1], m)[0]) == ok
    assert bake_check_points(np.zeros((0, 3), F), np.zeros((0, 3), F)) is None


def test_check_params():
    assert check_bake_params() and check_bake_params(radiance=True, ao=True, ao_distance=0.5, bias=-0.01)
    d = abi.BakeParams()
    lib().rmr_default_bake_params(d)
    assert (d.flags, d.bias, d.ao_distance, d.first_index) == (abi.BAKE_RADIANCE, F(0.002), np.inf, 0)
    assert not check_bake_params(radiance=False, ao=False)
    assert not check_bake_params(abi.BakeParams(4, 0.002, np.inf, 0.0, 0))
    for bias in (np.nan, np.inf, -np.inf):
        assert not check_bake_params(bias=bias)
    for dist in (np.nan, 0.0, -1.0, -np.inf):
        assert not check_bake_params(ao=True, ao_distance=dist)
    assert check_bake_params(first_index=1 << 36) and not check_bake_params(first_index=(1 << 36) + 1)
    assert not check_bake_params(first_index=1 << 40)


# ---- sRGB bytes and the coloured PLY --------------------------------------------------------------------------
def test_srgb8_matches_the_thresholds():
    thr = np.zeros(256, F)
    assert lib().rmr_srgb_thresholds(thr.ctypes.data_as(C.POINTER(C.c_float))) == 0
    assert (np.diff(thr) > 0).all() and thr[0] == 0
    rng = np.random.default_rng(5)
    x = np.concatenate([thr, np.nextafter(thr, F(-1)), np.nextafter(thr, F(2)), rng.uniform(-0.2, 1.2, 1000).astype(F),
                        np.array([np.nan, np.inf, -np.inf, -0.0, 1.0, 7.0], F)])
    x = np.concatenate([x, np.zeros(-len(x) % 3, F)]).reshape(-1, 3)
    got = srgb8(x)
    want = (x[..., None] >= thr[1:]).sum(axis=-1)     # the number of decision points at or below the value; NaN: 0
    assert got.dtype == np.uint8 and got.shape == x.shape and (got == want).all()
    assert srgb8([[0.0, 0.5, 1.0]]).tolist() == [[0, 188, 255]]
    # against the formula, away from the decision points
    y = rng.uniform(0, 1, (500, 3))
    enc = np.where(y <= 0.0031308, 12.92 * y, 1.055 * y ** (1 / 2.4) - 0.055) * 255
    far = np.abs(enc - np.floor(enc) - 0.5) > 1e-3
    assert (srgb8(y)[far] == np.round(enc)[far]).all()


def test_ply_with_colours(tmp_path):
    from .test_mesh_cpu import _parse_ply
    rng = np.random.default_rng(2)
    v = rng.normal(size=(6, 3)).astype(F)
    n = rng.normal(size=(6, 3)).astype(F)
    ids = np.arange(6, dtype=F)
    col = rng.integers(0, 256, (6, 3)).astype(np.uint8)
    q = np.array([[0, 1, 2, 3], [2, 3, 4, 5]], np.uint32)
    path = str(tmp_path / "c.ply")
    encode_ply(path, v, q, normals=n, ids=ids, colors=col)
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    assert head.decode().splitlines() == [
        "ply", "format binary_little_endian 1.0", "element vertex 6", "property float x", "property float y",
        "property float z", "property float nx", "property float ny", "property float nz", "property float material",
        "property uchar red", "property uchar green", "property uchar blue", "element face 2",
        "property list uchar uint vertex_indices"]
    vert = np.frombuffer(body, np.dtype([("f", "<f4", (7,)), ("c", "u1", (3,))]), 6)
    assert vert["f"][:, :3].tobytes() == v.tobytes() and vert["f"][:, 3:6].tobytes() == n.tobytes()
    assert (vert["f"][:, 6] == ids).all() and (vert["c"] == col).all()
    face = np.frombuffer(body, np.dtype([("n", "u1"), ("i", "<u4", (4,))]), 2, 31 * 6)
    assert len(body) == 31 * 6 + 17 * 2 and (face["n"] == 4).all() and (face["i"] == q).all()
    # bare vertices with colours; and without colours the file is rmr_encode_ply's, byte for byte
    encode_ply(path, v, q, colors=col)
    body = open(path, "rb").read().split(b"end_header\n", 1)[1]
    assert len(body) == 15 * 6 + 17 * 2 and (np.frombuffer(body, np.dtype([("f", "<f4", (3,)), ("c", "u1", (3,))]), 6)["c"] == col).all()
    encode_ply(path, v, q, normals=n, ids=ids)
    props, vert, face = _parse_ply(path)
    assert props == ["x", "y", "z", "nx", "ny", "nz", "material"] and b"red" not in open(path, "rb").read()
    with pytest.raises(ValueError):
        encode_ply(path, v, q, colors=col[:5])
    with pytest.raises(RMRError) as e:
        encode_ply(str(tmp_path / "no" / "such" / "c.ply"), v, q, colors=col)
    assert e.value.code == -4


# ---- the estimator ------------------------------------------------------------------------------------------------
ESTIMATOR_NORMALS = [(0, 1, 0), (0, -1, 0), (0, 0.99999994, 0), (1, 0, 0), (0.6, 0, 0.8), (1, 2, 3)]


@pytest.mark.parametrize("k", range(len(ESTIMATOR_NORMALS)))
def test_directions_and_cosines(k):
    """N = 4096 directions of one point: unit, in the normal's hemisphere, and the cosine's mean is 1/2: the
    cosine over a uniform hemisphere has mean 1/2 and variance 1/12, so (2 / N) sum c has standard deviation
    2 sqrt(1 / (12 N)) = 0.009, and the bound is four of them."""
    N = 4096
    n = np.array(ESTIMATOR_NORMALS[k], np.float64)
    n = (n / np.linalg.norm(n)).astype(F) if k == 5 else n.astype(F)
    p = np.array([[0.37 + k, 1.25 - 0.5 * k, -2.0 + 0.75 * k]], F)
    times = (1000.0 + 0.016 * np.arange(N)).astype(F)
    rays, c, ok = ref.rays(p, n[None], times, first_index=4093 + 5000 * k)
    assert ok.all() and (rays["gx"] >= 0).all()
    d = rays["d"][:, 0].astype(np.float64)
    assert np.abs(np.linalg.norm(d, axis=1) - 1.0).max() <= 1e-6
    assert (c >= 0).all()
    exact = d @ n.astype(np.float64)
    assert np.abs(np.maximum(exact, 0) - c[:, 0]).max() <= 1e-6
    assert (exact >= -1e-6).all()                      # the hemisphere about n (about -y for the ceiling)
    est = 2.0 * c.astype(np.float64).sum() / N
    print("normal %s: (2 / N) sum c = %.5f, min d.n %.2e, %d distinct directions" % (n, est, exact.min(), len(np.unique(d, axis=0))))
    assert abs(est - 1.0) <= 0.036
    assert len(np.unique(d, axis=0)) > N // 2
    # the origin is fma(n, bias, p), the chain is fresh, the invocation is idx & 4095, idx >> 12
    idx = 4093 + 5000 * k
    assert (rays["gx"] == (idx & 4095)).all() and (rays["gy"] == (idx >> 12)).all() and (rays["rc"] == 0).all()
    o64 = p[0].astype(np.float64) + n.astype(np.float64) * float(F(0.002))
    assert (np.abs(rays["o"][0, 0] - o64) <= np.spacing(np.abs(o64).astype(F)) / 2).all()   # one rounding of the exact value


# ---- the stand-alone program ------------------------------------------------------------------------------------
def _run_standalone(target, tmp_path):
    p = subprocess.run([_build(target), str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:]
    assert "bake_test ok" in p.stdout, p.stdout[-4000:]
    for word in ("Sanitizer", "runtime error"):
        assert word not in p.stdout, p.stdout[-4000:]


def test_bake_host_checks(tmp_path):
    _run_standalone("bake_test", tmp_path)


def test_bake_host_checks_sanitized(tmp_path):
    from .test_accel_cpu import _sanitizers_work
    if not _sanitizers_work(str(tmp_path)):
        pytest.skip("a one-line program does not build or start under -fsanitize=address,undefined")
    _run_standalone("bake_test_san", tmp_path)


def test_bake_cpp_has_no_hip():
    for name in ("bake.cpp", "bake_test.cpp", "rmr_bake_rule.h"):
        text = open(os.path.join(CSRC, name)).read()
        assert "#include <hip" not in text and "__global__" not in text, name


# ---- the kernels' resources -------------------------------------------------------------------------------------
def test_bake_kernels_resources(tmp_path):
    """rmr_bake.hip for gfx950 with the compiler's resource remarks: no dynamic stack and no LDS anywhere, no
    scratch except in the general map's node interpreter (k_bake_ao<-1>, as k_cast_rays<-1>); DESIGN.md §4.17 has
    the figures."""
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-slp-vectorize",
           "-Wno-pass-failed", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
           os.path.join(CSRC, "rmr_bake.hip"), "-o", str(tmp_path / "rmr_bake.o")]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-4000:]
    res, name = {}, None
    for line in p.stdout.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
        m = re.search(r"(ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|VGPRs|TotalSGPRs|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            res[name][m.group(1).split(" [")[0]] = int(m.group(2))
        m = re.search(r"Dynamic Stack: (\w+)", line)
        if m and name:
            res[name]["Dynamic Stack"] = m.group(1)
    for k in sorted(res):
        print(k, res[k])
    assert len(res) == 9, sorted(res)   # k_bake_rays, k_bake_ray_list, k_bake_ao x 5, k_bake_fold x 2
    for k, v in res.items():
        assert v["Dynamic Stack"] == "False" and v["LDS Size"] == 0, (k, v)
        if "ILin1E" not in k:
            assert v["ScratchSize"] == 0, (k, v)
        if "k_bake_ao" not in k:
            assert v["VGPRs"] <= 64, (k, v)


# ---- rmr_cli ------------------------------------------------------------------------------------------------------
def test_cli_help_and_usage_errors():
    help_text = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--mesh-bake N[:AO_DISTANCE]" in help_text

    def rc(*args):
        return subprocess.run([CLI, "--size", "8x8"] + list(args), capture_output=True, text=True, timeout=60).returncode
    good = ("--mesh-bounds", "-1.5,-0.5,-1.5,1.5,2.5,1.5")
    for bad in (("--mesh-bake", "4"),                                          # without --mesh
                ("--mesh-bake", "4") + good,
                ("--mesh", "m.obj", "--mesh-bake", "4") + good,                # an OBJ has no colours
                ("--mesh", "m.ply", "--mesh-bake") + good,
                ("--mesh", "m.ply", "--mesh-bake", "0") + good,
                ("--mesh", "m.ply", "--mesh-bake", "-3") + good,
                ("--mesh", "m.ply", "--mesh-bake", "x") + good,
                ("--mesh", "m.ply", "--mesh-bake", "4x") + good,
                ("--mesh", "m.ply", "--mesh-bake", "4:") + good,
                ("--mesh", "m.ply", "--mesh-bake", "4:0") + good,
                ("--mesh", "m.ply", "--mesh-bake", "4:-1") + good,
                ("--mesh", "m.ply", "--mesh-bake", "4:nan") + good,
                ("--mesh", "m.ply", "--mesh-bake", "4:0.5x") + good,
                ("--mesh", "m.ply", "--mesh-bake", "99999999") + good,
                ("--mesh", "m.ply", "--mesh-bake", "4", "--gpus", "2") + good):
        assert rc(*bad) == 2, bad
    # good sets parse (--print-tiles ends the program before a device is needed)
    for ok in (("--mesh-bake", "4"), ("--mesh-bake", "16:0.5"), ("--mesh-bake", "1:inf")):
        assert rc("--mesh", "m.ply", *good, *ok, "--print-tiles", "--grid", "1x1") == 0, ok
