"""The sampled AOVs (rmr_render_aov) without a GPU: the host functions rmr_aov_init /
rmr_aov_fold / rmr_aov_resolve, which run the header the kernels compile (csrc/rmr_aov_rule.h), against the
NumPy statement tests/aov_ref.py (the fold bit for bit, the resolve within bounds counted from its float32
roundings), the hand case and the edge states of the rule, the order property, a fold of the oracle's first
hits of Cornell-5, the stand-alone program csrc/aov_test.cpp plain and under the sanitizers, the resources of
the kernels compiled for gfx950 (not run), and rmr_cli's argument handling."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import camera, scene_compile
from raymarchrenderer_amd import RMRError, abi, aov_fold, aov_init, aov_resolve, time_schedule

from . import aov_ref as ref
from . import camera_ref
from .conftest import ROOT, SCENES

CSRC = os.path.join(ROOT, "raymarchrenderer_amd", "csrc")
CLI = os.path.join(ROOT, "raymarchrenderer_amd", "rmr_cli")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
F = np.float32
HIT = np.dtype(abi.HIT_DTYPE)
E = 2.0 ** -24   # the relative error bound of one float32 rounding


def same_bits(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    return a.view(np.uint32) == b.view(np.uint32)


def _hits(ids, seed=0, n_px=1):
    """(len(ids), n_px) hit records with the ids given (negative: a miss) and distinct t, n and pos."""
    rng = np.random.default_rng(seed)
    ids = np.asarray(ids, F).reshape(len(ids), -1)
    h = np.zeros((len(ids), n_px), HIT)
    h["id"] = ids
    h["t"] = rng.uniform(0.5, 40.0, h.shape).astype(F)
    n = rng.normal(size=h.shape + (3,))
    h["n"] = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(F)
    h["pos"] = rng.uniform(-30.0, 30.0, h.shape + (3,)).astype(F)
    miss = ids < 0
    h["n"][miss] = 0
    return h


def _slots(state, i=0):
    s = state[:, i]
    return [(s[3, 0], s[3, 1]), (s[3, 2], s[3, 3]), (s[4, 0], s[4, 1]), (s[4, 2], s[4, 3])]


# ---- the rule --------------------------------------------------------------------------------------------
def test_initial_state():
    s = aov_init(3)
    assert s.shape == (5, 3, 4) and s.dtype == F
    assert same_bits(s, ref.init(3)).all()
    assert (s[0] == [0, 0, 0, np.inf]).all() and (s[1] == 0).all() and (s[2] == 0).all()
    assert (s[3] == [-1, 0, -1, 0]).all() and (s[4] == [-1, 0, -1, 0]).all()


def test_hand_case():
    """ids 3, 1, 4, 1, 5, 9, 2, 6, all hits."""
    h = _hits([3, 1, 4, 1, 5, 9, 2, 6], seed=1)
    s = aov_fold(aov_init(1), h)
    assert _slots(s) == [(3, 1), (1, 2), (4, 1), (5, 1)]
    assert s[1, 0, 3] == 3 and s[0, 0, 0] == 8 and s[0, 0, 1] == 8
    # the sums are numpy's sequential float32 sums, bit for bit
    st, sn, sp = F(0), np.zeros(3, F), np.zeros(3, F)
    for k in range(8):
        st = F(st + h["t"][k, 0])
        sn = (sn + h["n"][k, 0]).astype(F)
        sp = (sp + h["pos"][k, 0]).astype(F)
    assert same_bits(s[0, 0, 2], st) and same_bits(s[0, 0, 3], h["t"].min())
    assert same_bits(s[1, 0, :3], sn).all() and same_bits(s[2, 0, :3], sp).all() and s[2, 0, 3] == 0
    assert same_bits(s, ref.fold(ref.init(1), h)).all()
    r = aov_resolve(s, 1000.0)
    assert [tuple(r[3, 0, :2]), tuple(r[3, 0, 2:]), tuple(r[4, 0, :2]), tuple(r[4, 0, 2:])] == \
        [(1, F(2 / 8)), (3, F(1 / 8)), (4, F(1 / 8)), (5, F(1 / 8))]
    assert r[0, 0, 2] == 1 and r[0, 0, 3] == 8 and r[2, 0, 3] == 8


def test_edge_states():
    # a miss-only pixel
    s = aov_fold(aov_init(1), _hits([-1, -1, -1]))
    r = aov_resolve(s, 250.0)
    assert (s[0, 0] == [3, 0, 0, np.inf]).all()
    assert (r[0, 0] == [250, 250, 0, 3]).all() and (r[1, 0] == 0).all() and (r[2, 0] == 0).all()
    assert (r[3, 0] == [-1, 0, -1, 0]).all() and (r[4, 0] == [-1, 0, -1, 0]).all()
    # n = 0: no NaN
    r = aov_resolve(aov_init(2), 250.0)
    assert not np.isnan(r).any()
    assert (r[0] == [250, 250, 0, 0]).all() and (r[3] == [-1, 0, -1, 0]).all()
    # a count tie sorts by id; the empty slot last; a miss among the hits counts in n only
    s = aov_fold(aov_init(1), _hits([7, 2, 9, -1, 2, 7]))
    assert _slots(s) == [(7, 2), (2, 2), (9, 1), (-1, 0)]
    r = aov_resolve(s, 250.0)
    assert (r[3, 0] == [2, F(2 / 6), 7, F(2 / 6)]).all() and (r[4, 0] == [9, F(1 / 6), -1, 0]).all()
    assert r[0, 0, 2] == F(5 / 6) and r[2, 0, 3] == 5
    # normals that cancel: the zero normal, alpha stays
    h = _hits([0, 0])
    h["n"][0, 0] = [0, 1, 0]
    h["n"][1, 0] = [0, -1, 0]
    r = aov_resolve(aov_fold(aov_init(1), h), 250.0)
    assert (r[1, 0] == [0, 0, 0, 1]).all()
    # the 2^24 limit
    s = aov_init(1)
    s[0, 0, 0] = 2.0 ** 24
    with pytest.raises(RMRError):
        aov_fold(s, _hits([1]))


def test_fold_matches_numpy_statement_bitwise():
    """Random hit sequences over 300 pixels, 12 samples, ids from 7 materials and misses: the library's fold
    equals tests/aov_ref.py bit for bit, and every `other` and slot case occurs."""
    rng = np.random.default_rng(5)
    n_px, nspp = 300, 12
    ids = rng.integers(-2, 7, (nspp, n_px)).astype(F)
    ids[:, :100] = rng.integers(-1, 3, (nspp, 100))   # few ids: no overflow there
    ids[ids < 0] = -1
    h = _hits(ids, seed=6, n_px=n_px)
    s = aov_fold(aov_init(n_px), h)
    assert same_bits(s, ref.fold(ref.init(n_px), h)).all()
    assert (s[1, :, 3] > 0).any() and (s[1, :, 3] == 0).any() and (s[4, :, 2] == -1).any()
    assert (s[0, :, 0] == nspp).all()
    assert (s[0, :, 1] == s[3, :, 1] + s[3, :, 3] + s[4, :, 1] + s[4, :, 3] + s[1, :, 3]).all()


def test_order_property():
    """[A; B] in one call equals A then B bit for bit; B then A differs for a constructed case (the slot order
    and the sums' rounding both see order)."""
    A, B = _hits([1, 2, 1], seed=2), _hits([3, 1, 4], seed=3)
    A["n"][0, 0] = [1e8, 0, 0]
    B["n"][0, 0] = [-1e8, 0, 0]
    one = aov_fold(aov_init(1), np.concatenate([A, B]))
    two = aov_fold(aov_fold(aov_init(1), A), B)
    rev = aov_fold(aov_fold(aov_init(1), B), A)
    assert same_bits(one, two).all()
    assert not same_bits(one, rev).all()
    assert _slots(one)[0][0] == 1 and _slots(rev)[0][0] == 3
    assert not same_bits(one[1, 0, :3], rev[1, 0, :3]).all()   # (1e8 + n) - 1e8 against (-1e8 + n) + 1e8


def test_resolve_accuracy():
    """Quotients within 1 ulp of the correctly rounded float32 quotient (they are IEEE divisions: the observed
    distance is 0); normal components within 4 x 2^-24 absolute of the float64 statement: three products and
    two sums under a square root, then one division, at most 3 relative roundings on a component of at most
    1 (the inputs' own products and sums each contribute at most half of one to the length)."""
    rng = np.random.default_rng(9)
    n_px, nspp = 400, 16
    ids = rng.integers(-1, 6, (nspp, n_px)).astype(F)
    h = _hits(ids, seed=10, n_px=n_px)
    s = aov_fold(aov_init(n_px), h)
    r = aov_resolve(s, 1000.0)
    w = ref.resolve64(s, 1000.0)
    quot = [(0, 0), (0, 2), (2, 0), (2, 1), (2, 2), (3, 1), (3, 3), (4, 1), (4, 3)]
    worst_q = 0.0
    for p, k in quot:
        want = w[p, :, k].astype(F)   # the correctly rounded quotient (float64 quotient of float32 values, rounded)
        ulps = np.abs(r[p, :, k].astype(np.float64) - want) / np.spacing(np.abs(want)).astype(np.float64)
        worst_q = max(worst_q, float(ulps.max()))
    worst_n = float(np.abs(r[1, :, :3] - w[1, :, :3]).max())
    print("resolve: worst quotient distance %.3g ulp, worst normal component error %.3g = %.2f x 2^-24"
          % (worst_q, worst_n, worst_n / E))
    assert worst_q <= 1.0
    assert worst_n <= 4 * E
    # exact planes: ids, counts, min_t, n, h, alpha's copy
    for p, k in [(0, 1), (0, 3), (2, 3), (3, 0), (3, 2), (4, 0), (4, 2)]:
        assert (r[p, :, k] == w[p, :, k]).all(), (p, k)
    assert same_bits(r[1, :, 3], r[0, :, 2]).all()


# ---- the oracle's hits, no GPU ------------------------------------------------------------------------------
def test_oracle_fold_cornell5():
    W, H, nspp = 16, 12, 4
    view = camera.default_view(W, H)
    tables = scene_compile.load_scene_file(os.path.join(SCENES, "cornell5.scene"), "rm1")
    prm = abi.default_params()
    o, d, _ = camera_ref.rays(camera_ref.VIEW, view, W, H, time_schedule(nspp), (0, 0, W, H))
    rays = np.zeros(o.shape[:3], np.dtype(abi.RAY_DTYPE))
    rays["o"], rays["d"] = o, d
    hits = ref.oracle_hits(tables, prm, rays).reshape(nspp, W * H)
    s = aov_fold(aov_init(W * H), hits)
    assert same_bits(s, ref.fold(ref.init(W * H), hits)).all()
    r = aov_resolve(s, prm.max_dist)
    alpha, depth = r[0, :, 2], r[0, :, 0]
    is_hit = hits["id"] >= 0
    # silhouette pixels (some samples hit, some miss) have a fractional alpha
    edge = is_hit.any(axis=0) & ~is_hit.all(axis=0)
    assert edge.sum() >= 1 and ((alpha[edge] > 0) & (alpha[edge] < 1)).all()
    assert (alpha[is_hit.all(axis=0)] == 1).all() and (alpha[~is_hit.any(axis=0)] == 0).all()
    # pixels whose every sample lands on the unit sphere at the origin: alpha 1, depth inside the samples' range
    on_sphere = is_hit & (np.abs(np.linalg.norm(hits["pos"].astype(np.float64), axis=-1) - 1.0) < 0.01)
    inside = on_sphere.all(axis=0)
    assert inside.sum() >= 4 and (alpha[inside] == 1).all()
    interior = is_hit.all(axis=0)
    t = hits["t"]
    assert ((depth[interior] >= t.min(axis=0)[interior]) & (depth[interior] <= t.max(axis=0)[interior])).all()
    assert same_bits(r[0, interior, 1], t.min(axis=0)[interior]).all()


# ---- the stand-alone host program ----------------------------------------------------------------------
def _run_standalone(target):
    """csrc/aov_test.cpp (its own main, aov.cpp alone: no HIP, no Python in the program)."""
    subprocess.run(["make", "-s", "-C", CSRC, target], check=True, timeout=600)
    p = subprocess.run([os.path.join(CSRC, "build", target)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:]
    assert "aov_test ok" in p.stdout, p.stdout[-4000:]
    for word in ("Sanitizer", "runtime error"):
        assert word not in p.stdout, p.stdout[-4000:]


def test_aov_host_checks():
    _run_standalone("aov_test")


def test_aov_host_checks_sanitized(tmp_path):
    from .test_accel_cpu import _sanitizers_work
    if not _sanitizers_work(str(tmp_path)):
        pytest.skip("a one-line program does not build or start under -fsanitize=address,undefined")
    _run_standalone("aov_test_san")


def test_aov_cpp_has_no_hip():
    for name in ("aov.cpp", "aov_test.cpp", "rmr_aov_rule.h"):
        text = open(os.path.join(CSRC, name)).read()
        assert "#include <hip" not in text and "__global__" not in text, name


def test_ray_and_cast_statements_are_written_once():
    """k_aov calls the generator's and the cast's own statements (rmr_camera_ray.h, rmr_cast.h); neither the
    kernels' files nor rmr_aov.hip hold a second copy."""
    def text(name):
        return open(os.path.join(CSRC, name)).read()
    assert "camera_ray(" in text("rmr_camera.hip") and "camera_ray(" in text("rmr_aov.hip")
    assert "march_first_hit<" in text("rmr_query.hip") and "march_first_hit<" in text("rmr_aov.hip")
    assert "hit_normal<" in text("rmr_query.hip") and "hit_normal<" in text("rmr_aov.hip")
    for name in ("rmr_camera.hip", "rmr_query.hip", "rmr_aov.hip"):
        assert "primary_dir(" not in text(name) and "MAP::eval(P, vfma" not in text(name), name


# ---- the kernels' resources ----------------------------------------------------------------------------
def test_aov_kernels_resources(tmp_path):
    """rmr_aov.hip for gfx950 with the compiler's resource remarks: no LDS and no dynamic stack anywhere; no
    scratch except in the general map's node interpreter (k_aov<-1>, as k_guides<-1>); DESIGN.md §4.15 has
    the figures."""
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-slp-vectorize",
           "-Wno-pass-failed", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
           os.path.join(CSRC, "rmr_aov.hip"), "-o", str(tmp_path / "rmr_aov.o")]
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
    assert len(res) == 7, sorted(res)   # k_aov<4, 8, 0, -2, -1>, k_aov_init, k_aov_resolve
    for k, v in res.items():
        assert v["LDS Size"] == 0 and v["Dynamic Stack"] == "False", k
        if "k_aovILin1E" not in k:
            assert v["ScratchSize"] == 0, (k, v)


# ---- rmr_cli ------------------------------------------------------------------------------------------------
def test_cli_help_and_usage_errors():
    help_text = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--sampled-aov" in help_text

    def rc(*args):
        return subprocess.run([CLI, "--size", "8x8"] + list(args), capture_output=True, text=True,
                              timeout=60).returncode
    for bad in (("--sampled-aov",), ("--sampled-aov", ""), ("--sampled-aov", "p", "--gpus", "2"),
                ("--sampled-aov", "p", "--devices", "0,1")):
        assert rc(*bad) == 2, bad
    # it parses with every camera model (--print-tiles ends the program before a device is needed); the
    # first-hit planes' refusal under equirect and ortho stays, and comes before any device work
    for cam in ("thinlens:0.1,5", "equirect", "ortho:6,5"):
        assert rc("--sampled-aov", "p", "--camera", cam, "--print-tiles", "--grid", "1x1") == 0, cam
    assert rc("--aov", "p", "--camera", "equirect") == 2
    assert rc("--aov", "p", "--sampled-aov", "q", "--camera", "ortho:6,5") == 2
