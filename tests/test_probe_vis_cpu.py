"""The probes' visibility (include/rmr.h rmr_bake_probe_visibility / rmr_probe_irradiance_vis)
without a GPU: the texel directions, the octahedral encode, the fold and the weighted lookup bit for bit against
the NumPy statement tests/probe_vis_ref.py (through the library and through the stand-alone program
csrc/probe_vis_test.cpp), the estimator and the leak as derived checks, the file's two versions, the parameter
ranges, the program's own checks plain and under the sanitizers, the kernels' resources as compiled for gfx950
(not run) and rmr_cli's argument handling."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from raymarchrenderer_amd import (RMRError, abi, load_probes, probe_irradiance_host, probe_irradiance_vis_host, probe_vis_dirs,
                                  probe_vis_fold, save_probes)

from . import probe_ref
from . import probe_vis_ref as ref
from .conftest import ROOT

CSRC = os.path.join(ROOT, "raymarchrenderer_amd", "csrc")
CLI = os.path.join(ROOT, "raymarchrenderer_amd", "rmr_cli")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
F = np.float32


def _build(target):
    subprocess.run(["make", "-s", "-C", CSRC, target], check=True, timeout=600)
    return os.path.join(CSRC, "build", target)


def _program(mode, payload, tmp_path):
    src, dst = str(tmp_path / (mode + ".in")), str(tmp_path / (mode + ".out"))
    with open(src, "wb") as f:
        f.write(payload)
    p = subprocess.run([_build("probe_vis_test"), mode, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=600)
    assert p.returncode == 0 and "probe_vis_test %s ok" % mode in p.stdout, p.stdout[-4000:]
    return open(dst, "rb").read()


def _unit(rng, shape):
    v = rng.normal(size=shape + (3,))
    return (v / np.linalg.norm(v, axis=-1)[..., None]).astype(F)


# ---- the texel directions and the encode ----------------------------------------------------------------------
def test_texel_dirs_and_encode(tmp_path):
    D = probe_vis_dirs()
    want = ref.texel_dirs()
    assert D.dtype == F and D.shape == (64, 3) and D.tobytes() == want.tobytes()
    assert np.abs(np.linalg.norm(D.astype(np.float64), axis=1) - 1.0).max() <= 2 * 2.0 ** -23       # unit within 2 ulp
    assert len(np.unique(D, axis=0)) == 64 and (D[:, 2] > 0).sum() == 24 and (D[:, 2] == 0).sum() == 16
    assert ref.texel_of(D).tolist() == list(range(64))                                              # the encode inverts the decode
    # the four texels nearest each pole
    assert sorted(np.argsort(-D[:, 2])[:4].tolist()) == [27, 28, 35, 36]
    assert sorted(np.argsort(D[:, 2])[:4].tolist()) == [0, 7, 56, 63]
    # the hard cases, the program's encode against the statement's: the axes, z = -0, texel borders in both
    # halves (s = 1 exactly, so ox and oy are the border values themselves), z < 0 with x = 0, 0 and NaN
    rng = np.random.default_rng(2)
    hard = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1],
            [1, 0, -0.0], [0.5, 0.5, -0.0], [-0.25, 0.75, -0.0], [0.25, -0.5, 0.25], [-0.75, 0.0, 0.25], [0.5, 0.25, 0.25],
            [0.0, -0.25, 0.75], [0.25, -0.5, -0.25], [-0.5, 0.25, -0.25], [0.25, 0.25, -0.5], [-0.125, -0.125, -0.75],
            [0, 0.5, -0.5], [0, -0.3, -0.7], [-0.0, 0.25, -0.75], [0.4, 0, -0.6], [0.4, -0.0, -0.6], [0, 0, 0], [np.nan, 0, 1],
            [0, np.inf, 0], [3, -4, 12], [1e-30, 1e-30, -1e-30]]
    d = np.concatenate([np.array(hard, F), D, _unit(rng, (400,)), (_unit(rng, (100,)) * F(1e20)).astype(F)])
    want_j = ref.texel_of(d)
    got_j = np.frombuffer(_program("texel", struct.pack("<I", len(d)) + d.tobytes(), tmp_path), np.int32)
    assert got_j.tolist() == want_j.tolist()
    assert want_j[:6].tolist() == [4 * 8 + 7, 4 * 8, 7 * 8 + 4, 4, 4 * 8 + 4, 63]
    assert want_j[6] == 4 * 8 + 7                          # z = -0 is the upper half: (1, 0) is not folded over
    assert want_j[17] % 8 >= 4 and want_j[19] % 8 >= 4     # z < 0, x = +-0: sgn(0) = sgn(-0) = 1, folded to the +x side
    assert want_j[22] == 0 and want_j[23] == 0             # 0 / 0 and NaN: texel 0
    assert len(set(want_j.tolist())) == 64


# ---- the fold -------------------------------------------------------------------------------------------------
RANGE = F(2.75)


def _fold_inputs():
    """33 samples of 9 probes: distances on both sides of the range; NaN, +inf and -inf distances; a probe with
    no finite distance; a probe whose samples all point into one cap, so that most of its texels stay at A == 0."""
    rng = np.random.default_rng(29)
    N, n = 33, 9
    s = np.zeros((N, n, 4), F)
    s[..., :3] = _unit(rng, (N, n))
    s[..., 3] = rng.uniform(0.05, 4.5, (N, n)).astype(F)
    s[1, 3, 3] = np.nan
    s[2, 3, 3] = np.inf
    s[5, 4, 3] = -np.inf
    s[:, 5, 3] = np.nan                                   # nothing sampled: every texel sees to the range
    cap = _unit(rng, (N,)) * F(0.2) + np.array([0, 0, 1], F)
    s[:, 6, :3] = (cap / np.linalg.norm(cap, axis=1)[:, None]).astype(F)
    return s


def test_fold_matches_statement(tmp_path):
    s = _fold_inputs()
    N, n = s.shape[:2]
    want = ref.fold(s, RANGE)
    assert (s[..., 3] > RANGE).sum() > 50 and want[..., 0].max() <= RANGE
    assert (want[5, :, 0] == RANGE).all() and (want[5, :, 1] == RANGE * RANGE).all()
    untouched = (want[6, :, 0] == RANGE) & (want[6, :, 1] == RANGE * RANGE)
    assert untouched.sum() >= 16                           # the cap's samples reach no texel of the lower half
    A33 = ref.fold_steps(ref.fold_state(n), s, RANGE)[0]
    assert (A33 == 0).any(axis=1).sum() >= 2 and (A33[0] > 0).all()
    assert np.isfinite(want).all()
    got = probe_vis_fold(s, RANGE)
    assert got.dtype == F and got.shape == (n, 64, 2) and got.tobytes() == want.tobytes()
    head = struct.pack("<2If", n, N, RANGE)
    assert _program("fold", head + s.tobytes(), tmp_path) == want.tobytes()
    # nspp = 1
    one = ref.fold(s[:1], RANGE)
    assert probe_vis_fold(s[:1], RANGE).tobytes() == one.tobytes() and (one[..., 0] == RANGE).sum() > 64
    # two runs of k through the carried sums: the same bits, in the statement and in the program
    for cut in (1, 16, 32):
        st = ref.fold_steps(ref.fold_state(n), s[:cut], RANGE)
        assert ref.resolve(ref.fold_steps(st, s[cut:], RANGE), RANGE).tobytes() == want.tobytes(), cut
    assert _program("fold2", head + s.tobytes(), tmp_path) == want.tobytes()
    # the sums are sequential float32 sums: a float64 accumulation rounds to other bits at some texels
    ok = np.isfinite(s[..., 3])
    r = np.minimum(np.where(ok, s[..., 3], 0), RANGE).astype(np.float64)
    D = ref.texel_dirs()
    c = (((D[None, None, :, 0] * s[:, :, None, 0]).astype(F) + (D[None, None, :, 1] * s[:, :, None, 1]).astype(F)).astype(F)
         + (D[None, None, :, 2] * s[:, :, None, 2]).astype(F)).astype(F).astype(np.float64)
    w = np.where(ok[..., None] & (c > 0), c ** 32, 0.0)
    A = w.sum(axis=0)
    m1 = np.where(A > 0, (w * r[..., None]).sum(axis=0) / np.where(A > 0, A, 1), float(RANGE)).astype(F)
    differ = int((m1 != want[..., 0]).sum())
    print("%d of %d texels: the float32 fold's m1 differs from a float64 one" % (differ, n * 64))
    assert differ >= 1
    # the parameter errors
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(RMRError):
            probe_vis_fold(s, bad)
    with pytest.raises(RMRError):
        probe_vis_fold(np.zeros((0, 3, 4), F), RANGE)     # nspp == 0
    with pytest.raises(ValueError):
        probe_vis_fold(s[..., :3], RANGE)


# ---- the estimator, derived -----------------------------------------------------------------------------------
def test_estimator_sees_each_hemisphere():
    """The oracle's 4096 directions of one invocation, r = 1.5 for d.z > 0 and 1 otherwise. The four texels nearest
    +z have their centres 13 degrees from the pole, so every direction of the other hemisphere is at least 77
    degrees away: c < 0.23, c^32 < 1e-21 of a near sample's weight. m1 there is 1.5 within 1e-4 (and 1 at the four
    nearest -z); a constant r = 1 gives m1 = m2 = 1 exactly: w * 1 = w, and M1 = M2 = A bit for bit."""
    from . import bake_ref
    N = 4096
    gx, gy = bake_ref.invocation(4101, 1)
    p = np.array([0.3, 1.1, -0.4], F)
    times = (0.016 * np.arange(N)).astype(F)
    s = np.zeros((N, 1, 4), F)
    for k in range(N):
        s[k, 0, :3] = probe_ref.direction(gx[0], gy[0], times[k], p)
    s[:, 0, 3] = np.where(s[:, 0, 2] > 0, F(1.5), F(1.0))
    D = ref.texel_dirs()
    up, down = [27, 28, 35, 36], [0, 7, 56, 63]
    assert np.degrees(np.arccos(D[up, 2])).max() < 13.5 and np.degrees(np.arccos(-D[down, 2])).max() < 13.5
    vis = probe_vis_fold(s, 4.0)
    assert vis.tobytes() == ref.fold(s, 4.0).tobytes()
    print("m1 near +z:", vis[0, up, 0], "near -z:", vis[0, down, 0])
    assert np.abs(vis[0, up, 0] - 1.5).max() <= 1e-4 and np.abs(vis[0, down, 0] - 1.0).max() <= 1e-4
    assert np.abs(vis[0, up, 1] - 2.25).max() <= 3e-4
    s[:, 0, 3] = 1.0
    flat = probe_vis_fold(s, 4.0)
    assert (flat == 1.0).all()


# ---- the lookup -----------------------------------------------------------------------------------------------
def _lookup_case():
    """probe_ref.lookup_cases' field and 200 queries with synthetic maps (NaN in the invalid probes' maps, which
    must not leak), plus a group `near`: queries with r <= m1 at every corner under maps that see to the range."""
    desc, sh, q, nr, groups = probe_ref.lookup_cases()
    vis, rng = ref.lookup_maps(desc)
    vis[sh[:, 27] == 0] = np.nan
    return desc, sh, vis, rng, q, nr, groups


def test_lookup_matches_statement(tmp_path):
    desc, sh, vis, rng, q, nr, groups = _lookup_case()
    r0, r1 = groups["rejected"]
    for bias in (0.0, 0.125):
        want, ok = ref.lookup(desc, sh, vis, q, nr, bias)
        got, bad = probe_irradiance_vis_host(desc, sh, vis, q, nr, bias)
        eq = (got.view(np.uint32) == want.view(np.uint32)).all(axis=1)
        assert eq.all(), (bias, np.flatnonzero(~eq)[:5], got[~eq][:2], want[~eq][:2])
        assert (~ok).nonzero()[0].tolist() == list(range(r0, r0 + 10)) and bad == r0
        assert (want[r0:r0 + 10] == 0).all() and (want[r0 + 10:r1, 3] > 0).all()
        assert np.isfinite(want).all() and (want[:, :3] >= 0).all()
        payload = bytes(desc) + struct.pack("<If", len(q), bias) + sh.tobytes() + vis.tobytes() + q.tobytes() + nr.tobytes()
        assert _program("lookup", payload, tmp_path) == want.tobytes() + struct.pack("<I", r0)
    want, _ = ref.lookup(desc, sh, vis, q, nr, 0.0)
    plain, _ = probe_ref.lookup(desc, sh, q, nr)
    # on a lattice point the result is that probe's alone, as in the plain lookup: r == 0, both weights 1
    a, b = groups["on_lattice"]
    assert want[a:b].tobytes() == plain[a:b].tobytes() and (want[a:b, 3] == 1).sum() == b - a - 2
    # cells with no valid corner give 0; cells with some are renormalised over the rest
    a, b = groups["all_invalid"]
    assert (want[a:b] == 0).all()
    a, b = groups["some_invalid"]
    assert (want[a:b, 3] > 0).all()
    a, b = groups["outside"]
    assert (want[a:b, 3] > 0).sum() == 8
    # the weights act: most queries differ from the plain lookup, both sides of r <= m1 and the floor occur
    a, b = groups["random"]
    assert (want[a:b] != plain[a:b]).any(axis=1).sum() > 100
    pts = probe_ref.lattice_points(desc)
    qq, nn = q[a:b], nr[a:b]
    n = [int(desc.n[k]) for k in range(3)]
    cw = [probe_ref.cell(qq[:, k], desc.origin[k], desc.spacing, n[k])[0] for k in range(3)]
    pi = cw[0] + n[0] * (cw[1] + n[1] * cw[2])
    wb, wv = ref.corner_weights(np.nan_to_num(vis[pi]), pts[pi], qq, nn)
    assert (wv == 1).sum() > 10 and (wv == ref.VIS_FLOOR).sum() > 10 and ((wv > ref.VIS_FLOOR) & (wv < 1)).sum() > 10
    assert wb.min() >= 0.2 and wb.max() <= F(1.2) and wb.max() > 1.0 and wb.min() < 0.3
    # r <= m1 at every corner, bias 0 and wb equal at every corner that carries weight: a query on a lattice
    # plane z with the normal along z has g0 = 0 at the four corners of the next plane and v.z = 0, so b = 0, at
    # the other four
    far = ref.far_maps(desc, rng)
    mid = np.array([[0.3, 1.1, 2.75], [-0.6, 0.6, 3.25], [0.9, 1.3, 2.25]], F)
    up = np.tile(np.array([[0, 0, 1]], F), (len(mid), 1))
    flat = mid.copy()
    flat[:, 2] = [2.5, 3.0, 2.0]
    w_flat, _ = ref.lookup(desc, sh, far, flat, up, 0.0)
    g_flat, _ = probe_irradiance_vis_host(desc, sh, far, flat, up, 0.0)
    p_flat, _ = probe_ref.lookup(desc, sh, flat, up)
    assert g_flat.tobytes() == w_flat.tobytes()
    # every weighted corner has b = 0: wb = 0.45 for all, W = 0.45 W_plain and rgb equal within a few roundings
    assert np.abs(w_flat[:, 3] / p_flat[:, 3] - 0.45).max() <= 1e-6
    assert np.abs(w_flat[:, :3] - p_flat[:, :3]).max() <= 1e-5 * np.abs(p_flat[:, :3]).max()
    # the parameter errors
    for bad in (-0.01, np.nan, np.inf):
        with pytest.raises(RMRError):
            probe_irradiance_vis_host(desc, sh, vis, q[:1], nr[:1], bad)
    with pytest.raises(ValueError):
        probe_irradiance_vis_host(desc, sh, vis[:-1], q[:1], nr[:1])
    with pytest.raises(ValueError):
        probe_irradiance_vis_host(desc, sh[:-1], vis, q[:1], nr[:1])
    with pytest.raises(RMRError):
        probe_irradiance_vis_host(((0, 0, 0), 1.0, (1, 2, 2)), np.zeros((4, 28), F), np.zeros((4, 64, 2), F), q[:1], nr[:1])


def test_leak_is_closed():
    """A 2 x 2 x 2 field, spacing 1: the four x = 0 probes hold the constant radiance 1, the four x = 1 probes 0.
    Every probe sees to the range, except the x = 0 probes towards +x: m1 = 0.5, m2 = m1^2 (a wall half a cell
    away, no variance). The query lies mid-cell at x = 0.75 behind that wall, normal along y. The plain lookup
    blends by position: 0.25. With visibility every x = 0 corner has var = 0, so ch = 0 and wv is the floor 0.05;
    every x = 1 corner has r <= m1, wv = 1. With g0 = 0.25 / 4 and 0.75 / 4 per corner and wb summed per side, the
    result is 0.25 * 0.05 / (0.25 * 0.05 + 0.75 * wb_ratio), wb_ratio = sum wb(x = 1) / sum wb(x = 0)."""
    desc = abi.volume_desc((0.0, 0.0, 0.0), 1.0, (2, 2, 2))
    pts = probe_ref.lattice_points(desc)
    lit = pts[:, 0] == 0
    sh = np.zeros((8, 28), F)
    sh[:, 27] = 16
    sh[lit, :3] = F(1.0) / probe_ref.Y0
    rng = F(2.6)
    vis = ref.far_maps(desc, rng)
    wall = ref.texel_dirs()[:, 0] > 0
    for i in np.flatnonzero(lit):
        vis[i, wall, 0] = 0.5
        vis[i, wall, 1] = 0.25
    q = np.array([[0.75, 0.5, 0.5]], F)
    nr = np.array([[0, 1, 0]], F)
    plain, _ = probe_irradiance_host(desc, sh, q, nr)
    assert abs(float(plain[0, 0]) - 0.25) <= 1e-6 and plain[0, 3] == 1
    got, bad = probe_irradiance_vis_host(desc, sh, vis, q, nr, 0.0)
    want, _ = ref.lookup(desc, sh, vis, q, nr, 0.0)
    assert bad is None and got.tobytes() == want.tobytes()
    wb, wv = ref.corner_weights(vis, pts, np.tile(q, (8, 1)), np.tile(nr, (8, 1)))
    assert (wv[lit] == ref.VIS_FLOOR).all() and (wv[~lit] == 1).all()
    wb_ratio = float(wb[~lit].astype(np.float64).sum() / wb[lit].astype(np.float64).sum())
    bound = 0.25 * 0.05 / (0.25 * 0.05 + 0.75 * wb_ratio)
    print("plain %.6f, with visibility %.6f, the derived value %.6f (wb_ratio %.4f)" % (plain[0, 0], got[0, 0], bound, wb_ratio))
    assert bound < 0.03
    assert float(got[0, 0]) <= bound * (1 + 1e-5) and got[0, 0] == got[0, 1] == got[0, 2]
    assert float(got[0, 0]) >= bound * (1 - 1e-5)


# ---- the file -------------------------------------------------------------------------------------------------
def test_file_versions(tmp_path):
    desc, sh, vis, rng, _, _, _ = _lookup_case()
    sh[3, 5] = np.nan
    path = str(tmp_path / "field.probes")
    # version 1: the bytes of the layout as it was, built by hand
    save_probes(path, desc, sh)
    v1 = b"RMRPROBES 1 5 4 4 -1 0.25 2 0.5\n" + sh.astype("<f4").tobytes()
    assert open(path, "rb").read() == v1
    d1, sh1 = load_probes(path)
    assert bytes(d1) == bytes(desc) and sh1.tobytes() == sh.tobytes()
    got = load_probes(path, visibility=True)
    assert len(got) == 4 and got[2] is None and got[3] is None and got[1].tobytes() == sh.tobytes()
    # version 2
    save_probes(path, desc, sh, vis, rng)
    raw = open(path, "rb").read()
    head, body = raw.split(b"\n", 1)
    assert head == b"RMRPROBES 2 5 4 4 -1 0.25 2 0.5 8 " + ("%.9g" % rng).encode() and head.endswith(b" 8 1.29999995")
    assert body == sh.astype("<f4").tobytes() + vis.astype("<f4").tobytes()
    d2, sh2 = load_probes(path)                                     # without the flag: (desc, sh) as ever
    assert bytes(d2) == bytes(desc) and sh2.tobytes() == sh.tobytes()
    d2, sh2, vis2, rng2 = load_probes(path, visibility=True)
    assert bytes(d2) == bytes(desc) and sh2.tobytes() == sh.tobytes()
    assert vis2.dtype == F and vis2.shape == (80, 64, 2) and vis2.tobytes() == vis.tobytes() and rng2 == rng and rng2.dtype == F
    for bad in (b"RMRPROBES 2 2 2 2 0 0 0 1\n" + bytes(8 * 112), b"RMRPROBES 2 2 2 2 0 0 0 1 8 2.5\n" + bytes(8 * 112),
                b"RMRPROBES 2 2 2 2 0 0 0 1 4 2.5\n" + bytes(8 * 624), b"RMRPROBES 1 2 2 2 0 0 0 1 8 2.5\n" + bytes(8 * 624),
                b"RMRPROBES 3 2 2 2 0 0 0 1 8 2.5\n" + bytes(8 * 624)):
        open(path, "wb").write(bad)
        with pytest.raises(ValueError):
            load_probes(path, visibility=True)
    open(path, "wb").write(b"RMRPROBES 2 2 2 2 0 0 0 1 8 0\n" + bytes(8 * 624))
    with pytest.raises(ValueError):
        load_probes(path, visibility=True)
    open(path, "wb").write(b"RMRPROBES 2 2 2 2 0 0 0 1 8 2.5\n" + bytes(8 * 624))
    assert load_probes(path, visibility=True)[3] == F(2.5)
    for kw in ({"vis": vis}, {"vis_range": rng}, {"vis": vis[:-1], "vis_range": rng}, {"vis": vis, "vis_range": 0.0},
               {"vis": vis, "vis_range": np.nan}):
        with pytest.raises(ValueError):
            save_probes(path, desc, sh, **kw)


# ---- the stand-alone program ----------------------------------------------------------------------------------
def _run_standalone(target):
    p = subprocess.run([_build(target)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:]
    assert "probe_vis_test ok" in p.stdout, p.stdout[-4000:]
    for word in ("Sanitizer", "runtime error"):
        assert word not in p.stdout, p.stdout[-4000:]


def test_probe_vis_host_checks():
    _run_standalone("probe_vis_test")


def test_probe_vis_host_checks_sanitized(tmp_path):
    from .test_accel_cpu import _sanitizers_work
    if not _sanitizers_work(str(tmp_path)):
        pytest.skip("a one-line program does not build or start under -fsanitize=address,undefined")
    _run_standalone("probe_vis_test_san")


def test_probe_vis_cpp_has_no_hip():
    for name in ("probe_vis.cpp", "probe_vis_test.cpp", "rmr_probe_vis_rule.h"):
        text = open(os.path.join(CSRC, name)).read()
        assert "#include <hip" not in text and "__global__" not in text, name


# ---- the kernels' resources -----------------------------------------------------------------------------------
def test_probe_vis_kernels_resources(tmp_path):
    """rmr_probe_vis.hip for gfx950 with the compiler's resource remarks: no dynamic stack and no LDS anywhere, no
    scratch except in the general map's node interpreter (k_probe_vis_cast<-1>, as k_cast_rays<-1>), and the
    register counts DESIGN.md §4.19 records as bounds."""
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-slp-vectorize",
           "-Wno-pass-failed", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
           os.path.join(CSRC, "rmr_probe_vis.hip"), "-o", str(tmp_path / "rmr_probe_vis.o")]
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
    assert len(res) == 7, sorted(res)   # k_probe_vis_cast x 5, k_probe_vis_fold, k_probe_lookup_vis
    for k, v in res.items():
        assert v["Dynamic Stack"] == "False" and v["LDS Size"] == 0, (k, v)
        if "ILin1E" not in k:
            assert v["ScratchSize"] == 0, (k, v)
        if "k_probe_vis_fold" in k:
            assert v["VGPRs"] <= VGPR_FOLD, (k, v)
        if "k_probe_lookup_vis" in k:
            assert v["VGPRs"] <= VGPR_LOOKUP, (k, v)
        if "k_probe_vis_cast" in k and "ILin1E" not in k:
            assert v["VGPRs"] <= VGPR_CAST, (k, v)


# as compiled: the fold 15, the lookup 72, the casts 22 to 26; the bounds leave a compiler some room
VGPR_FOLD, VGPR_LOOKUP, VGPR_CAST = 32, 96, 32


# ---- rmr_cli --------------------------------------------------------------------------------------------------
def test_cli_help_and_usage_errors():
    help_text = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--probe-visibility K[:RANGE]" in help_text and "RMRPROBES 2" in help_text

    def rc(*args):
        return subprocess.run([CLI, "--size", "8x8"] + list(args), capture_output=True, text=True, timeout=60).returncode
    good = ("--probes", "p.bin", "--probe-bounds", "-1.5,-0.5,-1.5,1.5,2.5,1.5")
    for bad in (("--probe-visibility", "4"),                                     # without --probes
                ("--probe-visibility", "4", "--probe-bounds", "-1.5,-0.5,-1.5,1.5,2.5,1.5"),
                good + ("--probe-visibility",),
                good + ("--probe-visibility", "0"),
                good + ("--probe-visibility", "-2"),
                good + ("--probe-visibility", "x"),
                good + ("--probe-visibility", "4x"),
                good + ("--probe-visibility", "99999999"),
                good + ("--probe-visibility", "4:"),
                good + ("--probe-visibility", "4:0"),
                good + ("--probe-visibility", "4:-1"),
                good + ("--probe-visibility", "4:nan"),
                good + ("--probe-visibility", "4:inf"),
                good + ("--probe-visibility", "4:0.5x"),
                good + ("--probe-visibility", "4", "--gpus", "2")):
        assert rc(*bad) == 2, bad
    # good sets parse (--print-tiles ends the program before a device is needed)
    for ok in (("--probe-visibility", "4"), ("--probe-visibility", "16:0.5"), ("--probe-visibility", "1:2.6", "--probe-grid", "4")):
        assert rc(*good, *ok, "--print-tiles", "--grid", "1x1") == 0, ok
