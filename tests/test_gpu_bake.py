"""Light baking on the GPU (include/rmr.h rmr_bake_points), every comparison bit for bit against
tests/bake_ref.py (the oracle's hemisphere, trace and march, the NumPy fold): the generated rays, the radiance
with the ahead-of-time and the hipRTC kernel, the occlusion, that cutting the work into launches and slices does
not change a byte, the rejects, the mesh's bake, rmr_cli --mesh-bake, that nothing else moved, and the errors.
Points: the first hits of a 16 x 12 grid of rays on Cornell-5 (a floor that is exactly up, a ceiling that takes
the degenerate rule, walls, a sphere), simple.scene (RM2) and csg_nodes, and hand-made points."""
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle
from raymarchrenderer_amd import Renderer, RMRError, abi, srgb8

from . import bake_ref as ref
from . import mesh_ref
from .conftest import SCENES
from .test_gpu_parity import _tables, same_bits
from .test_gpu_rays import CLI, H, SCENE_CASES, TIMES, VIEW, W, _context, _oracle

pytestmark = pytest.mark.gpu

F = np.float32
SCENE_NAMES = ["cornell5", "simple_rm2", "csg_nodes"]
N = 4                                   # seeds: TIMES, the schedule's frame 1
FIRST = (0, 4090, (1 << 24) + 5)        # the 4096 wrap inside the list; gy past 2^12 rows
TILE_BYTES = 64 * 64                    # one tile-sample of the radiance pass in the plane budget
SPHERE1 = os.path.join(SCENES, "sphere1.scene")


def _grid_rays():
    """A 16 x 12 grid of the view's rays (the pixel centres of a 16 x 12 image) from the eye; and, since that view
    sees no ceiling and little of the smaller scenes, a 12 x 12 grid of rays straight down from y = 3.5 and a
    4 x 4 grid straight up from y = 2 (the underside of Cornell-5's ceiling panel), and 96 rays from a sphere of
    radius 4 about (0, 1, 0) towards it (simple.scene is one unit sphere there)."""
    v = np.asarray(VIEW, np.float64).reshape(5, 3)
    u, w = np.meshgrid((np.arange(16) + 0.5) / 16, (np.arange(12) + 0.5) / 12)
    top = v[1] + (v[2] - v[1]) * u[..., None]
    bot = v[3] + (v[4] - v[3]) * u[..., None]
    d = top + (bot - top) * w[..., None]
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    rays = np.zeros(16 * 12 + 12 * 12 + 4 * 4 + 96, np.dtype(abi.RAY_DTYPE))
    rays["o"][:192], rays["d"][:192] = v[0].astype(F), d.reshape(-1, 3).astype(F)
    x, z = np.meshgrid(np.linspace(-2.9, 2.9, 12), np.linspace(-2.9, 2.9, 12))
    rays["o"][192:336] = np.stack([x.ravel(), np.full(144, 3.5), z.ravel()], axis=1).astype(F)
    rays["d"][192:336] = (0, -1, 0)
    x, z = np.meshgrid(np.linspace(-1.3, 1.3, 4), np.linspace(-1.3, 1.3, 4))
    rays["o"][336:352] = np.stack([x.ravel(), np.full(16, 2.0), z.ravel()], axis=1).astype(F)
    rays["d"][336:352] = (0, 1, 0)
    j = np.arange(96) + 0.5                      # a Fibonacci sphere
    y, phi = 1 - 2 * j / 96, j * np.pi * (3 - np.sqrt(5))
    out = np.stack([np.sqrt(1 - y * y) * np.cos(phi), y, np.sqrt(1 - y * y) * np.sin(phi)], axis=1)
    rays["o"][352:] = (np.array([0.0, 1.0, 0.0]) + 4 * out).astype(F)
    rays["d"][352:] = (-out).astype(F)
    return rays


HAND_POINTS = np.array([[0.3, 3.948, 0.2], [0.25, 1.5, -0.5], [-0.5, 0.5, 0.5], [1.6, -0.973, 0.3], [0.0, 1.0, 0.0],
                        [0.4, 0.3, -0.2]], F)
HAND_NORMALS = np.array([[0, -1, 0], [0, 0.99999994, 0], [-0.0, 1, 0], [0, 1, -0.0], [0.6, 0, 0.8],
                         [0.26726124, 0.5345225, 0.8017837]], F)

_cache = {}


def _case(name):
    """Per scene, once: the points and normals (the GPU's own first hits, which test_gpu_query pins to the
    oracle's, and the hand-made ones), and the reference's rays, cosines, radiance and occlusion for first_index 0."""
    if name in _cache:
        return _cache[name]
    path, variant, params = SCENE_CASES[name]
    r = _context(path, variant, params)
    try:
        hits = r.cast_rays(_grid_rays())
    finally:
        r.close()
    keep = hits["id"] >= 0
    p = np.concatenate([hits["pos"][keep], HAND_POINTS]).astype(F)
    n = np.concatenate([hits["n"][keep], HAND_NORMALS]).astype(F)
    prm = abi.default_params(**params)
    tables = _tables(path, variant)
    rays, c, ok = ref.rays(p, n, TIMES)
    case = {"p": p, "n": n, "rays": rays, "c": c, "ok": ok, "prm": prm, "tables": tables,
            "L": ref.trace_samples(_oracle(path, variant, params), rays),
            "blocked": {d: ref.march_blocked(tables, prm, rays, d) for d in (np.inf, 0.5)}}
    print("%s: %d points, %d rejected, %d exactly up, %d degenerate, %d of %d samples blocked (%d within 0.5)" % (
        name, len(p), (~ok).sum(), (n == [0, 1, 0]).all(axis=1).sum(), ((n[:, 0] == 0) & (n[:, 2] == 0)).sum(),
        case["blocked"][np.inf].sum(), c.size, case["blocked"][0.5].sum()))
    _cache[name] = case
    return case


def _want(case, nspp=N, ao_distance=None, m=None):
    """The reference's outputs of the first m points and the first nspp seeds."""
    m = len(case["p"]) if m is None else m
    blocked = None if ao_distance is None else case["blocked"][ao_distance][:nspp, :m]
    return ref.resolve(case["L"][:nspp, :m], case["c"][:nspp, :m], blocked, case["ok"][:m])


def _dev(a):
    """A host array as a torch tensor on the GPU. The device forms run on the context's own stream, which torch's
    stream is not ordered against: the caller keeps the tensor (and the results) alive until r.sync(), and reads
    a result only after it."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _extent(case, bias=0.002):
    return float(np.abs(case["p"]).max() + 2 * abs(bias))


# ---- 0. the lists are what the issue describes -----------------------------------------------------------------
def test_points_cover_the_cases():
    c = _case("cornell5")
    n = c["n"][:-len(HAND_POINTS)]
    assert (n == [0, 1, 0]).all(axis=1).sum() >= 10                       # the floor: exactly up
    assert ((n[:, 0] == 0) & (n[:, 2] == 0) & (n[:, 1] < 0)).sum() >= 5   # the ceiling: the degenerate rule
    assert ((n[:, 1] == 0) & (np.abs(n[:, 0]) == 1)).sum() >= 5            # a side wall
    assert ((n != 0).all(axis=1)).sum() >= 5                               # curved
    for name in SCENE_NAMES:
        c = _case(name)
        assert len(c["p"]) > 64 + len(HAND_POINTS) and c["ok"].all(), name
        L = c["L"]
        assert np.isfinite(L).all() and len(np.unique(L.reshape(-1, 3), axis=0)) > (1 if name == "simple_rm2" else 8), name
        if name != "simple_rm2":    # (one convex sphere under a constant sky occludes nothing)
            assert 0 < c["blocked"][0.5].sum() < c["blocked"][np.inf].sum() < c["c"].size, name


# ---- 1. the rays ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", FIRST)
def test_rays_bitexact(first):
    case = _case("cornell5")
    p, n = case["p"], case["n"]
    want = case["rays"] if first == 0 else ref.rays(p, n, TIMES, first_index=first)[0]
    if first == 4090:
        assert want["gx"][0, 5] == 4095 and want["gx"][0, 6] == 0 and want["gy"][0, 6] == 1
    if first == (1 << 24) + 5:
        assert want["gy"].min() == 4096
    r = Renderer(0, W, H)     # no scene: the generator needs none
    try:
        dp, dn = _dev(p), _dev(n)
        got = r.bake_rays_device(dp, dn, TIMES, first_index=first)
        r.sync()
        got = got.cpu().numpy().view(np.dtype(abi.RAY_DTYPE)).reshape(N, len(p))
        for k in ("o", "d", "time", "rc", "gx", "gy"):
            assert got[k].tobytes() == want[k].tobytes(), (first, k, np.argwhere(got[k] != want[k])[:3])
        assert got.tobytes() == want.tobytes()
        # another bias moves the origins alone
        g2 = r.bake_rays_device(dp, dn, TIMES[:1], first_index=first, bias=0.25)
        r.sync()
        g2 = g2.cpu().numpy().view(np.dtype(abi.RAY_DTYPE)).reshape(1, len(p))
        w2 = ref.rays(p[:70], n[:70], TIMES[:1], bias=0.25, first_index=first)[0]
        assert g2[:, :70].tobytes() == w2.tobytes() and g2["d"].tobytes() == want["d"][:1].tobytes()
        assert r.query_rejects() == 0
    finally:
        r.close()


# ---- 2. radiance ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jit", [0, 1])
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_radiance_bitexact(name, jit):
    case = _case(name)
    path, variant, params = SCENE_CASES[name]
    p, n = case["p"], case["n"]
    r = _context(path, variant, params, jit)
    try:
        for nspp in (N, 1):
            want, _ = _want(case, nspp)
            got = r.bake_points(p, n, TIMES[:nspp])
            assert got["ao"] is None and got["rgba"].shape == (len(p), 4) and got["rgba"].dtype == F
            eq = same_bits(got["rgba"], want).all(axis=1)
            assert eq.all(), "%s jit %d nspp %d: %d points differ, first %d gpu %s cpu %s" % (
                name, jit, nspp, (~eq).sum(), np.argmin(eq), got["rgba"][np.argmin(eq)], want[np.argmin(eq)])
            assert (got["rgba"][:, 3] == nspp).all()
            for m in (1, 63, 64, 65):
                assert r.bake_points(p[:m], n[:m], TIMES[:nspp])["rgba"].tobytes() == want[:m].tobytes(), (nspp, m)
        # the device form, with a generous bound on the origins
        dp, dn = _dev(p), _dev(n)
        d = r.bake_points_device(dp, dn, TIMES, _extent(case) * 3)
        r.sync()
        assert d["ao"] is None and d["rgba"].cpu().numpy().tobytes() == _want(case)[0].tobytes()
        assert r.query_rejects() == 0
        if jit:
            assert r.stats().jit_launches > 0
    finally:
        r.close()


# ---- 3. occlusion --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_occlusion_bitexact(name):
    case = _case(name)
    path, variant, params = SCENE_CASES[name]
    p, n = case["p"], case["n"]
    r = _context(path, variant, params)
    try:
        for dist in (np.inf, 0.5):
            _, want = _want(case, N, dist)
            got = r.bake_points(p, n, TIMES, radiance=False, ao=True, ao_distance=dist)
            assert got["rgba"] is None and got["ao"].shape == (len(p),)
            eq = same_bits(got["ao"], want)
            assert eq.all(), "%s ao %s: %d points differ, first %d gpu %s cpu %s" % (
                name, dist, (~eq).sum(), np.argmin(eq), got["ao"][np.argmin(eq)], want[np.argmin(eq)])
            assert ((want >= 0) & (want <= 1)).all() and (name == "simple_rm2" or len(np.unique(want)) > 4)
            for m in (1, 63, 65):
                assert r.bake_points(p[:m], n[:m], TIMES, radiance=False, ao=True, ao_distance=dist)["ao"].tobytes() == want[:m].tobytes()
            # one seed; capped grids (several strides per thread)
            w1 = _want(case, 1, dist)[1]
            assert r.bake_points(p, n, TIMES[:1], radiance=False, ao=True, ao_distance=dist)["ao"].tobytes() == w1.tobytes()
            for blocks in (1, 3):
                r.set_query_grid(blocks)
                assert r.bake_points(p, n, TIMES, radiance=False, ao=True, ao_distance=dist)["ao"].tobytes() == want.tobytes()
            r.set_query_grid(0)
            # both flags in one call: the two calls done separately
            both = r.bake_points(p, n, TIMES, radiance=True, ao=True, ao_distance=dist)
            assert both["ao"].tobytes() == want.tobytes() and both["rgba"].tobytes() == _want(case)[0].tobytes()
        # the rays' own cast gives the same verdicts (rmr_cast_rays_device on rmr_bake_rays_device's list)
        dp, dn = _dev(p), _dev(n)
        rays = r.bake_rays_device(dp, dn, TIMES)
        hits = r.cast_rays_device(rays, normals=False)
        r.sync()
        t = hits.cpu().numpy()[:, 3].reshape(N, len(p))
        assert ((t < case["prm"].max_dist) == case["blocked"][np.inf]).all()
    finally:
        r.close()


# ---- 4. cutting ----------------------------------------------------------------------------------------------------
def test_cutting_does_not_change_a_byte():
    case = _case("cornell5")
    p, n = case["p"], case["n"]
    want_rgba, want_ao = _want(case, N, np.inf)
    tiles = (len(p) + 63) // 64
    assert tiles >= 3
    r = _context(*SCENE_CASES["cornell5"])
    try:
        before = r.stats().trace_launches
        # 3 tile-samples per radiance launch: cuts inside a point's 4 samples and inside the point list;
        # 1 per launch: every sample on its own; 5: a launch spans two tiles
        for per_launch in (3, 1, 5):
            r.set_tuning(samp_budget=per_launch * TILE_BYTES)
            t0 = r.stats().trace_launches
            got = r.bake_points(p, n, TIMES, radiance=True, ao=True)
            assert r.stats().trace_launches - t0 == -(-tiles * N // per_launch), per_launch
            assert got["rgba"].tobytes() == want_rgba.tobytes() and got["ao"].tobytes() == want_ao.tobytes(), per_launch
        # the occlusion's launches hold 8 bytes per ray: 3 tile-samples of them
        r.set_tuning(samp_budget=3 * 64 * 8)
        assert r.bake_points(p[:130], n[:130], TIMES, radiance=False, ao=True)["ao"].tobytes() == want_ao[:130].tobytes()
        r.set_tuning(samp_budget=48 << 30)
        assert r.stats().trace_launches > before
        # a slice baked with first_index gives the bytes of the whole
        for a, b in ((0, 64), (64, 70), (70, len(p)), (129, 130)):
            got = r.bake_points(p[a:b], n[a:b], TIMES, radiance=True, ao=True, first_index=a)
            assert got["rgba"].tobytes() == want_rgba[a:b].tobytes() and got["ao"].tobytes() == want_ao[a:b].tobytes(), (a, b)
        # and a list that starts elsewhere is another list
        assert r.bake_points(p[:64], n[:64], TIMES, first_index=7)["rgba"].tobytes() != want_rgba[:64].tobytes()
    finally:
        r.close()


# ---- 5. rejects ----------------------------------------------------------------------------------------------------
def test_rejects():
    case = _case("cornell5")
    p, n = case["p"][:100].copy(), case["n"][:100].copy()
    bad = {3: ("n", [np.nan, 0, 1]), 17: ("n", [0, 0, 0]), 63: ("n", [0, 1.000001, 0]), 64: ("p", [0, np.nan, 0]),
           65: ("n", [0.6, 0.1, 0.8]), 99: ("p", [np.inf, 0, 0])}
    for i, (what, v) in bad.items():
        (p if what == "p" else n)[i] = v
    ok = ref.point_ok(p, n)
    assert sorted(np.flatnonzero(~ok)) == sorted(bad)
    want_rgba, want_ao = _want(case, N, np.inf, 100)
    want_rgba[~ok], want_ao[~ok] = 0, 0
    r = _context(*SCENE_CASES["cornell5"])
    try:
        assert r.query_rejects() == 0
        got = r.bake_points(p, n, TIMES, radiance=True, ao=True)
        assert r.query_rejects() == len(bad)        # once per point: not per sample, not per pass
        assert (got["rgba"][~ok].view(np.uint32) == 0).all() and (got["ao"][~ok].view(np.uint32) == 0).all()
        assert got["rgba"].tobytes() == want_rgba.tobytes() and got["ao"].tobytes() == want_ao.tobytes()   # the neighbours
        for flags in (dict(radiance=True, ao=False), dict(radiance=False, ao=True)):
            r.set_tuning(samp_budget=2 * TILE_BYTES if flags["radiance"] else 2 * 512)
            r.bake_points(p, n, TIMES, **flags)
            assert r.query_rejects() == len(bad), flags
        r.set_tuning(samp_budget=48 << 30)
        dp, dn = _dev(p), _dev(n)
        rays = r.bake_rays_device(dp, dn, TIMES)
        r.sync()
        assert r.query_rejects() == len(bad)
        rays_h = rays.cpu().numpy().view(np.dtype(abi.RAY_DTYPE)).reshape(N, 100)
        assert (rays_h["gx"][:, ~ok] == -1).all() and (rays_h["gx"][:, ok] >= 0).all()
        assert rays_h.tobytes() == ref.rays(p, n, TIMES)[0].tobytes()
        # such rays are rejected by the queries that take the list
        out = r.trace_rays_device(rays, 10.0)
        r.sync()
        assert r.query_rejects() == N * len(bad)
        assert (out.cpu().numpy().reshape(N, 100, 4)[:, ~ok] == 0).all()
        # an origin beyond the caller's bound is rejected as well (the device form)
        reach = np.abs(case["rays"]["o"][0, :64]).max(axis=1)
        bound = float(np.median(reach))
        dp, dn = _dev(case["p"][:64]), _dev(case["n"][:64])
        d = r.bake_points_device(dp, dn, TIMES, bound)
        r.sync()
        far = reach > F(bound)
        assert far.any() and not far.all() and r.query_rejects() == far.sum()
        got = d["rgba"].cpu().numpy()
        assert (got[far] == 0).all() and got[~far].tobytes() == _want(case)[0][:64][~far].tobytes()
    finally:
        r.close()


# ---- 6. the mesh ---------------------------------------------------------------------------------------------------
MESHES = {"sphere1": (SPHERE1, (-1.55, -0.55, -1.55), 3.1 / 23, (24, 24, 24)),
          # where Cornell-5's floor (its top at y = -0.975) meets the red wall (its face at x = -2.95)
          "cornell_corner": (SCENE_CASES["cornell5"][0], (-3.6, -1.6, -0.6), 1.2 / 23, (24, 24, 24))}


@pytest.mark.parametrize("name", sorted(MESHES))
def test_mesh_bake(name):
    path, origin, spacing, shape = MESHES[name]
    r = _context(path, "rm1", {"max_bounces": 4})
    try:
        m = r.extract_mesh(origin, spacing, shape)
        nv = len(m["vertices"])
        print("%s: %d vertices, %d quads" % (name, nv, len(m["quads"])))
        assert nv > 300
        with pytest.raises(RMRError) as e:
            r.read_mesh_bake()
        assert e.value.code == -5 and r.mesh_bake_device() == {"rgba": None, "ao": None}
        bias = float(F(spacing / 8))     # (past the vertices' distance from the surface)
        r.bake_mesh(TIMES[:2], radiance=True, ao=True, ao_distance=0.5, bias=bias)
        got = r.read_mesh_bake(rgba=True, ao=True)
        want = r.bake_points(m["vertices"], m["normals"], TIMES[:2], radiance=True, ao=True, ao_distance=0.5, bias=bias)
        assert got["rgba"].tobytes() == want["rgba"].tobytes() and got["ao"].tobytes() == want["ao"].tobytes()
        assert (got["rgba"][:, 3] == 2).all() and len(np.unique(got["rgba"][:, :3], axis=0)) > 30
        # (a lone convex sphere blocks nothing; where the floor meets the wall each blocks the other's hemisphere)
        assert (got["ao"] == 1).all() if name == "sphere1" else len(np.unique(got["ao"])) > 30
        dev = r.mesh_bake_device()
        r.sync()
        assert dev["rgba"].cpu().numpy().tobytes() == got["rgba"].tobytes() and dev["ao"].cpu().numpy().tobytes() == got["ao"].tobytes()
        # against the oracle, on a stride of the vertices
        pick = np.arange(0, nv, max(1, nv // 24))
        # (each vertex with its own invocation: first_index = its index)
        parts = [ref.rays(m["vertices"][i:i + 1], m["normals"][i:i + 1], TIMES[:2], bias=bias, first_index=int(i)) for i in pick]
        rays, c, ok = (np.concatenate([q[k] for q in parts], axis=-1) for k in range(3))
        orc = oracle.Oracle(_tables(path, "rm1"), abi.default_params(max_bounces=4), VIEW, W, H)
        w_rgba, w_ao = ref.resolve(ref.trace_samples(orc, rays), c,
                                   ref.march_blocked(_tables(path, "rm1"), abi.default_params(max_bounces=4), rays, 0.5), ok)
        assert same_bits(got["rgba"][pick], w_rgba).all() and same_bits(got["ao"][pick], w_ao).all()
        # the mesh itself is untouched; a second bake replaces what its flags name
        again = r.read_mesh()
        for k in m:
            assert again[k].tobytes() == m[k].tobytes(), k
        r.bake_mesh(TIMES[:1], bias=bias)
        got1 = r.read_mesh_bake(rgba=True, ao=True)
        assert got1["ao"].tobytes() == got["ao"].tobytes() and (got1["rgba"][:, 3] == 1).all()
        # the buffers go with the mesh: the next extraction, mesh_free
        r.extract_mesh(origin, spacing, shape)
        with pytest.raises(RMRError) as e:
            r.read_mesh_bake()
        assert e.value.code == -5 and not r.lib.rmr_mesh_bake_device_ptr(r.ctx, abi.MESH_BAKE_RGBA)
        r.bake_mesh(TIMES[:1], bias=bias)
        with pytest.raises(RMRError) as e:
            r.read_mesh_bake(rgba=False, ao=True)        # not baked
        assert e.value.code == -5 and r.lib.rmr_mesh_bake_device_ptr(r.ctx, abi.MESH_BAKE_RGBA)
        assert not r.lib.rmr_mesh_bake_device_ptr(r.ctx, abi.MESH_BAKE_AO) and not r.lib.rmr_mesh_bake_device_ptr(r.ctx, 5)
        assert r.read_mesh_bake()["rgba"].tobytes() == got1["rgba"].tobytes()
        r.mesh_free()
        with pytest.raises(RMRError) as e:
            r.bake_mesh(TIMES[:1])
        assert e.value.code == -5 and not r.lib.rmr_mesh_bake_device_ptr(r.ctx, abi.MESH_BAKE_RGBA)
        # without normals there is nothing to bake about
        r.extract_mesh(origin, spacing, shape, normals=False)
        with pytest.raises(RMRError) as e:
            r.bake_mesh(TIMES[:1])
        assert e.value.code == -5 and "normals" in str(e.value)
    finally:
        r.close()


def test_cli_mesh_bake(tmp_path):
    """rmr_cli --mesh-bake 3 on Cornell-5 writes a PLY whose positions, normals and ids are extract_mesh's and whose
    colours are srgb8 of bake_mesh's radiance with the render's seeds and the CLI's bias (0.002 + spacing / 8: the
    vertices lie a fraction of a cell inside the sphere); with :0.5 of the radiance times the occlusion."""
    out, ply = str(tmp_path / "cli.bmp"), str(tmp_path / "m.ply")
    _, origin, spacing, shape, iso = mesh_ref.CASES["cornell5"]     # 21 x 18 x 10 points at 0.33
    hi = [origin[a] + (shape[a] - 1) * spacing for a in range(3)]
    base = [CLI, "--scene", SCENE_CASES["cornell5"][0], "--variant", "rm1", "--size", "16x16", "--samples", "1", "--grid", "1x1",
            "--bounces", "4", "--frame", "1", "--out", out, "--quiet", "--mesh-bounds",
            ",".join("%.17g" % x for x in list(origin) + hi), "--mesh-grid", str(shape[0] - 1), "--mesh", ply]
    times = np.array([1000.0 + 0.016 * s for s in range(3)]).astype(F)
    r = _context(*SCENE_CASES["cornell5"])
    try:
        m = r.extract_mesh(origin, spacing, shape)
        r.bake_mesh(times, radiance=True, ao=True, ao_distance=0.5, bias=F(F(0.002) + F(0.125) * F(spacing)))
        bake = r.read_mesh_bake(rgba=True, ao=True)
    finally:
        r.close()
    assert len(np.unique(bake["ao"])) > 10
    lit = bake["rgba"][:, :3]
    shaded = (lit * bake["ao"][:, None]).astype(F)
    assert (srgb8(lit) != srgb8(shaded)).any()
    dt = np.dtype([("f", "<f4", (7,)), ("c", "u1", (3,))])
    for opt, rgb in (("3", lit), ("3:0.5", shaded)):
        p = subprocess.run(base + ["--mesh-bake", opt], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
        head, body = open(ply, "rb").read().split(b"end_header\n", 1)
        assert b"property uchar red\nproperty uchar green\nproperty uchar blue\n" in head
        assert ("element vertex %d\n" % len(m["vertices"])).encode() in head
        vert = np.frombuffer(body, dt, len(m["vertices"]))
        assert vert["f"][:, :3].tobytes() == m["vertices"].tobytes() and vert["f"][:, 3:6].tobytes() == m["normals"].tobytes()
        assert (vert["f"][:, 6] == m["ids"]).all()
        assert (vert["c"] == srgb8(rgb)).all() and len(np.unique(vert["c"], axis=0)) > 10, opt
        assert len(body) == dt.itemsize * len(vert) + 17 * len(m["quads"])


# ---- 7. nothing else moves --------------------------------------------------------------------------------------
def test_bake_leaves_everything_else_alone():
    rect = (3, 2, 41, 35)
    case = _case("cornell5")
    p, n = case["p"], case["n"]
    _, origin, spacing, shape, iso = mesh_ref.CASES["cornell5"]
    r = _context(*SCENE_CASES["cornell5"])
    fresh = _context(*SCENE_CASES["cornell5"])
    try:
        r.set_error_estimate(True)
        r.render_spp(TIMES, rect)
        r.render_guides()
        dn = r.denoise(iterations=2)
        r.tonemap("denoised", curve="aces")
        tm = r.read_tonemapped()
        r.render_aov(TIMES)
        aov = r.read_aov()
        mesh = r.extract_mesh(origin, spacing, shape)
        state = (r.read_accum(), r.read_half(), r.tile_error(), r.read_guides())

        def unchanged(what):
            assert same_bits(r.read_accum(), state[0]).all() and same_bits(r.read_half(), state[1]).all(), what
            assert same_bits(r.tile_error(), state[2]).all(), what
            assert same_bits(r.read_denoised(), dn).all() and same_bits(r.read_tonemapped(), tm).all(), what
            for k, g in r.read_guides().items():
                assert same_bits(g, state[3][k]).all(), (what, k)
            for k, g in r.read_aov().items():
                assert same_bits(g, aov[k]).all(), (what, k)
            again = r.read_mesh()
            for k in mesh:
                assert again[k].tobytes() == mesh[k].tobytes(), (what, k)

        got = r.bake_points(p, n, TIMES, radiance=True, ao=True)
        assert got["rgba"].tobytes() == _want(case)[0].tobytes()
        unchanged("bake_points")
        dev_p, dev_n = _dev(p), _dev(n)
        dev = r.bake_points_device(dev_p, dev_n, TIMES, _extent(case), radiance=True, ao=True)
        dev_rays = r.bake_rays_device(dev_p, dev_n, TIMES)
        r.sync()
        assert dev["rgba"].cpu().numpy().tobytes() == got["rgba"].tobytes() and dev["ao"].cpu().numpy().tobytes() == got["ao"].tobytes()
        assert dev_rays.cpu().numpy().view(np.dtype(abi.RAY_DTYPE)).tobytes() == case["rays"].tobytes()
        unchanged("the device forms")
        r.bake_mesh(TIMES[:1], radiance=True, ao=True)
        r.read_mesh_bake(rgba=True, ao=True)
        unchanged("bake_mesh")
        assert r.query_rejects() == 0
        # a following render finds a clean work queue: the same bits as a context that never baked
        r.render_spp(TIMES[:1], rect, first_sample=4)
        got = r.read_accum()
        fresh.set_error_estimate(True)
        fresh.render_spp(TIMES, rect)
        fresh.render_spp(TIMES[:1], rect, first_sample=4)
        assert same_bits(got, fresh.read_accum()).all() and not same_bits(got, state[0]).all()
    finally:
        r.close()
        fresh.close()


# ---- 8. errors -----------------------------------------------------------------------------------------------------
def test_state_and_errors():
    import torch
    case = _case("cornell5")
    p, n = case["p"][:8], case["n"][:8]
    r = Renderer(0, W, H)
    try:
        def code(call):
            with pytest.raises(RMRError) as e:
                call()
            return e.value.code

        assert code(lambda: r.bake_points(p, n, TIMES)) == -5                       # no scene
        assert code(lambda: r.bake_points(p, n, TIMES, radiance=False, ao=True)) == -5
        assert code(lambda: r.bake_points_device(_dev(p), _dev(n), TIMES, 10.0)) == -5
        assert code(lambda: r.bake_mesh(TIMES)) == -5
        r.load_scene(SCENE_CASES["cornell5"][0], "rm1")
        r.set_params(abi.default_params(max_bounces=4, separate_channels=1))
        assert code(lambda: r.bake_points(p, n, TIMES)) == -5                       # separate_channels
        assert code(lambda: r.bake_points(p, n, TIMES, radiance=False, ao=True)) == -5
        assert "separate_channels" in r.lib.rmr_last_error(r.ctx).decode()
        r.set_params(abi.default_params(max_bounces=4))
        want = _want(case, N, None, 8)[0]
        assert r.bake_points(p, n, TIMES)["rgba"].tobytes() == want.tobytes()
        assert code(lambda: r.bake_points(p, n, TIMES, radiance=False, ao=False)) == -1      # bad flags
        assert code(lambda: r.bake_points(p, n, TIMES, params=abi.BakeParams(4, 0.002, np.inf, 0.0, 0))) == -1
        assert code(lambda: r.bake_points(p, n, TIMES, params=abi.BakeParams(7, 0.002, np.inf, 0.0, 0))) == -1
        for bias in (np.nan, np.inf):
            assert code(lambda: r.bake_points(p, n, TIMES, bias=bias)) == -1                 # a non-finite bias
            assert code(lambda: r.bake_rays_device(_dev(p), _dev(n), TIMES, bias=bias)) == -1
        for dist in (0.0, -1.0, np.nan):
            assert code(lambda: r.bake_points(p, n, TIMES, ao=True, ao_distance=dist)) == -1
        assert code(lambda: r.bake_points(p, n, TIMES, first_index=(1 << 36) - 7)) == -1     # idx >= 2^36
        assert code(lambda: r.bake_rays_device(_dev(p), _dev(n), TIMES, first_index=(1 << 36) - 7)) == -1
        assert code(lambda: r.bake_points(p, n, TIMES, first_index=1 << 40)) == -1
        last = r.bake_points(p, n, TIMES, first_index=(1 << 36) - 8)["rgba"]                 # the last valid slice
        assert (last[:, 3] == N).all()
        assert code(lambda: r.bake_points(p, n, [])) == -1                                   # no seeds
        for ext in (-1.0, np.nan, np.inf):
            assert code(lambda: r.bake_points_device(_dev(p), _dev(n), TIMES, ext)) == -1    # origin_extent
        with pytest.raises(ValueError):
            r.bake_points(p, n[:7], TIMES)
        with pytest.raises(ValueError):
            r.bake_points(p, n, TIMES, params=abi.bake_params(), ao=True)      # params and keywords: one or the other
        with pytest.raises(ValueError):
            r.bake_points_device(_dev(p), torch.from_numpy(n.astype(np.float64)).cuda(), TIMES, 10.0)
        # an empty list is fine and touches nothing
        e = r.bake_points(np.zeros((0, 3), F), np.zeros((0, 3), F), TIMES, radiance=True, ao=True)
        assert e["rgba"].shape == (0, 4) and e["ao"].shape == (0,)
        assert r.bake_points(p, n, TIMES)["rgba"].tobytes() == want.tobytes()
        assert r.query_rejects() == 0
    finally:
        r.close()
