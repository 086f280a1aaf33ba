"""The probes' visibility on the GPU (include/rmr.h rmr_bake_probe_visibility / rmr_probe_irradiance_vis, DESIGN.md
§4.19), every comparison bit for bit against tests/probe_vis_ref.py (the oracle's sphere directions, map and
march, the NumPy fold and lookup): the list bake on Cornell-5 with buried and rejected probes under the default
plane budget and budgets that cut inside a probe's samples and inside the list; a node-program scene and an RM2
scene; the field form against the list form; the lookup on synthetic and on baked maps; what drops the
visibility; that nothing else moved; and the errors."""
import numpy as np
import pytest

from raymarchrenderer_amd import Renderer, RMRError, abi, probe_irradiance_vis_host, time_schedule

from . import probe_ref
from . import probe_vis_ref as ref
from .test_gpu_parity import _tables, same_bits
from .test_gpu_rays import H, SCENE_CASES, TIMES, VIEW, W, _context

pytestmark = pytest.mark.gpu

F = np.float32
TIMES33 = time_schedule(33, frame=1)
UNIT_TILE_BYTES = 64 * 16               # one tile-sample of 16-byte records in the plane budget
FIRST = 4090                            # gx wraps and gy steps inside the list
EXTENT = 5.0                            # the device forms' bound: probe BEYOND lies outside it
RANGE = F(2.0)
N_PROBES = 70                           # one full 64-probe tile and a partial one
BURIED = {3: (1.0, -1.03, 1.0), 63: (-3.0, 1.0, 0.5), 64: (3.01, 2.0, -1.0)}   # inside the floor and the two walls
AT_CLEARANCE, NAN, BEYOND = 17, 65, 69
FIELD = ((-2.2, -0.6, -1.8), 2.2, (3, 3, 2))

_cache = {}


def _dev(a):
    """A host array as a torch tensor on the GPU (the caller keeps it alive until r.sync())."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _points():
    rng = np.random.default_rng(41)
    p = np.stack([rng.uniform(-2.8, 2.8, N_PROBES), rng.uniform(-0.9, 3.8, N_PROBES), rng.uniform(-3.0, 3.0, N_PROBES)],
                 axis=1).astype(F)
    for i, v in BURIED.items():
        p[i] = v
    p[AT_CLEARANCE] = (1.5, -0.9, 0.7)            # 0.075 above Cornell-5's floor
    p[NAN] = (0.5, np.nan, 0.5)
    p[BEYOND] = (0.5, 1.0, 9.0)
    return p


def _case(name):
    """Once per scene: the 70 probes, the statement's maps of them with 33 seeds, first_index FIRST and no extent."""
    if name in _cache:
        return _cache[name]
    from oracle import oracle
    path, variant, params = SCENE_CASES[name]
    tables = _tables(path, variant)
    prm = abi.default_params(**params)
    p = _points()
    clearance = float(oracle.map_p(tables, p[AT_CLEARANCE], prm.max_dist)[0]) if name == "cornell5" else 0.0
    vis, rejected, buried, s = ref.bake(tables, p, TIMES33, RANGE, FIRST, clearance, np.inf, prm)
    case = {"p": p, "clearance": clearance, "vis": vis, "rejected": rejected, "buried": buried, "samples": s}
    _cache[name] = case
    return case


def _want(case, extent):
    vis = case["vis"].copy()
    if extent < 9.0:
        vis[BEYOND] = 0
    return vis


def _same(got, want, what):
    eq = same_bits(got, want).reshape(len(want), -1).all(axis=1)
    assert eq.all(), "%s: %d probes differ, first %d gpu %s cpu %s" % (
        what, (~eq).sum(), np.argmin(eq), np.asarray(got)[np.argmin(eq)].ravel()[:4], want[np.argmin(eq)].ravel()[:4])


def test_probes_cover_the_cases():
    c = _case("cornell5")
    assert 0.07 < c["clearance"] < 0.08
    assert c["rejected"].nonzero()[0].tolist() == [NAN]
    assert all(c["buried"][i] for i in BURIED) and not c["buried"][AT_CLEARANCE] and not c["buried"][BEYOND]
    used = ~(c["rejected"] | c["buried"])
    assert used.sum() >= 50 and (c["vis"][~used] == 0).all() and (c["vis"][used, :, 0] > 0).all()
    t = c["samples"][:, used, 3]
    assert np.isfinite(t).all() and (t > RANGE).sum() > 100 and (t < RANGE).sum() > 100     # both sides of the clamp
    assert (c["vis"][used, :, 0] == RANGE).any() and (c["vis"][used, :, 0] < RANGE).any()
    # 33 samples leave texels nobody touched (c^32 underflows to 0 at wide angles) at some probes
    A = ref.fold_steps(ref.fold_state(N_PROBES), c["samples"], RANGE)[0]
    print("texels with A == 0 over the used probes: %d" % (A[used] == 0).sum())


# ---- 1. the list bake on Cornell-5 -------------------------------------------------------------------------------
@pytest.mark.parametrize("per_launch", [None, 1, 5, 40])
def test_list_bake_cornell(per_launch):
    c = _case("cornell5")
    p = c["p"]
    r = _context(*SCENE_CASES["cornell5"])
    try:
        if per_launch:
            r.set_tuning(samp_budget=per_launch * UNIT_TILE_BYTES)
        dp = _dev(p)
        got = r.bake_probe_visibility_device(dp, TIMES33, EXTENT, RANGE, first_index=FIRST, clearance=c["clearance"])
        r.sync()
        got = got.cpu().numpy()
        assert got.shape == (N_PROBES, 64, 2) and got.dtype == F
        _same(got, _want(c, EXTENT), "device, %s per launch" % per_launch)
        assert r.query_rejects() == 2                   # the NaN and the one beyond the extent, once each
        # the host form takes the extent from the list: only the NaN is rejected
        host = r.bake_probe_visibility(p, TIMES33, RANGE, first_index=FIRST, clearance=c["clearance"])
        _same(host, c["vis"], "host, %s per launch" % per_launch)
        assert r.query_rejects() == 1
        if per_launch is None:
            # a slice baked with first_index gives the bytes of the whole; fewer seeds are a prefix's fold
            for a, b in ((0, 64), (64, 70), (5, 6)):
                part = r.bake_probe_visibility(p[a:b], TIMES33, RANGE, first_index=FIRST + a, clearance=c["clearance"])
                _same(part, c["vis"][a:b], "slice %d:%d" % (a, b))
            one = r.bake_probe_visibility(p, TIMES33[:1], RANGE, first_index=FIRST, clearance=c["clearance"])
            unused = c["rejected"] | c["buried"]
            want1 = ref.fold(c["samples"][:1], RANGE)
            want1[unused] = 0
            _same(one, want1, "one seed")
            r.query_rejects()
    finally:
        r.close()


# ---- 2. a node-program scene and an RM2 scene --------------------------------------------------------------------
@pytest.mark.parametrize("name", ["csg_nodes", "simple_rm2"])
def test_other_scenes(name):
    c = _case(name)
    path, variant, params = SCENE_CASES[name]
    if name == "simple_rm2":
        params = dict(params, separate_channels=1)      # nothing is traced: the probe bake's refusal does not apply
    assert c["rejected"].sum() == 1 and 40 <= (~(c["rejected"] | c["buried"])).sum() <= 69
    r = _context(path, variant, params)
    try:
        if name == "simple_rm2":
            with pytest.raises(RMRError) as e:
                r.bake_probes(c["p"], TIMES33[:1])
            assert e.value.code == -5
        got = r.bake_probe_visibility(c["p"], TIMES33, RANGE, first_index=FIRST)
        _same(got, c["vis"], name)
        assert r.query_rejects() == 1
    finally:
        r.close()


# ---- 3. the field form -------------------------------------------------------------------------------------------
def test_field_form():
    desc = abi.volume_desc(*FIELD)
    pts = probe_ref.lattice_points(desc)
    r = _context(*SCENE_CASES["cornell5"])
    try:
        r.bake_probe_field(desc, times=TIMES33[:3], clearance=0.3)
        _, sh = r.read_probe_field()
        invalid = sh[:, 27] == 0
        assert 1 <= invalid.sum() <= 6 and len(pts) == 18          # (a lattice point inside the sphere or near a wall)
        assert r.probe_field_visibility_device() is None
        r.bake_probe_field_visibility(TIMES33[:7], RANGE)
        vis, rng = r.read_probe_field_visibility()
        assert rng == RANGE and rng.dtype == F and vis.shape == (18, 64, 2)
        want = r.bake_probe_visibility(pts, TIMES33[:7], RANGE, clearance=0.3)
        _same(vis, want, "field against list")
        assert (vis[invalid] == 0).all() and (vis[~invalid, :, 0] > 0).all()
        dev = r.probe_field_visibility_device()
        r.sync()
        assert same_bits(dev.cpu().numpy(), vis).all()
        # the field's validity decides, not a buried test of the bake's own: a written field with other flags
        sh2 = sh.copy()
        sh2[:, 27] = 1
        sh2[0, 27] = 0
        r.write_probe_field(desc, sh2)
        r.bake_probe_field_visibility(TIMES33[:7], RANGE)
        vis2, _ = r.read_probe_field_visibility()
        all_used = r.bake_probe_visibility(pts, TIMES33[:7], RANGE, clearance=0.0)
        buried0 = (all_used.reshape(18, -1) == 0).all(axis=1)
        assert (vis2[0] == 0).all() and same_bits(vis2[1:][~buried0[1:]], all_used[1:][~buried0[1:]]).all()
        # (a probe inside a shape marches to t = 0 at once: its map is zeros either way; one that the clearance alone
        # had buried now has a map)
        revived = invalid & ~buried0
        revived[0] = False
        assert revived.any() and (vis2[revived, :, 0] > 0).all()
        # the default range
        r.bake_probe_field_visibility(TIMES33[:2])
        assert r.read_probe_field_visibility()[1] == F(2.6) * F(2.2)
        assert r.query_rejects() == 0
    finally:
        r.close()


# ---- 4. the lookup -----------------------------------------------------------------------------------------------
def test_lookup_synthetic_maps():
    desc, sh, q, nr, groups = probe_ref.lookup_cases()
    vis, rng = ref.lookup_maps(desc)
    vis[sh[:, 27] == 0] = np.nan
    r = Renderer(0, W, H)                       # no scene: the lookup needs none
    try:
        r.write_probe_field(desc, sh)
        r.write_probe_field_visibility(vis, rng)
        back, rng2 = r.read_probe_field_visibility()
        assert back.tobytes() == vis.tobytes() and rng2 == rng
        for bias in (0.0, 0.125):
            want, ok = ref.lookup(desc, sh, vis, q, nr, bias)
            host, bad = probe_irradiance_vis_host(desc, sh, vis, q, nr, bias)
            assert host.tobytes() == want.tobytes() and bad == groups["rejected"][0]
            got = r.probe_irradiance(q, nr, visibility=True, bias=bias)
            eq = same_bits(got, want).all(axis=1)
            assert eq.all(), "bias %s: %d queries differ, first %d gpu %s cpu %s" % (
                bias, (~eq).sum(), np.argmin(eq), got[np.argmin(eq)], want[np.argmin(eq)])
            assert r.query_rejects() == (~ok).sum() == 10
        dq, dn = _dev(q), _dev(nr)
        dev = r.probe_irradiance_device(dq, dn, visibility=True, bias=0.125)
        r.sync()
        assert same_bits(dev.cpu().numpy(), want).all() and r.query_rejects() == 10
        for m in (1, 63, 64, 65):
            assert same_bits(r.probe_irradiance(q[:m], nr[:m], visibility=True, bias=0.125), want[:m]).all(), m
        assert r.probe_irradiance(q[:0], nr[:0], visibility=True).shape == (0, 4)
        # visibility=False is the plain lookup, bytewise
        plain, _ = probe_ref.lookup(desc, sh, q, nr)
        assert same_bits(r.probe_irradiance(q, nr), plain).all() and same_bits(r.probe_irradiance(q, nr, visibility=False, bias=0.3), plain).all()
        r.query_rejects()
    finally:
        r.close()


def test_lookup_baked_maps():
    rng = np.random.default_rng(9)
    r = _context(*SCENE_CASES["cornell5"])
    try:
        r.bake_probe_field(*FIELD, times=TIMES33[:8], clearance=0.3)
        r.bake_probe_field_visibility(TIMES33)
        desc, sh = r.read_probe_field()
        vis, vr = r.read_probe_field_visibility()
        pts = probe_ref.lattice_points(desc)
        q = rng.uniform(pts[0] - 0.5, pts[-1] + 0.5, (150, 3)).astype(F)
        q[:10] = pts[rng.integers(0, len(pts), 10)]
        v = rng.normal(size=(150, 3))
        nr = (v / np.linalg.norm(v, axis=1)[:, None]).astype(F)
        q[140], nr[141] = (np.nan, 0, 0), (0, 0, 0)
        for bias in (0.0, 0.55):
            want, ok = ref.lookup(desc, sh, vis, q, nr, bias)
            assert (~ok).sum() == 2 and (want[ok, 3] > 0).sum() >= 130
            got = r.probe_irradiance(q, nr, visibility=True, bias=bias)
            assert same_bits(got, want).all() and r.query_rejects() == 2
            host, bad = probe_irradiance_vis_host(desc, sh, vis, q, nr, bias)
            assert host.tobytes() == want.tobytes() and bad == 140
        plain = r.probe_irradiance(q, nr)
        assert (plain[ok] != want[ok]).any(axis=1).sum() > 100 and r.query_rejects() == 2
    finally:
        r.close()


# ---- 5. state ----------------------------------------------------------------------------------------------------
def test_what_drops_the_visibility():
    desc, sh, q, nr, _ = probe_ref.lookup_cases(0)
    vis, rng = ref.lookup_maps(desc)
    q, nr = q[:8], nr[:8]
    r = _context(*SCENE_CASES["cornell5"])
    try:
        def state_error(call):
            with pytest.raises(RMRError) as e:
                call()
            return e.value.code == -5

        def no_vis():
            return (state_error(lambda: r.probe_irradiance(q, nr, visibility=True)) and state_error(r.read_probe_field_visibility)
                    and state_error(lambda: r.probe_irradiance_device(_dev(q), _dev(nr), visibility=True))
                    and r.probe_field_visibility_device() is None)

        # without a field
        assert no_vis() and state_error(lambda: r.bake_probe_field_visibility(TIMES33[:1], RANGE))
        assert state_error(lambda: r.write_probe_field_visibility(vis, rng))
        r.write_probe_field(desc, sh)
        assert no_vis()                                             # a field, no visibility yet
        r.probe_irradiance(q, nr)
        for drop in ("write_probe_field", "bake_probe_field", "probe_field_free", "reload"):
            r.write_probe_field_visibility(vis, rng)
            assert r.probe_irradiance(q, nr, visibility=True).shape == (8, 4)
            if drop == "write_probe_field":
                r.write_probe_field(desc, sh)
            elif drop == "bake_probe_field":
                r.bake_probe_field(*FIELD, times=TIMES33[:1])
                r.sync()
            elif drop == "probe_field_free":
                r.probe_field_free()
            else:
                r.reload()
            assert no_vis(), drop
            if drop in ("write_probe_field", "bake_probe_field"):
                r.probe_irradiance(q, nr)                           # the plain lookup goes on
            r.write_probe_field(desc, sh)
        r.query_rejects()
    finally:
        r.close()


def test_visibility_leaves_everything_else_alone():
    from . import mesh_ref
    rect = (3, 2, 41, 35)
    c = _case("cornell5")
    _, origin, spacing, shape, iso = mesh_ref.CASES["cornell5"]
    r = _context(*SCENE_CASES["cornell5"])
    try:
        r.render_spp(TIMES, rect)
        r.render_guides()
        mesh = r.extract_mesh(origin, spacing, shape)
        r.bake_probe_field(*FIELD, times=TIMES33[:2], clearance=0.3)
        desc, sh = r.read_probe_field()
        q = probe_ref.lattice_points(desc) + F(0.25)
        nr = np.tile(np.array([[0, 1, 0]], F), (len(q), 1))
        plain = r.probe_irradiance(q, nr)
        state = (r.read_accum(), r.read_guides())

        def unchanged(what):
            assert same_bits(r.read_accum(), state[0]).all(), what
            for k, g in r.read_guides().items():
                assert same_bits(g, state[1][k]).all(), (what, k)
            again = r.read_mesh()
            for k in mesh:
                assert again[k].tobytes() == mesh[k].tobytes(), (what, k)
            assert r.read_probe_field()[1].tobytes() == sh.tobytes(), what
            assert same_bits(r.probe_irradiance(q, nr), plain).all(), what      # visibility=False: the same bytes as before

        p = c["p"]
        host = r.bake_probe_visibility(p, TIMES33[:4], RANGE, first_index=FIRST, clearance=c["clearance"])
        unchanged("bake_probe_visibility")
        dp = _dev(p)
        dev = r.bake_probe_visibility_device(dp, TIMES33[:4], 10.0, RANGE, first_index=FIRST, clearance=c["clearance"])
        r.sync()
        assert same_bits(dev.cpu().numpy(), host).all()
        unchanged("bake_probe_visibility_device")
        r.bake_probe_field_visibility(TIMES33[:4])
        vis, rng = r.read_probe_field_visibility()
        r.probe_field_visibility_device()
        unchanged("bake_probe_field_visibility")
        out = r.probe_irradiance(q, nr, visibility=True, bias=0.1)
        dq, dn = _dev(q), _dev(nr)
        dout = r.probe_irradiance_device(dq, dn, visibility=True, bias=0.1)
        r.sync()
        assert same_bits(dout.cpu().numpy(), out).all()
        r.write_probe_field_visibility(vis, rng)
        unchanged("the lookup and write_probe_field_visibility")
        assert r.query_rejects() == 2                       # the NaN probe of the two list calls
    finally:
        r.close()


# ---- 6. errors ---------------------------------------------------------------------------------------------------
def test_state_and_errors():
    p = _points()[:8]
    desc, sh, q, nr, _ = probe_ref.lookup_cases(0)
    vis, rng = ref.lookup_maps(desc)
    r = Renderer(0, W, H)
    try:
        def code(call):
            with pytest.raises(RMRError) as e:
                call()
            return e.value.code

        assert code(lambda: r.bake_probe_visibility(p, TIMES, RANGE)) == -5                     # no scene
        assert code(lambda: r.bake_probe_visibility_device(_dev(p), TIMES, 10.0, RANGE)) == -5
        r.write_probe_field(desc, sh)
        assert code(lambda: r.bake_probe_field_visibility(TIMES, RANGE)) == -5                  # a field, no scene
        r.load_scene(SCENE_CASES["cornell5"][0], "rm1")
        r.set_view(VIEW)
        r.set_params(abi.default_params(max_bounces=4))
        r.probe_field_free()
        assert code(lambda: r.bake_probe_field_visibility(TIMES, RANGE)) == -5                  # a scene, no field
        want = r.bake_probe_visibility(p, TIMES, RANGE)
        assert (want[:, :, 0] > 0).all(axis=1).sum() >= 6
        for bad in (0.0, -1.0, np.nan, np.inf):
            assert code(lambda: r.bake_probe_visibility(p, TIMES, bad)) == -1                   # range
            assert code(lambda: r.bake_probe_visibility_device(_dev(p), TIMES, 10.0, bad)) == -1
        for cl in (np.nan, np.inf, -0.5):
            assert code(lambda: r.bake_probe_visibility(p, TIMES, RANGE, clearance=cl)) == -1
        assert code(lambda: r.bake_probe_visibility(p, TIMES, RANGE, first_index=(1 << 36) - 7)) == -1
        assert code(lambda: r.bake_probe_visibility(p, [], RANGE)) == -1                        # no seeds
        for ext in (-1.0, np.nan, np.inf):
            assert code(lambda: r.bake_probe_visibility_device(_dev(p), TIMES, ext, RANGE)) == -1
        with pytest.raises(ValueError):
            r.bake_probe_visibility_device(_dev(p.astype(np.float64)), TIMES, 10.0, RANGE)
        assert r.bake_probe_visibility(np.zeros((0, 3), F), TIMES, RANGE).shape == (0, 64, 2)   # an empty list is fine
        r.write_probe_field(desc, sh)
        for bad in (0.0, np.nan, np.inf, -2.0):
            assert code(lambda: r.bake_probe_field_visibility(TIMES, bad)) == -1
            assert code(lambda: r.write_probe_field_visibility(vis, bad)) == -1
        assert code(lambda: r.bake_probe_field_visibility([], RANGE)) == -1
        with pytest.raises(ValueError):
            r.write_probe_field_visibility(vis[:-1], rng)
        r.write_probe_field_visibility(vis, rng)
        for bad in (-0.1, np.nan, np.inf):
            assert code(lambda: r.probe_irradiance(q[:4], nr[:4], visibility=True, bias=bad)) == -1
            assert code(lambda: r.probe_irradiance_device(_dev(q[:4]), _dev(nr[:4]), visibility=True, bias=bad)) == -1
        with pytest.raises(ValueError):
            r.probe_irradiance(q, nr[:5], visibility=True)
        assert same_bits(r.bake_probe_visibility(p, TIMES, RANGE), want).all()
        assert r.query_rejects() == 0
    finally:
        r.close()


# ---- 7. rmr_cli --------------------------------------------------------------------------------------------------
def test_cli_probe_visibility(tmp_path):
    """rmr_cli --probes FILE --probe-visibility K[:RANGE] writes the bytes save_probes writes for the same field:
    the version-2 line, the sh payload of --probe-samples seeds, the maps of the schedule's first K seeds."""
    import os
    import subprocess
    from raymarchrenderer_amd import load_probes, save_probes
    from .conftest import ROOT
    cli = os.path.join(ROOT, "raymarchrenderer_amd", "rmr_cli")
    out, path, mine = str(tmp_path / "cli.bmp"), str(tmp_path / "cli.probes"), str(tmp_path / "py.probes")
    base = [cli, "--scene", SCENE_CASES["cornell5"][0], "--variant", "rm1", "--size", "16x16", "--samples", "1", "--grid", "1x1",
            "--bounces", "4", "--frame", "1", "--out", out, "--quiet", "--probes", path, "--probe-bounds", "-2.2,-0.6,-1.8,2.2,3.8,0.4",
            "--probe-grid", "2", "--probe-samples", "3"]
    r = _context(*SCENE_CASES["cornell5"])
    try:
        for opt, rng in (("5", None), ("5:1.75", F(1.75))):
            p = subprocess.run(base + ["--probe-visibility", opt], capture_output=True, text=True, timeout=120)
            assert p.returncode == 0, p.stdout + p.stderr
            desc, sh, vis, got_rng = load_probes(path, visibility=True)
            assert vis.shape == (desc.n[0] * desc.n[1] * desc.n[2], 64, 2)
            assert got_rng == (F(2.6) * F(desc.spacing) if rng is None else rng)
            r.bake_probe_field(desc, times=time_schedule(3, frame=1))
            r.bake_probe_field_visibility(time_schedule(5, frame=1), rng)
            save_probes(mine, desc, r.read_probe_field()[1], *r.read_probe_field_visibility())
            assert open(mine, "rb").read() == open(path, "rb").read(), opt
        # without the flag: the version-1 file, as ever
        p = subprocess.run(base, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and open(path, "rb").read().startswith(b"RMRPROBES 1 ")
        save_probes(mine, desc, r.read_probe_field()[1])
        assert open(mine, "rb").read() == open(path, "rb").read()
    finally:
        r.close()
