"""Irradiance probes on the GPU (include/rmr.h rmr_bake_probes / rmr_probe_irradiance), every
comparison bit for bit against tests/probe_ref.py (the oracle's sphere directions, map and trace, the NumPy fold
and lookup): the generated rays, the list bake on Cornell-5 with buried and rejected probes under the default
plane budget, a budget that cuts inside a probe's samples, and the hipRTC kernel; a node-program scene and an RM2
scene; the field form against the list form; the lookup on a synthetic and on a baked field; that nothing else
moved; and the errors."""
import numpy as np
import pytest

from raymarchrenderer_amd import Renderer, RMRError, abi, probe_irradiance_host, time_schedule

from . import probe_ref as ref
from .test_gpu_parity import _tables, same_bits
from .test_gpu_rays import H, SCENE_CASES, TIMES, VIEW, W, _context, _oracle

pytestmark = pytest.mark.gpu

F = np.float32
TIMES33 = time_schedule(33, frame=1)
TILE_BYTES = 64 * 64                    # one tile-sample in the plane budget
FIRST = 4090                            # gx wraps and gy steps inside the list
EXTENT = 5.0                            # the device forms' bound: probe BEYOND lies outside it
BURIED = {3: (1.0, -1.03, 1.0), 63: (-3.0, 1.0, 0.5), 64: (3.01, 2.0, -1.0)}   # inside the floor and the two walls
AT_CLEARANCE, NAN, BEYOND = 17, 65, 79
FIELD = ((-2.2, -0.6, -1.8), 1.1, (5, 4, 4))

_cache = {}


def _dev(a):
    """A host array as a torch tensor on the GPU (the caller keeps it alive until r.sync())."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cornell():
    """Once: 80 probes in Cornell-5 (two tiles, the second partial) with three inside the boxes, one whose distance
    is exactly the call's clearance, one NaN and one beyond the device forms' extent; the reference's bake of them
    with 33 seeds, first_index FIRST and no extent."""
    if "cornell" in _cache:
        return _cache["cornell"]
    path, variant, params = SCENE_CASES["cornell5"]
    tables = _tables(path, variant)
    prm = abi.default_params(**params)
    rng = np.random.default_rng(41)
    p = np.stack([rng.uniform(-2.8, 2.8, 80), rng.uniform(-0.9, 3.8, 80), rng.uniform(-3.0, 3.0, 80)], axis=1).astype(F)
    for i, v in BURIED.items():
        p[i] = v
    p[AT_CLEARANCE] = (1.5, -0.9, 0.7)            # 0.075 above the floor
    p[NAN] = (0.5, np.nan, 0.5)
    p[BEYOND] = (0.5, 1.0, 9.0)
    from oracle import oracle
    clearance = float(oracle.map_p(tables, p[AT_CLEARANCE], prm.max_dist)[0])
    assert 0.07 < clearance < 0.08
    sh, rejected, buried = ref.bake(_oracle(path, variant, params), tables, p, TIMES33, FIRST, clearance, np.inf, prm.max_dist)
    case = {"p": p, "clearance": clearance, "sh": sh, "rejected": rejected, "buried": buried, "tables": tables, "prm": prm}
    _cache["cornell"] = case
    return case


def _want(case, extent):
    """The reference's bake with the device forms' extent: the probe beyond it is rejected as well."""
    sh = case["sh"].copy()
    if extent < 9.0:
        sh[BEYOND] = 0
    return sh


def test_probes_cover_the_cases():
    c = _cornell()
    assert c["rejected"].nonzero()[0].tolist() == [NAN]
    assert all(c["buried"][i] for i in BURIED) and not c["buried"][AT_CLEARANCE] and not c["buried"][BEYOND]
    assert 3 <= c["buried"].sum() <= 20                    # the three, and whatever lies within the clearance or in the sphere
    used = ~(c["rejected"] | c["buried"])
    assert (c["sh"][used, 27] == 33).all() and (c["sh"][~used] == 0).all()
    assert np.isfinite(c["sh"]).all() and len(np.unique(c["sh"][used, 0])) > 40
    assert (np.abs(c["sh"][used, 3:27]).max(axis=1) > 0).all()


# ---- 1. the rays -------------------------------------------------------------------------------------------------
def test_rays_bitexact():
    c = _cornell()
    p = c["p"]
    unused = c["rejected"] | c["buried"]
    want = ref.rays(p, TIMES33[:5], FIRST, unused)
    assert want["gx"][0, 5] == 4095 and want["gx"][0, 6] == 0 and want["gy"][0, 6] == 1
    r = _context(*SCENE_CASES["cornell5"])
    try:
        dp = _dev(p)
        got = r.probe_rays_device(dp, TIMES33[:5], first_index=FIRST, clearance=c["clearance"])
        r.sync()
        got = got.cpu().numpy().view(np.dtype(abi.RAY_DTYPE)).reshape(5, len(p))
        for k in ("o", "d", "time", "rc", "gx", "gy"):
            assert same_bits(got[k], want[k]).all(), (k, np.argwhere(got[k] != want[k])[:3])
        assert (got["gx"][:, unused] == -1).all() and (got["gx"][:, ~unused] >= 0).all()
        assert r.query_rejects() == 1                       # the NaN probe, once: buried probes are not counted
        # without a clearance the probe above the floor's neighbours come back, the boxes' insides stay out
        g0 = r.probe_rays_device(dp, TIMES33[:1])
        r.sync()
        g0 = g0.cpu().numpy().view(np.dtype(abi.RAY_DTYPE)).reshape(len(p))
        assert all(g0["gx"][i] == -1 for i in BURIED) and (g0["gx"] >= 0).sum() >= (~unused).sum()
        # the directions cover the sphere: both signs on every axis for one probe's five samples' neighbours
        d = got["d"][:, ~unused].reshape(-1, 3)
        assert (d.min(axis=0) < -0.9).all() and (d.max(axis=0) > 0.9).all()
        assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1).max() <= 1e-6
    finally:
        r.close()


# ---- 2. the list bake on Cornell-5 -------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["default", "cut", "jit"])
def test_list_bake_cornell(mode):
    c = _cornell()
    p = c["p"]
    r = _context(*SCENE_CASES["cornell5"], jit=1 if mode == "jit" else 0)
    try:
        per_launch = [None] if mode != "cut" else [5, 1, 40]    # cuts inside a probe's 33 samples and inside the list
        for pl in per_launch:
            if pl:
                r.set_tuning(samp_budget=pl * TILE_BYTES)
            t0 = r.stats().trace_launches
            dp = _dev(p)
            got = r.bake_probes_device(dp, TIMES33, EXTENT, first_index=FIRST, clearance=c["clearance"])
            r.sync()
            got = got.cpu().numpy()
            if pl:
                assert r.stats().trace_launches - t0 == -(-2 * 33 // pl), pl
            want = _want(c, EXTENT)
            eq = same_bits(got, want).all(axis=1)
            assert eq.all(), "%s %s: %d probes differ, first %d gpu %s cpu %s" % (
                mode, pl, (~eq).sum(), np.argmin(eq), got[np.argmin(eq)][:4], want[np.argmin(eq)][:4])
            assert r.query_rejects() == 2                   # the NaN and the one beyond the extent, once each
            # the host form takes the extent from the list: only the NaN is rejected
            host = r.bake_probes(p, TIMES33, first_index=FIRST, clearance=c["clearance"])
            assert same_bits(host, c["sh"]).all() and r.query_rejects() == 1
        if mode == "jit":
            assert r.stats().jit_launches > 0
        if mode == "default":
            # a slice baked with first_index gives the bytes of the whole; fewer seeds are a prefix's fold
            for a, b in ((0, 64), (64, 70), (70, 80)):
                part = r.bake_probes(p[a:b], TIMES33, first_index=FIRST + a, clearance=c["clearance"])
                assert same_bits(part, c["sh"][a:b]).all(), (a, b)
            one = r.bake_probes(p, TIMES33[:1], first_index=FIRST, clearance=c["clearance"])
            assert set(np.unique(one[:, 27])) == {0.0, 1.0}
            r.query_rejects()
    finally:
        r.close()


# ---- 3. a node-program scene and an RM2 scene --------------------------------------------------------------------
@pytest.mark.parametrize("name", ["csg_nodes", "simple_rm2"])
def test_other_scenes(name):
    path, variant, params = SCENE_CASES[name]
    tables = _tables(path, variant)
    prm = abi.default_params(**params)
    rng = np.random.default_rng(5)
    p = np.stack([rng.uniform(-2.5, 2.5, 10), rng.uniform(-0.5, 3.0, 10), rng.uniform(-2.5, 2.5, 10)], axis=1).astype(F)
    p[4] = (0.0, 1.0, 0.0) if name == "simple_rm2" else (-1.4827238, -0.53426456, 1.2518233)    # inside a shape
    want, rejected, buried = ref.bake(_oracle(path, variant, params), tables, p, TIMES33[:5], 7, 0.0, np.inf, prm.max_dist)
    assert buried[4] and not rejected.any() and (~buried).sum() >= 6
    r = _context(path, variant, params)
    try:
        got = r.bake_probes(p, TIMES33[:5], first_index=7)
        eq = same_bits(got, want).all(axis=1)
        assert eq.all(), "%s: %d probes differ, first %d gpu %s cpu %s" % (
            name, (~eq).sum(), np.argmin(eq), got[np.argmin(eq)][:4], want[np.argmin(eq)][:4])
        assert r.query_rejects() == 0
    finally:
        r.close()


# ---- 4. the field ------------------------------------------------------------------------------------------------
def test_field_form():
    desc = abi.volume_desc(*FIELD)
    pts = ref.lattice_points(desc)
    r = _context(*SCENE_CASES["cornell5"])
    try:
        def state_error(call):
            with pytest.raises(RMRError) as e:
                call()
            return e.value.code == -5

        q1, n1 = np.zeros((1, 3), F), np.array([[0, 1, 0]], F)
        assert state_error(r.read_probe_field) and state_error(lambda: r.probe_irradiance(q1, n1))
        assert state_error(lambda: r.probe_irradiance_device(_dev(q1), _dev(n1))) and r.probe_field_device() is None
        r.bake_probe_field(*FIELD, times=TIMES33[:5])
        d, sh = r.read_probe_field()
        assert bytes(d) == bytes(desc) and sh.shape == (80, 28)
        want = r.bake_probes(pts, TIMES33[:5])
        assert same_bits(sh, want).all()
        buried = want[:, 27] == 0
        assert 1 <= buried.sum() <= 12 and (want[~buried, 27] == 5).all()      # (lattice points inside the sphere)
        dev = r.probe_field_device()
        r.sync()
        assert same_bits(dev.cpu().numpy(), sh).all()
        # a second bake replaces the field; a clearance buries more
        r.bake_probe_field(desc, times=TIMES33[:2], clearance=0.4)
        sh2 = r.read_probe_field()[1]
        assert same_bits(sh2, r.bake_probes(pts, TIMES33[:2], clearance=0.4)).all() and (sh2[:, 27] == 0).sum() > buried.sum()
        # write then read returns the bytes, whatever they are
        cdesc, csh, _, _, _ = ref.lookup_cases(0)
        csh[7, 3] = np.nan
        r.write_probe_field(cdesc, csh)
        d, back = r.read_probe_field()
        assert bytes(d) == bytes(cdesc) and back.tobytes() == csh.tobytes()
        r.probe_field_free()
        assert state_error(r.read_probe_field) and r.probe_field_device() is None
        r.probe_field_free()                                                    # (nothing to free: fine)
        r.write_probe_field(cdesc, csh)
        r.reload()
        assert state_error(r.read_probe_field) and state_error(lambda: r.probe_irradiance(q1, n1))
        # the errors of the field form
        for bad in (((0, 0, 0), 1.0, (1, 4, 4)), ((0, 0, 0), 0.0, (4, 4, 4)), ((np.nan, 0, 0), 1.0, (4, 4, 4))):
            with pytest.raises(RMRError) as e:
                r.bake_probe_field(abi.volume_desc(*bad), times=TIMES33[:1])
            assert e.value.code == -1
        with pytest.raises(RMRError) as e:
            r.bake_probe_field(desc, times=TIMES33[:1], first_index=3)
        assert e.value.code == -1 and state_error(r.read_probe_field)
        assert r.query_rejects() == 0
    finally:
        r.close()


# ---- 5. the lookup -----------------------------------------------------------------------------------------------
def test_lookup_synthetic_field():
    desc, sh, q, nr, groups = ref.lookup_cases()
    assert len(q) == 200 and len(q) % 64 != 0
    want, ok = ref.lookup(desc, sh, q, nr)
    host, bad = probe_irradiance_host(desc, sh, q, nr)
    assert host.tobytes() == want.tobytes() and bad == groups["rejected"][0]
    r = Renderer(0, W, H)                       # no scene: the lookup needs none
    try:
        r.write_probe_field(desc, sh)
        got = r.probe_irradiance(q, nr)
        eq = same_bits(got, want).all(axis=1)
        assert eq.all(), "%d queries differ, first %d gpu %s cpu %s" % ((~eq).sum(), np.argmin(eq), got[np.argmin(eq)], want[np.argmin(eq)])
        assert r.query_rejects() == (~ok).sum() == 10
        dq, dn = _dev(q), _dev(nr)
        dev = r.probe_irradiance_device(dq, dn)
        r.sync()
        assert same_bits(dev.cpu().numpy(), want).all() and r.query_rejects() == 10
        for m in (1, 63, 64, 65):
            assert same_bits(r.probe_irradiance(q[:m], nr[:m]), want[:m]).all(), m
        assert r.probe_irradiance(q[:0], nr[:0]).shape == (0, 4)
        with pytest.raises(ValueError):
            r.probe_irradiance(q, nr[:5])
    finally:
        r.close()


def test_lookup_baked_field():
    rng = np.random.default_rng(9)
    r = _context(*SCENE_CASES["cornell5"])
    try:
        r.bake_probe_field(*FIELD, times=TIMES33[:8])
        desc, sh = r.read_probe_field()
        pts = ref.lattice_points(desc)
        q = rng.uniform(pts[0] - 0.5, pts[-1] + 0.5, (150, 3)).astype(F)
        q[:20] = pts[rng.integers(0, len(pts), 20)]
        v = rng.normal(size=(150, 3))
        nr = (v / np.linalg.norm(v, axis=1)[:, None]).astype(F)
        want, ok = ref.lookup(desc, sh, q, nr)
        # (some cells have buried corners; a query on a buried lattice point has no valid corner at all)
        assert ok.all() and (want[:, 3] > 0).sum() >= 140 and ((want[:, 3] > 0) & (want[:, 3] < 0.99)).any()
        got = r.probe_irradiance(q, nr)
        assert same_bits(got, want).all()
        assert len(np.unique(got[:, :3], axis=0)) > 100 and (got[:, :3].max(axis=0) > 0).all()
    finally:
        r.close()


# ---- 6. nothing else moves ---------------------------------------------------------------------------------------
def test_probes_leave_everything_else_alone():
    from . import mesh_ref
    rect = (3, 2, 41, 35)
    c = _cornell()
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
        r.bake_mesh(TIMES[:1], radiance=True, ao=True)
        mb = r.read_mesh_bake(rgba=True, ao=True)
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
            again = r.read_mesh_bake(rgba=True, ao=True)
            assert again["rgba"].tobytes() == mb["rgba"].tobytes() and again["ao"].tobytes() == mb["ao"].tobytes(), what

        p = c["p"]
        got = r.bake_probes(p, TIMES33[:4], first_index=FIRST, clearance=c["clearance"])
        unchanged("bake_probes")
        dp = _dev(p)
        dev = r.bake_probes_device(dp, TIMES33[:4], 10.0, first_index=FIRST, clearance=c["clearance"])
        rays = r.probe_rays_device(dp, TIMES33[:4], first_index=FIRST, clearance=c["clearance"])
        r.sync()
        assert same_bits(dev.cpu().numpy(), got).all() and rays.shape == (4 * 80, 10)
        unchanged("the device forms")
        r.bake_probe_field(*FIELD, times=TIMES33[:2])
        desc, sh = r.read_probe_field()
        r.probe_field_device()
        unchanged("bake_probe_field")
        q = ref.lattice_points(desc)[:70] + F(0.25)
        nr = np.tile(np.array([[0, 1, 0]], F), (70, 1))
        out = r.probe_irradiance(q, nr)
        dq, dn_ = _dev(q), _dev(nr)
        dout = r.probe_irradiance_device(dq, dn_)
        r.sync()
        assert same_bits(dout.cpu().numpy(), out).all()
        r.write_probe_field(desc, sh)
        unchanged("the lookup and write_probe_field")
        r.probe_field_free()
        unchanged("probe_field_free")
        assert r.query_rejects() == 3                       # the NaN probe of the three list calls
        # a following render finds a clean work queue: the same bits as a context that never baked
        r.render_spp(TIMES[:1], rect, first_sample=4)
        after = r.read_accum()
        fresh.set_error_estimate(True)
        fresh.render_spp(TIMES, rect)
        fresh.render_spp(TIMES[:1], rect, first_sample=4)
        assert same_bits(after, fresh.read_accum()).all() and not same_bits(after, state[0]).all()
    finally:
        r.close()
        fresh.close()


# ---- 7. errors ---------------------------------------------------------------------------------------------------
def test_state_and_errors():
    c = _cornell()
    p = c["p"][:8]
    r = Renderer(0, W, H)
    try:
        def code(call):
            with pytest.raises(RMRError) as e:
                call()
            return e.value.code

        assert code(lambda: r.bake_probes(p, TIMES)) == -5                          # no scene
        assert code(lambda: r.bake_probes_device(_dev(p), TIMES, 10.0)) == -5
        assert code(lambda: r.probe_rays_device(_dev(p), TIMES)) == -5
        assert code(lambda: r.bake_probe_field(*FIELD, times=TIMES)) == -5
        r.load_scene(SCENE_CASES["cornell5"][0], "rm1")
        r.set_view(VIEW)
        r.set_params(abi.default_params(max_bounces=4, separate_channels=1))
        assert code(lambda: r.bake_probes(p, TIMES)) == -5                          # separate_channels
        assert "separate_channels" in r.lib.rmr_last_error(r.ctx).decode()
        assert code(lambda: r.bake_probe_field(*FIELD, times=TIMES)) == -5
        r.set_params(abi.default_params(max_bounces=4))
        want = r.bake_probes(p, TIMES)
        assert (want[:, 27] == 4).sum() >= 6
        for cl in (np.nan, np.inf, -0.5):
            assert code(lambda: r.bake_probes(p, TIMES, clearance=cl)) == -1
            assert code(lambda: r.probe_rays_device(_dev(p), TIMES, clearance=cl)) == -1
        assert code(lambda: r.bake_probes(p, TIMES, first_index=(1 << 36) - 7)) == -1        # idx >= 2^36
        assert code(lambda: r.bake_probes(p, TIMES, first_index=1 << 40)) == -1
        assert (r.bake_probes(p, TIMES, first_index=(1 << 36) - 8)[:, 27] == want[:, 27]).all()   # the last valid slice
        assert code(lambda: r.bake_probes(p, [])) == -1                                      # no seeds
        for ext in (-1.0, np.nan, np.inf):
            assert code(lambda: r.bake_probes_device(_dev(p), TIMES, ext)) == -1             # origin_extent
        with pytest.raises(ValueError):
            r.bake_probes(p, TIMES, params=abi.probe_params(), clearance=0.1)   # params and keywords: one or the other
        with pytest.raises(ValueError):
            r.bake_probes_device(_dev(p.astype(np.float64)), TIMES, 10.0)
        assert r.bake_probes(np.zeros((0, 3), F), TIMES).shape == (0, 28)                    # an empty list is fine
        assert same_bits(r.bake_probes(p, TIMES), want).all()
        assert r.query_rejects() == 0
    finally:
        r.close()
