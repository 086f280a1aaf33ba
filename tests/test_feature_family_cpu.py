"""The inputs of tests/feature_family.py on the statements alone, no GPU: for every (case, step) pair that
tests/test_gpu_feature_family.py runs, the lists, lattices and views are worth running (the conditions below are
decided by the oracle and the NumPy statements, never by a kernel), and the host forms the library exports (the
bake's fold, the probe fold, rmr_probe_irradiance_host, the visibility's fold and lookup, the AOV fold) give the
statements' bits on these inputs, NaN equal to NaN. That pins the host side of every rule at the family's
magnitudes, so a later mismatch on the GPU is the kernel's and not the rule's.

The march cannot return a distance that is not a number: map() starts from (max_dist, -1) and only ever takes a
smaller value, so every step adds at most max_dist to a finite t (oracle/rmr_oracle.c o_march; a NaN object never
shows in map, tests/test_node_family_cpu.py), as long as max_dist is finite. nan_objects brings a probe where map
is -inf (buried), one on the plane where an object is NaN (used), and pixels that see the -inf / NaN half plane. The
records skipped for a distance that is not finite come from the case nan_objects_inf: the same scene and list
under max_dist = +inf, where every miss marches to t = +inf. A hit has t < max_dist, so the AOV fold, which takes
hits alone, never meets such a distance."""
import numpy as np
import pytest

from raymarchrenderer_amd import (abi, aov_fold, aov_init, bake_fold, probe_fold, probe_irradiance_host,
                                  probe_irradiance_vis_host, probe_vis_fold)

from . import aov_ref, bake_ref, camera_ref, mesh_ref, probe_ref
from . import feature_family as ff
from . import probe_vis_ref as pv
from . import scene_family as sf
from .test_gpu_parity import same_bits

F = np.float32


def _same(got, want, what):
    eq = same_bits(np.asarray(got), np.asarray(want))
    eq = eq.reshape(len(eq), -1).all(axis=1)
    assert eq.all(), "%s: %d/%d entries differ; first %d host=%s statement=%s" % (
        what, (~eq).sum(), len(eq), np.argmin(eq), np.asarray(got)[np.argmin(eq)].ravel()[:4], np.asarray(want)[np.argmin(eq)].ravel()[:4])


# ---- a. the bake's points -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ff.SCENE_CASES)
def test_bake_points(name):
    c = ff.bake_case(name)
    p, n, ok = c["p"], c["n"], c["ok"]
    assert p.dtype == F and n.dtype == F and 129 <= len(p) <= ff.N_LIST
    assert np.flatnonzero(~ok).tolist() == list(c["rejects"])                      # exactly the intended rejects
    assert (n == [0, 1, 0]).all(axis=1).sum() >= 2 and ((n[:, 0] == 0) & (n[:, 2] == 0) & (n[:, 1] < 0)).sum() >= 1
    assert (np.signbit(n[:, 0]) & (n[:, 0] == 0) & (n[:, 1] == 1)).sum() == 1      # (-0, 1, 0)
    nn = (n.astype(np.float64) ** 2).sum(axis=1) - 1.0
    assert ((nn > 0.9e-6) & (nn <= 1e-6)).sum() == 1 and ((nn > 1e-6) & (nn < 1.3e-6)).sum() == 1   # both sides of the bound
    assert (c["rays"]["gx"][0, :7] >= 4090).sum() == 6 and c["rays"]["gy"].max() == 1   # the 4096 wrap inside the list
    # the bias is a few ulps of the coordinates at the far cases, and still moves the origin
    moved = (c["rays"]["o"][0][ok] != p[ok]).any(axis=1)
    assert moved.sum() >= 100, (name, moved.sum())
    blocked, cos = c["blocked"][:, ok], c["c"][:, ok]
    assert blocked.sum() >= 10 and (~blocked).sum() >= 10, (name, blocked.sum())
    L = c["L"][:, ok].reshape(-1, 3)
    assert np.isfinite(L).all() and len(np.unique(L, axis=0)) >= 3 and (L != 0).any(axis=1).all()
    assert (cos > 0).sum() >= 300
    # the host fold and the resolve against the statement
    cv = np.where(c["blocked"], F(0.0), c["c"]).astype(F)
    rgba, ao = bake_fold(c["L"], c["c"], cv)
    w_rgba, w_ao = bake_ref.fold(c["L"], c["c"], cv)
    _same(rgba, w_rgba, "%s: bake fold, radiance" % name)
    _same(ao, w_ao, "%s: bake fold, occlusion" % name)
    r_rgba, r_ao = ff.bake_want(c)
    assert (r_rgba[~ok] == 0).all() and (r_ao[~ok] == 0).all()
    _same(rgba[ok], r_rgba[ok], "%s: bake resolve, radiance" % name)
    _same(ao[ok], r_ao[ok], "%s: bake resolve, occlusion" % name)
    for nspp, m in ((1, 65), (2, 129)):
        w = ff.bake_want(c, nspp, m)
        g = bake_fold(c["L"][:nspp, :m], c["c"][:nspp, :m], cv[:nspp, :m])
        _same(g[0][ok[:m]], w[0][ok[:m]], "%s: bake fold of %d seeds, %d points" % (name, nspp, m))
        _same(g[1][ok[:m]], w[1][ok[:m]], "%s: bake occlusion of %d seeds, %d points" % (name, nspp, m))
    assert len(np.unique(r_ao[ok])) >= 3 and len(np.unique(r_rgba[ok, :3], axis=0)) >= 3
    print("%-13s bake: %d points, %d rejected, %d/%d samples blocked, bias %.3g = %.1f ulp of the largest coordinate" % (
        name, len(p), (~ok).sum(), blocked.sum(), blocked.size, ff.bias(name), ff.bias(name) / np.spacing(F(np.abs(p[ok]).max()))))


# ---- b. the probes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ff.CASES)
def test_probe_lists(name):
    c = ff.probe_case(name)
    p, tb, prm = c["p"], ff.tables(name), ff.params(name)
    assert p.dtype == F and len(p) == ff.N_LIST
    used = ~(c["rejected"] | c["buried"])
    assert used.sum() >= 30
    assert all(c["buried"][i] for i in ff.BURIED) and c["buried"].sum() >= 3
    assert np.flatnonzero(c["rejected"]).tolist() == [ff.NAN]
    # the clearance: the oracle's own map value, used at it (the rule is >=), buried one ulp above it
    cl = c["clearance"]
    assert cl > 0 and np.isfinite(cl) and not c["buried"][ff.AT_CLEARANCE]
    _, b_hi = probe_ref.probe_state(tb, p, ff.above(cl), np.inf, prm.max_dist)
    assert b_hi[ff.AT_CLEARANCE] and (b_hi[np.arange(len(p)) != ff.AT_CLEARANCE] == c["buried"][np.arange(len(p)) != ff.AT_CLEARANCE]).all()
    # the extent: one probe exactly on it, rejected one ulp below it and no other with it
    ext = c["extent"]
    assert np.abs(p[ff.AT_EXTENT]).max() == F(ext)
    r_at, _ = probe_ref.probe_state(tb, p, cl, ext, prm.max_dist)
    r_lo, _ = probe_ref.probe_state(tb, p, cl, ff.below(ext), prm.max_dist)
    assert np.flatnonzero(r_at).tolist() == [ff.NAN] and np.flatnonzero(r_lo).tolist() == [ff.AT_EXTENT, ff.NAN]
    if name == "nan_objects":
        from . import node_family as nf
        assert np.isneginf(nf.oracle_map(tb, p[[ff.NEG_INF]])[0, 0]) and c["buried"][ff.NEG_INF] and used[ff.ON_NAN_PLANE]
    # the radiance
    sh = c["sh"]
    assert (sh[used, 27] == ff.PROBE_SEEDS).all() and (sh[~used] == 0).all()
    fin = np.isfinite(sh).all(axis=1)
    assert fin[used].sum() * 2 >= used.sum() and len(np.unique(sh[used, 0])) >= 3
    assert len(np.unique(c["L"][:, used].reshape(-1, 3), axis=0)) >= 3
    # the host fold against the statement, whole and on the prefixes the GPU test runs
    _same(probe_fold(c["L"][:, used], c["rays"]["d"][:, used]), sh[used], "%s: probe fold" % name)
    for nspp in (1, 8) + ff.CUT_SEEDS:
        w = ff.probe_want(c, nspp)
        _same(probe_fold(c["L"][:nspp, used], c["rays"]["d"][:nspp, used]), w[used], "%s: probe fold of %d seeds" % (name, nspp))
        assert (w[~used] == 0).all()
    assert (ff.probe_want(c, low_extent=True)[ff.AT_EXTENT] == 0).all() and (ff.probe_want(c, high_clearance=True)[ff.AT_CLEARANCE] == 0).all()
    for m in ff.LENGTHS[1:]:
        assert (~(c["rejected"] | c["buried"])[:m]).sum() >= 30, m
    print("%-13s probes: %d used, %d buried, %d rejected, clearance %.6g, extent %.9g" % (
        name, used.sum(), c["buried"].sum(), c["rejected"].sum(), cl, ext))


# ---- c. the visibility --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ff.CASES + (ff.INF_CASE,))
def test_visibility_samples(name):
    c = ff.vis_case(name)
    used, rng = ~c["unused"], c["range"]
    assert rng == F(2.0 * ff.scale(name)) and used.sum() >= 30 and c["unused"].sum() >= 4
    if name == ff.INF_CASE:
        # with max_dist = +inf a miss marches to t = +inf: records the cast writes as NaN and the fold skips, in
        # every tile, at probes that also have finite samples, under every seed count the GPU test cuts at
        assert ff.params(name).max_dist == np.inf
        inf = np.isinf(c["samples"][:, :, 3]) & used[None, :]
        assert not np.isnan(c["samples"][..., 3]).any()
        for nspp in (1, 2, 3, 8, 9, ff.VIS_SEEDS):
            assert all(inf[:nspp, a:a + 64].sum() >= 1 for a in range(0, ff.N_LIST, 64)), nspp
        assert (inf.any(axis=0) & ~inf.all(axis=0)).sum() >= 30
        # the statement skips them: folding the finite samples alone gives the same maps
        only = c["samples"].copy()
        only[inf, 3] = np.nan
        assert same_bits(pv.fold(only, rng), pv.fold(c["samples"], rng)).all()
        # and the skip matters: a fold that clamped them to the range like any far sample gives other maps
        only[inf, 3] = rng
        clamped = same_bits(pv.fold(only, rng), pv.fold(c["samples"], rng)).reshape(ff.N_LIST, -1).all(axis=1)
        assert (~clamped[used]).sum() >= 30
    for nspp in (ff.PROBE_SEEDS, ff.VIS_SEEDS):
        t = c["samples"][:nspp, used, 3]
        fin = np.isfinite(t)
        assert (fin & (t < rng)).sum() >= 10 and (fin & (t >= rng)).sum() >= 10, (name, nspp)
    d = c["samples"][:, used, :3].reshape(-1, 3)
    assert (d.min(axis=0) < -0.9).all() and (d.max(axis=0) > 0.9).all()
    want = ff.vis_want(c)
    assert (want[~used] == 0).all() and (want[used, :, 0] > 0).all()
    assert (want[used, :, 0] == rng).any() and (want[used, :, 0] < rng).any()      # both sides of the clamp
    _same(probe_vis_fold(c["samples"][:, used], rng), want[used], "%s: visibility fold" % name)
    for m in (ff.LENGTHS if name in ff.GRID_CASES else (129, ff.N_LIST)):
        for nspp in (ff.SEED_COUNTS + ff.CUT_SEEDS if name in ff.GRID_CASES else (8, 9) + ff.CUT_SEEDS):
            u = used[:m]
            w = ff.vis_want(c, nspp, m)
            if u.any():
                _same(probe_vis_fold(c["samples"][:nspp, :m][:, u], rng), w[u], "%s: visibility fold, %d probes, %d seeds" % (name, m, nspp))
            assert (w[~u] == 0).all()
    t = c["samples"][:, used, 3]
    print("%-13s visibility: range %.6g, %d distances below it, %d at or above it, %d not finite" % (
        name, rng, (t < rng).sum(), (t >= rng).sum(), (~np.isfinite(t)).sum()))


# ---- d. the lookups -----------------------------------------------------------------------------------------
def _fields(name):
    desc = ff.lattice(name)
    syn = ff.synthetic_field()
    syn_vis, syn_rng = ff.synthetic_maps(desc, syn)
    _, sh, vis, rng = ff.baked_field(name)
    return desc, (("synthetic", syn, syn_vis, syn_rng), ("baked", sh, vis, rng))


@pytest.mark.parametrize("name", ff.SCENE_CASES)
def test_lookup_queries(name):
    desc, fields = _fields(name)
    q, nr, groups = ff.lookup_queries(name)
    assert q.dtype == F and nr.dtype == F and tuple(groups) == ff.GROUPS
    assert all(b > a for a, b in groups.values())                                   # every group is non-empty
    ok = bake_ref.point_ok(q, nr)
    a, b = groups["rejected"]
    assert np.flatnonzero(~ok).tolist() == list(range(a, b))
    # a lattice point and its float neighbour fall in different cells; away from the origin many queries share a
    # float with a neighbour on the other side of a cell's face
    on = ff.cells(desc, q[slice(*groups["on_lattice"])])
    lo_ = ff.cells(desc, q[slice(*groups["neighbour_below"])]).reshape(3, -1, 3)
    hi_ = ff.cells(desc, q[slice(*groups["neighbour_above"])]).reshape(3, -1, 3)
    split = sum(int((lo_[k][:, k] != on[:, k]).sum() + (hi_[k][:, k] != on[:, k]).sum()) for k in range(3))
    assert split >= 1, name
    pts = probe_ref.lattice_points(desc)
    o, f = groups["outside"]
    assert ((q[o:f] < pts[0]) | (q[o:f] > pts[-1])).any(axis=1).all()
    o, f = groups["faces"]
    assert ((q[o:f] == pts[0]) | (q[o:f] == pts[-1])).any(axis=1).all()
    # a kernel that multiplied by 1 / spacing would be seen: it puts some query into other weights
    sp = F(desc.spacing)
    rcp = F(1.0) / sp
    differ = 0
    for k in range(3):
        qq = q[ok, k]
        with np.errstate(invalid="ignore", over="ignore"):
            differ += int((((qq - F(desc.origin[k])).astype(F) / sp).astype(F) != ((qq - F(desc.origin[k])).astype(F) * rcp).astype(F)).sum())
    assert differ >= 1, name
    counts = {}
    for label, sh, vis, rng in fields:
        valid = ff.corner_validity(desc, sh, q)
        want, ok2 = probe_ref.lookup(desc, sh, q, nr)
        assert (ok2 == ok).all()
        some = ok & valid.any(axis=1) & ~valid.all(axis=1)
        none = ok & (want[:, 3] == 0)
        assert some.sum() >= 1 and none.sum() >= 1 and (ok & (want[:, 3] > 0)).sum() >= 500, (name, label)
        if label == "synthetic":
            a, b = groups["some_invalid"]
            assert some[a:b].all()
            a, b = groups["all_invalid"]
            assert none[a:b].all() and not valid[a:b].any()
        host, bad = probe_irradiance_host(desc, sh, q, nr)
        assert bad == groups["rejected"][0]
        _same(host, want, "%s: lookup, %s field" % (name, label))
        assert len(np.unique(want[ok, :3], axis=0)) >= 100
        for bias in (0.0, float(F(0.25) * sp)):
            wv, _ = pv.lookup(desc, sh, vis, q, nr, bias)
            hv, bad = probe_irradiance_vis_host(desc, sh, vis, q, nr, bias)
            assert bad == groups["rejected"][0]
            _same(hv, wv, "%s: weighted lookup, %s field, bias %.4g" % (name, label, bias))
            assert (wv[ok] != want[ok]).any(axis=1).sum() >= 100, (name, label, bias)   # the maps matter
        counts[label] = (int(some.sum()), int(none.sum()))
    print("%-13s lookups: %d queries, %d neighbour pairs in different cells, %d coordinates a reciprocal would move; "
          "some / all corners invalid: synthetic %s, baked %s" % (name, len(q), split, differ, counts["synthetic"], counts["baked"]))


# ---- e. the AOVs --------------------------------------------------------------------------------------------
def _view_rays(name, model, **fields):
    """The float64 statement of the camera's rays over RECT0 (tests/camera_ref.py), rounded: close to the
    library's own rays, which the GPU test reads back; enough to decide what the view sees."""
    o, d, rc = camera_ref.rays(model, ff.view(name), sf.W0, sf.H0, sf.times(), sf.RECT0, **fields)
    rays = np.zeros(o.shape[:3], np.dtype(abi.RAY_DTYPE))
    rays["o"], rays["d"] = o.astype(F), d.astype(F)
    return rays


@pytest.mark.parametrize("name", ff.AOV_CASES)
def test_aov_views(name):
    tb, prm = ff.tables(name), ff.params(name)
    models = [("view", camera_ref.VIEW, {})] + ([("thinlens", camera_ref.THIN_LENS, ff.lens(name))] if name == ff.LENS_CASE else [])
    for label, model, fields in models:
        rays = _view_rays(name, model, **fields)
        n_px = rays.shape[1] * rays.shape[2]
        hits = aov_ref.oracle_hits(tb, prm, rays).reshape(len(rays), n_px)
        is_hit = hits["id"] >= 0
        assert is_hit.sum() >= 200 and (~is_hit).sum() >= 50, (name, label)
        assert np.isfinite(hits["t"]).all() and len(np.unique(hits["id"][is_hit])) >= 3
        want = aov_ref.fold(aov_ref.init(n_px), hits)
        _same(aov_fold(aov_init(n_px), hits).reshape(5 * n_px, 4), want.reshape(5 * n_px, 4), "%s %s: AOV fold" % (name, label))
        mixed = (is_hit.any(axis=0) & ~is_hit.all(axis=0)).sum()
        assert mixed >= 1, (name, label)                          # a pixel whose samples both hit and miss
        if name == "nan_objects":
            # the slab's visible surface is the half plane where its distance jumps from +inf to -inf
            assert (hits["id"] == 4).sum() >= 50
        print("%-13s AOV %s: %d hits, %d misses, %d pixels with both, ids %s" % (
            name, label, is_hit.sum(), (~is_hit).sum(), mixed, np.unique(hits["id"]).tolist()))


# ---- f, g. the guides' and the volume's cases ---------------------------------------------------------------
@pytest.mark.parametrize("name", ff.GUIDE_CASES)
def test_guide_views(name):
    e, dirs, t, ident, pos = sf.primary_hits(name)
    assert (ident >= 0).sum() >= 100 and (ident < 0).sum() >= 50 and len(np.unique(ident)) >= 4


@pytest.mark.parametrize("name", ff.VOLUME_CASES)
def test_volume_lattices(name):
    origin, spacing, shape = ff.volume(name)
    assert shape[0] * shape[1] * shape[2] > 256 and (shape[0] * shape[1] * shape[2]) % 64 != 0
    dist, ids = mesh_ref.oracle_volume(ff.tables(name), origin, spacing, shape, ff.params(name).max_dist)
    assert (dist < 0).sum() >= 50 and (dist > 0).sum() >= 500 and set(np.unique(ids)) >= {0.0, 3.0}   # the floor and the ball
    m = mesh_ref.surface_nets(dist, origin, spacing, 0.0)
    assert len(m["vertices"]) >= 100 and len(m["quads"]) >= 100
    print("%-13s volume: %d inside, %d vertices, %d quads" % (name, (dist < 0).sum(), len(m["vertices"]), len(m["quads"])))
