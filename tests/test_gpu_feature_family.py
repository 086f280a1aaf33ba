"""The kernels built on the trace and query kernels, on the generated families (tests/feature_family.py): the
light bake, the irradiance probes, their visibility, both lookups, the sampled AOVs, the guide planes, volumes and
meshes, with scenes scaled by 0.02 to 200 and moved up to 16384 from the origin, a ground sphere of radius 10^4,
exact ties, node-program materials and node-program objects. Every other test of these features sits at extent 4
to 10 about the origin with lists of 70 and a dyadic lattice. Here

  a. bake_points radiance and occlusion (table kernel everywhere, hipRTC kernel on three cases), the generated
     rays, the reject count, lists of 1, 63, 64, 65 and 129 points and the whole list (143 points, 151 on the
     ground sphere), the whole list cut into launches of 1 and 5 tile-samples;
  b. the probe bake's list, device and field forms and its rays, both sides of the extent and clearance boundaries,
     lists of 1 to 200 probes with 1 to 9 seeds, cut into launches of 1 and 5 tile-samples;
  c. the visibility's list, device and field forms; on two cases every list length of 1, 63, 64, 65, 129, 200 with
     1, 2, 3, 8, 9 and 16 records per probe under the default budget and budgets of 1 and 5 tile-samples per launch;
     and nan_objects under max_dist = +inf, where half the records are misses at t = +inf that the fold skips;
  d. both lookups on the case's lattice (origin float32(s (-2.2, -0.6, -1.8) + T), spacing float32(1.1 s)) with the
     baked and with a synthetic field, host and device-tensor forms;
  e. render_aov's raw planes, one run under the thin lens, cut into launches and calls;
  f. the guide planes against cast_rays of the same rays;
  g. the volume and the surface-nets mesh around the ball and the floor.

Every comparison is bit for bit (NaN equals NaN) against the NumPy statements over the CPU oracle; the only bound
is mesh_ref.position_bound, the mesh's own. tests/test_feature_family_cpu.py shows on the statements alone that
the inputs are worth running and that the host forms agree with the statements on them. One line per case goes to
the log with its counts."""
import numpy as np
import pytest

from raymarchrenderer_amd import abi

from . import aov_ref, mesh_ref, probe_ref
from . import feature_family as ff
from . import probe_vis_ref as pv
from . import scene_family as sf
from .denoise_ref import oracle_normals
from .test_gpu_bake import TILE_BYTES
from .test_gpu_parity import same_bits
from .test_gpu_probe_vis import UNIT_TILE_BYTES
from .test_gpu_query import _map, _view_rays

pytestmark = pytest.mark.gpu

F = np.float32
DEFAULT_BUDGET = 48 << 30               # rmr_api.cpp: the context's plane budget until rmr_set_tuning names one
RAY = np.dtype(abi.RAY_DTYPE)

STEPS = ("bake", "probes", "visibility", "lookups", "aov", "guides", "volume")
APPLIES = {"bake": ff.SCENE_CASES, "probes": ff.CASES, "visibility": ff.CASES + (ff.INF_CASE,), "lookups": ff.SCENE_CASES,
           "aov": ff.AOV_CASES, "guides": ff.GUIDE_CASES, "volume": ff.VOLUME_CASES}
ORDER = list(ff.CASES) + [ff.INF_CASE] + [n for n in ff.GUIDE_CASES + ff.VOLUME_CASES if n not in ff.CASES]
PAIRS = [(name, step) for name in ORDER for step in STEPS if name in APPLIES[step]]

_loaded = {"name": None}
_counts = {}


def _dev(a):
    """A copy of a host array (the family's are read-only) as a torch tensor on the GPU; the caller keeps it alive
    until r.sync()."""
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _assert_same(got, want, case, step, what):
    """Bit for bit over the entries of the first axis; the case, the step, the number of differing entries, the
    first of them and its GPU and CPU values. Adds the count to the case's line."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, "%s %s: %s: %s %s, the statement gives %s %s" % (
        case, step, what, got.dtype, got.shape, want.dtype, want.shape)
    eq = same_bits(got, want)
    eq = eq.reshape(len(eq), -1).all(axis=1) if eq.ndim > 1 else eq
    _counts.setdefault(case, {}).setdefault("differing", 0)
    _counts[case]["differing"] += int((~eq).sum())
    _counts[case]["compared"] = _counts[case].get("compared", 0) + 1
    assert eq.all(), "%s %s: %s: %d/%d entries differ; first %d gpu=%s cpu=%s" % (
        case, step, what, (~eq).sum(), len(eq), np.argmin(eq), got[np.argmin(eq)].ravel()[:6], want[np.argmin(eq)].ravel()[:6])


def _note(case, **kw):
    _counts.setdefault(case, {}).update(kw)


def _load(r, name):
    """The case in the session's context, once per case: the steps of a case follow each other."""
    if _loaded["name"] == name:
        return
    _loaded["name"] = None
    r.set_image_size(sf.W0, sf.H0)
    r.reload()
    r.load_scene(ff.scene(name), "rm1")
    r.set_params(ff.params(name))
    r.set_view(ff.view(name))
    r.set_env_map(None)
    r.set_camera_model("view")
    r.query_rejects()
    _loaded["name"] = name


def _restore(r):
    r.set_jit(2)
    r.set_tuning(samp_budget=DEFAULT_BUDGET)
    r.set_query_grid(0)
    r.set_aov_launch_samples(6)
    r.set_camera_model("view")
    r.query_rejects()


def _ray_fields(got, want, case, step, what):
    got = got.cpu().numpy().view(RAY).reshape(want.shape)
    for k in ("o", "d", "time", "rc", "gx", "gy"):
        _assert_same(got[k].reshape(-1, *got[k].shape[2:]), want[k].reshape(-1, *want[k].shape[2:]), case, step, "%s, field %s" % (what, k))
    assert got.tobytes() == want.tobytes(), (case, step, what)


# ---- a. the bake --------------------------------------------------------------------------------------------
def _bake(r, name):
    c = ff.bake_case(name)
    p, n, ok = c["p"], c["n"], c["ok"]
    times = ff.seeds(ff.BAKE_SEEDS)
    kw = dict(bias=ff.bias(name), ao_distance=ff.ao_distance(name), first_index=ff.FIRST)
    n_rej = len(c["rejects"])
    want_rgba, want_ao = ff.bake_want(c)
    for jit in ((0, 1) if name in ff.JIT_CASES else (0,)):
        r.set_jit(jit)
        r.reset_stats()
        got = r.bake_points(p, n, times, radiance=True, ao=True, **kw)
        st = r.stats()
        assert st.trace_launches > 0 and (st.jit_launches > 0) == bool(jit), (name, jit, st.jit_launches)
        _assert_same(got["rgba"], want_rgba, name, "bake", "radiance, jit %d" % jit)
        _assert_same(got["ao"], want_ao, name, "bake", "occlusion, jit %d" % jit)
        assert r.query_rejects() == n_rej, (name, jit)
    r.set_jit(0)
    for m in (1, 63, 64, 65, 129):
        for nspp in (1, ff.BAKE_SEEDS):
            w = ff.bake_want(c, nspp, m)
            got = r.bake_points(p[:m], n[:m], times[:nspp], radiance=True, ao=True, **kw)
            _assert_same(got["rgba"], w[0], name, "bake", "radiance, %d points, %d seeds" % (m, nspp))
            _assert_same(got["ao"], w[1], name, "bake", "occlusion, %d points, %d seeds" % (m, nspp))
    r.query_rejects()
    tiles = -(-len(p) // 64)
    for per_launch in (1, 5):
        for nspp in (1, ff.BAKE_SEEDS):
            w = ff.bake_want(c, nspp)
            r.set_tuning(samp_budget=per_launch * TILE_BYTES)
            t0 = r.stats().trace_launches
            got = r.bake_points(p, n, times[:nspp], radiance=True, ao=False, **kw)
            assert r.stats().trace_launches - t0 == -(-tiles * nspp // per_launch), (name, per_launch, nspp)
            _assert_same(got["rgba"], w[0], name, "bake", "radiance, %d tile-samples per launch, %d seeds" % (per_launch, nspp))
            r.set_tuning(samp_budget=per_launch * 64 * 8)         # the occlusion's launches hold 8 bytes per ray
            got = r.bake_points(p, n, times[:nspp], radiance=False, ao=True, **kw)
            _assert_same(got["ao"], w[1], name, "bake", "occlusion, %d tile-samples per launch, %d seeds" % (per_launch, nspp))
            assert r.query_rejects() == 2 * n_rej
    r.set_tuning(samp_budget=DEFAULT_BUDGET)
    # the rays, and the device form on both sides of the largest origin coordinate
    dp, dn = _dev(p), _dev(n)
    rays = r.bake_rays_device(dp, dn, times, bias=kw["bias"], first_index=ff.FIRST)
    r.sync()
    _ray_fields(rays, c["rays"], name, "bake", "rmr_bake_rays_device")
    assert r.query_rejects() == n_rej
    reach = np.abs(c["rays"]["o"][0]).max(axis=1)
    ext = float(reach[ok].max())
    for bound in (ext, ff.below(ext)):
        far = ok & (reach > F(bound))
        w_rgba, w_ao = want_rgba.copy(), want_ao.copy()
        w_rgba[far], w_ao[far] = 0, 0
        d = r.bake_points_device(dp, dn, times, bound, radiance=True, ao=True, **kw)
        r.sync()
        _assert_same(d["rgba"].cpu().numpy(), w_rgba, name, "bake", "device form, radiance, extent %.9g" % bound)
        _assert_same(d["ao"].cpu().numpy(), w_ao, name, "bake", "device form, occlusion, extent %.9g" % bound)
        assert r.query_rejects() == n_rej + far.sum() and far.sum() == (0 if bound == ext else 1), (name, bound, far.sum())
    blocked = c["blocked"][:, ok]
    _note(name, points=len(p), bake_rejected=n_rej, blocked="%d/%d" % (blocked.sum(), blocked.size))


# ---- b. the probe bake --------------------------------------------------------------------------------------
def _probes(r, name):
    c = ff.probe_case(name)
    p, cl, ext = c["p"], c["clearance"], c["extent"]
    times = ff.seeds(ff.PROBE_SEEDS)
    r.set_jit(0)
    want = ff.probe_want(c)
    got = r.bake_probes(p, times, first_index=ff.FIRST, clearance=cl)
    _assert_same(got, want, name, "probes", "list form")
    assert r.query_rejects() == 1                               # the NaN probe: the host form takes the extent from the list
    got = r.bake_probes(p, times, first_index=ff.FIRST, clearance=ff.above(cl))
    _assert_same(got, ff.probe_want(c, high_clearance=True), name, "probes", "list form, clearance one ulp up")
    assert r.query_rejects() == 1
    dp = _dev(p)
    for bound, low in ((ext, False), (ff.below(ext), True)):
        got = r.bake_probes_device(dp, times, bound, first_index=ff.FIRST, clearance=cl)
        r.sync()
        _assert_same(got.cpu().numpy(), ff.probe_want(c, low_extent=low), name, "probes", "device form, extent %.9g" % bound)
        assert r.query_rejects() == (2 if low else 1), (name, bound)
    rays = r.probe_rays_device(dp, times[:3], first_index=ff.FIRST, clearance=cl)
    r.sync()
    _ray_fields(rays, c["rays"][:3], name, "probes", "rmr_probe_rays_device")
    assert r.query_rejects() == 1
    for m in ff.LENGTHS:
        for nspp in (1, 8):
            got = r.bake_probes(p[:m], times[:nspp], first_index=ff.FIRST, clearance=cl)
            _assert_same(got, ff.probe_want(c, nspp, m), name, "probes", "%d probes, %d seeds" % (m, nspp))
    tiles = -(-len(p) // 64)
    for per_launch in (1, 5):
        for nspp in (1, 8) + ff.CUT_SEEDS:
            r.set_tuning(samp_budget=per_launch * TILE_BYTES)
            t0 = r.stats().trace_launches
            got = r.bake_probes(p, times[:nspp], first_index=ff.FIRST, clearance=cl)
            assert r.stats().trace_launches - t0 == -(-tiles * nspp // per_launch), (name, per_launch, nspp)
            _assert_same(got, ff.probe_want(c, nspp), name, "probes", "%d tile-samples per launch, %d seeds" % (per_launch, nspp))
    r.set_tuning(samp_budget=DEFAULT_BUDGET)
    r.query_rejects()
    # the field form: the statement's bake of the lattice, and the list form on its points
    desc, sh, _, _ = ff.baked_field(name)
    r.bake_probe_field(desc, times=ff.seeds(ff.FIELD_SEEDS), clearance=ff.field_clearance(name))
    d, got = r.read_probe_field()
    assert bytes(d) == bytes(desc)
    _assert_same(got, sh, name, "probes", "field form")
    lst = r.bake_probes(probe_ref.lattice_points(desc), ff.seeds(ff.FIELD_SEEDS), clearance=ff.field_clearance(name))
    _assert_same(got, lst, name, "probes", "field form against the list form")
    assert r.query_rejects() == 0
    _note(name, used=int((~(c["rejected"] | c["buried"])).sum()), buried=int(c["buried"].sum()), rejected=int(c["rejected"].sum()),
          field_invalid=int((sh[:, 27] == 0).sum()))


# ---- c. the visibility --------------------------------------------------------------------------------------
def _visibility(r, name):
    c = ff.vis_case(name)
    p, cl, ext, rng = c["p"], c["clearance"], c["extent"], c["range"]
    times = ff.seeds(ff.VIS_SEEDS)
    got = r.bake_probe_visibility(p, times, rng, first_index=ff.FIRST, clearance=cl)
    _assert_same(got, ff.vis_want(c), name, "visibility", "list form")
    assert r.query_rejects() == 1
    got = r.bake_probe_visibility(p, times, rng, first_index=ff.FIRST, clearance=ff.above(cl))
    _assert_same(got, ff.vis_want(c, high_clearance=True), name, "visibility", "list form, clearance one ulp up")
    assert r.query_rejects() == 1
    dp = _dev(p)
    for bound, low in ((ext, False), (ff.below(ext), True)):
        got = r.bake_probe_visibility_device(dp, times, bound, rng, first_index=ff.FIRST, clearance=cl)
        r.sync()
        _assert_same(got.cpu().numpy(), ff.vis_want(c, low_extent=low), name, "visibility", "device form, extent %.9g" % bound)
        assert r.query_rejects() == (2 if low else 1), (name, bound)
    # lengths, records per probe and cuts: the whole grid on two cases, one line of it on the others
    grid = [(b, m, k) for b in ff.BUDGETS for m in ff.LENGTHS for k in ff.SEED_COUNTS] if name in ff.GRID_CASES else \
           [(b, ff.N_LIST, k) for b in ff.BUDGETS[1:] for k in (8, 9)]
    grid += [(5, m, k) for m in (129, ff.N_LIST) for k in ff.CUT_SEEDS]     # a whole tile between two partial ones
    wants, budget = {}, None
    for b, m, k in grid:
        if b != budget:
            r.set_tuning(samp_budget=b * UNIT_TILE_BYTES if b else DEFAULT_BUDGET)
            budget = b
        if (m, k) not in wants:
            wants[(m, k)] = ff.vis_want(c, k, m)
        got = r.bake_probe_visibility(p[:m], times[:k], rng, first_index=ff.FIRST, clearance=cl)
        _assert_same(got, wants[(m, k)], name, "visibility", "%d probes, %d records each, %s tile-samples per launch" % (m, k, b or "all"))
    r.set_tuning(samp_budget=DEFAULT_BUDGET)
    r.query_rejects()
    # the field form: the field's validity decides which probes have a map
    desc, sh, vis, _ = ff.baked_field(name)
    if name == ff.INF_CASE:
        r.write_probe_field(desc, sh)        # the statement's field: this case runs the cast and the fold alone
    else:
        r.bake_probe_field(desc, times=ff.seeds(ff.FIELD_SEEDS), clearance=ff.field_clearance(name))
    r.bake_probe_field_visibility(ff.seeds(ff.PROBE_SEEDS), rng)
    got, got_rng = r.read_probe_field_visibility()
    assert got_rng == rng
    _assert_same(got, vis, name, "visibility", "field form")
    lst = r.bake_probe_visibility(probe_ref.lattice_points(desc), ff.seeds(ff.PROBE_SEEDS), rng, clearance=ff.field_clearance(name))
    _assert_same(got, lst, name, "visibility", "field form against the list form")
    assert r.query_rejects() == 0
    t = c["samples"][:, ~c["unused"], 3]
    _note(name, below_range=int((t < rng).sum()), at_or_above_range=int((t >= rng).sum()), skipped_records=int((~np.isfinite(t)).sum()))
    if name == ff.INF_CASE:
        assert np.isinf(t).sum() >= 1000, name               # records the cast writes as NaN and the fold skips
    if ff.base(name) == "nan_objects":
        full = ff.vis_want(c)
        assert (full[ff.NEG_INF] == 0).all() and (full[ff.ON_NAN_PLANE, :, 0] > 0).all()


# ---- d. the lookups -----------------------------------------------------------------------------------------
def _lookups(r, name):
    desc, sh, vis, rng = ff.baked_field(name)
    q, nr, groups = ff.lookup_queries(name)
    n_rej = groups["rejected"][1] - groups["rejected"][0]
    dq, dn = _dev(q), _dev(nr)
    quarter = float(F(0.25) * F(desc.spacing))

    def run(label, sh, vis):
        want, ok = probe_ref.lookup(desc, sh, q, nr)
        got = r.probe_irradiance(q, nr)
        _assert_same(got, want, name, "lookups", "%s field" % label)
        assert r.query_rejects() == n_rej == (~ok).sum()
        dev = r.probe_irradiance_device(dq, dn)
        r.sync()
        _assert_same(dev.cpu().numpy(), want, name, "lookups", "%s field, device tensors" % label)
        for bias in (0.0, quarter):
            wv, _ = pv.lookup(desc, sh, vis, q, nr, bias)
            got = r.probe_irradiance(q, nr, visibility=True, bias=bias)
            _assert_same(got, wv, name, "lookups", "%s field, weighted, bias %.4g" % (label, bias))
            dev = r.probe_irradiance_device(dq, dn, visibility=True, bias=bias)
            r.sync()
            _assert_same(dev.cpu().numpy(), wv, name, "lookups", "%s field, weighted, bias %.4g, device tensors" % (label, bias))
        for m in (1, 63, 64, 65):
            _assert_same(r.probe_irradiance(q[:m], nr[:m], visibility=True, bias=quarter), wv[:m], name, "lookups",
                         "%s field, weighted, %d queries" % (label, m))
        r.query_rejects()
        return int((ok & (want[:, 3] == 0)).sum())

    try:
        # the field baked here, which (b) and (c) hold to the statement's
        r.bake_probe_field(desc, times=ff.seeds(ff.FIELD_SEEDS), clearance=ff.field_clearance(name))
        r.bake_probe_field_visibility(ff.seeds(ff.PROBE_SEEDS), rng)
        _assert_same(r.read_probe_field()[1], sh, name, "lookups", "the baked field")
        _assert_same(r.read_probe_field_visibility()[0], vis, name, "lookups", "the baked maps")
        none_b = run("baked", sh, vis)
        syn = ff.synthetic_field()
        syn_vis, syn_rng = ff.synthetic_maps(desc, syn)
        r.write_probe_field(desc, syn)
        r.write_probe_field_visibility(syn_vis, syn_rng)
        none_s = run("synthetic", syn, syn_vis)
    finally:
        r.probe_field_free()
    _note(name, queries=len(q), no_valid_corner="%d baked, %d synthetic" % (none_b, none_s))


# ---- e. the AOVs --------------------------------------------------------------------------------------------
def _raw(r):
    return np.stack([r.read_aov_raw(k) for k in range(5)])     # (5, H, W, 4)


def _aov(r, name):
    tb, prm = ff.tables(name), ff.params(name)
    times = ff.seeds(4)
    x0, y0, x1, y1 = sf.RECT0
    n_px = (x1 - x0) * (y1 - y0)
    models = [("view", {})] + ([("thinlens", ff.lens(name))] if name == ff.LENS_CASE else [])
    for model, fields in models:
        r.set_camera_model(model, **fields)
        rays = r.camera_rays(times, sf.RECT0)
        hits = aov_ref.oracle_hits(tb, prm, rays).reshape(len(times), n_px)
        want = np.array(aov_ref.init(sf.W0 * sf.H0)).reshape(5, sf.H0, sf.W0, 4)
        want[:, y0:y1, x0:x1] = aov_ref.fold(aov_ref.init(n_px), hits).reshape(5, y1 - y0, x1 - x0, 4)
        r.aov_reset()
        r.render_aov(times, rect=sf.RECT0)
        got = _raw(r)
        for k in range(5):
            _assert_same(got[k].reshape(-1, 4), want[k].reshape(-1, 4), name, "aov", "%s, plane %d" % (model, k))
        assert (got[0, y0:y1, x0:x1, 0] == len(times)).all()
        # launches of one sample; one call per sample
        r.set_aov_launch_samples(1)
        r.render_aov(times, rect=sf.RECT0, restart=True)
        _assert_same(_raw(r).reshape(-1, 4), want.reshape(-1, 4), name, "aov", "%s, launches of one sample" % model)
        r.set_aov_launch_samples(6)
        r.aov_reset()
        for k in range(len(times)):
            r.render_aov(times[k:k + 1], rect=sf.RECT0)
        _assert_same(_raw(r).reshape(-1, 4), want.reshape(-1, 4), name, "aov", "%s, one call per sample" % model)
        is_hit = hits["id"] >= 0
        _note(name, **{"aov_%s" % model: "%d hits, %d misses, %d distances not finite" % (is_hit.sum(), (~is_hit).sum(),
                                                                                       (~np.isfinite(hits["t"])).sum())})
        assert is_hit.sum() >= 200 and (~is_hit).sum() >= 50, (name, model)


# ---- f. the guides ------------------------------------------------------------------------------------------
def _guides(r, name):
    r.render_guides()
    g = r.read_guides()
    rays = _view_rays(ff.view(name), g["ray"][..., :3])
    hits = r.cast_rays(rays).reshape(sf.H0, sf.W0)
    vis = r.cast_rays(rays, normals=False).reshape(sf.H0, sf.W0)
    n_hit, n_miss = int((g["normal"][..., 3] >= 0).sum()), int((g["normal"][..., 3] < 0).sum())
    assert n_hit > 100 and n_miss > 50, (name, n_hit, n_miss)
    for what, a, b in (("pos", hits["pos"], g["hit"][..., :3]), ("t", hits["t"], g["hit"][..., 3]), ("n", hits["n"], g["normal"][..., :3]),
                       ("id", hits["id"], g["normal"][..., 3]), ("id, no normals", vis["id"], g["normal"][..., 3]),
                       ("t, no normals", vis["t"], g["hit"][..., 3])):
        _assert_same(np.ascontiguousarray(a).reshape(sf.H0 * sf.W0, -1), np.ascontiguousarray(b).reshape(sf.H0 * sf.W0, -1), name, "guides",
                     "cast_rays %s against the guide plane" % what)
    _note(name, guide_hits=n_hit, guide_misses=n_miss)


# ---- g. the volume and the mesh -----------------------------------------------------------------------------
def _volume(r, name):
    origin, spacing, shape = ff.volume(name)
    tb, md = ff.tables(name), ff.params(name).max_dist
    want_d, want_i = mesh_ref.oracle_volume(tb, origin, spacing, shape, md)
    dist, ids = r.sample_volume(origin, spacing, shape, ids=True)
    _assert_same(dist.reshape(-1), want_d.reshape(-1), name, "volume", "distances")
    _assert_same(ids.reshape(-1), want_i.reshape(-1), name, "volume", "ids")
    try:
        m = r.extract_mesh(origin, spacing, shape)
        want = mesh_ref.surface_nets(want_d, origin, spacing, 0.0)
        worst = mesh_ref.compare(m["vertices"], m["quads"], want, spacing, "%s volume" % name)
        v = np.ascontiguousarray(m["vertices"])
        _assert_same(m["normals"], oracle_normals(tb, md, v, np.ones(len(v), bool)), name, "volume", "vertex normals")
        _assert_same(m["ids"], _map(tb, md, v)[:, 1], name, "volume", "vertex ids")
    finally:
        r.mesh_free()
    _note(name, inside=int((want_d < 0).sum()), vertices=len(v), quads=len(m["quads"]), worst_position="%.2f of its bound" % worst)


RUN = {"bake": _bake, "probes": _probes, "visibility": _visibility, "lookups": _lookups, "aov": _aov, "guides": _guides,
       "volume": _volume}


@pytest.mark.parametrize("name,step", PAIRS, ids=["%s-%s" % p for p in PAIRS])
def test_feature_family(renderer, name, step):
    r = renderer
    try:
        _load(r, name)
        RUN[step](r, name)
    finally:
        _restore(r)
        if (name, step) == [p for p in PAIRS if p[0] == name][-1]:
            print("%-13s %s" % (name, ", ".join("%s %s" % (k, v) for k, v in _counts.get(name, {}).items())))
