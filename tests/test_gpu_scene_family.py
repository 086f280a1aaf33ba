"""The kernels on the generated scene family (tests/scene_family.py): scenes scaled by 0.02 to 200, moved
up to 16384 from the origin, with ground spheres of radius 10^3 and 10^4, with exact ties, and the glass
scene at an offset. The work-skipping paths (approximate-then-exact map, escape bound, nearest-primitive
cache with its BVH and candidate grid, certified getNormal, trailing steps) keep the contract "every sample
bitwise equal to the oracle" by proofs stated in constants the host derives from the scene (err_extent,
am_r2, npc_eps0, cert_k, bvh_margin, esc_extent, am_dmax); every other scene of the suite puts those
constants at about the same values. Here each case is rendered by the release library with its defaults
(lane slots, batch probes, trailing steps, all culling) through

  a. the hipRTC-specialised kernel,                           against the oracle's samples;
  b. the ahead-of-time table kernel of the class,             against the oracle's samples;
  c. the table kernel with every work-skipping path off,      against (b), with map_evals equal to the oracle's;
  d. counters showing that the fast paths ran at all (and one printed line of rates per case);
  e. rmr_eval_map and rmr_cast_rays                           against the oracle's map / march / getNormal;
  f. rmr_trace_rays (the ray-source kernels and their org_extent escape bound, three cases)
                                                              against the oracle's trace(o, d).

Everything is compared bit for bit (NaN equals NaN); nothing here has a tolerance. tests/test_scene_family_cpu.py
shows on the oracle alone that the cases are scenes worth rendering."""
import numpy as np
import pytest

from oracle import oracle
from raymarchrenderer_amd import abi, check_rays

from . import scene_family as sf
from .test_gpu_batch_probes import _same
from .test_gpu_query import _check_cast, _map, _march

pytestmark = pytest.mark.gpu

TRAIL_STEPS, TRAIL_LANES, NPC_FULL = 31, 33, 3   # rmr.h rmr_get_counters_n
TRAIL_CASES = ("unit", "large", "offset_1000", "ground_1000", "ties")
RAY_CASES = ("offset_1000", "ground_1000", "ties_offset")
N_EVAL = 4000


def _assert_same(got, want, what):
    """Bit for bit over (..., 3 or 4) samples; the case, the number of differing samples, the first one."""
    eq = _same(got, want)
    bad = np.argwhere(~eq.all(axis=-1))
    assert bad.size == 0, "%s: %d/%d samples differ; first %s gpu=%s cpu=%s" % (
        what, len(bad), int(np.prod(eq.shape[:-1])), bad[0], np.asarray(got)[tuple(bad[0])], np.asarray(want)[tuple(bad[0])])


def _load(r, name):
    r.set_image_size(sf.W0, sf.H0)
    r.reload()
    r.load_scene(sf.scene(name), "rm1")
    r.set_params(sf.params(name))
    r.set_view(sf.view(name))
    r.set_env_map(None)
    r.set_tuning(lane_slots=True)
    r.set_trail_steps(-1)
    r.set_culling(abi.CULL_ALL)


def _render(r, jit, culling=abi.CULL_ALL):
    """trace_samples over RECT0 by the specialised (jit 1) or the table kernel (jit 0): samples, stats, counters."""
    r.set_jit(jit)
    r.set_culling(culling)
    r.reset_stats()
    gpu = r.trace_samples(sf.times(), sf.RECT0)
    st = r.stats()
    assert st.trace_launches > 0 and st.jit_launches == (st.trace_launches if jit else 0)
    return gpu, st, r.counters(34)


# ---- point and ray lists ------------------------------------------------------------------------------
def _room_box(prims):
    """The box of the primitives without those 100 times the smallest (the ground spheres): (lo, hi)."""
    size = [max(r) for _, _, _, r in prims]
    keep = [p for p, s in zip(prims, size) if s <= 100.0 * min(size)]
    lo = np.min([np.array(c) - np.array(r) for _, _, c, r in keep], axis=0)
    hi = np.max([np.array(c) + np.array(r) for _, _, c, r in keep], axis=0)
    return lo, hi


def _surface_points(prims, rng, n):
    """n float32 points on the primitives with their outward normals: box faces and sphere surfaces, the
    coordinate on the face c +- r in float32 arithmetic (exactly the face's plane as the map sees it)."""
    pts, nrm = np.zeros((n, 3), np.float32), np.zeros((n, 3))
    for i in range(n):
        kind, _, c, r = prims[int(rng.integers(len(prims)))]
        c, r = np.array(c, np.float32), np.array(r, np.float32)
        if kind == "s":
            u = rng.normal(size=3)
            u /= np.linalg.norm(u)
            pts[i], nrm[i] = (c.astype(np.float64) + float(r[0]) * u).astype(np.float32), u
        else:
            k, sg = int(rng.integers(3)), (1.0, -1.0)[int(rng.integers(2))]
            p = (c.astype(np.float64) + r.astype(np.float64) * rng.uniform(-1.0, 1.0, 3)).astype(np.float32)
            p[k] = c[k] + np.float32(sg) * r[k]
            pts[i], nrm[i, k] = p, sg
    return pts, nrm


def _special_points(prims):
    """Exactly on the boxes' corners, edge midpoints and face centres and on the spheres' six poles."""
    out = []
    for kind, _, c, r in prims:
        c, r = np.array(c, np.float32), np.array(r, np.float32)
        for sx in (-1, 0, 1):
            for sy in (-1, 0, 1):
                for sz in (-1, 0, 1):
                    s = np.array([sx, sy, sz], np.float32)
                    if kind == "s" and np.abs(s).sum() != 1:
                        continue
                    if kind == "b" and np.abs(s).sum() == 0:
                        continue
                    out.append(c + s * r)
    return np.asarray(out, np.float32)


def _eval_points(name, rng):
    """About N_EVAL points: the oracle's primary hit points and their six probes, points exactly on
    faces, edges, corners and poles, the tie regions, the room's box doubled, and 3 to 300 extents away."""
    prims = sf.prims(name)
    e, dirs, t, ident, pos = sf.primary_hits(name)
    hits = pos[ident >= 0][::6][:300]
    probes = [hits]
    for k in range(3):
        for sg in (1.0, -1.0):
            q = hits.copy()
            q[:, k] += np.float32(sg * 0.001)
            probes.append(q)
    lo, hi = _room_box(prims)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    ext = float(np.max(np.abs([lo, hi])))
    special = _special_points(prims)[:900]
    surf, _ = _surface_points(prims, rng, 300)
    parts = probes + [special, surf]
    if name.startswith("ties"):
        # inside and on the inner slab (the floor's centre and height) and the doubled sphere
        (_, _, c1, r1), (_, _, c5, r5) = prims[1], prims[5]
        slab = np.array(c1) + np.array(r1) * rng.uniform(-1.0, 1.0, (200, 3))
        slab[100:, 1] = np.float32(c1[1]) + np.float32(r1[1])            # on the shared top face
        ball = np.array(c5) + r5[0] * rng.uniform(-1.2, 1.2, (100, 3))
        parts += [slab.astype(np.float32), ball.astype(np.float32)]
    parts.append((mid + 2.0 * half * rng.uniform(-1.0, 1.0, (600, 3))).astype(np.float32))
    u = rng.normal(size=(200, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    parts.append((mid + u * (ext * 10.0 ** rng.uniform(0.5, 2.5, 200))[:, None]).astype(np.float32))
    pts = np.concatenate(parts).astype(np.float32)
    assert 3000 <= len(pts) <= 5000, len(pts)
    return pts


def _rays(o, d, rng):
    rays = np.zeros(len(o), np.dtype(abi.RAY_DTYPE))
    d = np.asarray(d, np.float64)
    rays["o"], rays["d"] = np.asarray(o, np.float32), (d / np.linalg.norm(d, axis=1)[:, None]).astype(np.float32)
    rays["gx"], rays["gy"] = rng.integers(0, 2000, len(o)), rng.integers(0, 1200, len(o))
    rays["time"] = rng.uniform(0, 2000, len(o)).astype(np.float32)
    assert check_rays(rays)
    return rays


def _surface_rays(name, rng, n):
    """n rays starting on the surfaces, pointing away along seeded hemisphere directions: one in four
    exactly on the surface (a hit at t = 0), the others 0.003 off it, where a bounce ray starts."""
    pts, nrm = _surface_points(sf.prims(name), rng, n)
    off = np.where(np.arange(n) % 4 == 0, 0.0, 0.003)[:, None]
    pts = (pts.astype(np.float64) + off * nrm).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d *= np.where((d * nrm).sum(axis=1) < 0, -1.0, 1.0)[:, None]
    return _rays(pts, d, rng)


# ---- a to e: one function per case, one compile -------------------------------------------------------
@pytest.mark.parametrize("name", list(sf.CASES))
def test_family_bitexact(renderer, name):
    r = renderer
    tables, prm = sf.tables(name), sf.params(name)
    orc = oracle.Oracle(tables, prm, sf.view(name), sf.W0, sf.H0)
    cpu = orc.trace_samples(sf.times(), sf.RECT0)
    rng = np.random.default_rng(sorted(sf.CASES).index(name))
    try:
        _load(r, name)
        # a. the specialised kernel
        jit, st_jit, cnt = _render(r, 1)
        assert st_jit.jit_launches == st_jit.trace_launches > 0
        _assert_same(jit[..., :3], cpu[..., :3], "%s: specialised kernel vs oracle" % name)
        # b. the table kernel
        tab, st_tab, cnt_tab = _render(r, 0)
        _assert_same(tab[..., :3], cpu[..., :3], "%s: table kernel vs oracle" % name)
        # c. the table kernel with the work-skipping paths off
        off, st_off, _ = _render(r, 0, culling=0)
        _assert_same(off, tab, "%s: table kernel, culling off vs on" % name)
        assert st_tab.map_evals <= st_off.map_evals, (name, st_tab.map_evals, st_off.map_evals)
        assert st_off.map_evals == orc.map_evals, (name, st_off.map_evals, orc.map_evals)
        # d. the fast paths ran
        march = cnt[0] - cnt[14]
        print("%-13s trailing steps %.4f of march evaluations, %.4f of evaluated lanes accepted; map_evals %d (culling on) "
              "%d (off); full-map batches of the cache %d"
              % (name, cnt[TRAIL_STEPS] / max(1, march), cnt[TRAIL_STEPS] / max(1, cnt[TRAIL_LANES]), st_tab.map_evals,
                 st_off.map_evals, cnt[NPC_FULL]))
        if name in TRAIL_CASES:
            assert cnt[TRAIL_STEPS] > 0, name
        if name in sf.ROOM_CASES:   # open above and to the right: rays leave, the escape bound ends their marches
            assert st_tab.map_evals < st_off.map_evals, name
        if name.startswith("bvh40"):
            assert cnt[NPC_FULL] > 0, name
        # e. the map and the first hit
        pts = _eval_points(name, rng)
        got, want = r.eval_map(pts), _map(tables, prm.max_dist, pts)
        eq = _same(got, want).all(axis=1)
        assert eq.all(), "%s eval_map: %d/%d points differ; first %d: p %s gpu %s oracle %s" % (
            name, (~eq).sum(), len(pts), np.argmin(eq), pts[np.argmin(eq)], got[np.argmin(eq)], want[np.argmin(eq)])
        assert (want[:, 0] < 0.001).sum() >= 100 and (want[:, 0] > 0.001).sum() >= 100
        e, dirs, t, ident, pos = sf.primary_hits(name)
        rays = np.concatenate([_rays(np.tile(e, (len(dirs), 1)), dirs, rng), _surface_rays(name, rng, len(dirs))])
        rays["d"][:len(dirs)] = dirs   # the primary rays' own float32 directions
        mt, mid = _march(tables, prm, rays)
        assert np.array_equal(mt[:len(dirs)], t)   # (the list's first half is the CPU test's march)
        is_hit = _check_cast(r.cast_rays(rays), rays, tables, prm, mt, mid, name)
        assert is_hit[len(dirs):].sum() >= 100 and (~is_hit[len(dirs):]).sum() >= 100, name
    finally:
        r.set_culling(abi.CULL_ALL)
        r.set_jit(2)
        r.set_tuning(lane_slots=True)


# ---- f. caller's rays ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RAY_CASES)
def test_family_trace_rays_bitexact(renderer, name):
    r = renderer
    rng = np.random.default_rng(100 + sorted(sf.CASES).index(name))
    e, dirs, t, ident, pos = sf.primary_hits(name)
    pick = rng.choice(len(dirs), 128, replace=False)
    rays = np.concatenate([_surface_rays(name, rng, 384), _rays(np.tile(e, (128, 1)), dirs[pick], rng)])
    rays["d"][384:] = dirs[pick]
    assert len(rays) == 512
    orc = oracle.Oracle(sf.tables(name), sf.params(name), sf.view(name), sf.W0, sf.H0)
    want = np.array([orc.trace(int(q["gx"]), int(q["gy"]), float(q["time"]), q["o"], q["d"]) for q in rays])
    assert len(np.unique(want, axis=0)) > 3, "a degenerate ray list"
    try:
        _load(r, name)
        for jit in (1, 0):
            r.set_jit(jit)
            r.reset_stats()
            got = r.trace_rays(rays)
            st = r.stats()
            assert st.trace_launches > 0 and st.jit_launches == (st.trace_launches if jit else 0)
            assert (got[:, 3] == 1).all()
            _assert_same(got[:, :3], want, "%s: trace_rays, jit %d vs oracle" % (name, jit))
    finally:
        r.set_jit(2)
