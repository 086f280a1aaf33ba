"""Inputs for the kernels built on the trace and query kernels (the light bake §4.17, the irradiance probes
§4.18, their visibility §4.19, the sampled AOVs §4.15, volumes and meshes §4.16) on the generated families:
for a case of scene_family.CASES everything is put through the case's own transform p -> float32(s p + T),
each coordinate rounded once; for a case of node_family.CASES the transform is the identity. Every other test
of those features sits at one point of parameter space (extent 4 to 10 about the origin, lists of 70, lookups
on a dyadic lattice); here the scene-scaled quantities scale with the case:

  bias 0.003 max(1, s), AO distance 1.5 s, clearance the oracle's own map value at one probe, range 2 s,
  extent the largest |coordinate| of the list (one probe lies exactly on it), a lattice of origin
  float32(s (-2.2, -0.6, -1.8) + T) and spacing float32(1.1 s), a thin lens focused at 6 s.

Everything is seeded and deterministic. The statements' results (tests/bake_ref.py, probe_ref.py,
probe_vis_ref.py) are computed once per case and shared, read-only, between tests/test_feature_family_cpu.py
(the inputs are worth running; the host forms agree with the statements) and tests/test_gpu_feature_family.py
(the kernels agree with the statements, bit for bit).

Not a test and not a conftest: a helper module like scene_family.py."""
import numpy as np

from oracle import camera, oracle
from raymarchrenderer_amd import abi, time_schedule

from . import bake_ref, probe_ref, probe_vis_ref
from . import node_family as nf
from . import scene_family as sf
from .test_gpu_scene_family import _room_box, _special_points, _surface_points

F = np.float32
SCENE_CASES = ("unit", "small", "large", "offset_1000", "offset_16384", "small_offset", "ground_1e4", "ties_offset",
               "glass_offset")
NODE_CASES = ("trig", "nan_objects")
CASES = SCENE_CASES + NODE_CASES
# nan_objects with max_dist = +inf (rmr_set_params takes any max_dist > 0): every miss marches to t = +inf, a
# distance the visibility's cast writes as a NaN record and its fold must skip. The visibility step alone runs it.
INF_CASE = "nan_objects_inf"
_BASE = {INF_CASE: "nan_objects"}
JIT_CASES = ("small", "offset_16384", "ties_offset")          # the bake under the hipRTC kernel as well
GRID_CASES = ("unit", "offset_1000")                          # the visibility's grid of lengths, seeds and budgets
AOV_CASES = ("small", "offset_16384", "ties_offset", "nan_objects")
LENS_CASE = "small"                                           # the thin lens: aperture 0.15 s, focus 6 s
GUIDE_CASES = ("large", "offset_4096")
VOLUME_CASES = ("small_offset", "large")

LENGTHS = (1, 63, 64, 65, 129, 200)
SEED_COUNTS = (1, 8, 9, 16)
BUDGETS = (None, 1, 5)                                        # tile-samples per launch (None: the default budget)
# with 5 tile-samples per launch and 2 or 3 seeds a launch over the 200-entry list holds a whole tile strictly
# between two partial ones (3 seeds: tile-samples 5..9 are the last of tile 1, all of tile 2, the first of tile 3)
CUT_SEEDS = (2, 3)
N_LIST = 200
FIRST = 4090                                                  # gx wraps and gy steps inside the lists
BAKE_SEEDS, PROBE_SEEDS, VIS_SEEDS, FIELD_SEEDS = 3, 9, 16, 8
# slots of the probe list (all within its first 64 entries, or in the tile after them)
BURIED, AT_CLEARANCE, NAN, AT_EXTENT = (3, 63, 64), 17, 40, 5
# nan_objects alone: a probe where map is -inf (on y = -0 beside the slab: buried) and one on the plane x = 0, where
# the edge object is NaN and map is the other objects' (used)
NEG_INF, ON_NAN_PLANE = 7, 9
FIELD_UNIT = ((-2.2, -0.6, -1.8), 1.1, (5, 4, 4))
FIELD_CLEARANCE = 0.45                                        # times s: buries the lattice's lowest layer

# unit coordinates per layout: the box the seeded probes come from, three points inside shapes (the centre of a
# box, the centre of the ball, a point inside the left wall or, where there is none, inside the floor), a point
# a little above the floor whose map value becomes the clearance, and points for the degenerate normals
_LAYOUT = {
    "room": {"lo": (-2.9, -0.95, -3.0), "hi": (3.5, 2.8, 5.9),
             "buried": (sf.LIGHT[2], sf.BALL[2], (-2.96, 1.0, 0.5)), "at": (1.5, -0.9, 0.7),
             "up": (0.5, -1.0, 1.2), "down": (0.2, 1.45, 4.2)},
    "glass": {"lo": (-2.5, -0.9, -2.5), "hi": (3.0, 2.5, 2.5),
              "buried": ((0.0, 0.5, 0.0), (1.75, -0.475, -0.5), (-1.0, -1.025, 0.5)), "at": (-1.5, -0.9, 0.7),
              "up": (0.5, -0.975, 1.2), "down": (0.2, 1.475, 0.0)},
    "node": {"lo": (-2.5, -0.7, -2.5), "hi": (3.0, 2.2, 4.0),
             "buried": ((1.4, -0.21, 1.05), (-1.2, 0.0, 0.5), (0.0, -1.2, 1.0)), "at": (1.5, -0.8, -1.0)},
}


def _ro(a):
    a.setflags(write=False)
    return a


# ---- the case ---------------------------------------------------------------------------------------------
def base(name):
    """The case whose scene this case renders."""
    return _BASE.get(name, name)


def is_node(name):
    return base(name) in nf.CASES


def transform(name):
    """(s, T) of the case; the identity for a node-family case."""
    if is_node(name):
        return 1.0, (0.0, 0.0, 0.0)
    return float(sf.CASES[name][1]), tuple(float(v) for v in sf.CASES[name][2])


def scale(name):
    return transform(name)[0]


def xf(name, unit):
    """float32(s p + T) of unit coordinates (..., 3), each coordinate rounded once."""
    s, T = transform(name)
    return (s * np.asarray(unit, np.float64) + np.asarray(T, np.float64)).astype(F)


def _layout(name):
    if is_node(name):
        return _LAYOUT["node"]
    return _LAYOUT["glass" if sf.CASES[name][0] == "glass" else "room"]


def scene(name):
    return nf.scene(base(name)) if is_node(name) else sf.scene(name)


def tables(name):
    return nf.tables(base(name)) if is_node(name) else sf.tables(name)


def params(name):
    if name == INF_CASE:
        return nf.params(max_dist=np.inf)
    return nf.params() if is_node(name) else sf.params(name)


def view(name):
    """The case's view at W0 x H0: the default camera under the transform."""
    if is_node(name):
        m = float(np.linalg.norm(sf.LOOK))
        return camera.view_uniforms(sf.EYE, tuple(x / m for x in sf.LOOK), float(sf.W0) / float(sf.H0), sf.PI32 / F(4))
    return sf.view(name)


def make_oracle(name):
    return oracle.Oracle(tables(name), params(name), view(name), sf.W0, sf.H0)


def seeds(n):
    return time_schedule(n, frame=1)


def bias(name):
    return float(F(0.003 * max(1.0, scale(name))))


def ao_distance(name):
    return float(F(1.5 * scale(name)))


def vis_range(name):
    return F(2.0 * scale(name))


def lens(name):
    """The thin lens of the case: the home scenes' aperture scaled, focused at 6 s."""
    return {"aperture": float(F(0.15 * scale(name))), "focus": float(F(6.0 * scale(name)))}


def _rng(name, salt):
    return np.random.default_rng(1000 * salt + CASES.index(name) if name in CASES else 1000 * salt + 99)


# ---- a. the bake's points -----------------------------------------------------------------------------------
_bake = {}


def _unit32(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F)


def bake_points(name):
    """(p, n, rejects) of a sphere/box case: float32 points and normals and the indices the reject rule takes.
    96 seeded surface points (one in four exactly on its face or sphere, the others up to 0.002 s off it along
    the normal), the corners and edge midpoints of two boxes with a face's normal, on a ground sphere eight
    points of it inside the room, the degenerate normals (0, 1, 0), (-0, 1, 0), (0, -1, 0), the normal
    (0, 1 + 4 ulp, 0) (n.n - 1 = 0.95e-6: used) and, rejected: (0, 1 + 5 ulp, 0) (n.n - 1 = 1.19e-6), a NaN
    point and a zero normal."""
    if name in _bake:
        return _bake[name]
    assert not is_node(name)
    s, _ = transform(name)
    rng = _rng(name, 1)
    prims = sf.prims(name)
    size = [max(r) for _, _, _, r in prims]
    room = [q for q, z in zip(prims, size) if z <= 100.0 * min(size)]
    P, N = [], []
    pts, nrm = _surface_points(room, rng, 96)
    off = np.where(np.arange(96) % 4 == 0, 0.0, rng.uniform(0.0, 0.002 * s, 96))[:, None]
    P.append((pts.astype(np.float64) + off * nrm).astype(F))
    N.append(_unit32(nrm))
    boxes = [q for q in room if q[0] == "b"][:2]
    for q in boxes:
        c = np.array(q[2], F)
        for sp in _special_points([q]):
            sg = np.sign(sp.astype(np.float64) - c)
            if np.abs(sg).sum() < 2:
                continue                                      # (the face centres: the seeded points cover the faces)
            k = int(np.flatnonzero(sg)[0])
            n = np.zeros(3, F)
            n[k] = sg[k]
            P.append(sp[None])
            N.append(n[None])
    for kind, _, c, r in prims:
        if kind == "s" and r[0] > 100.0 * min(size):          # a ground sphere: its cap under the room
            lo, hi = _room_box(prims)
            xz = rng.uniform((lo[0], lo[2]), (hi[0], hi[2]), (8, 2))
            c64 = np.array(c, np.float64)
            y = c64[1] + np.sqrt(float(r[0]) ** 2 - (xz[:, 0] - c64[0]) ** 2 - (xz[:, 1] - c64[2]) ** 2)
            q = np.stack([xz[:, 0], y, xz[:, 1]], axis=1).astype(F)
            P.append(q)
            N.append(_unit32(q.astype(np.float64) - c64))
    lay = _layout(name)
    up, down = xf(name, lay["up"]), xf(name, lay["down"])
    u4, u5 = F(1.0) + F(4.0) * F(2.0 ** -23), F(1.0) + F(5.0) * F(2.0 ** -23)
    hand = [(up, (0, 1, 0)), (up, (-0.0, 1, 0)), (down, (0, -1, 0)), (up, (0, u4, 0)), (up, (0, u5, 0)),
            ((np.nan, up[1], up[2]), (0, 1, 0)), (down, (0, 0, 0))]
    n0 = sum(len(a) for a in P)
    P.append(np.array([h[0] for h in hand], F))
    N.append(np.array([h[1] for h in hand], F))
    p, n = _ro(np.concatenate(P).astype(F)), _ro(np.concatenate(N).astype(F))
    _bake[name] = (p, n, (n0 + 4, n0 + 5, n0 + 6))
    return _bake[name]


_bake_want = {}


def bake_case(name):
    """Once per case, read-only: the points, the statement's rays, cosines, radiance samples and blocked flags of
    BAKE_SEEDS seeds with the case's bias and AO distance, first_index FIRST."""
    if name not in _bake_want:
        p, n, rejects = bake_points(name)
        rays, c, ok = bake_ref.rays(p, n, seeds(BAKE_SEEDS), bias=bias(name), first_index=FIRST)
        L = bake_ref.trace_samples(make_oracle(name), rays)
        blocked = bake_ref.march_blocked(tables(name), params(name), rays, ao_distance(name))
        _bake_want[name] = {"p": p, "n": n, "rejects": rejects, "rays": _ro(rays), "c": _ro(c), "ok": _ro(ok), "L": _ro(L),
                            "blocked": _ro(blocked)}
    return _bake_want[name]


def bake_want(case, nspp=BAKE_SEEDS, m=None):
    """The statement's (rgba, ao) of the first m points and the first nspp seeds."""
    m = len(case["p"]) if m is None else m
    return bake_ref.resolve(case["L"][:nspp, :m], case["c"][:nspp, :m], case["blocked"][:nspp, :m], case["ok"][:m])


# ---- b, c. the probes ---------------------------------------------------------------------------------------
_probes = {}


def probes(name):
    """N_LIST float32 probes: seeded points inside the room's box under the transform (kept 2 % of the box off
    its faces), and in fixed slots three buried ones, one whose map value is the clearance, one NaN, and one on
    a face of the box whose coordinate is the largest of the list: the device forms' extent."""
    if name not in _probes:
        lay = _layout(name)
        lo, hi = np.array(lay["lo"]), np.array(lay["hi"])
        rng = _rng(name, 2)
        m = 0.02 * (hi - lo)
        p = xf(name, rng.uniform(lo + m, hi - m, (N_LIST, 3)))
        for i, u in zip(BURIED, lay["buried"]):
            p[i] = xf(name, u)
        p[AT_CLEARANCE] = xf(name, lay["at"])
        p[NAN, 1] = np.nan
        if base(name) == "nan_objects":
            p[NEG_INF], p[ON_NAN_PLANE] = (1.0, -0.0, -3.0), (0.0, 1.0, -2.0)
        s, T = transform(name)
        far = max(((abs(s * face[a] + T[a]), a, face[a]) for face in (lo, hi) for a in range(3)))
        u = 0.5 * (lo + hi)
        u[far[1]] = far[2]
        p[AT_EXTENT] = xf(name, u)
        rest = np.delete(p, [AT_EXTENT, NAN], axis=0)
        assert np.abs(rest).max() < np.abs(p[AT_EXTENT]).max(), name      # that probe alone lies on the extent
        _probes[name] = _ro(p)
    return _probes[name]


def extent(points):
    """The largest |coordinate| of the list's finite probes, a float32 value."""
    p = np.asarray(points, F)
    fin = np.isfinite(p).all(axis=1)
    return float(np.abs(p[fin]).max()) if fin.any() else 1.0


def below(x):
    return float(np.nextafter(F(x), F(0.0)))


def above(x):
    return float(np.nextafter(F(x), F(np.inf)))


_probe_want = {}


def probe_case(name):
    """Once per case, read-only: the list, its clearance (the oracle's map value at probe AT_CLEARANCE) and
    extent, the reject and buried flags without an extent, the statement's rays (PROBE_SEEDS seeds, first_index
    FIRST), radiance samples and the fold of all of them."""
    if name not in _probe_want:
        p, tb, prm = probes(name), tables(name), params(name)
        clearance = float(oracle.map_p(tb, p[AT_CLEARANCE], prm.max_dist)[0])
        rejected, buried = probe_ref.probe_state(tb, p, clearance, np.inf, prm.max_dist)
        rl = probe_ref.rays(p, seeds(PROBE_SEEDS), FIRST, rejected | buried)
        L = bake_ref.trace_samples(make_oracle(name), rl)
        sh = probe_ref.fold(L, rl["d"], rl["gx"] >= 0)
        _probe_want[name] = {"p": p, "clearance": clearance, "extent": extent(p), "rejected": _ro(rejected),
                             "buried": _ro(buried), "rays": _ro(rl), "L": _ro(L), "sh": _ro(sh)}
    return _probe_want[name]


def probe_want(case, nspp=PROBE_SEEDS, m=None, low_extent=False, high_clearance=False):
    """The statement's sh of the first m probes and the first nspp seeds; low_extent: with
    extent = nextafter(extent, 0), which rejects probe AT_EXTENT; high_clearance: with
    clearance = nextafter(clearance, inf), which buries probe AT_CLEARANCE."""
    m = len(case["p"]) if m is None else m
    rl = case["rays"][:nspp, :m]
    sh = case["sh"][:m].copy() if nspp == PROBE_SEEDS else probe_ref.fold(case["L"][:nspp, :m], rl["d"], rl["gx"] >= 0)
    if low_extent and m > AT_EXTENT:
        sh[AT_EXTENT] = 0
    if high_clearance and m > AT_CLEARANCE:
        sh[AT_CLEARANCE] = 0
    return sh


_vis_want = {}


def vis_case(name):
    """Once per case, read-only: the probe case's list, flags and clearance, and the statement's samples
    (direction and march distance) of VIS_SEEDS seeds at first_index FIRST."""
    if name not in _vis_want:
        pc = probe_case(name)
        unused = pc["rejected"] | pc["buried"]
        s = probe_vis_ref.samples(tables(name), pc["p"], seeds(VIS_SEEDS), FIRST, unused, params(name))
        _vis_want[name] = dict(pc, samples=_ro(s), unused=_ro(unused), range=vis_range(name))
    return _vis_want[name]


def vis_want(case, nspp=VIS_SEEDS, m=None, low_extent=False, high_clearance=False):
    """The statement's maps (m, 64, 2) of the first m probes and the first nspp seeds."""
    m = len(case["p"]) if m is None else m
    vis = probe_vis_ref.fold(case["samples"][:nspp, :m], case["range"])
    vis[case["unused"][:m]] = 0
    if low_extent and m > AT_EXTENT:
        vis[AT_EXTENT] = 0
    if high_clearance and m > AT_CLEARANCE:
        vis[AT_CLEARANCE] = 0
    return vis


# ---- d. the lattice and its queries -------------------------------------------------------------------------
def lattice(name):
    """The case's probe lattice: origin float32(s (-2.2, -0.6, -1.8) + T), spacing float32(1.1 s), 5 x 4 x 4."""
    o, sp, shape = FIELD_UNIT
    return abi.volume_desc(tuple(float(v) for v in xf(name, o)), float(F(sp * scale(name))), shape)


def field_clearance(name):
    return float(F(FIELD_CLEARANCE * scale(name)))


def synthetic_field():
    """probe_ref.lookup_cases' 5 x 4 x 4 field: invalid along (ix, 0, 0) and around point (3, 2, 2)."""
    return probe_ref.lookup_cases(0)[1]


def synthetic_maps(desc, sh):
    """probe_vis_ref.lookup_maps on the lattice (its range scales with the spacing), NaN at the invalid probes."""
    vis, rng = probe_vis_ref.lookup_maps(desc)
    vis[sh[:, 27] == 0] = np.nan
    return vis, rng


_fields = {}


def baked_field(name):
    """Once per case, read-only: the statement's bake of the lattice (FIELD_SEEDS seeds, clearance 0.45 s) and of
    its maps (PROBE_SEEDS seeds, range 2 s): (desc, sh, vis, range). The field's validity decides which probes
    have a map."""
    if name not in _fields:
        desc, tb, prm = lattice(name), tables(name), params(name)
        pts = probe_ref.lattice_points(desc)
        sh, _, _ = probe_ref.bake(make_oracle(name), tb, pts, seeds(FIELD_SEEDS), 0, field_clearance(name), np.inf, prm.max_dist)
        unused = sh[:, 27] == 0
        vis = probe_vis_ref.fold(probe_vis_ref.samples(tb, pts, seeds(PROBE_SEEDS), 0, unused, prm), vis_range(name))
        vis[unused] = 0
        _fields[name] = (desc, _ro(sh), _ro(vis), vis_range(name))
    return _fields[name]


GROUPS = ("on_lattice", "neighbour_below", "neighbour_above", "faces", "outside", "some_invalid", "all_invalid",
          "rejected", "random", "axis_normals")
_queries = {}


def lookup_queries(name):
    """(q, normals, groups) on the case's lattice, groups naming index ranges: the lattice's own float32 points
    and their nextafter neighbours on both sides on every axis, points on the six outer faces, points outside by
    up to a cell, points in the cells the synthetic field's holes touch (some corners invalid: cells (2, 2, 2)
    and (0, 0, 0); all: cell (3, 2, 2)), ten rejected queries, seeded interior points, and the six axis normals
    at one point. The other normals are seeded unit vectors."""
    if name in _queries:
        return _queries[name]
    desc = lattice(name)
    rng = _rng(name, 3)
    pts = probe_ref.lattice_points(desc)
    o = np.array([float(desc.origin[a]) for a in range(3)])
    sp = float(desc.spacing)
    nn = np.array([int(desc.n[a]) for a in range(3)])
    lo, hi = pts[0].astype(np.float64), pts[-1].astype(np.float64)
    groups, Q, Nn = {}, [], []

    def unit(k):
        return _unit32(rng.normal(size=(k, 3)))

    def add(gname, q, n=None):
        q = np.asarray(q, F).reshape(-1, 3)
        start = sum(len(a) for a in Q)
        groups[gname] = (start, start + len(q))
        Q.append(q)
        Nn.append(unit(len(q)) if n is None else np.asarray(n, F).reshape(-1, 3))

    def at(f):
        """Cell coordinates to float32 points."""
        return (o + np.asarray(f, np.float64) * sp).astype(F)

    add("on_lattice", pts)
    for gname, to in (("neighbour_below", -np.inf), ("neighbour_above", np.inf)):
        parts = []
        for a in range(3):
            q = pts.copy()
            q[:, a] = np.nextafter(q[:, a], F(to))
            parts.append(q)
        add(gname, np.concatenate(parts))
    faces = []
    for a in range(3):
        for side in (lo, hi):
            q = rng.uniform(lo, hi, (8, 3)).astype(F)
            q[:, a] = F(side[a])
            faces.append(q)
    add("faces", np.concatenate(faces))
    out = rng.uniform(lo - sp, hi + sp, (60, 3))
    a = rng.integers(0, 3, 60)
    beyond = np.where(rng.integers(0, 2, 60) == 0, lo[a] - rng.uniform(0.01, 1.0, 60) * sp, hi[a] + rng.uniform(0.01, 1.0, 60) * sp)
    out[np.arange(60), a] = beyond
    add("outside", out)
    add("some_invalid", at(np.concatenate([(2, 2, 2) + rng.uniform(0.1, 0.9, (4, 3)), rng.uniform(0.1, 0.9, (4, 3))])))
    add("all_invalid", at((3, 2, 2) + rng.uniform(0.1, 0.9, (4, 3))))
    inside = at((1.3, 1.4, 1.6))
    rq, rn = np.tile(inside, (10, 1)), np.tile(np.array([[0, 1, 0]], F), (10, 1))
    rq[0, 0], rq[1, 1], rq[2, 2], rq[3, 0] = np.nan, np.inf, -np.inf, np.nan
    rn[4], rn[5], rn[6], rn[7], rn[8], rn[9] = (0, 0, 0), (0, np.nan, 0), (1.000001, 0, 0), (0, 0, 0.999999), (np.inf, 0, 0), (0, 2, 0)
    add("rejected", rq, rn)
    add("random", at(rng.uniform(0.0, 1.0, (150, 3)) * (nn - 1)))
    add("axis_normals", np.tile(inside, (6, 1)), [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])
    assert tuple(groups) == GROUPS
    _queries[name] = (_ro(np.concatenate(Q)), _ro(np.concatenate(Nn)), groups)
    return _queries[name]


def corner_validity(desc, sh, q):
    """(n, 8) bool: which corners of each query's cell are valid probes of the field."""
    n = [int(desc.n[a]) for a in range(3)]
    c = [probe_ref.cell(np.where(np.isfinite(q[:, a]), q[:, a], F(0.0)), desc.origin[a], desc.spacing, n[a])[0] for a in range(3)]
    base = c[0] + n[0] * (c[1] + n[1] * c[2])
    off = np.array([(k & 1) + n[0] * (((k >> 1) & 1) + n[1] * (k >> 2)) for k in range(8)])
    return sh[base[:, None] + off[None, :], 27] > 0


def cells(desc, q):
    """(n, 3) the cell index of each query on every axis."""
    n = [int(desc.n[a]) for a in range(3)]
    return np.stack([probe_ref.cell(q[:, a], desc.origin[a], desc.spacing, n[a])[0] for a in range(3)], axis=1)


# ---- g. the volume's lattice --------------------------------------------------------------------------------
def volume(name):
    """(origin, spacing, shape): 12 x 11 x 13 samples at float32(0.27 s) around the ball (0.75, -0.5, 0.5), through
    the floor's top face y = -1."""
    s = scale(name)
    origin = tuple(float(v) for v in xf(name, (-0.8, -1.6, -1.1)))
    return origin, float(F(0.27 * s)), (12, 11, 13)
