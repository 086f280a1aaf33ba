"""A small deterministic family of generated sphere/box scenes away from the point of parameter space at
which every other scene of the suite sits (extent 4 to 10 about the origin, radii up to 1): one base
layout in unit coordinates, a uniform scale s and a translation T. The kernels' error constants
(err_extent, am_r2, npc_eps0, cert_k, bvh_margin, esc_extent, am_dmax) are functions of the
scene, so each case puts them at other values; tests/test_scene_family_cpu.py shows on the oracle alone
that every case is a scene worth rendering, tests/test_gpu_scene_family.py compares the kernels with the
oracle on them bit for bit.

Every centre is float32(s * x + T) and every half-extent float32(s * r), rounded once and written into the
scene as that float's value. The unit coordinates have at most three decimals, so the values are short
decimals and pass the v1 scene format's six-decimal literals unchanged (scene_compile.quant_v1). The
camera is the default camera's eye and direction under the same transform; max_dist is 1000 max(1, s).

Not a test and not a conftest: a helper module like denoise_ref.py."""
import copy
import json
import os

import numpy as np

from oracle import camera, scene_compile
from raymarchrenderer_amd import abi, time_schedule

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

W0, H0, RECT0 = 72, 40, (3, 5, 67, 38)   # the clip rect cuts 8x8 tiles on every side
EYE, LOOK = (0.0, 4.0, -6.0), (0.0, -3.0, 6.0)   # the default camera (oracle/camera.py default_view)
PI32 = np.float32(3.141592653)


def times():
    return time_schedule(2, frame=1)


# ---- the pieces of a scene dictionary -----------------------------------------------------------------
def _diffuse(i, c):
    return {"id": i, "total_vars": 2, "nodes": [{"name": "shader_diffuse", "inputs": [c], "outputs": [0, 1]}],
            "color": 0, "dir": 1}


def _emission(i, c=(1.0, 1.0, 1.0), p=(16, 16, 16)):
    return {"id": i, "total_vars": 1, "nodes": [{"name": "shader_emission", "inputs": [list(c), list(p)], "outputs": [0]}],
            "color": 0, "dir": -1}


def _box(mat, c, r):
    return {"matID": mat, "total_vars": 1, "distance": 0, "nodes": [{"name": "map_box", "inputs": [-1, c, r], "outputs": [0]}]}


def _sphere(mat, c, rad):
    return {"matID": mat, "total_vars": 1, "distance": 0,
            "nodes": [{"name": "map_sphere", "inputs": [-1, c, [rad, rad, rad]], "outputs": [0]}]}


def _primary_dirs(view, W, H, rect):
    """The rect's pixel rays without the jitter (RayMarch.glsl main: mix of the four corner rays)."""
    v = np.asarray(view, np.float64)
    r00, r01, r10, r11 = v[3:6], v[6:9], v[9:12], v[12:15]
    x0, y0, x1, y1 = rect
    out = []
    for py in range(y0, y1):
        for px in range(x0, x1):
            u, w = px / W, py / H
            top, bot = r00 + (r01 - r00) * u, r10 + (r11 - r10) * u
            d = top + (bot - top) * w
            out.append(d / np.linalg.norm(d))
    return np.asarray(out, np.float32)


# ---- base layouts, in unit coordinates: lists of (kind, material, centre, half-extent or radius) --------
# materials 0-5 diffuse, 6 the emission. The floor's top face is y = -1; the default camera looks down at
# it from (0, 4, -6), every primary ray pointing below the horizon, so the "ceiling" light hangs low
# enough (y = 1.5) to be seen. The rooms are open above, in front and to the right.
FLOOR = ("b", 0, (0.0, -1.05, 1.0), (6.0, 0.05, 9.0))
LEFT = ("b", 1, (-3.0, 1.0, 1.0), (0.05, 3.0, 7.0))
BACK = ("b", 2, (0.0, 1.0, 6.0), (6.0, 3.0, 0.05))
BALL = ("s", 3, (0.75, -0.5, 0.5), 0.5)          # tangent to the floor's top face
LIGHT = ("b", 6, (0.0, 1.5, 4.0), (1.5, 0.05, 1.0))


def _room4():
    return [FLOOR, LEFT, BALL, LIGHT]


def _room5():
    return [FLOOR, LEFT, BACK, BALL, LIGHT]


def _room5g(G):
    return [("s", 0, (0.0, -1.0 - G, 0.0), G), LEFT, BACK, BALL, LIGHT]


def _ties8():
    return [FLOOR,
            # the floor's own centre and height, a smaller footprint: over it the two smallest distances
            # are equal and scene order decides the id (opU keeps the later one)
            ("b", 4, FLOOR[2], (2.0, 0.05, 1.5)),
            LEFT, BACK, BALL,
            ("s", 5, BALL[2], BALL[3]),                       # the sphere again, another material
            ("b", 1, (-1.25, -0.6, -0.5), (0.4, 0.4, 0.4)),   # resting on the floor: coplanar contact
            LIGHT]


def _clutter(n, seed, spheres_only=False):
    """n seeded small primitives (radius or half-extent 0.05 to 0.3) inside the room, three decimals."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        c = tuple(round(float(v), 3) for v in rng.uniform((-2.5, -0.6, -3.0), (3.5, 2.0, 4.5)))
        mat = int(rng.integers(0, 6))
        if spheres_only or i % 2 == 0:
            out.append(("s", mat, c, round(float(rng.uniform(0.05, 0.3)), 3)))
        else:
            out.append(("b", mat, c, tuple(round(float(v), 3) for v in rng.uniform(0.05, 0.3, 3))))
    return out


BASES = {
    "room4": _room4, "room5": _room5, "ties8": _ties8,
    "loop20": lambda: _room5() + _clutter(15, 20),
    "bvh40": lambda: _room5() + _clutter(35, 40),
    "bvh40s": lambda: _room5() + _clutter(35, 41, spheres_only=True),
}

GLASS = "glass_offset"
# name: (base, s, T, G)
CASES = {
    "unit": ("room5", 1.0, (0.0, 0.0, 0.0), None),
    "unit4": ("room4", 1.0, (0.0, 0.0, 0.0), None),
    "small": ("room5", 0.02, (0.0, 0.0, 0.0), None),
    "large": ("room5", 200.0, (0.0, 0.0, 0.0), None),
    "offset_1000": ("room5", 1.0, (1000.0, -500.0, 750.0), None),
    "offset_4096": ("room5", 1.0, (4096.0, 0.0, 4096.0), None),
    "offset_16384": ("room5", 1.0, (16384.0, 0.0, 0.0), None),
    "small_offset": ("room5", 0.05, (100.0, 100.0, 100.0), None),
    "ground_1000": ("room5g", 1.0, (0.0, 0.0, 0.0), 1000.0),
    "ground_1e4": ("room5g", 1.0, (0.0, 0.0, 0.0), 10000.0),
    "ties": ("ties8", 1.0, (0.0, 0.0, 0.0), None),
    "ties_offset": ("ties8", 1.0, (300.0, -200.0, 100.0), None),
    "loop20_offset": ("loop20", 1.0, (0.0, 1000.0, 0.0), None),
    "bvh40_offset": ("bvh40", 1.0, (200.0, 0.0, 0.0), None),
    "bvh40s_scale": ("bvh40s", 30.0, (0.0, 0.0, 0.0), None),
    # node-program materials away from the origin: tests/golden/scenes/glass_test.scene translated
    GLASS: ("glass", 1.0, (500.0, 0.0, -500.0), None),
}
ROOM_CASES = [n for n, c in CASES.items() if c[0].startswith("room")]
RULE_CASES = [n for n, c in CASES.items() if c[0] in ("room4", "room5", "room5g", "ties8")]   # sphere/box, <= 8


def _f32(x):
    return float(np.float32(x))


def _layout(name):
    base, s, T, G = CASES[name]
    return _room5g(G) if base == "room5g" else BASES[base]()


def prims(name):
    """The case's primitives after the transform: (kind, material, centre, half-extent), float32 values."""
    base, s, T, G = CASES[name]
    out = []
    if base == "glass":
        for o in scene(name)["objects"]:
            n = o["nodes"][0]
            out.append(("s" if n["name"] == "map_sphere" else "b", o["matID"], tuple(n["inputs"][1]), tuple(n["inputs"][2])))
        return out
    for kind, mat, c, r in _layout(name):
        rr = (r, r, r) if kind == "s" else r
        out.append((kind, mat, tuple(_f32(s * c[k] + T[k]) for k in range(3)), tuple(_f32(s * rr[k]) for k in range(3))))
    return out


_scenes = {}


def scene(name):
    """The case's scene dictionary (the reference's v1 format); a fresh copy."""
    if name not in _scenes:
        base, s, T, G = CASES[name]
        if base == "glass":
            with open(os.path.join(GOLDEN, "scenes", "glass_test.scene")) as f:
                sc = json.load(f)
            for o in sc["objects"]:
                c = o["nodes"][0]["inputs"][1]
                o["nodes"][0]["inputs"][1] = [_f32(c[k] + T[k]) for k in range(3)]
            # the file has three materials; a diffuse sphere beside the pane is the fourth id that the
            # family's condition asks of every case
            sc["materials"].append(_diffuse(3, [0.2, 0.3, 0.8]))
            sc["objects"].append(_sphere(3, [_f32(1.75 + T[0]), _f32(-0.475 + T[1]), _f32(-0.5 + T[2])], 0.5))
        else:
            mats = [_diffuse(0, [0.8, 0.8, 0.8]), _diffuse(1, [0.8, 0.1, 0.1]), _diffuse(2, [0.1, 0.8, 0.1]),
                    _diffuse(3, [0.2, 0.3, 0.8]), _diffuse(4, [0.8, 0.7, 0.2]), _diffuse(5, [0.6, 0.2, 0.7]), _emission(6)]
            objs = [_sphere(m, list(c), r[0]) if kind == "s" else _box(m, list(c), list(r)) for kind, m, c, r in prims(name)]
            sc = {"materials": mats, "objects": objs}
        _scenes[name] = sc
    return copy.deepcopy(_scenes[name])


def tables(name):
    return scene_compile.compile_scene(scene(name), "rm1")


def eye(name):
    """The default camera's eye under the case's transform (float64; the view rounds it to float32)."""
    base, s, T, G = CASES[name]
    return tuple(s * EYE[k] + T[k] for k in range(3))


def view(name, W=W0, H=H0):
    m = float(np.linalg.norm(LOOK))
    return camera.view_uniforms(eye(name), tuple(x / m for x in LOOK), float(W) / float(H), PI32 / np.float32(4))


def max_dist(name):
    return 1000.0 * max(1.0, CASES[name][1])


def params(name, **kw):
    kw.setdefault("max_bounces", 4)
    return abi.default_params(max_dist=max_dist(name), **kw)


_primary = {}


def primary_hits(name):
    """The oracle's march of the pixel-centre primary rays of RECT0, once per case and read-only:
    (eye, dirs, t, id, pos) with id -1 on the misses and pos = float32(eye + t d) in float32 steps."""
    if name not in _primary:
        from .denoise_ref import far_hit_rule, oracle_march
        v = view(name)
        e = np.asarray(v[:3], np.float32)
        dirs = _primary_dirs(v, W0, H0, RECT0)
        t, ident = oracle_march(tables(name), params(name), e, dirs)
        ident = far_hit_rule(t, ident, max_dist(name))
        pos = (e + t[:, None] * dirs).astype(np.float32)
        for a in (dirs, t, ident, pos):
            a.setflags(write=False)
        _primary[name] = (e, dirs, t, ident, pos)
    return _primary[name]


def exact_tie_share(name):
    """Share of the primary hits whose two smallest single-primitive distances are exactly equal
    (test_gpu_batch_probes.near_tie_share with a margin of 0)."""
    from oracle import oracle
    sc = scene(name)
    singles = [scene_compile.compile_scene({"materials": sc["materials"], "objects": [o]}, "rm1") for o in sc["objects"]]
    e, dirs, t, ident, pos = primary_hits(name)
    hit = np.flatnonzero(ident >= 0)
    ties = 0
    for k in hit:
        ds = sorted(float(oracle.map_p(s, pos[k], max_dist(name))[0]) for s in singles)
        ties += ds[1] == ds[0]
    return ties / max(1, len(hit)), len(hit)


def write_rule_scene(name, path):
    """The case as csrc/trail_rule_test.cpp --scene reads it: max_dist, then one line per primitive,
    `b|s id cx cy cz rx ry rz`, every number a C hex float. Data, written at test time."""
    with open(path, "w") as f:
        f.write("%s\n" % float(np.float32(max_dist(name))).hex())
        for kind, mat, c, r in prims(name):
            f.write("%s %s\n" % (kind, " ".join(float(v).hex() for v in (float(mat),) + tuple(c) + tuple(r))))
