"""A small family of generated node-program scenes (the v1 format's object and material programs): the
nodes, operand kinds and distances that no scene file of the suite executes. math_sine / math_cosine /
misc_getX / misc_getZ, products and quotients by real divisors, two variable operands, map_sphere /
map_box with a variable centre or radius, domain_repeat with a negative, a y and a zero period after an
offset, all RMR_MAX_VARS variables, the material nodes math_subtract / math_multiply / math_divide, node
programs among more than 32 primitives, and objects whose distance is NaN or +-inf beside finite ones.

  trig         a cosine height-field floor, a sine-rippled sphere, a box scaled by division by 0.7, a light
               (scenes/trig_nodes.scene is this case written out)
  trig_mat     trig with node-program materials (has_prog)
  varops       trig + a sphere of variable radius, a box of variable centre, a 16-variable lattice program
  nan_objects  trig + an object that is NaN on the plane x = 0 and one that is +-inf / NaN on y = 0
  table40      trig + 36 seeded spheres and boxes: 40 primitives, three of them programs

Every literal has at most six decimals (scene_compile.quant_v1 leaves it unchanged); the camera is the
default view, the image 44x36 with the rect (3, 2, 41, 35), max_bounces 3. tests/node_ref.py is the
float64 statement of the object programs, tests/test_node_family_cpu.py shows on the oracle alone that
every case is worth rendering, tests/test_gpu_node_family.py compares the kernels with the oracle bit for
bit.

Not a test and not a conftest: a helper module like scene_family.py."""
import copy

import numpy as np

from oracle import camera, scene_compile
from raymarchrenderer_amd import abi

from .scene_family import EYE, _clutter, _diffuse, _emission, _primary_dirs, times   # noqa: F401 (times: re-exported)

W, H, RECT = 44, 36, (3, 2, 41, 35)
MAX_BOUNCES = 3
P = -1   # the operand "p"
CASES = ("trig", "trig_mat", "varops", "nan_objects", "table40")
RAY_CASES = ("trig", "varops", "nan_objects", "table40")
LO, HI = (-5.0, -1.5, -5.0), (5.0, 5.0, 5.0)   # the box of the random points
N_RANDOM = 2000


# ---- node-list builders -------------------------------------------------------------------------------
def _n(name, ins, outs):
    return {"name": name, "inputs": [list(a) if isinstance(a, (list, tuple)) else a for a in ins],
            "outputs": [outs] if isinstance(outs, int) else list(outs)}


def _v(x):
    return [x, x, x]


def _obj(mat, nodes, dist):
    used = [o for nd in nodes for o in nd["outputs"]]
    return {"matID": mat, "total_vars": max(used) + 1, "distance": dist, "nodes": nodes}


def _floor():
    return _obj(0, [_n("math_multiply", [P, _v(2.5)], 0), _n("math_cosine", [0], 1), _n("misc_getX", [1], 2),
                    _n("misc_getZ", [1], 3), _n("math_multiply", [2, 3], 4), _n("math_multiply", [4, _v(0.08)], 5),
                    _n("map_box", [P, [0, -1.2, 1], [6, 0.2, 9]], 6), _n("math_subtract", [6, 5], 7)], 7)


def _ripple():
    return _obj(1, [_n("math_multiply", [P, _v(7)], 0), _n("math_sine", [0], 1), _n("misc_getX", [1], 2),
                    _n("misc_getY", [1], 3), _n("misc_getZ", [1], 4), _n("math_multiply", [2, 3], 5),
                    _n("math_multiply", [5, 4], 6), _n("math_multiply", [6, _v(0.06)], 7),
                    _n("map_sphere", [P, [-1.2, 0, 0.5], _v(0.9)], 8), _n("math_add", [8, 7], 9)], 9)


def _scaled():
    return _obj(2, [_n("math_divide", [P, _v(0.7)], 0), _n("map_box", [0, [2, -0.3, 1.5], _v(0.8)], 1),
                    _n("math_multiply", [1, _v(0.7)], 2)], 2)


def _light():
    return _obj(3, [_n("map_box", [P, [0, 2.5, 3], [1.5, 0.05, 1]], 0)], 0)


def _trig_objects():
    return [_floor(), _ripple(), _scaled(), _light()]


def _trig_materials():
    return [_diffuse(0, [0.8, 0.8, 0.8]), _diffuse(1, [0.8, 0.1, 0.1]), _diffuse(2, [0.1, 0.8, 0.1]), _emission(3)]


# ---- trig_mat: materials 1 and 2 as node programs ------------------------------------------------------
def _mat1_prog():
    return {"id": 1, "total_vars": 6, "color": 4, "dir": 5,
            "nodes": [_n("misc_facing", [], 0), _n("math_multiply", [0, [0.5, 0.2, 0.1]], 1),
                      _n("math_subtract", [[0.9, 0.6, 0.3], 1], 2), _n("math_divide", [2, _v(1.25)], 3),
                      _n("shader_diffuse", [3], [4, 5])]}


def _mat2_prog():
    """A mix of a diffuse and a glossy lobe; the factor (inside + facing) / 2 (shader_mix clamps it)."""
    return {"id": 2, "total_vars": 12, "color": 9, "dir": 10, "inside": 11,
            "nodes": [_n("shader_diffuse", [[0.1, 0.8, 0.1]], [0, 1]), _n("shader_glossy", [[0.8, 0.8, 0.8], _v(0.1)], [2, 3]),
                      _n("misc_inside", [], 4), _n("misc_facing", [], 5), _n("math_add", [4, 5], 6),
                      _n("math_divide", [6, _v(2)], 7),
                      _n("shader_mix", [0, 1, [0, 0, 0], 2, 3, [0, 0, 0], 7], [9, 10, 11])]}


# ---- varops: variable radius, variable centre, all 16 variables ---------------------------------------
VAR_SPHERE_C = [0.3, 0.3, -1.5]
VAR_BOX_C0 = [-2.9, -0.4, 2.8]
LATTICE_OFFSET = [0.4, 0.3, -0.2]
LATTICE_PERIOD = [-1.5, 0.9, 0]


def _var_sphere(mat):
    """r = 0.5 + 0.2 sin(3 y)."""
    return _obj(mat, [_n("misc_getY", [P], 0), _n("math_multiply", [0, _v(3)], 1), _n("math_sine", [1], 2),
                      _n("math_multiply", [2, _v(0.2)], 3), _n("math_add", [_v(0.5), 3], 4),
                      _n("map_sphere", [P, VAR_SPHERE_C, 4], 5)], 5)


def _var_box(mat):
    """c = c0 + (0.3, 0, 0) cos(2 z)."""
    return _obj(mat, [_n("misc_getZ", [P], 0), _n("math_multiply", [0, _v(2)], 1), _n("math_cosine", [1], 2),
                      _n("math_multiply", [2, [0.3, 0, 0]], 3), _n("math_add", [VAR_BOX_C0, 3], 4),
                      _n("map_box", [P, 4, [0.6, 0.5, 0.9]], 5)], 5)


def _lattice(mat):
    """Small spheres on a lattice of period (-1.5, 0.9, none) inside a bounding box, a sphere carved out of
    them (op_subtract of two variables), a bar joined on (op_union of two variables), a sine ripple in y,
    divided and multiplied by 1.25: variables 0 to 15."""
    return _obj(mat, [_n("math_add", [P, LATTICE_OFFSET], 0), _n("domain_repeat", [0, LATTICE_PERIOD], 1),
                      _n("map_sphere", [1, [0, 0, 2.2], _v(0.3)], 2), _n("map_box", [P, [2.9, 0.4, 2.4], [1.4, 1.3, 0.5]], 3),
                      _n("op_intersect", [2, 3], 4), _n("map_sphere", [P, [2.6, 0.6, 2.1], _v(0.45)], 5),
                      _n("op_subtract", [4, 5], 6), _n("map_box", [P, [2.9, -0.85, 2.4], [1.4, 0.05, 0.1]], 7),
                      _n("op_union", [6, 7], 8), _n("misc_getY", [P], 9), _n("math_multiply", [9, _v(3)], 10),
                      _n("math_sine", [10], 11), _n("math_multiply", [11, _v(0.02)], 12), _n("math_add", [8, 12], 13),
                      _n("math_divide", [13, _v(1.25)], 14), _n("math_multiply", [14, _v(1.25)], 15)], 15)


# ---- nan_objects --------------------------------------------------------------------------------------
SLAB_C, SLAB_R = [0, -500, 1998.5], [2000, 500, 2000]   # its top face is the plane y = 0 for z >= -1.5


def _edge(mat):
    """sphere + sin(p / p.x).x: sphere + sin(1) off the plane x = 0 (never a surface), NaN on it."""
    return _obj(mat, [_n("misc_getX", [P], 0), _n("math_divide", [P, 0], 1), _n("math_sine", [1], 2),
                      _n("map_sphere", [P, [0, 5, 0], _v(0.5)], 3), _n("math_add", [3, 2], 4)], 4)


def _slab_over_y(mat):
    """box / p.y. Above y = 0 the box is outside (positive over positive), below it inside where z >= -1.5
    (negative over negative), so the quotient is positive there and NaN (0 / 0) on the plane; beside the
    box, z < -1.5, it is +inf at y = +0, -inf at y = -0 and negative below: the half plane y = 0, z < -1.5 is
    the object's visible surface."""
    return _obj(mat, [_n("misc_getY", [P], 0), _n("map_box", [P, SLAB_C, SLAB_R], 1), _n("math_divide", [1, 0], 2)], 2)


# ---- the cases ------------------------------------------------------------------------------------------
EXTRA_MATS = {"varops": 3, "nan_objects": 1, "table40": 2}   # diffuse materials 4.. for the added objects
TABLE40_SEED = 40
_EXTRA_COLOURS = ([0.2, 0.3, 0.8], [0.8, 0.7, 0.2], [0.6, 0.2, 0.7])
_scenes = {}


def scene(name):
    """The case's scene dictionary (the reference's v1 format); a fresh copy."""
    if name not in _scenes:
        mats, objs = _trig_materials(), _trig_objects()
        mats += [_diffuse(4 + k, _EXTRA_COLOURS[k]) for k in range(EXTRA_MATS.get(name, 0))]
        if name == "trig_mat":
            mats[1], mats[2] = _mat1_prog(), _mat2_prog()
        elif name == "varops":
            objs += [_var_sphere(4), _var_box(5), _lattice(6)]
        elif name == "nan_objects":
            objs += [_slab_over_y(4), _edge(2)]   # the NaN object last: on x = 0 it takes the id
        elif name == "table40":
            for kind, m, c, r in _clutter(36, TABLE40_SEED):
                mat = 4 + m % 2   # ids 0 to 2 stay the program objects' own
                nd = _n("map_sphere", [P, c, _v(r)], 0) if kind == "s" else _n("map_box", [P, c, r], 0)
                objs.append(_obj(mat, [nd], 0))
        elif name != "trig":
            raise KeyError(name)
        _scenes[name] = {"materials": mats, "objects": objs}
    return copy.deepcopy(_scenes[name])


def program_ids(name):
    """The material ids of the case's program objects that have a surface (the edge object of nan_objects
    has none: its distance is at least 0.34 wherever it is a number)."""
    return {"varops": (0, 1, 2, 4, 5, 6), "nan_objects": (0, 1, 2, 4)}.get(name, (0, 1, 2))


def tables(name):
    return scene_compile.compile_scene(scene(name), "rm1")


def view():
    return camera.default_view(W, H)


def params(**kw):
    kw.setdefault("max_bounces", MAX_BOUNCES)
    return abi.default_params(**kw)


def oracle_map(tb, pts, max_dist=1000.0):
    """The oracle's map (distance, id) at every float32 point: (n, 2)."""
    import ctypes as C
    from oracle import oracle
    L, fp, s = oracle.lib(), C.POINTER(C.c_float), tb.to_ctypes()
    pts = np.ascontiguousarray(pts, np.float32)
    out = np.zeros((len(pts), 2), np.float32)
    for k in range(len(pts)):
        L.oracle_map(C.byref(s), C.c_float(max_dist), pts[k:k + 1].ctypes.data_as(fp), out[k:k + 1].ctypes.data_as(fp))
    return out


def primary_dirs():
    """The rect's pixel-centre rays of the default camera, float32, row by row."""
    return _primary_dirs(view(), W, H, RECT)


# ---- the points at which map is compared --------------------------------------------------------------
def random_points(name):
    rng = np.random.default_rng(1000 + CASES.index(name))
    return rng.uniform(LO, HI, (N_RANDOM, 3)).astype(np.float32)


def nan_rule_points():
    """Hand-computed points of nan_objects (tests/test_node_family_cpu.py states what map gives at each)."""
    return np.array([(0.0, 5.0, 0.0),      # the edge object NaN; the slab 5 / 5 = 1
                     (-0.0, 5.0, 0.0),     # ... on x = -0
                     (0.0, 2.5, 3.0),      # NaN edge object inside the light's box
                     (1.0, 0.0, -3.0),     # beside the slab, y = +0: +inf
                     (1.0, -0.0, -3.0),    # y = -0: -inf
                     (1.0, 0.0, 1.0),      # on the slab's top face: 0 / 0
                     (0.0, -0.0, 1.0),     # both objects NaN
                     (1.0, -0.5, -3.0),    # below the plane beside the slab: 1.5 / -0.5
                     (0.0, -0.0, -3.0)],   # x = 0 before the slab's near end: -inf, and the NaN edge object's id
                    np.float32)


def edge_points(name):
    """Float32 points, all finite: N_RANDOM seeded uniform ones first, then the coordinate planes at +0 and
    -0, the domain_repeat lattice (varops), large, overflowing, tiny and denormal coordinates."""
    rng = np.random.default_rng(2000 + CASES.index(name))
    parts = [random_points(name)]
    for k in range(3):
        for zero in (0.0, -0.0):
            q = rng.uniform(LO, HI, (50, 3)).astype(np.float32)
            q[:, k] = np.float32(zero)
            parts.append(q)
    if name == "varops":
        for k in range(3):
            m = np.float32(LATTICE_PERIOD[k])
            if m == 0:
                continue
            n = np.arange(-6, 7, dtype=np.float32)
            x = n * m - np.float32(LATTICE_OFFSET[k])     # p + offset is the multiple (up to the sum's rounding)
            for xs in (x, np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))):
                q = rng.uniform((2.0, -0.6, 2.0), (4.0, 1.5, 2.8), (len(xs), 3)).astype(np.float32)
                q[:, k] = xs
                parts.append(q)
    if name == "nan_objects":
        parts.append(nan_rule_points())
    big = []
    for mag in (1e3, 1e6, 3e38):
        u = rng.uniform(-1.0, 1.0, (24, 3))
        u[:6] = np.sign(u[:6])                            # every coordinate at the magnitude
        big.append((u * mag).astype(np.float32))
    parts += big
    half_pi_2_23 = 2.0 ** 23 * np.pi / 2
    parts.append(np.array([(1.1 * half_pi_2_23 / 7, 0.3, -0.4), (-0.2, -2.0 * half_pi_2_23 / 7, 0.1),   # 7 p past the clamp of the reduction
                           (1e38, 0.5, 0.5), (0.5, -2e38, 1e38),                                        # 7 p overflows
                           (1e-30, 0.2, 0.3), (1e-40, 0.2, 0.3), (-1e-40, -1e-30, 1e-40),               # tiny and denormal
                           (1e-40, 5.0, 0.0), (-1e-30, 1e-40, 1.0)], np.float32))
    pts = np.concatenate(parts).astype(np.float32)
    assert np.isfinite(pts).all()
    return pts
