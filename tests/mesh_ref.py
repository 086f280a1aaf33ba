"""The lattice and the surface-nets rule of rmr_sample_volume / rmr_extract_mesh (include/rmr.h; DESIGN.md
§4.16) as a vectorised NumPy statement: the lattice's float32 coordinates, and on a float32 volume the active
cells, one vertex per active cell (positions in float64) and the quads in the rule's order.

Topology is compared exactly: the vertex count, the quad count and every quad index; the active cell list is
the order of the vertices, which the position bound pins (a vertex lies in its own cell, and the bound is a
small fraction of the spacing).

The position bound, counted from the rule's float32 operations on one coordinate (E = 2^-24, the relative
error of one rounding; the reference runs the same formula in float64 on the same float32 distances and the
same float32 lower corner, so only the roundings below separate them):
  a crossing t = (iso - d0) / (d1 - d0): two subtractions of float32 inputs and a division, 3 E relative on
    t <= 1; at most 4 of a cell's 12 edges run along the coordinate's axis, the other 8 contribute exactly 0
    or 1;
  the sum of m <= 12 contributions, each <= 1: the first addition is exact (0 + c), the j-th partial sum is
    <= j, so the m - 1 additions add at most (2 + ... + m) E = (m (m + 1) / 2 - 1) E;
  the mean: that sum's error over m, at most (m + 1) / 2 E <= 6.5 E, plus the crossings' min(4, m) 3 E / m
    <= 3 E, plus the division's own rounding, E on a mean <= 1: 10.5 E;
  the product with the spacing: one more rounding, 11.5 E spacing; 13 E spacing covers it with every
    second-order term;
  the final addition: half an ulp of the coordinate.
So |x - x_ref| <= 13 E spacing + ulp(|x_ref| + 13 E spacing) / 2."""
import numpy as np

F = np.float32
E = 2.0 ** -24
POSITION_ROUNDINGS = 13.0


def lattice_coords(origin, spacing, shape):
    """The float32 coordinates of the lattice's points per axis: origin[a] + float32(i) * spacing, the product
    rounded, then the sum. shape = (nx, ny, nz)."""
    return [(F(origin[a]) + (np.arange(shape[a]).astype(F) * F(spacing)).astype(F)).astype(F) for a in range(3)]


def lattice_points(origin, spacing, shape):
    """(nz, ny, nx, 3) float32: the points in the volume's index order [iz, iy, ix]."""
    x, y, z = lattice_coords(origin, spacing, shape)
    p = np.empty((shape[2], shape[1], shape[0], 3), F)
    p[..., 0] = x[None, None, :]
    p[..., 1] = y[None, :, None]
    p[..., 2] = z[:, None, None]
    return p


def position_bound(ref, spacing):
    """The bound of the module docstring at the float64 reference positions."""
    b = POSITION_ROUNDINGS * E * float(F(spacing))
    return b + np.spacing((np.abs(ref) + b).astype(F)).astype(np.float64) / 2.0


def _corner(a, k):
    """Corner k (offsets k & 1, k >> 1 & 1, k >> 2 on x, y, z) of every cell of a volume [iz, iy, ix]."""
    dx, dy, dz = k & 1, (k >> 1) & 1, k >> 2
    nz, ny, nx = a.shape
    return a[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]


def surface_nets(dist, origin, spacing, iso=0.0):
    """dist: float32 [iz, iy, ix]. Returns a dict: 'vertices' (V, 3) float64, 'quads' (Q, 4) int64, 'cells' (V,)
    the active cells' linear indices in order, 'crossings' (V,) the cells' crossing-edge counts."""
    d = np.asarray(dist, F)
    nz, ny, nx = d.shape
    iso = F(iso)
    inside = d < iso   # (a NaN is outside, dist == iso is outside)
    d64 = d.astype(np.float64)
    n_in = sum(_corner(inside, k).astype(np.int32) for k in range(8))
    active = (n_in > 0) & (n_in < 8)
    # the sums over the 12 edges: axis a, then (ou, ov) on u = a + 1, v = a + 2 (cyclic)
    s = np.zeros(active.shape + (3,), np.float64)
    count = np.zeros(active.shape, np.int32)
    with np.errstate(all="ignore"):
        for e in range(12):
            a, ou, ov = e >> 2, e & 1, (e >> 1) & 1
            u, v = (a + 1) % 3, (a + 2) % 3
            k0 = (ou << u) | (ov << v)
            k1 = k0 | (1 << a)
            cross = _corner(inside, k0) != _corner(inside, k1)
            d0, d1 = _corner(d64, k0), _corner(d64, k1)
            t = (float(iso) - d0) / (d1 - d0)
            t = np.where((t >= 0.0) & (t <= 1.0), t, 0.5)
            c = np.zeros(active.shape + (3,), np.float64)
            c[..., a] = t
            c[..., u] = ou
            c[..., v] = ov
            s += np.where(cross[..., None], c, 0.0)
            count += cross
    cz, cy, cx = np.nonzero(active)   # (C order: the cells' linear order, x fastest)
    x, y, z = lattice_coords(origin, spacing, (nx, ny, nz))
    corner = np.stack([x[cx], y[cy], z[cz]], axis=-1).astype(np.float64)
    m = count[cz, cy, cx].astype(np.float64)
    vertices = corner + float(F(spacing)) * (s[cz, cy, cx] / m[:, None])
    vidx = np.full(active.shape, -1, np.int64)
    vidx[cz, cy, cx] = np.arange(len(cz))
    # the quads: interior lattice edges whose ends differ, by the lower point's linear index, then by axis
    keys, quads = [], []
    for ax in range(3):
        u, v = (ax + 1) % 3, (ax + 2) % 3
        emit = np.zeros(d.shape, bool)
        lo = [slice(1, -1)] * 3   # indexed [z, y, x]: axis a is dimension 2 - a
        hi = [slice(1, -1)] * 3
        lo[2 - ax], hi[2 - ax] = slice(0, -1), slice(1, None)
        emit[tuple(lo)] = inside[tuple(lo)] != inside[tuple(hi)]
        pz, py, px = np.nonzero(emit)
        p = [px, py, pz]
        cells = []
        for du, dv in ((-1, -1), (0, -1), (0, 0), (-1, 0)):
            c = [None, None, None]
            c[ax], c[u], c[v] = p[ax], p[u] + du, p[v] + dv
            cells.append(vidx[c[2], c[1], c[0]])
        q = np.stack(cells, axis=-1)
        lower_in = inside[pz, py, px]
        q = np.where(lower_in[:, None], q, q[:, ::-1])
        keys.append((px + nx * (py + ny * pz)) * 3 + ax)
        quads.append(q)
    keys, quads = np.concatenate(keys), np.concatenate(quads)
    order = np.argsort(keys, kind="stable")
    return {"vertices": vertices, "quads": quads[order].astype(np.int64).reshape(-1, 4),
            "cells": cx + (nx - 1) * (cy + (ny - 1) * cz), "crossings": count[cz, cy, cx]}


def compare(got_vertices, got_quads, ref, spacing, what=""):
    """Topology exactly, positions within the bound; returns the worst position error over its bound."""
    gv, gq = np.asarray(got_vertices), np.asarray(got_quads)
    assert gv.shape == ref["vertices"].shape, "%s: %d vertices, the rule gives %d" % (what, len(gv), len(ref["vertices"]))
    assert gq.shape == ref["quads"].shape, "%s: %d quads, the rule gives %d" % (what, len(gq), len(ref["quads"]))
    assert (gq.astype(np.int64) == ref["quads"]).all(), "%s: quad indices differ, first at quad %d" % (
        what, np.argmin((gq.astype(np.int64) == ref["quads"]).all(axis=1)))
    if not len(gv):
        return 0.0
    err = np.abs(gv.astype(np.float64) - ref["vertices"])
    bound = position_bound(ref["vertices"], spacing)
    worst = float((err / bound).max())
    print("%s: %d vertices, %d quads, worst position error %.3g = %.3f of the bound" % (
        what, len(gv), len(gq), float(err.max()), worst))
    assert (err <= bound).all(), "%s: %d coordinates off by more than the bound, worst %.3f of it" % (
        what, int((err > bound).sum()), worst)
    return worst


# ---- what a mesh is ---------------------------------------------------------------------------------------
def edge_census(quads):
    """(directed, undirected): for every directed edge (a, b) of the quads its count, and for every undirected
    edge {a, b} the number of quads that share it, as dicts of arrays: keys (n, 2), counts (n,)."""
    q = np.asarray(quads, np.int64).reshape(-1, 4)
    a, b = q.reshape(-1), np.roll(q, -1, axis=1).reshape(-1)
    dk, dc = np.unique(np.stack([a, b], axis=1), axis=0, return_counts=True)
    uk, uc = np.unique(np.stack([np.minimum(a, b), np.maximum(a, b)], axis=1), axis=0, return_counts=True)
    return (dk, dc), (uk, uc)


def euler_number(n_vertices, quads):
    _, (uk, _) = edge_census(quads)
    return int(n_vertices) - len(uk) + len(np.asarray(quads).reshape(-1, 4))


def signed_volume(vertices, quads):
    """The volume the oriented quads enclose (each split (0, 1, 2), (0, 2, 3)); positive for outward normals."""
    v = np.asarray(vertices, np.float64)
    q = np.asarray(quads, np.int64).reshape(-1, 4)
    tri = q[:, [0, 1, 2, 0, 2, 3]].reshape(-1, 3)
    a, b, c = v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


# ---- the lattices the CPU and the GPU tests share ---------------------------------------------------------
# name: (scene, origin, spacing, shape (nx, ny, nz), iso); scene: a file of scenes/, or "nf:<case>" of
# tests/node_family.py. sphere1 is the unit sphere at (0, 1, 0).
CASES = {
    "sphere17": ("sphere1.scene", (-1.5, -0.5, -1.5), 3.0 / 16.0, (17, 17, 17), 0.0),
    "sphere_cut": ("sphere1.scene", (-1.4, -0.3, -1.3), 0.27, (13, 11, 9), 0.0),        # leaves the lattice at z = 0.86
    "sphere_iso": ("sphere1.scene", (-1.5, -0.5, -1.5), 3.0 / 16.0, (17, 17, 17), 0.25),  # the sphere of radius 1.25
    "sphere_empty": ("sphere1.scene", (5.0, 5.0, 5.0), 0.05, (5, 5, 5), 0.0),
    "sphere_full": ("sphere1.scene", (-0.1, 0.9, -0.1), 0.05, (5, 5, 5), 0.0),
    "cornell5": ("cornell5.scene", (-3.3, -1.3, -1.6), 0.33, (21, 18, 10), 0.0),
    "csg_nodes": ("csg_nodes.scene", (-3.5, -1.2, -2.0), 0.3, (24, 10, 14), 0.0),
    "nan_objects": ("nf:nan_objects", (-1.0, -0.5, -2.0), 0.25, (9, 9, 9), 0.0),          # the planes x = 0 and y = 0
}
MAX_DIST = 1000.0   # abi.default_params().max_dist
_volumes = {}
_refs = {}


def case_scene(name):
    """What Renderer.load_scene takes for the case, and the oracle's tables of it."""
    import os
    from oracle import scene_compile
    from .conftest import SCENES
    scene = CASES[name][0]
    if scene.startswith("nf:"):
        from . import node_family as nf
        return nf.scene(scene[3:]), nf.tables(scene[3:])
    path = os.path.join(SCENES, scene)
    return path, scene_compile.load_scene_file(path, "rm1")


def oracle_volume(tables, origin, spacing, shape, max_dist=MAX_DIST):
    """The oracle's map at the lattice's float32 points: (distances, ids), each float32 [iz, iy, ix]."""
    import ctypes as C
    from oracle import oracle
    L, fp, s = oracle.lib(), C.POINTER(C.c_float), tables.to_ctypes()
    pts = np.ascontiguousarray(lattice_points(origin, spacing, shape).reshape(-1, 3))
    out = np.zeros((len(pts), 2), F)
    for k in range(len(pts)):
        L.oracle_map(C.byref(s), C.c_float(max_dist), pts[k:k + 1].ctypes.data_as(fp), out[k:k + 1].ctypes.data_as(fp))
    nz_ny_nx = (shape[2], shape[1], shape[0])
    return out[:, 0].reshape(nz_ny_nx).copy(), out[:, 1].reshape(nz_ny_nx).copy()


def case_volume(name):
    """The oracle's distances of the case's lattice, once per process; not to be written to."""
    if name not in _volumes:
        _, origin, spacing, shape, _ = CASES[name]
        _volumes[name] = oracle_volume(case_scene(name)[1], origin, spacing, shape)[0]
        _volumes[name].setflags(write=False)
    return _volumes[name]


def case_ref(name):
    """surface_nets of the case on the oracle's volume, once per process."""
    if name not in _refs:
        _, origin, spacing, _, iso = CASES[name]
        _refs[name] = surface_nets(case_volume(name), origin, spacing, iso)
    return _refs[name]
