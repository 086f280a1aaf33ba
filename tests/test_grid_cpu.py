"""The nearest-primitive cache's candidate grid (rmr_trace.h map_grid_npc; host construction
csrc/grid.cpp), checked on the CPU through the rmr_candidate_grid hook: at random points of the grid
region and at points a float ulp either side of cell boundaries, the cell the kernel's float32 index
arithmetic selects lists the primitive attaining the exact (float64) minimum distance, every unlisted
primitive is above that minimum by more than the grid's margin, and the cell's stored bound is a lower
bound of every unlisted primitive's distance minus the float error bound."""
import json
import os

import numpy as np
import pytest

from raymarchrenderer_amd.renderer import candidate_grid

from .conftest import SCENES

SPHERE, BOX = 1.0, 2.0


def _prims(scene):
    """Leaf-order rows (the large ground box first, as accel.cpp build_bvh orders it)."""
    with open(os.path.join(SCENES, scene)) as f:
        sc = json.load(f)
    rows = []
    for o in sc["objects"]:
        nd = o["nodes"][0]
        c, r = nd["inputs"][1], nd["inputs"][2]
        t = SPHERE if nd["name"] == "map_sphere" else BOX
        rows.append([c[0], c[1], c[2], r[0], r[1], r[2], t, o["matID"]])
    a = np.array(rows, np.float32)
    ext = np.where(a[:, 6:7] == SPHERE, np.abs(a[:, 3:4]), np.abs(a[:, 3:6])).max(1) * 2
    large = ext > 8 * np.median(ext)
    order = np.concatenate([np.nonzero(large)[0], np.nonzero(~large)[0]])
    rr = np.where(a[:, 6:7] == SPHERE, np.abs(a[:, 3:4]), np.abs(a[:, 3:6])).max(1)
    E = float((np.abs(a[:, 0:3]).max(1) + rr).max())
    return a[order], int(large.sum()), E


def _dist(prims, p):
    """Exact (float64) distances of every primitive at points p (N x 3) -> N x n."""
    c = prims[None, :, 0:3].astype(np.float64)
    r = prims[None, :, 3:6].astype(np.float64)
    box = prims[:, 6] == BOX
    v = p[:, None, :] - c
    ds = np.sqrt((v * v).sum(-1)) - r[..., 0]
    q = np.abs(v) - r
    db = np.minimum(q.max(-1), 0.0) + np.sqrt((np.maximum(q, 0.0) ** 2).sum(-1))
    return np.where(box[None, :], db, ds)


def _cells(g, p32):
    lo = g["lo"].astype(np.float32)
    inv = np.float32(g["inv"])
    f = np.floor((p32 - lo) * inv).astype(np.float64)   # float32 arithmetic, as the kernel
    dim = np.array(g["dim"])
    inside = ((f >= 0) & (f < dim)).all(1)
    fi = f.astype(np.int64)
    ci = (fi[:, 2] * dim[1] + fi[:, 1]) * dim[0] + fi[:, 0]
    return inside, ci


@pytest.mark.parametrize("scene,cells", [("csg64.scene", 32768), ("csg256.scene", 65536)])
def test_candidate_grid_lists_the_minimiser(scene, cells):
    prims, n_large, E = _prims(scene)
    g = candidate_grid(prims, n_large, E, target=cells)
    assert g is not None and g["margin"] > 0
    rng = np.random.default_rng(7)
    dim = np.array(g["dim"], np.float64)
    cs = 1.0 / float(g["inv"])
    lo = g["lo"].astype(np.float64)
    # uniform points, and points within a few float ulps of a cell face on every axis
    pu = lo + rng.random((20000, 3)) * dim * cs
    pf = lo + (rng.integers(1, dim.astype(np.int64), size=(20000, 3)).astype(np.float64)) * cs
    pf = pf + rng.integers(-3, 4, size=pf.shape) * np.spacing(np.abs(pf).astype(np.float32)).astype(np.float64)
    pts = np.concatenate([pu, pf]).astype(np.float32)
    inside, ci = _cells(g, pts)
    pts, ci = pts[inside], ci[inside]
    assert len(pts) > 30000
    d = _dist(prims, pts.astype(np.float64))
    cellw = g["cells"][ci]
    cnt = cellw[:, 0] >> 24
    off = cellw[:, 0] & 0xFFFFFF
    bound = cellw[:, 1].view(np.float32)
    checked = 0
    for i in range(len(pts)):
        if cnt[i] == 255:
            continue
        listed = np.zeros(prims.shape[0], bool)
        listed[:n_large] = True
        listed[g["list"][off[i]:off[i] + cnt[i]]] = True
        dmin = d[i].min()
        assert listed[np.argmin(d[i])], "point %s: minimiser not listed" % pts[i]
        if (~listed).any():
            dn = d[i][~listed].min()
            assert dn - dmin > g["margin"], "point %s: unlisted primitive within the margin" % pts[i]
            assert bound[i] <= dn - 0.99 * g["eps"], "point %s: cell bound above an unlisted distance" % pts[i]
        checked += 1
    assert checked > 30000


def test_candidate_grid_declines_without_small_primitives():
    prims, n_large, E = _prims("csg64.scene")
    assert candidate_grid(prims[:1], 1, E) is None
