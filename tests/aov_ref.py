"""A NumPy statement of the sampled AOVs' rule (include/rmr.h rmr_render_aov; csrc/rmr_aov_rule.h): the fold
in float32, one IEEE operation per step in the rule's order (so it gives the library's bits), the resolve in
float64 (the reference the library's float32 resolve is bounded against), and the oracle's first hits of a
ray list as the rmr_hit records the fold takes."""
import ctypes as C

import numpy as np

from oracle import oracle
from raymarchrenderer_amd import abi

F = np.float32
HIT = np.dtype(abi.HIT_DTYPE)
STATS, NORMAL, POSITION, IDS01, IDS23 = range(5)


def init(n_px):
    s = np.zeros((5, n_px, 4), F)
    s[STATS, :, 3] = np.inf
    s[IDS01, :, 0::2] = -1.0
    s[IDS23, :, 0::2] = -1.0
    return s


def fold(state, hits):
    """hits (nspp, n_px) of HIT folded into a copy of the (5, n_px, 4) state, sample 0 first."""
    s = np.array(state, F)
    hits = np.asarray(hits, HIT).reshape(-1, s.shape[1])
    one = F(1.0)
    for h in hits:
        hit = h["id"] >= 0
        s[STATS, :, 0] = s[STATS, :, 0] + one
        s[STATS, hit, 1] = s[STATS, hit, 1] + one
        s[STATS, hit, 2] = s[STATS, hit, 2] + h["t"][hit]
        s[STATS, hit, 3] = np.where(h["t"][hit] < s[STATS, hit, 3], h["t"][hit], s[STATS, hit, 3])
        for k in range(3):
            s[NORMAL, hit, k] = s[NORMAL, hit, k] + h["n"][hit, k]
            s[POSITION, hit, k] = s[POSITION, hit, k] + h["pos"][hit, k]
        ids = np.stack([s[IDS01, :, 0], s[IDS01, :, 2], s[IDS23, :, 0], s[IDS23, :, 2]], axis=1)
        cnt = np.stack([s[IDS01, :, 1], s[IDS01, :, 3], s[IDS23, :, 1], s[IDS23, :, 3]], axis=1)
        todo = hit.copy()
        for j in range(4):   # the first slot holding the id
            m = todo & (ids[:, j] == h["id"])
            cnt[m, j] = cnt[m, j] + one
            todo &= ~m
        for j in range(4):   # else the first empty slot
            m = todo & (ids[:, j] == -1.0)
            ids[m, j] = h["id"][m]
            cnt[m, j] = one
            todo &= ~m
        s[NORMAL, todo, 3] = s[NORMAL, todo, 3] + one   # else `other`
        s[IDS01, :, 0], s[IDS01, :, 2], s[IDS23, :, 0], s[IDS23, :, 2] = ids.T
        s[IDS01, :, 1], s[IDS01, :, 3], s[IDS23, :, 1], s[IDS23, :, 3] = cnt.T
    return s


def resolve64(state, max_dist):
    """The resolve in float64 from the float32 state: (5, n_px, 4) float64 in the resolved planes' order."""
    s = np.asarray(state, F).astype(np.float64)
    n_px = s.shape[1]
    out = np.zeros((5, n_px, 4))
    n, h = s[STATS, :, 0], s[STATS, :, 1]
    hn, hh = np.maximum(n, 1.0), np.maximum(h, 1.0)
    alpha = np.where(n > 0, h / hn, 0.0)
    md = float(F(max_dist))
    out[0, :, 0] = np.where(h > 0, s[STATS, :, 2] / hh, md)
    out[0, :, 1] = np.where(h > 0, s[STATS, :, 3], md)
    out[0, :, 2] = alpha
    out[0, :, 3] = n
    N = s[NORMAL, :, :3]
    ln = np.sqrt((N * N).sum(axis=1))
    ok = (h > 0) & (ln > 0) & np.isfinite(ln)
    out[1, :, :3] = np.where(ok[:, None], N / np.where(ok, ln, 1.0)[:, None], 0.0)
    out[1, :, 3] = alpha
    out[2, :, :3] = np.where((h > 0)[:, None], s[POSITION, :, :3] / hh[:, None], 0.0)
    out[2, :, 3] = np.where(h > 0, h, 0.0)
    ids = np.stack([s[IDS01, :, 0], s[IDS01, :, 2], s[IDS23, :, 0], s[IDS23, :, 2]], axis=1)
    cnt = np.stack([s[IDS01, :, 1], s[IDS01, :, 3], s[IDS23, :, 1], s[IDS23, :, 3]], axis=1)
    for i in range(n_px):
        order = sorted(range(4), key=lambda j: (ids[i, j] < 0, -cnt[i, j], ids[i, j]))
        for k, j in enumerate(order):
            out[3 + k // 2, i, 2 * (k % 2)] = ids[i, j]
            out[3 + k // 2, i, 2 * (k % 2) + 1] = cnt[i, j] / n[i] if ids[i, j] >= 0 else 0.0
    return out


def fma32(a, b, c):
    """fmaf(a, b, c) of float32 arrays, correctly rounded: the product is exact in float64, TwoSum gives the
    sum's rounding error, and the float32 rounding of the float64 sum is corrected where it was a tie that
    the error breaks."""
    a, b, c = (np.asarray(x, F).astype(np.float64) for x in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    r = s.astype(F)
    d = s - r.astype(np.float64)
    toward = np.where(d > 0, np.inf, -np.inf).astype(F)
    other = np.nextafter(r, toward)
    tie = (d != 0) & (s == (r.astype(np.float64) + other.astype(np.float64)) / 2)
    wrong = tie & (np.sign(e) == np.sign(d))
    return np.where(wrong, other, r).astype(F)


def oracle_hits(tables, prm, rays):
    """The oracle's first hit of each ray of an abi.RAY_DTYPE array (any shape), as rmr_cast_rays states it:
    march, the far-hit rule, pos = fma(d, t, o), getNormal at the hits; HIT records of the rays' shape."""
    L = oracle.lib()
    fp = C.POINTER(C.c_float)
    sc = tables.to_ctypes()
    flat = np.ascontiguousarray(rays).reshape(-1)
    o = np.ascontiguousarray(flat["o"], F)
    d = np.ascontiguousarray(flat["d"], F)
    td = np.zeros((len(flat), 2), F)
    for k in range(len(flat)):
        L.oracle_march(C.byref(sc), C.byref(prm), o[k:k + 1].ctypes.data_as(fp), d[k:k + 1].ctypes.data_as(fp),
                       C.c_float(1.0), td[k:k + 1].ctypes.data_as(fp))
    out = np.zeros(len(flat), HIT)
    out["t"] = td[:, 0]
    out["id"] = np.where(td[:, 0] < F(prm.max_dist), td[:, 1], F(-1.0))
    out["pos"] = fma32(d, td[:, 0:1], o)
    pos = np.ascontiguousarray(out["pos"])
    nrm = np.zeros((len(flat), 3), F)
    for k in np.flatnonzero(out["id"] >= 0):
        L.oracle_normal(C.byref(sc), C.c_float(prm.max_dist), pos[k:k + 1].ctypes.data_as(fp),
                        nrm[k:k + 1].ctypes.data_as(fp))
    out["n"] = nrm
    return out.reshape(np.shape(rays))


def overflow_scene():
    """A v1 scene of eight diffuse materials for the slot-overflow case: around the origin (where the test
    puts the eye), above the horizon a shell of 40 small spheres whose materials cycle through all eight, below
    it three large spheres of materials 0, 1 and 2 with sky between them."""
    def diffuse(i):
        return {"id": i, "total_vars": 2, "color": 0, "dir": 1,
                "nodes": [{"name": "shader_diffuse", "inputs": [[0.1 * (i + 1), 0.5, 0.9 - 0.1 * i]], "outputs": [0, 1]}]}

    def sphere(mat, c, rad):
        return {"matID": mat, "total_vars": 1, "distance": 0,
                "nodes": [{"name": "map_sphere", "inputs": [-1, [round(float(x), 3) for x in c], [rad, rad, rad]],
                           "outputs": [0]}]}
    objs = []
    k = 0
    for ring, (elev, count) in enumerate([(15.0, 16), (40.0, 14), (65.0, 10)]):
        for j in range(count):
            az = np.radians(360.0 * j / count + 11.0 * ring)
            el = np.radians(elev)
            c = 4.0 * np.array([np.cos(el) * np.sin(az), np.sin(el), np.cos(el) * np.cos(az)])
            objs.append(sphere((k * 3 + ring) % 8, c, 1.0))
            k += 1
    objs.append(sphere(0, (3.0, -4.0, 3.0), 2.5))
    objs.append(sphere(1, (3.0, -4.0, 0.0), 2.0))
    objs.append(sphere(2, (-3.0, -4.0, -3.0), 2.5))
    return {"materials": [diffuse(i) for i in range(8)], "objects": objs}
