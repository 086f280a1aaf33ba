"""Float64 numpy statement of the edge-avoiding a-trous preview filter (include/rmr.h rmr_denoise,
DESIGN.md §4.7), and the first-hit guides it needs from the CPU oracle. A helper, not a test.

Pass i = 0 .. iterations-1, step s = 2^i, c_0 = the accumulator. A pixel is live iff its guide
id >= 0, its alpha != 0 and its current rgb is finite. For a live centre p, with
h = (1/16, 1/4, 3/8, 1/4, 1/16) and taps q = p + s (dx, dy), dx, dy in [-2, 2]:

    c_{i+1}(p).rgb = sum_q k_q w_q c_i(q).rgb / sum_q k_q w_q,  k_q = h[dx+2] h[dy+2],  alpha unchanged
    w_p = 1;  w_q = 0 if q is off the image or not live, else
    w_q = [id_q == id_p] max(0, n_p.n_q)^(2^normal_pow2)
          exp(-|n_p.(x_q - x_p)| / (sigma_z s max(t_p, FLT_MIN)))
          (sigma_c > 0 ? exp(-|c_i(q).rgb - c_i(p).rgb|^2 / (sigma_c 2^-i)^2) : 1)

A centre that is not live keeps its value.
"""
import ctypes as C

import numpy as np

H5 = np.array([1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16])
FLT_MIN = float(np.finfo(np.float32).tiny)


def live_mask(rgba, nrm):
    with np.errstate(invalid="ignore"):
        return (nrm[..., 3] >= 0) & (rgba[..., 3] != 0) & np.isfinite(rgba[..., :3]).all(axis=-1)


def denoise_ref(accum, hit, nrm, iterations=5, normal_pow2=5, sigma_z=0.02, sigma_c=0.0):
    """accum, hit, nrm: (H, W, 4) float32 (the accumulator, RMR_GUIDE_HIT, RMR_GUIDE_NORMAL). Returns
    the filtered image as (H, W, 4) float64; sigma_z / sigma_c are taken as the float32 values the
    library receives."""
    sigma_z = float(np.float32(sigma_z))
    sigma_c = float(np.float32(sigma_c))
    c = np.asarray(accum, np.float32).astype(np.float64)
    n = np.asarray(nrm, np.float32)[..., :3].astype(np.float64)
    ident = np.asarray(nrm, np.float32)[..., 3]
    x = np.asarray(hit, np.float32)[..., :3].astype(np.float64)
    t = np.asarray(hit, np.float32)[..., 3].astype(np.float64)
    H, W = c.shape[:2]
    for i in range(int(iterations)):
        s = 1 << i
        live = live_mask(c, np.asarray(nrm, np.float32))
        num = np.zeros((H, W, 3))
        den = np.zeros((H, W))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                k = H5[dx + 2] * H5[dy + 2]
                oy, ox = s * dy, s * dx
                # centres p whose tap q = p + (ox, oy) is on the image
                py = slice(max(0, -oy), min(H, H - oy))
                px = slice(max(0, -ox), min(W, W - ox))
                if py.start >= py.stop or px.start >= px.stop:
                    continue
                qy = slice(py.start + oy, py.stop + oy)
                qx = slice(px.start + ox, px.stop + ox)
                if dx == 0 and dy == 0:
                    w = np.ones((H, W))
                    ok = live.copy()
                else:
                    ok = live[py, px] & live[qy, qx] & (ident[py, px] == ident[qy, qx])
                    with np.errstate(all="ignore"):
                        w = np.maximum(0.0, (n[py, px] * n[qy, qx]).sum(-1)) ** (2 ** int(normal_pow2))
                        dz = np.abs((n[py, px] * (x[qy, qx] - x[py, px])).sum(-1))
                        w = w * np.exp(-dz / (sigma_z * s * np.maximum(t[py, px], FLT_MIN)))
                        if sigma_c > 0:
                            d2 = ((c[qy, qx, :3] - c[py, px, :3]) ** 2).sum(-1)
                            w = w * np.exp(-d2 / (sigma_c * 2.0 ** -i) ** 2)
                with np.errstate(all="ignore"):
                    kw = np.where(ok, k * w, 0.0)
                    num[py, px] += np.where(ok[..., None], kw[..., None] * c[qy, qx, :3], 0.0)
                den[py, px] += kw
        out = c.copy()
        with np.errstate(all="ignore"):
            out[..., :3] = np.where(live[..., None], num / den[..., None], c[..., :3])
        c = out
    return c


def tolerance_scale(accum, nrm):
    """M of the GPU comparison's bound |gpu - ref| <= 1e-4 (|ref| + M): the largest finite |rgb| over
    live input pixels (0 without any)."""
    a = np.asarray(accum, np.float32)
    live = live_mask(a, np.asarray(nrm, np.float32))
    return float(np.abs(a[..., :3][live]).max()) if live.any() else 0.0


def pixel_centre_dirs(view, W, H):
    """Float64 evaluation of the guide pass's ray formula from the float32 view (eye, ray00, ray01,
    ray10, ray11): u = px / W + 0.5 / W, v = py / H + 0.5 / H,
    dir = normalize(mix(ray00 + (ray01 - ray00) u, ray10 + (ray11 - ray10) u, v)). (H, W, 3)."""
    v = np.asarray(view, np.float32).reshape(5, 3)
    r00, r01, r10, r11 = (v[k].astype(np.float64) for k in (1, 2, 3, 4))
    # the kernel takes r01 - r00 and r11 - r10 as float32 differences (rmr_internal.h KParams dr01 / dr11)
    d0 = (v[2] - v[1]).astype(np.float64)
    d1 = (v[4] - v[3]).astype(np.float64)
    u = (np.arange(W, dtype=np.float64) / W + 0.5 / W)[None, :, None]
    w = (np.arange(H, dtype=np.float64) / H + 0.5 / H)[:, None, None]
    top = r00 + d0 * u
    bot = r10 + d1 * u
    d = top + (bot - top) * w
    return d / np.sqrt((d * d).sum(-1, keepdims=True))


def oracle_march(tables, prm, eye, dirs):
    """The CPU oracle's march(eye, dir, +1) for float32 directions dirs (..., 3): (t, id) as march
    returns them (a hit it returns at t >= max_dist keeps its id here)."""
    from oracle import oracle
    L = oracle.lib()
    fp = C.POINTER(C.c_float)
    s = tables.to_ctypes()
    dirs = np.ascontiguousarray(dirs, np.float32)
    flat = dirs.reshape(-1, 3)
    eye = np.ascontiguousarray(eye, np.float32)
    out = np.zeros((len(flat), 2), np.float32)
    for k in range(len(flat)):
        L.oracle_march(C.byref(s), C.byref(prm), eye.ctypes.data_as(fp), flat[k:k + 1].ctypes.data_as(fp),
                       C.c_float(1.0), out[k:k + 1].ctypes.data_as(fp))
    shape = dirs.shape[:-1]
    return out[:, 0].reshape(shape), out[:, 1].reshape(shape)


def far_hit_rule(t, ident, max_dist):
    """The guide pass's id: a pixel is a hit iff t < max_dist; everything else is a miss, id -1."""
    return np.where(t < np.float32(max_dist), ident, np.float32(-1.0)).astype(np.float32)


def oracle_normals(tables, max_dist, points, mask):
    """The CPU oracle's getNormal at the float32 points (..., 3) where mask, (0, 0, 0) elsewhere."""
    from oracle import oracle
    L = oracle.lib()
    fp = C.POINTER(C.c_float)
    s = tables.to_ctypes()
    points = np.ascontiguousarray(points, np.float32)
    flat = points.reshape(-1, 3)
    m = np.asarray(mask, bool).reshape(-1)
    out = np.zeros((len(flat), 3), np.float32)
    for k in np.flatnonzero(m):
        L.oracle_normal(C.byref(s), C.c_float(max_dist), flat[k:k + 1].ctypes.data_as(fp), out[k:k + 1].ctypes.data_as(fp))
    return out.reshape(points.shape)


def oracle_guides(tables, prm, view, W, H):
    """HIT and NORMAL planes (H, W, 4) float32 from the CPU oracle at the pixel-centre rays (the
    directions and positions rounded from float64: the planes the GPU pass gives up to the last bit)."""
    dirs = pixel_centre_dirs(view, W, H).astype(np.float32)
    eye = np.asarray(view, np.float32).reshape(5, 3)[0]
    t, ident = oracle_march(tables, prm, eye, dirs)
    ident = far_hit_rule(t, ident, prm.max_dist)
    pos = (eye.astype(np.float64) + dirs.astype(np.float64) * t[..., None].astype(np.float64)).astype(np.float32)
    nrm = oracle_normals(tables, prm.max_dist, pos, ident >= 0)
    hit = np.concatenate([pos, t[..., None]], axis=-1).astype(np.float32)
    nr = np.concatenate([nrm, ident[..., None]], axis=-1).astype(np.float32)
    return hit, nr
