"""Float64 numpy statement of the variance-guided a-trous filter (include/rmr.h rmr_denoise_variance,
DESIGN.md §4.11). A helper, not a test.

Inputs: the accumulator A (the mean of n samples), the half image B (the mean of the odd-indexed
ones), the guide planes HIT and NORMAL, rmr_denoise_params, and sigma_l, var_radius.

lum(v) = (0.2126 v.r + 0.7152 v.g) + 0.0722 v.b, always of a per-channel difference of two colours.

A pixel is v-live iff it is live in denoise_ref's sense for A (id >= 0, A.w != 0, A.rgb finite) and
B.w != 0 and B.rgb is finite; settled once, from A and B. A pixel that is not v-live passes through
every pass, is in no window and no tap, and has variance -1 in both planes.

Seed: d(p) = lum(A(p).rgb - B(p).rgb); var_0(p) = mean of d(q)^2 over the q with |dx|, |dy| <=
var_radius that are on the image, v-live and of p's id.

Pass i = 0 .. iterations-1, step s = 2^i, c_0 = A: for a v-live centre p, w_q is denoise_ref's tap
weight (live read as v-live) times

    l_q = exp(-|lum(c_i(q).rgb - c_i(p).rgb)| / (sigma_l sqrt(max(var_i(p), 0)) + 1e-8)),  w_p = 1;

    c_{i+1}(p).rgb = sum_q k_q w_q c_i(q).rgb / sum_q k_q w_q,   alpha unchanged
    var_{i+1}(p)   = sum_q (k_q w_q)^2 var_i(q) / (sum_q k_q w_q)^2
"""
import numpy as np

from .denoise_ref import FLT_MIN, H5, live_mask

LUM = (0.2126, 0.7152, 0.0722)


def lum(v):
    return (LUM[0] * v[..., 0] + LUM[1] * v[..., 1]) + LUM[2] * v[..., 2]


def vlive_mask(a, b, nrm):
    with np.errstate(invalid="ignore"):
        return live_mask(a, nrm) & (b[..., 3] != 0) & np.isfinite(b[..., :3]).all(axis=-1)


def variance_seed_ref(a, b, nrm, var_radius=3):
    """var_0 as (H, W) float64; -1 where the pixel is not v-live."""
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    nrm = np.asarray(nrm, np.float32)
    H, W = a.shape[:2]
    vl = vlive_mask(a, b, nrm)
    ident = nrm[..., 3]
    with np.errstate(all="ignore"):
        d = lum(a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64))
    d2 = np.where(vl, d * d, 0.0)
    tot = np.zeros((H, W))
    cnt = np.zeros((H, W))
    R = int(var_radius)
    for oy in range(-R, R + 1):
        for ox in range(-R, R + 1):
            py = slice(max(0, -oy), min(H, H - oy))
            px = slice(max(0, -ox), min(W, W - ox))
            if py.start >= py.stop or px.start >= px.stop:
                continue
            qy = slice(py.start + oy, py.stop + oy)
            qx = slice(px.start + ox, px.stop + ox)
            ok = vl[py, px] & vl[qy, qx] & (ident[py, px] == ident[qy, qx])
            tot[py, px] += np.where(ok, d2[qy, qx], 0.0)
            cnt[py, px] += ok
    return np.where(vl, tot / np.maximum(cnt, 1.0), -1.0)


def denoise_variance_ref(a, b, hit, nrm, iterations=5, normal_pow2=5, sigma_z=0.02, sigma_c=0.0,
                         sigma_l=4.0, var_radius=3):
    """a, b, hit, nrm: (H, W, 4) float32. Returns (image (H, W, 4), seed (H, W), filtered variance
    (H, W)) as float64; the sigmas are taken as the float32 values the library receives."""
    sigma_z = float(np.float32(sigma_z))
    sigma_c = float(np.float32(sigma_c))
    sigma_l = float(np.float32(sigma_l))
    a32 = np.asarray(a, np.float32)
    nrm32 = np.asarray(nrm, np.float32)
    c = a32.astype(np.float64)
    n = nrm32[..., :3].astype(np.float64)
    ident = nrm32[..., 3]
    x = np.asarray(hit, np.float32)[..., :3].astype(np.float64)
    t = np.asarray(hit, np.float32)[..., 3].astype(np.float64)
    H, W = c.shape[:2]
    vl = vlive_mask(a32, np.asarray(b, np.float32), nrm32)
    seed = variance_seed_ref(a, b, nrm, var_radius)
    var = seed.copy()
    for i in range(int(iterations)):
        s = 1 << i
        num = np.zeros((H, W, 3))
        den = np.zeros((H, W))
        vnum = np.zeros((H, W))
        inv_l = 1.0 / (sigma_l * np.sqrt(np.maximum(var, 0.0)) + 1e-8)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                k = H5[dx + 2] * H5[dy + 2]
                oy, ox = s * dy, s * dx
                py = slice(max(0, -oy), min(H, H - oy))
                px = slice(max(0, -ox), min(W, W - ox))
                if py.start >= py.stop or px.start >= px.stop:
                    continue
                qy = slice(py.start + oy, py.stop + oy)
                qx = slice(px.start + ox, px.stop + ox)
                if dx == 0 and dy == 0:
                    w = np.ones((H, W))
                    ok = vl.copy()
                else:
                    ok = vl[py, px] & vl[qy, qx] & (ident[py, px] == ident[qy, qx])
                    with np.errstate(all="ignore"):
                        w = np.maximum(0.0, (n[py, px] * n[qy, qx]).sum(-1)) ** (2 ** int(normal_pow2))
                        dz = np.abs((n[py, px] * (x[qy, qx] - x[py, px])).sum(-1))
                        w = w * np.exp(-dz / (sigma_z * s * np.maximum(t[py, px], FLT_MIN)))
                        dc = c[qy, qx, :3] - c[py, px, :3]
                        if sigma_c > 0:
                            w = w * np.exp(-(dc ** 2).sum(-1) / (sigma_c * 2.0 ** -i) ** 2)
                        w = w * np.exp(-np.abs(lum(dc)) * inv_l[py, px])
                with np.errstate(all="ignore"):
                    kw = np.where(ok, k * w, 0.0)
                    num[py, px] += np.where(ok[..., None], kw[..., None] * c[qy, qx, :3], 0.0)
                    vnum[py, px] += np.where(ok, kw * kw * var[qy, qx], 0.0)
                den[py, px] += kw
        out = c.copy()
        with np.errstate(all="ignore"):
            out[..., :3] = np.where(vl[..., None], num / den[..., None], c[..., :3])
            var = np.where(vl, vnum / (den * den), -1.0)
        c = out
    return c, seed, var


def variance_scale(a, b, nrm, var_radius=3):
    """M_v of the GPU comparison's bound |gpu - ref| <= 1e-4 (ref + M_v): the largest reference seed
    variance (0 without a v-live pixel)."""
    s = variance_seed_ref(a, b, nrm, var_radius)
    return float(max(s.max(), 0.0))


def flat_guides(H, W, ids):
    """tests/test_denoise_cpu.py's _flat_guides: a plane z = 5 facing the camera."""
    from .test_denoise_cpu import _flat_guides
    return _flat_guides(H, W, ids)


def synthetic_case(W, H, seed=11):
    """A, B, HIT, NORMAL (H, W, 4) float32 on the flat-plane guides: two ids, a region where A == B
    exactly (variance 0) next to noisy pixels, a 1e4 firefly, 1e-20 and denormal colours, and every kind
    of pixel that is not v-live (sky, A.w = 0, B.w = 0, NaN and inf in A, NaN in B), each where the image
    has room for it. Returns (A, B, hit, nrm, dead): dead lists the (y, x) of the planted pixels."""
    rng = np.random.default_rng(seed)
    split = max(1, int(W * 0.45))
    ids = np.where(np.arange(W)[None, :] < split, 1.0, 4.0) * np.ones((H, 1))
    hit, nrm = flat_guides(H, W, ids)
    a = np.ones((H, W, 4), np.float32)
    a[..., :3] = np.where(ids[..., None] == 1.0, 0.25, 0.7) + rng.uniform(-0.2, 0.2, (H, W, 3))
    b = a.copy()
    b[..., :3] += rng.normal(0.0, 0.08, (H, W, 3)).astype(np.float32)
    # the zero-variance region (distinct colours inside, so its neighbours differ)
    zy, zx = slice(H // 3, H // 3 + 10), slice(W // 2, W // 2 + 12)
    b[zy, zx] = a[zy, zx]

    def put(img, y, x, value):
        if y < H and x < W:
            img[y, x] = value
            return True
        return False
    put(a, 2, 1, (1e4, 2e3, 5e3, 1.0))                       # firefly
    put(a, 3, 3, (1e-20, 1e-20, 1e-20, 1.0))
    put(b, 3, 3, (3e-20, 1e-20, 0.0, 1.0))
    put(a, 4, 2, (1e-40, 3e-40, 2e-41, 1.0))                  # denormals
    put(b, 4, 2, (2e-40, 1e-40, 2e-41, 1.0))
    dead = []
    if put(nrm, 1, 4, (0, 0, 0, -1)):                         # sky
        dead.append((1, 4))
    for y, x, img, value in ((5, 6, a, (0.9, 0.9, 0.9, 0.0)),  # A.w = 0
                             (6, 2, b, (0.5, 0.5, 0.5, 0.0)),  # B.w = 0: fewer than two samples
                             (7, 8, a, (0.4, np.nan, 0.4, 1.0)),
                             (8, 5, a, (np.inf, 0.4, 0.4, 1.0)),
                             (2, 9, b, (0.4, 0.4, np.nan, 1.0))):
        if put(img, y, x, value):
            dead.append((y, x))
    return a, b, hit, nrm, dead
