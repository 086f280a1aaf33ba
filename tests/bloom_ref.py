"""The bloom stage's rule (include/rmr.h rmr_bloom) in NumPy, twice: bloom_f32 in float32
in the rule's exact order of operations (what rmr_bloom_pixels and the kernels must equal bit for bit), and
bloom_f64, the same statement in float64 (the float32 constants and parameters widened, every decision
taken in float64 except the two the rule takes on float32 values: a pixel's validity and L's finiteness).

Images are (H, W, 4) float32; x is axis 1."""
import numpy as np

F = np.float32
D = np.float64
DEFAULTS = dict(levels=5, threshold=1.0, clamp=0.0, scatter=0.7, intensity=0.2)


def level_sizes(w, h, levels):
    out = [(w, h)]
    for _ in range(levels):
        w, h = (w + 1) >> 1, (h + 1) >> 1
        out.append((w, h))
    return out


def gain(intensity, scatter, levels, dt=F):
    """(float)((double)I / (p_0 + ... + p_{N-1})), p_0 = 1, p_j = p_{j-1} (double)s; in float64: not rounded."""
    total, p = D(0.0), D(1.0)
    for _ in range(levels):
        total = total + p
        p = p * D(F(scatter))
    g = D(F(intensity)) / total
    return F(g) if dt is F else g


def invalid(img):
    img = np.asarray(img, F)
    return (img[..., 3] == 0) | ~np.isfinite(img[..., :3]).all(axis=-1)


def bright(img, threshold, clamp, dt):
    img = np.asarray(img, F)
    T, cl = dt(F(threshold)), dt(F(clamp))
    rgb = img[..., :3].astype(dt)
    with np.errstate(all="ignore"):
        c = np.where(rgb > 0, rgb, dt(0.0))
        L = (dt(F(0.2126)) * c[..., 0] + dt(F(0.7152)) * c[..., 1]) + dt(F(0.0722)) * c[..., 2]
        e = L - T
        zero = invalid(img) | ~np.isfinite(L.astype(F)) | ~(e > 0)
        if cl > 0:
            e = np.where(e > cl, cl, e)
        f = e / L
        p = c * f[..., None]
    return np.where(zero[..., None], dt(0.0), p).astype(dt)


def _down_axis(a, axis, dt):
    n = a.shape[axis]
    i = 2 * np.arange((n + 1) >> 1)

    def t(idx):
        return np.take(a, np.clip(idx, 0, n - 1), axis=axis)
    with np.errstate(all="ignore"):
        return ((t(i - 1) + t(i + 2)) + dt(3.0) * (t(i) + t(i + 1))) * dt(0.125)


def down(a, dt):
    return _down_axis(_down_axis(a, 1, dt), 0, dt)


def _up_axis(b, n, axis, dt):
    m = b.shape[axis]
    i = np.arange(n)
    j = i >> 1
    far = np.clip(np.where(i & 1, j + 1, j - 1), 0, m - 1)
    with np.errstate(all="ignore"):
        return (dt(3.0) * np.take(b, j, axis=axis) + np.take(b, far, axis=axis)) * dt(0.25)


def up(b, w, h, dt):
    return _up_axis(_up_axis(b, w, 1, dt), h, 0, dt)


def spread(img, levels, threshold, clamp, scatter, dt):
    """G = up(U_1) of the rule, (H, W, 3)."""
    H, W = img.shape[:2]
    s = dt(F(scatter))
    B = [bright(img, threshold, clamp, dt)]
    for _ in range(levels):
        B.append(down(B[-1], dt))
    U = B[levels]
    with np.errstate(all="ignore"):
        for k in range(levels - 1, 0, -1):
            U = B[k] + s * up(U, B[k].shape[1], B[k].shape[0], dt)
    return up(U, W, H, dt)


def _bloom(img, dt, levels, threshold, clamp, scatter, intensity):
    img = np.ascontiguousarray(img, F)
    G = spread(img, levels, threshold, clamp, scatter, dt)
    g = gain(intensity, scatter, levels, dt)
    out = img.astype(dt)
    with np.errstate(all="ignore"):
        out[..., :3] = out[..., :3] + g * G
    bad = invalid(img)
    out[bad] = img[bad].astype(dt)
    out[..., 3] = img[..., 3].astype(dt)
    if dt is F:   # the copies are bit for bit (a NaN's payload, a zero's sign)
        o = out.view(np.uint32)
        o[bad] = img.view(np.uint32)[bad]
        o[..., 3] = img.view(np.uint32)[..., 3]
    return out


def bloom_f32(img, **kw):
    p = dict(DEFAULTS, **kw)
    return _bloom(img, F, **p)


def bloom_f64(img, **kw):
    p = dict(DEFAULTS, **kw)
    return _bloom(img, D, **p)
