"""The tone-mapping stage's rule (include/rmr.h) as a NumPy statement: float32 arrays
throughout with every product and sum rounded on its own, np.fmax / np.fmin for the NaN rules, and a
Python loop in bin order for the meter (float64)."""
import math

import numpy as np

F = np.float32
LINEAR, REINHARD, ACES = 0, 1, 2
BIAS = (127 - 16) << 3


def luminance(rgba):
    a = np.ascontiguousarray(rgba, F).reshape(-1, 4)
    with np.errstate(all="ignore"):
        return (F(0.2126) * a[:, 0] + F(0.7152) * a[:, 1]) + F(0.0722) * a[:, 2]


def bins_ref(rgba):
    """(n,) int32: the bin of each pixel, -1 for a skipped one."""
    a = np.ascontiguousarray(rgba, F).reshape(-1, 4)
    L = luminance(a)
    with np.errstate(all="ignore"):
        counted = (a[:, 3] != 0) & np.isfinite(a[:, 0]) & np.isfinite(a[:, 1]) & np.isfinite(a[:, 2]) & np.isfinite(L) & (L >= 0)
    bits = L.view(np.uint32) & np.uint32(0x7FFFFFFF)   # (L = -0 is counted and belongs to bin 0)
    k = np.clip((bits >> np.uint32(20)).astype(np.int64) - BIAS, 0, 255)
    return np.where(counted, k, -1).astype(np.int32)


def hist_ref(rgba):
    """(hist (256,) uint32, skipped)."""
    b = bins_ref(rgba)
    return np.bincount(b[b >= 0], minlength=256).astype(np.uint32), int((b < 0).sum())


def bin_lower_edge(b):
    """The smallest float32 of bin b (1..255)."""
    return np.array([(b + BIAS) << 20], np.uint32).view(F)[0]


def lc_table():
    """lc[b] for b = 1..255 (index 0 unused)."""
    lc = [0.0] * 256
    for b in range(1, 256):
        e, m = (b >> 3) - 16, b & 7
        lc[b] = float(e) + math.log2(1.0 + (m + 0.5) / 8.0)
    return lc


_LC = lc_table()


def meter_target(hist, key=0.18, low_pct=0.10, high_pct=0.90, exposure_ev=0.0):
    """l_target of a histogram, or None when nothing is metered (N == 0)."""
    n = [int(x) for x in np.asarray(hist).reshape(256)]
    N = sum(n[1:])
    if N == 0:
        return None
    lo, hi = float(F(low_pct)) * float(N), float(F(high_pct)) * float(N)
    C = sw = swl = 0.0
    for b in range(1, 256):
        c1 = C + float(n[b])
        a, z = max(C, lo), min(c1, hi)
        w = z - a if z > a else 0.0
        swl = swl + w * _LC[b]
        sw = sw + w
        C = c1
    return (math.log2(float(F(key))) - swl / sw) + float(F(exposure_ev))


def meter_ref(hist, l_prev=None, key=0.18, low_pct=0.10, high_pct=0.90, adapt=1.0, exposure_ev=0.0):
    """l of the metering rule; l_prev None: no previous state."""
    t = meter_target(hist, key, low_pct, high_pct, exposure_ev)
    if t is None:
        return l_prev if l_prev is not None else float(F(exposure_ev))
    if l_prev is None:
        return t
    return l_prev + float(F(adapt)) * (t - l_prev)


def curve_ref(curve, rgba, scale, white=4.0):
    """The curve on (..., 4) float32 pixels at `scale`; alpha passes through."""
    a = np.ascontiguousarray(rgba, F)
    out = a.copy()
    c = a[..., :3]
    s = F(scale)
    with np.errstate(all="ignore"):
        x = np.fmax(c * s, F(0)) + F(0)   # (+ 0: a -0 product reads as +0)
        if curve == LINEAR:
            v = x
        elif curve == REINHARD:
            iw2 = F(1.0 / (float(F(white)) * float(F(white))))
            v = (x * (F(1) + x * iw2)) / (F(1) + x)
        else:
            num = x * (F(2.51) * x + F(0.03))
            den = x * (F(2.43) * x + F(0.59)) + F(0.14)
            v = num / den
        out[..., :3] = np.fmax(np.fmin(v, F(1)), F(0))
    assert out.dtype == F
    return out
