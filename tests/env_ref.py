"""skyColor's env-map lookup (useEnvTex != 0) in float64 NumPy, written from the reference's text (RM1:78-113 =
RM2:84-107) and GL's rule for texture() on a GL_LINEAR, CLAMP_TO_EDGE, single-level RGBA8 texture (GL 4.5 §8.14.2):

    phi = atan(d.z, d.x); if (phi < 0) phi += 2 PI;  uv = (phi / (2 PI), 1 - (d.y / 2 + 1 / 2))      PI = 3.141592653
    (fu, fv) = (u W - 1/2, v H - 1/2); i0 = floor(fu), j0 = floor(fv); a = fu - i0, b = fv - j0
    tau = (1 - a)(1 - b) T[j0][i0] + a (1 - b) T[j0][i1] + (1 - a) b T[j1][i0] + a b T[j1][i1]        T = c / 255
    with i1 = i0 + 1, j1 = j0 + 1 and every index clamped to [0, W - 1] or [0, H - 1]; row 0 of the map is up.

It shares no code with oracle/rmr_oracle.c's or csrc/rmr_trace.h's sky_color. PI is the float the shader's literal
becomes. GLSL leaves atan(0, 0) undefined; the project defines it as 0 (oracle/detmath.h det_atan2), and so does
this statement: at d = (0, +-1, 0) the column is the project's own choice, not the reference's.

bound() is what a float32 evaluation of the same formula may differ from this statement by, per direction and
channel. The bilinear function is continuous across texel borders and, inside a cell, changes along u by at most
the difference of two horizontally adjacent texels per texel of fu (and likewise along v). A float32 coordinate
that is off by less than one texel lands in the float64 cell or a neighbouring one, so with

    D  the largest minus the smallest texel among the cells around the float64 cell (3 x 3 cells: texels
       i0 - 1 .. i0 + 2, j0 - 1 .. j0 + 2, clamped),
    M  the largest texel among them,
    e = 2^-24, a bound of one float32 rounding relative to a bound of the value rounded,

    |float32 - float64| <= D (Eu + Ev) + 10 e M

  Eu = W ((E_PHI + 4 e) / (2 pi) + e) + 2 W e + e:
         atan2 within E_PHI (2e-5, what tests/test_oracle_math.py holds det_atan2 to); phi + 2 PI rounds a value
         below 8: 4 e; the quotient s <= 1: e; s W and the subtraction of 1/2 round values <= W: 2 W e; a = fu - i0f
         rounds a value <= 1: e.
  Ev = H (2 e) + 2 H e + e:
         d.y / 2 is exact; adding 1/2 and subtracting from 1 round values <= 1: 2 e; then as for u.
  10 e M: c / 255 in float32: e M on every texel. 1 - a: e, so e M on a product; the two products and their sum:
         3 e M; the same for the other row; the second lerp carries those 4 e M through weights that sum to 1 within
         e and adds 1 - b, two products and a sum: 4 e M. 9 e M in all, and one more for the second-order terms.

Nothing here is fitted to a run. Not a test and not a conftest: a helper module like camera_ref.py."""
import numpy as np

PI = float(np.float32(3.141592653))
E = 2.0 ** -24
E_PHI = 2e-5


def texels(env):
    """The map as float64 c / 255, (h, w, 4)."""
    env = np.asarray(env)
    assert env.dtype == np.uint8 and env.ndim == 3 and env.shape[2] == 4
    return env.astype(np.float64) / 255.0


def coordinates(dirs, w, h):
    """(fu, fv) in texels of (n, 3) float32 directions, float64."""
    d = np.asarray(dirs, np.float32).astype(np.float64).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    with np.errstate(invalid="ignore"):
        phi = np.where((x == 0) & (z == 0), 0.0, np.arctan2(z, x))
        phi = np.where(phi < 0, phi + 2 * PI, phi)
        u = phi / (2 * PI)
        v = 1.0 - (y * 0.5 + 0.5)
    return u * w - 0.5, v * h - 0.5


def cell(dirs, w, h):
    """(i0, i1, j0, j1, a, b) of the float64 lookup: clamped indices and the weights. NaN coordinates take texel 0
    with NaN weights."""
    fu, fv = coordinates(dirs, w, h)
    with np.errstate(invalid="ignore"):
        i0f, j0f = np.floor(fu), np.floor(fv)
        a, b = fu - i0f, fv - j0f
    nan = np.isnan(fu) | np.isnan(fv)
    i0f, j0f = np.where(nan, 0.0, i0f), np.where(nan, 0.0, j0f)
    i0, i1 = np.clip(i0f, 0, w - 1).astype(np.int64), np.clip(i0f + 1, 0, w - 1).astype(np.int64)
    j0, j1 = np.clip(j0f, 0, h - 1).astype(np.int64), np.clip(j0f + 1, 0, h - 1).astype(np.int64)
    return i0, i1, j0, j1, a, b


def sky(env, dirs):
    """skyColor(d) with the map bound: (n, 3) float64."""
    T = texels(env)[..., :3]
    h, w = T.shape[:2]
    i0, i1, j0, j1, a, b = cell(dirs, w, h)
    a, b = a[:, None], b[:, None]
    with np.errstate(invalid="ignore"):
        return (1 - a) * (1 - b) * T[j0, i0] + a * (1 - b) * T[j0, i1] + (1 - a) * b * T[j1, i0] + a * b * T[j1, i1]


def selected(env, dirs):
    """The four texels the float64 lookup selects, (n, 4, 3) float64 in the order 00, 10, 01, 11."""
    T = texels(env)[..., :3]
    h, w = T.shape[:2]
    i0, i1, j0, j1, _, _ = cell(dirs, w, h)
    return np.stack([T[j0, i0], T[j0, i1], T[j1, i0], T[j1, i1]], axis=1)


def spread(env, dirs):
    """Largest minus smallest of the four selected texels, per channel: (n, 3)."""
    s = selected(env, dirs)
    return s.max(axis=1) - s.min(axis=1)


def _window(T, lo_i, hi_i, lo_j, hi_j):
    """(max, min) per channel over the texel windows [lo_i, hi_i] x [lo_j, hi_j] (clamped, inclusive)."""
    h, w = T.shape[:2]
    n = len(lo_i)
    mx, mn = np.full((n, 3), -np.inf), np.full((n, 3), np.inf)
    for dj in range(int((hi_j - lo_j).max()) + 1):
        for di in range(int((hi_i - lo_i).max()) + 1):
            jj = np.clip(np.minimum(lo_j + dj, hi_j), 0, h - 1)
            ii = np.clip(np.minimum(lo_i + di, hi_i), 0, w - 1)
            t = T[jj, ii]
            mx, mn = np.maximum(mx, t), np.minimum(mn, t)
    return mx, mn


def coordinate_error(w, h):
    """(Eu, Ev) in texels: the module's text."""
    eu = w * ((E_PHI + 4 * E) / (2 * np.pi) + E) + 2 * w * E + E
    ev = h * (2 * E) + 2 * h * E + E
    return eu, ev


def bound(env, dirs):
    """(n, 3): what a float32 evaluation may differ from sky() by; NaN where the direction is not finite."""
    T = texels(env)[..., :3]
    h, w = T.shape[:2]
    eu, ev = coordinate_error(w, h)
    assert eu < 1 and ev < 1
    fu, fv = coordinates(dirs, w, h)
    nan = np.isnan(fu) | np.isnan(fv)
    i0 = np.floor(np.where(nan, 0.0, fu)).astype(np.int64)
    j0 = np.floor(np.where(nan, 0.0, fv)).astype(np.int64)
    mx, mn = _window(T, i0 - 1, i0 + 2, j0 - 1, j0 + 2)
    out = (mx - mn) * (eu + ev) + 10 * E * mx
    out[nan] = np.nan
    return out


def flat(env, dirs, margin=1.0 / 64):
    """(n,) bool: every texel that a lookup within `margin` texels of the direction's float64 coordinates can
    fetch has the same rgb: the result is that texel whatever the filter's weights are."""
    T = texels(env)[..., :3]
    h, w = T.shape[:2]
    fu, fv = coordinates(dirs, w, h)
    ok = np.isfinite(fu) & np.isfinite(fv)
    fu, fv = np.where(ok, fu, 0.0), np.where(ok, fv, 0.0)
    lo_i, hi_i = np.floor(fu - margin).astype(np.int64), np.floor(fu + margin).astype(np.int64) + 1
    lo_j, hi_j = np.floor(fv - margin).astype(np.int64), np.floor(fv + margin).astype(np.int64) + 1
    mx, mn = _window(T, lo_i, hi_i, lo_j, hi_j)
    return ok & (mx == mn).all(axis=1)
