"""numpy float64 statement of the camera models (include/rmr.h rmr_camera_model) and of
rmr_camera_frame / rmr_check_rays / rmr_check_camera_model, for tests/test_camera_cpu.py and
tests/test_gpu_rays.py.

The random numbers are the reference's rand() chain through the CPU oracle (oracle.rand_chain), so the
chain values and the final rc are the library's bits; everything after them is float64 here, float32
in the generator kernel.
"""
import numpy as np

from oracle import oracle

F = np.float32
TWO_PI = float(F(6.28318548202514648438))
PI = float(F(3.14159274101257324219))

VIEW, THIN_LENS, EQUIRECT, ORTHO = 0, 1, 2, 3


def frame(view):
    """U, V, FWD of a 15-float view in float64 (rmr_camera_frame's statement); None if degenerate."""
    v = np.asarray(view, np.float32).astype(np.float64).reshape(5, 3)
    if not np.isfinite(v).all():
        return None
    r00, r01, r10, r11 = v[1], v[2], v[3], v[4]
    U = r01 - r00
    V = r10 - r00
    Fw = ((r00 + r01) + r10) + r11
    lv, lf = np.linalg.norm(V), np.linalg.norm(Fw)
    if not np.linalg.norm(U) > 0:
        return None
    U = U / np.linalg.norm(U)
    V = V - V.dot(U) * U
    if not np.linalg.norm(V) > 1e-9 * lv:
        return None
    V = V / np.linalg.norm(V)
    Fw = (Fw - Fw.dot(U) * U) - Fw.dot(V) * V
    if not np.linalg.norm(Fw) > 1e-9 * lf:
        return None
    return np.stack([U, V, Fw / np.linalg.norm(Fw)])


def model_ok(model, aperture=0.0, focus=1.0, width=1.0, height=1.0):
    if model in (VIEW, EQUIRECT):
        return True
    if model == THIN_LENS:
        return bool(np.isfinite(aperture) and aperture >= 0 and np.isfinite(focus) and focus > 0)
    if model == ORTHO:
        return bool(np.isfinite(width) and width > 0 and np.isfinite(height) and height > 0)
    return False


def rays_ok(rays):
    for r in np.asarray(rays).reshape(-1):
        vals = [float(r["time"]), float(r["rc"])] + [float(x) for x in r["o"]] + [float(x) for x in r["d"]]
        if not np.isfinite(vals).all():
            return False
        d = np.asarray(r["d"], np.float64)
        if not abs(d.dot(d) - 1.0) <= 1e-5:
            return False
        if not (0 <= int(r["gx"]) < 2 ** 24 and 0 <= int(r["gy"]) < 2 ** 24):
            return False
    return True


def chain(px, py, time, n_calls):
    """The first n_calls values of the pixel sample's rand() chain (float32): main()'s three jitters
    rand(gxt, gyt), rand(gxt, gyt), rand(gyt, gxt), then the thin lens's rand(gxt, gyt), rand(gyt, gxt)."""
    gxt, gyt = F(px) + F(time), F(py) + F(time)
    cos = [(gxt, gyt), (gxt, gyt), (gyt, gxt), (gxt, gyt), (gyt, gxt)][:n_calls]
    return oracle.rand_chain(int(px), int(py), float(time), np.array(cos, np.float32))


def dir0(view, W, H, px, py, j):
    """main()'s jittered corner-ray direction in float64 from the jitters j (RM1:569-584)."""
    v = np.asarray(view, np.float32).astype(np.float64).reshape(5, 3)
    r00, r01, r10, r11 = v[1], v[2], v[3], v[4]
    top = r00 + (r01 - r00) * (px / W + float(j[0]) / W)
    bot = r10 + (r11 - r10) * (px / W + float(j[1]) / W)
    m = top + (bot - top) * (py / H + float(j[2]) / H)
    return m / np.linalg.norm(m)


def ray(model, view, W, H, px, py, time, aperture=0.0, focus=1.0, width=1.0, height=1.0, fr=None):
    """(o, d) in float64, rc (float32) and, for the thin lens, its focus point F (else None)."""
    v = np.asarray(view, np.float32).astype(np.float64).reshape(5, 3)
    eye = v[0]
    lens = model == THIN_LENS and aperture > 0
    c = chain(px, py, time, 5 if lens else 3)
    if model in (VIEW, THIN_LENS):
        d0 = dir0(view, W, H, px, py, c)
        if not lens:
            return eye.copy(), d0, c[-1], (eye + d0 * focus if model == THIN_LENS else None)
        U, V, _ = frame(view) if fr is None else fr
        rad, phi = np.sqrt(float(c[3])), TWO_PI * float(c[4])
        lx, ly = rad * np.cos(phi), rad * np.sin(phi)
        Fp = eye + d0 * float(focus)
        o = eye + U * (float(aperture) * lx) + V * (float(aperture) * ly)
        d = Fp - o
        return o, d / np.linalg.norm(d), c[-1], Fp
    U, V, FWD = frame(view) if fr is None else fr
    u, w = px / W + float(c[0]) / W, py / H + float(c[2]) / H
    if model == EQUIRECT:
        lon, pol = TWO_PI * (u - 0.5), PI * w
        d = U * (np.sin(pol) * np.sin(lon)) + FWD * (np.sin(pol) * np.cos(lon)) - V * np.cos(pol)
        return eye.copy(), d / np.linalg.norm(d), c[-1], None
    if model == ORTHO:
        o = eye + U * ((u - 0.5) * float(width)) + V * ((w - 0.5) * float(height))
        return o, FWD.copy(), c[-1], None
    raise ValueError("unknown model %r" % (model,))


def rays(model, view, W, H, times, rect, **fields):
    """ray() over a rect and seeds: o, d (k, h, w, 3) float64, rc (k, h, w) float32."""
    x0, y0, x1, y1 = rect
    fr = frame(view)
    o = np.zeros((len(times), y1 - y0, x1 - x0, 3))
    d = np.zeros_like(o)
    rc = np.zeros(o.shape[:3], np.float32)
    for k, t in enumerate(times):
        for y in range(y0, y1):
            for x in range(x0, x1):
                o[k, y - y0, x - x0], d[k, y - y0, x - x0], rc[k, y - y0, x - x0], _ = ray(
                    model, view, W, H, x, y, t, fr=fr, **fields)
    return o, d, rc
