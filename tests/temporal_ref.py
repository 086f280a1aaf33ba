"""Float64 numpy statement of the temporal reprojection stage (include/rmr.h rmr_temporal_accumulate,
DESIGN.md §4.12), the counted coordinate bound of rmr.h, and synthetic two-view cases. A helper, not a
test.

S: the source image with sample count n_cur; HIT, NORMAL: the current guides; Hc, Hn, Hhit, Hnrm: the
history's colour, count and guides; (eye', r00', r01', r10', r11'): the history's view.

1. p is live iff id >= 0, S.a != 0 and S.rgb is finite; otherwise out = S, n_out = 0.
2. The history's guide ray at (u, v) is B(u, v) = mix(mix(r00', r01', u), mix(r10', r11', u), v). Solve
   lambda B(u, v) = x - eye' with lambda > 0 (here: Newton on the full bilinear system in float64, to
   convergence, from the affine solution); fx = u W, fy = v H. No history when lambda <= 0 or (fx, fy)
   is not finite.
3. q0 = floor((fx, fy) - 0.5); the taps q0 + {0,1}^2 with bilinear weights b_q weigh
   g_q = b_q [q on the image] [Hn(q) > 0] [Hid(q) == id] max(0, n.n_q)^(2^normal_pow2)
         exp(-|n.(x_q - x)| / (sigma_z max(t, FLT_MIN))).
4. G = sum g_q, h = sum g_q Hc(q) / G, m = min(max_history, sum g_q Hn(q));
   out.rgb = (m h + n_cur S.rgb) / (m + n_cur), out.a = S.a, n_out = min(m + n_cur, max_history);
   G == 0, m == 0 or h not finite: out = S, n_out = min(n_cur, max_history).
"""
import numpy as np

from .denoise_ref import FLT_MIN, live_mask

EPS = 2.0 ** -24


def view_basis(view):
    """(eye, r00, a, b, c) in float64 of a float32 view: B(u, v) = r00 + u a + v b + u v c."""
    v = np.asarray(view, np.float32).reshape(5, 3).astype(np.float64)
    eye, r00, r01, r10, r11 = v
    return eye, r00, r01 - r00, r10 - r00, (r11 - r10) - (r01 - r00)


def guide_dirs(view, W, H, u=None, v=None):
    """B(u, v) (not normalised) at the pixel centres, or at the given coordinates."""
    _, r00, a, b, c = view_basis(view)
    if u is None:
        u = ((np.arange(W) + 0.5) / W)[None, :]
        v = ((np.arange(H) + 0.5) / H)[:, None]
    u = np.asarray(u, np.float64)[..., None]
    v = np.asarray(v, np.float64)[..., None]
    return r00 + u * a + v * b + (u * v) * c


def project_ref(x, h_view, iterations=60):
    """(U, V, w) with lambda = w, u = U / w, v = V / w of the points x (..., 3) in the view h_view."""
    eye, r00, a, b, c = view_basis(h_view)
    M = np.stack([a, b, r00], axis=1)
    d = np.asarray(x, np.float64) - eye
    shape = d.shape[:-1]
    d = d.reshape(-1, 3)
    with np.errstate(all="ignore"):
        s = np.linalg.solve(M, d.T).T
        if np.abs(c).max() > 0:
            for _ in range(iterations):
                U, V, w = s[:, 0], s[:, 1], s[:, 2]
                F = s @ M.T + ((U * V / w)[:, None]) * c - d
                g = np.stack([V / w, U / w, -U * V / (w * w)], axis=1)
                J = M[None] + c[None, :, None] * g[:, None, :]
                ok = np.isfinite(J).all(axis=(1, 2)) & np.isfinite(F).all(axis=1)
                step = np.zeros_like(s)
                if ok.any():
                    try:
                        step[ok] = np.linalg.solve(J[ok], F[ok][..., None])[..., 0]
                    except np.linalg.LinAlgError:
                        break
                s = np.where(ok[:, None], s - step, np.nan)
    return s[:, 0].reshape(shape), s[:, 1].reshape(shape), s[:, 2].reshape(shape)


def coordinate_bound(x, h_view, minv, k, W, H):
    """rmr.h's counted bound on |fx - fx*|, |fy - fy*| (two (...) float64 arrays; inf where the bound's
    condition |A C| <= B^2 / 16 does not hold). minv (3, 3), k (3,): rmr_temporal_view_inverse's output
    rounded to float32 (the kernel's operands)."""
    eye = np.asarray(h_view, np.float32).reshape(5, 3)[0].astype(np.float64)
    Mi = np.asarray(minv, np.float32).astype(np.float64)
    kk = np.asarray(k, np.float32).astype(np.float64)
    K = np.abs(kk)
    d = np.asarray(x, np.float64) - eye
    with np.errstate(all="ignore"):
        s0 = d @ Mi.T
        ab = np.abs(d) @ np.abs(Mi).T
        a0, a1, a2 = ab[..., 0], ab[..., 1], ab[..., 2]
        A = kk[0] * kk[1] + kk[2]
        B = s0[..., 2] + s0[..., 0] * kk[1] + s0[..., 1] * kk[0]
        Cc = s0[..., 0] * s0[..., 1]
        U, V, w = project_ref(x, h_view)
        T = U * V / w
        Ta = (a0 * a1 + np.abs(T) * (a2 + a0 * K[1] + a1 * K[0]) + T * T * (K[0] * K[1] + K[2])) / np.abs(B)
        bx = 20 * EPS * W * ((a0 + K[0] * Ta) + np.abs(U / w) * (a2 + K[2] * Ta)) / w
        by = 20 * EPS * H * ((a1 + K[1] * Ta) + np.abs(V / w) * (a2 + K[2] * Ta)) / w
        good = np.abs(A * Cc) <= B * B / 16
    return np.where(good, bx, np.inf), np.where(good, by, np.inf)


def temporal_ref(S, hit, nrm, h_rgba, h_n, h_hit, h_nrm, h_view, samples, max_history=64.0, sigma_z=0.02,
                 normal_pow2=5):
    """Returns a dict: out (H, W, 4), n (H, W), xy (H, W, 2; NaN without a projection), live, projected
    (masks), spread (H, W): the largest channel range over S(p) and the taps that are on the image with
    Hn > 0; spread_n (H, W): the largest Hn over those taps. All float64."""
    S32 = np.asarray(S, np.float32)
    nrm32 = np.asarray(nrm, np.float32)
    hn32 = np.asarray(h_nrm, np.float32)
    sigma_z = float(np.float32(sigma_z))
    max_history = float(np.float32(max_history))
    n_cur = float(np.float32(samples))
    s = S32.astype(np.float64)
    H, W = s.shape[:2]
    x = np.asarray(hit, np.float32)[..., :3].astype(np.float64)
    t = np.asarray(hit, np.float32)[..., 3].astype(np.float64)
    n = nrm32[..., :3].astype(np.float64)
    ident = nrm32[..., 3]
    Hc = np.asarray(h_rgba, np.float32).astype(np.float64)
    Hn = np.asarray(h_n, np.float32).astype(np.float64)
    Hx = np.asarray(h_hit, np.float32)[..., :3].astype(np.float64)
    Hnr = hn32[..., :3].astype(np.float64)
    Hid = hn32[..., 3]
    live = live_mask(S32, nrm32)
    with np.errstate(all="ignore"):
        U, V, w = project_ref(x, h_view)
        fx, fy = U / w * W, V / w * H
        proj = live & (w > 0) & np.isfinite(fx) & np.isfinite(fy)
        gx = np.where(proj, fx - 0.5, 0.0)
        gy = np.where(proj, fy - 0.5, 0.0)
        # (far off the image: no tap; clamped so that the integer conversion is defined)
        gx = np.clip(gx, -4.0, W + 4.0)
        gy = np.clip(gy, -4.0, H + 4.0)
        qx0 = np.floor(gx)
        qy0 = np.floor(gy)
        tx, ty = gx - qx0, gy - qy0
        G = np.zeros((H, W))
        num = np.zeros((H, W, 3))
        msum = np.zeros((H, W))
        lo = np.where(live[..., None], s[..., :3], np.inf)
        hi = np.where(live[..., None], s[..., :3], -np.inf)
        spread_n = np.zeros((H, W))
        inv_z = 1.0 / (sigma_z * np.maximum(t, FLT_MIN))
        for j in (0, 1):
            for i in (0, 1):
                qx = (qx0 + i).astype(np.int64)
                qy = (qy0 + j).astype(np.int64)
                on = proj & (qx >= 0) & (qy >= 0) & (qx < W) & (qy < H)
                cx, cy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                has = on & (Hn[cy, cx] > 0)
                lo = np.where(has[..., None], np.minimum(lo, Hc[cy, cx, :3]), lo)
                hi = np.where(has[..., None], np.maximum(hi, Hc[cy, cx, :3]), hi)
                spread_n = np.where(has, np.maximum(spread_n, Hn[cy, cx]), spread_n)
                ok = has & (Hid[cy, cx] == ident)
                b = (tx if i else 1.0 - tx) * (ty if j else 1.0 - ty)
                a = np.maximum(0.0, (n * Hnr[cy, cx]).sum(-1)) ** (2 ** int(normal_pow2))
                z = np.exp(-np.abs((n * (Hx[cy, cx] - x)).sum(-1)) * inv_z)
                g = np.where(ok, b * a * z, 0.0)
                G += g
                num += np.where(ok[..., None], g[..., None] * Hc[cy, cx, :3], 0.0)
                msum += np.where(ok, g * Hn[cy, cx], 0.0)
        h = num / G[..., None]
        m = np.minimum(max_history, msum)
        use = proj & (G > 0) & (m > 0) & np.isfinite(h).all(-1)
        out = s.copy()
        blend = (m[..., None] * h + n_cur * s[..., :3]) / (m + n_cur)[..., None]
        out[..., :3] = np.where(use[..., None], blend, s[..., :3])
        n_out = np.where(use, np.minimum(m + n_cur, max_history), np.where(live, min(n_cur, max_history), 0.0))
        xy = np.stack([np.where(proj, fx, np.nan), np.where(proj, fy, np.nan)], axis=-1)
        spread = np.where(live, (hi - lo).max(-1), 0.0)
    return {"out": out, "n": n_out, "xy": xy, "live": live, "projected": proj, "used": use, "spread": spread,
            "spread_n": spread_n}


# ---- synthetic two-view cases ------------------------------------------------------------------------
NORMAL2 = np.array([0.3, 0.0, -1.0]) / np.sqrt(1.09)


def surface_guides(view, W, H, dirs=None):
    """HIT and NORMAL (H, W, 4) float32 of a static surface seen through `view`: the plane z = 5 with
    id 1 where x < 0, the plane z = 5 + 0.3 x with id 4 where x >= 0 (they meet at x = 0)."""
    eye = view_basis(view)[0]
    d = guide_dirs(view, W, H) if dirs is None else np.asarray(dirs, np.float64)
    d = d / np.sqrt((d * d).sum(-1, keepdims=True))
    t1 = (5.0 - eye[2]) / d[..., 2]
    x1 = eye + d * t1[..., None]
    # z - 0.3 x = 5
    t2 = (5.0 - (eye[2] - 0.3 * eye[0])) / (d[..., 2] - 0.3 * d[..., 0])
    x2 = eye + d * t2[..., None]
    first = x1[..., 0] < 0
    t = np.where(first, t1, t2)
    x = np.where(first[..., None], x1, x2)
    hit = np.concatenate([x, t[..., None]], axis=-1).astype(np.float32)
    nrm = np.zeros(hit.shape, np.float32)
    nrm[..., :3] = np.where(first[..., None], np.array([0.0, 0.0, -1.0]), NORMAL2)
    nrm[..., 3] = np.where(first, 1.0, 4.0)
    return hit, nrm


def twisted(view, factor=1.05):
    """The view with r11 scaled: its guide rays are no planar patch."""
    v = np.array(view, np.float32).reshape(15).copy()
    v[12:15] *= np.float32(factor)
    return v


def synthetic_case(W, H, view, h_view, seed=5):
    """Two views of surface_guides' scene with everything the stage has to survive, each where the image
    has room for it: two ids, sky pixels, an S.a == 0 pixel, a NaN colour, a 1e4 firefly in the history,
    Hn == 0 holes, current hits that lie behind the history view (lambda <= 0) and hits that project off
    the history image on each of its four sides. Returns a dict of the hook's inputs and `planted`, the
    list of (what, y, x)."""
    rng = np.random.default_rng(seed)
    hit, nrm = surface_guides(view, W, H)
    h_hit, h_nrm = surface_guides(h_view, W, H)
    S = np.ones((H, W, 4), np.float32)
    S[..., :3] = np.where(nrm[..., 3:4] == 1.0, 0.25, 0.7) + rng.uniform(-0.2, 0.2, (H, W, 3))
    Hc = np.ones((H, W, 4), np.float32)
    Hc[..., :3] = np.where(h_nrm[..., 3:4] == 1.0, 0.3, 0.65) + rng.uniform(-0.2, 0.2, (H, W, 3))
    Hn = rng.uniform(1.0, 40.0, (H, W)).astype(np.float32)
    Hn[rng.uniform(size=(H, W)) < 0.08] = 0.0              # scattered holes
    if W >= 12 and H >= 12:
        Hn[H // 2:H // 2 + 5, W // 3:W // 3 + 6] = 0.0      # a block of them
    else:
        Hn[0, 0] = 7.0                                      # (a 1 x 1 image keeps its one history pixel)
    planted = []

    def put(img, y, x, value, what):
        if 0 <= y < H and 0 <= x < W:
            img[y, x] = value
            planted.append((what, y, x))
            return True
        return False
    put(Hc, 3, 2, (1e4, 2e3, 5e3, 1.0), "firefly")
    put(Hc, 9, 20, (1e4, 1e4, 1e4, 1.0), "firefly")
    put(nrm, 1, 4, (0, 0, 0, -1), "sky")
    put(nrm, 20, 30, (0, 0, 0, -1), "sky")
    put(h_nrm, 6, 6, (0, 0, 0, -1), "history sky")
    put(S, 5, 6, (0.9, 0.9, 0.9, 0.0), "alpha 0")
    put(S, 7, 8, (0.4, np.nan, 0.4, 1.0), "nan")
    put(S, 8, 3, (np.inf, 0.4, 0.4, 1.0), "inf")
    # current hits planted relative to the history view: behind it, and off each side of its image
    eye, r00, a, b, c = view_basis(h_view)
    fwd = r00 + 0.5 * a + 0.5 * b + 0.25 * c
    cur_eye = view_basis(view)[0]
    spots = [("behind", 10, 10, eye - 3.0 * fwd, None), ("behind", 2, W - 2, eye - 0.5 * fwd, None)]
    for what, y, x, (u, v) in (("off left", 12, 5, (-0.2, 0.5)), ("off right", 13, 7, (1.3, 0.4)),
                               ("off top", 14, 9, (0.5, -0.1)), ("off bottom", 15, 11, (0.6, 1.25)),
                               ("edge left", 16, 13, (0.2 / W, 0.5)), ("edge bottom", 17, 15, (0.5, 1.0 - 0.3 / H)),
                               ("corner", 18, 17, (1.0 - 0.4 / W, 1.0 - 0.4 / H)), ("corner", 19, 19, (0.1 / W, 0.2 / H))):
        # the surface point the history ray (u, v) sees, with its normal and id
        ph, pn = surface_guides(h_view, 1, 1, dirs=(r00 + u * a + v * b + (u * v) * c)[None, None])
        spots.append((what, y, x, ph[0, 0, :3].astype(np.float64), pn[0, 0]))
    for what, y, x, p, pn in spots:
        if 0 <= y < H and 0 <= x < W and nrm[y, x, 3] >= 0:
            hit[y, x, :3] = p.astype(np.float32)
            if pn is not None:
                hit[y, x, 3] = np.float32(np.sqrt(((p - cur_eye) ** 2).sum()))
                nrm[y, x] = pn
            planted.append((what, y, x))
    return {"S": S, "hit": hit, "nrm": nrm, "view": np.asarray(view, np.float32), "h_rgba": Hc, "h_n": Hn,
            "h_hit": h_hit, "h_nrm": h_nrm, "h_view": np.asarray(h_view, np.float32), "planted": planted}
