"""A float64 statement of the v1 object programs and of map, with a counted error bound for a float32
evaluation of the same nodes. Written from the node functions' semantics (RayMarch.glsl:121-135 misc_get*,
137-166 math_*, 169-179 map_sphere / map_box, 182-195 op_*, 198-214 domain_repeat, 218-231 opU / map), on
the scene dictionary itself: it uses neither the oracle nor the scene compilers.

  op_subtract(a, b) = max(a, -b); mod(x, y) = x - y floor(x / y); domain_repeat skips an axis whose period
  is 0; opU keeps the earlier object on a.x < b.x, so a tie goes to the later one; map starts at
  (maxDist, -1).

Beside every value stands an absolute bound on |float32 evaluation - float64 value|:
  one float32 rounding, U = 2^-24 relative (plus 2^-149 for a denormal result), for each arithmetic result;
  the operands' bounds through the operation's local derivative (sum: e_a + e_b; product: |a| e_b + |b| e_a
  + e_a e_b; quotient: (e_a + |a / b| e_b) / (|b| - e_b); sine / cosine: e_a; min / max: the larger; a
  length: the sum of its components' bounds, and 3 U of the length for the fused dot product (three
  roundings of a sum of squares, halved by the root) and the root;
  for math_sine / math_cosine the term T: the error of the float32 implementation against float64 at
  float32 arguments, which the caller measures (trig_args gives the arguments) and passes in.
A float32 result that is the fused mod (x - y k in one rounding) counts one rounding.

Where such a bound means nothing the point has none (valid is False), decided from the float64 values
alone: x / m within 1e-4 of an integer in domain_repeat (or within four times the quotient's own bound),
a divisor below 1e-3 in magnitude, a sine or cosine argument above 1e6, a non-finite intermediate or one
that float32 cannot hold.

Not a test and not a conftest: a helper module like camera_ref.py."""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149
F32_MAX = 3.0e38
REPEAT_MARGIN, MIN_DIVISOR, MAX_TRIG_ARG = 1e-4, 1e-3, 1e6


def lit(x):
    """A scene literal as the shader reads it: the float32 nearest the (at most six-decimal) number."""
    return float(np.float32(x))


class _Eval:
    def __init__(self, pts, T, trig_args=None):
        self.p = np.asarray(pts, np.float32).astype(np.float64)
        self.n = len(self.p)
        self.T = T
        self.valid = np.ones(self.n, bool)
        self.trig_args = trig_args

    def _round(self, r, e):
        """The bound after one float32 rounding of a result r whose exact-input error is e."""
        bad = ~np.isfinite(r) | (np.abs(r) + e >= F32_MAX)
        self.valid &= ~bad.any(axis=1)
        return r, e + U * (np.abs(r) + e) + TINY

    def operand(self, a, vars_):
        if isinstance(a, (list, tuple)):
            v = np.array([lit(x) for x in (list(a) + [0, 0, 0])[:3]], np.float64)
            return np.tile(v, (self.n, 1)), np.zeros((self.n, 3))
        if a == -1:
            return self.p, np.zeros((self.n, 3))
        return vars_[a]

    def length(self, q, eq):
        ln = np.sqrt((q * q).sum(axis=1))
        return ln, eq.sum(axis=1) + 3 * U * (ln + eq.sum(axis=1)) + TINY

    def node(self, name, ins):
        with np.errstate(all="ignore"):
            return self._node(name, ins)

    def _node(self, name, ins):
        (a, ea) = ins[0]
        if name.startswith("misc_get"):
            k = "XYZ".index(name[-1])
            return np.repeat(a[:, k:k + 1], 3, axis=1), np.repeat(ea[:, k:k + 1], 3, axis=1)
        if name in ("math_sine", "math_cosine"):
            self.valid &= ~(np.abs(a) + ea > MAX_TRIG_ARG).any(axis=1)
            self.valid &= np.isfinite(a).all(axis=1)
            if self.trig_args is not None:
                self.trig_args.append(a[self.valid].ravel().copy())
            r = np.sin(a) if name == "math_sine" else np.cos(a)
            return r, ea + self.T
        (b, eb) = ins[1]
        if name == "math_add":
            return self._round(a + b, ea + eb)
        if name == "math_subtract":
            return self._round(a - b, ea + eb)
        if name == "math_multiply":
            return self._round(a * b, np.abs(a) * eb + np.abs(b) * ea + ea * eb)
        if name == "math_divide":
            self.valid &= ~(np.abs(b) - eb < MIN_DIVISOR).any(axis=1)
            den = np.maximum(np.abs(b) - eb, MIN_DIVISOR)
            r = a / b
            return self._round(r, (ea + np.abs(r) * eb) / den)
        if name == "op_union":
            return np.minimum(a, b), np.maximum(ea, eb)
        if name == "op_intersect":
            return np.maximum(a, b), np.maximum(ea, eb)
        if name == "op_subtract":
            return np.maximum(a, -b), np.maximum(ea, eb)
        if name == "domain_repeat":
            r, e = a.copy(), ea.copy()
            for k in range(3):
                mk, emk = b[:, k], eb[:, k]   # a period may be a variable: per point
                on = mk != 0.0
                if not on.any():
                    continue
                msafe = np.where(on, mk, 1.0)
                q = a[:, k] / msafe
                eq = (ea[:, k] + np.abs(q) * emk) / np.maximum(np.abs(msafe) - emk, TINY) + U * np.abs(q)
                fl = np.floor(q)
                near = np.minimum(q - fl, fl + 1.0 - q) <= np.maximum(REPEAT_MARGIN, 4.0 * eq)
                self.valid &= ~(on & (near | ~np.isfinite(q)))
                mod = a[:, k] - msafe * fl
                emod = ea[:, k] + np.abs(fl) * emk
                emod = emod + U * (np.abs(mod) + emod) + TINY
                out = mod - 0.5 * msafe
                eout = emod + 0.5 * emk
                eout = eout + U * (np.abs(out) + eout) + TINY
                r[:, k] = np.where(on, out, a[:, k])
                e[:, k] = np.where(on, eout, ea[:, k])
            self.valid &= np.isfinite(r).all(axis=1)
            return r, e
        (c, ec) = ins[2]
        if name == "map_sphere":
            q, eq = self._round(a - b, ea + eb)
            ln, eln = self.length(q, eq)
            d, ed = self._round((ln - c[:, 0])[:, None], (eln + ec[:, 0])[:, None])
            return np.repeat(d, 3, axis=1), np.repeat(ed, 3, axis=1)
        if name == "map_box":
            q, eq = self._round(a - b, ea + eb)
            q, eq = self._round(np.abs(q) - c, eq + ec)
            inner, einner = np.minimum(q.max(axis=1), 0.0), eq.max(axis=1)
            ln, eln = self.length(np.maximum(q, 0.0), eq)
            d, ed = self._round((inner + ln)[:, None], (einner + eln)[:, None])
            return np.repeat(d, 3, axis=1), np.repeat(ed, 3, axis=1)
        raise KeyError(name)

    def obj(self, o):
        """(distance, bound) of one object at every point."""
        zero = (np.zeros((self.n, 3)), np.zeros((self.n, 3)))
        vars_ = [zero] * int(o["total_vars"])
        for nd in o["nodes"]:
            ins = [self.operand(a, vars_) for a in nd["inputs"]]
            vars_[nd["outputs"][0]] = self.node(nd["name"], ins)
        d, e = vars_[o["distance"]]
        self.valid &= np.isfinite(d[:, 0]) & np.isfinite(e[:, 0])
        return d[:, 0], e[:, 0]


def trig_args(scene, pts):
    """The float64 arguments that the scene's math_sine / math_cosine nodes receive at the points (those
    with a bound), for the caller to measure T at."""
    args = []
    ev = _Eval(pts, 0.0, args)
    for o in scene["objects"]:
        ev.obj(o)
    return np.concatenate(args) if args else np.zeros(0)


def objects64(scene, pts, T):
    """Every object's float64 distance and bound at the points: (dist (n_obj, n), bound (n_obj, n), valid (n,))."""
    ev = _Eval(pts, T)
    out = [ev.obj(o) for o in scene["objects"]]
    return np.array([d for d, _ in out]), np.array([e for _, e in out]), ev.valid.copy()


def map64(scene, pts, T, max_dist=1000.0):
    """map at the points: (distance, its bound, id, id_sure, valid). id_sure: the two smallest distances
    differ by more than the sum of their bounds, so a float32 evaluation must name the same object."""
    dist, bound, valid = objects64(scene, pts, T)
    n = dist.shape[1]
    ids = np.array([float(o.get("matID", 0)) for o in scene["objects"]])
    dist = np.concatenate([np.full((1, n), float(max_dist)), dist])
    bound = np.concatenate([np.zeros((1, n)), bound])
    ids = np.concatenate([[-1.0], ids])
    with np.errstate(invalid="ignore"):
        d = np.where(np.isfinite(dist), dist, np.inf)
        # opU: a later object replaces the running minimum unless the minimum is strictly smaller
        best = np.zeros(n, int)
        for j in range(1, len(d)):
            take = ~(d[best, np.arange(n)] < d[j])
            best = np.where(take, j, best)
        dmin = d[best, np.arange(n)]
        emin = bound[best, np.arange(n)]
        e = np.where(np.isfinite(bound), bound, np.inf)
        cand = d - e <= (dmin + emin)[None, :]
        err = np.where(cand, e, 0.0).max(axis=0)
        others = d.copy()
        others[best, np.arange(n)] = np.inf
        second = others.argmin(axis=0)
        gap = others[second, np.arange(n)] - dmin
        sure = gap > emin + e[second, np.arange(n)]
    return dmin, err, ids[best], sure, valid


# ---- march and getNormal in float64, the reference's rules (RayMarch.glsl:233-268) ----------------------
def _map_at(scene, pts64, T, max_dist):
    """map (distance, id) at float64 points: the sphere trace and the normal probes are not float32 points."""
    ev = _Eval(np.zeros((len(pts64), 3), np.float32), T)
    ev.p = np.asarray(pts64, np.float64)
    best, ident = np.full(len(pts64), float(max_dist)), np.full(len(pts64), -1.0)
    for o in scene["objects"]:
        d = ev.obj(o)[0]
        d = np.where(np.isfinite(d), d, np.inf)
        take = ~(best < d)
        best, ident = np.where(take, d, best), np.where(take, float(o.get("matID", 0)), ident)
    return best, ident


def march64(scene, o, d, T, max_dist=1000.0, max_steps=512, step_multiply=0.5):
    """One ray: t where map < 0.001 (and the id), or (max_dist, -1)."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    t = 0.0
    for _ in range(max_steps):
        m, ident = _map_at(scene, (o + d * t)[None, :], T, max_dist)
        if m[0] < 0.001:
            return t, ident[0]
        if t >= max_dist:
            return max_dist, -1.0
        t += m[0] * step_multiply
    return max_dist, -1.0


def normal64(scene, p, T, max_dist=1000.0, h=0.001):
    """Central differences of map at p +- h along each axis, normalised."""
    p = np.asarray(p, np.float64)
    q = np.array([p + h * np.eye(3)[k] * s for k in range(3) for s in (1.0, -1.0)])
    m, _ = _map_at(scene, q, T, max_dist)
    n = np.array([m[0] - m[1], m[2] - m[3], m[4] - m[5]])
    return n / np.linalg.norm(n)
