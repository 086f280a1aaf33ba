"""Pin the CPU oracle to the reference GLSL itself (RayMarch*.glsl run on Mesa llvmpipe by
oracle/glsl_ref/, fixtures committed in tests/golden/ with MANIFEST.json).

Deterministic reference functions must agree within float tolerance; the RNG stream of the
reference (chained fract(sin(x)*43758.5453), RayMarch.glsl:43-57) is driver-defined, so whole
images are compared statistically at equal seed schedules.
"""
import os

import numpy as np
import pytest

from oracle import oracle, scene_compile
from raymarchrenderer_amd import abi, parity_schedule, time_schedule

from .conftest import GOLDEN, SCENES

KATS = {"rm3": (None, "rm3"), "cornell5": (os.path.join(SCENES, "cornell5.scene"), "rm1"),
        "default": (os.path.join(GOLDEN, "scenes", "default.scene"), "rm1"),
        # RM1's object node set: op_union / op_subtract / op_intersect / domain_repeat / math / misc
        "csg_nodes": (os.path.join(SCENES, "csg_nodes.scene"), "rm1"),
        # C3's Mandelbulb node added to the reference path (oracle/glsl_ref/shader_build.py X1)
        "mandelbulb": (os.path.join(SCENES, "mandelbulb.scene"), "rm1"),
        # C4's generator cut to 64 primitives (the BVH / nearest-primitive-cache scene size class)
        "csg64": (os.path.join(SCENES, "csg64.scene"), "rm1"),
        # math_sine / math_cosine / misc_getX / misc_getZ, real divisors, products of two and three variables
        # (the trig case of tests/node_family.py)
        "trig_nodes": (os.path.join(SCENES, "trig_nodes.scene"), "rm1")}


def _tables(path, variant):
    return scene_compile.compile_scene({}, variant) if path is None else scene_compile.load_scene_file(path, variant)


# The Mandelbulb's distance estimator iterates pow / acos / atan / sin / cos / log of the driver
# (llvmpipe) against the oracle's deterministic ones (oracle/detmath.h): GLSL leaves their precision
# to the implementation, and the fractal iteration amplifies ulp-level differences (measured: map
# within 3e-5 relative, march within 1e-4, normals — central differences with h = 0.001 of that
# distance — median 1e-6, worst 0.04 of 104). Its tolerances say so; every other scene is held to
# float rounding.
MAP_RTOL = {"mandelbulb": 1e-4}


@pytest.mark.parametrize("name", sorted(KATS))
def test_kat_map(name):
    k = np.load(os.path.join(GOLDEN, "kat_%s.npz" % name))
    t = _tables(*KATS[name])
    out = np.array([oracle.map_p(t, p) for p in k["map_in"]])
    ref = k["map_out"]
    assert np.all(np.abs(out[:, 0] - ref[:, 0]) <= MAP_RTOL.get(name, 2e-6) * np.maximum(1.0, np.abs(ref[:, 0])))
    assert np.array_equal(out[:, 1], ref[:, 1])


@pytest.mark.parametrize("name", sorted(KATS))
def test_kat_march(name):
    k = np.load(os.path.join(GOLDEN, "kat_%s.npz" % name))
    t = _tables(*KATS[name])
    out = np.array([oracle.march(t, r[:3], r[3:]) for r in k["march_in"]])
    ref = k["march_out"]
    assert np.array_equal(out[:, 0] >= 1000, ref[:, 0] >= 1000)
    assert np.array_equal(out[:, 1], ref[:, 1])
    assert np.all(np.abs(out[:, 0] - ref[:, 0]) <= 1e-3)


@pytest.mark.parametrize("name", sorted(KATS))
def test_kat_normal(name):
    k = np.load(os.path.join(GOLDEN, "kat_%s.npz" % name))
    t = _tables(*KATS[name])
    hit = k["march_out"][:, 0] < 1000
    out = np.array([oracle.normal(t, p) for p in k["normal_in"][hit]])
    err = np.abs(out - k["normal_out"][hit]).max(axis=1)
    if name == "mandelbulb":   # see MAP_RTOL
        assert np.median(err) <= 1e-4 and np.percentile(err, 90) <= 5e-3 and err.max() <= 0.1
    else:
        assert err.max() <= 1e-4


@pytest.mark.parametrize("name", ["cornell5", "default"])
def test_kat_nan_direction_semantics(name):
    """A NaN ray direction (normalize(vec3(0)) after total internal reflection) on the reference:
    map(NaN) and march(o, NaN, +-1) as llvmpipe evaluates them (opU per component, see o_map)."""
    k = np.load(os.path.join(GOLDEN, "kat_nan.npz"))
    t = _tables(*KATS[name])
    nan3 = np.full(3, np.nan, np.float32)
    ref = k["%s_out" % name]
    for o, r in zip(k["%s_origin" % name], ref):
        m = oracle.map_p(t, nan3)
        a = oracle.march(t, o, nan3, 1.0)
        b = oracle.march(t, o, nan3, -1.0)
        np.testing.assert_array_equal(np.concatenate([m, a, b]), r)


def test_kat_nan_and_infinite_objects_exact():
    """opU with one object NaN or +-inf beside finite ones, on the reference as llvmpipe runs it: map of the
    nan_objects case of tests/node_family.py at its hand-computed points (edge_in / edge_out of the trig_nodes
    fixture, through the ordinary map probe). The oracle returns the same distance and id, float for
    float: a NaN object never becomes the distance but takes the id, -inf is the distance, +inf never wins."""
    from . import node_family
    k = np.load(os.path.join(GOLDEN, "kat_trig_nodes.npz"))
    assert np.array_equal(k["edge_in"].view(np.uint32), node_family.nan_rule_points().view(np.uint32))
    t = node_family.tables("nan_objects")
    out = np.array([oracle.map_p(t, p) for p in k["edge_in"]])
    ref = k["edge_out"]
    assert not np.isnan(ref).any() and np.isneginf(ref[:, 0]).sum() == 2
    np.testing.assert_array_equal(out, ref)


def test_kat_wavelength_to_color_exact():
    k = np.load(os.path.join(GOLDEN, "kat_rm3.npz"))
    out = np.array([oracle.wl2rgb(int(w)) for w in k["wl_in"]])
    np.testing.assert_array_equal(out, k["wl_out"])


@pytest.mark.parametrize("name", sorted(KATS))
def test_kat_rand_and_hemisphere_distributions(name):
    """The reference hash stream is driver-defined: compare its distribution, not values."""
    k = np.load(os.path.join(GOLDEN, "kat_%s.npz" % name))
    ref = k["rand_out"]
    n = len(ref)
    w = int(k["probe_width"])
    ours = np.array([oracle.rand_chain(i % w, i // w, float(k["rand_time"]), k["rand_in"][i]) for i in range(n)])
    for x in (ref, ours):
        assert x.min() >= 0.0 and x.max() < 1.0
        assert abs(x.mean() - 0.5) < 0.03 and abs(x.var() - 1.0 / 12) < 0.01
    h = k["hemi_out"]
    nrm = k["hemi_in"][:, 4:7]
    assert np.abs(np.linalg.norm(h, axis=1) - 1).max() < 1e-5
    assert (np.sum(h * nrm, axis=1) >= -1e-6).all()
    ours_h = np.array([oracle.hemisphere(i % w, i // w, float(k["rand_time"]), r[8], r[0:2], r[2:4], r[4:7])
                       for i, r in enumerate(k["hemi_in"])])
    assert np.abs(np.linalg.norm(ours_h, axis=1) - 1).max() < 1e-5
    assert (np.sum(ours_h * nrm, axis=1) >= -1e-6).all()


def _ks_uniform(x):
    """One-sample Kolmogorov-Smirnov statistic of x against U[0, 1]."""
    x = np.sort(np.asarray(x, np.float64))
    n = len(x)
    i = np.arange(1, n + 1)
    return max(np.max(i / n - x), np.max(x - (i - 1) / n))


def _hemi_polar(h, n):
    """cos(theta) about the normal and the azimuth / 2pi in a tangent frame fixed by the normal.
    A uniform hemisphere (RM1:270-304) makes both U[0, 1]; a cosine-weighted one makes cos(theta)
    ~ sqrt(U) (KS distance 0.25)."""
    h = np.asarray(h, np.float64)
    n = np.asarray(n, np.float64)
    n = n / np.linalg.norm(n, axis=1, keepdims=True)
    a = np.where(np.abs(n[:, 1:2]) > 0.9, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])
    t = np.cross(n, a)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    b = np.cross(n, t)
    ct = np.sum(h * n, axis=1)
    phi = np.arctan2(np.sum(h * b, axis=1), np.sum(h * t, axis=1))
    return np.clip(ct, 0.0, 1.0), (phi / (2.0 * np.pi)) % 1.0


def _hemi_kats():
    ins, outs = [], []
    for name in sorted(KATS):
        k = np.load(os.path.join(GOLDEN, "kat_%s.npz" % name))
        ins.append((k["hemi_in"], float(k["rand_time"]), int(k["probe_width"])))
        outs.append(k["hemi_out"])
    return ins, outs


def test_hemisphere_distribution_ks_vs_reference():
    """randHemisphere (RM1:270-304) as a distribution: the reference's own samples (llvmpipe,
    3072 pooled over the KAT scenes) and the oracle's on the same inputs are each uniform on the
    hemisphere by KS (cos(theta) and the azimuth; critical distance at alpha = 0.001 is 1.95/sqrt(n)),
    and the two samples agree by a two-sample KS. A cosine-weighted or a tilted sampler fails."""
    ins, outs = _hemi_kats()
    ref_h = np.concatenate(outs)
    nrm = np.concatenate([i[0][:, 4:7] for i in ins])
    ours = np.concatenate([
        np.array([oracle.hemisphere(j % w, j // w, t, r[8], r[0:2], r[2:4], r[4:7]) for j, r in enumerate(hin)])
        for hin, t, w in ins])
    n = len(ref_h)
    crit = 1.95 / np.sqrt(n)
    polar = {}
    for label, h in (("reference", ref_h), ("oracle", ours)):
        ct, ph = _hemi_polar(h, nrm)
        polar[label] = (ct, ph)
        assert _ks_uniform(ct) < crit, (label, "cos theta", _ks_uniform(ct))
        assert _ks_uniform(ph) < crit, (label, "azimuth", _ks_uniform(ph))
        # a cosine-weighted sampler (cos theta = sqrt(u)) would be far outside
        assert _ks_uniform(np.sqrt(np.linspace(0, 1, n))) > 4 * crit
    # two-sample KS between reference and oracle: critical 1.95 sqrt(2/n)
    for j in range(2):
        a, b = np.sort(polar["reference"][j]), np.sort(polar["oracle"][j])
        grid = np.concatenate([a, b])
        d = np.max(np.abs(np.searchsorted(a, grid, "right") / n - np.searchsorted(b, grid, "right") / n))
        assert d < 1.95 * np.sqrt(2.0 / n), (j, d)


def test_hemisphere_algebraic_form_vs_literal_within_ulps():
    """The default oracle (and kernel) takes cos(acos(u)) = u and sin(acos(u)) = sqrt(1 - u^2)
    algebraically; the literal build (RMR_HEMI_ALGEBRAIC=0) evaluates RM1:270-304's acos / sin / cos.
    On every KAT input the two directions agree within a few float ulps of a unit vector.

    One exception, and it is the reference's own driver-defined edge: when rand() returns exactly 0,
    u = -1 and the direction lies in the tangent plane; sin(acos(-1)) is sin(float(pi)) = -8.7e-8 in
    the literal form (the driver's sign, GLSL does not fix it) and +0 algebraically, so RM1:287's
    `if (b.z < 0) b = -b` flips one and not the other. Both are the same grazing direction up to the
    flip (4 of the 3072 KAT inputs)."""
    lit = oracle.literal_lib()
    ins, _ = _hemi_kats()
    worst, flips = 0.0, 0
    for hin, t, w in ins:
        for j, r in enumerate(hin):
            a = oracle.hemisphere(j % w, j // w, t, r[8], r[0:2], r[2:4], r[4:7])
            b = oracle.hemisphere(j % w, j // w, t, r[8], r[0:2], r[2:4], r[4:7], L=lit)
            d = float(np.abs(a - b).max())
            if d > 8 * 2.0 ** -23 and abs(float(np.dot(a, r[4:7]))) < 1e-6 and np.abs(a + b).max() <= 8 * 2.0 ** -23:
                flips += 1
                continue
            worst = max(worst, d)
    assert worst <= 8 * 2.0 ** -23, worst   # <= 8 ulps of 1.0 per component
    assert flips <= 8, flips


def test_mandelbulb_poly_vs_literal_within_map_rtol():
    """The power-8 Mandelbulb as complex powers (mb_iter8_poly, default) against the angle-doubling
    form (RMR_MB_POLY=0), both transcendental-free restatements of the trigonometric iteration:
    the distance estimates on the KAT points agree within MAP_RTOL, the tolerance the oracle is held
    to against the reference GLSL's own trigonometric iteration on llvmpipe."""
    lit = oracle.literal_lib()
    k = np.load(os.path.join(GOLDEN, "kat_mandelbulb.npz"))
    t = _tables(*KATS["mandelbulb"])
    a = np.array([oracle.map_p(t, p) for p in k["map_in"]])
    b = np.array([oracle.map_p(t, p, L=lit) for p in k["map_in"]])
    assert np.all(np.abs(a[:, 0] - b[:, 0]) <= MAP_RTOL["mandelbulb"] * np.maximum(1.0, np.abs(b[:, 0])))
    assert np.array_equal(a[:, 1], b[:, 1])
    # and the literal build is itself within the same tolerance of the reference
    ref = k["map_out"]
    assert np.all(np.abs(b[:, 0] - ref[:, 0]) <= MAP_RTOL["mandelbulb"] * np.maximum(1.0, np.abs(ref[:, 0])))


IMAGES = {
    "rm3_builtin": (None, "rm3", {}),
    "rm1_cornell5_b4": (os.path.join(SCENES, "cornell5.scene"), "rm1", {"max_bounces": 4}),
    "rm1_sphere1_b1": (os.path.join(SCENES, "sphere1.scene"), "rm1", {"max_bounces": 1}),
    "rm2_simple": (os.path.join(GOLDEN, "scenes", "simple.scene"), "rm2", {}),
    "rm1_glass": (os.path.join(GOLDEN, "scenes", "glass_test.scene"), "rm1", {}),
    "rm1_multilight": (os.path.join(GOLDEN, "scenes", "multilight.scene"), "rm1", {}),
    "rm1_default": (os.path.join(GOLDEN, "scenes", "default.scene"), "rm1", {}),
    "rm1_sphere1_env": (os.path.join(SCENES, "sphere1.scene"), "rm1", {"max_bounces": 4, "use_env_tex": 1}),
    "rm2_simple_env": (os.path.join(GOLDEN, "scenes", "simple.scene"), "rm2", {"use_env_tex": 1}),
    # round-2 goldens: C4's generator cut to 64 primitives, RM1's object node set, C3's Mandelbulb
    "rm1_csg64_b4": (os.path.join(SCENES, "csg64.scene"), "rm1", {"max_bounces": 4}),
    "rm1_csg_nodes_b4": (os.path.join(SCENES, "csg_nodes.scene"), "rm1", {"max_bounces": 4}),
    "rm1_mandelbulb_b2": (os.path.join(SCENES, "mandelbulb.scene"), "rm1", {"max_bounces": 2}),
    "rm1_trig_nodes_b3": (os.path.join(SCENES, "trig_nodes.scene"), "rm1", {"max_bounces": 3}),
}


@pytest.mark.parametrize("name", sorted(IMAGES))
def test_image_statistics_vs_reference(name):
    """Oracle samples (same seed schedule, 512 spp, centre 32x24 crop) vs the llvmpipe converged
    image: per-pixel z-scores must be centred (|median z| < 0.25), rare outliers only, means within
    3%. (Consecutive `time` seeds give correlated hash streams, so small-N z-scores have fat tails;
    512 spp keeps the iid approximation usable.)"""
    g = np.load(os.path.join(GOLDEN, "img_%s.npz" % name))
    path, variant, kw = IMAGES[name]
    H, W = g["conv"].shape[:2]
    env = g["env"] if "env" in g.files else None
    o = oracle.Oracle(_tables(path, variant), abi.default_params(**kw), g["view"], W, H, env=env)
    spp = 512
    x0, y0, x1, y1 = W // 4, H // 4, W // 4 + 32, H // 4 + 24
    n_ref = int(g["spp_conv"])
    times = parity_schedule(n_ref)[:: n_ref // spp][:spp]   # same schedule, strided over its full range
    s = o.trace_samples(times, rect=(x0, y0, x1, y1))[..., :3].astype(np.float64)
    m, v = s.mean(0), s.var(0, ddof=1)
    ref = g["conv"][y0:y1, x0:x1, :3].astype(np.float64)
    # 4x4-pixel blocks: 16 independent pixel streams x 512 samples per block mean (CLT regime)
    def blocks(a):
        h, w, c = a.shape
        return a.reshape(h // 4, 4, w // 4, 4, c).mean(axis=(1, 3))
    mb, rb = blocks(m), blocks(ref)
    se = np.sqrt(blocks(v) / 16.0 * (1.0 / spp + 1.0 / int(g["spp_conv"])))
    # plus a 0.1 % systematic allowance: the driver's texture-filter precision (envTex) and sin() are
    # implementation-defined (llvmpipe filters with 8-bit weights), visible where samples barely vary
    se = np.sqrt(se ** 2 + (1e-3 * np.abs(blocks(ref))) ** 2)
    ok = se > 0
    z = (mb - rb)[ok] / se[ok]
    # blocks whose samples never vary (sky, shadow) may still see rare events in the 16k-64k
    # reference samples: small absolute tolerance there
    assert np.abs((mb - rb)[~ok]).max(initial=0) < 0.01
    # statistically consistent, or (for near-deterministic scenes such as RM2 simple, whose sample
    # values are a handful of discrete levels) absolutely negligible differences
    tiny = np.abs(mb - rb).max() < 2e-3
    assert tiny or abs(np.mean(np.clip(z, -8, 8))) < 0.5
    assert tiny or (np.abs(z) > 6).mean() < 0.05
    assert abs(m.mean() - ref.mean()) <= 0.03 * ref.mean() + 1e-6
    # the 4-spp reference render has the same noise level as the oracle at 4 spp
    lo = g["lo"][y0:y1, x0:x1, :3]
    a4 = o.render(time_schedule(4))[y0:y1, x0:x1, :3]
    e_ref = np.mean((np.clip(lo, 0, 1) - np.clip(ref, 0, 1)) ** 2)
    e_our = np.mean((np.clip(a4, 0, 1) - np.clip(ref, 0, 1)) ** 2)
    assert 0.5 < (e_our + 1e-12) / (e_ref + 1e-12) < 2.0
