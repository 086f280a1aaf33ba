"""The deterministic float32 math both the oracle and the kernels implement (oracle/detmath.h,
csrc/rmr_math.h): accuracy against float64 numpy."""
import numpy as np
import pytest

from oracle import oracle


def _ulp(x):
    return np.spacing(np.abs(np.float32(x))).astype(np.float64)


@pytest.mark.parametrize("fn,ref,lo,hi,tol", [
    ("sin", np.sin, -10.0, 10.0, 2e-7), ("cos", np.cos, -10.0, 10.0, 2e-7),
    ("sin", np.sin, 0.0, 3.15, 1.5e-7), ("acos", np.arccos, -1.0, 1.0, 4e-7),
    ("log", np.log, 1e-6, 1e6, 4e-7), ("exp", np.exp, -20.0, 20.0, 1e-6),
])
def test_det_functions_accuracy(fn, ref, lo, hi, tol):
    xs = np.linspace(lo, hi, 4001).astype(np.float32)
    got = np.array([oracle.det(fn, float(x)) for x in xs], np.float64)
    want = ref(xs.astype(np.float64))
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    assert err.max() < tol


def test_det_atan2_quadrants():
    for y, x in [(1, 1), (1, -1), (-1, -1), (-1, 1), (0, -1), (2, 0.1), (-0.1, -3)]:
        assert abs(oracle.det("atan2", y, x) - np.arctan2(y, x)) < 2e-5


def _atan2(pairs):
    """(det_atan2, float64 arctan2) at float32 (y, x) pairs."""
    p = np.asarray(pairs, np.float32).reshape(-1, 2)
    got = np.array([oracle.det("atan2", float(y), float(x)) for y, x in p], np.float64)
    return got, np.arctan2(p[:, 0].astype(np.float64), p[:, 1].astype(np.float64))


def test_det_atan2_against_float64():
    """det_atan2 decides the texel column of skyColor's env-map lookup (tests/env_ref.py counts on the 2e-5 held
    here): a dense seeded set over all quadrants, ratios of 1e-6 and 1e6 either way round, and denormals."""
    rng = np.random.default_rng(41)
    n = 20000
    mag = 10.0 ** rng.uniform(-3, 3, (n, 2))
    dense = mag * rng.choice([-1.0, 1.0], (n, 2))
    ang = rng.uniform(-np.pi, np.pi, 4000)
    unit = np.stack([np.sin(ang), np.cos(ang)], axis=1)
    signs = [(a, b) for a in (-1.0, 1.0) for b in (-1.0, 1.0)]
    ratios = [(a * y, b * x) for a, b in signs for y, x in ((1e-6, 1.0), (1.0, 1e-6), (3e-3, 3e3), (7e3, 7e-3), (1e-30, 1.0), (1.0, 1e-30))]
    den = [(a * y, b * x) for a, b in signs for y, x in ((1e-40, 1.0), (1.0, 1e-40), (1e-40, 1e-40), (3e-42, 1e-41), (1e-45, 1e-39))]
    for name, pairs in (("dense", dense), ("unit", unit), ("ratios", ratios), ("denormals", den)):
        got, want = _atan2(pairs)
        err = np.abs(got - want)
        print("%s: %d points, largest error %.3g" % (name, len(got), err.max()))
        assert err.max() < 2e-5, (name, np.asarray(pairs)[np.argmax(err)])
        assert (np.sign(got) == np.sign(want))[want != 0].all(), name      # the lookup branches on phi < 0


def test_det_atan2_signed_zeros():
    """A zero on either argument: arctan2 modulo 2 pi (the lookup adds 2 pi to a negative phi, so -pi and pi are
    the same column; det_atan2 does not tell -0 from +0 in x). (0, 0) -> 0 is the project's definition: GLSL
    leaves atan(0, 0) undefined, and skyColor's column at the poles d = (0, +-1, 0) follows from this line."""
    for y in (0.0, -0.0):
        for x in (0.0, -0.0):
            assert oracle.det("atan2", y, x) == 0.0
    pairs = [(y, x) for y in (0.0, -0.0) for x in (1.0, -1.0, 1e-40, -1e-40, 3e30, -3e30)]
    pairs += [(y, x) for x in (0.0, -0.0) for y in (1.0, -1.0, 1e-40, -1e-40, 3e30, -3e30)]
    got, want = _atan2(pairs)
    off = np.abs(got - want)
    off = np.minimum(off, np.abs(off - 2 * np.pi))
    assert off.max() < 2e-5, np.asarray(pairs)[np.argmax(off)]
    # y = +-0 with x > 0 is +0 or -0, never below zero: the lookup then takes column 0's side of the seam
    assert all(oracle.det("atan2", y, 1.0) == 0.0 for y in (0.0, -0.0))


def test_det_acos_edges():
    assert oracle.det("acos", 1.0) == 0.0
    assert oracle.det("acos", -1.0) == np.float32(np.pi)
    assert np.isnan(oracle.det("acos", 1.5))
