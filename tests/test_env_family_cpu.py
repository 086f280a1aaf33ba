"""skyColor's env-map lookup on the CPU (tests/env_family.py): the inputs are worth running, and the oracle's
sky_color is held to the float64 statement (tests/env_ref.py) on every map and direction, and to the reference's
own skyColor run on llvmpipe (tests/golden/kat_sky.npz).

The poles d = (0, +-1, 0) are not in the fixture: GLSL leaves atan(0, 0) undefined, llvmpipe returns something of
its own there (0.27 to 0.65 away on a noise map), and the project defines det_atan2(0, 0) = 0. At the poles the
texel column is the project's definition, held by the float64 statement alone (which defines the same).

llvmpipe filters an RGBA8 texture in 8-bit integers: its weights have 8 bits and its result lies on the lattice
n / 255. Where every texel a lookup can fetch is equal (the block map, half the directions) none of that matters
and the oracle must agree to rounding: that pins the orientation, the seam, row 0 = up and the clamp to the
reference. On the noise map the tolerance is measured, as k 2^-8 times the spread of the four texels the statement
selects: MANIFEST.json records the measured ratio 128.0019 (directions whose four texels lie within 2 / 255 of each
other in a channel while the reference's result moves by a whole 1 / 255 decide it), K is its ceiling plus one."""
import json
import math
import os

import numpy as np
import pytest

from oracle import oracle

from . import env_family as ef
from . import env_ref
from .conftest import GOLDEN

E = 2.0 ** -24
K_LLVMPIPE = 130


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "kat_sky.npz"))


# ---- the inputs are worth running -----------------------------------------------------------------------------
def test_maps_are_what_the_family_says():
    m = ef.maps()
    assert {k: v.shape[:2] for k, v in m.items()} == {
        "noise1x1": (1, 1), "noise1x7": (7, 1), "noise5x1": (1, 5), "noise2x2": (2, 2), "noise37x19": (19, 37),
        "noise64x32": (32, 64), "noise16x8": (8, 16), "checker64x32": (32, 64), "ramp4096x1": (1, 4096),
        "ramp2x1024": (1024, 2), "block64x32": (32, 64), "alpha23x11": (11, 23), "bytes16x16": (16, 16)}
    for name, env in m.items():
        assert env.dtype == np.uint8 and env.shape[2] == 4
        if name == "block64x32":
            continue
        rgb = env[..., :3].astype(np.int32)
        for axis in (0, 1):
            assert (np.abs(np.diff(rgb, axis=axis)).sum(axis=-1) > 0).all(), name   # every texel differs from its neighbours
    blk = m["block64x32"][..., :3]
    assert (blk.reshape(8, 4, 16, 4, 3) == blk[::4, ::4].reshape(8, 1, 16, 1, 3)).all()
    assert len(np.unique(m["alpha23x11"][..., 3])) > 100
    assert all(len(np.unique(m["bytes16x16"][..., k])) == 256 for k in range(3))
    assert set(np.unique(m["checker64x32"][..., :3])) == {0, 255}
    assert (ef.ramp_index(m["ramp4096x1"][0, :, :3] / 255.0) == np.arange(4096)).all()
    assert (ef.ramp_index(m["ramp2x1024"][:, 0, :3] / 255.0) == np.arange(1024)).all()


def test_directions_are_what_the_family_says():
    d, lab = ef.directions(), ef.labels()
    assert d.dtype == np.float32 and 2900 <= len(d) <= 3100
    counts = dict(zip(*np.unique(lab, return_counts=True)))
    print(counts)
    assert counts["pole"] == 2 and counts["seam"] == 36 and counts["x_zero"] == 12 and counts["near_pole"] == 32
    seam = d[lab == "seam"]
    for z in (0.0, 1e-30, 1e-40):
        for sign in (False, True):
            hit = (np.abs(seam[:, 2]) == np.float32(z)) & (np.signbit(seam[:, 2]) == sign)
            assert (seam[hit, 0] < 0).any() and (seam[hit, 0] > 0).any(), (z, sign)
    assert 0 < np.float32(1e-40) < np.finfo(np.float32).tiny          # a denormal
    xz = d[lab == "x_zero"]
    assert (xz[:, 0] == 0).all() and np.signbit(xz[:, 0]).any() and (~np.signbit(xz[:, 0])).any()
    near = d[lab == "near_pole"]
    assert (np.abs(near[:, 1]) == np.nextafter(np.float32(1), np.float32(0))).all()
    fx = ef.fixture_directions()
    assert len(fx) == len(ef.core_directions()) - 2 and not ((fx[:, 0] == 0) & (fx[:, 2] == 0)).any()


@pytest.mark.parametrize("scene", sorted(ef.DIRECT))
def test_direct_rays_miss(scene):
    """The oracle's march of every direct ray is a miss, so Oracle.trace of it is skyColor(d) exactly."""
    tb, prm = ef.direct_tables(scene), ef.direct_params(scene)
    t = np.array([oracle.march(tb, q["o"], q["d"], params=prm)[0] for q in ef.direct_rays(scene)])
    assert (t >= prm.max_dist).all(), (scene, t.min())


def test_rm2_direct_rays_give_rm1s_sky():
    for name in ("noise37x19", "checker64x32"):
        a, b = ef.oracle_sky("sphere1", name), ef.oracle_sky("simple_rm2", name)
        assert a.tobytes() == b.tobytes() and len(np.unique(a, axis=0)) > 100


@pytest.mark.parametrize("name", ef.SMALL_MAPS)
def test_every_column_and_row_and_both_clamps_are_fetched(name):
    """From the float64 statement: the directions fetch every column and row of the map, and on each axis a fetch
    clamps at the low end (floor(f) = -1) and at the high end (floor(f) + 1 = size)."""
    env = ef.maps()[name]
    h, w = env.shape[:2]
    d = ef.directions()
    i0, i1, j0, j1, _, _ = env_ref.cell(d, w, h)
    assert set(i0) | set(i1) == set(range(w)) and set(j0) | set(j1) == set(range(h))
    fu, fv = env_ref.coordinates(d, w, h)
    lo_u, hi_u, lo_v, hi_v = (np.floor(fu) == -1).sum(), (np.floor(fu) == w - 1).sum(), (np.floor(fv) == -1).sum(), (np.floor(fv) == h - 1).sum()
    print("%s: clamped fetches: u low %d, u high %d, v low %d, v high %d of %d" % (name, lo_u, hi_u, lo_v, hi_v, len(d)))
    assert min(lo_u, hi_u, lo_v, hi_v) >= 5
    if w == 1:
        assert (i0 == 0).all() and (i1 == 0).all()
    if h == 1:
        assert (j0 == 0).all() and (j1 == 0).all()


@pytest.mark.parametrize("name", ef.BORDER_MAPS)
def test_border_directions_sit_on_both_sides_of_every_border(name):
    """Counted from the float64 statement: at each chosen column border i and row border j the weight is within
    1e-5 above 0 for some direction and within 1e-5 below 1 for another; at i = w - 1 the second column is clamped."""
    env = ef.maps()[name]
    h, w = env.shape[:2]
    d = ef.directions()[ef.labels() == "border_%dx%d" % (w, h)]
    assert len(d) == 120
    fu, fv = env_ref.coordinates(d, w, h)
    for f, size, what in ((fu, w, "column"), (fv, h, "row")):
        for k in (0, size // 2, size - 1):
            off = f - k
            above, below = (off >= 0) & (off < 1e-5), (off < 0) & (off > -1e-5)
            assert above.sum() >= 5 and below.sum() >= 5, (name, what, k, above.sum(), below.sum())
            assert (np.abs(off[above]).min() < 2e-6) and (np.abs(off[below]).min() < 2e-6)
    _, i1, _, j1, _, _ = env_ref.cell(d, w, h)
    assert ((np.floor(fu) == w - 1) & (i1 == w - 1)).sum() >= 5 and ((np.floor(fv) == h - 1) & (j1 == h - 1)).sum() >= 5


# ---- the oracle against the float64 statement -------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ef.maps()))
def test_oracle_against_the_float64_statement(name):
    """Every direction, the poles included (the statement defines atan(0, 0) = 0 as the project does), within
    env_ref.bound: the texel contrast around the cell times the coordinate error, plus the lerps' roundings."""
    env, d = ef.maps()[name], ef.directions()
    got = ef.oracle_sky("sphere1", name).astype(np.float64)
    want, bound = env_ref.sky(env, d), env_ref.bound(env, d)
    err = np.abs(got - want)
    worst = np.argmax((err - bound).max(axis=1))
    used = bound > 0
    print("%s: largest error %.3g; largest error / bound %.3f" % (name, err.max(), (err[used] / bound[used]).max()))
    assert (err <= bound).all(), "%s: direction %s (%s): oracle %s statement %s bound %s" % (
        name, d[worst], ef.labels()[worst], got[worst], want[worst], bound[worst])


# ---- the oracle against the reference ---------------------------------------------------------------------------
def test_fixture_is_the_familys(fixture):
    assert fixture["dirs"].tobytes() == ef.fixture_directions().tobytes()
    for m in ef.FIXTURE_MAPS:
        assert fixture["map_" + m].tobytes() == ef.maps()[m].tobytes()
        assert fixture["rm1_" + m].shape == (len(fixture["dirs"]), 3)
        assert len(np.unique(fixture["rm1_" + m], axis=0)) > 100
    assert os.path.getsize(os.path.join(GOLDEN, "kat_sky.npz")) <= os.path.getsize(os.path.join(GOLDEN, "kat_default.npz"))


@pytest.mark.parametrize("variant,scene", [(1, "sphere1"), (2, "simple_rm2")])
def test_oracle_equals_the_reference_where_the_filter_cannot_matter(fixture, variant, scene):
    """The block map, the directions for which every texel within 1 / 64 texel of the lookup is equal: the
    reference returns that texel, and the oracle may differ by its roundings alone: c / 255 (e) and the lerps of
    equal values (8 e: the count in env_ref), and the reference's own c / 255 (e): 10 e v for a texel value v."""
    m = ef.FIXTURE_MAPS[0]
    env, d = fixture["map_" + m], fixture["dirs"]
    flat = env_ref.flat(env, d)
    got = ef.oracle_trace(ef.direct_oracle(scene, env), ef.direct_rays(scene, d)).astype(np.float64)[flat]
    ref = fixture["rm%d_%s" % (variant, m)].astype(np.float64)[flat]
    v = env_ref.selected(env, d).max(axis=1)[flat]
    err = np.abs(got - ref)
    print("rm%d: %d of %d directions (%.0f %%), %d texels of the map; largest difference %.3g = %.2f e v" % (
        variant, flat.sum(), len(d), 100 * flat.mean(), len(np.unique(ref, axis=0)), err.max(), (err[v > 0] / (E * v[v > 0])).max()))
    assert flat.mean() >= 0.45 and len(np.unique(ref, axis=0)) >= 100     # (the map has 128 blocks)
    assert (err <= 10 * E * v).all()
    # the seam, both clamps and both signs of every axis are among them
    fu, fv = env_ref.coordinates(d[flat], 64, 32)
    assert (fu < 0).any() and (fu > 63).any() and (fv < 0).any() and (fv > 31).any()
    for axis in range(3):
        assert (d[flat][:, axis] > 0.5).any() and (d[flat][:, axis] < -0.5).any()


@pytest.mark.parametrize("variant,scene", [(1, "sphere1"), (2, "simple_rm2")])
def test_oracle_against_the_reference_on_noise(fixture, variant, scene):
    """Per-texel noise: within K 2^-8 times the spread of the four texels the statement selects (plus the
    roundings counted above). K is measured: the ceiling of MANIFEST.json's ratio, plus one."""
    with open(os.path.join(GOLDEN, "MANIFEST.json")) as f:
        measured = json.load(f)["kat"]["sky"]["llvmpipe_ratio"]
    assert K_LLVMPIPE == math.ceil(measured) + 1
    m = ef.FIXTURE_MAPS[1]
    env, d = fixture["map_" + m], fixture["dirs"]
    got = ef.oracle_trace(ef.direct_oracle(scene, env), ef.direct_rays(scene, d)).astype(np.float64)
    ref = fixture["rm%d_%s" % (variant, m)].astype(np.float64)
    spread = env_ref.spread(env, d)
    v = env_ref.selected(env, d).max(axis=1)
    err = np.abs(got - ref)
    some = spread > 0
    print("rm%d: largest difference %.4g; largest ratio %.4f (MANIFEST %.4f); %d entries without spread" % (
        variant, err.max(), (err[some] / (spread[some] * 2.0 ** -8)).max(), measured, (~some).sum()))
    assert (err <= K_LLVMPIPE * 2.0 ** -8 * spread + 10 * E * v).all()


# ---- the sky-lit cases ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ef.CASES)
def test_a_quarter_of_the_render_ends_on_the_sky(name):
    share = ef.render_sky_share(name)
    print("%s: %.0f %% of the traced samples end on the sky" % (name, 100 * share))
    assert share >= 0.25


def test_a_quarter_of_the_separate_channels_render_ends_on_the_sky():
    share = ef.render_sky_share(ef.CASES[0], separate_channels=1)
    assert share >= 0.25


def test_glass_case_gives_no_nan_sample():
    """glass_offset renders node-program materials (refraction, glossy) under the map. A NaN direction (normalize of
    a zero vector after total internal reflection) does not reach the lookup on this scene: the march of a NaN
    direction ends as a hit (tests/golden/kat_nan.npz holds the reference to the same), so no sample is NaN, with
    the map as without it (tests/test_scene_family_cpu.py)."""
    orc = ef.case_oracle("glass_offset")
    acc = orc.trace_samples(ef.case_times(), ef.RECT0)
    assert not np.isnan(acc).any()
    e = np.asarray(ef.case_view("glass_offset")[:3], np.float32)
    assert not np.isnan(orc.trace(1, 1, 0.016, e, np.full(3, np.nan, np.float32))).any()


def test_a_quarter_of_the_consumers_rays_end_on_the_sky():
    b, p, f = ef.bake_case(), ef.probe_case(), ef.field_case()
    print("bake %.0f %%, probes %.0f %% (%d rejected, %d buried), field %.0f %% (%d buried)" % (
        100 * b["share"], 100 * p["share"], p["rejected"], p["buried"], 100 * f["share"], f["buried"]))
    assert min(b["share"], p["share"], f["share"]) >= 0.25
    assert (b["rgba"][:, 3] > 0).sum() >= 100 and (p["sh"][:, 27] > 0).sum() >= 50 and (f["sh"][:, 27] > 0).sum() >= 12


# ---- the wave form ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere1", "ground_1e4"])
def test_wave_form_equals_the_scalar_oracle(name):
    orc = ef.case_oracle(name)
    want = orc.render(ef.case_times(), rect=ef.RECT0)
    got = ef.case_oracle(name).render_wave(ef.case_times(), rect=ef.RECT0)
    assert got is not None
    assert not ef.differs(got, want).any()
    assert len(np.unique(want[..., :3].reshape(-1, 3), axis=0)) > 500
