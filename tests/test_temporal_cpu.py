"""The temporal reprojection stage (rmr_temporal_accumulate) without a GPU: the parameter
ranges and the host's view inverse, the float64 statement tests/temporal_ref.py against itself, and the
stage's gain on the CPU oracle."""
import math
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle, scene_compile
from raymarchrenderer_amd import (abi, camera_view, check_temporal_params, default_camera_view, temporal_view_inverse,
                                 time_schedule, parity_schedule)
from raymarchrenderer_amd._lib import RMRError, lib

from .conftest import ROOT, SCENES
from .denoise_ref import oracle_guides
from .temporal_ref import (coordinate_bound, project_ref, surface_guides, synthetic_case, temporal_ref, twisted,
                           view_basis)
from .test_denoise_cpu import mse

CSRC = os.path.join(ROOT, "raymarchrenderer_amd", "csrc")


def view_pair(W, H):
    """The default camera for W x H (the current view B) and a small move away from it (the history's
    view A): the eye 0.2 along x, 2 degrees of yaw."""
    m = math.sqrt(45.0)
    fov = float(np.float32(3.141592653) / np.float32(4))
    d = np.array([0.0, -3.0 / m, 6.0 / m])
    yaw = math.radians(2.0)
    d2 = np.array([d[0] * math.cos(yaw) + d[2] * math.sin(yaw), d[1], -d[0] * math.sin(yaw) + d[2] * math.cos(yaw)])
    return default_camera_view(W, H), camera_view((0.2, 4.0, -6.0), d2, float(W) / float(H), fov)


# ---- params and the view inverse ---------------------------------------------------------------------
def test_default_and_checked_params():
    p = abi.TemporalParams()
    lib().rmr_default_temporal_params(p)
    q = abi.default_temporal_params()
    assert (p.max_history, p.sigma_z, p.normal_pow2) == (q.max_history, q.sigma_z, q.normal_pow2) == (64.0, np.float32(0.02), 5)
    assert check_temporal_params()
    assert check_temporal_params(max_history=1.0, sigma_z=1e-30, normal_pow2=0)
    assert check_temporal_params(max_history=1e30, normal_pow2=7)
    for bad in ({"max_history": 0.999}, {"max_history": 0.0}, {"max_history": -4.0}, {"max_history": float("nan")},
                {"max_history": float("inf")}, {"sigma_z": 0.0}, {"sigma_z": -1.0}, {"sigma_z": float("nan")},
                {"sigma_z": float("inf")}, {"normal_pow2": -1}, {"normal_pow2": 8}):
        assert not check_temporal_params(**bad), bad
    assert lib().rmr_check_temporal_params(None) == -1
    with pytest.raises(TypeError):
        abi.default_temporal_params(sigma_c=1.0)


def _numpy_inverse(view):
    _, r00, a, b, c = view_basis(view)
    Mi = np.linalg.inv(np.stack([a, b, r00], axis=1))
    return Mi, Mi @ c


@pytest.mark.parametrize("W,H", [(44, 36), (64, 48), (1, 1)])
def test_view_inverse_matches_numpy(W, H):
    for base in view_pair(W, H):
        for view in (base, twisted(base)):
            Mi, k = temporal_view_inverse(view)
            want_M, want_k = _numpy_inverse(view)
            assert np.allclose(Mi, want_M, rtol=1e-12, atol=1e-12 * np.abs(want_M).max())
            assert np.allclose(k, want_k, rtol=1e-10, atol=1e-12)
        # rmr_camera_view's corner rays are a planar patch up to their float rounding; 5% on r11 is not
        assert np.abs(temporal_view_inverse(base)[1]).max() < 1e-6
        assert np.abs(temporal_view_inverse(twisted(base))[1]).max() > 1e-2


def test_view_inverse_refuses_degenerate_views():
    base = view_pair(44, 36)[0]
    flat = base.copy().reshape(5, 3)
    flat[1:, 2] = 0.0                                    # corner rays coplanar with the eye
    zero = base.copy().reshape(5, 3)
    zero[1] = 0.0                                        # a zero ray
    nan = base.copy()
    nan[7] = np.nan
    for bad in (flat, zero, nan):
        with pytest.raises(RMRError) as e:
            temporal_view_inverse(bad)
        assert e.value.code == -1


def _run_standalone(target):
    """csrc/temporal_test.cpp (its own main, temporal.cpp alone: no HIP, no Python in the program)."""
    subprocess.run(["make", "-s", "-C", CSRC, target], check=True, timeout=600)
    p = subprocess.run([os.path.join(CSRC, "build", target)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:]
    assert "temporal_test ok" in p.stdout, p.stdout[-4000:]
    for word in ("Sanitizer", "runtime error"):
        assert word not in p.stdout, p.stdout[-4000:]


def test_temporal_host_checks():
    _run_standalone("temporal_test")


def test_temporal_host_checks_sanitized(tmp_path):
    from .test_accel_cpu import _sanitizers_work
    if not _sanitizers_work(str(tmp_path)):
        pytest.skip("a one-line program does not build or start under -fsanitize=address,undefined")
    _run_standalone("temporal_test_san")


def test_temporal_cpp_has_no_hip():
    for name in ("temporal.cpp", "temporal.hpp", "temporal_test.cpp"):
        text = open(os.path.join(CSRC, name)).read()
        assert "#include <hip" not in text and "__global__" not in text, name


# ---- the reference against itself --------------------------------------------------------------------
def test_projection_inverts_the_guide_rays():
    """project_ref of points along the history's own rays gives back (u, v), twisted view included."""
    W, H = 44, 36
    for view in (view_pair(W, H)[1], twisted(view_pair(W, H)[1])):
        eye, r00, a, b, c = view_basis(view)
        u = np.array([0.013, 0.5, 0.987, 0.31])[None, :]
        v = np.array([0.02, 0.77, 0.45])[:, None]
        d = r00 + u[..., None] * a + v[..., None] * b + (u * v)[..., None] * c
        U, V, w = project_ref(eye + 3.7 * d, view)
        assert np.allclose(w, 3.7, rtol=1e-12) and np.allclose(U / w, u + 0 * v, atol=1e-12) and np.allclose(V / w, v + 0 * u, atol=1e-12)
        bx, by = coordinate_bound(eye + 3.7 * d, view, *temporal_view_inverse(view), W, H)
        assert (bx > 0).all() and (bx < 1e-3).all() and (by > 0).all() and (by < 1e-3).all()


def test_same_view_projects_to_own_centres_and_blends_by_count():
    W, H = 23, 19
    view = view_pair(W, H)[0]
    hit, nrm = surface_guides(view, W, H)
    rng = np.random.default_rng(3)
    S = np.ones((H, W, 4), np.float32)
    S[..., :3] = rng.uniform(0.1, 0.9, (H, W, 3))
    Hc = np.ones((H, W, 4), np.float32)
    Hc[..., :3] = rng.uniform(0.1, 0.9, (H, W, 3))
    Hn = rng.uniform(1.0, 30.0, (H, W)).astype(np.float32)
    nrm[2, 3] = (0, 0, 0, -1)
    S[4, 5, 3] = 0.0
    n_cur = 4.0
    r = temporal_ref(S, hit, nrm, Hc, Hn, hit, nrm, view, n_cur)
    live = r["live"]
    assert not live[2, 3] and not live[4, 5] and live.sum() == W * H - 2
    ys, xs = np.mgrid[0:H, 0:W]
    # the hit points are float32 roundings of points on the pixel-centre rays: 1e-4 of a pixel
    assert np.abs(r["xy"][..., 0] - (xs + 0.5))[live].max() < 1e-4 and np.abs(r["xy"][..., 1] - (ys + 0.5))[live].max() < 1e-4
    m = Hn.astype(np.float64)[..., None]
    want = (m * Hc[..., :3] + n_cur * S[..., :3].astype(np.float64)) / (m + n_cur)
    # (the three neighbouring taps carry the 1e-4 of bilinear weight the centre tap lacks)
    assert np.abs(r["out"][..., :3] - want)[live].max() < 1e-3
    assert np.abs(r["n"] - np.minimum(Hn + n_cur, 64.0))[live].max() < 1e-2
    assert (r["out"][~live] == S[~live]).all() and (r["n"][~live] == 0).all()
    assert (r["out"][..., 3] == S[..., 3]).all()


def test_history_of_other_ids_is_ignored():
    W, H = 23, 19
    view, h_view = view_pair(W, H)
    c = synthetic_case(W, H, view, h_view)
    other = c["h_nrm"].copy()
    other[..., 3] = np.where(other[..., 3] >= 0, other[..., 3] + 10.0, -1.0)
    r = temporal_ref(c["S"], c["hit"], c["nrm"], c["h_rgba"], c["h_n"], c["h_hit"], other, h_view, 4.0)
    S = c["S"]
    assert r["live"].any() and not r["used"].any()
    same = (r["out"] == S) | (np.isnan(r["out"]) & np.isnan(S))
    assert same.all()
    assert (r["n"][r["live"]] == 4.0).all() and (r["n"][~r["live"]] == 0).all()
    # and with the real ids most live pixels do find their history
    r = temporal_ref(c["S"], c["hit"], c["nrm"], c["h_rgba"], c["h_n"], c["h_hit"], c["h_nrm"], h_view, 4.0)
    assert r["used"].sum() > 0.5 * r["live"].sum()
    assert np.isnan(r["xy"][~r["projected"]]).all() and np.isfinite(r["xy"][r["projected"]]).all()
    whats = {w for w, _, _ in c["planted"]}
    assert {"behind", "off left", "off right", "off top", "off bottom", "sky", "nan", "alpha 0", "firefly"} <= whats
    for what, y, x in c["planted"]:
        if what == "behind":
            assert r["live"][y, x] and not r["projected"][y, x]
        if what.startswith("off "):
            assert r["projected"][y, x] and not r["used"][y, x] and r["n"][y, x] == 4.0


# ---- quality, on the oracle ---------------------------------------------------------------------------
# measured ratio (see the test): 4 spp of B blended with 4 spp of A against 4 spp of B alone
MEASURED_RATIO = 0.607


def test_blend_of_two_views_beats_one_on_the_oracle():
    """Cornell-5 at 64x48, view B the default camera, view A 0.2 along x (2% of the room's 10 units) and 2
    degrees of yaw away. MSE against a 512-spp oracle render of B: 4 spp of B blended with 4 spp of A
    (independent seeds) through temporal_ref with the oracle's own guides, over 4 spp of B alone. Two
    independent equal-weight estimates halve the variance where the history is valid. The assertion is
    the midpoint between the measured ratio and 1, so that the noise of the 512-spp stand-in cannot
    flip it."""
    W, H = 64, 48
    B, A = view_pair(W, H)
    tables = scene_compile.load_scene_file(os.path.join(SCENES, "cornell5.scene"), "rm1")
    prm = abi.default_params(max_bounces=4)

    def render(view, times):
        orc = oracle.Oracle(tables, prm, view, W, H)
        img = orc.render_wave(times)
        return img if img is not None else orc.render(times)
    ref = render(B, parity_schedule(512))
    b4 = render(B, time_schedule(4, first_sample=1000))
    a4 = render(A, time_schedule(4, first_sample=2000))
    hit, nrm = oracle_guides(tables, prm, B, W, H)
    h_hit, h_nrm = oracle_guides(tables, prm, A, W, H)
    h_n = np.full((H, W), 4.0, np.float32)
    r = temporal_ref(b4, hit, nrm, a4, h_n, h_hit, h_nrm, A, 4.0)
    e_one, e_two = mse(b4, ref), mse(r["out"], ref)
    ratio = e_two / e_one
    print("cornell5 64x48: MSE 4 spp of B %.4e, blended with 4 spp of A %.4e, ratio %.3f; history used at %.1f%% of the live pixels"
          % (e_one, e_two, ratio, 100.0 * r["used"].sum() / max(1, r["live"].sum())))
    assert ratio < 0.5 * (MEASURED_RATIO + 1.0)
