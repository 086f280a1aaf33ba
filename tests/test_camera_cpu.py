"""Camera models and caller-supplied rays, the parts that need no GPU: rmr_check_camera_model,
rmr_check_rays and rmr_camera_frame against their numpy statement (tests/camera_ref.py), the float64
statement of the three models itself, and the hipRTC ray-source kernel of every scene class (compiled
for gfx950, not run).
"""
import os
import subprocess

import numpy as np
import pytest

from oracle import camera
from raymarchrenderer_amd import abi, camera_frame, check_camera_model, check_rays, lib
from raymarchrenderer_amd._lib import RMRError
from raymarchrenderer_amd.renderer import jit_compile_scene

from . import camera_ref
from .conftest import GOLDEN, ROOT, SCENES

CSRC = os.path.join(ROOT, "raymarchrenderer_amd", "csrc")
W, H = 44, 36
VIEW = camera.default_view(W, H)
NAN, INF = float("nan"), float("inf")


def test_abi_sizes_and_defaults():
    import ctypes as C
    assert np.dtype(abi.RAY_DTYPE).itemsize == 40 and C.sizeof(abi.Ray) == 40 and C.sizeof(abi.CameraModel) == 20
    m = abi.CameraModel(9, 9, 9, 9, 9)
    lib().rmr_default_camera_model(C.byref(m))
    assert (m.model, m.aperture, m.focus, m.width, m.height) == (abi.CAMERA_VIEW, 0.0, 1.0, 1.0, 1.0)
    d = abi.default_camera_model()
    assert bytes(m) == bytes(d)


MODEL_CASES = [
    (abi.CAMERA_VIEW, {}), (abi.CAMERA_EQUIRECT, {}),
    # a model's check looks at its own fields only
    (abi.CAMERA_VIEW, {"aperture": NAN, "width": -1.0}), (abi.CAMERA_EQUIRECT, {"focus": -1.0}),
    (abi.CAMERA_THIN_LENS, {"aperture": 0.0, "focus": 1.0}), (abi.CAMERA_THIN_LENS, {"aperture": 0.25, "focus": 1e-30}),
    (abi.CAMERA_THIN_LENS, {"aperture": 0.0, "focus": 5.0, "width": NAN}),
    (abi.CAMERA_THIN_LENS, {"aperture": -1e-30, "focus": 1.0}), (abi.CAMERA_THIN_LENS, {"aperture": -0.0, "focus": 1.0}),
    (abi.CAMERA_THIN_LENS, {"aperture": 0.1, "focus": 0.0}), (abi.CAMERA_THIN_LENS, {"aperture": 0.1, "focus": -2.0}),
    (abi.CAMERA_THIN_LENS, {"aperture": NAN, "focus": 1.0}), (abi.CAMERA_THIN_LENS, {"aperture": 0.1, "focus": NAN}),
    (abi.CAMERA_THIN_LENS, {"aperture": INF, "focus": 1.0}), (abi.CAMERA_THIN_LENS, {"aperture": 0.1, "focus": INF}),
    (abi.CAMERA_ORTHO, {"width": 2.0, "height": 1e-30}), (abi.CAMERA_ORTHO, {"width": 0.0, "height": 1.0}),
    (abi.CAMERA_ORTHO, {"width": 1.0, "height": -1.0}), (abi.CAMERA_ORTHO, {"width": INF, "height": 1.0}),
    (abi.CAMERA_ORTHO, {"width": 1.0, "height": NAN}), (abi.CAMERA_ORTHO, {"width": 3.0, "height": 2.0, "aperture": -1.0}),
    (-1, {}), (4, {}), (1 << 30, {}),
]


@pytest.mark.parametrize("model,fields", MODEL_CASES, ids=[str(i) for i in range(len(MODEL_CASES))])
def test_check_camera_model(model, fields):
    f = dict(aperture=0.0, focus=1.0, width=1.0, height=1.0)
    f.update(fields)
    want = camera_ref.model_ok(model, **{k: float(np.float32(v)) for k, v in f.items()})
    assert check_camera_model(abi.CameraModel(model, f["aperture"], f["focus"], f["width"], f["height"])) == want


def test_check_camera_model_accepts_and_rejects():
    """The cases above are not all on one side."""
    got = [camera_ref.model_ok(m, **dict(dict(aperture=0.0, focus=1.0, width=1.0, height=1.0), **f)) for m, f in MODEL_CASES]
    assert 8 <= sum(got) <= len(got) - 8
    assert lib().rmr_check_camera_model(None) == -1


def _rays(n=4):
    r = np.zeros(n, np.dtype(abi.RAY_DTYPE))
    r["d"][:, 2] = 1.0
    return r


def _ray_cases():
    cases = []
    ok = _rays()
    ok["o"] = [[0, 0, 0], [1e30, -1e30, 5], [-3, 2, 1], [0.5, 0.25, 0]]
    ok["d"][1] = np.array([3.0, -4.0, 12.0], np.float32) / np.float32(13.0)
    ok["gx"], ok["gy"] = [0, 2 ** 24 - 1, 7, 9], [2 ** 24 - 1, 0, 3, 1]
    ok["time"], ok["rc"] = [0, 1000.016, -3, 0.5], [0, 0.999, 0.25, 0]
    cases.append(("ok", ok))
    cases.append(("empty", _rays(0)))
    for field, idx, val in [("o", (2, 1), NAN), ("o", (0, 0), INF), ("d", (3, 2), NAN), ("time", (1,), INF),
                            ("rc", (2,), NAN), ("gx", (0,), -1), ("gy", (3,), 2 ** 24), ("gx", (3,), 2 ** 24),
                            ("gy", (1,), -(2 ** 31))]:
        r = ok.copy()
        r[field][idx] = val
        cases.append(("%s%s=%s" % (field, idx, val), r))
    # |d.d - 1| <= 1e-5 in double, on both sides of the bound, for the last ray of the list
    for s in [1.0 + 4e-6, 1.0 - 4e-6, 1.0 + 6e-6, 1.0 - 6e-6, 0.0, 2.0]:
        r = ok.copy()
        r["d"][3] = [0.0, 0.0, s]
        cases.append(("len%g" % s, r))
    return cases


@pytest.mark.parametrize("name,rays", _ray_cases(), ids=[c[0] for c in _ray_cases()])
def test_check_rays(name, rays):
    assert check_rays(rays) == camera_ref.rays_ok(rays), name


def test_check_rays_accepts_and_rejects():
    got = [camera_ref.rays_ok(r) for _, r in _ray_cases()]
    assert sum(got) >= 4 and len(got) - sum(got) >= 10
    assert lib().rmr_check_rays(None, 3) == -1 and lib().rmr_check_rays(None, 0) == 0


def _views():
    rng = np.random.default_rng(5)
    out = [("default", VIEW), ("wide", camera.default_view(200, 50)),
           ("tilted", camera.view_uniforms((3.0, -2.0, 1.0), tuple(np.array([1.0, 2.0, -2.0]) / 3.0), 1.5, 1.0))]
    # a sheared frustum: corner rays that are neither unit nor symmetric
    v = VIEW.copy().reshape(5, 3)
    v[2] *= np.float32(1.7)
    v[4] += np.float32(0.3)
    out.append(("sheared", v.reshape(15)))
    out.append(("random", rng.normal(size=15).astype(np.float32)))
    return out


@pytest.mark.parametrize("name,view", _views(), ids=[v[0] for v in _views()])
def test_camera_frame_matches_numpy(name, view):
    got = camera_frame(view)
    want = camera_ref.frame(view)
    assert got.dtype == np.float32 and got.shape == (3, 3)
    # computed in double, rounded once: the float nearest to the float64 statement, or its neighbour
    # where the two double evaluations (different summation order in dot products) straddle a tie
    assert np.abs(got.astype(np.float64) - want).max() <= 2.0 ** -24, name
    g = got.astype(np.float64)
    assert np.abs(g @ g.T - np.eye(3)).max() <= 4 * 2.0 ** -24, name   # orthonormal to float precision


def test_camera_frame_of_the_default_view():
    U, V, FWD = camera_frame(VIEW).astype(np.float64)
    v = VIEW.astype(np.float64).reshape(5, 3)
    assert U.dot(v[2] - v[1]) > 0 and V.dot(v[3] - v[1]) > 0 and FWD.dot(v[1:].sum(axis=0)) > 0
    # Program.cpp's camera looks along (0, -3, 6) / sqrt(45) with x to the right and the image's rows downwards
    assert np.abs(FWD - np.array([0.0, -3.0, 6.0]) / np.sqrt(45.0)).max() < 1e-6
    assert np.abs(U - [1.0, 0.0, 0.0]).max() < 1e-6 and V[1] < 0


@pytest.mark.parametrize("name", ["nan", "inf", "u0", "v_parallel", "fwd0", "all_equal"])
def test_camera_frame_degenerate(name):
    v = VIEW.copy().reshape(5, 3)
    if name == "nan":
        v[3, 1] = NAN
    elif name == "inf":
        v[0, 0] = INF
    elif name == "u0":
        v[2] = v[1]
    elif name == "v_parallel":
        v[3] = v[1] + np.float32(2.0) * (v[2] - v[1])
    elif name == "fwd0":
        v[1], v[2], v[3], v[4] = [-1, -1, 0], [1, -1, 0], [-1, 1, 0], [1, 1, 0]
    else:
        v[1:] = v[1]
    assert camera_ref.frame(v.reshape(15)) is None
    with pytest.raises(RMRError) as e:
        camera_frame(v.reshape(15))
    assert e.value.code == -1


def _run_standalone(target):
    """csrc/camera_test.cpp (its own main, camera.cpp alone: no HIP, no Python in the program)."""
    subprocess.run(["make", "-s", "-C", CSRC, target], check=True, timeout=600)
    p = subprocess.run([os.path.join(CSRC, "build", target)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:]
    assert "camera_test ok" in p.stdout, p.stdout[-4000:]
    for word in ("Sanitizer", "runtime error"):
        assert word not in p.stdout, p.stdout[-4000:]


def test_camera_host_checks():
    _run_standalone("camera_test")


def test_camera_host_checks_sanitized(tmp_path):
    from .test_accel_cpu import _sanitizers_work
    if not _sanitizers_work(str(tmp_path)):
        pytest.skip("a one-line program does not build or start under -fsanitize=address,undefined")
    _run_standalone("camera_test_san")


# ---- the float64 statement of the models ----------------------------------------------------------
TIMES = [0.0, 0.016, 1000.5]
PIXELS = [(0, 0), (43, 35), (17, 9), (8, 31)]


def test_chain_is_the_oracles_and_rc_its_last_value():
    from oracle import oracle
    for (px, py) in PIXELS:
        for t in TIMES:
            c5 = camera_ref.chain(px, py, t, 5)
            c3 = camera_ref.chain(px, py, t, 3)
            assert (c5[:3].view(np.uint32) == c3.view(np.uint32)).all()
            assert ((c5 >= 0) & (c5 < 1)).all()
            gxt, gyt = np.float32(px) + np.float32(t), np.float32(py) + np.float32(t)
            want = oracle.rand_chain(px, py, t, np.array([(gxt, gyt), (gxt, gyt), (gyt, gxt)], np.float32))
            assert (c3.view(np.uint32) == want.view(np.uint32)).all()
            for model, f, n in [(camera_ref.THIN_LENS, dict(aperture=0.0, focus=2.0), 3), (camera_ref.EQUIRECT, {}, 3),
                                (camera_ref.ORTHO, dict(width=2.0, height=1.0), 3),
                                (camera_ref.THIN_LENS, dict(aperture=0.5, focus=2.0), 5)]:
                rc = camera_ref.ray(model, VIEW, W, H, px, py, t, **f)[2]
                assert np.float32(rc).view(np.uint32) == c5[n - 1].view(np.uint32)


def test_thin_lens_rays_pass_through_the_focus_point():
    """Every lens sample of a pixel sample's dir0 meets the sphere of radius focus about the eye at the
    same point F: the distance from F to the ray's line is zero (float64: <= 1e-12 of the focus)."""
    eye = VIEW.astype(np.float64)[:3]
    for focus in (0.5, 6.0):
        for (px, py) in PIXELS:
            for t in TIMES:
                o, d, _, Fp = camera_ref.ray(camera_ref.THIN_LENS, VIEW, W, H, px, py, t, aperture=0.4, focus=focus)
                assert abs(np.linalg.norm(d) - 1) < 1e-12
                assert abs(np.linalg.norm(Fp - eye) - focus) < 1e-12 * max(1.0, focus)
                assert np.linalg.norm(np.cross(Fp - o, d)) <= 1e-12 * focus
                assert (Fp - o).dot(d) > 0
                # the origin lies on the lens: in the U-V plane through the eye, within the aperture
                U, V, FWD = camera_ref.frame(VIEW)
                assert abs((o - eye).dot(FWD)) < 1e-12 and np.linalg.norm(o - eye) <= 0.4 * (1 + 1e-12)
                # aperture 0: the view's own ray
                o0, d0, _, F0 = camera_ref.ray(camera_ref.THIN_LENS, VIEW, W, H, px, py, t, aperture=0.0, focus=focus)
                assert (o0 == eye).all() and np.abs(F0 - Fp).max() < 1e-12
                assert np.abs(d0 - camera_ref.ray(camera_ref.VIEW, VIEW, W, H, px, py, t)[1]).max() == 0


def test_lens_samples_fill_the_disk():
    eye = VIEW.astype(np.float64)[:3]
    U, V, _ = camera_ref.frame(VIEW)
    pts = []
    for px in range(0, W, 3):
        for py in range(0, H, 3):
            o = camera_ref.ray(camera_ref.THIN_LENS, VIEW, W, H, px, py, 0.016, aperture=1.0, focus=3.0)[0]
            pts.append(((o - eye).dot(U), (o - eye).dot(V)))
    pts = np.array(pts)
    r = np.linalg.norm(pts, axis=1)
    assert r.max() <= 1 + 1e-12 and r.max() > 0.95
    for sx in (-1, 1):
        for sy in (-1, 1):   # every quadrant, and the inner half of the area holds about half the points
            assert ((pts[:, 0] * sx > 0) & (pts[:, 1] * sy > 0)).mean() > 0.15
    assert 0.35 < (r * r < 0.5).mean() < 0.65


def test_equirect_covers_the_sphere():
    U, V, FWD = camera_ref.frame(VIEW)
    d = np.array([[camera_ref.ray(camera_ref.EQUIRECT, VIEW, W, H, px, py, 0.0)[1] for px in range(W)] for py in range(H)])
    assert np.abs(np.linalg.norm(d, axis=-1) - 1).max() < 1e-12
    assert (d[0] @ V).max() < -0.99 and (d[-1] @ V).min() > 0.99            # row 0 looks up (-V), the last row down
    mid = d[H // 2]
    assert (mid[W // 2] @ FWD) > 0.98 and (mid[0] @ FWD) < -0.98             # centre column forward, the edge behind
    assert (mid[3 * W // 4] @ U) > 0.98 and (mid[W // 4] @ U) < -0.98        # longitude grows towards U
    for axis in (U, V, FWD):                                                # every octant of the frame is hit
        assert ((d @ axis) > 0.5).any() and ((d @ axis) < -0.5).any()
    signs = {tuple(np.sign(np.array([q @ U, q @ V, q @ FWD])).astype(int)) for q in d.reshape(-1, 3)}
    assert len({s for s in signs if 0 not in s}) == 8   # (a direction exactly in a coordinate plane counts for none)
    # rows are circles of constant polar angle up to the row's jitter: pi / H
    pol = np.arccos(np.clip(-(d @ V), -1, 1))
    assert (pol.max(axis=1) - pol.min(axis=1)).max() <= np.pi / H + 1e-9


def test_ortho_rays_are_parallel():
    U, V, FWD = camera_ref.frame(VIEW)
    eye = VIEW.astype(np.float64)[:3]
    for (px, py) in PIXELS + [(0, 35), (43, 0)]:
        for t in TIMES:
            o, d, _, _ = camera_ref.ray(camera_ref.ORTHO, VIEW, W, H, px, py, t, width=8.0, height=6.0)
            assert (d == FWD).all()
            x, y = (o - eye).dot(U), (o - eye).dot(V)
            assert abs((o - eye).dot(FWD)) < 1e-12
            assert 8.0 * (px / W - 0.5) <= x + 1e-12 and x < 8.0 * ((px + 1) / W - 0.5) + 1e-12   # inside its pixel's cell
            assert 6.0 * (py / H - 0.5) <= y + 1e-12 and y < 6.0 * ((py + 1) / H - 0.5) + 1e-12


# ---- the specialised ray-source kernel, compiled for gfx950 (not run) ------------------------------
JIT_CASES = [("cornell5", os.path.join(SCENES, "cornell5.scene"), "rm1"),
             ("default", os.path.join(GOLDEN, "scenes", "default.scene"), "rm1"),
             ("csg64", os.path.join(SCENES, "csg64.scene"), "rm1"),
             ("mandelbulb", os.path.join(SCENES, "mandelbulb.scene"), "rm1"),
             ("simple_rm2", os.path.join(GOLDEN, "scenes", "simple.scene"), "rm2"),
             ("rm3", None, "rm3")]


@pytest.mark.parametrize("name,path,variant", JIT_CASES, ids=[c[0] for c in JIT_CASES])
def test_ray_source_kernel_compiles(name, path, variant, tmp_path, monkeypatch):
    """rmr_jit_trace_rays of every kernel class builds, under its own code-object key."""
    import ctypes as C
    monkeypatch.setenv("RMR_JIT_CACHE", str(tmp_path))
    text = open(path, "rb").read() if path else b""
    log = C.create_string_buffer(65536)
    rc = lib().rmr_jit_compile_scene_rays(abi.VARIANTS[variant], text or None, len(text), log, len(log))
    assert rc == 0, log.value.decode(errors="replace")[:2000]
    key_rays = log.value.decode()
    assert key_rays != jit_compile_scene(path, variant)
    assert os.path.exists(os.path.join(str(tmp_path), key_rays + ".hsaco"))
