"""skyColor's env-map lookup on the GPU (sky_color in csrc/rmr_trace.h), on the maps, directions and sky-lit cases
of tests/env_family.py. Every comparison is bit for bit (NaN equals NaN) against the CPU oracle, which
tests/test_env_family_cpu.py holds to a float64 statement of the lookup and to the reference's own skyColor.

  1. the lookup alone: trace_rays of rays that leave the scene, on every map, under the table interpreter and the
     generated kernel, with every culling switch and with none (the escape bound ends these marches), for RM1 and
     for simple.scene under rm2; the device form on the 37 x 19 map;
  2. replacing the map on one context, the error returns, and a context that had a map and cleared it;
  3. renders with a clip rect that cuts 8x8 tiles on every sky-lit case, one with separateChannels, and one
     context switching useEnvTex 0 -> 1 -> 0 with lane slots on (the slot request and the hipRTC kernel change);
  4. the consumers under an open sky: bake_points, bake_probes, bake_probe_field, a render under the equirect
     model, a one-device DeviceGroup, and rmr_cli --env-map."""
import os
import subprocess

import numpy as np
import pytest

from oracle import camera, oracle
from raymarchrenderer_amd import Renderer, RMRError, abi, default_camera_view, time_schedule
from raymarchrenderer_amd.group import DeviceGroup

from . import env_family as ef
from . import feature_family as ff
from .conftest import ROOT
from .test_gpu_parity import same_bits
from .test_gpu_rays import _running_means

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "raymarchrenderer_amd", "rmr_cli")
ENV = ef.maps()[ef.RENDER_MAP]


def _assert_same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    eq = same_bits(got, want)
    eq = eq.reshape(len(eq), -1).all(axis=1)
    assert eq.all(), "%s: %d/%d entries differ; first %d gpu=%s cpu=%s" % (
        what, (~eq).sum(), len(eq), np.argmin(eq), got[np.argmin(eq)].ravel()[:6], want[np.argmin(eq)].ravel()[:6])


def _direct_context(scene, jit=0):
    path, variant = ef.DIRECT[scene][:2]
    r = Renderer(0, 8, 8)
    r.set_jit(jit)
    r.load_scene(path, variant)
    r.set_params(ef.direct_params(scene))
    r.set_view(camera.default_view(8, 8))
    return r


def _case_context(name, jit=0, **kw):
    r = Renderer(0, ef.W0, ef.H0)
    r.set_jit(jit)
    r.load_scene(ef.case_scene(name), "rm1")
    r.set_params(ef.case_params(name, **kw))
    r.set_view(ef.case_view(name))
    r.set_env_map(ENV)
    return r


# ---- 1. the lookup alone ------------------------------------------------------------------------------------
@pytest.mark.parametrize("culling", [abi.CULL_ALL, 0], ids=["cull_all", "no_culling"])
@pytest.mark.parametrize("jit", [0, 1], ids=["table", "jit"])
@pytest.mark.parametrize("scene", sorted(ef.DIRECT))
def test_lookup_alone(scene, jit, culling):
    rays = ef.direct_rays(scene)
    r = _direct_context(scene, jit)
    try:
        r.set_culling(culling)
        for name, env in ef.maps().items():
            r.set_env_map(env)
            t0 = r.stats().trace_launches
            out = r.trace_rays(rays)
            assert r.stats().trace_launches - t0 == 1                  # the list fits in one launch
            assert (out[:, 3] == 1).all()
            _assert_same(out[:, :3], ef.oracle_sky(scene, name), "%s, map %s, jit %d, culling %d" % (scene, name, jit, culling))
        st = r.stats()
        assert st.jit_launches == (st.trace_launches if jit else 0)
    finally:
        r.close()


def test_lookup_alone_device_form():
    import torch
    scene = "sphere1"
    rays = ef.direct_rays(scene)
    want = ef.oracle_sky(scene, ef.RENDER_MAP)
    r = _direct_context(scene)
    try:
        r.set_env_map(ENV)
        host = r.trace_rays(rays)
        dev_rays = torch.from_numpy(np.array(rays).view(np.uint8).reshape(len(rays), 40)).cuda()
        dev = r.trace_rays_device(dev_rays, float(np.abs(rays["o"]).max()))
        r.sync()
        assert r.query_rejects() == 0
        _assert_same(dev.cpu().numpy(), host, "trace_rays_device against trace_rays")
        _assert_same(host[:, :3], want, "trace_rays against the oracle")
    finally:
        r.close()


# ---- 2. replacing the map -----------------------------------------------------------------------------------
def _set_raw(r, buf, w, h):
    r._chk(r.lib.rmr_set_env_map(r.ctx, buf.ctypes.data, w, h))


def test_replacing_the_map_and_error_returns():
    scene = "sphere1"
    rays = ef.direct_rays(scene)
    r = _direct_context(scene)
    try:
        for name in ("noise64x32", "noise5x1", "ramp4096x1", "noise1x1"):
            r.set_env_map(ef.maps()[name])
            _assert_same(r.trace_rays(rays)[:, :3], ef.oracle_sky(scene, name), "after replacing the map by %s" % name)
        # sizes that are refused: code -1, and the map in place stays
        small = np.zeros(64, np.uint8)
        for w, h in ((0, 4), (4, -1), (-3, 4), (1 << 13, (1 << 13) + 1), (1 << 26, 2)):
            with pytest.raises(RMRError) as e:
                _set_raw(r, small, w, h)                                # (refused before the pointer is read)
            assert e.value.code == -1, (w, h)
        _assert_same(r.trace_rays(rays)[:, :3], ef.oracle_sky(scene, "noise1x1"), "after the refused sizes")
        # useEnvTex without a map: code -5
        r.set_env_map(None)
        with pytest.raises(RMRError) as e:
            r.trace_rays(rays)
        assert e.value.code == -5
        with pytest.raises(RMRError) as e:
            r.render_spp(time_schedule(1))
        assert e.value.code == -5
        # a map without useEnvTex: the constant sky
        r.set_env_map(ef.maps()["noise64x32"])
        prm = ef.direct_params(scene)
        prm.use_env_tex = 0
        r.set_params(prm)
        const = ef.oracle_trace(oracle.Oracle(ef.direct_tables(scene), prm, camera.default_view(8, 8), 8, 8), rays)
        assert len(np.unique(const)) == 1
        _assert_same(r.trace_rays(rays)[:, :3], const, "useEnvTex = 0 with a map set")
    finally:
        r.close()


def test_a_cleared_map_leaves_a_fresh_context():
    name = "sphere1"
    times = ef.case_times()
    prm = ef.case_params(name)
    prm.use_env_tex = 0
    r = _case_context(name)
    fresh = Renderer(0, ef.W0, ef.H0)
    try:
        r.render_spp(times, ef.RECT0)
        with_map = r.read_accum()
        r.set_env_map(None)
        r.set_params(prm)
        r.reload()
        r.render_spp(times, ef.RECT0)
        fresh.set_jit(0)
        fresh.load_scene(ef.case_scene(name), "rm1")
        fresh.set_params(prm)
        fresh.set_view(ef.case_view(name))
        fresh.render_spp(times, ef.RECT0)
        want = oracle.Oracle(ef.case_tables(name), prm, ef.case_view(name), ef.W0, ef.H0).render(times, rect=ef.RECT0)
        _assert_same(r.read_accum(), fresh.read_accum(), "cleared against fresh")
        _assert_same(r.read_accum(), want, "cleared against the oracle")
        assert not same_bits(with_map, want).all()
    finally:
        r.close()
        fresh.close()


# ---- 3. renders -----------------------------------------------------------------------------------------------
_render_want = {}


def _oracle_render(name, **kw):
    key = (name, tuple(sorted(kw.items())))
    if key not in _render_want:
        _render_want[key] = ef.case_oracle(name, **kw).render(ef.case_times(), rect=ef.RECT0)
    return _render_want[key]


@pytest.mark.parametrize("jit", [0, 1], ids=["table", "jit"])
@pytest.mark.parametrize("name", ef.CASES)
def test_render_bitexact(name, jit):
    want = _oracle_render(name)
    r = _case_context(name, jit)
    try:
        r.render_spp(ef.case_times(), ef.RECT0)
        _assert_same(r.read_accum(), want, "%s, jit %d" % (name, jit))
        st = r.stats()
        assert st.jit_launches == (st.trace_launches if jit else 0) and st.trace_launches >= 1
    finally:
        r.close()


@pytest.mark.parametrize("jit", [0, 1], ids=["table", "jit"])
def test_render_separate_channels_bitexact(jit):
    name = ef.CASES[0]
    want = _oracle_render(name, separate_channels=1)
    r = _case_context(name, jit, separate_channels=1)
    try:
        r.render_spp(ef.case_times(), ef.RECT0)
        _assert_same(r.read_accum(), want, "%s, separateChannels, jit %d" % (name, jit))
    finally:
        r.close()


def test_switching_use_env_tex_with_lane_slots_on():
    """0 -> 1 -> 0 on one context under the generated kernel with lane slots on: an env-map launch is generated with
    the slot request 0, so the kernel changes each time; each render is the oracle's."""
    name = ef.CASES[0]
    times = ef.case_times()
    off = ef.case_params(name)
    off.use_env_tex = 0
    want_off = oracle.Oracle(ef.case_tables(name), off, ef.case_view(name), ef.W0, ef.H0).render(times, rect=ef.RECT0)
    want_on = _oracle_render(name)
    assert not same_bits(want_on, want_off).all()
    r = _case_context(name, jit=1)
    try:
        r.set_tuning(lane_slots=True)
        for k, (prm, want) in enumerate(((off, want_off), (ef.case_params(name), want_on), (off, want_off))):
            r.set_params(prm)
            r.reload()
            r.reset_stats()
            r.render_spp(times, ef.RECT0)
            _assert_same(r.read_accum(), want, "render %d, useEnvTex %d" % (k, prm.use_env_tex))
            assert r.stats().jit_launches >= 1
    finally:
        r.close()


# ---- 4. the consumers -----------------------------------------------------------------------------------------
def test_bake_points_under_the_sky():
    c = ef.bake_case()
    r = _case_context(ef.BAKE_CASE)
    try:
        got = r.bake_points(c["p"], c["n"], ff.seeds(ef.BAKE_SEEDS), radiance=True, ao=False, bias=ff.bias(ef.BAKE_CASE),
                            first_index=ef.FIRST)
        _assert_same(got["rgba"], c["rgba"], "bake_points radiance")
        assert r.query_rejects() == len(c["rejects"])
    finally:
        r.close()


def test_bake_probes_under_the_sky():
    c = ef.probe_case()
    r = _case_context(ef.PROBE_CASE)
    try:
        got = r.bake_probes(c["p"], ff.seeds(ef.PROBE_SEEDS), first_index=ef.FIRST, clearance=0.0)
        _assert_same(got, c["sh"], "bake_probes")
        assert r.query_rejects() == c["rejected"]
    finally:
        r.close()


def test_bake_probe_field_under_the_sky():
    c = ef.field_case()
    r = _case_context(ef.FIELD_CASE)
    try:
        r.bake_probe_field(c["desc"], times=ff.seeds(ef.FIELD_SEEDS), clearance=0.0)
        d, got = r.read_probe_field()
        assert bytes(d) == bytes(c["desc"])
        _assert_same(got, c["sh"], "bake_probe_field")
    finally:
        r.probe_field_free()
        r.close()


def test_equirect_render_is_the_mean_of_its_traced_camera_rays():
    name = ef.EQUIRECT_CASE
    times = ef.case_times()
    x0, y0, x1, y1 = ef.RECT0
    r = _case_context(name)
    try:
        r.set_camera_model("equirect")
        rays = r.camera_rays(times, ef.RECT0)
        rad = r.trace_rays(rays).reshape(rays.shape + (4,))
        # the rays that miss the scene see the sky alone: Oracle.trace of them (it starts a fresh chain, the camera's
        # rays carry theirs, so the rays that bounce are left to the mean below)
        flat = rays.reshape(-1)
        tb, prm = ef.case_tables(name), ef.case_params(name)
        miss = np.array([oracle.march(tb, q["o"], q["d"], params=prm)[0] >= prm.max_dist for q in flat])
        assert 0.9 <= miss.mean() < 1.0
        _assert_same(rad.reshape(-1, 4)[miss, :3], ef.oracle_trace(ef.case_oracle(name), flat[miss]), "trace_rays of the camera's sky rays")
        assert len(np.unique(rad[..., :3].reshape(-1, 3), axis=0)) > 1000      # the map, not a constant
        want = np.zeros((ef.H0, ef.W0, 4), np.float32)
        want[y0:y1, x0:x1, :3] = _running_means(rad)[-1]
        want[y0:y1, x0:x1, 3] = 1.0
        r.render_spp(times, ef.RECT0)
        _assert_same(r.read_accum(), want, "render_spp under equirect")
    finally:
        r.close()


def test_device_group_set_env_map():
    name = ef.GROUP_CASE
    times = ef.case_times()
    want = ef.case_oracle(name).render(times)
    g = DeviceGroup([0], ef.W0, ef.H0, tile=16)
    r = _case_context(name)
    try:
        g.load_scene(ef.case_scene(name), "rm1")
        g.set_params(ef.case_params(name))
        g.set_view(ef.case_view(name))
        g.set_env_map(ENV)
        g.reload()
        g.render_frame(times)
        got = g.read_frame()
        r.render_spp(times)
        _assert_same(got, r.read_accum(), "group against one context")
        _assert_same(got, want, "group against the oracle")
    finally:
        g.close()
        r.close()


def test_cli_env_map_option(tmp_path):
    """rmr_cli --env-map FILE WxH at 48 x 32: the BMP the Python pipeline writes, byte for byte; another image than
    without the map; a file of the wrong size is an error."""
    W, H = 48, 32
    raw = str(tmp_path / "env.rgba8")
    ENV.tofile(raw)
    h, w = ENV.shape[:2]
    out, want, plain = str(tmp_path / "cli.bmp"), str(tmp_path / "want.bmp"), str(tmp_path / "plain.bmp")
    base = [CLI, "--scene", ef.SPHERE1, "--variant", "rm1", "--size", "%dx%d" % (W, H), "--samples", "3", "--bounces", "4", "--quiet"]
    p = subprocess.run(base + ["--out", out, "--env-map", raw, "%dx%d" % (w, h)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    q = subprocess.run(base + ["--out", plain], capture_output=True, text=True, timeout=120)
    assert q.returncode == 0, q.stdout + q.stderr
    bad = subprocess.run(base + ["--out", plain, "--env-map", raw, "%dx%d" % (w + 1, h)], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 1
    r = Renderer(0, W, H)
    try:
        r.load_scene(ef.SPHERE1, "rm1")
        r.set_params(abi.default_params(max_bounces=4, use_env_tex=1))
        r.set_view(default_camera_view(W, H))
        r.set_env_map(ENV)
        r.render_spp(time_schedule(3))
        r.save_bmp(want)
    finally:
        r.close()
    cli_bytes = open(out, "rb").read()
    assert cli_bytes == open(want, "rb").read()
    assert cli_bytes != open(plain, "rb").read()
