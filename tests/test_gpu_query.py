"""First-hit and distance queries and the device-resident ray list on the GPU (include/rmr.h, DESIGN.md
§4.10): rmr_cast_rays bit for bit against the oracle's march / getNormal and against the guide planes,
rmr_eval_map against the oracle's map, the device forms against the host forms (and so against the
oracle's trace), the GPU's ray check, and that nothing else moved.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle
from raymarchrenderer_amd import Renderer, RMRError, abi, check_rays

from .denoise_ref import far_hit_rule, oracle_normals
from .test_gpu_guides import _far_hit_case
from .test_gpu_parity import _tables, same_bits
from .test_gpu_rays import CORNELL, H, RECT, SCENE_CASES, TIMES, VIEW, W, _context, _oracle_trace, _ray_list

pytestmark = pytest.mark.gpu

CAST_SCENES = ["cornell5", "default", "csg_nodes", "csg64", "mandelbulb", "simple_rm2"]
TRACE_SCENES = ["cornell5", "csg64", "mandelbulb", "simple_rm2", "default_env"]
LENGTHS = (0, 1, 63, 64, 65)
MISS = np.array([0, 0, 0, -1], np.float32)


def _rays_of(name):
    """The 1,000-ray list test_gpu_rays traces for the scene (the same seed)."""
    path, variant, _ = SCENE_CASES[name]
    return _ray_list(_tables(path, variant), seed=sorted(SCENE_CASES).index(name))


def _march(tables, prm, rays):
    """oracle.march(tables, o, d, 1.0, prm) of every ray: (t, id) as march returns them."""
    L = oracle.lib()
    fp = C.POINTER(C.c_float)
    s = tables.to_ctypes()
    o = np.ascontiguousarray(rays["o"], np.float32)
    d = np.ascontiguousarray(rays["d"], np.float32)
    out = np.zeros((len(rays), 2), np.float32)
    for k in range(len(rays)):
        L.oracle_march(C.byref(s), C.byref(prm), o[k:k + 1].ctypes.data_as(fp), d[k:k + 1].ctypes.data_as(fp),
                       C.c_float(1.0), out[k:k + 1].ctypes.data_as(fp))
    return out[:, 0], out[:, 1]


def _map(tables, max_dist, pts):
    """oracle.map_p(tables, p, max_dist) of every point: (n, 2)."""
    L = oracle.lib()
    fp = C.POINTER(C.c_float)
    s = tables.to_ctypes()
    pts = np.ascontiguousarray(pts, np.float32)
    out = np.zeros((len(pts), 2), np.float32)
    for k in range(len(pts)):
        L.oracle_map(C.byref(s), C.c_float(max_dist), pts[k:k + 1].ctypes.data_as(fp), out[k:k + 1].ctypes.data_as(fp))
    return out


_march_cache = {}


def _oracle_cast(name):
    """The scene's rays and the oracle's raw march of each, once per scene."""
    if name not in _march_cache:
        path, variant, params = SCENE_CASES[name]
        rays = _rays_of(name)
        _march_cache[name] = (rays,) + _march(_tables(path, variant), abi.default_params(**params), rays)
    return _march_cache[name]


def _check_cast(hits, rays, tables, prm, t, ident, name, normals=True):
    """A cast's result against the oracle's raw march (t, ident) of the same rays."""
    want_id = far_hit_rule(t, ident, prm.max_dist)
    assert same_bits(hits["t"], t).all(), "%s: t differs at %s" % (name, np.flatnonzero(~same_bits(hits["t"], t))[:5])
    assert same_bits(hits["id"], want_id).all(), "%s: id differs" % name
    # pos = fma(d, t, o): one rounding of the exact value, so within 1 ulp of the float64 evaluation
    p64 = rays["o"].astype(np.float64) + rays["d"].astype(np.float64) * t[:, None].astype(np.float64)
    ulp = np.spacing(np.abs(p64.astype(np.float32))).astype(np.float64)
    assert (np.abs(hits["pos"].astype(np.float64) - p64) <= ulp).all(), name
    is_hit = want_id >= 0
    if normals:
        want_n = oracle_normals(tables, prm.max_dist, np.ascontiguousarray(hits["pos"]), is_hit)
        eq = same_bits(hits["n"], want_n).all(axis=-1)
        assert eq.all(), "%s: %d normals differ, first ray %d gpu %s cpu %s" % (
            name, (~eq).sum(), np.argmin(eq), hits["n"][np.argmin(eq)], want_n[np.argmin(eq)])
    else:
        assert (hits["n"].view(np.uint32) == 0).all()
    assert (hits["n"][~is_hit].view(np.uint32) == 0).all() and (hits["id"][~is_hit] == -1).all()
    return is_hit


# ---- 1. cast, bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", CAST_SCENES)
def test_cast_rays_bitexact(name):
    path, variant, params = SCENE_CASES[name]
    rays, t, ident = _oracle_cast(name)
    prm = abi.default_params(**params)
    tables = _tables(path, variant)
    # the list is not degenerate (the oracle alone decides this)
    want_id = far_hit_rule(t, ident, prm.max_dist)
    n_hit, n_miss = int(((want_id >= 0) & (t > 0)).sum()), int((want_id < 0).sum())
    print("%s: %d hits with t > 0, %d misses" % (name, n_hit, n_miss))
    assert n_hit >= 200 and n_miss >= 300
    r = _context(path, variant, params)
    try:
        hits = r.cast_rays(rays)
        assert hits.shape == (len(rays),) and hits.dtype == np.dtype(abi.HIT_DTYPE)
        _check_cast(hits, rays, tables, prm, t, ident, name)
        # the visibility form: the same march, no normal
        vis = r.cast_rays(rays, normals=False)
        _check_cast(vis, rays, tables, prm, t, ident, name + " (no normals)", normals=False)
        for k in ("t", "id", "pos"):
            assert vis[k].tobytes() == hits[k].tobytes(), k
        # prefixes of the same list, and capped grids (several strides per wave)
        for n in LENGTHS:
            assert r.cast_rays(rays[:n]).tobytes() == hits[:n].tobytes(), n
            assert r.cast_rays(rays[:n], normals=False).tobytes() == vis[:n].tobytes(), n
        for blocks in (1, 3):
            r.set_query_grid(blocks)
            assert r.cast_rays(rays).tobytes() == hits.tobytes(), blocks
            assert r.cast_rays(rays, normals=False).tobytes() == vis.tobytes(), blocks
            assert r.cast_rays(rays[:65]).tobytes() == hits[:65].tobytes(), blocks
        r.set_query_grid(0)
        assert r.query_rejects() == 0   # the host form's verdicts are not the device forms' counter
    finally:
        r.close()


@pytest.mark.parametrize("name", ["cornell5", "default"])
def test_cast_rays_zero_steps_all_miss(name):
    path, variant, params = SCENE_CASES[name]
    rays = _rays_of(name)
    r = _context(path, variant, dict(params, max_steps=0))
    try:
        hits = r.cast_rays(rays)
    finally:
        r.close()
    md = abi.default_params().max_dist
    assert (hits["t"] == md).all() and (hits["id"] == -1).all() and (hits["n"].view(np.uint32) == 0).all()
    p64 = rays["o"].astype(np.float64) + rays["d"].astype(np.float64) * md
    assert (np.abs(hits["pos"] - p64) <= np.spacing(np.abs(p64.astype(np.float32)))).all()


def _view_rays(view, dirs):
    """A ray list from one eye and (..., 3) float32 directions."""
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    rays = np.zeros(len(d), np.dtype(abi.RAY_DTYPE))
    rays["o"] = np.asarray(view, np.float32)[:3]
    rays["d"] = d
    return rays


@pytest.mark.parametrize("name", ["cornell5", "default"])
def test_cast_rays_far_hits(name):
    """step_multiply 1.7 overshoots into objects beyond a reduced max_dist: march returns those as hits at
    t >= max_dist; the cast shows them as misses that keep march's t."""
    path, variant, params = SCENE_CASES[name]
    tables = _tables(path, variant)
    view, prm = _far_hit_case(tables)
    r = _context(path, variant, params)
    try:
        r.set_params(prm)
        r.set_view(view)
        r.render_guides(RECT)
        dirs = r.read_guide("ray")[RECT[1]:RECT[3], RECT[0]:RECT[2], :3]
        rays = _view_rays(view, dirs)
        assert check_rays(rays)
        hits = r.cast_rays(rays)
    finally:
        r.close()
    t, ident = _march(tables, prm, rays)
    _check_cast(hits, rays, tables, prm, t, ident, name + " far")
    far = (ident >= 0) & (t >= prm.max_dist)
    n_hit, n_miss = ((ident >= 0) & (t < prm.max_dist)).sum(), (ident < 0).sum()
    print("far hits %d, hits %d, misses %d at max_dist %g" % (far.sum(), n_hit, n_miss, prm.max_dist))
    assert far.sum() >= 3 and n_hit >= 3 and n_miss >= 3
    assert (hits["id"][far] == -1).all() and (hits["t"][far] >= prm.max_dist).all()
    assert (hits["n"][far].view(np.uint32) == 0).all()


def test_cast_rays_are_the_guide_planes():
    """GPU against GPU: casting (eye, the guide pass's directions) over the image gives its HIT and NORMAL
    planes bit for bit."""
    r = _context(*SCENE_CASES["cornell5"])
    try:
        r.render_guides()
        g = r.read_guides()
        hits = r.cast_rays(_view_rays(VIEW, g["ray"][..., :3])).reshape(H, W)
        vis = r.cast_rays(_view_rays(VIEW, g["ray"][..., :3]), normals=False).reshape(H, W)
    finally:
        r.close()
    assert (g["normal"][..., 3] >= 0).sum() > 100 and (g["normal"][..., 3] < 0).sum() > 100
    assert same_bits(hits["pos"], g["hit"][..., :3]).all() and same_bits(hits["t"], g["hit"][..., 3]).all()
    assert same_bits(hits["n"], g["normal"][..., :3]).all() and same_bits(hits["id"], g["normal"][..., 3]).all()
    assert same_bits(vis["id"], g["normal"][..., 3]).all() and same_bits(vis["t"], g["hit"][..., 3]).all()


# ---- 2. eval ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CAST_SCENES)
def test_eval_map_bitexact(name):
    path, variant, params = SCENE_CASES[name]
    rays = _rays_of(name)
    prm = abi.default_params(**params)
    tables = _tables(path, variant)
    r = _context(path, variant, params)
    try:
        hits = r.cast_rays(rays, normals=False)
        far = (np.random.default_rng(11).uniform(-1.0, 1.0, (16, 3)) * 1e6).astype(np.float32)
        pts = np.concatenate([rays["o"], hits["pos"], far]).astype(np.float32)
        got = r.eval_map(pts)
        assert got.shape == (len(pts), 2) and got.dtype == np.float32
        want = _map(tables, prm.max_dist, pts)
        eq = same_bits(got, want).all(axis=1)
        assert eq.all(), "%s: %d points differ; first %d: p %s gpu %s oracle %s" % (
            name, (~eq).sum(), np.argmin(eq), pts[np.argmin(eq)], got[np.argmin(eq)], want[np.argmin(eq)])
        # both sides of the surface and the empty start value occur
        assert (want[:, 0] < 0.001).sum() >= 100 and (want[:, 0] > 0.001).sum() >= 100
        assert (want[-16:, 0] == prm.max_dist).all() and (want[-16:, 1] == -1).all()
        for n in LENGTHS:
            assert r.eval_map(pts[:n]).tobytes() == got[:n].tobytes(), n
        for blocks in (1, 3):
            r.set_query_grid(blocks)
            assert r.eval_map(pts).tobytes() == got.tobytes(), blocks
            assert r.eval_map(pts[:65]).tobytes() == got[:65].tobytes(), blocks
    finally:
        r.close()


# ---- 3. the device forms ----------------------------------------------------------------------------
def _torch_rays(torch, rays, as_float=False):
    flat = np.ascontiguousarray(rays).reshape(-1)
    if as_float:
        return torch.from_numpy(flat.view(np.float32).reshape(len(flat), 10).copy()).cuda()
    return torch.from_numpy(flat.view(np.uint8).reshape(len(flat), 40).copy()).cuda()


def _extent(rays):
    return float(np.abs(rays["o"]).max()) if len(rays) else 0.0


@pytest.mark.parametrize("jit", [0, 1], ids=["table", "jit"])
@pytest.mark.parametrize("name", TRACE_SCENES)
def test_trace_rays_device_is_the_host_form(name, jit):
    import torch
    path, variant, params = SCENE_CASES[name]
    bounces = abi.default_params(**params).max_bounces
    rays, want = _oracle_trace(name, bounces)
    ext = _extent(rays)
    r = _context(path, variant, params, jit)
    try:
        host = r.trace_rays(rays)
        assert same_bits(host[:, :3], want).all()
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            r.set_stream(torch.cuda.current_stream().cuda_stream)
            d_rays = _torch_rays(torch, rays)
            before = r.read_accum()
            n0 = r.stats().trace_launches
            out = r.trace_rays_device(d_rays, ext)
            assert out.is_cuda and out.shape == (len(rays), 4) and out.dtype == torch.float32
            got = out.cpu().numpy()
            assert same_bits(got, host).all(), "%s jit %d: %d rays differ" % (name, jit, (~same_bits(got, host).all(axis=1)).sum())
            assert r.stats().trace_launches - n0 == 1
            # a looser bound on the origins, the (n, 10) float32 view, a caller's output tensor
            buf = torch.full((len(rays), 4), 7.0, dtype=torch.float32, device="cuda")
            assert r.trace_rays_device(_torch_rays(torch, rays, as_float=True), 10.0 * ext, out=buf) is buf
            assert same_bits(buf.cpu().numpy(), host).all(), "10 x extent"
            for n in (0, 1, 65):
                assert same_bits(r.trace_rays_device(d_rays[:n].contiguous(), ext).cpu().numpy(), host[:n]).all(), n
            # the plane budget cuts the list into launches of 256 rays
            r.set_tuning(samp_budget=256 * 64)
            n1 = r.stats().trace_launches
            cut = r.trace_rays_device(d_rays, ext).cpu().numpy()
            assert r.stats().trace_launches - n1 == 4
            assert same_bits(cut, host).all(), "4 launches"
            st = r.stats()
            assert st.jit_launches == (st.trace_launches if jit else 0)
            assert r.query_rejects() == 0
            assert same_bits(r.read_accum(), before).all()
    finally:
        r.close()
    assert same_bits(got[:, :3], want).all() and (got[:, 3] == 1).all()


@pytest.mark.parametrize("name", ["cornell5", "csg64", "csg_nodes"])
def test_cast_and_eval_device_are_the_host_forms(name):
    import torch
    path, variant, params = SCENE_CASES[name]
    rays = _rays_of(name)
    r = _context(path, variant, params)
    try:
        hits = r.cast_rays(rays)
        vis = r.cast_rays(rays, normals=False)
        pts = np.concatenate([rays["o"], hits["pos"]]).astype(np.float32)
        dist = r.eval_map(pts)
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            r.set_stream(torch.cuda.current_stream().cuda_stream)
            d_rays = _torch_rays(torch, rays)
            got = r.cast_rays_device(d_rays)
            assert got.is_cuda and got.shape == (len(rays), 8)
            assert got.cpu().numpy().tobytes() == hits.tobytes()
            assert r.cast_rays_device(_torch_rays(torch, rays, as_float=True), normals=False).cpu().numpy().tobytes() == vis.tobytes()
            d_pts = torch.from_numpy(pts).cuda()
            buf = torch.empty((len(pts), 2), dtype=torch.float32, device="cuda")
            assert r.eval_map_device(d_pts, out=buf) is buf
            assert buf.cpu().numpy().tobytes() == dist.tobytes()
            for blocks in (1, 3):
                r.set_query_grid(blocks)
                assert r.cast_rays_device(d_rays).cpu().numpy().tobytes() == hits.tobytes(), blocks
                assert r.eval_map_device(d_pts).cpu().numpy().tobytes() == dist.tobytes(), blocks
            r.set_query_grid(0)
            for n in LENGTHS:
                assert r.cast_rays_device(d_rays[:n].contiguous()).cpu().numpy().tobytes() == hits[:n].tobytes(), n
                assert r.eval_map_device(d_pts[:n].contiguous()).cpu().numpy().tobytes() == dist[:n].tobytes(), n
            assert r.query_rejects() == 0
    finally:
        r.close()


@pytest.mark.parametrize("jit", [0, 1], ids=["table", "jit"])
def test_device_forms_reject_on_the_gpu(jit):
    import torch
    path, variant, params = SCENE_CASES["cornell5"]
    rays = _rays_of("cornell5")
    ext = _extent(rays)
    bad = rays.copy()
    bad["o"][5, 1] = np.nan                      # a NaN origin
    bad["d"][70] *= np.float32(1.01)             # not a unit direction
    bad["gx"][200] = 2 ** 24                     # gx + time would round twice
    bad["o"][333] = (0.0, -4.0 * ext, 0.0)       # a fine ray, but beyond origin_extent
    rule, beyond = [5, 70, 200], [333]
    assert check_rays(rays) and not check_rays(bad) and check_rays(bad[201:])
    r = _context(path, variant, params, jit)
    try:
        host_rgba, host_hits = r.trace_rays(rays), r.cast_rays(rays)
        far_hit = r.cast_rays(bad[333:334])      # (the cast has no extent rule)
        for call in (r.trace_rays, r.cast_rays):
            with pytest.raises(RMRError) as e:   # the host forms name the first of the three
                call(bad)
            assert e.value.code == -1 and "ray 5 " in str(e.value)
        with pytest.raises(RMRError) as e:
            r.cast_rays(bad[6:], normals=False)
        assert e.value.code == -1 and "ray 64 " in str(e.value)
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            r.set_stream(torch.cuda.current_stream().cuda_stream)
            d_bad = _torch_rays(torch, bad)
            assert r.query_rejects() == 0
            rgba = r.trace_rays_device(d_bad, ext).cpu().numpy()
            assert r.query_rejects() == 4 and r.query_rejects() == 0
            rejected = np.zeros(len(rays), bool)
            rejected[rule + beyond] = True
            assert (rgba[rejected].view(np.uint32) == 0).all()
            assert same_bits(rgba[~rejected], host_rgba[~rejected]).all() and (rgba[~rejected, 3] == 1).all()
            # cut into 4 launches: every ray is checked once
            r.set_tuning(samp_budget=256 * 64)
            cut = r.trace_rays_device(d_bad, ext).cpu().numpy()
            assert r.query_rejects() == 4
            assert cut.tobytes() == rgba.tobytes()
            # a bound that covers ray 333 accepts it
            wide = r.trace_rays_device(d_bad, 4.0 * ext).cpu().numpy()
            assert r.query_rejects() == 3 and wide[333, 3] == 1
            hits = r.cast_rays_device(d_bad).cpu().numpy().view(np.dtype(abi.HIT_DTYPE)).reshape(-1)
            assert r.query_rejects() == 3 and r.query_rejects() == 0
            rejected[beyond] = False
            assert (hits["pos"][rejected] == 0).all() and (hits["n"][rejected] == 0).all()
            assert (hits["t"][rejected] == -1).all() and (hits["id"][rejected] == -2).all()
            keep = ~rejected
            keep[beyond] = False
            assert hits[keep].tobytes() == host_hits[keep].tobytes()
            assert hits[333:334].tobytes() == far_hit.tobytes()
    finally:
        r.close()


# ---- 4. nothing else moved --------------------------------------------------------------------------
def test_queries_leave_the_images_alone():
    import torch
    rays = _rays_of("cornell5")
    ext = _extent(rays)
    r = _context(*SCENE_CASES["cornell5"])
    fresh = _context(*SCENE_CASES["cornell5"])
    try:
        r.set_error_estimate(True)
        r.render_spp(TIMES, RECT)
        r.render_guides()
        dn = r.denoise(iterations=2)
        state = (r.read_accum(), r.read_half(), r.tile_error(), r.read_guides())

        def unchanged(what):
            assert same_bits(r.read_accum(), state[0]).all() and same_bits(r.read_half(), state[1]).all(), what
            assert same_bits(r.tile_error(), state[2]).all(), what
            assert same_bits(r.read_denoised(), dn).all(), what
            for k, g in r.read_guides().items():
                assert same_bits(g, state[3][k]).all(), (what, k)

        hits = r.cast_rays(rays)
        unchanged("cast_rays")
        r.eval_map(hits["pos"])
        unchanged("eval_map")
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            r.set_stream(torch.cuda.current_stream().cuda_stream)
            d_rays = _torch_rays(torch, rays)
            r.trace_rays_device(d_rays, ext)
            unchanged("trace_rays_device")
            r.cast_rays_device(d_rays)
            unchanged("cast_rays_device")
            r.eval_map_device(torch.from_numpy(np.ascontiguousarray(hits["pos"])).cuda())
            unchanged("eval_map_device")
            assert r.query_rejects() == 0
            unchanged("query_rejects")
            # the next launch finds a clean work queue: the same bits as a context that made no query
            r.render_spp(TIMES[:1], RECT, first_sample=4)
            got = r.read_accum()
        fresh.set_error_estimate(True)
        fresh.render_spp(TIMES, RECT)
        fresh.render_spp(TIMES[:1], RECT, first_sample=4)
        assert same_bits(got, fresh.read_accum()).all() and not same_bits(got, state[0]).all()
    finally:
        r.close()
        fresh.close()


def test_query_error_returns():
    import torch
    rays = _rays_of("cornell5")
    r = Renderer(0, W, H)
    try:
        d_rays = _torch_rays(torch, rays[:70])
        d_pts = torch.zeros((4, 3), dtype=torch.float32, device="cuda")
        for call in (lambda: r.cast_rays(rays[:3]), lambda: r.eval_map(rays["o"][:3]),
                     lambda: r.trace_rays_device(d_rays, 100.0), lambda: r.cast_rays_device(d_rays),
                     lambda: r.eval_map_device(d_pts)):
            with pytest.raises(RMRError) as e:
                call()
            assert e.value.code == -5                              # no scene
        r.load_scene(CORNELL, "rm1")
        r.set_view(VIEW)
        r.set_params(abi.default_params(max_bounces=2))
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(RMRError) as e:
                r.trace_rays_device(d_rays, bad)
            assert e.value.code == -1                              # the extent: finite and >= 0
        assert r.trace_rays_device(d_rays, 0.0).shape == (70, 4)   # 0 is a bound (it rejects what lies beyond)
        assert r.query_rejects() == int((np.abs(rays["o"][:70]).max(axis=1) > 0).sum())
        bad = rays[:70].copy()
        bad["d"][69] *= np.float32(1.01)
        with pytest.raises(RMRError) as e:
            r.cast_rays(bad)
        assert e.value.code == -1 and "69" in str(e.value)
        assert r.cast_rays(bad[:69]).shape == (69,)                # the call after a refused one is fine
        with pytest.raises(RMRError) as e:
            r._chk(r.lib.rmr_cast_rays_device(r.ctx, d_rays.data_ptr(), 70, 2, d_rays.data_ptr()))
        assert e.value.code == -1                                  # unknown flags
        with pytest.raises(RMRError):
            r.set_query_grid(-1)
        for wrong in (torch.zeros((70, 39), dtype=torch.uint8, device="cuda"), torch.zeros((70, 10), dtype=torch.float32)):
            with pytest.raises(ValueError):
                r.cast_rays_device(wrong)
        r.set_params(abi.default_params(separate_channels=1))
        with pytest.raises(RMRError) as e:
            r.trace_rays_device(d_rays, 100.0)
        assert e.value.code == -5                                  # separateChannels
        assert r.cast_rays_device(d_rays).shape == (70, 8)         # (the geometry queries have no channels)
        r.sync()
    finally:
        r.close()
