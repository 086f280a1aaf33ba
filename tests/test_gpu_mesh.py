"""SDF volume sampling and surface-nets extraction on the GPU (include/rmr.h): the volume bit
for bit against the oracle's map for every map class, the mesh against the NumPy statement tests/mesh_ref.py on
the oracle's volume (topology exactly, positions within the bound counted there), normals and ids bit for bit
against the oracle at the GPU's own vertices, a lattice that needs more than one scan workgroup, determinism,
that nothing else moved, the errors, and rmr_cli --mesh."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from raymarchrenderer_amd import Renderer, RMRError, abi

from . import mesh_ref as ref
from . import node_family as nf
from .conftest import SCENES
from .denoise_ref import oracle_normals
from .test_gpu_parity import _tables, same_bits
from .test_gpu_query import _map
from .test_gpu_rays import CLI, H, SCENE_CASES, TIMES, VIEW, W, _context
from .test_mesh_cpu import _parse_obj

pytestmark = pytest.mark.gpu

F = np.float32
# 23 x 19 x 29 = 12,673 points: more than one block, not a multiple of 64; 0.3 is not a float32 number
VOLUME = ((-3.1, -1.2, -4.05), 0.3, (23, 19, 29))
VOLUME_SCENES = ["cornell5", "default", "csg_nodes", "csg64", "mandelbulb", "simple_rm2", "nf:nan_objects"]
SPHERE1 = os.path.join(SCENES, "sphere1.scene")


def _scene_context(name):
    """A context with the scene, its oracle tables and its maxDist; name: of SCENE_CASES, or nf:<case>."""
    if name.startswith("nf:"):
        r = Renderer(0, W, H)
        r.load_scene(nf.scene(name[3:]), "rm1")
        r.set_params(nf.params())
        return r, nf.tables(name[3:]), nf.params().max_dist
    path, variant, params = SCENE_CASES[name]
    return _context(path, variant, params), _tables(path, variant), abi.default_params(**params).max_dist


def _case_context(name):
    """A context with the scene of a lattice case of mesh_ref.CASES (default params: maxDist 1000)."""
    r = Renderer(0, W, H)
    r.load_scene(ref.case_scene(name)[0], "rm1")
    return r


# ---- 1. the volume, bit for bit -----------------------------------------------------------------------------
def test_lattice_coordinates_are_two_roundings():
    """The statement the volume tests rely on: at this lattice the two-rounding coordinates differ from the
    fused and from the float64-then-rounded ones, so a kernel that computed those would fail below."""
    origin, spacing, shape = VOLUME
    two = ref.lattice_coords(origin, spacing, shape)
    differs_fused = differs_f64 = 0
    for a in range(3):
        i = np.arange(shape[a], dtype=np.float64)
        fused = (float(F(origin[a])) + i * float(F(spacing))).astype(F)   # one rounding of the exact value
        differs_fused += int((fused != two[a]).sum())
        differs_f64 += int(((origin[a] + i * spacing).astype(F) != two[a]).sum())
    assert differs_fused >= 3 and differs_f64 >= 3


@pytest.mark.parametrize("name", VOLUME_SCENES)
def test_volume_bitexact(name):
    origin, spacing, shape = VOLUME
    r, tables, max_dist = _scene_context(name)
    try:
        dist, ids = r.sample_volume(origin, spacing, shape, ids=True)
        want_d, want_i = ref.oracle_volume(tables, origin, spacing, shape, max_dist)
        assert dist.shape == (shape[2], shape[1], shape[0]) and dist.dtype == F and ids.shape == dist.shape
        eq_d, eq_i = same_bits(dist, want_d), same_bits(ids, want_i)
        assert eq_d.all(), "%s: %d distances differ, first at %s" % (name, (~eq_d).sum(), np.argwhere(~eq_d)[0])
        assert eq_i.all(), "%s: %d ids differ" % (name, (~eq_i).sum())
        print("%s: %d inside, %d NaN, ids %s" % (name, (want_d < 0).sum(), np.isnan(want_d).sum(), np.unique(want_i)))
        assert (want_d < 0).any() and (want_d > 0).any()
        # the coordinates: the existing point query at the two-rounding points gives the same bytes
        pts = ref.lattice_points(origin, spacing, shape)
        assert r.eval_map(pts)[:, 0].tobytes() == dist.tobytes()
        # without ids, capped grids (several strides per thread), and the device form
        assert r.sample_volume(origin, spacing, shape).tobytes() == dist.tobytes()
        for blocks in (1, 3):
            r.set_query_grid(blocks)
            d2, i2 = r.sample_volume(origin, spacing, shape, ids=True)
            assert d2.tobytes() == dist.tobytes() and i2.tobytes() == ids.tobytes(), blocks
        r.set_query_grid(0)
        dd, di = r.sample_volume_device(origin, spacing, shape, ids=True)
        d1 = r.sample_volume_device(origin, spacing, shape)
        r.sync()
        assert dd.is_cuda and tuple(dd.shape) == dist.shape
        assert dd.cpu().numpy().tobytes() == dist.tobytes() and di.cpu().numpy().tobytes() == ids.tobytes()
        assert d1.cpu().numpy().tobytes() == dist.tobytes()
    finally:
        r.close()


# ---- 2. the mesh against the statement ------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_mesh_matches_statement(name):
    _, origin, spacing, shape, iso = ref.CASES[name]
    r = _case_context(name)
    try:
        # the GPU's own volume is the oracle's, so the statement on the oracle's volume is the GPU's reference
        assert same_bits(r.sample_volume(origin, spacing, shape), ref.case_volume(name)).all()
        m = r.extract_mesh(origin, spacing, shape, iso=iso, normals=False, ids=False)
    finally:
        r.close()
    want = ref.case_ref(name)
    assert m["vertices"].dtype == F and m["quads"].dtype == np.uint32 and m["normals"] is None and m["ids"] is None
    ref.compare(m["vertices"], m["quads"], want, spacing, name)
    if name in ("sphere_empty", "sphere_full"):
        assert m["vertices"].shape == (0, 3) and m["quads"].shape == (0, 4)
    if name == "sphere_iso":
        assert np.abs(np.linalg.norm(m["vertices"] - [0.0, 1.0, 0.0], axis=1) - 1.25).max() <= spacing / 2


# ---- 3. normals and ids at the GPU's own vertices ---------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere_cut", "cornell5", "csg_nodes", "nan_objects"])
def test_normals_and_ids_bitexact(name):
    _, origin, spacing, shape, iso = ref.CASES[name]
    tables = ref.case_scene(name)[1]
    r = _case_context(name)
    try:
        m = r.extract_mesh(origin, spacing, shape, iso=iso)
        only_n = r.extract_mesh(origin, spacing, shape, iso=iso, normals=True, ids=False)
        only_i = r.extract_mesh(origin, spacing, shape, iso=iso, normals=False, ids=True)
    finally:
        r.close()
    v = np.ascontiguousarray(m["vertices"])
    assert len(v) > 40 and len(v) % 64 != 0   # the last wave of the attribute kernel is partly empty
    want_n = oracle_normals(tables, ref.MAX_DIST, v, np.ones(len(v), bool))
    want_i = _map(tables, ref.MAX_DIST, v)[:, 1]
    eq = same_bits(m["normals"], want_n).all(axis=-1)
    assert eq.all(), "%s: %d normals differ, first vertex %d gpu %s cpu %s" % (
        name, (~eq).sum(), np.argmin(eq), m["normals"][np.argmin(eq)], want_n[np.argmin(eq)])
    assert same_bits(m["ids"], want_i).all()
    assert len(np.unique(want_i)) >= (1 if name.startswith("sphere") else 2)
    # each attribute alone
    assert only_n["ids"] is None and only_n["normals"].tobytes() == m["normals"].tobytes()
    assert only_i["normals"] is None and only_i["ids"].tobytes() == m["ids"].tobytes()
    assert only_n["vertices"].tobytes() == v.tobytes() and only_i["quads"].tobytes() == m["quads"].tobytes()


# ---- 4. a lattice that outgrows one scan workgroup ----------------------------------------------------------
def test_lattice_beyond_one_scan_workgroup():
    """rmr_volume.hip: kMeshBlock = 256 points per block, kScanGroup = 1024 block totals per k_mesh_scan1
    workgroup, so one workgroup holds the scan up to 262,144 points. 65 x 64 x 64 would pass that, but only with
    points of its last z layer, which hold no cell and no emitting edge: its second group's totals are all zero.
    64 x 64 x 88 = 360,448 points are 1,408 blocks in two scan groups, the boundary (point 262,144) is the layer
    iz = 64 at z = 0.1, through the middle of the sphere, so vertices and quads lie on both sides of it and the
    second group's base is not zero. The second level (k_mesh_scan2) is one workgroup in which a thread takes
    ceil(groups / 256) consecutive groups: it has one path for every lattice rmr_check_volume accepts (at most
    4,096 groups), so there is no further size at which it changes. The reference volume is rmr_eval_map's
    over the same points (pinned to the oracle by test_gpu_query)."""
    origin, spacing, shape = (-1.6, -0.6, -3.1), 0.05, (64, 64, 88)
    boundary = 256 * 1024
    assert shape[0] * shape[1] * shape[2] > boundary
    r = Renderer(0, W, H)
    try:
        r.load_scene(SPHERE1, "rm1")
        pts = ref.lattice_points(origin, spacing, shape)
        vol = r.eval_map(pts)[:, 0].reshape(pts.shape[:3])
        assert r.sample_volume(origin, spacing, shape).tobytes() == vol.tobytes()
        m = r.extract_mesh(origin, spacing, shape, normals=False, ids=False)
    finally:
        r.close()
    want = ref.surface_nets(vol, origin, spacing, 0.0)
    ref.compare(m["vertices"], m["quads"], want, spacing, "64x64x88")
    c = want["cells"]
    cell_point = c % 63 + 64 * (c // 63 % 63 + 64 * (c // (63 * 63)))   # a cell's lower point's linear index
    assert (cell_point < boundary).sum() > 1000 and (cell_point >= boundary).sum() > 1000
    assert ref.euler_number(len(m["vertices"]), m["quads"]) == 2


# ---- 5. determinism -------------------------------------------------------------------------------------------
def test_two_extractions_give_the_same_bytes():
    _, origin, spacing, shape, iso = ref.CASES["csg_nodes"]
    r = _case_context("csg_nodes")
    try:
        a = r.extract_mesh(origin, spacing, shape)
        dev = r.mesh_device()
        r.sync()
        for k in ("vertices", "normals", "ids"):
            assert dev[k].is_cuda and dev[k].cpu().numpy().tobytes() == a[k].tobytes(), k
        assert dev["quads"].cpu().numpy().view(np.uint32).tobytes() == a["quads"].tobytes()
        del dev
        other = r.extract_mesh((0.0, 0.0, 0.0), 0.5, (4, 5, 6))   # a different lattice in between
        assert len(other["vertices"]) != len(a["vertices"])
        b = r.extract_mesh(origin, spacing, shape)
        again = r.read_mesh()
    finally:
        r.close()
    for k in ("vertices", "normals", "ids", "quads"):
        assert a[k].tobytes() == b[k].tobytes() == again[k].tobytes(), k


# ---- 6. nothing else moved -------------------------------------------------------------------------------------
def test_extraction_leaves_everything_else_alone():
    import torch
    rect = (3, 2, 41, 35)
    _, origin, spacing, shape, iso = ref.CASES["cornell5"]
    r = _context(*SCENE_CASES["cornell5"])
    fresh = _context(*SCENE_CASES["cornell5"])
    try:
        r.set_error_estimate(True)
        r.render_spp(TIMES, rect)
        r.render_guides()
        dn = r.denoise(iterations=2)
        r.tonemap("denoised", curve="aces")
        tm = r.read_tonemapped()
        r.render_aov(TIMES)
        aov = r.read_aov()
        bad = np.zeros(3, np.dtype(abi.RAY_DTYPE))
        bad["d"][:, 2] = 1.0
        bad["d"][1] = np.nan   # one ray the GPU's check rejects
        r.cast_rays_device(torch.from_numpy(bad.view(np.uint8).reshape(3, 40)).cuda())
        state = (r.read_accum(), r.read_half(), r.tile_error(), r.read_guides())

        def unchanged(what):
            assert same_bits(r.read_accum(), state[0]).all() and same_bits(r.read_half(), state[1]).all(), what
            assert same_bits(r.tile_error(), state[2]).all(), what
            assert same_bits(r.read_denoised(), dn).all() and same_bits(r.read_tonemapped(), tm).all(), what
            for k, g in r.read_guides().items():
                assert same_bits(g, state[3][k]).all(), (what, k)
            for k, g in r.read_aov().items():
                assert same_bits(g, aov[k]).all(), (what, k)

        r.sample_volume(origin, spacing, shape, ids=True)
        unchanged("sample_volume")
        m = r.extract_mesh(origin, spacing, shape)
        unchanged("extract_mesh")
        assert r.query_rejects() == 1
        # a view change, a parameter change and a render keep the mesh
        r.set_view(VIEW)
        r.set_params(abi.default_params(max_bounces=4))
        r.render_spp(TIMES[:1], rect, first_sample=4)
        again = r.read_mesh()
        for k in m:
            assert again[k].tobytes() == m[k].tobytes(), k
        # that render found a clean work queue: the same bits as a context that never extracted
        got = r.read_accum()
        fresh.set_error_estimate(True)
        fresh.render_spp(TIMES, rect)
        fresh.render_spp(TIMES[:1], rect, first_sample=4)
        assert same_bits(got, fresh.read_accum()).all() and not same_bits(got, state[0]).all()
    finally:
        r.close()
        fresh.close()


# ---- 7. errors ---------------------------------------------------------------------------------------------------
def test_state_and_errors():
    _, origin, spacing, shape, iso = ref.CASES["sphere_cut"]
    r = Renderer(0, W, H)
    try:
        def code(call):
            with pytest.raises(RMRError) as e:
                call()
            return e.value.code

        assert code(lambda: r.sample_volume(origin, spacing, shape)) == -5       # no scene
        assert code(lambda: r.sample_volume_device(origin, spacing, shape)) == -5
        assert code(lambda: r.extract_mesh(origin, spacing, shape)) == -5
        assert code(r.read_mesh) == -5 and code(r.mesh_device) == -5
        r.load_scene(SPHERE1, "rm1")
        assert code(r.read_mesh) == -5                                           # before an extraction
        # a bad descriptor, through the library itself: the field is named
        info, mp = abi.MeshInfo(), abi.MeshParams(0.0, 0)
        out = np.zeros(8, F)
        fp = out.ctypes.data_as(C.POINTER(C.c_float))
        for field, d in (("origin", abi.volume_desc((0, np.nan, 0), 0.5, (2, 2, 2))),
                         ("spacing", abi.volume_desc((0, 0, 0), 0.0, (2, 2, 2))),
                         ("n", abi.volume_desc((0, 0, 0), 0.5, (2, 1, 2))),
                         ("points", abi.volume_desc((0, 0, 0), 0.5, (4096, 4096, 65)))):
            assert r.lib.rmr_extract_mesh(r.ctx, C.byref(d), C.byref(mp), C.byref(info)) == -1
            assert ("'%s'" % field) in r.lib.rmr_last_error(r.ctx).decode()
            assert r.lib.rmr_sample_volume(r.ctx, C.byref(d), fp, None) == -1
            assert r.lib.rmr_sample_volume_device(r.ctx, C.byref(d), 1, None) == -1
        assert code(lambda: r.extract_mesh(origin, -1.0, shape)) == -1
        good = abi.volume_desc(origin, spacing, shape)
        for bad_mp in (abi.MeshParams(np.nan, 0), abi.MeshParams(np.inf, 0), abi.MeshParams(0.0, 4)):
            assert r.lib.rmr_extract_mesh(r.ctx, C.byref(good), C.byref(bad_mp), C.byref(info)) == -1
        assert code(r.read_mesh) == -5                                           # a failed extraction leaves no mesh
        # attributes that were not extracted
        m = r.extract_mesh(origin, spacing, shape, normals=False, ids=False)
        assert len(m["vertices"]) == len(ref.case_ref("sphere_cut")["vertices"])
        assert code(lambda: r.read_mesh(normals=True, ids=False)) == -5
        assert code(lambda: r.read_mesh(normals=False, ids=True)) == -5
        assert r.read_mesh(normals=False, ids=False)["quads"].tobytes() == m["quads"].tobytes()
        assert not r.lib.rmr_mesh_device_ptr(r.ctx, abi.MESH_BUF_NORMALS) and not r.lib.rmr_mesh_device_ptr(r.ctx, 7)
        assert r.lib.rmr_mesh_device_ptr(r.ctx, abi.MESH_BUF_VERTICES) and r.lib.rmr_mesh_device_ptr(r.ctx, abi.MESH_BUF_QUADS)
        # a failed extraction drops the mesh that was there
        bad = abi.volume_desc(origin, spacing, (1, 2, 3))
        assert r.lib.rmr_extract_mesh(r.ctx, C.byref(bad), C.byref(mp), C.byref(info)) == -1
        assert code(lambda: r.read_mesh(normals=False, ids=False)) == -5
        assert not r.lib.rmr_mesh_device_ptr(r.ctx, abi.MESH_BUF_VERTICES)
        r.extract_mesh(origin, spacing, shape)
        # mesh_free and reload
        r.mesh_free()
        assert code(r.read_mesh) == -5 and not r.lib.rmr_mesh_device_ptr(r.ctx, abi.MESH_BUF_VERTICES)
        r.mesh_free()                                                            # nothing to do
        full = r.extract_mesh(origin, spacing, shape)
        r.reload()
        assert code(r.read_mesh) == -5 and code(r.mesh_device) == -5
        assert r.extract_mesh(origin, spacing, shape)["normals"].tobytes() == full["normals"].tobytes()
        # an empty mesh is a mesh
        e = r.extract_mesh((5.0, 5.0, 5.0), 0.05, (5, 5, 5))
        assert e["vertices"].shape == (0, 3) and e["quads"].shape == (0, 4) and e["ids"].shape == (0,)
        assert r.read_mesh()["normals"].shape == (0, 3) and r.mesh_device()["quads"].shape == (0, 4)
    finally:
        r.close()


# ---- 8. rmr_cli ----------------------------------------------------------------------------------------------------
def test_cli_mesh(tmp_path):
    """rmr_cli --mesh at a 16-cell grid on sphere1 writes an OBJ whose v / vn / f equal extract_mesh's on the
    lattice the options describe (spacing 3 / 16, 17^3 points), and a PLY with the same arrays."""
    out, obj, ply = str(tmp_path / "cli.bmp"), str(tmp_path / "m.obj"), str(tmp_path / "m.ply")
    base = [CLI, "--scene", SPHERE1, "--variant", "rm1", "--size", "16x16", "--samples", "1", "--grid", "1x1",
            "--out", out, "--quiet", "--mesh-bounds", "-1.5,-0.5,-1.5,1.5,2.5,1.5", "--mesh-grid", "16"]
    p = subprocess.run(base + ["--mesh", obj], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    _, origin, spacing, shape, iso = ref.CASES["sphere17"]
    r = _case_context("sphere17")
    try:
        m = r.extract_mesh(origin, spacing, shape)
        grown = r.extract_mesh(origin, spacing, shape, iso=0.25)
    finally:
        r.close()
    v, vn, f = _parse_obj(obj)
    assert v.tobytes() == m["vertices"].tobytes() and vn.tobytes() == m["normals"].tobytes()
    assert (np.array([[c[0] for c in face] for face in f]) == m["quads"].astype(np.int64) + 1).all()
    assert all(c[0] == c[2] for face in f for c in face)
    ref.compare(v, np.array([[c[0] - 1 for c in face] for face in f]), ref.case_ref("sphere17"), spacing, "rmr_cli --mesh")
    from .test_mesh_cpu import _parse_ply
    p = subprocess.run(base + ["--mesh", ply, "--mesh-iso", "0.25"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    props, vert, face = _parse_ply(ply)
    assert props == ["x", "y", "z", "nx", "ny", "nz", "material"]
    assert vert[:, :3].tobytes() == grown["vertices"].tobytes() and vert[:, 3:6].tobytes() == grown["normals"].tobytes()
    assert (vert[:, 6] == grown["ids"]).all() and (face["i"] == grown["quads"]).all()
    # the option errors end with status 2 before any device work
    for bad in (["--mesh", obj], ["--mesh", obj, "--mesh-bounds", "0,0,0,1,1"], ["--mesh", str(tmp_path / "m.stl"), "--mesh-bounds", "0,0,0,1,1,1"]):
        assert subprocess.run([CLI, "--size", "8x8"] + bad, capture_output=True, text=True, timeout=60).returncode == 2, bad
