"""SDF volume sampling and surface-nets extraction (include/rmr.h) without a GPU: the NumPy
statement tests/mesh_ref.py on the oracle's volumes (what a closed and what a cut-open mesh is), the host
function rmr_surface_nets through the stand-alone program csrc/mesh_test.cpp against it (topology exactly,
positions within the bound counted in mesh_ref.py), the program's own checks plain and under the sanitizers,
rmr_check_volume field by field, the OBJ and PLY writers read back, the kernels' resources as compiled for
gfx950 (not run) and rmr_cli's argument handling."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from raymarchrenderer_amd import (RMRError, abi, check_volume, encode_obj, encode_ply, quads_to_triangles,
                                  surface_nets)

from . import mesh_ref as ref
from .conftest import ROOT

CSRC = os.path.join(ROOT, "raymarchrenderer_amd", "csrc")
CLI = os.path.join(ROOT, "raymarchrenderer_amd", "rmr_cli")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
F = np.float32
RULE_CASES = ["sphere17", "sphere_cut", "sphere_iso", "cornell5", "csg_nodes", "nan_objects"]


# ---- the statement on the oracle's volumes ----------------------------------------------------------------
def test_reference_closed_sphere():
    """The unit sphere inside a 17^3 lattice: a closed, outward-oriented surface near the sphere."""
    _, origin, spacing, shape, _ = ref.CASES["sphere17"]
    m = ref.case_ref("sphere17")
    v, q = m["vertices"], m["quads"]
    (dk, dc), (uk, uc) = ref.edge_census(q)
    assert (uc == 2).all()                       # every undirected edge is shared by exactly two quads
    assert (dc == 1).all()                       # every directed edge occurs once
    assert ref.euler_number(len(v), q) == 2      # V - E + F
    vol = ref.signed_volume(v, q)
    worst = float(np.abs(np.linalg.norm(v - [0.0, 1.0, 0.0], axis=1) - 1.0).max())
    print("sphere17: %d vertices, %d quads, volume %.3f, worst |r - 1| %.4f = %.3f of the spacing"
          % (len(v), len(q), vol, worst, worst / spacing))
    assert vol > 0.0
    assert worst <= spacing / 2
    assert (m["cells"][1:] > m["cells"][:-1]).all() and (m["crossings"] >= 3).all()


def test_reference_cut_open_sphere():
    """The 13 x 11 x 9 lattice ends at z = 0.86 inside the sphere: the surface has boundary edges there; every
    index is valid and the orientation is still consistent."""
    m = ref.case_ref("sphere_cut")
    v, q = m["vertices"], m["quads"]
    (dk, dc), (uk, uc) = ref.edge_census(q)
    assert (uc == 1).any() and (uc <= 2).all()
    assert (dc == 1).all()                       # no edge is walked twice in the same direction
    assert q.min() >= 0 and q.max() < len(v)
    assert ref.euler_number(len(v), q) == 1      # a disc
    # a boundary edge's vertices lie in the lattice's last layer of cells
    _, origin, spacing, shape, _ = ref.CASES["sphere_cut"]
    z_last = ref.lattice_coords(origin, spacing, shape)[2][-2]
    assert (v[uk[uc == 1].reshape(-1), 2] >= z_last).all()


def test_reference_iso_grows_the_sphere():
    m = ref.case_ref("sphere_iso")
    r = np.linalg.norm(m["vertices"] - [0.0, 1.0, 0.0], axis=1)
    assert np.abs(r - 1.25).max() <= ref.CASES["sphere_iso"][2] / 2
    assert ref.euler_number(len(m["vertices"]), m["quads"]) == 2
    assert ref.signed_volume(m["vertices"], m["quads"]) > ref.signed_volume(*[ref.case_ref("sphere17")[k] for k in ("vertices", "quads")])


# ---- rmr_surface_nets through the stand-alone program ------------------------------------------------------
def _build(target):
    subprocess.run(["make", "-s", "-C", CSRC, target], check=True, timeout=600)
    return os.path.join(CSRC, "build", target)


def _run_volume(exe, tmp_path, dist, origin, spacing, iso):
    """mesh_test run IN OUT: (vertices (V, 3) float32, quads (Q, 4) uint32)."""
    nz, ny, nx = dist.shape
    src, dst = str(tmp_path / "volume.bin"), str(tmp_path / "mesh.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<4f3i", *[float(x) for x in origin], float(spacing), nx, ny, nz))
        f.write(struct.pack("<f", float(iso)))
        f.write(np.ascontiguousarray(dist, F).tobytes())
    p = subprocess.run([exe, "run", src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0 and "mesh_test run ok" in p.stdout, p.stdout[-4000:]
    raw = open(dst, "rb").read()
    nv, nq = struct.unpack("<2Q", raw[:16])
    assert len(raw) == 16 + 12 * nv + 16 * nq
    v = np.frombuffer(raw, F, 3 * nv, 16).reshape(nv, 3)
    q = np.frombuffer(raw, np.uint32, 4 * nq, 16 + 12 * nv).reshape(nq, 4)
    return v, q


@pytest.mark.parametrize("name", RULE_CASES)
def test_surface_nets_matches_statement(name, tmp_path):
    _, origin, spacing, shape, iso = ref.CASES[name]
    v, q = _run_volume(_build("mesh_test"), tmp_path, ref.case_volume(name), origin, spacing, iso)
    ref.compare(v, q, ref.case_ref(name), spacing, name)
    # the library's copy of the same function (ctypes) gives the same bytes
    v2, q2 = surface_nets(ref.case_volume(name), origin, spacing, iso)
    assert v2.tobytes() == v.tobytes() and q2.tobytes() == q.tobytes()


@pytest.mark.parametrize("name", ["sphere_empty", "sphere_full"])
def test_surface_nets_empty_and_full(name, tmp_path):
    _, origin, spacing, shape, iso = ref.CASES[name]
    d = ref.case_volume(name)
    assert (d < 0).all() if name == "sphere_full" else (d > 0).all()
    v, q = _run_volume(_build("mesh_test"), tmp_path, d, origin, spacing, iso)
    assert v.shape == (0, 3) and q.shape == (0, 4)
    assert len(ref.case_ref(name)["vertices"]) == 0 and len(ref.case_ref(name)["quads"]) == 0


def test_surface_nets_nan_and_infinite_distances():
    """A random volume with NaN, +inf and -inf sprinkled in: crossings fall back to 0.5, a NaN is outside."""
    rng = np.random.default_rng(16)
    d = rng.normal(size=(9, 10, 11)).astype(F)
    pick = rng.integers(0, 12, d.shape)
    d[pick == 0] = np.nan
    d[pick == 1] = np.inf
    d[pick == 2] = -np.inf
    origin, spacing = (-0.7, 0.3, 11.1), 0.37
    want = ref.surface_nets(d, origin, spacing, 0.1)
    assert len(want["quads"]) > 200 and np.isfinite(want["vertices"]).all()
    v, q = surface_nets(d, origin, spacing, 0.1)
    ref.compare(v, q, want, spacing, "random with NaN and inf")
    assert np.isfinite(v).all()
    tri = quads_to_triangles(q)
    assert tri.shape == (2 * len(q), 3) and (tri[0] == q[0, [0, 1, 2]]).all() and (tri[1] == q[0, [0, 2, 3]]).all()


def _run_standalone(target, tmp_path):
    p = subprocess.run([_build(target), str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:]
    assert "mesh_test ok" in p.stdout, p.stdout[-4000:]
    for word in ("Sanitizer", "runtime error"):
        assert word not in p.stdout, p.stdout[-4000:]


def test_mesh_host_checks(tmp_path):
    _run_standalone("mesh_test", tmp_path)


def test_mesh_host_checks_sanitized(tmp_path):
    from .test_accel_cpu import _sanitizers_work
    if not _sanitizers_work(str(tmp_path)):
        pytest.skip("a one-line program does not build or start under -fsanitize=address,undefined")
    _run_standalone("mesh_test_san", tmp_path)
    # and the rule on a whole volume, under the sanitizers
    _, origin, spacing, shape, iso = ref.CASES["sphere_cut"]
    v, q = _run_volume(os.path.join(CSRC, "build", "mesh_test_san"), tmp_path, ref.case_volume("sphere_cut"), origin, spacing, iso)
    ref.compare(v, q, ref.case_ref("sphere_cut"), spacing, "sphere_cut (sanitized)")


def test_mesh_cpp_has_no_hip():
    for name in ("mesh.cpp", "mesh_test.cpp", "rmr_mesh_rule.h"):
        text = open(os.path.join(CSRC, name)).read()
        assert "#include <hip" not in text and "__global__" not in text, name


# ---- rmr_check_volume -----------------------------------------------------------------------------------------
def test_check_volume_names_the_field():
    ok = ((0.0, 0.0, 0.0), 0.5, (2, 2, 2))
    assert check_volume(*ok) is None
    assert check_volume((0.0, 0.0, 0.0), 1e-3, (4096, 4096, 64)) is None      # 2^30 points
    for origin in ((np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf)):
        assert check_volume(origin, 0.5, (2, 2, 2)) == "origin"
    for spacing in (0.0, -0.5, np.inf, np.nan):
        assert check_volume((0, 0, 0), spacing, (2, 2, 2)) == "spacing"
    for shape in ((1, 2, 2), (2, 0, 2), (2, 2, -3), (4097, 2, 2)):
        assert check_volume((0, 0, 0), 0.5, shape) == "n"
    assert check_volume((0, 0, 0), 0.5, (4096, 4096, 65)) == "points"
    with pytest.raises(RMRError) as e:
        surface_nets(np.zeros((2, 2, 2), F), (0, 0, 0), -1.0)
    assert e.value.code == -1 and "spacing" in str(e.value)


# ---- the writers --------------------------------------------------------------------------------------------
def _parse_obj(path):
    v, vn, f = [], [], []
    for line in open(path):
        w = line.split()
        if not w or w[0].startswith("#"):
            continue
        if w[0] == "v":
            v.append([F(x) for x in w[1:]])
        elif w[0] == "vn":
            vn.append([F(x) for x in w[1:]])
        elif w[0] == "f":
            f.append([tuple(int(i) if i else 0 for i in c.split("/")) for c in w[1:]])
        else:
            raise AssertionError("unexpected OBJ line %r" % line)
    return np.array(v, F).reshape(-1, 3), np.array(vn, F).reshape(-1, 3), f


def _parse_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode().splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    nv = int([ln for ln in lines if ln.startswith("element vertex")][0].split()[2])
    nf = int([ln for ln in lines if ln.startswith("element face")][0].split()[2])
    props = [ln.split()[2] for ln in lines if ln.startswith("property float")]
    assert "property list uchar uint vertex_indices" in lines
    vert = np.frombuffer(body, "<f4", nv * len(props)).reshape(nv, len(props))
    face = np.frombuffer(body, np.dtype([("n", "u1"), ("i", "<u4", (4,))]), nf, 4 * nv * len(props))
    assert len(body) == 4 * nv * len(props) + 17 * nf
    return props, vert, face


def test_obj_and_ply_read_back(tmp_path):
    _, origin, spacing, shape, iso = ref.CASES["sphere_cut"]
    v, q = surface_nets(ref.case_volume("sphere_cut"), origin, spacing, iso)
    rng = np.random.default_rng(3)
    n = rng.normal(size=v.shape).astype(F)
    ids = rng.integers(0, 4, len(v)).astype(F)
    # OBJ with normals: v, vn, f a//a ... 1-based; the float32 values read back exactly
    path = str(tmp_path / "m.obj")
    encode_obj(path, v, q, normals=n)
    pv, pn, pf = _parse_obj(path)
    assert pv.tobytes() == v.tobytes() and pn.tobytes() == n.tobytes()
    assert len(pf) == len(q) and all(len(c) == 3 and c[0] == c[2] and c[1] == 0 for face in pf for c in face)
    assert (np.array([[c[0] for c in face] for face in pf]) == q.astype(np.int64) + 1).all()
    # OBJ without
    encode_obj(path, v, q)
    pv, pn, pf = _parse_obj(path)
    assert pv.tobytes() == v.tobytes() and len(pn) == 0
    assert (np.array([[c[0] for c in face] for face in pf]) == q.astype(np.int64) + 1).all() and all(len(c) == 1 for c in pf[0])
    # PLY with everything, with ids alone and bare
    path = str(tmp_path / "m.ply")
    encode_ply(path, v, q, normals=n, ids=ids)
    props, vert, face = _parse_ply(path)
    assert props == ["x", "y", "z", "nx", "ny", "nz", "material"]
    assert vert[:, :3].tobytes() == v.tobytes() and vert[:, 3:6].tobytes() == n.tobytes() and (vert[:, 6] == ids).all()
    assert (face["n"] == 4).all() and (face["i"] == q).all()
    encode_ply(path, v, q, ids=ids)
    props, vert, face = _parse_ply(path)
    assert props == ["x", "y", "z", "material"] and (vert[:, 3] == ids).all() and (face["i"] == q).all()
    encode_ply(path, v, q)
    props, vert, face = _parse_ply(path)
    assert props == ["x", "y", "z"] and vert.tobytes() == v.tobytes() and (face["i"] == q).all()
    # an empty mesh is a valid file; a bad index and a bad path are errors
    encode_obj(path, np.zeros((0, 3), F), np.zeros((0, 4), np.uint32))
    with pytest.raises(RMRError) as e:
        encode_obj(path, v[:5], q)
    assert e.value.code == -1
    with pytest.raises(RMRError) as e:
        encode_ply(str(tmp_path / "no" / "such" / "m.ply"), v, q)
    assert e.value.code == -4


# ---- the kernels' resources -------------------------------------------------------------------------------
def test_volume_kernels_resources(tmp_path):
    """rmr_volume.hip for gfx950 with the compiler's resource remarks: no dynamic stack anywhere, no scratch
    except in the general map's node interpreter (the <-1> kernels, as k_eval_map<-1>), and LDS only for the
    extraction kernels' per-wave totals; DESIGN.md §4.16 has the figures."""
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-slp-vectorize",
           "-Wno-pass-failed", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
           os.path.join(CSRC, "rmr_volume.hip"), "-o", str(tmp_path / "rmr_volume.o")]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-4000:]
    res, name = {}, None
    for line in p.stdout.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
        m = re.search(r"(ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|VGPRs|TotalSGPRs|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            res[name][m.group(1).split(" [")[0]] = int(m.group(2))
        m = re.search(r"Dynamic Stack: (\w+)", line)
        if m and name:
            res[name]["Dynamic Stack"] = m.group(1)
    for k in sorted(res):
        print(k, res[k])
    assert len(res) == 20, sorted(res)   # k_sample_volume x 10, k_mesh_attr x 5, classify, scan1, scan2, vertices, quads
    for k, v in res.items():
        assert v["Dynamic Stack"] == "False", k
        if "ILin1E" not in k:
            assert v["ScratchSize"] == 0, (k, v)
        if "k_sample_volume" in k or "k_mesh_attr" in k:
            assert v["LDS Size"] == 0, (k, v)
        else:
            assert v["LDS Size"] <= 4096, (k, v)


# ---- rmr_cli ------------------------------------------------------------------------------------------------
def test_cli_help_and_usage_errors():
    help_text = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60).stdout
    for word in ("--mesh ", "--mesh-bounds", "--mesh-grid", "--mesh-iso"):
        assert word in help_text, word

    def rc(*args):
        return subprocess.run([CLI, "--size", "8x8"] + list(args), capture_output=True, text=True, timeout=60).returncode
    good = "-1.5,-0.5,-1.5,1.5,2.5,1.5"
    for bad in (("--mesh", "m.obj"),                                       # the bounds are required
                ("--mesh",), ("--mesh", ""), ("--mesh", "m.stl", "--mesh-bounds", good),
                ("--mesh", "m.obj", "--mesh-bounds", "0,0,0,1,1"),
                ("--mesh", "m.obj", "--mesh-bounds", "0,0,0,1,1,x"),
                ("--mesh", "m.obj", "--mesh-bounds", "0,0,0,1,0,1"),       # an empty side
                ("--mesh", "m.obj", "--mesh-bounds", "0,0,0,1,1,nan"),
                ("--mesh", "m.obj", "--mesh-bounds", good, "--mesh-grid", "0"),
                ("--mesh", "m.obj", "--mesh-bounds", good, "--mesh-grid", "5000"),
                ("--mesh", "m.obj", "--mesh-bounds", good, "--mesh-iso", "inf"),
                ("--mesh-bounds", good), ("--mesh-grid", "16"), ("--mesh-iso", "0.1"),   # without --mesh
                ("--mesh", "m.obj", "--mesh-bounds", good, "--gpus", "2")):
        assert rc(*bad) == 2, bad
    # a good set parses (--print-tiles ends the program before a device is needed)
    assert rc("--mesh", "m.ply", "--mesh-bounds", good, "--mesh-grid", "16", "--mesh-iso", "0.25", "--print-tiles",
              "--grid", "1x1") == 0
