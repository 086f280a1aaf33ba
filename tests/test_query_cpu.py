"""First-hit and distance queries, the parts that need no GPU (include/rmr.h): the
layout of rmr_hit, the ray rule the kernels share with rmr_check_rays (csrc/rmr_ray_check.h) through the
stand-alone program csrc/query_test.cpp, plain and under the sanitizers, and the resources of the query
kernels compiled for gfx950 (not run): no scratch outside the general map's node interpreter.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from raymarchrenderer_amd import abi, lib

from .conftest import ROOT

CSRC = os.path.join(ROOT, "raymarchrenderer_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_hit_layout():
    dt = np.dtype(abi.HIT_DTYPE)
    assert dt.itemsize == 32 and C.sizeof(abi.Hit) == 32
    assert dt.names == ("pos", "t", "n", "id") == tuple(f[0] for f in abi.Hit._fields_)
    assert [dt.fields[k][1] for k in dt.names] == [0, 12, 16, 28]
    assert [getattr(abi.Hit, k).offset for k in dt.names] == [0, 12, 16, 28]
    assert dt["pos"].shape == (3,) and dt["n"].shape == (3,) and dt["t"] == np.float32 and dt["id"] == np.float32
    assert abi.CAST_NORMALS == 1


def test_library_exports_the_queries():
    L = lib()
    for name in ("rmr_cast_rays", "rmr_eval_map", "rmr_trace_rays_device", "rmr_cast_rays_device", "rmr_eval_map_device",
                 "rmr_query_rejects", "rmr_set_query_grid"):
        assert hasattr(L, name), name
    # null contexts and lists: RMR_E_INVALID before anything touches a GPU
    assert L.rmr_cast_rays(None, None, 0, 0, None) == -1 and L.rmr_eval_map(None, None, 0, None) == -1
    assert L.rmr_set_query_grid(None, 0) == -1 and L.rmr_query_rejects(None, None) == -1
    sizes = (C.c_int32 * 16)()
    assert L.rmr_abi_sizes(sizes, 16) == 8   # (unchanged: rmr_hit's size is a static_assert in the library)


def _run_standalone(target):
    """csrc/query_test.cpp (its own main; rmr_ray_check.h and camera.cpp alone: no HIP, no Python)."""
    subprocess.run(["make", "-s", "-C", CSRC, target], check=True, timeout=600)
    p = subprocess.run([os.path.join(CSRC, "build", target)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:]
    assert "query_test ok" in p.stdout, p.stdout[-4000:]
    for word in ("Sanitizer", "runtime error"):
        assert word not in p.stdout, p.stdout[-4000:]


def test_query_host_checks():
    _run_standalone("query_test")


def test_query_host_checks_sanitized(tmp_path):
    from .test_accel_cpu import _sanitizers_work
    if not _sanitizers_work(str(tmp_path)):
        pytest.skip("a one-line program does not build or start under -fsanitize=address,undefined")
    _run_standalone("query_test_san")


def test_query_kernels_need_no_scratch(tmp_path):
    """rmr_query.hip for gfx950 with the compiler's resource remarks: every k_cast_rays / k_eval_map
    instantiation but the general map's (NP = -1, the node interpreter's variables) has no scratch; so do
    the pack and unpack kernels."""
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-slp-vectorize",
           "-Wno-pass-failed", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
           os.path.join(CSRC, "rmr_query.hip"), "-o", str(tmp_path / "rmr_query.o")]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-4000:]
    scratch, name = {}, None
    for line in p.stdout.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
    cast = {k: v for k, v in scratch.items() if "k_cast_rays" in k}
    evalm = {k: v for k, v in scratch.items() if "k_eval_map" in k}
    # 5 map classes x with / without normals; 5 map classes (Itanium names: NP as Li4E, Li8E, Li0E, Lin2E, Lin1E)
    assert len(cast) == 10 and len(evalm) == 5, sorted(scratch)
    general = [k for k in list(cast) + list(evalm) if "ILin1E" in k]
    assert len(general) == 3
    for k, v in list(cast.items()) + list(evalm.items()):
        if k not in general:
            assert v == 0, "%s: %d bytes of scratch per lane" % (k, v)
    for k, v in scratch.items():
        if "k_pack_rays" in k or "k_unpack_rgba" in k:
            assert v == 0, k
    assert sum("k_pack_rays" in k or "k_unpack_rgba" in k for k in scratch) == 2
    print({k[:40]: v for k, v in scratch.items()})
