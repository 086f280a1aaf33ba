"""The lane-slot schedule (rmr_trace.h RMR_LANE_SLOTS) is a specialisation-time switch of one kernel
class, RM1's certified sphere/box kernels (CPU; hipRTC and hipcc cross-compile).

* Every other class generates the same source, byte for byte, and the same code-object key whether the
  switch is left at its default, forced on or forced off.
* Cornell-5's source with the schedule on compiles for gfx950 without scratch: no spilled VGPR, no
  private segment (the schedule's second register set must fit beside the marching state)."""
import os
import re
import subprocess

import pytest

from raymarchrenderer_amd.renderer import jit_compile_scene

from .conftest import GOLDEN, ROOT, SCENES

HIPCC = "/opt/rocm/bin/hipcc"
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
# rmr_jit.cpp kOptions
OPTS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-unused-function",
        "-fno-slp-vectorize", "-DRMR_MANDELBULB_INLINE=1"]
OTHER_CLASSES = [
    ("mandelbulb", os.path.join(SCENES, "mandelbulb.scene"), "rm1"),
    ("csg256", os.path.join(SCENES, "csg256.scene"), "rm1"),
    ("rm2_simple", os.path.join(GOLDEN, "scenes", "simple.scene"), "rm2"),
    ("rm3_builtin", None, "rm3"),
]


def _source(tmp, scene, variant, monkeypatch, slots):
    d = tmp / ("dump_%s" % slots)
    d.mkdir(exist_ok=True)
    monkeypatch.setenv("RMR_JIT_DUMP", str(d))
    monkeypatch.setenv("RMR_JIT_CACHE", str(tmp / "cache"))
    if slots is None:
        monkeypatch.delenv("RMR_JIT_SLOTS", raising=False)
    else:
        monkeypatch.setenv("RMR_JIT_SLOTS", slots)
    key = jit_compile_scene(scene, variant, diag=True)
    return key, (d / (key + ".hip")).read_text()


def _compile(src_path, extra):
    src = open(src_path).read()
    opts = list(OPTS)
    for line in src.splitlines():
        if line.startswith("//@opts "):
            opts += line[8:].split()
    inc = ["-I", os.path.join(ROOT, "raymarchrenderer_amd", "csrc"), "-I", os.path.join(ROOT, "include")]
    out = src_path + ".o"
    subprocess.run([HIPCC] + opts + extra + inc + ["--offload-device-only", "--no-gpu-bundle-output", "-c", "-o", out,
                                                   "-x", "hip", src_path], check=True, capture_output=True)
    notes = subprocess.run([READELF, "--notes", out], check=True, capture_output=True, text=True).stdout
    return {k: int(v) for k, v in re.findall(
        r"\.(vgpr_count|vgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\d+)", notes)}


@pytest.mark.parametrize("name,scene,variant", OTHER_CLASSES, ids=[c[0] for c in OTHER_CLASSES])
def test_other_classes_do_not_see_the_switch(tmp_path, monkeypatch, name, scene, variant):
    got = [_source(tmp_path, scene, variant, monkeypatch, s) for s in (None, "1", "0")]
    assert "RMR_LANE_SLOTS" not in got[0][1]
    for key, src in got[1:]:
        assert key == got[0][0]
        assert src == got[0][1]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_cornell5_slots_kernel_has_no_scratch(tmp_path, monkeypatch):
    scene = os.path.join(SCENES, "cornell5.scene")
    key_on, on = _source(tmp_path, scene, "rm1", monkeypatch, "1")
    key_off, off = _source(tmp_path, scene, "rm1", monkeypatch, "0")
    # the switch is part of the source, hence of the code-object key
    assert "#define RMR_LANE_SLOTS 1" in on and "RMR_LANE_SLOTS" not in off
    assert key_on != key_off
    p = tmp_path / "cornell5_slots.hip"
    p.write_text(on)
    nt = _compile(str(p), [])
    assert nt["vgpr_spill_count"] == 0 and nt["private_segment_fixed_size"] == 0, nt
    # 6 workgroups per CU: at most 80 VGPRs, and 6 x the block's LDS within the CU's 160 KiB
    assert nt["vgpr_count"] <= 80 and 6 * nt["group_segment_fixed_size"] <= 160 * 1024, nt
