"""Batch probes (rmr_trace.h RMR_BATCH_PROBES) are a specialisation-time switch of the lane-slot kernels
alone (CPU; hipRTC and hipcc cross-compile).

* Classes without lane slots generate the same source, byte for byte, and the same code-object key
  whether the switch is left at its default, forced on or forced off.
* Cornell-5's source with the switch on compiles for gfx950 without scratch, at no more than 80 VGPRs and
  with LDS for six blocks per CU: the marching lane has lost its probe offset and its normal, and the
  batch's whole-map probes fit beside the marching state."""
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
NO_SLOT_CLASSES = [
    ("mandelbulb", os.path.join(SCENES, "mandelbulb.scene"), "rm1", None),
    ("csg256", os.path.join(SCENES, "csg256.scene"), "rm1", None),
    ("rm2_simple", os.path.join(GOLDEN, "scenes", "simple.scene"), "rm2", None),
    ("rm3_builtin", None, "rm3", None),
    ("default_prog_mats", os.path.join(GOLDEN, "scenes", "default.scene"), "rm1", None),
    ("cornell5_slots_off", os.path.join(SCENES, "cornell5.scene"), "rm1", "0"),   # the class, schedule off
]


def _source(tmp, scene, variant, monkeypatch, bprobes, slots=None):
    d = tmp / ("dump_%s" % bprobes)
    d.mkdir(exist_ok=True)
    monkeypatch.setenv("RMR_JIT_DUMP", str(d))
    monkeypatch.setenv("RMR_JIT_CACHE", str(tmp / "cache"))
    for name, val in (("RMR_JIT_BPROBES", bprobes), ("RMR_JIT_SLOTS", slots)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)
    key = jit_compile_scene(scene, variant, diag=True)
    return key, (d / (key + ".hip")).read_text()


def _compile(src_path):
    src = open(src_path).read()
    opts = list(OPTS)
    for line in src.splitlines():
        if line.startswith("//@opts "):
            opts += line[8:].split()
    inc = ["-I", os.path.join(ROOT, "raymarchrenderer_amd", "csrc"), "-I", os.path.join(ROOT, "include")]
    out = src_path + ".o"
    subprocess.run([HIPCC] + opts + inc + ["--offload-device-only", "--no-gpu-bundle-output", "-c", "-o", out,
                                           "-x", "hip", src_path], check=True, capture_output=True)
    notes = subprocess.run([READELF, "--notes", out], check=True, capture_output=True, text=True).stdout
    return {k: int(v) for k, v in re.findall(
        r"\.(vgpr_count|vgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\d+)", notes)}


@pytest.mark.parametrize("name,scene,variant,slots", NO_SLOT_CLASSES, ids=[c[0] for c in NO_SLOT_CLASSES])
def test_classes_without_lane_slots_do_not_see_the_switch(tmp_path, monkeypatch, name, scene, variant, slots):
    got = [_source(tmp_path, scene, variant, monkeypatch, b, slots) for b in (None, "1", "0")]
    assert "RMR_BATCH_PROBES" not in got[0][1] and "RMR_LANE_SLOTS" not in got[0][1]
    for key, src in got[1:]:
        assert key == got[0][0]
        assert src == got[0][1]


def test_switch_is_part_of_the_lane_slot_source(tmp_path, monkeypatch):
    scene = os.path.join(SCENES, "cornell5.scene")
    key_def, dflt = _source(tmp_path, scene, "rm1", monkeypatch, None)
    key_on, on = _source(tmp_path, scene, "rm1", monkeypatch, "1")
    key_off, off = _source(tmp_path, scene, "rm1", monkeypatch, "0")
    assert "#define RMR_LANE_SLOTS 1" in on and "#define RMR_LANE_SLOTS 1" in off
    assert "#define RMR_BATCH_PROBES 1" in on and "RMR_BATCH_PROBES" not in off
    assert dflt == on and key_def == key_on   # on by default wherever the lane slots are
    assert key_on != key_off


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_cornell5_batch_probe_kernel_has_no_scratch(tmp_path, monkeypatch):
    scene = os.path.join(SCENES, "cornell5.scene")
    _, on = _source(tmp_path, scene, "rm1", monkeypatch, "1")
    p = tmp_path / "cornell5_batch_probes.hip"
    p.write_text(on)
    nt = _compile(str(p))
    assert nt["vgpr_spill_count"] == 0 and nt["private_segment_fixed_size"] == 0, nt
    # 6 workgroups per CU: at most 80 VGPRs, and 6 x the block's LDS within the CU's 160 KiB
    assert nt["vgpr_count"] <= 80 and 6 * nt["group_segment_fixed_size"] <= 160 * 1024, nt
