"""The overflow deposit (rmr_trace.h RMR_SLOT_OVERFLOW) is a specialisation-time switch of the lane-slot
kernels (CPU; hipRTC and hipcc cross-compile).

* With the switch forced on, Cornell-5's source compiles for gfx950 without scratch, within 80 VGPRs and
  with 6 x its LDS within the CU's 160 KiB: the deposit adds no LDS array and keeps nothing alive across the
  map loop.
* The switch is part of the generated source, hence of the code-object key.
* Every class without lane slots generates the same source, byte for byte, and the same key whether the
  switch is left at its default, forced on or forced off."""
import os

import pytest

from raymarchrenderer_amd.renderer import jit_compile_scene

from .conftest import SCENES
from .test_kernel_slots_cpu import HIPCC, OTHER_CLASSES, _compile


def _source(tmp, scene, variant, monkeypatch, overflow):
    d = tmp / ("dump_%s" % overflow)
    d.mkdir(exist_ok=True)
    monkeypatch.setenv("RMR_JIT_DUMP", str(d))
    monkeypatch.setenv("RMR_JIT_CACHE", str(tmp / "cache"))
    for k in ("RMR_JIT_SLOTS", "RMR_JIT_BPROBES"):
        monkeypatch.delenv(k, raising=False)
    if overflow is None:
        monkeypatch.delenv("RMR_JIT_OVERFLOW", raising=False)
    else:
        monkeypatch.setenv("RMR_JIT_OVERFLOW", overflow)
    key = jit_compile_scene(scene, variant, diag=True)
    return key, (d / (key + ".hip")).read_text()


@pytest.mark.parametrize("name,scene,variant", OTHER_CLASSES, ids=[c[0] for c in OTHER_CLASSES])
def test_other_classes_do_not_see_the_switch(tmp_path, monkeypatch, name, scene, variant):
    got = [_source(tmp_path, scene, variant, monkeypatch, s) for s in (None, "1", "0")]
    assert "RMR_SLOT_OVERFLOW" not in got[0][1]
    for key, src in got[1:]:
        assert key == got[0][0]
        assert src == got[0][1]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_cornell5_overflow_kernel_fits_the_budgets(tmp_path, monkeypatch):
    scene = os.path.join(SCENES, "cornell5.scene")
    key_on, on = _source(tmp_path, scene, "rm1", monkeypatch, "1")
    key_off, off = _source(tmp_path, scene, "rm1", monkeypatch, "0")
    assert "#define RMR_SLOT_OVERFLOW 1" in on and "RMR_SLOT_OVERFLOW" not in off
    assert "#define RMR_LANE_SLOTS 1" in on and "#define RMR_LANE_SLOTS 1" in off
    assert key_on != key_off
    # without the lane slots the source never sees the switch
    monkeypatch.setenv("RMR_JIT_SLOTS", "0")
    monkeypatch.setenv("RMR_JIT_OVERFLOW", "1")
    d = tmp_path / "dump_noslots"
    d.mkdir()
    monkeypatch.setenv("RMR_JIT_DUMP", str(d))
    key = jit_compile_scene(scene, "rm1", diag=True)
    assert "RMR_SLOT_OVERFLOW" not in (d / (key + ".hip")).read_text()
    p = tmp_path / "cornell5_overflow.hip"
    p.write_text(on)
    nt = _compile(str(p), [])
    print(nt)
    assert nt["vgpr_spill_count"] == 0 and nt["private_segment_fixed_size"] == 0, nt
    assert nt["vgpr_count"] <= 80 and 6 * nt["group_segment_fixed_size"] <= 160 * 1024, nt
