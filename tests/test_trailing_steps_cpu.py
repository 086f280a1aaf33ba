"""Trailing steps (rmr_trace.h RMR_TRAIL_STEPS) on the CPU: the acceptance rule's host program, and the
specialisation-time switch (hipRTC and hipcc cross-compile; no GPU).

* csrc/trail_rule_test.cpp, plain and under the address and undefined-behaviour sanitizers (its own main:
  nothing is loaded into Python): over 10^6 ray / anchor / step triples per scene, wherever rmr_trail_rule.h
  accepts a step the whole float opU fold at that point is (F_w, id_w) bit for bit, and wherever it
  certifies, w is the strict minimiser at getNormal's six probes. The accept share is reported and must not
  be zero on Cornell-5.
* Classes other than the lane-slot kernels generate the same source, byte for byte, and the same
  code-object key with RMR_JIT_TRAIL unset, 1, 2 and 0.
* The lane-slot class's source without the switch has nothing of the feature; with it, the defines, the
  map's eval_t, and a kernel for gfx950 without scratch, at no more than 80 VGPRs and with LDS for six
  blocks per CU."""
import os
import subprocess

import pytest

from .conftest import GOLDEN, ROOT, SCENES
from .test_kernel_batch_probes_cpu import HIPCC, _compile

from raymarchrenderer_amd.renderer import jit_compile_scene

CSRC = os.path.join(ROOT, "raymarchrenderer_amd", "csrc")
CORNELL = os.path.join(SCENES, "cornell5.scene")
OTHER_CLASSES = [
    ("rm2_simple", os.path.join(GOLDEN, "scenes", "simple.scene"), "rm2", None),
    ("rm3_builtin", None, "rm3", None),
    ("mandelbulb", os.path.join(SCENES, "mandelbulb.scene"), "rm1", None),
    ("csg256", os.path.join(SCENES, "csg256.scene"), "rm1", None),
    ("default_prog_mats", os.path.join(GOLDEN, "scenes", "default.scene"), "rm1", None),
    ("glass_prog_mats", os.path.join(GOLDEN, "scenes", "glass_test.scene"), "rm1", None),
    ("cornell5_slots_off", CORNELL, "rm1", {"RMR_JIT_SLOTS": "0"}),          # the class, schedule off
    ("cornell5_bprobes_off", CORNELL, "rm1", {"RMR_JIT_BPROBES": "0"}),      # ... in-loop probes
]
FEATURE_WORDS = ("RMR_TRAIL", "eval_t", "s2 = m.s2", "trail")


def _run_standalone(target):
    subprocess.run(["make", "-s", "-C", CSRC, target], check=True, timeout=600)
    p = subprocess.run([os.path.join(CSRC, "build", target)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:]
    lines = p.stdout.splitlines()
    assert lines[-1] == "ok" and "FAIL" not in p.stdout, p.stdout[-4000:]
    for word in ("Sanitizer", "runtime error"):
        assert word not in p.stdout, p.stdout[-4000:]
    rows = [l for l in lines if " triples " in l]
    assert len(rows) == 5, p.stdout[-4000:]   # Cornell-5 at two maxDist, the two overlay scenes, the large sphere
    for l in rows:
        w = l.split()
        triples, accepted = int(w[w.index("triples") + 1]), int(w[w.index("accepted") + 1])
        assert triples >= 1000000, l
        if l.startswith("cornell5"):
            assert accepted > 0 and int(w[-1]) > 0, l   # accepted steps, certified hits
    return rows


def test_trail_rule_host_checks():
    for l in _run_standalone("trail_rule_test"):
        print(l)


def test_trail_rule_host_checks_sanitized(tmp_path):
    from .test_accel_cpu import _sanitizers_work
    if not _sanitizers_work(str(tmp_path)):
        pytest.skip("a one-line program does not build or start under -fsanitize=address,undefined")
    _run_standalone("trail_rule_test_san")


def test_trail_rule_header_has_no_hip():
    for name in ("rmr_trail_rule.h", "trail_rule_test.cpp"):
        text = open(os.path.join(CSRC, name)).read()
        assert "#include <hip" not in text and "__global__" not in text, name


def _source(tmp, scene, variant, monkeypatch, trail, env=None):
    d = tmp / ("dump_%s" % trail)
    d.mkdir(exist_ok=True)
    monkeypatch.setenv("RMR_JIT_DUMP", str(d))
    monkeypatch.setenv("RMR_JIT_CACHE", str(tmp / "cache"))
    for name in ("RMR_JIT_SLOTS", "RMR_JIT_BPROBES", "RMR_JIT_OVERFLOW", "RMR_JIT_TRAIL"):
        monkeypatch.delenv(name, raising=False)
    for name, val in (env or {}).items():
        monkeypatch.setenv(name, val)
    if trail is not None:
        monkeypatch.setenv("RMR_JIT_TRAIL", trail)
    key = jit_compile_scene(scene, variant, diag=True)
    return key, (d / (key + ".hip")).read_text()


@pytest.mark.parametrize("name,scene,variant,env", OTHER_CLASSES, ids=[c[0] for c in OTHER_CLASSES])
def test_other_classes_do_not_see_the_switch(tmp_path, monkeypatch, name, scene, variant, env):
    got = [_source(tmp_path, scene, variant, monkeypatch, t, env) for t in (None, "1", "2", "0")]
    for word in FEATURE_WORDS:
        assert word not in got[0][1], word
    for key, src in got[1:]:
        assert key == got[0][0]
        assert src == got[0][1]


def test_switch_is_part_of_the_lane_slot_source(tmp_path, monkeypatch):
    key_def, dflt = _source(tmp_path, CORNELL, "rm1", monkeypatch, None)
    key_off, off = _source(tmp_path, CORNELL, "rm1", monkeypatch, "0")
    key_on, on = _source(tmp_path, CORNELL, "rm1", monkeypatch, "1")
    key_gl, gl = _source(tmp_path, CORNELL, "rm1", monkeypatch, "2")
    assert "#define RMR_LANE_SLOTS 1" in off and "#define RMR_BATCH_PROBES 1" in off
    for word in FEATURE_WORDS:   # the source without the switch has nothing of the feature
        assert word not in off, word
    assert "#define RMR_TRAIL_STEPS 1" in on and "#define RMR_TRAIL_LDS 1" in on and "eval_t(" in on and "s2 = m.s2;" in on
    assert "#define RMR_TRAIL_STEPS 1" in gl and "RMR_TRAIL_LDS" not in gl
    assert len({key_off, key_on, key_gl}) == 3
    # the class's default is one of the two, whichever DESIGN.md §4.2 settled on
    assert (dflt, key_def) in ((off, key_off), (on, key_on))
    # ... and apart from the switch's own lines the two sources are the same text
    strip = lambda s: [l for l in s.splitlines() if "RMR_TRAIL" not in l]
    a, b = strip(off), strip(on)
    extra = [l for l in b if l not in a]
    assert all("eval_t" in l or "s2" in l or l.strip() in ("}",) for l in extra), extra


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("trail", ["1", "2"])
def test_cornell5_trailing_kernel_has_no_scratch(tmp_path, monkeypatch, trail):
    _, on = _source(tmp_path, CORNELL, "rm1", monkeypatch, trail)
    p = tmp_path / ("cornell5_trail_%s.hip" % trail)
    p.write_text(on)
    nt = _compile(str(p))
    assert nt["vgpr_spill_count"] == 0 and nt["private_segment_fixed_size"] == 0, nt
    # 6 workgroups per CU: at most 80 VGPRs, and the block's LDS within the 21 granules of 1280 B that the
    # kernel without the steps occupies (six blocks of 22 granules do not fit the CU's 160 KiB)
    assert nt["vgpr_count"] <= 80 and nt["group_segment_fixed_size"] <= 21 * 1280, nt
