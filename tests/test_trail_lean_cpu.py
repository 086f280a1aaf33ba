"""The statements the trailing steps run (rmr_trail_rule.h trail_row, trail_anchor_hi, trail_rule_hi; the
launch's eps bound, accel.cpp trail_eps_bound) on the CPU.

* csrc/trail_lean_test.cpp, plain and under the address and undefined-behaviour sanitizers (its own main:
  nothing is loaded into Python), on trail_rule_test.cpp's scenes and marches, each ray with its escape bound:
  wherever the rule accepts, the whole float opU fold is (F_w, id_w) bit for bit; wherever it certifies, w is
  the strict minimiser at getNormal's six probes; the table row's box form has sd_box's / sd_sphere's bits; the
  launch's eps_hi is at least eps(p) at every evaluated point; and no point with a NaN or infinite coordinate
  is accepted. The share of the first rule's accepts that this rule refuses is printed, not gated.
* The same on every sphere/box case of tests/scene_family.py of at most 8 primitives (--scene FILE).
* The lane-slot kernel with the steps still compiles for gfx950 without scratch, at no more than 80 VGPRs and
  with LDS for six blocks per CU, and the diagnostic guard (-DRMR_TRAIL_CHECK) compiles."""
import os
import subprocess

import pytest

from . import scene_family as sf
from .conftest import ROOT, SCENES
from .test_kernel_batch_probes_cpu import HIPCC, _compile
from .test_trailing_steps_cpu import _source

CSRC = os.path.join(ROOT, "raymarchrenderer_amd", "csrc")
CORNELL = os.path.join(SCENES, "cornell5.scene")


def _run(target, args=()):
    p = subprocess.run([os.path.join(CSRC, "build", target)] + list(args), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:]
    lines = p.stdout.splitlines()
    assert lines[-1] == "ok" and "FAIL" not in p.stdout, p.stdout[-4000:]
    for word in ("Sanitizer", "runtime error"):
        assert word not in p.stdout, p.stdout[-4000:]
    rows = [l for l in lines if " triples " in l]
    out = []
    for l in rows:
        w = l.split()
        out.append((l, {k: int(w[w.index(k) + 1]) for k in ("triples", "accepted", "nonfinite")},
                    int(w[w.index("hits", w.index("certified")) + 1])))
    return out


def _compiled_in(target):
    subprocess.run(["make", "-s", "-C", CSRC, target], check=True, timeout=600)
    rows = _run(target)
    assert len(rows) == 5   # Cornell-5 at two maxDist, the two overlay scenes, the large sphere
    for l, n, cert_hits in rows:
        print(l)
        assert n["triples"] >= 1000000 and n["nonfinite"] >= 60000, l
        if l.startswith("cornell5"):
            assert n["accepted"] > 0 and cert_hits > 0, l


def _family(target, tmp_path):
    subprocess.run(["make", "-s", "-C", CSRC, target], check=True, timeout=600)
    for name in sf.RULE_CASES:
        path = str(tmp_path / (name + ".txt"))
        sf.write_rule_scene(name, path)
        rows = _run(target, ["--scene", path])
        assert len(rows) == 1
        l, n, _ = rows[0]
        print(l)
        assert l.startswith(name + " maxDist %g:" % sf.max_dist(name)), l
        assert n["triples"] >= 200000 and n["nonfinite"] >= 60000, l
        if name == "unit":
            assert n["accepted"] > 0, l


def test_lean_rule_host_checks():
    _compiled_in("trail_lean_test")


def test_lean_rule_on_the_family(tmp_path):
    _family("trail_lean_test", tmp_path)


def test_lean_rule_host_checks_sanitized(tmp_path):
    from .test_accel_cpu import _sanitizers_work
    if not _sanitizers_work(str(tmp_path)):
        pytest.skip("a one-line program does not build or start under -fsanitize=address,undefined")
    _compiled_in("trail_lean_test_san")
    _family("trail_lean_test_san", tmp_path)


def test_lean_program_has_no_hip():
    text = open(os.path.join(CSRC, "trail_lean_test.cpp")).read()
    assert "#include <hip" not in text and "__global__" not in text


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_guard_build_compiles_and_is_not_in_the_plain_kernel(tmp_path, monkeypatch):
    """The kernel with -DRMR_TRAIL_CHECK compiles (a diagnostic build may spill; it only has to run), and the
    plain source's kernel keeps the schedule's limits."""
    _, on = _source(tmp_path, CORNELL, "rm1", monkeypatch, "1")
    assert "#define RMR_TRAIL_STEPS 1" in on and "RMR_TRAIL_CHECK" not in on
    plain = tmp_path / "plain.hip"
    plain.write_text(on)
    nt = _compile(str(plain))
    assert nt["vgpr_spill_count"] == 0 and nt["private_segment_fixed_size"] == 0, nt
    assert nt["vgpr_count"] <= 80 and nt["group_segment_fixed_size"] <= 21 * 1280, nt
    guard = tmp_path / "guard.hip"
    guard.write_text("//@opts -DRMR_TRAIL_CHECK\n" + on)
    ng = _compile(str(guard))
    assert ng["group_segment_fixed_size"] == nt["group_segment_fixed_size"], ng
