"""The lane-slot park step's overflow rule (csrc/rmr_slot_rule.h, the header trace_main compiles) and the
wave schedule around it, on the host: the stand-alone program csrc/slot_rule_test.cpp, plain and under the
address and undefined-behaviour sanitizers (its own main: nothing is loaded into Python).

The program checks, over every slot state of a 6-lane wave and 200,000 random 64-lane masks, that the
candidate-to-slot assignment is injective and uses only empty slots, that the event count afterwards is the
number of event slots, and that no candidate is left over while a slot is empty; then it runs a whole wave
of the schedule with random march lengths and event kinds through the exhaustion of the work queue, for P
in {1, 8, 20, 255}, T2 in {1, 24, 32, 48, 56, 64, 255}, three refill thresholds and launches of 1 to 3000
units, with the deposit on and off: the loop ends, every unit is stored exactly once, and no pass runs with
neither an active lane nor progress."""
import os
import subprocess

import pytest

from .conftest import ROOT

CSRC = os.path.join(ROOT, "raymarchrenderer_amd", "csrc")


def _run_standalone(target):
    subprocess.run(["make", "-s", "-C", CSRC, target], check=True, timeout=600)
    p = subprocess.run([os.path.join(CSRC, "build", target)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:]
    lines = p.stdout.splitlines()
    assert lines[-1] == "ok" and "FAIL" not in p.stdout, p.stdout[-4000:]
    assert any(l.startswith("rule: ") and int(l.split()[1]) > 200000 for l in lines), p.stdout[-4000:]
    assert "wave: 1680 runs" in lines, p.stdout[-4000:]   # 4 P x 7 T2 x 3 refill x 5 sizes x on / off x 2 seeds
    for word in ("Sanitizer", "runtime error"):
        assert word not in p.stdout, p.stdout[-4000:]


def test_slot_rule_host_checks():
    _run_standalone("slot_rule_test")


def test_slot_rule_host_checks_sanitized(tmp_path):
    from .test_accel_cpu import _sanitizers_work
    if not _sanitizers_work(str(tmp_path)):
        pytest.skip("a one-line program does not build or start under -fsanitize=address,undefined")
    _run_standalone("slot_rule_test_san")


def test_slot_rule_header_has_no_hip():
    for name in ("rmr_slot_rule.h", "slot_rule_test.cpp"):
        text = open(os.path.join(CSRC, name)).read()
        assert "#include <hip" not in text and "__global__" not in text, name
