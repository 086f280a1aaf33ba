"""The trailing passes chosen per wave (rmr_trail_rule.h trail_word; rmr_trace.h, the pass rule) on the CPU.

* csrc/trail_word_test.cpp, plain and under the address and undefined-behaviour sanitizers (its own main:
  nothing is loaded into Python): the launch word's packing and unpacking round-trip over the whole range
  (k_max 0..15, ratio 0..8 eighths, park exit on / off), the word stays clear of the thresholds below it, a
  fixed schedule's word is its pass count, and the range check refuses what lies outside.
* The change is in the trailing steps' block alone: every kernel class without the steps generates the source
  it generated before the change, byte for byte (tests/golden/trail_adaptive_parent_sources.json: the sha256 of
  each class's generated source at the parent commit; a later change of the generator re-records it with
  `python -m tests.test_trail_adaptive_cpu`), and that source has none of the feature's words, so the rule's three
  launch values are compile-time zeros there.
* The pass rule is a code object of its own (-DRMR_TRAIL_RULE=1, what a launch tuned with a ratio or the park
  exit runs): it keeps the schedule's limits — no scratch, at most 80 VGPRs, LDS for six blocks per CU — as the
  plain kernel does. The profiling build (-DRMR_PROFILE), which counts the passes by pass index in counter
  slots of its own, compiles with and without the rule; its LDS is the plain kernel's (a diagnostic build may
  spill; it only has to run)."""
import hashlib
import json
import os
import subprocess

import pytest

from .conftest import GOLDEN, ROOT
from .test_kernel_batch_probes_cpu import HIPCC, _compile
from .test_trailing_steps_cpu import CORNELL, FEATURE_WORDS, OTHER_CLASSES, _source

CSRC = os.path.join(ROOT, "raymarchrenderer_amd", "csrc")
PARENT_SOURCES = os.path.join(GOLDEN, "trail_adaptive_parent_sources.json")


def _run(target):
    subprocess.run(["make", "-s", "-C", CSRC, target], check=True, timeout=600)
    p = subprocess.run([os.path.join(CSRC, "build", target)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-4000:]
    lines = p.stdout.splitlines()
    assert lines[-1] == "ok" and "FAIL" not in p.stdout, p.stdout[-4000:]
    for word in ("Sanitizer", "runtime error"):
        assert word not in p.stdout, p.stdout[-4000:]
    return lines


def test_tuning_word_round_trip():
    lines = _run("trail_word_test")
    assert lines[-2] == "tunings %d k_max 0..15 ratio 0..8" % (16 * 9 * 2), lines[-2]


def test_tuning_word_round_trip_sanitized(tmp_path):
    from .test_accel_cpu import _sanitizers_work
    if not _sanitizers_work(str(tmp_path)):
        pytest.skip("a one-line program does not build or start under -fsanitize=address,undefined")
    _run("trail_word_test_san")


def test_word_program_has_no_hip():
    text = open(os.path.join(CSRC, "trail_word_test.cpp")).read()
    assert "#include <hip" not in text and "__global__" not in text


def _digest(text):
    return hashlib.sha256(text.encode()).hexdigest()


@pytest.mark.parametrize("name,scene,variant,env", OTHER_CLASSES, ids=[c[0] for c in OTHER_CLASSES])
def test_other_classes_generate_the_parent_source(tmp_path, monkeypatch, name, scene, variant, env):
    with open(PARENT_SOURCES) as f:
        want = json.load(f)
    _, src = _source(tmp_path, scene, variant, monkeypatch, None, env)
    for word in FEATURE_WORDS:
        assert word not in src, (name, word)
    assert _digest(src) == want[name], name


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_rule_and_profile_builds(tmp_path, monkeypatch):
    _, on = _source(tmp_path, CORNELL, "rm1", monkeypatch, "1")
    assert "#define RMR_TRAIL_STEPS 1" in on and "RMR_PROFILE" not in on
    plain = tmp_path / "plain.hip"
    plain.write_text(on)
    nt = _compile(str(plain))
    # the schedule's limits, without the pass rule and with it: six blocks per CU (21 LDS granules of 1280 B)
    assert nt["vgpr_spill_count"] == 0 and nt["private_segment_fixed_size"] == 0, nt
    assert nt["vgpr_count"] <= 80 and nt["group_segment_fixed_size"] <= 21 * 1280, nt
    rule = tmp_path / "rule.hip"
    rule.write_text("//@opts -DRMR_TRAIL_RULE=1\n" + on)
    nr = _compile(str(rule))
    assert nr["vgpr_spill_count"] == 0 and nr["private_segment_fixed_size"] == 0, nr
    assert nr["vgpr_count"] <= 80 and nr["group_segment_fixed_size"] <= 21 * 1280, nr
    for name, opts in (("profile", "-DRMR_PROFILE"), ("profile_rule", "-DRMR_PROFILE -DRMR_TRAIL_RULE=1")):
        prof = tmp_path / (name + ".hip")
        prof.write_text("//@opts %s\n" % opts + on)
        npf = _compile(str(prof))
        assert npf["group_segment_fixed_size"] == nt["group_segment_fixed_size"], (name, npf)


if __name__ == "__main__":   # re-record the fixture: the generated source of every class without the steps
    import tempfile

    class _Env:
        def setenv(self, k, v):
            os.environ[k] = v

        def delenv(self, k, raising=False):
            os.environ.pop(k, None)

    import pathlib
    out = {}
    for name, scene, variant, env in OTHER_CLASSES:
        tmp = pathlib.Path(tempfile.mkdtemp())
        out[name] = _digest(_source(tmp, scene, variant, _Env(), None, env)[1])
    with open(PARENT_SOURCES, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))
