"""The output stages' validity rule (csrc/stage_state.hpp, the one place that says when the guides, the
denoised, temporal, bloom and tonemapped images are valid) on the host: the stand-alone program
csrc/stage_state_test.cpp, plain and under the address and undefined-behaviour sanitizers (its own main:
nothing is loaded into Python).

The program holds the assignments rmr_api.cpp used to make by hand at some twenty sites, transcribed
literally, and runs 250,000 random sequences of 1 to 40 entry-point calls through them and through the
rule: after every call all nine fields are equal. After every call it also checks the invariants the
hand-kept sites only implied (a valid tonemapped image of the bloom image implies a valid bloom image, ...),
and then the pinned cases tests/test_gpu_bloom.py walks on the GPU, as a table of calls and the validity
expected after them."""
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
    count = {l.split(": ")[0]: int(l.split(": ")[1]) for l in lines[:-1]}
    assert count["walks"] >= 200000, p.stdout[-4000:]
    assert count["calls"] > 10 * count["walks"] and count["skipped"] > 0, p.stdout[-4000:]
    assert count["pinned"] >= 12, p.stdout[-4000:]     # the chain, its ten invalidators, the temporal step
    for word in ("Sanitizer", "runtime error"):
        assert word not in p.stdout, p.stdout[-4000:]


def test_stage_state_host_checks():
    _run_standalone("stage_state_test")


def test_stage_state_host_checks_sanitized(tmp_path):
    from .test_accel_cpu import _sanitizers_work
    if not _sanitizers_work(str(tmp_path)):
        pytest.skip("a one-line program does not build or start under -fsanitize=address,undefined")
    _run_standalone("stage_state_test_san")


def test_stage_state_header_has_no_hip():
    for name in ("stage_state.hpp", "stage_state_test.cpp"):
        text = open(os.path.join(CSRC, name)).read()
        assert "#include <hip" not in text and "__global__" not in text and "rmr_internal.h" not in text, name


def test_only_the_rule_assigns_the_fields():
    api = open(os.path.join(CSRC, "rmr_api.cpp")).read()
    for field in ("guides_valid", "dn_result", "dn_guided", "var_result", "t_cur", "tm_valid", "tm_source",
                  "bl_valid", "bl_source"):
        assert field + " =" not in api.replace(field + " ==", ""), field
