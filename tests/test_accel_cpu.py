"""Scene acceleration and launch planning on the host (csrc/accel.cpp), checked on the CPU by the
stand-alone program csrc/accel_test.cpp, linked with the HIP-free units only (scene.cpp, grid.cpp,
accel.cpp): the BVH's structure, the escape boxes' coverage and inflation, the launch plan's bounds,
the grouping of deferred calls, and the record tests/golden/accel_record.json (digests of the tables
and the error constants as the parent of the split computed them). Run once plain and once under the
address and undefined-behaviour sanitizers; no GPU, no Python in the program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raymarchrenderer_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SAN = ["-Xarch_host", "-fsanitize=address,undefined"]


def _run(target):
    subprocess.run(["make", "-s", "-C", CSRC, target], check=True, timeout=600)
    p = subprocess.run([os.path.join(CSRC, "build", target), ROOT], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:]
    assert "accel_test ok" in p.stdout, p.stdout[-4000:]
    for word in ("Sanitizer", "runtime error"):
        assert word not in p.stdout, p.stdout[-4000:]


def test_accel_host_checks():
    _run("accel_test")


def _sanitizers_work(tmp):
    """A one-line program builds and starts under the sanitizers."""
    src = os.path.join(tmp, "one.cpp")
    with open(src, "w") as f:
        f.write("int main() { return 0; }\n")
    exe = os.path.join(tmp, "one")
    try:
        subprocess.run([HIPCC] + SAN + [src, "-o", exe], check=True, timeout=300,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return subprocess.run([exe], timeout=60).returncode == 0
    except (OSError, subprocess.SubprocessError):
        return False


def test_accel_host_checks_sanitized(tmp_path):
    if not _sanitizers_work(str(tmp_path)):
        pytest.skip("a one-line program does not build or start under -fsanitize=address,undefined")
    _run("accel_test_san")
