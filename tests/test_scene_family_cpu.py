"""The generated scene family (tests/scene_family.py) does what it is here for, on the CPU oracle alone:
every case is a scene whose pixel-centre primary rays mostly hit, on at least four materials, without a
NaN sample; the two tie cases have exact ties over a tenth of their hits; the rounded coordinates pass
the scene compiler bit for bit; and the trailing steps' rule (csrc/trail_rule_test.cpp --scene) holds on
every sphere/box case of at most 8 primitives, plain and under the address and undefined-behaviour
sanitizers (the stand-alone program with its own main: nothing of it is loaded into Python).

These are conditions on the family, not measurements of the kernels: a layout that misses one is
changed, the condition is not."""
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle

from . import scene_family as sf
from .conftest import ROOT

CSRC = os.path.join(ROOT, "raymarchrenderer_amd", "csrc")
ALL = sorted(sf.CASES)


def test_the_family_has_the_cases():
    assert len(sf.CASES) == 16 and sf.GLASS in sf.CASES
    assert sorted(sf.RULE_CASES) == sorted(n for n in sf.CASES if n != sf.GLASS and len(sf.prims(n)) <= 8)
    assert len(sf.RULE_CASES) == 12
    for name, n in (("unit4", 4), ("unit", 5), ("ties", 8), ("loop20_offset", 20), ("bvh40_offset", 40), ("bvh40s_scale", 40)):
        assert len(sf.prims(name)) == n, name
    assert all(k == "s" for k, _, _, _ in sf.prims("bvh40s_scale")[5:])
    assert sf.max_dist("large") == 200000.0 and sf.max_dist("small") == 1000.0 and sf.params("bvh40s_scale").max_dist == 30000.0


@pytest.mark.parametrize("name", ALL)
def test_primary_rays_hit_four_materials(name):
    e, dirs, t, ident, pos = sf.primary_hits(name)
    x0, y0, x1, y1 = sf.RECT0
    assert len(dirs) == (x1 - x0) * (y1 - y0)
    hit = ident >= 0
    ids = sorted(set(int(i) for i in ident[hit]))
    print("%s: %.3f of %d primary rays hit, material ids %s" % (name, hit.mean(), len(hit), ids))
    assert hit.mean() >= 0.8, name
    assert len(ids) >= 4, (name, ids)


@pytest.mark.parametrize("name", ALL)
def test_no_oracle_sample_is_nan(name):
    cpu = oracle.Oracle(sf.tables(name), sf.params(name), sf.view(name), sf.W0, sf.H0).trace_samples(sf.times(), sf.RECT0)
    assert not np.isnan(cpu).any(), "%s: %d NaN values" % (name, np.isnan(cpu).sum())
    assert (cpu[..., :3] > 0).any(), name


@pytest.mark.parametrize("name", ["ties", "ties_offset"])
def test_tie_cases_have_exact_ties(name):
    share, hits = sf.exact_tie_share(name)
    print("%s: %.3f of %d primary hits have their two smallest primitive distances equal" % (name, share, hits))
    assert hits > 500 and share >= 0.10, (name, share, hits)


@pytest.mark.parametrize("name", ALL)
def test_rounded_scene_survives_the_compiler(name):
    """compile_scene quantises the v1 format's literals to six decimals; the generator's float32 values pass
    unchanged, centre and half-extent, and so does the transformed eye through the view."""
    tb = sf.tables(name)
    want = sf.prims(name)
    assert len(tb.prims) == len(want)
    for p, (kind, mat, c, r) in zip(tb.prims, want):
        assert np.array(list(p.c), np.float32).tobytes() == np.array(c, np.float32).tobytes(), (name, list(p.c), c)
        assert np.array(list(p.r), np.float32).tobytes() == np.array(r, np.float32).tobytes(), (name, list(p.r), r)
        assert p.mat_id == mat
    base, s, T, G = sf.CASES[name]
    if base != "glass":
        # rounded once: the float32 nearest the exact s x + T (the unit coordinates are short decimals, so
        # the product in double is the decimal's nearest double, well within a float32's half-ulp of exact)
        for (kind, mat, c, r), (_, _, c0, r0) in zip(want, sf._layout(name)):
            assert c == tuple(float(np.float32(s * c0[k] + T[k])) for k in range(3))
    assert np.array_equal(sf.view(name)[:3], np.asarray(sf.eye(name), np.float32))


def _rule(target, path):
    p = subprocess.run([os.path.join(CSRC, "build", target), "--scene", path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:]
    lines = p.stdout.splitlines()
    assert lines[-1] == "ok" and "FAIL" not in p.stdout, p.stdout[-4000:]
    for word in ("Sanitizer", "runtime error"):
        assert word not in p.stdout, p.stdout[-4000:]
    rows = [l for l in lines if " triples " in l]
    assert len(rows) == 1, p.stdout[-4000:]
    w = rows[0].split()
    return rows[0], int(w[w.index("triples") + 1]), int(w[w.index("accepted") + 1])


def _rule_on_family(target, tmp_path):
    subprocess.run(["make", "-s", "-C", CSRC, target], check=True, timeout=600)
    for name in sf.RULE_CASES:
        path = str(tmp_path / (name + ".txt"))
        sf.write_rule_scene(name, path)
        row, triples, accepted = _rule(target, path)
        print(row)
        assert row.startswith(name + " maxDist %g:" % sf.max_dist(name)), row
        assert triples >= 200000, row
        if name == "unit":
            assert accepted > 0, row


def test_trail_rule_on_the_family(tmp_path):
    _rule_on_family("trail_rule_test", tmp_path)


def test_trail_rule_on_the_family_sanitized(tmp_path):
    from .test_accel_cpu import _sanitizers_work
    if not _sanitizers_work(str(tmp_path)):
        pytest.skip("a one-line program does not build or start under -fsanitize=address,undefined")
    _rule_on_family("trail_rule_test_san", tmp_path)


def test_rule_scene_file_is_hex_floats(tmp_path):
    path = tmp_path / "offset_1000.txt"
    sf.write_rule_scene("offset_1000", str(path))
    lines = path.read_text().splitlines()
    assert float.fromhex(lines[0]) == 1000.0 and len(lines) == 1 + 5
    for l, (kind, mat, c, r) in zip(lines[1:], sf.prims("offset_1000")):
        w = l.split()
        assert w[0] == kind and [float.fromhex(x) for x in w[1:]] == [float(mat)] + list(c) + list(r)


def test_rule_program_refuses_a_broken_file(tmp_path):
    subprocess.run(["make", "-s", "-C", CSRC, "trail_rule_test"], check=True, timeout=600)
    path = tmp_path / "broken.txt"
    path.write_text("0x1.f4p+9\nb 0x0p+0 0x1p+0\n")
    p = subprocess.run([os.path.join(CSRC, "build", "trail_rule_test"), "--scene", str(path)], stdout=subprocess.PIPE, text=True, timeout=60)
    assert p.returncode != 0 and "FAIL" in p.stdout and "ok" not in p.stdout.splitlines()
