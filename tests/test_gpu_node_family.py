"""The kernels on the generated node-program family (tests/node_family.py): every object node, products and
quotients of variables, variable centres and radii, domain_repeat with negative / y / zero periods, all 16
variables, program materials, a program among 40 primitives, and objects that are NaN or +-inf beside
finite ones. Each case runs through the table interpreter (obj_node / run_material of the ahead-of-time
kernels, rmr_set_jit 0) and through the generated straight-line code of the hipRTC kernels (rmr_set_jit 1; the
query kernels behind eval_map and cast_rays are ahead-of-time code in both modes),
and is compared with the CPU oracle bit for bit (NaN equals NaN); nothing is left out and nothing has a
tolerance:

  rmr_eval_map at node_family.edge_points: the per-node check (zeros of both signs, the repeat lattice and
      its float neighbours, huge, overflowing, tiny and denormal coordinates, NaN and infinite distances);
  rmr_cast_rays on 1,000 rays, with and without normals (march and getNormal);
  trace_samples over the rect;
  render_spp under both kernels and rmr_trace_rays on the 1,000 rays, for the case with program materials
      and the case of 40 primitives.

tests/test_node_family_cpu.py shows on the oracle alone that the cases are worth rendering and holds the
oracle's map to a float64 statement."""
import numpy as np
import pytest

from oracle import oracle

from . import node_family as nf
from .denoise_ref import far_hit_rule
from .test_gpu_parity import same_bits
from .test_gpu_query import _check_cast, _map, _march
from .test_gpu_rays import _ray_list

pytestmark = pytest.mark.gpu

CASES = list(nf.CASES)
FULL_CASES = ["trig_mat", "table40"]   # program materials; more than 32 primitives


def _load(r, name):
    r.set_image_size(nf.W, nf.H)
    r.reload()
    r.load_scene(nf.scene(name), "rm1")
    r.set_params(nf.params())
    r.set_view(nf.view())
    r.set_env_map(None)


def _under_both(r, name, body, traces=True):
    """body(jit) on the loaded case under the table kernels (rmr_set_jit 0), then under the specialised ones
    (rmr_set_jit 1); mode 2 afterwards. Every trace launch of mode 1 is a hipRTC kernel, none of mode 0; the
    query kernels (eval_map, cast_rays) are ahead-of-time code in both modes and launch no trace kernel."""
    _load(r, name)
    try:
        for jit in (0, 1):
            r.set_jit(jit)
            r.reset_stats()
            body(jit)
            st = r.stats()
            assert st.jit_launches == (st.trace_launches if jit else 0), (name, jit, st.jit_launches, st.trace_launches)
            assert (st.trace_launches > 0) == traces, (name, jit, st.trace_launches)
            if traces:
                assert (st.jit_launches > 0) == bool(jit), (name, jit, st.jit_launches)
    finally:
        r.set_jit(2)
        r.set_kernel(0)


def _assert_same(got, want, what):
    eq = same_bits(got, want)
    eq = eq.reshape(eq.shape[0], -1).all(axis=1) if eq.ndim > 1 else eq
    assert eq.all(), "%s: %d/%d differ; first %d gpu=%s cpu=%s" % (
        what, (~eq).sum(), len(eq), np.argmin(eq), np.asarray(got)[np.argmin(eq)], np.asarray(want)[np.argmin(eq)])


_rays = {}


def _ray_case(name):
    """The case's 1,000 rays and the oracle's raw march of each, once per case."""
    if name not in _rays:
        tb = nf.tables(name)
        rays = _ray_list(tb, seed=100 + CASES.index(name))
        _rays[name] = (rays,) + _march(tb, nf.params(), rays)
    return _rays[name]


@pytest.mark.parametrize("name", CASES)
def test_eval_map_bitexact(renderer, name):
    pts = nf.edge_points(name)
    want = _map(nf.tables(name), nf.params().max_dist, pts)
    # the list holds what it is there for (the oracle alone decides)
    assert (want[:, 0] < 0.001).sum() >= 50 and (want[:, 0] > 0.001).sum() >= 1000
    if name == "nan_objects":
        assert np.isneginf(want[:, 0]).sum() >= 10 and not np.isnan(want[:, 0]).any()

    def body(jit):
        got = renderer.eval_map(pts)
        eq = same_bits(got, want).all(axis=1)
        assert eq.all(), "%s jit %d: %d/%d points differ; first %d: p %s gpu %s oracle %s" % (
            name, jit, (~eq).sum(), len(pts), np.argmin(eq), pts[np.argmin(eq)], got[np.argmin(eq)], want[np.argmin(eq)])

    _under_both(renderer, name, body, traces=False)


@pytest.mark.parametrize("name", nf.RAY_CASES)
def test_cast_rays_bitexact(renderer, name):
    rays, t, ident = _ray_case(name)
    tb, prm = nf.tables(name), nf.params()
    want_id = far_hit_rule(t, ident, prm.max_dist)
    n_hit, n_miss = int(((want_id >= 0) & (t > 0)).sum()), int((want_id < 0).sum())
    print("%s: %d hits with t > 0, %d misses" % (name, n_hit, n_miss))
    assert n_hit >= 200 and n_miss >= 300

    def body(jit):
        hits = renderer.cast_rays(rays)
        _check_cast(hits, rays, tb, prm, t, ident, "%s jit %d" % (name, jit))
        vis = renderer.cast_rays(rays, normals=False)
        _check_cast(vis, rays, tb, prm, t, ident, "%s jit %d (no normals)" % (name, jit), normals=False)

    _under_both(renderer, name, body, traces=False)


@pytest.mark.parametrize("name", CASES)
def test_trace_samples_bitexact(renderer, name):
    cpu = oracle.Oracle(nf.tables(name), nf.params(), nf.view(), nf.W, nf.H).trace_samples(nf.times(), nf.RECT)
    assert not np.isnan(cpu).any() and len(np.unique(cpu[..., :3].reshape(-1, 3), axis=0)) > 10

    def body(jit):
        gpu = renderer.trace_samples(nf.times(), nf.RECT)
        _assert_same(gpu[..., :3].reshape(-1, 3), cpu[..., :3].reshape(-1, 3), "%s jit %d: trace_samples" % (name, jit))

    _under_both(renderer, name, body)


@pytest.mark.parametrize("name", FULL_CASES)
def test_render_spp_bitexact(renderer, name):
    """The running mean under the persistent kernel (rmr_set_kernel 0), table and specialised, and under the
    per-path kernel (rmr_set_kernel 1), which has no hipRTC form: the jit mode launches nothing there."""
    cpu = oracle.Oracle(nf.tables(name), nf.params(), nf.view(), nf.W, nf.H).render(nf.times(), rect=nf.RECT)

    def body(jit):
        renderer.reload()
        renderer.render_spp(nf.times(), nf.RECT)
        _assert_same(renderer.read_accum().reshape(-1, 4), cpu.reshape(-1, 4), "%s jit %d: render_spp" % (name, jit))

    _under_both(renderer, name, body)
    _load(renderer, name)
    try:
        renderer.set_kernel(1)
        renderer.set_jit(0)
        renderer.reset_stats()
        renderer.render_spp(nf.times(), nf.RECT)
        st = renderer.stats()
        assert st.trace_launches > 0 and st.jit_launches == 0
        _assert_same(renderer.read_accum().reshape(-1, 4), cpu.reshape(-1, 4), "%s: render_spp, per-path kernel" % name)
    finally:
        renderer.set_kernel(0)
        renderer.set_jit(2)


@pytest.mark.parametrize("name", FULL_CASES)
def test_trace_rays_bitexact(renderer, name):
    rays = _ray_case(name)[0]
    orc = oracle.Oracle(nf.tables(name), nf.params(), nf.view(), nf.W, nf.H)
    want = np.array([orc.trace(int(q["gx"]), int(q["gy"]), float(q["time"]), q["o"], q["d"]) for q in rays])
    assert len(np.unique(want, axis=0)) > 3, "a degenerate ray list"

    def body(jit):
        got = renderer.trace_rays(rays)
        assert (got[:, 3] == 1).all()
        _assert_same(got[:, :3], want, "%s jit %d: trace_rays" % (name, jit))

    _under_both(renderer, name, body)
