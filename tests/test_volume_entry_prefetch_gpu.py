"""The entry-prefetch schedule of the metric stream in the collocated-gradient one-wavefront stiffness kernels (deg_quad = deg <= 7,
streamed metric: stiffness_wave_eo_kernel / stiffness_wave_eo_multi_kernel, wave_eo_load_element in d4est_hip_volume.hip).

Tuning key 16 (D4EST_HIP_TUNE_STIFFNESS_ENTRY) switches one plan between the first schedule (0: the first metric plane is requested
before the last forward contraction) and the entry-prefetch schedule (1: the first planes are requested at kernel entry).  Both run the
same arithmetic in the same order, so the results must agree bit for bit.  The hazards are per wavefront (which lanes request what,
and when), hence the small meshes: 8 elements, 61 elements (a partial last workgroup wherever several elements share a wavefront) and
a plan with p = 3 and p = 7 interleaved (strides from the lists, the one-launch kernel of several buckets, wave-uniform strides)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-12
AFFINE, ENTRY = 7, 16   # tuning keys
GUARD_BITS = 0x7FF8000000000BAD   # a quiet NaN with a payload no arithmetic produces


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _mesh(kind, deg):
    from disco4est_amd import mesh as M
    if kind == "8":
        return M.BrickMesh(1, deg)
    if kind == "61":
        return M.BrickMesh(2, deg, count=61)
    assert kind == "mixed"
    return M.BrickMesh(2, np.where(np.arange(64) % 2 == 0, 3, 7))


def _general_plan(m, J, rst):
    from disco4est_amd import Plan
    plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, m.quad_type)
    plan.set_geometry(J, rst)
    plan.set_tuning(AFFINE, 0)
    return plan


def _random_u(n, dev, seed):
    return _t(np.random.default_rng(seed).standard_normal(n), dev)


def _apply(plan, du):
    import torch
    out = torch.full_like(du, float("nan"))
    plan.apply_stiffness_matrix(du, out)
    torch.cuda.synchronize()
    return out


def _both_schedules(plan, du, kernel, tag):
    """A u on the first schedule and on the entry-prefetch schedule of one plan; checks that last_kernel() names what was launched"""
    outs = []
    for value in (0, 1):
        plan.set_tuning(ENTRY, value)
        outs.append(_apply(plan, du))
        name = plan.last_kernel()
        assert kernel in name and "cg" in name, (tag, value, name)
        assert ("entry" in name) == (value == 1), (tag, value, name)
    plan.set_tuning(ENTRY, -1)
    return outs


@pytest.mark.parametrize("kind", ["8", "61"])
@pytest.mark.parametrize("deg", [1, 2, 3, 4, 5, 6, 7])
def test_schedules_bit_identical(gpu, hiplib, deg, kind):
    import torch
    from disco4est_amd import mesh as M
    m = _mesh(kind, deg)
    J, rst = m.geometry(M.SineMap(0.05))
    plan = _general_plan(m, J, rst)
    du = _random_u(m.local_nodes, gpu, 1000 + deg)
    parent, new = _both_schedules(plan, du, "stiffness_wave_eo_kernel<%d,%d," % (deg + 1, deg + 1), (deg, kind))
    assert torch.isfinite(parent).all() and torch.isfinite(new).all()
    assert torch.equal(new, parent)
    plan.destroy()


def test_schedules_bit_identical_mixed_degrees(gpu, hiplib):
    import torch
    from disco4est_amd import mesh as M
    m = _mesh("mixed", None)
    J, rst = m.geometry(M.SineMap(0.05))
    plan = _general_plan(m, J, rst)
    du = _random_u(m.local_nodes, gpu, 37)
    parent, new = _both_schedules(plan, du, "stiffness_wave_eo_multi_kernel<general", "mixed")
    assert torch.isfinite(parent).all() and torch.isfinite(new).all()
    assert torch.equal(new, parent)
    plan.destroy()


@pytest.mark.parametrize("kind", ["8", "61"])
@pytest.mark.parametrize("deg", [3, 7])
def test_default_schedule_oracle_parity(gpu, hiplib, oracle, deg, kind):
    """what a plan runs when nobody sets key 16, against the CPU oracle; the default is the entry-prefetch schedule at p = 7"""
    from disco4est_amd import mesh as M
    m = _mesh(kind, deg)
    mp = M.SineMap(0.05)
    J, rst = m.geometry(mp)
    u = m.field(mp)
    ref = oracle.apply_stiffness(m, J, rst, u, nthreads=4)
    plan = _general_plan(m, J, rst)
    got = _apply(plan, _t(u, gpu)).cpu().numpy()
    name = plan.last_kernel()
    assert ("entry" in name) == (deg == 7), name
    err = _rel(got, ref)
    print("p=%d, %s elements, %s: rel-inf error vs oracle %.3e" % (deg, kind, name, err))
    assert np.isfinite(got).all()
    assert err <= RTOL
    plan.destroy()


@pytest.mark.parametrize("deg", [1, 2, 3, 4, 5, 6, 7])
def test_guard_bands(gpu, hiplib, deg):
    """A u inside NaN guard bands on both sides, and the metric followed by a NaN guard: the plan gets one more element of the same
    degree behind its 60 real ones, whose geometry is NaN -- its metric block is the trailing guard of the metric buffer, and its nodes
    lie behind the trailing guard band of A u.  A metric value requested by a lane that has no element, and consumed later, would
    put a NaN into A u of a real element; a store outside an element's nodes would change a guard band."""
    import torch
    from disco4est_amd import Plan, mesh as M
    m = M.BrickMesh(2, deg, count=60)
    J, rst = m.geometry(M.SineMap(0.05))
    n3 = (deg + 1) ** 3
    real_n, real_q = m.local_nodes, m.local_nodes_quad
    rng = np.random.default_rng(2000 + deg)
    u = rng.standard_normal(real_n)

    plain = _general_plan(m, J, rst)
    plain.set_tuning(ENTRY, 1)
    want = _apply(plain, _t(u, gpu))
    plain.destroy()

    G = max(2 * n3, 256)
    last = G + real_n + G                           # the NaN-geometry element's nodes
    nodal_stride = np.concatenate([m.nodal_stride + G, [last]]).astype(np.int32)
    quad_stride = np.concatenate([m.quad_stride, [real_q]]).astype(np.int32)
    degs = np.full(m.n_elements + 1, deg, dtype=np.int32)
    Jg = np.concatenate([J, np.full(n3, np.nan)])
    rstg = np.concatenate([rst.reshape(9, real_q), np.full((9, n3), np.nan)], axis=1).reshape(-1)
    plan = Plan(degs, degs, nodal_stride, quad_stride, m.quad_type)
    assert plan.local_nodes == last + n3 and plan.local_nodes_quad == real_q + n3
    plan.set_geometry(Jg, rstg)
    plan.set_tuning(AFFINE, 0)
    ug = np.zeros(plan.local_nodes)
    ug[G:G + real_n] = u
    ug[last:] = 1.0
    du = _t(ug, gpu)
    for value in (1, 0):
        plan.set_tuning(ENTRY, value)
        out = torch.empty_like(du)
        out.view(torch.int64).fill_(GUARD_BITS)
        plan.apply_stiffness_matrix(du, out)
        torch.cuda.synchronize()
        name = plan.last_kernel()
        assert ("entry" in name) == (value == 1), name
        bits = out.view(torch.int64)
        assert (bits[:G] == GUARD_BITS).all(), (deg, name, "leading guard band of A u was written")
        assert (bits[G + real_n:last] == GUARD_BITS).all(), (deg, name, "trailing guard band of A u was written")
        inner = out[G:G + real_n]
        assert not torch.isnan(inner).any(), (deg, name)
        assert torch.equal(inner, want), (deg, name)
        tail = out[last:]
        assert torch.isnan(tail).all() and not (tail.view(torch.int64) == GUARD_BITS).any(), (deg, name, "the guard element's metric is not NaN")
    plan.destroy()
