"""The collocated-gradient form of the one-wavefront stiffness body (deg_quad = deg <= 7: stiffness_wave_eo_element_cg, 12 one-dimensional
products per thread instead of 16) against the CPU oracle, and against the 16-product body it replaces.

Both bodies compute the same operator; they differ by re-association only.  Each is therefore held to the oracle at the tolerance of
tests/test_volume_gpu.py (1e-12 relative to ||A u||_inf); the distance between the two is printed, not bounded on its own.
Tuning key 1 (D4EST_HIP_TUNE_STIFFNESS_WAVE) = 12 selects the 16-product body in the same kernels."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-12
WAVE, AFFINE, FACE_DIRECT = 1, 7, 11   # tuning keys
OLD_BODY = 12


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _both_bodies(plan, apply, want, tag):
    """runs `apply` with the collocated body (default) and with the 16-product body; returns (new, old) and checks the kernel names"""
    outs = []
    for key, cg in ((-1, True), (OLD_BODY, False)):
        plan.set_tuning(WAVE, key)
        got = apply()
        name = plan.last_kernel()
        assert want in name, (tag, name)
        assert ("cg" in name) == cg, (tag, key, name)
        assert np.isfinite(got).all(), (tag, name)
        outs.append(got)
    plan.set_tuning(WAVE, -1)
    return outs


@pytest.mark.parametrize("curved,path", [(True, "general"), (False, "general"), (False, "affine")])
@pytest.mark.parametrize("deg", [1, 2, 3, 4, 5, 6, 7])
def test_stiffness_cg_parity(gpu, hiplib, oracle, deg, curved, path):
    """N = 2 ... 8, SineMap and brick geometry, streamed metric and (brick only) the affine path: both bodies against the oracle"""
    import torch
    from disco4est_amd import Plan, mesh as M
    m = M.BrickMesh(1, deg, count=7)   # 7 elements: a ragged last wavefront where several elements share one
    mp = M.SineMap(0.06) if curved else None
    J, rst = m.geometry(mp)
    u = m.field(mp)
    ref = oracle.apply_stiffness(m, J, rst, u, nthreads=4)
    plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, m.quad_type)
    plan.set_geometry(J, rst)
    if path == "general":
        plan.set_tuning(AFFINE, 0)
    du = _t(u, gpu)

    def apply():
        out = torch.full_like(du, float("nan"))
        plan.apply_stiffness_matrix(du, out)
        return out.cpu().numpy()

    new, old = _both_bodies(plan, apply, "stiffness_wave_eo_kernel", (deg, curved, path))
    assert ("affine" in plan.last_kernel()) == (path == "affine")
    e_new, e_old = _rel(new, ref), _rel(old, ref)
    print("p=%d %s %s: new vs oracle %.3e, old vs oracle %.3e, new vs old %.3e" % (deg, "curved" if curved else "brick", path, e_new, e_old, _rel(new, old)))
    assert e_new <= RTOL
    assert e_old <= RTOL
    plan.destroy()


@pytest.mark.parametrize("mass", [False, True])
@pytest.mark.parametrize("curved", [True, False])
@pytest.mark.parametrize("deg", [1, 2, 3, 4, 5, 6, 7])
def test_whole_operator_cg_parity(gpu, hiplib, oracle, deg, curved, mass):
    """apply_aij / apply_lhs with a zeroth-order coefficient through the whole-operator kernel, whose volume stage is the same body
    (streamed metric on the curved mesh, affine on the brick; MASS: V u passes through registers), against the oracle.  With the
    16-product body selected the volume term runs in its own kernel beside the direct face kernel."""
    import torch
    from disco4est_amd import Plan, mesh as M
    m = M.BrickMesh(1, deg)
    mp = M.SineMap(0.05) if curved else None
    J, rst = m.geometry(mp)
    sides = m.build_sides(mp)
    u = m.field(mp)
    ref = oracle.apply_aij(m, J, rst, sides, u, penalty_prefactor=7.5, penalty_fcn=0, nthreads=4)
    coeff = None
    if mass:
        uq = oracle.interpolate(m, u)
        coeff = 1.0 + uq * uq
        ref = ref + oracle.apply_weighted_mass(m, J, coeff, u)
    plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, m.quad_type)
    plan.set_geometry(J, rst)
    plan.set_faces(sides, 7.5, 0)
    plan.set_tuning(FACE_DIRECT, 2)
    du = _t(u, gpu)
    if mass:
        plan.set_lhs_coefficient(_t(coeff, gpu))
    outs = []
    for key, path in ((-1, "direct+volume"), (OLD_BODY, "direct")):
        plan.set_tuning(WAVE, key)
        assert plan.face_path() == path, (key, plan.face_path())
        out = torch.full_like(du, float("nan"))
        (plan.apply_lhs if mass else plan.apply_aij)(du, out)
        if key == -1:
            name = plan.last_kernel()
            assert "faces_direct_kernel" in name and "cg" in name, name
            assert ("affine" in name) == (not curved), name
        outs.append(out.cpu().numpy())
    new, old = outs
    e_new, e_old = _rel(new, ref), _rel(old, ref)
    print("p=%d %s mass=%d: new vs oracle %.3e, old vs oracle %.3e, new vs old %.3e" % (deg, "curved" if curved else "brick", mass, e_new, e_old, _rel(new, old)))
    assert np.isfinite(new).all() and np.isfinite(old).all()
    assert e_new <= RTOL
    assert e_old <= RTOL
    plan.destroy()


@pytest.mark.parametrize("curved", [True, False])
@pytest.mark.parametrize("lo,hi,kernel", [(3, 7, "stiffness_wave_eo_multi_kernel"), (3, 9, "stiffness_all_multi_kernel")])
def test_mixed_degree_one_launch_cg_parity(gpu, hiplib, oracle, lo, hi, kernel, curved):
    """a mixed p = 3 ... 7 plan through the one-launch kernel of the one-wavefront buckets, and p = 3 ... 9 through the kernel that takes
    the multi-wave buckets along: both bodies, element by element against the oracle"""
    import torch
    from disco4est_amd import Plan, mesh as M
    deg = lo + (np.arange(512) * 3) % (hi - lo + 1)
    m = M.BrickMesh(3, deg)
    mp = M.SineMap(0.05) if curved else None
    J, rst = m.geometry(mp)
    u = m.field(mp)
    ref = oracle.apply_stiffness(m, J, rst, u, nthreads=8)
    plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, m.quad_type)
    plan.set_geometry(J, rst)
    if kernel == "stiffness_all_multi_kernel":
        plan.set_tuning(AFFINE, 0)   # (that kernel serves the streamed-metric buckets)
    du = _t(u, gpu)

    def apply():
        out = torch.full_like(du, float("nan"))
        plan.apply_stiffness_matrix(du, out)
        return out.cpu().numpy()

    new, old = _both_bodies(plan, apply, kernel, (lo, hi, curved))
    print("p=%d..%d %s: new vs oracle %.3e, old vs oracle %.3e, new vs old %.3e" % (lo, hi, "curved" if curved else "brick", _rel(new, ref), _rel(old, ref), _rel(new, old)))
    for got in (new, old):
        assert _rel(got, ref) <= RTOL
        for e in range(m.n_elements):   # so that a small-p element cannot hide behind a large-p norm
            s = m.nodal_stride[e]; n3 = (deg[e] + 1) ** 3
            assert _rel(got[s:s + n3], ref[s:s + n3]) <= 10 * RTOL, (e, deg[e])
    plan.destroy()
