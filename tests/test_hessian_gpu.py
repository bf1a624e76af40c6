"""GPU tests of the device Laplacian at the quadrature nodes (d4est_hip_plan_set_hessian_* / d4est_hip_hessian_trace,
csrc/d4est_hip_hessian.hip) against the numpy restatement of src/dGMath/d4est_hessian.c (tests/dense_hessian.py): the brick, analytic
and numerical coefficient forms, every degree class of the apply kernel, bitwise repeatability, isolation of plans that never ask
for it, and the LDS limit.

Tolerance.  Second derivatives amplify rounding by roughly N^4, so no bound is derived: per case the dense reference is evaluated
in long double and in float64 in two summation orders (the reference's nine-term order and the folded symmetric one), and the device
result must lie within 4 x the larger float64 error against the long-double result, with a floor of 64 eps max|Lap u|
(dense_hessian.error_bound).  The bounds the CPU gave (absolute, with max|Lap u| of the case):
    brick p=1 inc=0 qt=0               bound 0.00e+00   max|Lap u| 0.00e+00
    brick p=2 inc=0 qt=0               bound 5.53e-14   max|Lap u| 3.36e+00
    brick p=3 inc=0 qt=0               bound 2.56e-13   max|Lap u| 5.53e+00
    brick p=7 inc=0 qt=0               bound 8.20e-12   max|Lap u| 5.89e+00
    brick p=8 inc=0 qt=0               bound 1.74e-11   max|Lap u| 5.91e+00
    brick p=11 inc=0 qt=0              bound 5.38e-11   max|Lap u| 5.95e+00
    brick p=15 inc=0 qt=0              bound 2.61e-10   max|Lap u| 5.97e+00
    brick p=19 inc=0 qt=0              bound 7.05e-10   max|Lap u| 5.98e+00
    brick p=2 inc=1 qt=0               bound 6.85e-14   max|Lap u| 3.38e+00
    brick p=2 inc=2 qt=0               bound 6.92e-14   max|Lap u| 3.41e+00
    brick p=7 inc=1 qt=0               bound 8.43e-12   max|Lap u| 5.91e+00
    brick p=7 inc=2 qt=0               bound 9.13e-12   max|Lap u| 5.93e+00
    brick p=11 inc=1 qt=0              bound 6.29e-11   max|Lap u| 5.95e+00
    brick p=11 inc=2 qt=0              bound 6.79e-11   max|Lap u| 5.96e+00
    brick p=15 inc=1 qt=0              bound 3.32e-10   max|Lap u| 5.97e+00
    brick p=15 inc=2 qt=0              bound 3.13e-10   max|Lap u| 5.98e+00
    brick p=4 inc=1 qt=1               bound 1.60e-12   max|Lap u| 6.04e+00
    brick mixed p=2..9                 bound 2.10e-11   max|Lap u| 5.93e+00
    13tree-p4                          bound 9.23e-14   max|Lap u| 1.43e+00
    13tree-p9                          bound 1.80e-12   max|Lap u| 1.31e+00
    13tree-compact-p4                  bound 8.58e-12   max|Lap u| 6.04e+02
    13tree-compact-p9                  bound 1.06e-11   max|Lap u| 7.46e+02
    sphere-hole-p4                     bound 3.70e-14   max|Lap u| 1.43e+00
    sphere-hole-compact-both-p4        bound 8.58e-12   max|Lap u| 6.04e+02
    7tree-p3                           bound 3.37e-14   max|Lap u| 5.01e-01
    numerical p=4 rst=True             bound 1.48e-12   max|Lap u| 5.82e+00
    numerical p=4 rst=False            bound 1.49e-12   max|Lap u| 5.82e+00
    numerical p=8 rst=True             bound 3.62e-11   max|Lap u| 5.93e+00
    numerical p=8 rst=False            bound 3.63e-11   max|Lap u| 5.93e+00
"""
import numpy as np
import pytest

from tests import dense_hessian as DH

pytestmark = pytest.mark.gpu
EXTENTS = (0., 1., 0., 1., 0., 1.)


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _smooth(x, y, z):
    return np.sin(2.0 * x) * np.cos(y) + z ** 3 + x * y * z


def _device_trace(gpu, m, u, setup, calls=1):
    """the device result(s) of `calls` hessian_trace calls on a fresh plan prepared by setup(plan)"""
    import torch
    from disco4est_amd import Plan
    plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, m.quad_type)
    assert plan.hessian_info() == 0 and plan.hessian_supported()
    form = setup(plan)
    assert plan.hessian_info() == form
    du = _t(u, gpu)
    outs = []
    for _ in range(calls):
        out = torch.full((m.local_nodes_quad,), float("nan"), dtype=torch.float64, device=gpu)
        plan.hessian_trace(du, out)
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
    plan.destroy()
    return outs


def _check(name, got, d64, dld, u):
    bound, ref, errs = DH.error_bound(d64, dld, u)
    err = float(np.abs(got - ref).max())
    print("%s: device error %.3e, bound %.3e (float64 reference order %.3e, folded %.3e), max|Lap u| %.3e"
          % (name, err, bound, errs[0], errs[1], np.abs(ref).max()))
    assert np.isfinite(got).all()
    assert err <= bound, (name, err, bound)


# ---- brick ----------------------------------------------------------------------------------------------------------------------
BRICK = [(p, 0, 0) for p in (1, 2, 3, 7, 8, 11, 15, 19)] + [(p, inc, 0) for p in (2, 7, 11, 15) for inc in (1, 2)] + [(4, 1, 1)]


def _brick_case(gpu, name, m):
    u = _smooth(*m.nodal_coords())
    dq = np.ones(m.n_elements, dtype=np.int32)

    def setup(plan):
        plan.set_hessian_brick(dq, float(1 << m.level), EXTENTS)
        return 1
    got = _device_trace(gpu, m, u, setup)[0]
    _check(name, got, DH.DenseHessian(m, "brick"), DH.DenseHessian(m, "brick", dtype=np.longdouble), u)


@pytest.mark.parametrize("p,inc,quad_type", BRICK)
def test_brick(gpu, hiplib, p, inc, quad_type):
    """level 1, 8 elements: every degree class of the kernel (workgroups of 64, 128 and 256 threads, LDS above 64 KB at p >= 17),
    over-integration by one and two, and one Lobatto-quadrature plan"""
    from disco4est_amd import mesh as M
    _brick_case(gpu, "brick p=%d inc=%d qt=%d" % (p, inc, quad_type), M.BrickMesh(1, p, deg_quad_inc=inc, quad_type=quad_type))


def test_brick_mixed_degree(gpu, hiplib):
    """p = 2 ... 9 over the 8 elements: one bucket per element"""
    from disco4est_amd import mesh as M
    _brick_case(gpu, "brick mixed p=2..9", M.BrickMesh(1, np.arange(2, 10), deg_quad_inc=1))


# ---- analytic -------------------------------------------------------------------------------------------------------------------
def _analytic_cases():
    from disco4est_amd import forest as F
    c13, ch, c7 = F.cubed_sphere_13tree_connectivity, F.sphere_with_hole_connectivity, F.cubed_sphere_7tree_connectivity
    return {
        "13tree-p4": (c13, lambda: F.CubedSphere13Map(1.0, 2.0, 6.0), 2, 4),
        "13tree-p9": (c13, lambda: F.CubedSphere13Map(1.0, 2.0, 6.0), 2, 9),
        "13tree-compact-p4": (c13, lambda: F.CubedSphere13Map(1.0, 2.0, 20.0, compactify_outer=True), 2, 4),
        "13tree-compact-p9": (c13, lambda: F.CubedSphere13Map(1.0, 2.0, 20.0, compactify_outer=True), 2, 9),
        "sphere-hole-p4": (ch, lambda: F.SphereWithHoleMap(1.0, 2.0, 6.0), 3, 4),
        "sphere-hole-compact-both-p4": (ch, lambda: F.SphereWithHoleMap(1.0, 2.0, 20.0, compactify_outer=True, compactify_inner=True), 3, 4),
        "7tree-p3": (c7, lambda: F.CubedSphere7Map(1.0, 2.0), 1, 3),
    }


@pytest.mark.parametrize("name", ["13tree-p4", "13tree-p9", "13tree-compact-p4", "13tree-compact-p9", "sphere-hole-p4",
                                  "sphere-hole-compact-both-p4", "7tree-p3"])
def test_analytic(gpu, hiplib, name):
    """level 0 of each forest: outer, inner blended and inner plain wedges and the centre cube, with and without compactification"""
    from disco4est_amd import forest as F
    conn, mk, gtype, p = _analytic_cases()[name]
    mp = mk()
    fm = F.ForestMesh(conn(), 0, p, mp)
    params = (mp.R0, mp.R1, float(mp.compactify)) if gtype == 1 else mp.params
    x, y, z = fm.nodal_coords()
    u = _smooth(0.3 * x, 0.3 * y, 0.3 * z)
    tree, q, dq = fm.cells()

    def setup(plan):
        plan.set_hessian_analytic(gtype, params, tree, q, dq, fm.nf)
        return 2
    got = _device_trace(gpu, fm, u, setup)[0]
    _check(name, got, DH.DenseHessian(fm, "analytic", mapping=mp), DH.DenseHessian(fm, "analytic", dtype=np.longdouble, mapping=mp), u)


# ---- numerical ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [4, 8])
@pytest.mark.parametrize("with_rst", [True, False])
def test_numerical(gpu, hiplib, p, with_rst):
    """a curved brick from its node coordinates alone, dr/dx from the mesh's rst_xyz_quad or from the coordinates"""
    from disco4est_amd import mesh as M
    m = M.BrickMesh(1, p, deg_quad_inc=1)
    mp = M.SineMap(0.03)
    xyz = m.nodal_coords(mp)
    rst = m.geometry(mp)[1] if with_rst else None
    u = _smooth(*xyz)

    def setup(plan):
        plan.set_hessian_numerical(xyz, rst)
        return 3
    got = _device_trace(gpu, m, u, setup)[0]
    _check("numerical p=%d rst=%s" % (p, with_rst), got, DH.DenseHessian(m, "numerical", xyz=xyz, rst=rst),
           DH.DenseHessian(m, "numerical", dtype=np.longdouble, xyz=xyz, rst=rst), u)


def test_numerical_device_arrays(gpu, hiplib):
    """the same coefficients from device pointers as from host pointers, bit for bit"""
    from disco4est_amd import mesh as M
    m = M.BrickMesh(1, 4, deg_quad_inc=1)
    mp = M.SineMap(0.03)
    xyz = m.nodal_coords(mp)
    rst = m.geometry(mp)[1]
    u = _smooth(*xyz)
    dx, dr = _t(np.concatenate(xyz), gpu), _t(rst, gpu)
    a = _device_trace(gpu, m, u, lambda plan: plan.set_hessian_numerical(xyz, rst) or 3)[0]
    b = _device_trace(gpu, m, u, lambda plan: plan.set_hessian_numerical(dx, dr) or 3)[0]
    assert np.array_equal(a, b)


# ---- repeatability, isolation, limit ----------------------------------------------------------------------------------------------
def test_bitwise_repeat(gpu, hiplib):
    from disco4est_amd import forest as F
    mp = F.CubedSphere13Map(1.0, 2.0, 6.0)
    fm = F.ForestMesh(F.cubed_sphere_13tree_connectivity(), 0, 5, mp, deg_quad_inc=1)
    tree, q, dq = fm.cells()
    a, b = _device_trace(gpu, fm, fm.field(), lambda plan: plan.set_hessian_analytic(2, mp.params, tree, q, dq, fm.nf) or 2, calls=2)
    assert np.isfinite(a).all() and np.array_equal(a, b)


def test_plans_without_the_hessian_are_untouched(gpu, hiplib):
    """a plan that never calls set_hessian_* reports 0, and the operator of a twin plan that does is the same bit for bit"""
    import torch
    from disco4est_amd import Plan, mesh as M
    m = M.BrickMesh(1, 3, deg_quad_inc=1)
    mp = M.SineMap(0.05)
    J, rst = m.geometry(mp)
    sides = m.build_sides(mp)
    du = _t(m.field(mp), gpu)
    outs = []
    for with_hessian in (False, True):
        plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, 0)
        plan.set_geometry(J, rst)
        plan.set_faces(sides, 10.0, 0)
        if with_hessian:
            plan.set_hessian_numerical(m.nodal_coords(mp), rst)
            lap = torch.empty(m.local_nodes_quad, dtype=torch.float64, device=gpu)
            plan.hessian_trace(du, lap)
        assert plan.hessian_info() == (3 if with_hessian else 0)
        Au = torch.full_like(du, float("nan"))
        plan.apply_aij(du, Au)
        torch.cuda.synchronize()
        outs.append(Au.cpu().numpy())
        plan.destroy()
    assert np.isfinite(outs[0]).all() and np.array_equal(outs[0], outs[1])


def test_lds_limit(gpu, hiplib):
    """8 (N^3 + 3 N^2 + 9 N NQ) bytes <= 163840: every deg <= 19 fits, deg = deg_quad = 23 (165888 bytes) does not; asked without
    launching anything on the unsupported plan"""
    from disco4est_amd import Plan

    def supported(p, pq):
        n3, q3 = (p + 1) ** 3, (pq + 1) ** 3
        plan = Plan(np.array([p, 2]), np.array([pq, 2]), np.array([0, n3]), np.array([0, q3]), 0)
        ok = plan.hessian_supported()
        assert plan.hessian_info() == 0
        plan.destroy()
        return ok

    for p, pq in [(19, 19), (19, 21), (19, 23), (15, 17), (22, 23), (23, 23)]:
        n, nq = p + 1, pq + 1
        assert supported(p, pq) == (8 * (n ** 3 + 3 * n * n + 9 * n * nq) <= 160 * 1024), (p, pq)
    assert supported(19, 19) and not supported(23, 23)
