"""The fused device power term a (b + u)^k (d4est_hip_apply_nonlinear_term), its linearisation (d4est_hip_plan_linearise) and the
residual (d4est_hip_build_residual) against the oracle's interpolate / galerkin integral around tests/dense_nonlinear.py.
Tolerance 1e-12 relative to the reference's infinity norm: the project's fp64 bound for parity under re-association."""
import numpy as np
import pytest

from tests import dense_nonlinear as DN

pytestmark = pytest.mark.gpu

RTOL = 1e-12
MIXED = [2, 5, 3, 4, 5, 2, 4, 3]     # p = 2 ... 5 scattered over the 8 elements


def _t(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(gpu)


def _rel(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


class _Case:
    def __init__(self, gpu, deg, inc=0, level=1, faces=False, direct=None):
        from disco4est_amd import Plan, mesh as M
        self.gpu = gpu
        self.m = m = M.BrickMesh(level, np.array(deg, np.int32) if isinstance(deg, list) else deg, deg_quad_inc=inc)
        self.mp = mp = M.SineMap(0.03)
        self.J, self.rst = m.geometry(mp)
        self.plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, 0)
        if direct is not None:
            self.plan.set_tuning(11, direct)
        self.plan.set_geometry(self.J, self.rst)
        self.sides = None
        if faces:
            self.sides = m.build_sides(mp)
            self.plan.set_faces(self.sides, 10.0, 0)
        nq = m.local_nodes_quad
        self.a = -(0.5 + M.splitmix64_uniform(11, nq))
        self.b = 0.1 + 0.2 * M.splitmix64_uniform(12, nq)
        x, y, z = m.nodal_coords(mp)
        self.x, self.y, self.z = x, y, z

    def smooth(self, s):
        """a smooth nodal field in [0.75, 1.25]: b + V u stays inside [0.5, 2], where (b + u)^-8 is well-conditioned"""
        return 1.0 + 0.25 * np.sin(1.1 * self.x + 2.0 * self.y + 3.0 * self.z + s)

    def set_power(self, k, with_b):
        self.plan.set_nonlinear_power(_t(self.a, self.gpu), _t(self.b, self.gpu) if with_b else None, k)

    def term(self, u, beta=0, out0=None):
        import torch
        du = _t(u, self.gpu)
        out = torch.full_like(du, float("nan")) if out0 is None else _t(out0, self.gpu)
        self.plan.apply_nonlinear_term(du, out, beta)
        return out.cpu().numpy()


# (deg, deg_quad_inc, the one-kernel form): p in {1, 3, 7} the one-wavefront range and its limit, p = 8 the first multi-wave bucket, Nq != N
# with (p = 3) and without (p = 4: deg_quad = 5 has no compiled pair, the composed path) a kernel, a mixed-degree plan (one launch over
# its four buckets)
SHAPES = [(1, 0, True), (3, 0, True), (7, 0, True), (8, 0, True), (4, 1, False), (3, 1, True), (MIXED, 0, True)]
POWERS = [(5, False), (4, False), (-7, True), (-8, True), (1, True), (0, True)]


@pytest.mark.parametrize("deg,inc,fused", SHAPES, ids=lambda v: "mixed" if isinstance(v, list) else str(v))
def test_term_against_the_oracle(gpu, hiplib, oracle, deg, inc, fused):
    c = _Case(gpu, deg, inc)
    m = c.m
    assert c.plan.nonlinear_fused() == fused
    u = c.smooth(0.3)
    uq = oracle.interpolate(m, u)
    out0 = np.cos(3.0 * c.x - c.y) + 2.0
    for k, with_b in POWERS:
        bq = c.b if with_b else None
        base = uq if bq is None else bq + uq
        assert base.min() >= 0.5 and base.max() <= 2.0
        ref = oracle.apply_galerkin(m, c.J, DN.term(c.a, bq, uq, k))
        c.set_power(k, with_b)
        e0 = _rel(c.term(u), ref)                                # beta = 0 overwrites an out pre-filled with NaN
        e1 = _rel(c.term(u, 1, out0), out0 + ref)                # beta = 1 accumulates onto a non-zero out
        print("nonlinear term deg=%s inc=%d k=%d b=%s: rel-inf error beta=0 %.3e, beta=1 %.3e" % (deg, inc, k, with_b, e0, e1))
        assert e0 <= RTOL and e1 <= RTOL, (k, e0, e1)
    # k = 1, b = 0: the weighted mass matrix with coefficient a
    import torch
    c.set_power(1, False)
    wm = torch.empty(m.local_nodes, dtype=torch.float64, device=gpu)
    c.plan.apply_weighted_mass_matrix(_t(u, gpu), _t(c.a, gpu), wm)
    assert _rel(c.term(u), wm.cpu().numpy()) <= RTOL
    # the term switched off contributes zero
    c.plan.set_nonlinear_power(None, None, 0)
    assert np.array_equal(c.term(u), np.zeros(m.local_nodes))
    assert np.array_equal(c.term(u, 1, out0), out0)
    c.plan.destroy()


def test_power_values_are_captured(gpu, hiplib):
    """the plan keeps copies of a and b: the caller's tensors may change afterwards"""
    c = _Case(gpu, 3)
    da, db = _t(c.a, gpu), _t(c.b, gpu)
    c.plan.set_nonlinear_power(da, db, -7)
    u = c.smooth(0.1)
    first = c.term(u)
    da.fill_(float("nan")); db.fill_(float("nan"))
    assert np.array_equal(c.term(u), first)
    c.plan.destroy()


@pytest.mark.parametrize("direct", [0, 2])
@pytest.mark.parametrize("deg,level", [(7, 2), (3, 1), (9, 1)])
def test_linearise_sets_the_coefficient(gpu, hiplib, oracle, deg, level, direct):
    """after linearise(u0), apply_lhs = apply_aij + V^T W J c V with c = k a (b + V u0)^(k-1), on the separate-kernel path (tuning key
    11 = 0) and the whole-operator path (2), which reads the pre-combined w J c"""
    import torch
    c = _Case(gpu, deg, 0, level, faces=True, direct=direct)
    m, plan = c.m, c.plan
    k = -7
    c.set_power(k, True)
    v = _t(m.field(c.mp), gpu)
    lap = torch.empty_like(v)
    plan.apply_aij(v, lap)

    def expect(u0):
        c_ref = DN.dterm(c.a, c.b, oracle.interpolate(m, u0), k)
        wm = torch.empty_like(v)
        plan.apply_weighted_mass_matrix(v, _t(c_ref, gpu), wm)
        return lap + wm

    def got(u0=None):
        if u0 is not None:
            plan.linearise(_t(u0, gpu))
        out = torch.full_like(v, float("nan"))
        plan.apply_lhs(v, out)
        return out

    def rel(x, y):
        return float((x - y).abs().max() / y.abs().max())

    u0, u1 = c.smooth(0.0), c.smooth(1.7)
    r0, r1 = expect(u0), expect(u1)
    g0 = got(u0)
    print("linearise deg=%d level=%d key11=%d (%s): rel-inf error %.3e" % (deg, level, direct, plan.face_path(), rel(g0, r0)))
    assert rel(g0, r0) <= RTOL
    g1 = got(u1)                                               # a second linearisation: no stale w J c
    assert rel(g1, r1) <= RTOL
    assert float((g1 - g0).abs().max()) > 1e-3 * float((r0 - lap).abs().max())   # ... the change of u0 is visible in the term
    plan.set_lhs_coefficient(None)
    assert rel(got(), lap) <= RTOL                             # the term is off ...
    assert rel(got(u0), r0) <= RTOL                            # ... and linearise re-enables it
    # k = 0: the coefficient is zero
    c.set_power(0, True)
    assert rel(got(u0), lap) <= RTOL
    plan.destroy()


@pytest.mark.parametrize("deg,inc,k", [(3, 0, 5), (3, 0, -7), (4, 1, -7), (MIXED, 0, 4)], ids=lambda v: "mixed" if isinstance(v, list) else str(v))
def test_linearisation_is_the_derivative_of_the_term(gpu, hiplib, deg, inc, k):
    """(N(u + eps v) - N(u - eps v)) / 2 eps against the linearised term applied to v.  eps = 1e-5: truncation O(eps^2) = 1e-10, roundoff
    1e-16 / eps = 1e-11; the bound 1e-7 leaves three orders and still catches a wrong k or k - 1"""
    import torch
    c = _Case(gpu, deg, inc, faces=True)
    plan = c.plan
    c.set_power(k, True)
    u = c.smooth(0.4)
    v = np.cos(2.0 * c.x + c.y - c.z)
    eps = 1e-5
    fd = (c.term(u + eps * v) - c.term(u - eps * v)) / (2 * eps)
    plan.linearise(_t(u, gpu))
    dv = _t(v, gpu)
    lhs, lap = torch.empty_like(dv), torch.empty_like(dv)
    plan.apply_lhs(dv, lhs)
    plan.apply_aij(dv, lap)
    lin = (lhs - lap).cpu().numpy()
    err = _rel(fd, lin)
    print("derivative consistency deg=%s inc=%d k=%d: rel-inf %.3e" % (deg, inc, k, err))
    assert err <= 1e-7
    plan.destroy()


@pytest.mark.parametrize("deg,inc", [(3, 0), (4, 1)])
def test_build_residual(gpu, hiplib, deg, inc):
    """A u (with Dirichlet data) + N(u) - rhs against the composed calls"""
    import torch
    from disco4est_amd import mesh as M
    c = _Case(gpu, deg, inc, faces=True)
    plan, m = c.plan, c.m
    c.set_power(-7, True)
    bx = c.sides["bndry_xyz"]
    plan.set_dirichlet_values(np.sin(bx[0] + 0.3) * np.cos(bx[1]) + bx[2])
    du = _t(c.smooth(0.2), gpu)
    rhs = _t(M.splitmix64_uniform(5, m.local_nodes) - 0.5, gpu)
    Au, Nu = torch.empty_like(du), torch.empty_like(du)
    plan.apply_aij(du, Au)
    plan.apply_nonlinear_term(du, Nu, 0)
    out = torch.full_like(du, float("nan"))
    plan.build_residual(du, out, rhs)
    ref = (Au + Nu - rhs).cpu().numpy()
    assert _rel(out.cpu().numpy(), ref) <= RTOL
    plan.build_residual(du, out)                               # no right-hand side
    assert _rel(out.cpu().numpy(), (Au + Nu).cpu().numpy()) <= RTOL
    plan.destroy()
