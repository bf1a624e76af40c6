"""The real-power term a |b + u|^s on the device (d4est_hip_plan_set_nonlinear_abs_power): apply_nonlinear_term, plan_linearise +
apply_lhs and build_residual against tests/dense_problem_more.py around the oracle's interpolate / galerkin integral.
Tolerance: 1e-12 relative to the reference's infinity norm, the bound tests/test_nonlinear_fused_gpu.py holds the integer form to; the
device pow differs from libm's by a few ulp per node under the same quadrature sums."""
import numpy as np
import pytest

from tests import dense_nonlinear as DN
from tests import dense_problem_more as DM
from tests.test_nonlinear_sweep_gpu import _weights3

pytestmark = pytest.mark.gpu

RTOL = 1e-12
MIXED = [2, 3, 3, 2, 3, 2, 2, 3]
EXPONENTS = (0.5, 0.3)


def _t(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(gpu)


def _rel(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


class _Case:
    def __init__(self, gpu, deg, inc=0, amp=0.03, faces=False):
        from disco4est_amd import Plan, mesh as M
        self.gpu = gpu
        self.m = m = M.BrickMesh(1, np.array(deg, np.int32) if isinstance(deg, list) else deg, deg_quad_inc=inc)
        self.mp = mp = M.SineMap(amp)            # amp = 0: the affine 2 x 2 x 2 brick
        self.J, self.rst = m.geometry(mp)
        self.plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, 0)
        self.plan.set_geometry(self.J, self.rst)
        if faces:
            self.sides = m.build_sides(mp)
            self.plan.set_faces(self.sides, 10.0, 0)
        nq = m.local_nodes_quad
        self.a = -(0.5 + M.splitmix64_uniform(11, nq))
        self.b = 0.1 + 0.2 * M.splitmix64_uniform(12, nq)
        self.x, self.y, self.z = m.nodal_coords(mp)

    def smooth(self, s):
        """in [0.75, 1.25]: |b + V u| >= 0.1 with and without b"""
        return 1.0 + 0.25 * np.sin(1.1 * self.x + 2.0 * self.y + 3.0 * self.z + s)

    def set_abs(self, s, with_b):
        self.plan.set_nonlinear_abs_power(_t(self.a, self.gpu), _t(self.b, self.gpu) if with_b else None, s)

    def term(self, u, beta=0, out0=None):
        import torch
        du = _t(u, self.gpu)
        out = torch.full_like(du, float("nan")) if out0 is None else _t(out0, self.gpu)
        self.plan.apply_nonlinear_term(du, out, beta)
        return out.cpu().numpy()


# (deg, deg_quad_inc, map amplitude, one-kernel form): mixed p = 2, 3 affine and curved (the one-launch buckets), p = 7 (the one-wave
# limit), p = 8 (multi-wave), deg_quad = deg + 1 with (p = 3) and without (p = 4: the three-call fallback) a compiled pair
SHAPES = [(MIXED, 0, 0.0, True), (MIXED, 0, 0.03, True), (7, 0, 0.03, True), (8, 0, 0.03, True), (3, 1, 0.03, True), (4, 1, 0.03, False)]
IDS = ["mixed-affine", "mixed-curved", "p7", "p8", "p3q4", "p4q5-composed"]


@pytest.mark.parametrize("deg,inc,amp,fused", SHAPES, ids=IDS)
def test_term_and_coefficient_against_the_restatement(gpu, hiplib, oracle, deg, inc, amp, fused):
    c = _Case(gpu, deg, inc, amp)
    m, plan = c.m, c.plan
    assert plan.nonlinear_fused() == fused
    u = c.smooth(0.3)
    uq = oracle.interpolate(m, u)
    out0 = np.cos(3.0 * c.x - c.y) + 2.0
    for s in EXPONENTS:
        for with_b in (False, True):
            bq = c.b if with_b else None
            assert np.abs(uq if bq is None else bq + uq).min() >= 0.1
            ref = oracle.apply_galerkin(m, c.J, DM.abs_term(c.a, bq, uq, s))
            c.set_abs(s, with_b)
            assert plan.nonlinear_exponent() == s and plan.nonlinear_coefficients()[2] == 0
            e0 = _rel(c.term(u), ref)
            e1 = _rel(c.term(u, 1, out0), out0 + ref)
            plan.linearise(_t(u, gpu))
            cc, wjc = plan.lhs_coefficient_arrays()
            c_ref = DM.abs_dterm(c.a, bq, uq, s)
            e2 = _rel(cc.cpu().numpy(), c_ref)
            print("abs power %s s=%g b=%s: rel-inf error beta=0 %.3e, beta=1 %.3e, coefficient %.3e" % (deg, s, with_b, e0, e1, e2))
            assert e0 <= RTOL and e1 <= RTOL and e2 <= RTOL, (s, with_b, e0, e1, e2)
            if fused:   # the pre-combined w J c, bit for bit against (w_k (w_a w_b)) (J c) from the c just read and the plan's weights
                W3 = np.concatenate([_weights3(m.quad_type, int(dq)) for dq in m.deg_quad])
                assert wjc is not None and np.array_equal(wjc.cpu().numpy(), W3 * (c.J * cc.cpu().numpy()))
            else:
                assert wjc is None                               # the composed path leaves w J c to the first apply
            plan.set_lhs_coefficient(None)
    plan.set_nonlinear_abs_power(None, None, 0.5)              # off
    assert plan.nonlinear_exponent() is None and plan.nonlinear_coefficients() is None
    assert np.array_equal(c.term(u), np.zeros(m.local_nodes))
    plan.destroy()


@pytest.mark.parametrize("deg,inc", [(MIXED, 0), (4, 1)], ids=["mixed", "p4q5-composed"])
def test_linearise_apply_lhs_and_build_residual(gpu, hiplib, oracle, deg, inc):
    """apply_lhs after linearise = apply_aij + V^T W J c V with the restated c; build_residual = A u + N(u) - rhs"""
    import torch
    from disco4est_amd import mesh as M
    c = _Case(gpu, deg, inc, faces=True)
    m, plan = c.m, c.plan
    s = 0.3
    c.set_abs(s, True)
    u0 = c.smooth(0.0)
    v = _t(m.field(c.mp), gpu)
    lap, wm, got = torch.empty_like(v), torch.empty_like(v), torch.full_like(v, float("nan"))
    plan.apply_aij(v, lap)
    plan.apply_weighted_mass_matrix(v, _t(DM.abs_dterm(c.a, c.b, oracle.interpolate(m, u0), s), gpu), wm)
    plan.linearise(_t(u0, gpu))
    plan.apply_lhs(v, got)
    e = float((got - (lap + wm)).abs().max() / (lap + wm).abs().max())
    assert e <= RTOL, e
    assert float(wm.abs().max()) > 1e-5 * float(lap.abs().max())   # the bound resolves the term itself to seven digits
    plan.set_lhs_coefficient(None)
    bx = c.sides["bndry_xyz"]
    plan.set_dirichlet_values(np.sin(bx[0] + 0.3) * np.cos(bx[1]) + bx[2])
    du = _t(c.smooth(0.2), gpu)
    rhs = _t(M.splitmix64_uniform(5, m.local_nodes) - 0.5, gpu)
    Au = torch.empty_like(du)
    plan.apply_aij(du, Au)
    Nu = oracle.apply_galerkin(m, c.J, DM.abs_term(c.a, c.b, oracle.interpolate(m, c.smooth(0.2)), s))
    out = torch.full_like(du, float("nan"))
    plan.build_residual(du, out, rhs)
    ref = (Au - rhs).cpu().numpy() + Nu
    assert _rel(out.cpu().numpy(), ref) <= RTOL
    plan.destroy()


def test_each_form_gives_its_own_result(gpu, hiplib, oracle):
    """the integer form after the real form, and the reverse"""
    c = _Case(gpu, MIXED)
    m, plan = c.m, c.plan
    u = c.smooth(0.1)
    uq = oracle.interpolate(m, u)
    ref_abs = oracle.apply_galerkin(m, c.J, DM.abs_term(c.a, c.b, uq, 0.5))
    ref_int = oracle.apply_galerkin(m, c.J, DN.term(c.a, c.b, uq, -7))
    c.set_abs(0.5, True)
    assert _rel(c.term(u), ref_abs) <= RTOL
    plan.set_nonlinear_power(_t(c.a, gpu), _t(c.b, gpu), -7)
    assert plan.nonlinear_exponent() is None and plan.nonlinear_coefficients()[2] == -7
    assert _rel(c.term(u), ref_int) <= RTOL
    c.set_abs(0.5, True)
    assert plan.nonlinear_exponent() == 0.5 and plan.nonlinear_coefficients()[2] == 0
    assert _rel(c.term(u), ref_abs) <= RTOL
    assert _rel(ref_abs, ref_int) > 1e-2
    plan.destroy()
