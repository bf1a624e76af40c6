"""The Okendon, Boyen-York, Lorentzian and Stamm problem data on the device: the eight field ids against tests/dense_problem_more.py, the
two term setters against field_eval on the plan's coordinates bit for bit, the Lorentzian Robin coefficient by id against Robin data by
arrays, and the load vector by id against compute_xyz -> field_eval -> apply_galerkin_integral."""
import numpy as np
import pytest

from tests import dense_problem_more as DM
from tests.test_problem_gpu import EPS, MESHES, _apply, _eval, _t, _xyz_quad

pytestmark = pytest.mark.gpu

OK, BY, STAMM = (0.5,), (0.7, 1.3), (0.25, 0.3, 0.35)
PARAMS = {"OKENDON_U": OK, "BY_PSI": BY, "BY_A": BY, "LORENTZIAN_U": None, "LORENTZIAN_RHS": None, "LORENTZIAN_ROBIN": None,
          "STAMM_U": STAMM, "STAMM_RHS": STAMM}
# ulp bounds from the operation counts, the fields being contraction-free (the rule of tests/test_problem_gpu.py).  r2 = 3 products and
# 2 sums of positive terms: 2.5 ulp.  pow: 2 ulp on the device and 1 in libm, 3 between them, plus the exponent times the argument's error.
#   OKENDON_U (p = .5, exponent 2): 2 x 2.5 (r2) + 3 (pow) + 3 (M, a pow on each side) + 1 (product) = 12
#   BY_PSI: five positive terms of at most 6 roundings each, a quarter of that through pow(., .25), + 3 (pow): 5
#   BY_A: 1 - a2 / r2 >= 0.35 on the points (r2 >= 0.75, a = 0.7), so its 2 roundings are amplified by at most 3, twice; + r4, P2 / r4, the
#         three products: 2 x 6 + 2.5 x 2 + 5 = 22
#   LORENTZIAN_U: r2, sqrt, r r, 1 +, sqrt, division: 7;  _RHS: 2.5 x (2.5 + 1) (pow's argument) + 3 + 1 = 13;  _ROBIN: 2.5 + 1 + 1 + 1 = 6
#   STAMM_U: three differences, rp (4.5), two products for rp^3 and six factors x, 1 - x, ... (1 - x is exact for x in [0.5, 2]): 3 x 4.5 + 8 = 22
ULPS = {"OKENDON_U": 12, "BY_PSI": 5, "BY_A": 22, "LORENTZIAN_U": 7, "LORENTZIAN_RHS": 13, "LORENTZIAN_ROBIN": 6, "STAMM_U": 22}
X = np.random.default_rng(17).uniform(0.5, 1.5, (3, 257))      # 257: one full block and one thread


@pytest.mark.parametrize("fid", sorted(PARAMS))
def test_fields_against_the_restatement(gpu, hiplib, fid):
    from disco4est_amd import capi
    assert capi.FIELD[fid] == 6 + ["OKENDON_U", "BY_PSI", "BY_A", "LORENTZIAN_U", "LORENTZIAN_RHS", "LORENTZIAN_ROBIN", "STAMM_U",
                                   "STAMM_RHS"].index(fid)
    got = _eval(fid, PARAMS[fid], X, gpu)
    ref = DM.FIELDS[fid](X[0], X[1], X[2], PARAMS[fid])
    if fid == "STAMM_RHS":
        # thirteen terms of up to 12 roundings each that cancel: 16 ulp of sum |term| / sqrt(S), + 3 for the sum's own roundings
        t, rS = DM.stamm_rhs_terms(X[0], X[1], X[2], STAMM)
        bound = 19 * EPS * sum(np.abs(v) for v in t) / rS
    else:
        bound = ULPS[fid] * EPS * np.abs(ref)
    print("%s: worst error / bound = %.3f" % (fid, (np.abs(got - ref) / bound).max()))
    assert np.all(np.isfinite(got)) and np.all(np.abs(got - ref) <= bound)


def test_stamm_rhs_is_zero_at_the_corner(gpu, hiplib):
    P = np.array([[STAMM[0], 0.5], [STAMM[1], 0.5], [STAMM[2], 0.5]])
    got = _eval("STAMM_RHS", STAMM, P, gpu)
    assert got[0] == 0.0 and got[1] != 0.0


@pytest.mark.parametrize("mesh", ["brick", "sphere13", "hole_p9"])
def test_term_setters_equal_field_eval_bitwise(gpu, hiplib, mesh):
    """set_okendon_term / set_boyen_york_term in the source form and the _xyz form against field_eval on compute_xyz_*"""
    import torch
    from disco4est_amd import capi
    m, plan, sides, src, ext = MESHES[mesh](gpu)
    xyz = _xyz_quad(plan, src, gpu)
    nq = plan.local_nodes_quad
    a_ref = torch.empty(nq, dtype=torch.float64, device=gpu)
    capi.field_eval("BY_A", BY, xyz, a_ref)
    for kw in (src, dict(xyz=xyz)):
        plan.set_boyen_york_term(capi.boyen_york_params(*BY), **kw)
        a, b, k = plan.nonlinear_coefficients()
        assert k == -7 and b is None and plan.nonlinear_exponent() is None and torch.equal(a, a_ref)
        plan.set_okendon_term(capi.okendon_params(0.3), **kw)
        a, b, k = plan.nonlinear_coefficients()
        assert k == 0 and b is None and plan.nonlinear_exponent() == 0.3 and bool((a == 1.0).all())
    plan.destroy()


@pytest.mark.parametrize("mesh", ["brick", "sphere13"])
def test_lorentzian_robin_by_id_equals_robin_by_arrays(gpu, hiplib, mesh):
    """the bound of tests/test_problem_gpu.py::test_robin_by_id_equals_robin_by_arrays: both paths round c (6 roundings here, 7 there)
    and sj c, the boundary terms are bounded by 64 |A u|_inf"""
    import torch
    m, plan, sides, src, ext = MESHES[mesh](gpu)
    tm = int(sides["total_mortar_nodes"])
    u = _t(1.0 + 0.1 * np.random.default_rng(9).random(m.local_nodes), gpu)
    xyz = torch.ones(3 * tm, dtype=torch.float64, device=gpu)
    plan.compute_boundary_xyz(xyz, **src)
    Xm = xyz.cpu().numpy().reshape(3, tm)
    plan.set_robin_by_id("LORENTZIAN", "ZERO", **src)
    by_id = _apply(plan, u)
    plan.set_robin_values(DM.lorentzian_robin(Xm[0], Xm[1], Xm[2]), np.zeros(tm))
    by_arrays = _apply(plan, u)
    plan.set_robin_values(None, None)
    dirichlet = _apply(plan, u)
    err = float((by_id - by_arrays).abs().max())
    assert err <= 64 * 8 * EPS * float(by_arrays.abs().max())
    assert float((by_id - dirichlet).abs().max()) > 1e-6 * float(dirichlet.abs().max())
    plan.destroy()


@pytest.mark.parametrize("mesh", ["brick", "brick_lobatto", "sphere13", "hole_p9"])
def test_build_load_against_the_three_call_composition(gpu, hiplib, mesh):
    """build_load against compute_xyz_*, field_eval, apply_galerkin_integral (all existing code).  Where every bucket has a one-kernel
    pair (brick_lobatto: deg_quad = deg = 2, 3, 4; sphere13: p = 3) the load kernel runs the integrate body of the fused nonlinear term
    on the composition's own bits: equality.  brick (p = 4 with deg_quad = 5: no pair) and hole_p9 (deg_quad = 11 on p = 9) take the
    composition itself: equality as well."""
    import torch
    from disco4est_amd import capi
    m, plan, sides, src, ext = MESHES[mesh](gpu)
    plan.set_tuning(6, 1)      # D4EST_HIP_TUNE_STIFFNESS_EO at its default: the integral's even-odd body, which the load kernel shares
    assert plan.nonlinear_fused() == (mesh in ("brick_lobatto", "sphere13"))
    xyz = _xyz_quad(plan, src, gpu)
    nq, n = plan.local_nodes_quad, plan.local_nodes
    fq = torch.empty(nq, dtype=torch.float64, device=gpu)
    for fid in ("LORENTZIAN_RHS", "STAMM_RHS", "CDS_PSI"):
        params = PARAMS.get(fid, (0.25, -0.5, 0.125, 3.0, 0.01, 1.7, 5.0, -0.3))
        capi.field_eval(fid, params, xyz, fq)
        ref = torch.empty(n, dtype=torch.float64, device=gpu)
        plan.apply_galerkin_integral(fq, ref)
        for kw in (src, dict(xyz=xyz)):
            out = torch.full((n,), float("nan"), dtype=torch.float64, device=gpu)
            plan.build_load(fid, params, out, **kw)
            assert bool(torch.isfinite(out).all()) and float(ref.abs().max()) > 0
            assert torch.equal(out, ref), (fid, float((out - ref).abs().max()))
            out0 = torch.cos(torch.arange(n, dtype=torch.float64, device=gpu))
            acc = out0.clone()
            plan.build_load(fid, params, acc, beta=1, **kw)                 # beta = 1 accumulates
            assert float((acc - (out0 + ref)).abs().max()) <= 4 * EPS * float((out0.abs() + ref.abs()).max())
    plan.destroy()
