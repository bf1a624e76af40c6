"""The Okendon problem Laplace(u) = |u|^p end to end on the device: the brick [1, 2]^3 (u > 0), 2 x 2 x 2 elements, the term from
set_okendon_term (the real form, s = 0.5), Dirichlet data from OKENDON_U through boundary_gather + field_eval, d4est_hip_newton_solve
with FCG and no preconditioner -- against tests/dense_problem_more.py's Newton loop around the composed device pieces, with the
tolerances of tests/test_newton_gpu.py (the same iteration count, the history to 1e-8 relative above 1e-9 of its first entry)."""
import numpy as np
import pytest

from tests import dense_problem_more as DM

pytestmark = pytest.mark.gpu

EXT = (1., 2., 1., 2., 1., 2.)
S = 0.5
NEWTON = dict(atol=1e-15, rtol=1e-8, imin=0, imax=8, krylov_imax=400, krylov_atol=0.0, krylov_rtol=1e-13)


def _t(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(gpu)


def _setup(gpu, deg):
    import torch
    from disco4est_amd import Plan, capi, mesh as M
    m = M.BrickMesh(1, deg)
    tree, q, dq = m.cells()
    plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, 0)
    plan.set_geometry_brick(dq, m.root_len, EXT)
    plan.set_faces(m.build_sides(geometry=False), 10.0, 0, brick=(dq, m.root_len, EXT))
    params = capi.okendon_params(S)
    plan.set_okendon_term(params, brick=(q, dq, m.root_len, EXT))
    xyz = torch.empty(3 * m.local_nodes, dtype=torch.float64, device=gpu)
    plan.compute_xyz_brick(q, dq, m.root_len, EXT, xyz_lobatto=xyz)
    g = plan.dirichlet_from_field("OKENDON_U", params, xyz)
    u_star = torch.empty(m.local_nodes, dtype=torch.float64, device=gpu)
    capi.field_eval("OKENDON_U", params, xyz, u_star)
    return m, plan, g, u_star


def _device_newton(plan, m, g, gpu):
    import torch
    u = torch.ones(m.local_nodes, dtype=torch.float64, device=gpu)
    ierr, its, hist = plan.newton_solve(u, None, g, pc=None, **NEWTON)
    return ierr, its, hist, u


def test_okendon_newton_against_the_dense_loop(gpu, hiplib):
    import torch
    m, plan, g, u_star = _setup(gpu, 4)
    assert plan.nonlinear_exponent() == S and plan.nonlinear_fused()
    assert float(u_star.min()) > 0.02                           # M r^4 on [1, 2]^3: 9 / 400 at the near corner
    nq = m.local_nodes_quad
    a = np.ones(nq)

    def apply_A(x):
        plan.set_dirichlet_values(g)
        out = torch.empty(m.local_nodes, dtype=torch.float64, device=gpu)
        plan.apply_aij(_t(x, gpu), out)
        return out.cpu().numpy()

    def interpolate(x):
        out = torch.empty(nq, dtype=torch.float64, device=gpu)
        plan.interpolate(_t(x, gpu), out)
        return out.cpu().numpy()

    def galerkin(f):
        out = torch.empty(m.local_nodes, dtype=torch.float64, device=gpu)
        plan.apply_galerkin_integral(_t(f, gpu), out)
        return out.cpu().numpy()

    def solve_lhs(c, minus_f):
        """plain CG on apply_lhs with the restated coefficient (the loop of tests/test_newton_gpu.py)"""
        plan.set_dirichlet_values(None)
        plan.set_lhs_coefficient(_t(c, gpu))
        b = _t(minus_f, gpu)
        xk = torch.zeros_like(b); r = b.clone(); d = r.clone(); rr = float(r @ r); r0 = rr
        Ad = torch.empty_like(b)
        for _ in range(400):
            plan.apply_lhs(d, Ad)
            al = rr / float(d @ Ad)
            xk += al * d; r -= al * Ad
            rn = float(r @ r)
            if rn <= 1e-26 * r0:
                break
            d = r + (rn / rr) * d; rr = rn
        return xk.cpu().numpy()

    ierr_ref, x_ref, hist_ref = DM.newton_abs_power(apply_A, interpolate, galerkin, solve_lhs, a, None, S, np.ones(m.local_nodes),
                                                    NEWTON["atol"], NEWTON["rtol"], 0, NEWTON["imax"])
    plan.set_lhs_coefficient(None)
    plan.set_dirichlet_values(None)

    ierr, its, hist, u = _device_newton(plan, m, g, gpu)
    print("newton (Okendon, p = 4): device history %s\n                         restated history %s" % (list(hist), hist_ref))
    assert ierr == 0 and ierr_ref == 0
    assert its == len(hist_ref) - 1
    for h, hr in zip(hist, hist_ref):
        if hr > 1e-9 * hist_ref[0]:
            assert abs(h - hr) <= 1e-8 * hr, (h, hr)
    # the final u: both loops stop at |F| <= rtol |F_0|, so they agree to the Newton tolerance through the inverse Jacobian; the
    # coercivity of the SIPG Laplacian on this unit-size mesh is O(1), asserted with two orders to spare
    scale = float(u_star.abs().max())
    assert float((u - _t(x_ref, gpu)).abs().max()) <= 100 * NEWTON["rtol"] * scale
    err4 = float((u - u_star).abs().max())

    m3, plan3, g3, u_star3 = _setup(gpu, 3)
    ierr3, its3, hist3, u3 = _device_newton(plan3, m3, g3, gpu)
    err3 = float((u3 - u_star3).abs().max())
    print("nodal error against OKENDON_U: p = 3 %.3e, p = 4 %.3e" % (err3, err4))
    assert ierr3 == 0 and err4 < err3                           # M r^4 has degree 4 per variable: p = 4 holds it, p = 3 does not
    plan.destroy(); plan3.destroy()
