"""d4est_hip_newton_solve (the reference's d4est_solver_newton_solve with the device FCG) on the power term: against
tests/dense_nonlinear.py's loop driven by the composed device pieces, with a two-level multigrid preconditioner refreshed through
on_linearise, and the loop's edge rules."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import dense_nonlinear as DN

pytestmark = pytest.mark.gpu


def _t(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(gpu)


def _quad_coords(plan, m, mp, gpu):
    """coordinates of the quadrature nodes: the nodal coordinates interpolated (isoparametric, like the reference's xyz_quad)"""
    import torch
    out = []
    for c in m.nodal_coords(mp):
        t = torch.empty(m.local_nodes_quad, dtype=torch.float64, device=gpu)
        plan.interpolate(_t(c, gpu), t)
        out.append(t.cpu().numpy())
    return out


def test_newton_on_cubic_reaction_diffusion(gpu, hiplib):
    """-Laplace(u) + u^3 = g with Dirichlet data (mesh, exact solution and boundary data of tests/test_nonlinear_gpu.py): u^3 - g splits
    into the power term a = 1, b = 0, k = 3 and rhs = V^T W J g"""
    import torch
    from disco4est_amd import Plan, mesh as M
    m = M.BrickMesh(1, 4, deg_quad_inc=1)
    mp = M.SineMap(0.03)
    J, rst = m.geometry(mp); sides = m.build_sides(mp)
    plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, 0)
    plan.set_geometry(J, rst)
    plan.set_faces(sides, 10.0, 0)
    exact = lambda x, y, z: np.sin(1.3 * x + 0.4) * np.cos(0.9 * y) * np.exp(0.5 * z)
    lap = lambda x, y, z: (-(1.3 ** 2) - 0.9 ** 2 + 0.25) * exact(x, y, z)
    u_star = exact(*m.nodal_coords(mp))
    xq, yq, zq = _quad_coords(plan, m, mp, gpu)
    g_q = _t(-lap(xq, yq, zq) + exact(xq, yq, zq) ** 3, gpu)
    bx = sides["bndry_xyz"]
    g_bnd = _t(exact(bx[0], bx[1], bx[2]), gpu)
    rhs = torch.empty(m.local_nodes, dtype=torch.float64, device=gpu)
    plan.apply_galerkin_integral(g_q, rhs)

    # the composed device pieces of the existing test, under the restated loop
    state = {}

    def residual(x):
        u = _t(x, gpu)
        plan.set_dirichlet_values(g_bnd)
        Au = torch.empty_like(u)
        plan.apply_aij(u, Au)
        uq = torch.empty(m.local_nodes_quad, dtype=torch.float64, device=gpu)
        plan.interpolate(u, uq)
        out = torch.empty_like(u)
        plan.apply_galerkin_integral(uq ** 3 - g_q, out)
        state["uq"] = uq
        return (Au + out).cpu().numpy()

    def solve(x, minus_f):
        plan.set_dirichlet_values(None)
        plan.set_lhs_coefficient(3.0 * state["uq"] ** 2)
        b = _t(minus_f, gpu)
        xk = torch.zeros_like(b); r = b.clone(); d = r.clone(); rr = float(r @ r); r0 = rr
        Ad = torch.empty_like(b)
        for _ in range(400):
            plan.apply_lhs(d, Ad)
            a = rr / float(d @ Ad)
            xk += a * d; r -= a * Ad
            rn = float(r @ r)
            if rn <= 1e-26 * r0:
                break
            d = r + (rn / rr) * d; rr = rn
        return xk.cpu().numpy()

    atol, rtol, imax = 1e-15, 1e-8, 8
    ierr_ref, x_ref, hist_ref = DN.newton(residual, solve, np.zeros(m.local_nodes), atol, rtol, 0, imax)
    plan.set_lhs_coefficient(None)
    plan.set_dirichlet_values(None)

    plan.set_nonlinear_power(torch.ones(m.local_nodes_quad, dtype=torch.float64, device=gpu), None, 3)
    u = torch.zeros(m.local_nodes, dtype=torch.float64, device=gpu)
    ierr, its, hist = plan.newton_solve(u, rhs, g_bnd, atol=atol, rtol=rtol, imin=0, imax=imax, krylov_imax=400, krylov_atol=0.0,
                                        krylov_rtol=1e-13, pc=None)
    print("newton (cubic): device history %s\n                restated history %s" % (list(hist), hist_ref))
    assert ierr == 0 and ierr_ref == 0
    assert its == len(hist_ref) - 1                                        # the same iteration count
    for h, hr in zip(hist, hist_ref):
        if hr > 1e-9 * hist_ref[0]:
            assert abs(h - hr) <= 1e-8 * hr, (h, hr)
    assert hist[2] < 0.05 * hist[1]                                        # quadratic convergence
    assert float((u - _t(u_star, gpu)).abs().max()) < 2e-3                 # p = 4 on 8 elements
    # the plan's Dirichlet data is homogeneous on return: A 0 = 0
    z = torch.zeros_like(u); Az = torch.full_like(u, float("nan"))
    plan.apply_aij(z, Az)
    assert float(Az.abs().max()) == 0.0
    plan.destroy()


def _two_punctures_like(gpu, deg):
    """-Laplace(u) + a (b + u)^-7 = 0 on the unit cube under the sine map, u = 0 on the boundary: b = 1 + 0.5 / r from a point outside the
    mesh, a < 0 (the shape of two_punctures_neg_1o8_K2_psi_neg7)"""
    from disco4est_amd import Plan, mesh as M
    m = M.BrickMesh(1, deg)
    mp = M.SineMap(0.03)
    J, rst = m.geometry(mp); sides = m.build_sides(mp)
    plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, 0)
    plan.set_geometry(J, rst)
    plan.set_faces(sides, 10.0, 0)
    xq, yq, zq = _quad_coords(plan, m, mp, gpu)
    r = np.sqrt((xq + 0.5) ** 2 + (yq + 0.4) ** 2 + (zq + 0.3) ** 2)
    a = -4.0 * (1.0 + xq * yq)
    b = 1.0 + 0.5 / r
    plan.set_nonlinear_power(_t(a, gpu), _t(b, gpu), -7)
    return m, plan


NEWTON = dict(atol=1e-15, rtol=1e-6, imin=0, imax=8, krylov_imax=400, krylov_atol=0.0, krylov_rtol=1e-13)


def test_newton_with_a_multigrid_preconditioner(gpu, hiplib):
    """two-level p-multigrid (p = 4 over p = 2 on the same 8 elements) as the FCG preconditioner; on_linearise linearises the coarse plan
    at the projected u0.  The preconditioner must not change the Newton iterates beyond the Krylov tolerance"""
    import torch
    from disco4est_amd import Transfer, Multigrid
    mf, fine = _two_punctures_like(gpu, 4)
    mc, coarse = _two_punctures_like(gpu, 2)
    n_el = mf.n_elements
    degh = np.zeros(8 * n_el, np.int32); degh[::8] = 4
    tr = Transfer(np.zeros(n_el, np.int32), np.full(n_el, 2, np.int32), degh)
    mg = Multigrid([coarse, fine], [tr])
    assert mg.set_smoother_cheby(3, 5, 30.0, 1.1, 0, 0, 1, 0) == 0
    mg.set_bottom_solver_cg(40, 0.0, 1e-12)
    mg.set_pc(1, 0.0, 0.0)
    assert mg.ready() == 1

    u_plain = torch.zeros(mf.local_nodes, dtype=torch.float64, device=gpu)
    ierr0, its0, hist0 = fine.newton_solve(u_plain, None, None, pc=None, **NEWTON)

    u = torch.zeros_like(u_plain)
    uc = torch.zeros(mc.local_nodes, dtype=torch.float64, device=gpu)
    calls = []

    def on_linearise(u0_ptr):
        assert u0_ptr == u.data_ptr()
        tr.project(u, uc)
        coarse.linearise(uc)
        calls.append(1)

    ierr, its, hist = fine.newton_solve(u, None, None, pc=mg, on_linearise=on_linearise, **NEWTON)
    print("newton (k = -7): preconditioned history %s\n                 plain history          %s" % (list(hist), list(hist0)))
    assert ierr == 0 and ierr0 == 0
    assert its <= 8 and its == its0 and len(calls) == its
    assert np.all(np.abs(hist - hist0) <= 1e-6 * hist0)
    assert hist[-1] <= 1e-15 + 1e-6 * hist[0] and float(u.abs().max()) > 1e-3      # a solve, not a no-op
    mg.destroy(); tr.destroy(); fine.destroy(); coarse.destroy()


def test_newton_edge_rules(gpu, hiplib):
    import torch
    m, plan = _two_punctures_like(gpu, 3)
    u = torch.zeros(m.local_nodes, dtype=torch.float64, device=gpu)
    # imax = 0: no iteration, not converged, u untouched
    u0 = _t(0.01 * np.sin(np.arange(m.local_nodes)), gpu)
    u.copy_(u0)
    ierr, its, hist = plan.newton_solve(u, None, None, **dict(NEWTON, imax=0))
    assert ierr == 1 and its == 0 and len(hist) == 1 and torch.equal(u, u0)
    # a converged solution as the initial guess: imin = 2 forces exactly two iterations, imin = 0 none
    u.zero_()
    ierr, its, hist = plan.newton_solve(u, None, None, **dict(NEWTON, rtol=1e-10))
    assert ierr == 0 and its >= 2
    tol = dict(NEWTON, atol=1e3 * hist[-1] + 1e-12, rtol=0.0)
    v = u.clone()
    ierr, its, hist2 = plan.newton_solve(v, None, None, **dict(tol, imin=2))
    assert ierr == 0 and its == 2 and len(hist2) == 3
    v.copy_(u)
    ierr, its, _ = plan.newton_solve(v, None, None, **dict(tol, imin=0))
    assert ierr == 0 and its == 0 and torch.equal(v, u)
    plan.destroy()


_GHOST_CHILD = """
import numpy as np, torch
from disco4est_amd import Plan, mesh as M
deg = np.full(8, 2)
m = M.BrickMesh(1, deg, first=0, count=4)
J, rst = m.geometry()
plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, 0)
plan.set_geometry(J, rst)
plan.set_faces(m.build_sides())
assert plan.ghost_trace_size > 0
plan.set_nonlinear_power(torch.ones(m.local_nodes_quad, dtype=torch.float64, device="cuda"), None, 3)
u = torch.zeros(m.local_nodes, dtype=torch.float64, device="cuda")
plan.newton_solve(u, None, None, imax=1)
print("NOT REACHED")
"""


def test_newton_on_a_plan_with_ghost_sides_aborts_cleanly(gpu, hiplib):
    """a host-side argument check ([D4EST_HIP_ABORT], before any launch), seen from a child process"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-c", _GHOST_CHILD], capture_output=True, text=True, timeout=120, cwd=root, env=env)
    assert p.returncode != 0 and "NOT REACHED" not in p.stdout
    assert "[D4EST_HIP_ABORT] newton_solve: the plan has ghost sides" in p.stderr, p.stderr
