"""The device Krylov solves d4est_hip_cg_solve / d4est_hip_fcg_solve against the numpy restatement of the reference's solvers
(tests/ref_solvers.py) on the oracle's operator: iteration counts, histories, solutions, the stop rule, the batch size of the stop-flag
reads, the allreduce hook calls, and that a solve leaves the plan's operator alone."""
import numpy as np
import pytest

from tests import ref_solvers as R

pytestmark = pytest.mark.gpu

KRYLOV_CHECK = 15   # D4EST_HIP_TUNE_KRYLOV_CHECK


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


class _Case:
    """a plan and the oracle registered with the same operator"""

    def __init__(self, kind, oracle, gpu):
        from disco4est_amd import Plan, mesh as M
        self.oracle = oracle
        self.kind = kind
        self.coeff = None
        self.hanging = False
        if kind == "curved_p4":
            m = M.BrickMesh(1, 4)
            mp = M.SineMap(0.05)
        elif kind == "lobatto_p3":
            m = M.BrickMesh(1, 3, quad_type=1)
            mp = M.SineMap(0.05)
        elif kind == "hanging_mixed_p_term":      # the mesh of tests/test_config4_gpu.py: hanging faces, p = 3 ... 9, the zeroth-order term
            refine = np.zeros(8, dtype=bool)
            refine[[2, 5]] = True
            m0 = M.HangingBrickMesh(1, refine, 3)
            m = M.HangingBrickMesh(1, refine, 3 + (np.arange(m0.global_elements) * 5 % 7), deg_quad_inc=1)
            mp = M.SineMap(0.04)
            self.hanging = True
            self.coeff = 1.0 + 4.0 * M.splitmix64_uniform(7, m.local_nodes_quad)
        else:
            raise ValueError(kind)
        J, rst = m.geometry(mp); sides = m.build_sides(mp)
        self.m = m
        self.plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, m.quad_type)
        self.plan.set_geometry(J, rst)
        self.plan.set_faces(sides, 10.0, 0)
        oracle.set_operator(m, J, rst, sides, 10.0, 0)
        oracle.set_hanging(sides if self.hanging else None)
        if self.coeff is not None:
            self.dcoeff = _t(self.coeff, gpu)
            self.plan.set_lhs_coefficient(self.dcoeff)
            oracle.set_lhs_coefficient(self.coeff)

    def close(self):
        self.oracle.set_lhs_coefficient(None)
        self.oracle.set_hanging(None)
        self.plan.destroy()


@pytest.fixture
def case(request, oracle, gpu, hiplib):
    c = _Case(request.param, oracle, gpu)
    yield c
    c.close()


CASES = ["curved_p4", "hanging_mixed_p_term", "lobatto_p3"]
# solution against the restatement, relative-inf: the histories agree to ~1e-11, but the components of u along the operator's smallest
# eigenvectors carry the 1e-13 difference between the device operator and the oracle's amplified by the condition number -- large on
# the hanging, p = 3 ... 9 mesh and behind the preconditioner (whose device and oracle forms differ in rounding as well); measured
# 9.6e-10 / 4.3e-8 / 6.6e-10 there
U_TOL = {"curved_p4": 1e-10, "lobatto_p3": 1e-10, "hanging_mixed_p_term": 2e-7}
U_TOL_PC = 5e-9


def _problem(c, seed=41):
    from disco4est_amd import mesh as M
    n = c.m.local_nodes
    return M.splitmix64_uniform(seed, n) - 0.5, M.splitmix64_uniform(seed + 1, n) - 0.5


def _gap(hist, lo, hi):
    """the stop iteration j in [lo, hi) where the restated history leaves the widest gap below everything before it, and a threshold in
    the middle of that gap (in log scale): rounding differences between the device and the restatement cannot move the count"""
    h = np.asarray(hist, dtype=np.float64)
    best, jb = -1.0, None
    for j in range(max(lo, 2), min(hi, len(h))):
        g = np.log(h[1:j].min()) - np.log(h[j])
        if g > best:
            best, jb = g, j
    assert best > 0.05, best
    return jb, float(np.sqrt(h[1:jb].min() * h[jb]))


@pytest.mark.parametrize("case", CASES, indirect=True)
def test_cg_solve_against_the_restatement(case, gpu):
    import torch
    c = case
    u0, rhs = _problem(c)
    _, _, h_all, _ = R.cg_solve(c.oracle.apply_lhs, u0, rhs, 40, 0.0, 0.0)
    j, thr = _gap(h_all, 15, 40)                  # delta_j <= thr: stop after iteration j
    atol, rtol, imax = 0.0, float(np.sqrt(thr / h_all[0])), 400
    u_ref, it_ref, h_ref, Au_ref = R.cg_solve(c.oracle.apply_lhs, u0, rhs, imax, atol, rtol)
    assert it_ref == j
    du, drhs = _t(u0, gpu), _t(rhs, gpu)
    dAu = torch.full_like(du, float("nan"))
    it, hist = c.plan.cg_solve(du, drhs, dAu, imax, atol, rtol)
    n = min(it, it_ref) + 1
    print("cg", it, it_ref, thr, np.max(np.abs(hist[:n] / np.array(h_ref[:n]) - 1)), hist[-3:], h_ref[-3:])
    assert it == it_ref
    assert np.abs(hist - np.array(h_ref)).max() <= 1e-8 * h_ref[0]
    u = du.cpu().numpy()
    assert _rel(u, u_ref) <= U_TOL[c.kind]
    assert _rel(dAu.cpu().numpy(), Au_ref) <= 1e-6          # Au as the reference leaves it: A d of the last iteration (d ~ r: small)
    r = rhs - c.oracle.apply_lhs(u)
    assert float(np.dot(r, r)) <= 4.0 * (atol * atol + hist[0] * rtol * rtol)
    # the host-vector form gives the same solve, bit for bit
    uh, Auh, ith, hh = c.plan.cg_solve_host(u0, rhs, imax, atol, rtol)
    assert ith == it and np.array_equal(uh, u) and np.array_equal(Auh, dAu.cpu().numpy()) and np.array_equal(hh, hist)


@pytest.mark.parametrize("case", CASES, indirect=True)
@pytest.mark.parametrize("with_pc", [False, True])
def test_fcg_solve_against_the_restatement(case, gpu, with_pc):
    import torch
    c = case
    u0, rhs = _problem(c, 43)
    # a preconditioner through the C hook: the element-wise inverse of the 1-D mass matrices (M^-1 x M^-1 x M^-1 per element, SPD),
    # the library's own d4est_hip_apply_invmij on the plan's stream; the restatement applies the oracle's
    lib, handle = c.plan.lib, c.plan.handle

    def pc_dev(r_ptr, z_ptr):
        lib.d4est_hip_apply_invmij(handle, r_ptr, z_ptr)

    pc_ref = (lambda r: c.oracle.apply_mij(c.m, r, inverse=True)) if with_pc else None
    _, _, h_all, _ = R.fcg_solve(c.oracle.apply_lhs, u0, rhs, 30, 0.0, 0.0, pc=pc_ref)
    j, tol = _gap(h_all, 10, 30)                  # |r_j| <= tol: stop after update j (count j + 1)
    atol, rtol, imax = 0.0, tol / h_all[0], 400
    u_ref, it_ref, h_ref, Au_ref = R.fcg_solve(c.oracle.apply_lhs, u0, rhs, imax, atol, rtol, pc=pc_ref)
    assert it_ref == j + 1
    du, drhs = _t(u0, gpu), _t(rhs, gpu)
    dAu = torch.full_like(du, float("nan"))
    it, hist = c.plan.fcg_solve(du, drhs, dAu, imax, atol, rtol, pc=pc_dev if with_pc else None)
    n = min(it, it_ref)
    print("fcg", it, it_ref, tol, np.max(np.abs(hist[:n] / np.array(h_ref[:n]) - 1)), hist[-3:], h_ref[-3:])
    assert it == it_ref
    assert np.abs(hist - np.array(h_ref)).max() <= 1e-8 * h_ref[0]
    u = du.cpu().numpy()
    assert _rel(u, u_ref) <= max(U_TOL[c.kind], U_TOL_PC if with_pc else 0.0)
    assert _rel(dAu.cpu().numpy(), Au_ref) <= 1e-12         # A u of the start
    # the stop rule, rechecked with the oracle: |r| before the last update already met it, the update only lowers it further
    r = rhs - c.oracle.apply_lhs(u)
    assert np.linalg.norm(r) <= 2.0 * (atol + rtol * hist[0])


@pytest.mark.parametrize("case", ["curved_p4", "hanging_mixed_p_term"], indirect=True)
def test_cg_batch_size_is_invisible(case, gpu):
    """D4EST_HIP_TUNE_KRYLOV_CHECK in {1, 7, 64}: bit-identical u, Au, history and the same count"""
    import torch
    c = case
    u0, rhs = _problem(c)
    _, _, h_all, _ = R.cg_solve(c.oracle.apply_lhs, u0, rhs, 40, 0.0, 0.0)
    _, thr = _gap(h_all, 15, 40)
    rtol = float(np.sqrt(thr / h_all[0]))
    out = {}
    for check in (1, 7, 64, -1):
        c.plan.set_tuning(KRYLOV_CHECK, check)
        du = _t(u0, gpu); dAu = torch.full_like(du, float("nan"))
        it, hist = c.plan.cg_solve(du, _t(rhs, gpu), dAu, 200, 0.0, rtol)
        out[check] = (it, du.cpu().numpy(), dAu.cpu().numpy(), hist)
    c.plan.set_tuning(KRYLOV_CHECK, -1)
    it1, u1, Au1, h1 = out[1]
    assert 15 <= it1 < 40                      # the stop falls inside a batch of 64 (and of the default 8 unless a multiple): no-ops after it
    for check in (7, 64, -1):
        it, u, Au, h = out[check]
        assert it == it1 and np.array_equal(u, u1) and np.array_equal(Au, Au1) and np.array_equal(h, h1), check


@pytest.mark.parametrize("case", ["curved_p4"], indirect=True)
def test_edge_cases(case, gpu):
    import torch
    c = case
    u0, rhs = _problem(c)
    du = _t(u0, gpu); dAu = torch.full_like(du, float("nan"))
    # imax = 0: u untouched, Au = A u of the start
    it, hist = c.plan.cg_solve(du, _t(rhs, gpu), dAu, 0, 0.0, 1e-10)
    assert it == 0 and np.array_equal(du.cpu().numpy(), u0) and len(hist) == 1
    ref = torch.empty_like(du)
    c.plan.apply_lhs(du, ref)
    assert torch.equal(dAu, ref)
    it, hist = c.plan.fcg_solve(du, _t(rhs, gpu), dAu, 0, 0.0, 1e-10)
    assert it == 0 and len(hist) == 0 and np.array_equal(du.cpu().numpy(), u0)
    # a start at the exact solution (rhs = A u with the same operator: r = 0): no iteration
    for check in (1, 64):
        c.plan.set_tuning(KRYLOV_CHECK, check)
        it, hist = c.plan.cg_solve(du, ref, dAu, 50, 0.0, 1e-10)
        assert it == 0 and hist[0] == 0.0 and np.array_equal(du.cpu().numpy(), u0)
    c.plan.set_tuning(KRYLOV_CHECK, -1)


@pytest.mark.parametrize("case", ["curved_p4"], indirect=True)
def test_allreduce_hook_calls(case, gpu):
    """a single-rank plan with a counting allreduce hook that does nothing: called the reference's number of times with the
    reference's scalar counts, results unchanged"""
    import torch
    c = case
    u0, rhs = _problem(c)
    runs = {}
    for hooked in (False, True):
        calls = []
        c.plan.set_comm(allreduce=(lambda p, n: calls.append(n)) if hooked else None)
        c.plan.set_tuning(KRYLOV_CHECK, 1)
        du = _t(u0, gpu); dAu = torch.empty_like(du)
        it, _ = c.plan.cg_solve(du, _t(rhs, gpu), dAu, 200, 0.0, 1e-9)
        cg_calls = list(calls)
        dv = _t(u0, gpu)
        del calls[:]
        itf, _ = c.plan.fcg_solve(dv, _t(rhs, gpu), dAu, 200, 0.0, 1e-9)
        runs[hooked] = (it, du.cpu().numpy(), itf, dv.cpu().numpy(), cg_calls, list(calls))
    c.plan.set_comm()
    c.plan.set_tuning(KRYLOV_CHECK, -1)
    it, u, itf, uf, cg_calls, fcg_calls = runs[True]
    assert it == runs[False][0] and np.array_equal(u, runs[False][1])
    assert itf == runs[False][2] and np.array_equal(uf, runs[False][3])
    assert len(cg_calls) == R.cg_allreduce_calls(it) and set(cg_calls) == {1}
    ncalls, nscalars = R.fcg_allreduce_calls(itf)
    assert len(fcg_calls) == ncalls and sum(fcg_calls) == nscalars and fcg_calls[:2] == [1, 2]


@pytest.mark.parametrize("case", ["hanging_mixed_p_term"], indirect=True)
def test_solve_leaves_the_operator_alone(case, gpu):
    import torch
    c = case
    u0, rhs = _problem(c)
    x = _t(u0, gpu)
    before = torch.empty_like(x); after = torch.empty_like(x)
    c.plan.apply_lhs(x, before)
    du = torch.zeros_like(x); dAu = torch.empty_like(x)
    c.plan.cg_solve(du, _t(rhs, gpu), dAu, 30, 0.0, 1e-12)
    c.plan.fcg_solve(du, _t(rhs, gpu), dAu, 10, 0.0, 1e-12)
    c.plan.apply_lhs(x, after)
    assert torch.equal(before, after)
