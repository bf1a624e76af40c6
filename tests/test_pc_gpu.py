"""The Chebyshev and Schwarz Krylov preconditioners on the device (d4est_hip_pc_cheby_*, d4est_hip_pc_schwarz_*) and the multigrid with the
Schwarz smoother as a preconditioner, against tests/ref_schwarz_smoother.py's pc_cheby_apply / pc_schwarz_apply and tests/ref_solvers.py's
FCG, all driven by the device primitives (tests/mg_schwarz_levels.py).

Tolerances.  PcCheby.apply runs the same kernels in the same order as the restatement built from Plan.cg_eigs and Plan.cheby_iterate,
and PcSchwarz.apply the same as a zero fill followed by Schwarz.iterate: both are compared with equality.  The FCG runs use the
tolerances of tests/test_krylov_gpu.py::test_fcg_solve_against_the_restatement: the same count with the stop placed in a gap of the
restated history, the history within 1e-8 of its first entry, u within U_TOL_PC = 5e-9."""
import numpy as np
import pytest

from tests import mg_schwarz_levels as L
from tests import ref_multigrid as RM
from tests import ref_schwarz_smoother as RZ
from tests import ref_solvers as RS

pytestmark = pytest.mark.gpu
U_TOL_PC = 5e-9
CHEBY = dict(cheby_imax=4, cheby_eigs_cg_imax=5, cheby_eigs_lmax_lmin_ratio=30.0, cheby_eigs_max_multiplier=1.1, cheby_use_new_cg_eigs=1)
# as a preconditioner of a whole solve the window must cover the spectrum: a 5-iteration bound kept for every apply is too low on this
# mesh (the polynomial is then indefinite and FCG stalls -- in the restatement as on the device), so the solve takes 15 iterations and 1.2
CHEBY_FCG = dict(CHEBY, cheby_eigs_cg_imax=15, cheby_eigs_max_multiplier=1.2)


@pytest.fixture(scope="module")
def levels(gpu, hiplib):
    H = L.Levels("two", gpu)
    yield H
    H.close()


def _gap(hist, lo, hi):
    """as tests/test_krylov_gpu.py::_gap"""
    h = np.asarray(hist, dtype=np.float64)
    best, jb = -1.0, None
    for j in range(max(lo, 2), min(hi, len(h))):
        g = np.log(h[1:j].min()) - np.log(h[j])
        if g > best:
            best, jb = g, j
    assert best > 0.05, best
    return jb, float(np.sqrt(h[1:jb].min() * h[jb]))


def _dev_cg_eigs(H, u, rhs, imax, use_new):
    import torch
    x = L.t(u, H.gpu)
    bound, _ = H.plans[-1].cg_eigs(x, L.t(rhs, H.gpu), torch.empty_like(x), imax, use_new)
    return bound, x.cpu().numpy()


def _dev_cheby(H, u, rhs, iters, lmin, lmax):
    import torch
    x = L.t(u, H.gpu)
    H.plans[-1].cheby_iterate(x, L.t(rhs, H.gpu), torch.empty_like(x), torch.empty_like(x), iters, lmin, lmax, 0)
    return x.cpu().numpy()


def _ref_pc_cheby(H, st, reuse, zero, C=CHEBY):
    return lambda r: RZ.pc_cheby_apply(st, lambda u, b, i, n: _dev_cg_eigs(H, u, b, i, n), lambda u, b, i, lo, hi: _dev_cheby(H, u, b, i, lo, hi),
                                       r, C["cheby_imax"], C["cheby_eigs_cg_imax"], C["cheby_eigs_lmax_lmin_ratio"],
                                       C["cheby_eigs_max_multiplier"], reuse, C["cheby_use_new_cg_eigs"], zero)


@pytest.mark.parametrize("zero", [0, 1])
@pytest.mark.parametrize("reuse", [0, 1])
def test_pc_cheby_apply_against_the_restatement(levels, gpu, reuse, zero):
    import torch
    from disco4est_amd import PcCheby, mesh as M
    H = levels
    pc = PcCheby(H.plans[-1], cheby_reuse_eig=reuse, cheby_use_zero_guess_for_eigs=zero, **CHEBY)
    try:
        assert pc.eig() == (-1.0, 0)
        st = RZ.PcChebyState()
        ref = _ref_pc_cheby(H, st, reuse, zero)
        for k in range(3):
            r = M.splitmix64_uniform(200 + k, H.nodes[-1]) - 0.5
            z = torch.full((H.nodes[-1],), float("nan"), dtype=torch.float64, device=gpu)
            pc.apply(L.t(r, gpu), z)
            z_ref = ref(r)
            eig, runs = pc.eig()
            print("pc_cheby reuse=%d zero=%d apply %d: eig %.15e (restatement %.15e), runs %d, |z - z_ref| %.3e"
                  % (reuse, zero, k, eig, st.eig, runs, L.rel(z.cpu().numpy(), z_ref)))
            assert runs == st.runs == (1 if reuse else k + 1)
            assert eig == st.eig > 0
            assert np.array_equal(z.cpu().numpy(), z_ref)
        pc.reset_eig()
        assert pc.eig() == (-1.0, st.runs)
    finally:
        pc.destroy()


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("kind", ["two", "mixed", "hanging"])
def test_pc_schwarz_apply_is_zero_fill_and_iterate(gpu, hiplib, kind, fused, monkeypatch):
    """the store-form correction: one pass equals a zero fill followed by Schwarz.iterate, bit for bit (z is not read: it starts as NaN);
    two passes equal the restatement on the device primitives, with the second pass's residual formed by its own kernel (the default)
    and inside the CG start (fused: D4EST_HIP_SCHWARZ_FUSED_RESIDUAL=1 when the handle is created)"""
    import torch
    from disco4est_amd import PcSchwarz
    monkeypatch.delenv("D4EST_HIP_SCHWARZ_UNFUSED_RESIDUAL", raising=False)
    if fused:
        monkeypatch.setenv("D4EST_HIP_SCHWARZ_FUSED_RESIDUAL", "1")
    else:
        monkeypatch.delenv("D4EST_HIP_SCHWARZ_FUSED_RESIDUAL", raising=False)
    H = L.Levels(kind, gpu, sub=(12, 1e-15, 1e-4), schwarz_levels=[1])
    try:
        sz, plan = H.schwarz[1], H.plans[1]
        _, r = H.problem(81)
        dr = L.t(r, gpu)
        pc = PcSchwarz(sz, plan, 1)
        z = torch.full_like(dr, float("nan"))
        pc.apply(dr, z)
        want = torch.zeros_like(dr)
        sweeps = sz.iterate(want, dr)
        assert sweeps > 0 and torch.equal(z, want) and float(z.abs().max()) > 0
        pc.destroy()
        pc2 = PcSchwarz(sz, plan, 2)
        z2 = torch.full_like(dr, float("nan"))
        pc2.apply(dr, z2)
        ref = RZ.pc_schwarz_apply(lambda v: H.apply(1, v), lambda u, res: H.schwarz_iterate(1, u, res), r, 2)
        assert np.array_equal(z2.cpu().numpy(), ref)
        pc2.destroy()
    finally:
        H.close()


def _fcg_case(H, gpu, pc_dev, pc_ref, lo, hi, seed=71):
    import torch
    top = H.plans[-1]
    u0, rhs = H.problem(seed)
    apply = lambda x: H.apply(H.n_levels - 1, x)
    _, _, h_all, _ = RS.fcg_solve(apply, u0, rhs, hi, 0.0, 0.0, pc=pc_ref())
    j, tol = _gap(h_all, lo, hi)                     # |r_j| <= tol: stop after update j (count j + 1)
    atol, rtol, imax = 0.0, tol / h_all[0], 400
    u_ref, it_ref, h_ref, _ = RS.fcg_solve(apply, u0, rhs, imax, atol, rtol, pc=pc_ref())
    assert it_ref == j + 1
    du, drhs = L.t(u0, gpu), L.t(rhs, gpu)
    dAu = torch.full_like(du, float("nan"))
    it, hist = top.fcg_solve(du, drhs, dAu, imax, atol, rtol, pc=pc_dev)
    dv = L.t(u0, gpu)
    it_plain, _ = top.fcg_solve(dv, drhs, dAu, 2000, atol, rtol, pc=None)
    n = min(it, it_ref)
    print("fcg: iterations %d (restatement %d, no preconditioner %d), history %.3e, u %.3e"
          % (it, it_ref, it_plain, np.max(np.abs(hist[:n] / np.array(h_ref[:n]) - 1)), L.rel(du.cpu().numpy(), u_ref)))
    assert it == it_ref
    assert np.abs(hist - np.array(h_ref)).max() <= 1e-8 * h_ref[0]
    assert L.rel(du.cpu().numpy(), u_ref) <= U_TOL_PC
    assert it < it_plain


def test_fcg_with_pc_cheby(levels, gpu):
    from disco4est_amd import PcCheby
    H = levels
    pc = PcCheby(H.plans[-1], cheby_reuse_eig=1, cheby_use_zero_guess_for_eigs=1, **CHEBY_FCG)
    try:
        assert isinstance(pc.pc_fn, int) and pc.pc_fn != 0 and pc.pc_ctx == pc.handle

        def pc_ref():
            st = RZ.PcChebyState()
            return _ref_pc_cheby(H, st, 1, 1, CHEBY_FCG)

        # (a fresh state per restated solve; the device object makes one preconditioned solve, from no bound)
        _fcg_case(H, gpu, pc, pc_ref, 4, 14)
        assert pc.eig()[1] == 1
    finally:
        pc.destroy()


def test_fcg_with_pc_schwarz(levels, gpu):
    from disco4est_amd import PcSchwarz
    H = levels
    pc = PcSchwarz(H.schwarz[1], H.plans[1], 2)
    try:
        pc_ref = lambda: (lambda r: RZ.pc_schwarz_apply(lambda v: H.apply(1, v), lambda u, res: H.schwarz_iterate(1, u, res), r, 2))
        _fcg_case(H, gpu, pc, pc_ref, 4, 14)
    finally:
        pc.destroy()


def test_fcg_with_multigrid_schwarz(levels, gpu):
    H = levels
    mg = H.multigrid()
    assert mg.set_smoother_schwarz(H.schwarz, 1) == 0
    mg.set_bottom_solver_cg(12, 0.0, 0.0)
    mg.set_pc(1, 0.0, 0.0)

    def pc_ref():
        def pc(r):
            sm = RZ.SchwarzSmoother(1, H.schwarz_iterate)
            return RM.pc_apply(H.hierarchy(), sm, RM.BottomCG(12, 0.0, 0.0), r, 1, 0.0, 0.0)
        return pc

    _fcg_case(H, gpu, mg, pc_ref, 3, 10)
