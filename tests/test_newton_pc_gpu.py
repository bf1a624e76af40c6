"""d4est_hip_newton_solve with the Chebyshev and the Schwarz Krylov preconditioners (d4est_hip_pc_cheby_apply, d4est_hip_pc_schwarz_apply)
on one rank: both pass through the same pc / pc_ctx pair as the multigrid one.  The Okendon fixture of tests/test_okendon_newton_gpu.py
at p = 3, held to what tests/test_newton_gpu.py::test_newton_with_a_multigrid_preconditioner asks of its preconditioned solve: the
|F| history has the length of the unpreconditioned solve's and agrees with it to 1e-6 relative (the preconditioner must not change the
Newton iterates beyond the Krylov tolerance), and |F| ends below atol + rtol |F_0|."""
import numpy as np
import pytest

from tests.test_okendon_newton_gpu import NEWTON, _setup

pytestmark = pytest.mark.gpu


def test_newton_with_the_cheby_and_schwarz_preconditioners(gpu, hiplib):
    import torch
    from disco4est_amd import PcCheby, PcSchwarz
    from disco4est_amd.schwarz import Schwarz
    m, plan, g, u_star = _setup(gpu, 3)
    u0 = torch.ones(m.local_nodes, dtype=torch.float64, device=gpu)
    ierr0, its0, hist0 = plan.newton_solve(u0, None, g, pc=None, **NEWTON)
    assert ierr0 == 0 and its0 >= 2
    # the brick [1, 2]^3 is the unit cube shifted: the mesh's own geometric factors are the plan's
    J, rst = m.geometry()
    sz = Schwarz(m, m.build_sides(), J, rst, 2, 12, 1e-15, 1e-4)
    cheby = PcCheby(plan, 4, 10, 30.0, 1.1, cheby_reuse_eig=0, cheby_use_new_cg_eigs=1, cheby_use_zero_guess_for_eigs=1)
    schwarz = PcSchwarz(sz, plan, 2)
    try:
        for name, pc in (("cheby", cheby), ("schwarz", schwarz)):
            u = torch.ones_like(u0)
            ierr, its, hist = plan.newton_solve(u, None, g, pc=pc, **NEWTON)
            print("newton (Okendon, p = 3) pc = %s: history %s\n   no preconditioner: %s" % (name, list(hist), list(hist0)))
            assert ierr == 0 and its == its0 and len(hist) == len(hist0)
            big = hist0 > 1e-9 * hist0[0]                 # (as tests/test_okendon_newton_gpu.py: entries above 1e-9 of the first)
            assert np.all(np.abs(hist - hist0)[big] <= 1e-6 * hist0[big])
            assert hist[-1] <= NEWTON["atol"] + NEWTON["rtol"] * hist[0]
            assert float((u - u0).abs().max()) <= 100 * NEWTON["rtol"] * float(u_star.abs().max())
    finally:
        schwarz.destroy(); cheby.destroy(); sz.destroy(); plan.destroy()
