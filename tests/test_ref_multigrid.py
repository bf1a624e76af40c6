"""Pins of the numpy restatement of the reference's multigrid (tests/ref_multigrid.py), the yardstick of tests/test_vcycle_gpu.py, on
small dense SPD matrices with dense prolongations.  No GPU, no oracle."""
import numpy as np
import pytest

from tests import ref_multigrid as R


def _spd(n, seed):
    """a 1-D Laplacian-like SPD matrix with a perturbed diagonal"""
    rng = np.random.default_rng(seed)
    return np.diag(2.0 + 0.3 * rng.random(n)) - np.diag(np.ones(n - 1), 1) - np.diag(np.ones(n - 1), -1)


def _interp(nc, seed=0):
    """linear interpolation nc -> 2 nc + 1 (full column rank), slightly perturbed so that nothing is special"""
    nf = 2 * nc + 1
    P = np.zeros((nf, nc))
    for j in range(nc):
        P[2 * j, j] += 0.5
        P[2 * j + 1, j] = 1.0
        P[2 * j + 2, j] += 0.5
    return P + 0.01 * np.random.default_rng(seed).random((nf, nc)) * (P != 0)


def _galerkin_hierarchy(n_levels, n_bottom=5, seed=11):
    """As[top] SPD, As[l] = P^T As[l+1] P"""
    sizes = [n_bottom]
    for _ in range(n_levels - 1):
        sizes.append(2 * sizes[-1] + 1)
    Ps = [_interp(sizes[l], seed + l) for l in range(n_levels - 1)]
    As = [None] * n_levels
    As[-1] = _spd(sizes[-1], seed)
    for l in range(n_levels - 2, -1, -1):
        As[l] = Ps[l].T @ As[l + 1] @ Ps[l]
    return As, Ps


def test_two_level_cycle_without_smoothing_is_the_coarse_grid_correction():
    """(a) cheby_imax = 0, exact bottom solve, A_c = P^T A P: one cycle is u + P A_c^-1 P^T (rhs - A u); a second cycle changes
    nothing beyond rounding (the correction is an A-orthogonal projection)"""
    As, Ps = _galerkin_hierarchy(2)
    A, Ac, P = As[1], As[0], Ps[0]
    rng = np.random.default_rng(1)
    u0, rhs = rng.random(A.shape[0]) - 0.5, rng.random(A.shape[0]) - 0.5
    h = R.dense_hierarchy(As, Ps)
    # reuse from the down leg and a zero guess: the cg_eigs of the down leg does not touch u, the up leg runs none
    sm = R.ChebySmoother(2, 0, 3, 30.0, 1.0, cheby_eigs_reuse_fromdownvcycle=1, cheby_use_zero_guess_for_eigs=1)
    bottom = R.BottomCG(200, 0.0, 1e-15)
    u1, r2 = R.vcycle(h, sm, bottom, u0, rhs, 0)
    want = u0 + P @ np.linalg.solve(Ac, P.T @ (rhs - A @ u0))
    assert np.abs(u1 - want).max() <= 1e-12 * np.abs(want).max()
    r = rhs - A @ u1
    assert abs(r2 - r @ r) <= 1e-12 * (r @ r)
    u2, _ = R.vcycle(h, sm, bottom, u1, rhs, 1)
    assert np.abs(u2 - u1).max() <= 1e-11 * np.abs(u1).max()
    # with the cg_eigs of the smoother starting from the iterate it advances u (as the reference does): the cycle then differs
    sm2 = R.ChebySmoother(2, 0, 3, 30.0)
    u3, _ = R.vcycle(h, sm2, bottom, u0, rhs, 0)
    assert np.abs(u3 - want).max() > 1e-6 * np.abs(want).max()


def test_three_level_arena_indexing():
    """(b) each level's vectors are the ones used: the trace lists every level vector with its level's length, in the order of the
    reference's V (down: smooth, restrict; bottom; up: prolong, smooth)"""
    As, Ps = _galerkin_hierarchy(3)
    h = R.dense_hierarchy(As, Ps)
    n0, n1, n2 = h.nodes
    assert len({n0, n1, n2}) == 3
    rng = np.random.default_rng(2)
    u0, rhs = rng.random(n2) - 0.5, rng.random(n2) - 0.5
    trace = []
    sm = R.ChebySmoother(3, 2, 4, 20.0, 1.1)
    bottom = R.BottomCheby(4, 4, 20.0, 1.1)
    u1, r2 = R.vcycle(h, sm, bottom, u0, rhs, 0, trace=trace)
    assert trace == [("smooth", 2, n2), ("restrict_in", 2, n2), ("restrict_out", 1, n1),
                     ("smooth", 1, n1), ("restrict_in", 1, n1), ("restrict_out", 0, n0),
                     ("bottom", 0, n0),
                     ("prolong_in", 0, n0), ("prolong_out", 1, n1), ("smooth", 1, n1),
                     ("prolong_in", 1, n1), ("prolong_out", 2, n2), ("smooth", 2, n2)]
    r = rhs - As[2] @ u1
    assert abs(r2 - r @ r) <= 1e-12 * (r @ r)           # vcycle_r2 is |rhs - A u|^2 of the final iterate
    assert r2 < (rhs - As[2] @ u0) @ (rhs - As[2] @ u0)  # and the cycle reduces the residual
    assert all(e > 0 for e in sm.eigs[1:]) and sm.eigs[0] == -1.0 and bottom.eig > 0
    # the multiplier is applied: eigs = 1.1 * the bound of the last cg_eigs of the level (the up leg's, from the corrected iterate)
    assert bottom.iterations == 4


def test_stop_rule():
    """(c) stoptol = rtol^2 r2_0 + atol^2 as written, and the >= 0.99 stagnation break"""
    As, Ps = _galerkin_hierarchy(2)
    h = R.dense_hierarchy(As, Ps)
    rng = np.random.default_rng(3)
    n = h.nodes[1]
    u0, rhs = np.zeros(n), rng.random(n) - 0.5
    mk = lambda: (R.ChebySmoother(2, 3, 4, 30.0, 1.1), R.BottomCG(100, 0.0, 1e-14))  # noqa: E731
    _, cycles, hist = R.solve(h, *mk(), u0, rhs, 30, 0.0, 1e-6)
    stoptol = 1e-6 * 1e-6 * hist[0]
    assert 1 <= cycles < 30 and len(hist) == cycles + 1
    assert all(x > stoptol for x in hist[:-1]) and hist[-1] <= stoptol
    assert hist[0] == float(rhs @ rhs)
    # atol alone: stoptol = atol^2
    atol = float(np.sqrt(hist[2] * 1.5))
    _, c2, h2 = R.solve(h, *mk(), u0, rhs, 30, atol, 0.0)
    assert c2 == 2 and h2[-1] <= atol * atol < h2[-2]
    # imax bounds the count; a start that meets the test runs no cycle
    _, c3, h3 = R.solve(h, *mk(), u0, rhs, 1, 0.0, 1e-12)
    assert c3 == 1 and len(h3) == 2
    _, c4, h4 = R.solve(h, *mk(), u0, rhs, 5, 10.0 * float(np.sqrt(hist[0])), 0.0)
    assert c4 == 0 and len(h4) == 1
    # a deliberately useless smoother (no iterations) on a hierarchy whose coarse space is useless too (a zero prolongation): r2 does
    # not move, sqrt(r2 / r2_last) = 1 >= 0.99 fires after exactly one cycle
    hz = R.dense_hierarchy(As, [np.zeros_like(Ps[0])])
    hz.apply = lambda l, x: (As[l] @ x if l == 1 else x)          # (P = 0 makes P^T A P singular: the identity below)
    sm = R.ChebySmoother(2, 0, 2, 30.0, cheby_eigs_reuse_fromdownvcycle=1, cheby_use_zero_guess_for_eigs=1)
    _, c5, h5 = R.solve(hz, sm, R.BottomCG(1, 0.0, 0.0), u0, rhs, 10, 0.0, 1e-10)
    assert c5 == 1 and h5[1] == h5[0]


@pytest.mark.parametrize("fromdown", [0, 1])
@pytest.mark.parametrize("fromlast", [0, 1])
def test_eigenvalue_reuse_table(fromdown, fromlast):
    """(d) cg_eigs calls per level in the cycles with vcycle_index 0 and 1, from smoother_cheby.c:234-257:
         (fromdown, fromlast)   index 0   index 1
         (0, 0)                 2         2         down and up leg compute, every cycle
         (1, 0)                 1         1         the down leg's value serves the up leg
         (0, 1)                 2         0         the first cycle's values serve all later cycles
         (1, 1)                 1         0
       on every smoothed level (1 ... top); level 0 belongs to the bottom solver"""
    table = {(0, 0): (2, 2), (1, 0): (1, 1), (0, 1): (2, 0), (1, 1): (1, 0)}
    As, Ps = _galerkin_hierarchy(3)
    h = R.dense_hierarchy(As, Ps)
    rng = np.random.default_rng(4)
    n = h.nodes[2]
    u, rhs = rng.random(n) - 0.5, rng.random(n) - 0.5
    sm = R.ChebySmoother(3, 2, 3, 30.0, 1.1, fromdown, fromlast)
    bottom = R.BottomCG(50, 0.0, 1e-12)
    for index in (0, 1):
        sm.eigs_calls = [0, 0, 0]
        before = list(sm.eigs)
        u, _ = R.vcycle(h, sm, bottom, u, rhs, index)
        want = table[(fromdown, fromlast)][index]
        assert sm.eigs_calls == [0, want, want]
        assert sm.eigs_calls == R.expected_eigs_calls(3, fromdown, fromlast, index)
        if want == 0:
            assert sm.eigs == before       # reused, bit for bit
        else:
            assert all(a != b for a, b in zip(sm.eigs[1:], before[1:]))


def test_zero_guess_needs_reuse_from_the_down_leg():
    """(e) smoother_cheby.c:313-318"""
    As, Ps = _galerkin_hierarchy(2)
    h = R.dense_hierarchy(As, Ps)
    n = h.nodes[1]
    sm = R.ChebySmoother(2, 2, 3, 30.0, cheby_eigs_reuse_fromdownvcycle=0, cheby_use_zero_guess_for_eigs=1)
    with pytest.raises(RuntimeError, match="cheby_eigs_reuse_fromdownvcycle"):
        R.vcycle(h, sm, R.BottomCG(10, 0.0, 1e-10), np.zeros(n), np.ones(n), 0)
    # with it the zero guess leaves u alone: the same bound whatever u is
    sm1 = R.ChebySmoother(2, 0, 3, 30.0, cheby_eigs_reuse_fromdownvcycle=1, cheby_use_zero_guess_for_eigs=1)
    sm2 = R.ChebySmoother(2, 0, 3, 30.0, cheby_eigs_reuse_fromdownvcycle=1, cheby_use_zero_guess_for_eigs=1)
    rhs = np.linspace(-1, 1, n)
    R.vcycle(h, sm1, R.BottomCG(10, 0.0, 1e-10), np.zeros(n), rhs, 0)
    R.vcycle(h, sm2, R.BottomCG(10, 0.0, 1e-10), np.ones(n), rhs, 0)
    assert sm1.eigs[1] == sm2.eigs[1] > 0


def test_dense_kernels_against_linear_algebra():
    """the two numpy kernels the pins stand on: cg_eigs' bound is the largest Gershgorin row bound of the Lanczos tridiagonal (the old
    form sums both off-diagonal entries of a row, the new one the lower one only: old >= new, both of the size of lambda_max(A));
    n cg_eigs iterations solve the system; Chebyshev iterations on the exact window contract"""
    A = _spd(12, 5)
    lam = np.linalg.eigvalsh(A)
    rng = np.random.default_rng(6)
    rhs = rng.random(12) - 0.5
    bounds = []
    for use_new in (0, 1):
        bound, u = R.dense_cg_eigs(A, np.zeros(12), rhs, 12, use_new)
        assert 0.5 * lam[-1] <= bound <= 2.5 * lam[-1]
        assert np.abs(u - np.linalg.solve(A, rhs)).max() <= 1e-8
        bounds.append(bound)
    assert bounds[0] >= bounds[1]
    u, r = R.dense_cheby_iterate(A, np.zeros(12), rhs, 25, lam[0], lam[-1])
    assert np.abs(r - (rhs - A @ u)).max() <= 1e-14
    assert np.linalg.norm(r) <= 1e-3 * np.linalg.norm(rhs)
    u0, r0 = R.dense_cheby_iterate(A, np.ones(12), rhs, 0, 1.0, 2.0)
    assert np.array_equal(u0, np.ones(12)) and np.array_equal(r0, rhs + (-1.0) * (A @ np.ones(12)))


def test_pc_apply_is_the_solve_from_zero():
    As, Ps = _galerkin_hierarchy(3)
    h = R.dense_hierarchy(As, Ps)
    n = h.nodes[2]
    r = np.random.default_rng(7).random(n) - 0.5
    mk = lambda: (R.ChebySmoother(3, 2, 3, 30.0, 1.1), R.BottomCG(50, 0.0, 1e-12))  # noqa: E731
    z = R.pc_apply(h, *mk(), r, 1, 0.0, 0.0)
    u, cycles, _ = R.solve(h, *mk(), np.zeros(n), r, 1, 0.0, 0.0)
    assert cycles == 1 and np.array_equal(z, u)
    # as a preconditioner of the restated FCG it cuts the iteration count
    from tests import ref_solvers
    A = As[2]
    _, it_plain, _, _ = ref_solvers.fcg_solve(lambda x: A @ x, np.zeros(n), r, 200, 0.0, 1e-10)
    _, it_pc, _, _ = ref_solvers.fcg_solve(lambda x: A @ x, np.zeros(n), r, 200, 0.0, 1e-10, pc=lambda v: R.pc_apply(h, *mk(), v, 1, 0.0, 0.0))
    assert it_pc < it_plain
