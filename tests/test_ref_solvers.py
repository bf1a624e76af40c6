"""Pins of the numpy restatement of the reference's Krylov solvers (tests/ref_solvers.py), the yardstick of tests/test_krylov_gpu.py.
No GPU."""
import numpy as np

from tests import ref_solvers as R


def _tridiag(n, seed=3):
    rng = np.random.default_rng(seed)
    off = -1.0 - 0.2 * rng.random(n - 1)
    A = np.diag(4.0 + rng.random(n)) + np.diag(off, 1) + np.diag(off, -1)
    return A, rng.random(n) - 0.5


def test_cg_converges_to_the_direct_solve_within_n_iterations():
    A, b = _tridiag(24)
    u, it, hist, _ = R.cg_solve(lambda x: A @ x, np.zeros(24), b, 24, 0.0, 1e-13)
    assert it <= 24
    assert np.abs(u - np.linalg.solve(A, b)).max() <= 1e-11 * np.abs(u).max()
    assert len(hist) == it + 1 and hist[-1] <= 1e-26 * hist[0]


def test_cg_stop_rule_and_edge_cases():
    A, b = _tridiag(16)
    u0 = np.linspace(-1, 1, 16)
    # imax = 0: nothing moves, Au is A u of the start
    u, it, hist, Au = R.cg_solve(lambda x: A @ x, u0, b, 0, 1e-3, 1e-3)
    assert it == 0 and np.array_equal(u, u0) and np.allclose(Au, A @ u0) and len(hist) == 1
    # a start at the exact solution (rhs = A x with the same apply: r = 0 exactly) meets the test before the first iteration
    x = np.linalg.solve(A, b)
    u, it, hist, _ = R.cg_solve(lambda y: A @ y, x, A @ x, 10, 0.0, 0.0)
    assert it == 0 and hist == [0.0] and np.array_equal(u, x)
    # (FCG has no test before its first update, :283: from r = 0 the reference divides 0 by rho = 0)
    # the loop test delta > atol^2 + delta_0 rtol^2 holds before every iteration made and fails after the last
    _, it, hist, _ = R.cg_solve(lambda y: A @ y, np.zeros(16), b, 100, 1e-7, 1e-4)
    thr = 1e-7 * 1e-7 + hist[0] * 1e-4 * 1e-4
    assert 0 < it < 16 and all(h > thr for h in hist[:-1]) and hist[-1] <= thr


def test_fcg_identity_reproduces_cg_iterates():
    A, b = _tridiag(20, seed=5)
    apply = lambda x: A @ x  # noqa: E731
    for k in (1, 3, 6):
        u_cg, it_cg, _, _ = R.cg_solve(apply, np.zeros(20), b, k, 0.0, 0.0)
        u_f, it_f, _, _ = R.fcg_solve(apply, np.zeros(20), b, k, 0.0, 0.0)
        assert it_cg == it_f == k
        assert np.abs(u_f - u_cg).max() <= 1e-12 * np.abs(u_cg).max()


def test_fcg_stop_rule_and_preconditioner():
    A, b = _tridiag(30, seed=7)
    apply = lambda x: A @ x  # noqa: E731
    u, it, hist, _ = R.fcg_solve(apply, np.zeros(30), b, 200, 0.0, 1e-10)
    tol = 1e-10 * np.linalg.norm(b)
    # the test is on |r_k| (before the update) after the update: the last recorded norm meets it, the ones before do not
    assert it == len(hist) and hist[-1] <= tol and all(h > tol for h in hist[1:-1])
    assert np.linalg.norm(b - A @ u) <= tol
    # Jacobi preconditioning of a badly scaled system cuts the count
    S = np.diag(np.geomspace(1.0, 1e3, 30))
    As = S @ A @ S
    Dinv = 1.0 / np.diag(As)
    _, it_plain, _, _ = R.fcg_solve(lambda x: As @ x, np.zeros(30), b, 500, 0.0, 1e-10)
    _, it_pc, _, _ = R.fcg_solve(lambda x: As @ x, np.zeros(30), b, 500, 0.0, 1e-10, pc=lambda r: Dinv * r)
    assert it_pc < it_plain


def test_allreduce_counts():
    assert R.cg_allreduce_calls(0) == 1 and R.cg_allreduce_calls(5) == 11
    assert R.fcg_allreduce_calls(1) == (2, 3) and R.fcg_allreduce_calls(3) == (4, 11)
