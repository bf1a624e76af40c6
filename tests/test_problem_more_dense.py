"""Pins tests/dense_problem_more.py without the reference binary: each analytic solution satisfies its own equation under a 7-point
finite-difference Laplacian, and the real-power Jacobian is the derivative of the residual term.

Step and bound.  The 7-point Laplacian L_h has truncation error c h^2 + O(h^4), so L_h - L_2h = -3 c h^2 + O(h^4): the difference of the
two stencils is three times the truncation error of L_h, and |L_h - L_2h| bounds it with the factor 3 covering the O(h^4) remainder
(relative size h^2 = 1e-6).  Rounding adds at most 8 function values of 1 ulp each, divided by h^2: 16 eps max|u| / h^2 asserted.
h = 1e-3: truncation about 1e-7 |d^4 u|, rounding about 4e-9 |u| -- the two are balanced within two orders and both far below the
O(1) right-hand sides.  Points are drawn from [0.5, 1.5]^3, at least 0.86 from the origin and 0.26 from the Stamm corner."""
import numpy as np

from tests import dense_problem_more as D

EPS = 2.0 ** -52
H = 1e-3
X = np.random.default_rng(1).uniform(0.5, 1.5, (3, 257))
STAMM = (0.25, 0.3, 0.35)
BY = (0.7, 1.3)


def _check(fn, params, rhs, name):
    """L_h fn = rhs within |L_h - L_2h| + 16 eps max|fn| / h^2"""
    L, L2 = D.laplacian_fd(fn, X, params, H), D.laplacian_fd(fn, X, params, 2 * H)
    bound = np.abs(L - L2) + 16 * EPS * np.abs(fn(*X, params)).max() / (H * H)
    err = np.abs(L - rhs)
    print("%s: worst error / bound = %.3f (max |rhs| = %.3e)" % (name, (err / bound).max(), np.abs(rhs).max()))
    assert np.all(err <= bound), name
    assert bound.max() <= 1e-3 * np.abs(rhs).max()        # the bound resolves the right-hand side: a wrong sign is an error of 200 %


def test_lorentzian_solves_its_poisson_problem():
    _check(D.lorentzian_u, None, -D.lorentzian_rhs(*X), "-Laplace(LORENTZIAN_U) = LORENTZIAN_RHS")


def test_lorentzian_robin_condition_on_a_sphere():
    """d/dr u + ROBIN u = 0 at |x| = R: the radial derivative by a centred difference along x / R, step h, truncation h^2 / 6 |u'''|
    bounded as above by the difference of the h and 2h quotients"""
    R = 3.0
    n = X / np.sqrt((X * X).sum(axis=0))
    P = R * n

    def ddr(h):
        return (D.lorentzian_u(*(P + h * n)) - D.lorentzian_u(*(P - h * n))) / (2 * h)
    d1, d2 = ddr(H), ddr(2 * H)
    u = D.lorentzian_u(*P)
    err = np.abs(d1 + D.lorentzian_robin(*P) * u)
    bound = np.abs(d1 - d2) + 4 * EPS * np.abs(u).max() / H
    assert np.all(err <= bound) and bound.max() <= 1e-5 * np.abs(d1).max()


def test_okendon_solution_solves_its_equation():
    for p in (0.5, 0.3):
        _check(D.okendon_u, [p], np.power(D.okendon_u(*X, [p]), p), "Laplace(OKENDON_U) = OKENDON_U^p, p = %g" % p)


def test_boyen_york_solution_and_coefficient():
    """Laplace(BY_PSI) + BY_A BY_PSI^-7 = 0 is the identity the two functions satisfy (residual 8e-7 at h = 1e-3 against a term of
    8e-3).  Note the sign: boyen_york_model_build_residual forms A u + V^T W J BY_A u^-7 with A u the weak -Laplace(u), i.e.
    -Laplace(u) + BY_A u^-7, which BY_PSI does NOT annihilate (it leaves 2 BY_A BY_PSI^-7, 1.6e-2 here).  The library follows the
    reference's statements (a = +BY_A, k = -7); this test pins the two functions to each other with the sign that holds."""
    psi = D.by_psi(*X, BY)
    term = D.by_a(*X, BY) * D.DN.power(psi, -7)
    _check(D.by_psi, BY, -term, "Laplace(BY_PSI) = -BY_A BY_PSI^-7")


def test_stamm_solution_solves_its_poisson_problem():
    _check(D.stamm_u, STAMM, -D.stamm_rhs(*X, STAMM), "-Laplace(STAMM_U) = STAMM_RHS")
    assert D.stamm_rhs(np.array([STAMM[0]]), np.array([STAMM[1]]), np.array([STAMM[2]]), STAMM)[0] == 0.0   # the branch at x = c2


def test_abs_power_jacobian_is_the_derivative_of_the_term():
    """centred difference with step d = 1e-5 at |t| >= 0.1: truncation d^2 / 6 max|f'''|, f''' = a s (s-1) (s-2) |t|^(s-3) sign(t),
    evaluated at the smallest |t| in reach (|t| - d); rounding 2 ulp of |f| over 2 d"""
    rng = np.random.default_rng(2)
    n = 257
    a = -(0.5 + rng.random(n))
    b = 0.1 + 0.2 * rng.random(n)
    u = np.where(rng.random(n) < 0.5, -1.0, 1.0) * (0.4 + rng.random(n))      # b + u in [-1.3, -0.1] or [0.5, 1.7]
    d = 1e-5
    for s in (0.5, 0.3):
        for bb in (b, None):
            t = u if bb is None else bb + u
            assert np.abs(t).min() >= 0.1
            fd = (D.abs_term(a, bb, u + d, s) - D.abs_term(a, bb, u - d, s)) / (2 * d)
            jac = np.sign(t) * D.abs_dterm(a, bb, u, s)         # the reference's callback is s / |t|^(1-s): the derivative in |t|
            f3 = np.abs(a * s * (s - 1) * (s - 2)) * np.power(np.abs(t) - d, s - 3)
            bound = d * d / 6 * f3 + 2 * EPS * np.abs(D.abs_term(a, bb, u, s)) / (2 * d)
            assert np.all(np.abs(fd - jac) <= bound)
            assert bound.max() <= 1e-6 * np.abs(jac).min()


def test_load_vector_is_the_integral_of_the_field():
    """load_vector hands the field's values to the integral unchanged"""
    got = D.load_vector(lambda f: 2.0 * f, "LORENTZIAN_RHS", X, None)
    assert np.array_equal(got, 2.0 * D.lorentzian_rhs(*X))
