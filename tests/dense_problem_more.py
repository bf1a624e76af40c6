"""Plain numpy restatements of the problem data of the Okendon, Boyen-York, Poisson/Lorentzian and Stamm families
(src/Problems/Okendon/okendon_fcns.h, BoyenYorkModel/boyen_york_model_fcns.h, Poisson/poisson_lorentzian_fcns.h, Stamm/stamm_fcns.h), of
the real-power term a |b + u|^s with its Jacobian, and of the load vector V^T W J f.  Builds on tests/dense_problem.py and
tests/dense_nonlinear.py by import; shares no code with the library."""
import numpy as np

from tests import dense_nonlinear as DN
from tests import dense_problem as DP   # noqa: F401  (quad_xyz / boundary_xyz: the coordinates these fields are evaluated at)


def okendon_u(x, y, z, params):
    p = float(params[0])
    M = 1. / (np.power((2. / (1. - p)) * (1 + (2. / (1. - p))), (1. / (1. - p))))
    r2 = x * x + y * y + z * z
    return M * np.power(r2, 1 / (1 - p))


def by_psi(x, y, z, params):
    a, P = float(params[0]), float(params[1])
    r2 = x * x + y * y + z * z
    r = np.sqrt(r2)
    r3 = r * r2
    r4 = r2 * r2
    E = np.sqrt(P * P + 4 * a * a)
    return np.power(1. + 2. * E / r + 6 * a * a / r2 + 2 * a * a * E / r3 + a * a * a * a / r4, .25)


def by_a(x, y, z, params):
    a, P = float(params[0]), float(params[1])
    r2 = x * x + y * y + z * z
    r4 = r2 * r2
    return .75 * (P * P / r4) * (1 - (a * a / r2)) * (1 - (a * a / r2))


def lorentzian_u(x, y, z, params=None):
    r = np.sqrt(x * x + y * y + z * z)
    return 1. / np.sqrt(1. + r * r)


def lorentzian_rhs(x, y, z, params=None):
    return 3. / np.power((1. + x * x + y * y + z * z), 2.5)


def lorentzian_robin(x, y, z, params=None):
    r2 = x * x + y * y + z * z
    return np.sqrt(r2) / (1. + r2)


def stamm_u(x, y, z, params):
    xp, yp, zp = x - params[0], y - params[1], z - params[2]
    rp = np.sqrt(xp * xp + yp * yp + zp * zp)
    return x * (1. - x) * y * (1. - y) * z * (1. - z) * ((rp * rp) * rp)


def stamm_rhs_terms(x, y, z, params):
    """the thirteen signed terms of stamm_rhs_fcn's numerator (DIM == 3) and sqrt(S)"""
    c2x, c2y, c2z = (float(v) for v in params[:3])
    dx2, dy2, dz2 = (c2x - x) * (c2x - x), (c2y - y) * (c2y - y), (c2z - z) * (c2z - z)
    S = dx2 + dy2 + dz2
    S2 = S * S
    t = [-2 * (1 - x) * x * (1 - y) * y * S2,
         9 * (1 - x) * x * (1 - y) * y * S * (1 - z) * z,
         6 * (1 - x) * (-c2x + x) * (1 - y) * y * S * (1 - z) * z,
         -(6 * x * (-c2x + x) * (1 - y) * y * S * (1 - z) * z),
         6 * (1 - x) * x * (1 - y) * (-c2y + y) * S * (1 - z) * z,
         -(6 * (1 - x) * x * y * (-c2y + y) * S * (1 - z) * z),
         -(2 * (1 - x) * x * S2 * (1 - z) * z),
         -(2 * (1 - y) * y * S2 * (1 - z) * z),
         -(3 * dx2 * (-1 + x) * x * (-1 + y) * y * (-1 + z) * z),
         -(3 * (-1 + x) * x * dy2 * (-1 + y) * y * (-1 + z) * z),
         -(3 * (-1 + x) * x * (-1 + y) * y * dz2 * (-1 + z) * z),
         6 * (1 - x) * x * (1 - y) * y * S * (1 - z) * (-c2z + z),
         -(6 * (1 - x) * x * (1 - y) * y * S * z * (-c2z + z))]
    return t, np.sqrt(S)


def stamm_rhs(x, y, z, params):
    t, rS = stamm_rhs_terms(x, y, z, params)
    num = t[0]
    for v in t[1:]:
        num = num + v
    with np.errstate(invalid="ignore", divide="ignore"):
        ret = -1 * (num / rS)
    return np.where(rS == 0, 0., ret)


FIELDS = {"OKENDON_U": okendon_u, "BY_PSI": by_psi, "BY_A": by_a, "LORENTZIAN_U": lorentzian_u, "LORENTZIAN_RHS": lorentzian_rhs,
          "LORENTZIAN_ROBIN": lorentzian_robin, "STAMM_U": stamm_u, "STAMM_RHS": stamm_rhs}


def abs_term(a, b, u, s):
    """f = a |b + u|^s the reference's way: a pow(t t, s / 2); b None: b = 0"""
    u = np.asarray(u, dtype=np.float64)
    t = u if b is None else b + u
    return a * np.power(t * t, .5 * s)


def abs_dterm(a, b, u, s):
    """df/du = s a |b + u|^(s-1) as s a / pow(t t, (1 - s) / 2)"""
    u = np.asarray(u, dtype=np.float64)
    t = u if b is None else b + u
    return (s * a) / np.power(t * t, .5 * (1. - s))


def load_vector(galerkin, field, X, params):
    """V^T W J f(x_quad): `galerkin` is the integral of a quadrature-node array (the oracle's d4est_quadrature_apply_galerkin_integral),
    X the quadrature coordinates [3, nq]"""
    return galerkin(FIELDS[field](X[0], X[1], X[2], params))


def laplacian_fd(fn, X, params, h):
    """the 7-point finite-difference Laplacian of fn at the points X[3, n]"""
    s = -6.0 * fn(X[0], X[1], X[2], params)
    for d in range(3):
        e = np.zeros((3, 1))
        e[d] = h
        s = s + fn(*(X + e), params) + fn(*(X - e), params)
    return s / (h * h)


def newton_abs_power(apply_A, interpolate, galerkin, solve_lhs, a, b, s, x0, atol, rtol, imin, imax):
    """the reference's Newton loop (DN.newton, d4est_solver_newton.c:196-344) on F(x) = A x + V^T W J a |b + V x|^s, the shape of
    okendon_build_residual / okendon_apply_jac.  apply_A(x): the Laplacian with the inhomogeneous boundary data; interpolate(x): V x;
    galerkin(f): V^T W J f; solve_lhs(c, minus_f): the step from a zero guess for (A_0 + V^T W J c V) step = minus_f, A_0 the Laplacian
    with the boundary data zeroed.  The term and its Jacobian are abs_term / abs_dterm at the iterate's own V x."""
    state = {}

    def residual(x):
        state["xq"] = xq = interpolate(x)
        return apply_A(x) + galerkin(abs_term(a, b, xq, s))

    def solve(x, minus_f):
        return solve_lhs(abs_dterm(a, b, state["xq"], s), minus_f)

    return DN.newton(residual, solve, x0, atol, rtol, imin, imax)
