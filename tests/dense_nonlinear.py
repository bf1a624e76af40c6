"""An independent numpy restatement of the nonlinear power term f(x, u) = a (b + u)^k of the reference's shipped nonlinear problems
(the callbacks of src/Problems/ConstantDensityStar/constant_density_star_fcns.h:334-357 and
src/Problems/TwoPunctures/two_punctures_fcns.h:252-320), of its derivative in u, and of the reference's Newton loop
(src/Solver/d4est_solver_newton.c:196-344) around a residual and a linear-solve callable.  Shares no code with the library."""
import numpy as np


def power(base, k):
    """base^k as |k| multiplications; k < 0: one division of 1 by the product (never pow)"""
    base = np.asarray(base, dtype=np.float64)
    p = np.ones_like(base)
    for _ in range(abs(int(k))):
        p = p * base
    return 1.0 / p if k < 0 else p


def term(a, b, u, k):
    """f = a (b + u)^k; b None: b = 0"""
    u = np.asarray(u, dtype=np.float64)
    return a * power(u if b is None else b + u, k)


def dterm(a, b, u, k):
    """df/du = k a (b + u)^(k-1); k = 0: exactly 0"""
    u = np.asarray(u, dtype=np.float64)
    if int(k) == 0:
        return np.zeros_like(a * u)
    return (float(k) * a) * power(u if b is None else b + u, int(k) - 1)


def newton(residual, solve, x, atol, rtol, imin, imax):
    """d4est_solver_newton_solve: residual(x) -> F(x); solve(x, minus_f) -> the step from a zero initial guess for J(x) step = -F(x).
    Returns (ierr, x, history of |F|, iterations + 1 entries)."""
    f0 = residual(x)                                              # :196-208
    fnrm = float(np.sqrt(np.dot(f0, f0)))                         # :210-223
    stop_tol = atol + rtol * fnrm                                 # :226
    itc = 0
    hist = [fnrm]
    while (fnrm > stop_tol or itc < imin) and itc < imax:         # :234
        f0 = -1.0 * f0                                            # :238
        step = solve(x, f0)                                       # :240-263
        x = 1.0 * step + x                                        # :266 (always the full step)
        f0 = residual(x)                                          # :268-290
        fnrm = float(np.sqrt(np.dot(f0, f0)))                     # :293-305
        hist.append(fnrm)
        itc += 1                                                  # :343
    return (1 if fnrm > stop_tol else 0), x, hist                 # :346-348
