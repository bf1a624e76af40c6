"""A restatement in numpy of the reference's Krylov solvers, the yardstick of the device solves (tests/test_krylov_gpu.py).

`apply` is any callable u -> A u: a dense matrix in the pins (tests/test_ref_solvers.py), the oracle's apply_lhs (the registered
operator: oracle.set_operator with set_hanging / set_lhs_coefficient / set_lhs_element_blocks) on the GPU tests.  Every product and sum
is rounded one by one, in the reference's statement order; the dot products are numpy's.
"""
import math

import numpy as np


def cg_solve(apply, u, rhs, imax, atol, rtol):
    """d4est_solver_cg_solve (src/Solver/d4est_solver_cg.c:76-197).  Returns (u, iterations, [delta_0, delta_1, ...], Au) where Au is
    what the reference leaves in vecs->Au: A d of the last iteration, A u of the start when no iteration ran."""
    u = np.array(u, dtype=np.float64, copy=True)
    Au = apply(u)                                    # :116-127
    r = rhs + (-1.0) * Au                            # :129-132 (copy, xpby(rhs, -1, r))
    d = r.copy()                                     # :133
    delta = float(np.dot(r, r))                      # :134, :139-143
    delta0 = delta
    hist = [delta]
    i = 0
    while i < imax and delta > atol * atol + delta0 * rtol * rtol:    # :148
        Au = apply(d)                                # :150-161 (vecs->u = d)
        alpha = delta / float(np.dot(d, Au))         # :163-169
        u = u + alpha * d                            # :171
        r = r + (-alpha) * Au                        # :174
        delta_old = delta                            # :176
        delta = float(np.dot(r, r))                  # :177-181
        beta = delta / delta_old                     # :183
        d = r + beta * d                             # :184
        hist.append(delta)
        i += 1
    return u, i, hist, Au


def fcg_solve(apply, u, rhs, imax, atol, rtol, pc=None):
    """d4est_solver_fcg_solve as built (src/Solver/d4est_solver_fcg_improved.c:97-346); pc: r -> B r, None = the identity
    (do_not_use_preconditioner = 1).  Returns (u, iterations, [|r_k| per iteration], Au) -- Au = A u of the start (:163-174)."""
    u = np.array(u, dtype=np.float64, copy=True)
    Au = apply(u)                                    # :163-174
    r = (-1.0) * Au + rhs                            # :177 (axpyeqz(-1, Au, rhs, r))
    r0 = float(np.dot(r, r))                         # :180-190
    tol = atol + rtol * math.sqrt(r0)                # :192
    d = q = None
    rho = 0.0
    hist = []
    count = 0
    for k in range(imax):                            # :204
        v = pc(r) if pc is not None else r.copy()    # :206-216
        w = apply(v)                                 # :219-233
        alpha_k = float(np.dot(v, r))                # :236
        beta_k = float(np.dot(v, w))                 # :238
        if k > 0:
            gamma_k = float(np.dot(v, q))            # :241
            rr = float(np.dot(r, r))                 # :242
            c = -gamma_k / rho
            d = c * d + v                            # :262
            q = c * q + w                            # :264
            rho = beta_k - (gamma_k * gamma_k) / rho # :266
        else:
            rr = None
            rho = beta_k                             # :269
            d = v.copy()                             # :272
            q = w.copy()                             # :275
        u = (alpha_k / rho) * d + u                  # :279
        r = (-alpha_k / rho) * q + r                 # :281
        rk = math.sqrt(rr) if k > 0 else math.sqrt(r0)
        hist.append(rk)
        count = k + 1
        if k > 0 and rk <= tol:                      # :283-285
            break
    return u, count, hist, Au


def cg_allreduce_calls(iterations):
    """sc_allreduce calls of d4est_solver_cg_solve: one for delta_0, two per iteration (:139, :165, :179)"""
    return 1 + 2 * iterations


def fcg_allreduce_calls(iterations):
    """(calls, scalars) of d4est_solver_fcg_solve: one call for |r_0|^2, one per iteration with 2 scalars at k = 0, else 4 (:182, :245)"""
    return 1 + iterations, 1 + sum(2 if k == 0 else 4 for k in range(iterations))
