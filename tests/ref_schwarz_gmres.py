"""Numpy restatement of the reference's restarted GMRES subdomain solver for ONE subdomain:
d4est_solver_schwarz_subdomain_solver_gmres, src/Solver/d4est_solver_schwarz_subdomain_solver_gmres.c:243-422 (line numbers below are
that file's).  The yardstick of tests/test_schwarz_gmres_gpu.py, pinned on dense matrices by tests/test_ref_schwarz_gmres.py.

    gmres(apply, rhs, mr, itr_max, tol_abs, tol_rel, x0=None) -> GmresResult

apply(x) -> A x on a restricted vector.  Every scalar operation is rounded on its own, as the C source reads without contraction.
"""
import numpy as np

DELTA = 1.0e-03                                                           # :213


class GmresResult:
    """x, itr_used (inner steps made), rho (:441-442); margins: for each step at which the stop test rho <= rho_tol && rho <= tol_abs
    (:391) was evaluated, |rho - t| / t with t = min(rho_tol, tol_abs), the threshold that decides the AND; cycles: per restart cycle
    (x at its end, rho at its end, columns used)"""

    def __init__(self, x, itr_used, rho, margins, cycles):
        self.x, self.itr_used, self.rho, self.margins, self.cycles = x, itr_used, rho, margins, cycles

    def min_margin(self):
        return min(self.margins) if self.margins else np.inf

    def __iter__(self):                      # x, itr_used, rho = gmres(...)
        return iter((self.x, self.itr_used, self.rho))


def _dot(a, b, reverse):
    """d4est_linalg_vec_dot: a plain running sum in index order (reverse: the same sum taken from the other end, for the self-distance
    the GPU test's bound may fall back on)"""
    p = a * b
    if reverse:
        p = p[::-1]
    return float(np.cumsum(p)[-1]) if p.size else 0.0     # cumsum accumulates in index order: the C loop's running sum


def _mult_givens(c, s, k, g):                                             # :150-163
    g1 = c * g[k] - s * g[k + 1]
    g2 = s * g[k] + c * g[k + 1]
    g[k] = g1
    g[k + 1] = g2


def gmres(apply, rhs, mr, itr_max, tol_abs, tol_rel, x0=None, reverse_dots=False):
    rhs = np.asarray(rhs, dtype=np.float64)
    n = rhs.size
    if n < mr:
        raise ValueError("nodes < mr in schwarz_subdomain_solver_gmres")  # :203-205
    x = np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64, copy=True)
    dot = lambda a, b: _dot(a, b, reverse_dots)
    c = np.zeros(mr)
    s = np.zeros(mr)
    g = np.zeros(mr + 1)
    h = np.zeros((mr + 1, mr))
    v = np.zeros((mr + 1, n))
    y = np.zeros(mr + 1)
    itr_used = 0
    rho = rho_tol = 0.0
    margins, cycles = [], []
    stop = lambda: rho <= rho_tol and rho <= tol_abs
    for itr in range(itr_max):                                            # :243
        r = rhs - apply(x)                                                # :246-266
        rho = float(np.sqrt(dot(r, r)))                                   # :268
        if itr == 0:
            rho_tol = rho * tol_rel                                       # :274-277
        with np.errstate(invalid="ignore", divide="ignore"):
            v[0] = r / rho                                                # :279-282 (0 / 0 for a zero residual: the reference's NaN)
        g[:] = 0.0
        g[0] = rho                                                        # :284-288
        h[:] = 0.0                                                        # :290-296
        k_copy = 0
        for k in range(mr):                                               # :298
            k_copy = k
            v[k + 1] = apply(v[k])                                        # :302-317
            av = float(np.sqrt(dot(v[k + 1], v[k + 1])))                  # :321
            for j in range(k + 1):                                        # :323-331
                h[j, k] = dot(v[k + 1], v[j])
                v[k + 1] = v[k + 1] - h[j, k] * v[j]
            h[k + 1, k] = np.sqrt(dot(v[k + 1], v[k + 1]))                # :334
            if (av + DELTA * h[k + 1, k]) == av:                          # :336-350
                for j in range(k + 1):
                    htmp = dot(v[k + 1], v[j])
                    h[j, k] = h[j, k] + htmp
                    v[k + 1] = v[k + 1] - htmp * v[j]
                h[k + 1, k] = np.sqrt(dot(v[k + 1], v[k + 1]))
            if h[k + 1, k] != 0.0:                                        # :352-358
                v[k + 1] = v[k + 1] / h[k + 1, k]
            if 0 < k:                                                     # :360-374
                y[:k + 2] = h[:k + 2, k]
                for j in range(k):
                    _mult_givens(c[j], s[j], j, y)
                h[:k + 2, k] = y[:k + 2]
            mu = np.sqrt(h[k, k] * h[k, k] + h[k + 1, k] * h[k + 1, k])   # :376
            c[k] = h[k, k] / mu                                           # :377
            s[k] = -h[k + 1, k] / mu                                      # :378
            h[k, k] = c[k] * h[k, k] - s[k] * h[k + 1, k]                 # :379
            h[k + 1, k] = 0.0                                             # :380
            _mult_givens(c[k], s[k], k, g)                                # :381
            rho = float(abs(g[k + 1]))                                    # :383
            itr_used += 1                                                 # :385
            t = min(rho_tol, tol_abs)
            margins.append(abs(rho - t) / t if t > 0 else (0.0 if rho == 0 else np.inf))
            if stop():                                                    # :391
                break
        k = k_copy                                                        # :397
        y[k] = g[k] / h[k, k]                                             # :399
        for i in range(k - 1, -1, -1):                                    # :400-408
            y[i] = g[i]
            for j in range(i + 1, k + 1):
                y[i] = y[i] - h[i, j] * y[j]
            y[i] = y[i] / h[i, i]
        for j in range(k + 1):                                            # :410-416 (per node: j ascending)
            x = x + v[j] * y[j]
        cycles.append((x.copy(), rho, k + 1))
        if stop():                                                        # :418-421
            break
    return GmresResult(x, itr_used, rho, margins, cycles)
