"""Numpy restatements of the pieces of the reference that join the Schwarz smoother to the multigrid and to the Krylov solvers: the
yardstick of tests/test_vcycle_schwarz_gpu.py and tests/test_pc_gpu.py, pinned on dense matrices by tests/test_ref_schwarz_smoother.py.

File names below: ss = src/Solver/d4est_solver_multigrid_smoother_schwarz.c, rs = src/Solver/d4est_solver_multigrid_bottom_solver_reuse_smoother.c,
pch = src/Solver/d4est_krylov_pc_cheby.c, psz = src/Solver/d4est_krylov_pc_schwarz.c.

The smoother and the bottom solver have the interface tests/ref_multigrid.py's vcycle / solve / pc_apply expect.  Callables:

    schwarz_iterate(l, u, r)                 -> u + the Schwarz correction of the residual r on level l (d4est_solver_schwarz_iterate)
    apply(u)                                 -> A u
    cg_eigs(u, rhs, imax, use_new)           -> (bound, u_advanced)
    cheby_iterate(u, rhs, iters, lmin, lmax) -> u_new                   (iterate_aux with compute_residual_at_end = 0)
"""
import numpy as np


class SchwarzSmoother:
    """d4est_solver_multigrid_smoother_schwarz (ss :89-204) with [mg_smoother_schwarz] smoother_iterations"""

    def __init__(self, iterations, schwarz_iterate):
        self.iterations = iterations
        self.schwarz_iterate = schwarz_iterate
        self.iterate_calls = 0               # bookkeeping of the restatement
        self.eigs = None                     # no eigenvalue state

    def pre_v(self, vcycle):                 # ss :296-365: the update callback keeps debug counters and builds Schwarz data only
        pass

    def upv_pre_smooth(self, vcycle):
        pass

    def smooth(self, h, level, u, rhs):
        """returns (u, r)"""
        for _ in range(self.iterations):                                  # ss :110
            r = h.apply(level, u)                                         # ss :112-126 (vecs->Au = r)
            r = rhs + (-1.) * r                                           # ss :128 (xpby(rhs, -1., r))
            u = self.schwarz_iterate(level, u, r)                         # ss :136-146
            self.iterate_calls += 1
        r = h.apply(level, u)                                             # ss :154-168
        r = rhs + (-1.) * r                                               # ss :196
        return u, r


class BottomReuseSmoother:
    """d4est_solver_multigrid_bottom_solver_reuse_smoother (rs :20-39): the smoother on level 0"""

    def __init__(self, smoother):
        self.smoother = smoother             # rs :28-29 (mg_data->smoother)
        self.iterations = 0                  # the smoother reports no count
        self.eig = None

    def solve(self, h, u, rhs):
        u, _ = self.smoother.smooth(h, 0, u, rhs)                         # rs :30-37
        return u


class PcChebyState:
    """what d4est_krylov_pc_cheby_data_t carries from apply to apply"""

    def __init__(self):
        self.eig = -1.0                      # pch :196
        self.runs = 0                        # cg_eigs calls (bookkeeping of the restatement)


def pc_cheby_apply(st, cg_eigs, cheby_iterate, r, cheby_imax, cheby_eigs_cg_imax, cheby_eigs_lmax_lmin_ratio, cheby_eigs_max_multiplier,
                   cheby_reuse_eig, cheby_use_new_cg_eigs, cheby_use_zero_guess_for_eigs):
    """d4est_krylov_pc_cheby_apply (pch :92-171); returns z"""
    z = np.zeros_like(r)                                                  # pch :104
    if (not cheby_reuse_eig) or st.eig == -1:                             # pch :114-115
        start = np.zeros_like(r) if cheby_use_zero_guess_for_eigs else z  # pch :119-122
        bound, advanced = cg_eigs(start, r, cheby_eigs_cg_imax, cheby_use_new_cg_eigs)   # pch :123-138
        st.runs += 1
        if not cheby_use_zero_guess_for_eigs:
            z = advanced                                                  # cg_eigs works on vecs->u = yp itself
        st.eig = bound
        st.eig *= cheby_eigs_max_multiplier                               # pch :145
    return cheby_iterate(z, r, cheby_imax, st.eig / cheby_eigs_lmax_lmin_ratio, st.eig)   # pch :149-167


def pc_schwarz_apply(apply, schwarz_iterate, r, iterations):
    """d4est_krylov_pc_schwarz_apply (psz :59-116); schwarz_iterate(u, residual) -> u; returns z"""
    z = np.zeros_like(r)                                                  # psz :69
    for _ in range(iterations):                                           # psz :81
        Au = apply(z)                                                     # psz :83-94
        residual = (-1.) * Au + r                                         # psz :97 (axpyeqz(-1., Au, rhs, residual))
        z = schwarz_iterate(z, residual)                                  # psz :99-110
    return z


# ---- a dense additive Schwarz iterate for the pins: exact subdomain solves on index sets with weights --------------------------------

def dense_schwarz_iterate(A, subdomains, weights=None):
    """u + sum_s W_s R_s^T (R_s A R_s^T)^-1 R_s r over index arrays `subdomains`, added in ascending subdomain order; weights[s]: one
    weight per index of subdomain s (default 1)"""
    def iterate(u, r):
        u = np.array(u, dtype=np.float64, copy=True)
        for s, idx in enumerate(subdomains):
            du = np.linalg.solve(A[np.ix_(idx, idx)], r[idx])
            u[idx] += du if weights is None else weights[s] * du
        return u
    return iterate
