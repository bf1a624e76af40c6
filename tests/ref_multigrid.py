"""A restatement in numpy of the reference's hp-multigrid V-cycle, its solve loop, its Chebyshev smoother driver and its two bottom
solvers: the yardstick of the device multigrid (tests/test_vcycle_gpu.py), pinned on dense matrices by tests/test_ref_multigrid.py.

Levels as in the reference: 0 = bottom (coarsest) ... n_levels - 1 = top (finest).  The hierarchy is a set of per-level callables:

    apply(l, u)                                  -> A_l u
    cheby_iterate(l, u, rhs, iters, lmin, lmax)  -> (u_new, r) with r = rhs - A_l u_new
                                                    (d4est_solver_multigrid_smoother_cheby_iterate_aux, compute_residual_at_end = 1)
    cg_eigs(l, u, rhs, imax, use_new)            -> (bound, u_advanced)        (cg_eigs, src/Solver/d4est_solver_cg_eigs.c:116-275)
    prolong(l, x)                                -> P x, level l -> l + 1
    restrict(l, x)                               -> P^T x, level l + 1 -> l

File names below: mg = src/Solver/d4est_solver_multigrid.c, sm = src/Solver/d4est_solver_multigrid_smoother_cheby.c,
bcg = src/Solver/d4est_solver_multigrid_bottom_solver_cg.c, bch = src/Solver/d4est_solver_multigrid_bottom_solver_cheby.c,
pc = src/Solver/d4est_krylov_pc_multigrid.c.
"""
import math

import numpy as np

from tests import ref_solvers


class Hierarchy:
    def __init__(self, nodes, apply, cheby_iterate, cg_eigs, prolong, restrict):
        self.nodes = list(nodes)          # local_nodes per level, level 0 first
        self.n_levels = len(self.nodes)
        self.apply, self.cheby_iterate, self.cg_eigs, self.prolong, self.restrict = apply, cheby_iterate, cg_eigs, prolong, restrict


class ChebySmoother:
    """d4est_solver_multigrid_smoother_cheby with the [mg_smoother_cheby] keys"""

    def __init__(self, n_levels, cheby_imax, cheby_eigs_cg_imax, cheby_eigs_lmax_lmin_ratio, cheby_eigs_max_multiplier=1.0,
                 cheby_eigs_reuse_fromdownvcycle=0, cheby_eigs_reuse_fromlastvcycle=0, cheby_use_new_cg_eigs=0,
                 cheby_use_zero_guess_for_eigs=0):
        self.imax, self.eigs_imax = cheby_imax, cheby_eigs_cg_imax
        self.ratio, self.multiplier = cheby_eigs_lmax_lmin_ratio, cheby_eigs_max_multiplier
        self.fromdown, self.fromlast = cheby_eigs_reuse_fromdownvcycle, cheby_eigs_reuse_fromlastvcycle
        self.use_new, self.zero_guess = cheby_use_new_cg_eigs, cheby_use_zero_guess_for_eigs
        self.eigs = [-1.0] * n_levels      # sm :391 allocates the array without a value; -1 marks "none yet" here
        self.eigs_compute = 1
        self.eigs_calls = [0] * n_levels   # bookkeeping of the restatement: cg_eigs calls per level

    def pre_v(self, vcycle):               # sm :234-244
        self.eigs_compute = 0 if (self.fromlast == 1 and vcycle != 0) else 1

    def upv_pre_smooth(self, vcycle):      # sm :246-257
        self.eigs_compute = 0 if (self.fromdown == 1 or (self.fromlast == 1 and vcycle != 0)) else 1

    def smooth(self, h, level, u, rhs):
        """returns (u, r): sm :264-376"""
        if self.eigs_compute:                                                           # sm :280
            start = np.zeros_like(u) if self.zero_guess else u                          # sm :282-286
            bound, advanced = h.cg_eigs(level, start, rhs, self.eigs_imax, self.use_new)   # sm :288-303
            self.eigs_calls[level] += 1
            if not self.zero_guess:
                u = advanced                                                            # cg_eigs works on vecs->u itself
            self.eigs[level] = bound                                                    # sm :302
            self.eigs[level] *= self.multiplier                                         # sm :310
        if self.zero_guess == 1 and self.fromdown != 1:                                 # sm :313-318
            raise RuntimeError("If you set cheby_use_zero_guess_for_eigs == 1, please set cheby_eigs_reuse_fromdownvcycle = 1")
        # sm :320-353: a cg_eigs from a zero vector whose bound is discarded; it changes no vector the cycle reads (omitted)
        lmin = self.eigs[level] / self.ratio                                            # sm :356
        lmax = self.eigs[level]                                                         # sm :357
        return h.cheby_iterate(level, u, rhs, self.imax, lmin, lmax)                    # sm :364-375


class BottomCG:
    """d4est_solver_multigrid_bottom_solver_cg (bcg :48-198): the recurrence of d4est_solver_cg_solve"""

    def __init__(self, bottom_imax, bottom_atol, bottom_rtol):
        self.imax, self.atol, self.rtol = bottom_imax, bottom_atol, bottom_rtol
        self.iterations = 0
        self.eig = None

    def solve(self, h, u, rhs):
        u, it, _, _ = ref_solvers.cg_solve(lambda x: h.apply(0, x), u, rhs, self.imax, self.atol, self.rtol)   # bcg :91-194
        self.iterations = it
        return u


class BottomCheby:
    """d4est_solver_multigrid_bottom_solver_cheby (bch :59-113)"""

    def __init__(self, cheby_imax, cheby_eigs_cg_imax, lmax_lmin_ratio, max_multiplier=1.0, use_new_cg_eigs=0):
        self.imax, self.eigs_imax, self.ratio, self.multiplier, self.use_new = cheby_imax, cheby_eigs_cg_imax, lmax_lmin_ratio, \
            max_multiplier, use_new_cg_eigs
        self.iterations = 0
        self.eig = None

    def solve(self, h, u, rhs):
        eig, u = h.cg_eigs(0, u, rhs, self.eigs_imax, self.use_new)      # bch :73-88 (from the current iterate, every call)
        eig *= self.multiplier                                            # bch :90
        self.eig = eig
        u, _ = h.cheby_iterate(0, u, rhs, self.imax, eig / self.ratio, eig)   # bch :92-112
        self.iterations = self.imax
        return u


def vcycle(h, smoother, bottom, u, rhs, vcycle_index, trace=None):
    """d4est_solver_multigrid_vcycle (mg :751-1348).  Returns (u, vcycle_r2_local).  trace (optional list) receives
    (what, level, vector length) for every level vector the cycle touches: the arena indexing pinned by tests/test_ref_multigrid.py."""
    top = h.n_levels - 1
    u = np.array(u, dtype=np.float64, copy=True)
    err = [None] * h.n_levels
    res = [None] * h.n_levels
    rres = [None] * h.n_levels

    def note(what, level, v):
        if trace is not None:
            trace.append((what, level, len(v)))
        assert len(v) == h.nodes[level], (what, level, len(v), h.nodes[level])

    smoother.pre_v(vcycle_index)                                          # mg :843
    for level in range(top, 0, -1):                                       # mg :847
        if level != top:
            err[level] = np.zeros(h.nodes[level])                         # mg :859
        if level == top:                                                  # mg :861-866
            note("smooth", level, u)
            u, rres[level] = smoother.smooth(h, level, u, rhs)            # mg :905-912
        else:                                                             # mg :867-872
            note("smooth", level, err[level])
            err[level], rres[level] = smoother.smooth(h, level, err[level], res[level])
        note("restrict_in", level, rres[level])
        rres[level - 1] = h.restrict(level - 1, rres[level])              # mg :1054-1077
        note("restrict_out", level - 1, rres[level - 1])
        res[level - 1] = rres[level - 1].copy()                           # mg :1090-1095
    err[0] = np.zeros(h.nodes[0])                                         # mg :1115
    note("bottom", 0, res[0])
    err[0] = bottom.solve(h, err[0], res[0])                              # mg :1118-1148
    for level in range(0, top):                                           # mg :1168
        rres[level] = err[level].copy()                                   # mg :1182-1184
        note("prolong_in", level, rres[level])
        rres[level + 1] = h.prolong(level, rres[level])                   # mg :1199-1205
        note("prolong_out", level + 1, rres[level + 1])
        smoother_u = u if level + 1 == top else err[level + 1]            # mg :1231-1242
        smoother_u = smoother_u + 1.0 * rres[level + 1]                   # mg :1250 (axpy 1.0)
        smoother.upv_pre_smooth(vcycle_index)                             # mg :1261
        if level + 1 == top:
            note("smooth", level + 1, smoother_u)
            u, rres[level + 1] = smoother.smooth(h, level + 1, smoother_u, rhs)                       # mg :1263-1270
        else:
            note("smooth", level + 1, smoother_u)
            err[level + 1], rres[level + 1] = smoother.smooth(h, level + 1, smoother_u, res[level + 1])
    r2 = float(np.dot(rres[top], rres[top]))                              # mg :1330-1332
    return u, r2


def solve(h, smoother, bottom, u, rhs, vcycle_imax, vcycle_atol, vcycle_rtol):
    """d4est_solver_multigrid_solve (mg :1420-1506), one rank.  Returns (u, cycles, [r2_0, r2 after each cycle])."""
    if h.n_levels < 2:                                                    # mg :1435-1438
        raise RuntimeError("The code sees less than two multigrid levels, cannot run multigrid")
    u = np.array(u, dtype=np.float64, copy=True)
    top = h.n_levels - 1
    Au = h.apply(top, u)                                                  # mg :1373-1384
    r = (-1.0) * Au + rhs                                                 # mg :1387
    r2 = float(np.dot(r, r))                                              # mg :1388-1402
    r2_last = r2                                                          # mg :1455
    n = 0                                                                 # mg :1457
    stoptol = vcycle_rtol * vcycle_rtol * r2 + vcycle_atol * vcycle_atol  # mg :1458-1459
    hist = [r2]
    while n < vcycle_imax and r2 > stoptol:                               # mg :1467-1472
        u, r2 = vcycle(h, smoother, bottom, u, rhs, n)                    # mg :1475-1482
        n += 1                                                            # mg :1484
        hist.append(r2)
        if math.sqrt(r2 / r2_last) >= .99:                                # mg :1488-1491
            break
        r2_last = r2                                                      # mg :1493
    return u, n, hist


def pc_apply(h, smoother, bottom, r, vcycle_imax, vcycle_atol, vcycle_rtol):
    """d4est_krylov_pc_multigrid_apply (pc :40-77): z = 0, then the solve with rhs = r"""
    z = np.zeros_like(r)                                                  # pc :50
    z, _, _ = solve(h, smoother, bottom, z, r, vcycle_imax, vcycle_atol, vcycle_rtol)   # pc :68-74
    return z


# ---- numpy forms of the two smoother kernels around any apply: dense matrices in the pins, a perturbed operator in the GPU tests -----

def np_cheby_iterate(apply, u, rhs, iters, lmin, lmax):
    """d4est_solver_multigrid_smoother_cheby_iterate_aux (sm :81-176) with compute_residual_at_end = 1; apply: u -> A u"""
    d = (lmax + lmin) * .5                                                # sm :106
    c = (lmax - lmin) * .5                                                # sm :107
    u = np.array(u, dtype=np.float64, copy=True)
    p = np.zeros_like(u)                                                  # sm :118
    alpha = 0.0
    for i in range(iters):                                                # sm :119
        r = rhs + (-1.0) * apply(u)                                       # sm :122-136
        if i == 0:
            alpha = 1. / d                                                # sm :143
        elif i == 1:
            alpha = 2. * d / (2 * d * d - c * c)                          # sm :145
        else:
            alpha = 1. / (d - (alpha * c * c / 4.))                       # sm :147
        beta = alpha * d - 1.                                             # sm :149
        r = alpha * r                                                     # sm :151
        p = r + beta * p                                                  # sm :152
        u = u + 1. * p                                                    # sm :153
    r = rhs + (-1.0) * apply(u)                                           # sm :157-172
    return u, r


def np_cg_eigs(apply, u, rhs, imax, use_new):
    """cg_eigs (src/Solver/d4est_solver_cg_eigs.c:116-275) with tridiag_gershgorin (:9-37) / _new (:41-65).  Returns (bound, u)."""
    n = len(u)
    u = np.array(u, dtype=np.float64, copy=True)
    r = rhs + (-1.0) * apply(u)                                           # :160-174
    d = r.copy()                                                          # :175
    delta_new = float(np.dot(r, r))                                       # :176-191
    alpha = beta = -1.                                                    # :139-140
    bound = None
    for i in range(imax):                                                 # :199
        Ad = apply(d)                                                     # :201-212
        alpha_old = alpha                                                 # :227
        alpha = delta_new / float(np.dot(d, Ad))                          # :214-228
        u = u + alpha * d                                                 # :230
        r = r + (-alpha) * Ad                                             # :231
        delta_old = delta_new                                             # :233
        delta_new = float(np.dot(r, r))                                   # :234-245
        beta_old = beta                                                   # :247
        beta = delta_new / delta_old                                      # :248
        d = r + beta * d                                                  # :249
        a0, b0, a1, b1 = alpha_old, beta_old, alpha, beta
        if not use_new:                                                   # :9-37
            if i != 0 and i < n - 1:
                diag, off = 1. / a1 + b0 / a0, abs(math.sqrt(b1) / a1) + abs(math.sqrt(b0) / a0)
            elif i == 0:
                diag, off = 1. / a1, math.sqrt(b1) / a1
            else:
                diag, off = 1. / a1 + b0 / a0, abs(math.sqrt(b0) / a0)
        else:                                                             # :41-65
            if i != 0:
                diag, off = 1. / a1 + b0 / a0, abs(math.sqrt(b0) / a0)
            else:
                diag, off = 1. / a1, math.sqrt(b1) / a1
        temp_max = diag + off
        bound = max(bound, temp_max) if i > 0 else temp_max               # :258-263
    return bound, u


def dense_cheby_iterate(A, u, rhs, iters, lmin, lmax):
    return np_cheby_iterate(lambda x: A @ x, u, rhs, iters, lmin, lmax)


def dense_cg_eigs(A, u, rhs, imax, use_new):
    return np_cg_eigs(lambda x: A @ x, u, rhs, imax, use_new)


def dense_hierarchy(As, Ps):
    """levels of dense matrices As[0 .. L-1] (level 0 = bottom) and dense prolongations Ps[l]: level l -> l + 1"""
    return Hierarchy([A.shape[0] for A in As],
                     apply=lambda l, x: As[l] @ x,
                     cheby_iterate=lambda l, u, rhs, it, lmin, lmax: dense_cheby_iterate(As[l], u, rhs, it, lmin, lmax),
                     cg_eigs=lambda l, u, rhs, imax, use_new: dense_cg_eigs(As[l], u, rhs, imax, use_new),
                     prolong=lambda l, x: Ps[l] @ x,
                     restrict=lambda l, x: Ps[l].T @ x)


def expected_eigs_calls(n_levels, fromdown, fromlast, vcycle_index):
    """cg_eigs calls per level in one V-cycle, from sm :234-257: PRE_V leaves eigs_compute = 1 unless (fromlast and vcycle != 0), so the
    down leg computes on levels top ... 1; every UPV_PRE_SMOOTH leaves 1 unless fromdown or (fromlast and vcycle != 0), so the up leg
    computes again on levels 1 ... top.  Level 0 is the bottom solver's."""
    down = 0 if (fromlast == 1 and vcycle_index != 0) else 1
    up = 0 if (fromdown == 1 or (fromlast == 1 and vcycle_index != 0)) else 1
    return [0] + [down + up] * (n_levels - 1)
