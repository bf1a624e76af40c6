"""Pins of tests/ref_schwarz_smoother.py on small dense SPD matrices (no GPU), and the C-ABI side of the same feature: the new symbols
are exported and bound, and the header still compiles as C99."""
import os
import subprocess

import numpy as np

from tests import ref_multigrid as RM
from tests import ref_schwarz_smoother as RZ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _spd(n, seed, shift=None):
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, n))
    return B @ B.T + (n if shift is None else shift) * np.eye(n)


def _block_diag(blocks):
    n = sum(b.shape[0] for b in blocks)
    A = np.zeros((n, n))
    o = 0
    for b in blocks:
        A[o:o + b.shape[0], o:o + b.shape[0]] = b
        o += b.shape[0]
    return A


def test_exact_nonoverlapping_subdomains_solve_a_block_diagonal_system():
    sizes = [3, 5, 4]
    A = _block_diag([_spd(n, 10 + n) for n in sizes])
    offs = np.concatenate([[0], np.cumsum(sizes)])
    subs = [np.arange(offs[k], offs[k + 1]) for k in range(len(sizes))]
    it = RZ.dense_schwarz_iterate(A, subs)
    rng = np.random.default_rng(1)
    x, u0 = rng.standard_normal(A.shape[0]), rng.standard_normal(A.shape[0])
    rhs = A @ x
    h = RM.Hierarchy([A.shape[0]], apply=lambda l, v: A @ v, cheby_iterate=None, cg_eigs=None, prolong=None, restrict=None)
    sm = RZ.SchwarzSmoother(1, lambda l, u, r: it(u, r))
    u, r = sm.smooth(h, 0, u0, rhs)
    assert sm.iterate_calls == 1
    assert np.abs(u - x).max() <= 1e-12 * np.abs(x).max()
    assert np.abs(r).max() <= 1e-12 * np.abs(rhs).max()
    # the exit residual is rhs - A u of the iterate returned, whatever the iteration count
    sm3 = RZ.SchwarzSmoother(3, lambda l, u, r: u + 0.01 * r)
    u3, r3 = sm3.smooth(h, 0, u0, rhs)
    assert sm3.iterate_calls == 3 and np.array_equal(r3, rhs + (-1.) * (A @ u3))
    # zero iterations: u untouched, r = rhs - A u
    u_, r_ = RZ.SchwarzSmoother(0, None).smooth(h, 0, u0, rhs)
    assert np.array_equal(u_, u0) and np.array_equal(r_, rhs + (-1.) * (A @ u0))


def test_overlapping_weighted_subdomains_contract():
    n = 12
    A = _spd(n, 3, shift=2.0 * n)
    subs = [np.arange(0, 7), np.arange(5, 12)]
    w = [np.array([1, 1, 1, 1, 1, .5, .5]), np.array([.5, .5, 1, 1, 1, 1, 1])]     # a partition of unity on the overlap
    it = RZ.dense_schwarz_iterate(A, subs, w)
    rng = np.random.default_rng(2)
    x = rng.standard_normal(n)
    rhs = A @ x
    h = RM.Hierarchy([n], apply=lambda l, v: A @ v, cheby_iterate=None, cg_eigs=None, prolong=None, restrict=None)
    sm = RZ.SchwarzSmoother(1, lambda l, u, r: it(u, r))
    u = np.zeros(n)
    norms = [np.linalg.norm(rhs)]
    for _ in range(4):
        u, r = sm.smooth(h, 0, u, rhs)
        norms.append(np.linalg.norm(r))
    assert all(b < a for a, b in zip(norms[:-1], norms[1:])), norms


def test_pc_cheby_reuse_eig_counts_cg_eigs_runs():
    n = 10
    A = _spd(n, 5)
    calls = []

    def eigs(u, rhs, imax, use_new):
        calls.append((u.copy(), imax, use_new))
        return RM.dense_cg_eigs(A, u, rhs, imax, use_new)

    cheby = lambda u, rhs, it, lmin, lmax: RM.dense_cheby_iterate(A, u, rhs, it, lmin, lmax)[0]
    rng = np.random.default_rng(4)
    rs = [rng.standard_normal(n) for _ in range(3)]
    for reuse, want in ((1, 1), (0, 3)):
        for zero in (0, 1):
            del calls[:]
            st = RZ.PcChebyState()
            eig_seen = []
            for r in rs:
                z = RZ.pc_cheby_apply(st, eigs, cheby, r, 4, 3, 30.0, 1.1, reuse, 1, zero)
                eig_seen.append(st.eig)
                assert np.isfinite(z).all() and np.abs(z).max() > 0
            assert len(calls) == want == st.runs
            assert all(np.array_equal(c[0], np.zeros(n)) and c[1:] == (3, 1) for c in calls)    # every run starts from a zero vector
            if reuse:
                assert eig_seen[0] == eig_seen[1] == eig_seen[2] > 0
    # the first apply: the bound times the multiplier; without the zero guess cg_eigs' iterate is the Chebyshev start
    st = RZ.PcChebyState()
    z = RZ.pc_cheby_apply(st, eigs, cheby, rs[0], 2, 3, 30.0, 1.1, 1, 1, 0)
    bound, adv = RM.dense_cg_eigs(A, np.zeros(n), rs[0], 3, 1)
    assert st.eig == bound * 1.1
    assert np.array_equal(z, RM.dense_cheby_iterate(A, adv, rs[0], 2, st.eig / 30.0, st.eig)[0])
    st = RZ.PcChebyState()
    z0 = RZ.pc_cheby_apply(st, eigs, cheby, rs[0], 2, 3, 30.0, 1.1, 1, 1, 1)
    assert np.array_equal(z0, RM.dense_cheby_iterate(A, np.zeros(n), rs[0], 2, st.eig / 30.0, st.eig)[0])


def test_pc_schwarz_is_iterations_of_residual_and_iterate():
    n = 9
    A = _spd(n, 6)
    subs = [np.arange(0, 5), np.arange(4, 9)]
    it = RZ.dense_schwarz_iterate(A, subs, [np.full(5, .7), np.full(5, .7)])
    r = np.random.default_rng(7).standard_normal(n)
    assert np.array_equal(RZ.pc_schwarz_apply(lambda v: A @ v, it, r, 0), np.zeros(n))
    z1 = RZ.pc_schwarz_apply(lambda v: A @ v, it, r, 1)
    assert np.array_equal(z1, it(np.zeros(n), r))                         # the first pass: the residual is r itself
    z2 = RZ.pc_schwarz_apply(lambda v: A @ v, it, r, 2)
    assert np.array_equal(z2, it(z1, (-1.) * (A @ z1) + r))


def test_vcycle_runs_unchanged_with_the_schwarz_smoother_and_the_reuse_bottom_solver():
    rng = np.random.default_rng(8)
    sizes = [4, 8, 16]
    Ps = [np.kron(np.eye(sizes[l]), np.array([[1.0], [1.0]])) * (1.0 + 0.1 * rng.random((sizes[l + 1], sizes[l]))) for l in range(2)]
    A2 = _spd(16, 9)
    A1 = Ps[1].T @ A2 @ Ps[1]
    A0 = Ps[0].T @ A1 @ Ps[0]
    As = [A0, A1, A2]
    h = RM.dense_hierarchy(As, Ps)
    its = [RZ.dense_schwarz_iterate(A, [np.arange(0, A.shape[0] // 2 + 1), np.arange(A.shape[0] // 2 - 1, A.shape[0])],
                                    [np.full(A.shape[0] // 2 + 1, .6), np.full(A.shape[0] - A.shape[0] // 2 + 1, .6)]) for A in As]
    x = rng.standard_normal(16)
    rhs = A2 @ x
    for bottom_kind in ("cg", "reuse"):
        sm = RZ.SchwarzSmoother(2, lambda l, u, r: its[l](u, r))
        bs = RM.BottomCG(50, 0.0, 1e-14) if bottom_kind == "cg" else RZ.BottomReuseSmoother(sm)
        trace = []
        u, r2 = RM.vcycle(h, sm, bs, np.zeros(16), rhs, 0, trace)
        # down: smooth on 2 and 1; bottom; up: smooth on 1 and 2 -- two iterates per call, plus the bottom's two under reuse
        assert sm.iterate_calls == 2 * 4 + (2 if bottom_kind == "reuse" else 0)
        assert [t for t in trace if t[0] == "smooth"] == [("smooth", 2, 16), ("smooth", 1, 8), ("smooth", 1, 8), ("smooth", 2, 16)]
        res = rhs - A2 @ u
        assert abs(float(res @ res) - r2) <= 1e-10 * r2
        u_s, n, hist = RM.solve(h, sm, bs, np.zeros(16), rhs, 30, 0.0, 1e-8)
        assert n < 30 and hist[-1] <= 1e-16 * hist[0]
        assert np.abs(u_s - x).max() <= 1e-6 * np.abs(x).max()
        z = RM.pc_apply(h, sm, bs, rhs, 1, 0.0, 0.0)
        assert np.linalg.norm(rhs - A2 @ z) < np.linalg.norm(rhs)
    # the reuse bottom solver with the Chebyshev smoother: level 0 takes its bound like any other level
    sm = RM.ChebySmoother(3, 3, 4, 30.0, 1.1, 0, 0, 1, 0)
    u, r2 = RM.vcycle(h, sm, RZ.BottomReuseSmoother(sm), np.zeros(16), rhs, 0)
    assert sm.eigs_calls == [1, 2, 2] and sm.eigs[0] > 0 and np.isfinite(r2)


NEW_SYMBOLS = ["d4est_hip_multigrid_set_smoother_schwarz", "d4est_hip_multigrid_smooth_level", "d4est_hip_multigrid_set_bottom_solver_reuse_smoother",
               "d4est_hip_pc_cheby_create", "d4est_hip_pc_cheby_apply", "d4est_hip_pc_cheby_eig", "d4est_hip_pc_cheby_reset_eig",
               "d4est_hip_pc_cheby_destroy", "d4est_hip_pc_schwarz_create", "d4est_hip_pc_schwarz_apply", "d4est_hip_pc_schwarz_destroy"]


def test_new_symbols_are_exported_and_bound(hiplib):
    from disco4est_amd import capi
    import disco4est_amd
    for s in NEW_SYMBOLS:
        assert hasattr(hiplib, s), "libd4est_hip.so does not export %s" % s
        assert s in capi.SIGNATURES
    for name in ("PcCheby", "PcSchwarz"):
        assert hasattr(disco4est_amd, name)
    for name in ("set_smoother_schwarz", "set_bottom_solver_reuse_smoother", "smooth_level"):
        assert hasattr(capi.Multigrid, name)


def test_header_compiles_as_c99_with_the_new_entries(tmp_path):
    src = tmp_path / "pc_header.c"
    src.write_text('#include "d4est_hip.h"\n'
                   "int use(d4est_hip_multigrid_t* mg, d4est_hip_schwarz_t* const* sz, d4est_hip_plan_t* plan) {\n"
                   "  d4est_hip_pc_fn a = d4est_hip_pc_cheby_apply, b = d4est_hip_pc_schwarz_apply, c = d4est_hip_multigrid_pc_apply;\n"
                   "  d4est_hip_pc_cheby_t* pc = d4est_hip_pc_cheby_create(plan, 3, 5, 30.0, 1.1, 1, 1, 0);\n"
                   "  d4est_hip_multigrid_set_bottom_solver_reuse_smoother(mg);\n"
                   "  (void)a; (void)b; (void)c; (void)pc;\n"
                   "  return d4est_hip_multigrid_set_smoother_schwarz(mg, sz, 1, 12, 1e-15, 1e-4);\n"
                   "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "pc_header.o")])
