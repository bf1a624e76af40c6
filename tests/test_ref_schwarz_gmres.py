"""Pins tests/ref_schwarz_gmres.py (the numpy restatement of d4est_solver_schwarz_subdomain_solver_gmres.c:243-422) on dense
matrices, and holds the condition under which tests/test_schwarz_gmres_gpu.py may excuse marginal subdomains: with the reference alone
(the restatement on the oracle's subdomain operator), at most 10 % of the subdomains of each mesh have a stop test within 1e-6 of its
threshold."""
import numpy as np
import pytest

from tests import ref_schwarz_gmres as RG
from tests import schwarz_gmres_cases as C


def _matrix(n, seed):
    rng = np.random.default_rng(seed)
    return n * np.eye(n) + rng.standard_normal((n, n))          # non-symmetric, eigenvalues near n: well-conditioned


def test_dense_solve():
    n = 12
    A = _matrix(n, 1)
    b = np.random.default_rng(2).standard_normal(n)
    assert np.linalg.cond(A) < 10 and np.abs(A - A.T).max() > 0.1
    res = RG.gmres(lambda x: A @ x, b, n, 1, 1e-300, 1e-300)
    want = np.linalg.solve(A, b)
    assert res.itr_used == n
    assert np.linalg.norm(res.x - want) <= 1e-10 * np.linalg.norm(want)


def test_cycle_minimum():
    """after each restart cycle |b - A x| is the least-squares minimum over x_before + K_mr(A, r_before), and rho is that norm"""
    n, mr = 12, 4
    A = _matrix(n, 3)
    b = np.random.default_rng(4).standard_normal(n)
    res = RG.gmres(lambda x: A @ x, b, mr, 3, 1e-300, 1e-300)
    assert len(res.cycles) == 3 and res.itr_used == 3 * mr
    x_before = np.zeros(n)
    for x_after, rho, cols in res.cycles:
        assert cols == mr
        r0 = b - A @ x_before
        K = np.empty((n, mr))
        K[:, 0] = r0
        for j in range(1, mr):
            K[:, j] = A @ K[:, j - 1]
        K /= np.linalg.norm(K, axis=0)
        z = np.linalg.lstsq(A @ K, r0, rcond=None)[0]
        best = np.linalg.norm(r0 - A @ (K @ z))
        got = np.linalg.norm(b - A @ x_after)
        assert abs(got - best) <= 1e-10 * best
        assert abs(rho - got) <= 1e-10 * got
        x_before = x_after
    assert res.rho == res.cycles[-1][1]


def test_the_and_rule():
    """rho <= rho_tol holds steps before rho <= tol_abs: the loop stops at the later step (:391 -- both must hold)"""
    n = 12
    A = _matrix(n, 5)
    b = 1e3 * np.random.default_rng(6).standard_normal(n)
    trace = RG.gmres(lambda x: A @ x, b, n, 1, 1e-300, 1e-300)
    # rho after every step of the one cycle, from the margins' thresholds: run again step by step
    rhos = [RG.gmres(lambda x: A @ x, b, k, 1, 1e-300, 1e-300).rho for k in range(1, n + 1)]
    rho0 = np.linalg.norm(b)
    tol_rel = 1e-2
    first_rel = next(k for k, r in enumerate(rhos) if r <= rho0 * tol_rel)
    tol_abs = 0.5 * (rhos[first_rel + 2] + rhos[first_rel + 3])            # met three steps later
    first_abs = next(k for k, r in enumerate(rhos) if r <= tol_abs)
    assert first_abs == first_rel + 3 and first_abs < n - 1
    res = RG.gmres(lambda x: A @ x, b, n, 1, tol_abs, tol_rel)
    assert res.itr_used == first_abs + 1                                   # steps are counted from 1
    assert res.rho == rhos[first_abs] and res.rho <= tol_abs and res.rho <= rho0 * tol_rel
    assert len(res.margins) == res.itr_used and trace.itr_used == n
    # the other way round (tol_abs met first) stops at the later step, too
    res2 = RG.gmres(lambda x: A @ x, b, n, 1, 1e300, tol_rel)
    assert res2.itr_used == first_rel + 1


def test_zero_residual_is_the_references_nan():
    """the reference divides by rho unguarded (:281): the restatement keeps that, the device form documents its deviation"""
    res = RG.gmres(lambda x: 2.0 * x, np.zeros(5), 2, 1, 1e-6, 1e-6)
    assert np.isnan(res.x).all()


def _restricted_rhs(oracle, m, md, r, s):
    elem, faces, _ = md.subdomain(s)
    return np.concatenate([oracle.schwarz_apply_restrictor(r[m.nodal_stride[e]:m.nodal_stride[e] + (m.deg[e] + 1) ** 3], f, int(m.deg[e]),
                                                           md.num_nodes_overlap) for e, f in zip(elem, faces)])


@pytest.mark.parametrize("name", C.NAMES)
def test_marginal_subdomain_cap(oracle, name):
    """the convergent options of the GPU test's case 2 on the oracle's subdomain operator: subdomains with any margin below 1e-6 are at
    most 10 % of all -- the condition that lets the GPU test excuse them"""
    from disco4est_amd.schwarz import SchwarzMetadata
    m, mp, J, rst, sides, rs = C.build(name)
    md = SchwarzMetadata(m, sides, rs)
    oracle.set_operator(m, J, rst, sides, 10.0, 0, threads=1)
    hanging = "side_hang" in sides and np.any(np.asarray(sides["side_hang"]) != 0)
    if hanging:
        oracle.set_hanging(sides)
    try:
        r = C.residual(m)
        o = C.CONVERGENT
        results = []
        for s in range(md.num_subdomains):
            elem, faces, _ = md.subdomain(s)
            apply = lambda x, elem=elem, faces=faces: oracle.schwarz_apply_over_subdomain(elem, faces, rs, x)
            results.append(RG.gmres(apply, _restricted_rhs(oracle, m, md, r, s), o["mr"], o["cycles"], o["atol"], o["rtol"]))
    finally:
        if hanging:
            oracle.set_hanging(None)
    marginal = C.excused(results)
    its = np.array([x.itr_used for x in results])
    print("%s: %d subdomains, inner steps %d .. %d, smallest margin %.3e, marginal %s"
          % (name, md.num_subdomains, its.min(), its.max(), min(x.min_margin() for x in results), marginal))
    assert len(marginal) <= C.EXCUSED_SHARE * md.num_subdomains
    assert all(np.isfinite(x.x).all() for x in results)
    assert its.min() >= 1 and its.max() <= o["mr"] * o["cycles"]
