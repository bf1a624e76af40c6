"""The whole-operator kernels -- faces_direct_kernel (p <= 7), operator_mw_kernel (p = 8..15) and the hybrid operator's hanging-aware,
mixed-aware and ghost-aware instances -- on faces BETWEEN trees: they re-orient the neighbour's mortar block themselves
(reorder_index(code, ...), the neighbour's reference frame out of the side descriptor), and outside this module they meet an orientation
other than 0 only on the 7-tree cubed sphere (codes 0, 1, 2, 3, 7, a few (f_m, f_p) pairs).  Here: two warped trees glued through the
(f_m, f_p, orientation) triples of tests/forest_whole_operator_cases.py (tests/test_forest_whole_operator_cases.py proves on the CPU what
each list covers), uniform degree so that the one-kernel forms are what runs -- every test asserts plan.face_path() (and, where the
library names it, the kernel) before it compares anything.

Reference: the oracle's apply_aij / cheby_iterate, which restate the reference's re-orientation verbatim.  Bounds: RTOL of
tests/test_forest_gpu.py for one apply, the bounds of its test_cubed_sphere_smoothers for the Chebyshev iterate; nothing new.
Not in conftest's _BOTH_FACE_PATHS: the tuning keys 11 (face kernel) and 14 (hybrid operator) are set here, case by case."""
import numpy as np
import pytest

from disco4est_amd import forest as F, mesh as M
from tests import forest_whole_operator_cases as C
from tests.test_forest_gpu import RTOL, _rel, _t

pytestmark = pytest.mark.gpu

ALL_CODES, ALL_FACES = set(range(8)), set(range(6))
_WORST = {}


@pytest.fixture(autouse=True)
def _no_face_path_override(monkeypatch):
    monkeypatch.delenv("D4EST_HIP_FACE_DIRECT", raising=False)


def _note(family, err):
    _WORST[family] = max(_WORST.get(family, 0.0), float(err))


def _report(family, cov=None):
    print("whole-operator kernels on tree faces: %s: worst rel-inf error vs the oracle %.3e%s" % (
        family, _WORST.get(family, float("nan")),
        "" if cov is None else "; codes %s, f_p %s" % (sorted(cov["codes"]), sorted(cov["f_p"]))))


def _pair(rots, level, deg, **kw):
    conn = F.Connectivity.rotated_pair(*rots)
    return F.ForestMesh(conn, level, deg, F.TrilinearMap(conn, M.SineMap(0.03)), **kw)


def _make_plan(m, J, rst, sides, fcn, tune):
    from disco4est_amd import Plan
    plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, m.quad_type)
    for key, value in tune:
        plan.set_tuning(key, value)
    plan.set_geometry(J, rst)
    plan.set_faces(sides, 7.5, fcn)
    return plan


def _check(gpu, oracle, m, fcn, tune, path_ok, family, kernel=None, sides=None, stream=None):
    """apply_aij with non-zero Dirichlet data against the oracle, on the asserted path; returns (side tables, face path)"""
    import torch
    J, rst = m.geometry()
    sides = m.build_sides() if sides is None else sides
    u = m.field()
    bx = sides["bndry_xyz"]
    g = np.sin(bx[0]) + bx[1] * bx[2]
    ref = oracle.apply_aij(m, J, rst, sides, u, bndry_lobatto=g, penalty_prefactor=7.5, penalty_fcn=fcn, nthreads=8)
    plan = _make_plan(m, J, rst, sides, fcn, tune)
    try:
        path = plan.face_path()
        assert path_ok(path), path
        plan.set_dirichlet_values(g)
        du = _t(u, gpu)
        outs = []
        for key12 in ((None,) if stream is None else stream):
            if key12 is not None:
                plan.set_tuning(12, key12)
                assert plan.stream_mode() == key12
            dAu = torch.full_like(du, float("nan"))
            plan.apply_aij(du, dAu)
            if kernel is not None:
                assert kernel in plan.last_kernel(), plan.last_kernel()
            if key12 is not None:
                assert (",stream" in plan.last_kernel()) == bool(key12), plan.last_kernel()
            got = dAu.cpu().numpy()
            assert np.isfinite(got).all()
            err = _rel(got, ref)
            _note(family, err)
            assert err <= RTOL, (family, err)
            outs.append(dAu)
        if len(outs) == 2:
            assert torch.equal(outs[0], outs[1])     # the stream-mode twin: same bits
    finally:
        plan.destroy()
    return sides, path


def _sweep(gpu, oracle, cases, deg, inc, key11, family, kernel):
    """level 0, two elements, both views of the glued face, the penalty id running over the cases"""
    want = "direct+volume" if (key11 == 2 and inc == 0) else "direct"
    total = {}
    for k, (trip, rots) in enumerate(cases):
        m = _pair(rots, 0, deg, deg_quad_inc=inc)
        s, _ = _check(gpu, oracle, m, k % 4, ((11, key11),), lambda p: p == want, family, kernel if want == "direct+volume" else None)
        C.merge(total, C.coverage(m, s, C.tree_face_sides(m, s)))
    assert total["codes"] == ALL_CODES and total["f_p"] == ALL_FACES, total
    _report(family, total)


# ---- 1: uniform degree, in-memory neighbour (kind 1) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("key11", [2, 1])
@pytest.mark.parametrize("deg,inc,cases", [(d, i, c) for d, i, c in C.SINGLE_WAVE], ids=["p1-all", "p3-all", "p7-fifth", "p3q5-fifth"])
def test_single_wave_kernel_on_every_gluing(gpu, hiplib, oracle, deg, inc, cases, key11):
    """faces_direct_kernel, as the whole operator (key 11 = 2: "direct+volume" where deg_quad = deg) and for the faces alone
    (key 11 = 1, and every deg_quad > deg instance: "direct"): p = 1 and 3 through all 144 triples, p = 7 and the
    (N, NQ) = (4, 6) instance through every 5th"""
    N, NQ = deg + 1, deg + inc + 1
    _sweep(gpu, oracle, cases, deg, inc, key11, "faces_direct_kernel<%d,%d> key 11 = %d" % (N, NQ, key11), "faces_direct_kernel<%d,%d,vol" % (N, NQ))


@pytest.mark.parametrize("deg,inc,cases", [(d, i, c) for d, i, c in C.MULTI_WAVE], ids=["p8-fifth", "p11-fifth", "p15-tenth"])
def test_multi_wave_kernel_on_every_gluing(gpu, hiplib, oracle, deg, inc, cases):
    """operator_mw_kernel (key 11 = 2): p = 8 and 11 through every 5th triple, p = 15 through every 10th and the four triples that bring
    in the codes a stride of 10 cannot reach (tests/forest_whole_operator_cases.py: TENTH)"""
    _sweep(gpu, oracle, cases, deg, inc, 2, "operator_mw_kernel<%d>" % (deg + 1), "operator_mw_kernel<%d,vol" % (deg + 1))


def test_oriented_and_code0_sides_in_one_launch(gpu, hiplib, oracle):
    """level 1, 16 elements, p = 3: sides across the tree face (the triple's code) and sides inside a tree (code 0) in the same launch,
    plain and as the stream-mode instantiation (tuning key 12, as test_faces_gpu.py::test_stream_mode_whole_operator sets it)"""
    family = "faces_direct_kernel<4,4> level 1, plain and stream mode"
    total = {}
    for k, (trip, rots) in enumerate(C.LEVEL1):
        m = _pair(rots, 1, 3)
        s, _ = _check(gpu, oracle, m, k % 4, ((11, 2),), lambda p: p == "direct+volume", family, "faces_direct_kernel<4,4,vol", stream=(0, 1))
        face = C.tree_face_sides(m, s)
        assert {int(s["side_reorder"][sd]) for sd, _ in face} == {C.code_of(trip)}
        assert any(int(s["side_reorder"][sd]) == 0 for sd, n in C.interior_sides(m, s) if (sd, n) not in face)
        C.merge(total, C.coverage(m, s, face))
    assert total["codes"] == ALL_CODES
    _report(family, total)


# ---- 2: the Chebyshev update fused into the whole-operator kernels, across an oriented face -------------------------------------------------
@pytest.mark.parametrize("deg", [3, 9])
def test_fused_chebyshev_update_across_oriented_faces(gpu, hiplib, oracle, deg):
    """cheby_iterate with key 11 = 2 on two level-1 trees glued with the codes 4, 5 and 6 (none of them on the cubed sphere): 4 and 5
    iterations -- the iterate ends in either of the two vectors it alternates between -- against the oracle's recurrence, at the bounds
    of test_forest_gpu.py::test_cubed_sphere_smoothers.  No graph capture (key 9 untouched)."""
    import torch
    family = "cheby_iterate, %s" % ("faces_direct_kernel<4,4>" if deg == 3 else "operator_mw_kernel<10>")
    codes = set()
    for k, (trip, rots) in enumerate(C.CHEBY):
        m = _pair(rots, 1, deg)
        J, rst = m.geometry()
        sides = m.build_sides()
        codes |= C.coverage(m, sides, C.tree_face_sides(m, sides))["codes"]
        oracle.set_operator(m, J, rst, sides, 7.5, k % 4, threads=8)
        oracle.set_hanging(None); oracle.set_lhs_coefficient(None); oracle.set_lhs_element_blocks(None)
        plan = _make_plan(m, J, rst, sides, k % 4, ((11, 2),))
        try:
            assert plan.face_path() == "direct+volume", plan.face_path()
            rhs = M.splitmix64_uniform(5, m.local_nodes) - 0.5
            u0 = M.splitmix64_uniform(6, m.local_nodes)
            lmax, _ = oracle.cg_eigs(u0, rhs, 8)
            for iters in (4, 5):
                u_ref, r_ref = oracle.cheby_iterate(u0, rhs, iters, lmax / 30.0, lmax)
                du, drhs = _t(u0, gpu), _t(rhs, gpu)
                dAu, dr = torch.full_like(du, float("nan")), torch.full_like(du, float("nan"))
                plan.cheby_iterate(du, drhs, dAu, dr, iters, lmax / 30.0, lmax)
                eu, er = _rel(du.cpu().numpy(), u_ref), _rel(dr.cpu().numpy(), r_ref)
                _note(family, max(eu, er))
                assert eu <= 1e-11 and er <= 1e-10, (trip, iters, eu, er)
        finally:
            plan.destroy()
    assert codes == {4, 5, 6}
    _report(family)


# ---- 3: ghost blocks (kind 2; the hybrid operator's ghost-aware override) ------------------------------------------------------------------
def _ghost_coverage(s, total):
    ghost = np.nonzero(s["side_nbr"] <= -2)[0]
    total["codes"] |= {int(c) for c in s["side_reorder"][ghost]}
    total["f_p"] |= {int(f) for f in s["side_nbr_face"][ghost]}
    return ghost.size


@pytest.mark.parametrize("deg", [3, 9])
def test_direct_kernels_read_oriented_ghost_blocks(gpu, hiplib, oracle, deg):
    """one level-1 tree per rank, key 11 = 2, key 14 = 0: every ghost side is the oriented tree face, the direct kernels (one-wavefront at
    p = 3, multi-wave at p = 9) re-orient the exchanged mortar-node block; the gathered apply_lhs against the one-rank oracle"""
    from tests.test_hybrid_ghost_gpu import _LocalTransport, _Mailbox, _gathered_apply_lhs, _shards
    family = "ghost sides, %s" % ("faces_direct_kernel<4,4>" if deg == 3 else "operator_mw_kernel<10>")
    total = dict(codes=set(), f_p=set())
    for trip, rots in C.GHOST:
        assert C.geometric(trip)
        conn = F.Connectivity.rotated_pair(*rots)
        mp = F.TrilinearMap(conn, M.SineMap(0.03))
        make = lambda first, count: F.ForestMesh(conn, 1, deg, mp, first=first, count=count)
        mg = make(0, None)
        Jg, rstg = mg.geometry()
        sg = mg.build_sides()
        ref = oracle.apply_aij(mg, Jg, rstg, sg, mg.field(), nthreads=8)
        mb = _Mailbox()
        ranks = _shards(make, [(0, 8), (8, 8)], None, 0, gpu, lambda r: _LocalTransport(r, mb), tune=((11, 2),))
        try:
            for st in ranks:
                assert st["plan"].face_path() == "direct+volume" and st["plan"].ghost_trace_size > 0, st["plan"].face_path()
                assert _ghost_coverage(st["s"], total) == 4
            got = _gathered_apply_lhs(ranks, [st["m"].field() for st in ranks], ref.size, gpu)
        finally:
            for st in ranks:
                st["plan"].destroy()
        err = _rel(got, ref)
        _note(family, err)
        assert err <= RTOL, (trip, err)
    assert total["codes"] == ALL_CODES and total["f_p"] == ALL_FACES, total
    _report(family, total)


def test_hybrid_ghost_aware_override_on_oriented_faces(gpu, hiplib, oracle):
    """the same shards at p = 3 with key 14 = 2: the hybrid operator's ghost-aware side (override kind 4) reads the oriented block from the
    ghost buffer; test_hybrid_ghost_gpu.py's _parity holds it to the oracle and to key 14 = 0 on the same shards"""
    from tests.test_hybrid_ghost_gpu import _parity
    total = dict(codes=set(), f_p=set())
    for trip, rots in C.GHOST:
        assert C.geometric(trip)
        conn = F.Connectivity.rotated_pair(*rots)
        mp = F.TrilinearMap(conn, M.SineMap(0.03))

        def check(st, cgd):
            assert _ghost_coverage(st["s"], total) == 4
            assert cgd[1] > 0, cgd           # clean elements beside (oriented) ghost sides

        _parity(lambda first, count: F.ForestMesh(conn, 1, 3, mp, first=first, count=count), [(0, 8), (8, 8)], None, gpu, oracle, check=check)
    assert total["codes"] == ALL_CODES and total["f_p"] == ALL_FACES, total
    print("whole-operator kernels on tree faces: hybrid ghost-aware sides: codes %s, f_p %s (errors: the lines of _parity above)" % (
        sorted(total["codes"]), sorted(total["f_p"])))


# ---- 4: the hybrid operator's forms on oriented faces (key 14 = 1, degrees <= 7) -------------------------------------------------------------
def _n_clean(path):
    return int(path.split(" on ")[1].split()[0])


def test_mixed_aware_form_on_oriented_faces(gpu, hiplib, oracle):
    """level 1, degrees 5 / 4 in one tree and 3 / 2 in the other (checkerboards): the clean elements are exactly those without a
    higher-degree neighbour (asserted against the plan's count), and among them the top-degree elements on the glued face own an oriented
    side whose lower-degree neighbour block they read from the trace array and re-orient (override kind 2) -- every code 0..7"""
    family = "hybrid, mixed-aware"
    codes = set()
    for k, (trip, rots) in enumerate(C.MIXED):
        conn = F.Connectivity.rotated_pair(*rots)
        m = F.ForestMesh(conn, 1, C.level1_degrees(conn.num_trees, k % 2, 5), F.TrilinearMap(conn, M.SineMap(0.03)))
        s, path = _check(gpu, oracle, m, k % 4, ((14, 1),), lambda p: p.startswith("hybrid") and "mixed-aware" in p, family)
        assert _n_clean(path) == sum(C.clean_without_higher_neighbour(m, s)), path
        got = C.mixed_aware_tree_face_codes(m, s)
        assert got == {C.code_of(trip)}, (trip, got)
        codes |= got
    assert codes == ALL_CODES
    _report(family)


@pytest.mark.parametrize("half", [0, 1])
def test_hanging_aware_form_on_oriented_faces(gpu, hiplib, oracle, half):
    """The meshes of test_forest_gpu.py::test_apply_aij_hanging_across_trees (one tree refined, the hanging face ON the tree boundary,
    orientation 0..3) on the hanging-aware hybrid form (keys 13 = 1, 14 = 1), the refined tree first (half 0) or second (half 1).
    One degree (p = 4): all nine elements are clean (asserted) -- the big element owns the oriented hanging side as kind 3 (left to the
    record kernels), the four small elements own it with the kind-2 override wherever the reference's re-orientation is geometric from
    their side (csrc/d4est_hip_faces_setup.hip: u_shift = 0 there; elsewhere the side stays with the record kernels, and the engine would abort
    on sub-mortars of several quadrature degrees: one degree only).  Mixed degrees on the geometric views: small elements on the face and
    the big one at p = 4, the other small ones at p = 3 -- exactly five clean elements, the big one and the four with the kind-2
    override --, or, every other case, the big element at p = 5: it alone is clean, no small side can take the override."""
    family = "hybrid, hanging-aware"
    refine = C.HANGING_REFINES[half]
    ok_path = lambda p: p.startswith("hybrid") and "hanging-aware" in p
    big_role, small_role, n_nongeometric = set(), set(), 0
    for k, (trip, rots) in enumerate(C.HANGING):
        m = _pair(rots, 0, 4, refine=refine)
        s, path = _check(gpu, oracle, m, k % 4, ((13, 1), (14, 1)), ok_path, family)
        assert (s["side_hang"] == 1).sum() == 1 and int(s["side_orientation"].max()) == trip[2]
        assert _n_clean(path) == m.n_elements == 9, path
        big_role.add(trip[2])
        if not C.geometric(C.hanging_small_view(trip, refine)):
            n_nongeometric += 1
            continue
        small_role.add(trip[2])
        big_higher = bool(k % 2)
        mm = _pair(rots, 0, C.hanging_degrees(s, m.n_elements, 4, big_higher), refine=refine)
        _, path = _check(gpu, oracle, mm, (k + 1) % 4, ((13, 1), (14, 1)), ok_path, family)
        assert _n_clean(path) == (1 if big_higher else 5), path
    assert big_role == small_role == {0, 1, 2, 3}
    assert n_nongeometric > 0
    _report(family)
