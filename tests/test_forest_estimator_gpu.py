"""The estimator's and the energy norm's face kernels on faces BETWEEN trees.  Three device kernels outside the operator re-orient the
neighbour's mortar data themselves, each with its own reorder_index(code, ...): est_geom_kernel (the (+) side's drst_p through kp and
off_p), est_face_kernel (qp from the trace or, kind 2, the ghost trace, at kp [+ u_shift]) -- csrc/d4est_hip_estimator.hip -- and
norms_face_kernel (qp[kp + u_shift]) -- csrc/d4est_hip_norms.hip.  Outside this module they meet an orientation other than 0 only on the
7-tree cubed sphere at p = 3 (codes 0, 1, 2, 3, 7, deg_quad = deg, conforming, one rank).  Here: two warped trees glued through the
(f_m, f_p, orientation) triples of tests/forest_whole_operator_cases.py, at the degrees of tests/forest_estimator_cases.py
(tests/test_forest_estimator_dense.py proves on the CPU what each list covers, and pins the dense forms on these gluings): NQ != N, the
p >= 8 buckets, a degree jump across the oriented face, oriented and code-0 sides in one launch, a hanging face on the tree boundary,
oriented ghost blocks, and the pointwise estimator.

Reference: tests/dense_estimator.py and tests/dense_norms.py, which restate the reference's re-orientation (also where it is not the
geometric one).  Bounds: RTOL and _per_elem_rel of tests/test_estimator_gpu.py, the 1e-14 of its test_shards_match_one_plan between
shards and one plan; nothing new.  Every family prints one line with its worst error and what its cases covered."""
import contextlib

import numpy as np
import pytest

from disco4est_amd import forest as F, mesh as M
from tests import dense_estimator as DE, dense_norms as DN
from tests import forest_estimator_cases as E, forest_whole_operator_cases as C
from tests.test_estimator_gpu import RTOL, _LocalTransport, _Mailbox, _per_elem_rel, _rfo, _t

pytestmark = pytest.mark.gpu

ALL_CODES, ALL_FACES = set(range(8)), set(range(6))
EST_FCNS = [(7, 8, 9), (2, 3, 6), (4, 5, 9), (0, 1, 6)]      # the estimator's penalty ids, running with the case (ids 2 - 6 are not
EST_PREF, NORM_PREF = 10.0, 7.5                              # symmetric in (deg_m, h_m) <-> (deg_p, h_p)); the norm's id is k % 4
_WORST = {}


@pytest.fixture(autouse=True)
def _no_face_path_override(monkeypatch):
    monkeypatch.delenv("D4EST_HIP_FACE_DIRECT", raising=False)


def _one_blas_thread():
    """the dense forms are many small matrix products: one BLAS thread is the fast way through them (speed only)"""
    try:
        from threadpoolctl import threadpool_limits
    except ImportError:
        return contextlib.nullcontext()
    return threadpool_limits(limits=1, user_api="blas")


def _note(family, err):
    _WORST[family] = max(_WORST.get(family, 0.0), float(err))


def _report(family, cov=None):
    print("estimator and energy norm on tree faces: %s: worst per-element rel. error vs the dense forms %.3e%s" % (
        family, _WORST.get(family, float("nan")),
        "" if cov is None else "; codes %s, f_p %s" % (sorted(cov["codes"]), sorted(cov["f_p"]))))


def _pair(rots, level, deg, warp=None, **kw):
    conn = F.Connectivity.rotated_pair(*rots)
    return F.ForestMesh(conn, level, deg, F.TrilinearMap(conn, M.SineMap(0.03) if warp is None else warp), **kw)


def _dirichlet(sides):
    bx = sides["bndry_xyz"]
    return np.sin(bx[0]) + bx[1] * bx[2]


class _Case:
    """one mesh with its factors, side tables, data (field, random residual, random sizes, non-zero Dirichlet data) and, computed once,
    the dense estimator and the dense energy norm"""

    def __init__(self, m, k, dense=True):
        self.m, self.k = m, k
        self.J, self.rst = m.geometry()
        self.sides = m.build_sides()
        self.fcns, self.fcn = EST_FCNS[k % 4], k % 4
        self.u = m.field()
        self.r = M.splitmix64_uniform(5 + k, m.local_nodes, offset=m.global_nodal_offset) - 0.5
        self.diam = (0.5 + M.splitmix64_uniform(6 + k, m.global_elements))[m.first:m.first + m.n_elements]
        self.g = _dirichlet(self.sides)
        if dense:
            with _one_blas_thread():
                self.ref_terms, self.ref_eta2 = DE.DenseEstimator(m, self.J, self.rst, self.sides, _rfo(), self.fcns, EST_PREF).compute(
                    self.u, self.r, self.diam, g=self.g)
                self.ref_eterms, self.ref_esums = DN.DenseNorms(m, self.J, self.rst, self.sides, _rfo(), self.fcn, NORM_PREF).energy(self.u)

    def plan(self, tune=()):
        """set_estimator (and set_energy_norm) before set_faces, as _run of tests/test_estimator_gpu.py"""
        from disco4est_amd import Plan
        m = self.m
        plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, m.quad_type)
        plan.set_geometry(self.J, self.rst)
        for key, value in tune:
            plan.set_tuning(key, value)
        plan.set_estimator(*self.fcns, EST_PREF)
        plan.set_energy_norm(self.fcn, NORM_PREF)
        plan.set_faces(self.sides, 10.0, 0)
        return plan


def _device(gpu, plan, c, ghost_trace=None, pointwise=None):
    """(eta2, terms[4, ne], energy terms[3, ne], energy sums[4]) of the plan, every output pre-filled with NaN"""
    import torch
    ne = c.m.n_elements
    nan = lambda n: torch.full((n,), float("nan"), dtype=torch.float64, device=gpu)
    du = _t(c.u, gpu)
    eta2, terms, eterms, esums = nan(ne), nan(4 * ne), nan(3 * ne), nan(4)
    if pointwise is None:
        plan.estimator_bi(du, _t(c.r, gpu), c.diam, eta2, terms=terms, ghost_trace=ghost_trace, g=c.g)
    else:
        plan.estimator_bi_pointwise(du, _t(pointwise, gpu), c.diam, eta2, terms=terms, ghost_trace=ghost_trace, g=c.g)
    plan.ip_energy_norm_sqr(du, esums, elem_terms=eterms, ghost_trace=ghost_trace)
    torch.cuda.synchronize()
    out = (eta2.cpu().numpy(), terms.cpu().numpy().reshape(4, -1), eterms.cpu().numpy().reshape(3, -1), esums.cpu().numpy())
    assert all(np.isfinite(a).all() for a in out)
    return out


def _hold(family, got, c, what=""):
    """the device results against the case's dense forms: _per_elem_rel and RTOL of tests/test_estimator_gpu.py (the sums: relative)"""
    eta2, terms, eterms, esums = got
    assert np.abs(c.ref_terms[1:3]).min() > 0 and c.ref_eterms[2].min() > 0      # the jump terms are exercised
    rel = {"terms": _per_elem_rel(terms, c.ref_terms), "eta2": _per_elem_rel(eta2, c.ref_eta2),
           "energy terms": _per_elem_rel(eterms, c.ref_eterms),
           "energy sums": max(abs(esums[i] - c.ref_esums[i]) / max(abs(c.ref_esums[i]), 1e-300) for i in range(4))}
    _note(family, max(rel.values()))
    assert max(rel.values()) <= RTOL, (family, what, rel)


def _face_codes(c, face):
    return {int(c.sides["side_reorder"][sd]) for sd, _ in face}


# ---- 1: conforming, level 0, two elements -----------------------------------------------------------------------------------------------------
def _sweep(gpu, deg, inc, name, warp, family):
    """level 0, two elements, both views of the glued face in one plan, the penalty ids running over the cases"""
    total = {}
    for k, (trip, rots) in enumerate(getattr(C, name)):
        c = _Case(_pair(rots, 0, deg, warp, deg_quad_inc=inc), k)
        face = C.tree_face_sides(c.m, c.sides)
        assert len(face) == 2 and _face_codes(c, face) == {C.code_of(trip)}
        plan = c.plan()
        try:
            _hold(family, _device(gpu, plan, c), c, trip)
        finally:
            plan.destroy()
        C.merge(total, C.coverage(c.m, c.sides, face))
    assert total["codes"] == ALL_CODES and total["f_p"] == ALL_FACES, total
    _report(family, total)


@pytest.mark.parametrize("deg,inc,name", [(d, i, n) for d, i, n, _ in E.CONFORMING], ids=[i for _, _, _, i in E.CONFORMING])
def test_conforming_on_every_gluing(gpu, hiplib, deg, inc, name):
    """p = 2 with deg_quad = 3 (NQ != N) and p = 3 through all 144 triples, p = 7, p = 9 (the p >= 8 buckets) and the degree jumps
    [2, 3] / [3, 2] (deg_quad = deg + 1, the mortar at the larger one) through every 5th"""
    _sweep(gpu, deg, inc, name, None, "conforming, deg %s, deg_quad_inc %d, %s" % (deg, inc, name))


@pytest.mark.parametrize("deg,inc,name", [(d, i, n) for d, i, n, _ in E.ASYMMETRIC], ids=[i for _, _, _, i in E.ASYMMETRIC])
def test_conforming_on_a_face_without_symmetry(gpu, hiplib, deg, inc, name):
    """the same meshes under a warp that has no symmetry on the glued face (tests/forest_estimator_cases.py: ASYMMETRIC): under
    mesh.SineMap the (+) side's dr/dx on a level-0 face reads the same in every order, so only here do NQ != N, p = 9 and the degree
    jumps show the order in which est_geom_kernel reads it"""
    _sweep(gpu, deg, inc, name, E.SkewSineMap(0.03), "conforming, skew warp, deg %s, deg_quad_inc %d, %s" % (deg, inc, name))


# ---- 2: level 1: oriented and code-0 sides in one launch; the pointwise estimator ----------------------------------------------------------------
_LEVEL1 = {}


def _level1_case(k):
    if k not in _LEVEL1:
        _LEVEL1[k] = _Case(_pair(C.LEVEL1[k][1], 1, E.LEVEL1_DEG), k)
    return _LEVEL1[k]


def test_oriented_and_code0_sides_in_one_launch(gpu, hiplib):
    """16 elements, p = 3: sides across the tree face (the triple's code) and sides inside a tree (code 0) under one kernel launch; the
    operator's face path taken both ways (tuning key 11 = 2: the one-kernel operator, = 0: two-phase) -- the estimator and the norm form
    their own traces, so: equal bits, before and after an operator apply"""
    import torch
    family = "level 1, p = %d, oriented and code-0 sides together" % E.LEVEL1_DEG
    total = {}
    for k, (trip, rots) in enumerate(C.LEVEL1):
        c = _level1_case(k)
        face = C.tree_face_sides(c.m, c.sides)
        assert len(face) == 8 and _face_codes(c, face) == {C.code_of(trip)}
        assert any(int(c.sides["side_reorder"][sd]) == 0 for sd, n in C.interior_sides(c.m, c.sides) if (sd, n) not in face)
        out, paths = [], []
        for key11 in (2, 0):
            plan = c.plan(((11, key11),))
            try:
                paths.append(plan.face_path())
                a = _device(gpu, plan, c)
                du = _t(c.u, gpu)
                plan.apply_aij(du, torch.empty_like(du))          # an operator apply in between changes nothing
                b = _device(gpu, plan, c)
            finally:
                plan.destroy()
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
            _hold(family, a, c, (trip, key11))
            out.append(a)
        assert paths == ["direct+volume", "two-phase"], paths       # two different operator paths really were compared
        assert all(np.array_equal(x, y) for x, y in zip(out[0], out[1]))
        C.merge(total, C.coverage(c.m, c.sides, face))
    assert total["codes"] == ALL_CODES and total["f_p"] == ALL_FACES, total
    _report(family, total)


def test_pointwise_estimator_on_oriented_faces(gpu, hiplib):
    """d4est_hip_estimator_bi_pointwise on the same level-1 meshes: term 0 from a residual at the quadrature nodes against
    tests/dense_hessian.py's h^2 / p^2 sum_q w J r_q^2 at the 1e-13 of tests/test_estimator_pointwise_gpu.py, terms 1 - 3 (which do not
    depend on the residual) and eta2 against the dense face terms at RTOL"""
    from tests import dense_hessian as DH
    from tests.test_estimator_pointwise_gpu import RTOL_TERM0
    family = "pointwise estimator, level 1, p = %d" % E.LEVEL1_DEG
    codes = set()
    for k, (trip, rots) in enumerate(C.LEVEL1):
        c = _level1_case(k)
        codes |= _face_codes(c, C.tree_face_sides(c.m, c.sides))
        rq = M.splitmix64_uniform(9 + k, c.m.local_nodes_quad) - 0.5
        ref = c.ref_terms.copy()
        ref[0] = DH.DenseHessian(c.m, "numerical", xyz=c.m.nodal_coords(), rst=c.rst).pointwise_term0(rq, c.J, c.diam)
        ref_eta2 = ((ref[0] + ref[1]) + ref[2]) + ref[3]
        plan = c.plan()
        try:
            eta2, terms, _, _ = _device(gpu, plan, c, pointwise=rq)
        finally:
            plan.destroy()
        rel0 = (np.abs(terms[0] - ref[0]) / ref[0]).max()
        rel = max(_per_elem_rel(terms, ref), _per_elem_rel(eta2, ref_eta2))
        _note(family, max(rel0, rel))
        assert ref[0].min() > 0 and np.abs(ref[1:3]).min() > 0
        assert rel0 <= RTOL_TERM0 and rel <= RTOL, (trip, rel0, rel)
    assert codes == ALL_CODES
    _report(family)


# ---- 3: the hanging face ON the tree boundary ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [0, 1], ids=["tree0-refined", "tree1-refined"])
def test_hanging_face_on_the_tree_boundary(gpu, hiplib, half):
    """one tree refined, nine elements, the 1 <-> 4 face oriented: the big side's four sub-mortars read the small sides' blocks (off_p,
    the sub-face permutation), the small sides read the big side's (u_shift where the reference's re-orientation is not geometric), with
    the degree layouts of tests/test_forest_gpu.py::test_apply_aij_hanging_across_trees and tuning key 13 = 0 and 1 (the split hanging
    kernels), as tests/test_estimator_gpu.py::test_parity_hanging_mixed.  Left out by name: several degrees on a face whose small sides
    see a non-geometric re-orientation -- faces_setup refuses it (csrc/d4est_hip_faces_setup.hip: "plan_set_hanging: small side ...:
    its sub-mortars have different quadrature degrees"); one degree there."""
    refine = C.HANGING_REFINES[half]
    family = "hanging face on the tree boundary, tree %d refined" % half
    total, seen_o, mixed_o, n_nongeometric = {}, set(), set(), 0
    for k, (trip, rots) in enumerate(C.HANGING):
        m0 = _pair(rots, 0, E.HANGING_DEG, refine=refine)
        deg = E.hanging_degrees(trip, refine, m0.n_elements)
        if len(set(deg.tolist())) > 1:
            mixed_o.add(trip[2])
        n_nongeometric += not C.geometric(C.hanging_small_view(trip, refine))
        c = _Case(_pair(rots, 0, deg, refine=refine), k)
        s = c.sides
        face = C.tree_face_sides(c.m, s)
        assert (s["side_hang"] == 1).sum() == 1 and (s["side_hang"] == 2).sum() == 4
        assert {int(s["side_hang"][sd]) for sd, _ in face} == {1, 2} and _face_codes(c, face) == {C.code_of(trip)}
        assert int(s["side_orientation"].max()) == trip[2]
        seen_o.add(trip[2])
        out = []
        for key13 in (0, 1):
            plan = c.plan(((13, key13),))
            try:
                out.append(_device(gpu, plan, c))
            finally:
                plan.destroy()
            _hold(family, out[-1], c, (trip, key13))
        C.merge(total, C.coverage(c.m, s, face))
    # tree 0's face is the small sides' (half 0) or the big side's (half 1): the orientations 0..3 occur in either role, with one degree
    # and with the mixed layout
    assert seen_o == mixed_o == {0, 1, 2, 3} and n_nongeometric > 0
    assert total["codes"] == ALL_CODES and total["f_p"] == ALL_FACES, total
    _report(family, total)


# ---- 4: oriented ghost blocks (kind 2) ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hooks", [False, True], ids=["ghost_trace", "hooks"])
def test_oriented_ghost_blocks(gpu, hiplib, hooks):
    """one level-1 tree per rank: every ghost side is the oriented tree face, est_face_kernel and norms_face_kernel re-orient the
    exchanged block (kind 2).  The ghost trace handed over by the caller, or (hooks) exchanged by the calls themselves through the
    plan_set_comm hooks: the ranks' eta2 concatenated is the one-plan result to the 1e-14 of test_shards_match_one_plan, the norm's sums
    add up and its terms concatenate as in tests/test_norms_gpu.py::test_shards_add_up; the one-plan result against the dense forms"""
    import torch
    from disco4est_amd import parallel as P
    family = "oriented ghost blocks, %s" % ("plan_set_comm hooks" if hooks else "ghost_trace handed over")
    total = {}
    for k, (trip, rots) in enumerate(C.GHOST):
        conn = F.Connectivity.rotated_pair(*rots)
        mp = F.TrilinearMap(conn, M.SineMap(0.03))
        make = lambda first, count: F.ForestMesh(conn, 1, E.GHOST_DEG, mp, first=first, count=count)
        cg = _Case(make(0, None), k)
        assert _face_codes(cg, C.tree_face_sides(cg.m, cg.sides)) == {C.code_of(trip)}
        pg = cg.plan()
        try:
            one = _device(gpu, pg, cg)
        finally:
            pg.destroy()
        _hold(family, one, cg, trip)
        mb = _Mailbox()
        ranks = []
        for rk, (first, count) in enumerate(E.GHOST_PARTS):
            c = _Case(make(first, count), k, dense=False)
            lo, n = c.m.global_nodal_offset, c.m.local_nodes
            assert np.array_equal(c.u, cg.u[lo:lo + n]) and np.array_equal(c.r, cg.r[lo:lo + n])
            assert np.array_equal(c.diam, cg.diam[first:first + count])
            ghost = E.ghost_sides(c.sides)
            assert len(ghost) == 4 and _face_codes(c, ghost) == {C.code_of(trip)}
            C.merge(total, C.coverage(c.m, c.sides, ghost))
            plan = c.plan()
            if hooks:
                ex = P.attach(plan, c.m, c.sides, E.GHOST_PARTS, _LocalTransport(rk, mb), gpu)
            else:
                ex = P.TraceExchange(P.plan_schedule(plan, c.m, c.sides, E.GHOST_PARTS), _LocalTransport(rk, mb), plan.copy_blocks, gpu)
            assert plan.ghost_trace_size > 0
            ranks.append({"c": c, "plan": plan, "ex": ex, "tr": torch.empty(plan.trace_size, dtype=torch.float64, device=gpu),
                          "gt": torch.full((plan.ghost_trace_size,), float("nan"), dtype=torch.float64, device=gpu)})
        try:
            for st in ranks:   # every rank's traces posted up front (with the hooks, each call re-posts its own and then collects)
                st["plan"].compute_face_traces(_t(st["c"].u, gpu), st["tr"])
                st["ex"].begin(st["tr"])
            parts = []
            for st in ranks:
                if not hooks:
                    st["ex"].end(st["gt"])
                parts.append(_device(gpu, st["plan"], st["c"], ghost_trace=None if hooks else st["gt"]))
        finally:
            for st in ranks:
                st["plan"].destroy()
        eta2 = np.concatenate([p[0] for p in parts])
        assert np.abs(eta2 - one[0]).max() <= 1e-14 * np.abs(one[0]).max(), trip
        assert _per_elem_rel(np.concatenate([p[1] for p in parts], axis=1), one[1]) <= RTOL
        assert _per_elem_rel(np.concatenate([p[2] for p in parts], axis=1), one[2]) <= RTOL
        esums = parts[0][3] + parts[1][3]
        assert max(abs(esums[i] - one[3][i]) / abs(one[3][i]) for i in range(4)) <= RTOL
    assert total["codes"] == ALL_CODES and total["f_p"] == ALL_FACES, total
    _report(family, total)
