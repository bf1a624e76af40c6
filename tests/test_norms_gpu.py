"""GPU tests of the device error norms (csrc/d4est_hip_norms.hip: d4est_hip_norms_error, d4est_hip_norm_l2_sqr, d4est_hip_norm_linfty,
d4est_hip_ip_energy_norm_sqr, d4est_hip_masked_sum) against the numpy restatement of the reference's formulas (tests/dense_norms.py):
per-element values by term and the totals at the estimator tests' tolerance, Linfty and the error field exactly; uniform, graded,
hanging and cubed-sphere meshes; the four SIPG penalty ids; skip masks; shards with a trace exchange; determinism and independence
of the operator's face path; no change to plans without the energy norm.  The energy norm's jump term on oriented faces between trees
beyond the cubed sphere's (all eight reorder codes, NQ != N, p >= 8, degree jumps, hanging faces, ghost blocks):
tests/test_forest_estimator_gpu.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import dense_norms as DN
from tests.test_estimator_gpu import _LocalTransport, _Mailbox, _hanging, _per_elem_rel, _rfo, _t

pytestmark = pytest.mark.gpu
RTOL = 1e-12   # the project's tolerance for this class of reduction (tests/test_estimator_gpu.py)


def _plan(m, J, rst, sides, fcn=0, pref=10.0, energy=True, setup=None, estimator=False):
    from disco4est_amd import Plan
    plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, m.quad_type)
    plan.set_geometry(J, rst)
    if setup:
        setup(plan)
    if estimator:
        plan.set_estimator(7, 8, 9, 10.0)
    if energy:
        plan.set_energy_norm(fcn, pref)
    plan.set_faces(sides, 10.0, 0)
    return plan


def _device_norms(gpu, plan, v, skip=None, ghost_trace=None):
    """everything the device computes from the field v: (l2_array, l2 sum, linf, energy terms[3, ne], energy sums[4])"""
    import torch
    ne = plan.n_elements
    nan = lambda n: torch.full((n,), float("nan"), dtype=torch.float64, device=gpu)
    dv = _t(v, gpu)
    arr, s, mx, terms, sums = nan(ne), nan(1), nan(1), nan(3 * ne), nan(4)
    plan.norm_l2_sqr(dv, s, skip=skip, l2_array=arr)
    plan.norm_linfty(dv, mx, skip=skip)
    plan.ip_energy_norm_sqr(dv, sums, elem_terms=terms, ghost_trace=ghost_trace)
    torch.cuda.synchronize()
    return arr.cpu().numpy(), float(s.item()), float(mx.item()), terms.cpu().numpy().reshape(3, -1), sums.cpu().numpy()


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def _check_all(gpu, m, J, rst, sides, v, fcn=0, pref=10.0, skip=None, setup=None):
    plan = _plan(m, J, rst, sides, fcn, pref, setup=setup)
    arr, s, mx, terms, sums = _device_norms(gpu, plan, v, skip)
    dn = DN.DenseNorms(m, J, rst, sides, _rfo(), fcn, pref)
    ref_arr, ref_s = dn.l2_sqr(v, skip)
    ref_terms, ref_sums = dn.energy(v)
    rel = {"l2_array": _per_elem_rel(arr, ref_arr), "l2": _rel(s, ref_s), "terms": _per_elem_rel(terms, ref_terms),
           "sums": max(_rel(sums[i], ref_sums[i]) for i in range(4))}
    print("norms rel. differences:", rel)
    assert np.isfinite(arr).all() and np.isfinite(terms).all() and np.isfinite(sums).all()
    assert max(rel.values()) <= RTOL, rel
    assert mx == dn.linfty(v, skip)
    plan.destroy()
    return ref_terms, ref_sums


@pytest.mark.parametrize("level,deg,inc,curved,quad_type", [(1, 3, 0, False, 0), (1, 7, 0, False, 0), (1, 4, 1, True, 0), (1, 2, 1, True, 0),
                                                          (1, 3, 1, True, 1), (1, 5, 0, True, 1), (0, 15, 2, True, 0), (1, 1, 0, True, 0),
                                                          (1, 1, 1, False, 0)])
def test_parity_brick(gpu, hiplib, level, deg, inc, curved, quad_type):
    """uniform bricks, affine and curved, Gauss and Lobatto quadrature; p = 15 with deg_quad = 17 (LDS above 64 KB); p = 1 (the
    smallest bucket)"""
    from disco4est_amd import mesh as M
    m = M.BrickMesh(level, deg, deg_quad_inc=inc, quad_type=quad_type)
    mp = M.SineMap(0.05) if curved else None
    J, rst = m.geometry(mp)
    sides = m.build_sides(mp)
    rt, rs = _check_all(gpu, m, J, rst, sides, m.field(mp))
    assert rt[0].min() > 0 and rt[1].min() > 0 and (level == 0 or rt[2].min() > 0)   # every term is exercised


def test_parity_graded_mixed_p(gpu, hiplib):
    from disco4est_amd import mesh as M
    m = M.BrickMesh(1, np.array([3, 4, 5, 6, 7, 8, 9, 5]), deg_quad_inc=1)
    mp = M.SineMap(0.04)
    J, rst = m.geometry(mp)
    sides = m.build_sides(mp)
    _check_all(gpu, m, J, rst, sides, m.field(mp))


@pytest.mark.parametrize("hp_split", [0, 1])
def test_parity_hanging_mixed(gpu, hiplib, hp_split):
    from disco4est_amd import mesh as M
    m, _ = _hanging([2, 5], 3)
    mp = M.SineMap(0.04)
    J, rst = m.geometry(mp)
    sides = m.build_sides(mp)
    assert (sides["side_hang"] == 1).sum() > 0
    _check_all(gpu, m, J, rst, sides, m.field(mp), setup=lambda p: p.set_tuning(13, hp_split))


def test_parity_cubed_sphere(gpu, hiplib):
    from disco4est_amd import forest as F
    fm = F.ForestMesh(F.cubed_sphere_7tree_connectivity(), 0, 3, F.CubedSphere7Map(1.0, 2.0))
    J, rst = fm.geometry()
    sides = fm.build_sides()
    assert (np.asarray(sides["side_reorder"]) != 0).any()
    _check_all(gpu, fm, J, rst, sides, fm.field())


@pytest.mark.parametrize("fcn", [0, 1, 2, 3])
def test_penalty_ids(gpu, hiplib, fcn):
    """every SIPG penalty id on a mesh whose face neighbours differ in degree (and, curved, in h): ids 1 and 3 are not symmetric in
    (deg_m, deg_p), so a wrong deg_p shows"""
    from disco4est_amd import mesh as M
    deg = np.array([2, 3, 4, 5, 3, 2, 5, 4])
    m = M.BrickMesh(1, deg, deg_quad_inc=1)
    mp = M.SineMap(0.05)
    J, rst = m.geometry(mp)
    sides = m.build_sides(mp)
    nbr = np.asarray(sides["side_nbr"]).reshape(-1, 6)
    interior = nbr >= 0
    assert (deg[nbr[interior]] != np.repeat(deg, 6).reshape(-1, 6)[interior]).all()   # no interior face joins equal degrees
    _check_all(gpu, m, J, rst, sides, m.field(mp), fcn=fcn, pref=7.5)


def test_skip_masks(gpu, hiplib):
    """a mask that skips some elements (l2_array still filled for all of them), and one that skips all: sum and Linf exactly 0"""
    import torch
    from disco4est_amd import mesh as M
    m, _ = _hanging([2, 5], 3)
    mp = M.SineMap(0.04)
    J, rst = m.geometry(mp)
    sides = m.build_sides(mp)
    v = np.abs(m.field(mp))
    skip = (M.splitmix64_uniform(77, m.n_elements) < 0.4).astype(np.int32)
    assert 0 < skip.sum() < m.n_elements
    _check_all(gpu, m, J, rst, sides, v, skip=skip)
    plan = _plan(m, J, rst, sides)
    every = np.ones(m.n_elements, dtype=np.int32)
    arr, s, mx, _, _ = _device_norms(gpu, plan, v, every)
    assert s == 0.0 and mx == 0.0 and arr.min() > 0
    # the mask as a device tensor, and masked_sum on its own
    dskip = torch.from_numpy(skip).to(gpu)
    out = torch.empty(1, dtype=torch.float64, device=gpu)
    plan.masked_sum(_t(arr, gpu), out, skip=dskip)
    assert _rel(out.item(), DN.masked_sum(arr, skip)) <= RTOL
    plan.masked_sum(_t(arr, gpu), out, skip=every)
    assert out.item() == 0.0
    plan.destroy()


def test_linfty_of_negative_values_is_zero(gpu, hiplib):
    import torch
    from disco4est_amd import mesh as M
    m = M.BrickMesh(1, np.array([1, 2, 3, 4, 1, 2, 3, 4]))
    J, rst = m.geometry()
    plan = _plan(m, J, rst, m.build_sides(), energy=False)
    out = torch.full((1,), float("nan"), dtype=torch.float64, device=gpu)
    v = -1.0 - M.splitmix64_uniform(3, m.local_nodes)
    plan.norm_linfty(_t(v, gpu), out)
    assert out.item() == 0.0
    v[m.local_nodes - 1] = 0.25      # the last node of the last element
    plan.norm_linfty(_t(v, gpu), out)
    assert out.item() == 0.25
    plan.destroy()


def test_error_field_exact(gpu, hiplib):
    import torch
    from disco4est_amd import mesh as M
    m = M.BrickMesh(1, np.array([1, 2, 3, 4, 1, 2, 3, 4]))
    J, rst = m.geometry()
    plan = _plan(m, J, rst, m.build_sides(), energy=False)
    u = M.splitmix64_uniform(5, m.local_nodes) - 0.5
    c = M.splitmix64_uniform(6, m.local_nodes) - 0.5
    err = torch.full((m.local_nodes,), float("nan"), dtype=torch.float64, device=gpu)
    plan.norms_error(_t(u, gpu), _t(c, gpu), err)
    assert np.array_equal(err.cpu().numpy(), np.abs(u - c))
    plan.norms_error(_t(u, gpu), None, err)
    assert np.array_equal(err.cpu().numpy(), np.abs(u))
    plan.destroy()


@pytest.mark.parametrize("hooks", [False, True])
def test_shards_add_up(gpu, hiplib, hooks):
    """two virtual ranks on the hanging mixed-degree mesh, ghost traces handed over by the caller or exchanged by the norm itself
    through the plan_set_comm hooks: the ranks' sums add up to the one-plan values, the per-element terms concatenate to them"""
    import torch
    from disco4est_amd import Plan, mesh as M, parallel as P
    mg, deg_global = _hanging([2, 5], 3)
    mp = M.SineMap(0.04)
    Jg, rstg = mg.geometry(mp)
    sg = mg.build_sides(mp)
    ug = mg.field(mp)
    pg = _plan(mg, Jg, rstg, sg)
    one_arr, one_l2, one_mx, one_terms, one_sums = _device_norms(gpu, pg, ug)
    pg.destroy()
    parts = P.partition_by_dofs(deg_global, 2)
    mb = _Mailbox()
    ranks = []
    for rk, (first, count) in enumerate(parts):
        m, _ = _hanging([2, 5], 3, first=first, count=count, deg_global=deg_global)
        J, rst = m.geometry(mp); s = m.build_sides(mp)
        plan = _plan(m, J, rst, s)
        if hooks:
            ex = P.attach(plan, m, s, parts, _LocalTransport(rk, mb), gpu)
        else:
            ex = P.TraceExchange(P.plan_schedule(plan, m, s, parts), _LocalTransport(rk, mb), plan.copy_blocks, gpu)
        lo, n = m.global_nodal_offset, m.local_nodes
        assert plan.ghost_trace_size > 0
        ranks.append({"plan": plan, "ex": ex, "u": ug[lo:lo + n], "tr": torch.empty(plan.trace_size, dtype=torch.float64, device=gpu),
                      "gt": torch.full((max(plan.ghost_trace_size, 1),), float("nan"), dtype=torch.float64, device=gpu)})
    for st in ranks:   # every rank's traces posted up front (with the hooks, each call re-posts its own and then collects)
        st["plan"].compute_face_traces(_t(st["u"], gpu), st["tr"])
        st["ex"].begin(st["tr"])
    l2, mx, terms, sums = 0.0, 0.0, [], np.zeros(4)
    for st in ranks:
        if not hooks:
            st["ex"].end(st["gt"])
        a, s_, x_, t_, e_ = _device_norms(gpu, st["plan"], st["u"], ghost_trace=None if hooks else st["gt"])
        l2 += s_; mx = max(mx, x_); terms.append(t_); sums += e_
        st["plan"].destroy()
    assert _rel(l2, one_l2) <= RTOL and mx == one_mx
    assert max(_rel(sums[i], one_sums[i]) for i in range(4)) <= RTOL
    assert _per_elem_rel(np.concatenate(terms, axis=1), one_terms) <= RTOL


def test_deterministic_and_face_path_independent(gpu, hiplib):
    """two calls, with an operator apply in between, give the same bits; so do plans whose operator takes the direct, the two-phase
    and the hybrid face path (the norms form their own traces)"""
    import torch
    from disco4est_amd import mesh as M
    cases = []
    m = M.BrickMesh(1, 5)
    cases.append((m, M.SineMap(0.04), [("direct", lambda p: p.set_tuning(11, 1)), ("two-phase", lambda p: p.set_tuning(11, 0))]))
    mh, _ = _hanging([1, 6], 5, inc=0, mixed=False)
    cases.append((mh, M.SineMap(0.04), [("hybrid", lambda p: p.set_tuning(14, -1)), ("two-phase", lambda p: p.set_tuning(14, 0))]))
    for m, mp, variants in cases:
        J, rst = m.geometry(mp)
        sides = m.build_sides(mp)
        v = m.field(mp)
        out = []
        for want, setup in variants:
            plan = _plan(m, J, rst, sides, setup=setup)
            assert plan.face_path().startswith(want), (plan.face_path(), want)
            a = _device_norms(gpu, plan, v)
            du = _t(v, gpu)
            plan.apply_aij(du, torch.empty_like(du))
            b = _device_norms(gpu, plan, v)
            for x, y in zip(a, b):
                assert np.array_equal(np.asarray(x), np.asarray(y))
            out.append(a)
            plan.destroy()
        for x, y in zip(out[0], out[1]):
            assert np.array_equal(np.asarray(x), np.asarray(y))


_ABORT_CHILD = """
import numpy as np, torch
from disco4est_amd import Plan, mesh as M
m = M.BrickMesh(1, 2)
J, rst = m.geometry()
plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, 0)
plan.set_geometry(J, rst)
plan.set_faces(m.build_sides(), 10.0, 0)
assert plan.lib.d4est_hip_plan_energy_norm_info(plan.handle, None, None) == 0
v = torch.zeros(m.local_nodes, dtype=torch.float64, device="cuda")
plan.ip_energy_norm_sqr(v, torch.zeros(4, dtype=torch.float64, device="cuda"))
print("NOT REACHED")
"""


@pytest.mark.parametrize("deg,hanging", [(7, False), (3, True)])
def test_plans_without_the_energy_norm_unchanged(gpu, hiplib, deg, hanging):
    import torch
    from disco4est_amd import mesh as M
    from tests import dense_estimator as DE
    if hanging:
        m, _ = _hanging([2, 5], deg)
    else:
        m = M.BrickMesh(1, deg)
    mp = M.SineMap(0.04)
    J, rst = m.geometry(mp)
    sides = m.build_sides(mp)
    u = _t(m.field(mp), gpu)
    r = _t(M.splitmix64_uniform(8, m.local_nodes) - 0.5, gpu)
    diam = DE.element_diameters(m, mp)
    res = []
    for energy in (False, True):
        plan = _plan(m, J, rst, sides, energy=energy, estimator=True)
        assert plan.lib.d4est_hip_plan_energy_norm_info(plan.handle, None, None) == int(energy)
        Au = torch.empty_like(u)
        eta2 = torch.empty(m.n_elements, dtype=torch.float64, device=gpu)
        plan.apply_aij(u, Au)
        plan.estimator_bi(u, r, diam, eta2)
        res.append((Au.clone(), eta2.clone(), plan.face_path()))
        plan.destroy()
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and res[0][2] == res[1][2]


def test_energy_norm_without_the_request_aborts_cleanly(gpu, hiplib):
    """a host-side argument check ([D4EST_HIP_ABORT], before any launch), seen from a child process"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-c", _ABORT_CHILD], capture_output=True, text=True, timeout=120, cwd=root, env=env)
    assert p.returncode != 0 and "NOT REACHED" not in p.stdout
    assert "[D4EST_HIP_ABORT] ip_energy_norm_sqr: the plan has no energy-norm set-up" in p.stderr


def test_masked_sum_of_eta2(gpu, hiplib):
    """d4est_norms_fcn_energy_estimator: the masked sum of the estimator's eta2"""
    import torch
    from disco4est_amd import mesh as M
    from tests import dense_estimator as DE
    m, _ = _hanging([2, 5], 3)
    mp = M.SineMap(0.04)
    J, rst = m.geometry(mp)
    sides = m.build_sides(mp)
    plan = _plan(m, J, rst, sides, estimator=True)
    u = _t(m.field(mp), gpu)
    r = _t(M.splitmix64_uniform(9, m.local_nodes) - 0.5, gpu)
    eta2 = torch.empty(m.n_elements, dtype=torch.float64, device=gpu)
    plan.estimator_bi(u, r, DE.element_diameters(m, mp), eta2)
    skip = (M.splitmix64_uniform(10, m.n_elements) < 0.5).astype(np.int32)
    out = torch.empty(2, dtype=torch.float64, device=gpu)
    plan.masked_sum(eta2, out[0:1], skip=skip)
    plan.masked_sum(eta2, out[1:2])
    e = eta2.cpu().numpy()
    assert _rel(out[0].item(), DN.masked_sum(e, skip)) <= RTOL and _rel(out[1].item(), e.sum()) <= RTOL
    assert 0 < out[0].item() < out[1].item()
    plan.destroy()
