"""GPU tests of the device error estimator (d4est_hip_plan_set_estimator / d4est_hip_estimator_bi, csrc/d4est_hip_estimator.hip): every
term per element against the numpy restatement of d4est_estimator_bi_compute (tests/dense_estimator.py) on conforming, curved,
mixed-degree, hanging and cubed-sphere meshes; the ten penalty ids; shards with a trace exchange; determinism and independence of
the operator's face path; no change to plans without the estimator.  Faces between trees with an orientation other than 0 meet only
the cubed sphere here (codes 0, 1, 2, 3, 7, p = 3, conforming, one rank): every gluing, all eight codes, NQ != N, p >= 8, degree jumps,
hanging faces and ghost blocks on an oriented face are in tests/test_forest_estimator_gpu.py."""
import numpy as np
import pytest

from tests import dense_estimator as DE

pytestmark = pytest.mark.gpu
RTOL = 1e-12


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _rfo():
    from disco4est_amd import capi
    lib = capi.load_library()
    return lambda a, b, c, d: int(lib.d4est_hip_reorient_face_order(a, b, c, d))


def _per_elem_rel(got, ref):
    """largest relative difference per element, against that element's own scale (terms that vanish: against the row's scale)"""
    scale = np.maximum(np.abs(ref), 1e-300)
    row = np.abs(ref).max(axis=-1, keepdims=True) if ref.ndim == 2 else np.abs(ref).max()
    return (np.abs(got - ref) / np.maximum(scale, 1e-10 * np.maximum(row, 1e-300))).max()


def _hanging(level_pattern, deg, inc=1, mixed=True, first=0, count=None, deg_global=None):
    from disco4est_amd import mesh as M
    refine = np.zeros(8, dtype=bool)
    refine[level_pattern] = True
    if deg_global is None:
        m0 = M.HangingBrickMesh(1, refine, deg)
        deg_global = deg + (np.arange(m0.global_elements) * 5 % 7) if mixed else np.full(m0.global_elements, deg)
    return M.HangingBrickMesh(1, refine, deg_global, deg_quad_inc=inc, first=first, count=count), deg_global


def _run(gpu, m, J, rst, sides, fcns=(7, 8, 9), pref=10.0, g=None, seed=5, setup=None, mp=None, u=None, plan_hook=None):
    """(device eta2, device terms, dense terms, dense eta2, plan)"""
    import torch
    from disco4est_amd import Plan, mesh as M
    plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, m.quad_type)
    plan.set_geometry(J, rst)
    if setup:
        setup(plan)
    plan.set_estimator(*fcns, pref)
    plan.set_faces(sides, 10.0, 0)
    if plan_hook:
        plan_hook(plan)
    u = m.field(mp) if u is None else u
    r = M.splitmix64_uniform(seed, m.local_nodes) - 0.5
    diam = 0.5 + M.splitmix64_uniform(seed + 1, m.n_elements)
    du, dr = _t(u, gpu), _t(r, gpu)
    eta2 = torch.full((m.n_elements,), float("nan"), dtype=torch.float64, device=gpu)
    terms = torch.full((4 * m.n_elements,), float("nan"), dtype=torch.float64, device=gpu)
    plan.estimator_bi(du, dr, diam, eta2, terms=terms, g=g)
    torch.cuda.synchronize()
    ref_terms, ref_eta2 = DE.DenseEstimator(m, J, rst, sides, _rfo(), fcns, pref).compute(u, r, diam, g=g)
    return eta2.cpu().numpy(), terms.cpu().numpy().reshape(4, -1), ref_terms, ref_eta2, plan


def _check(eta2, terms, ref_terms, ref_eta2):
    assert np.isfinite(eta2).all() and np.isfinite(terms).all()
    assert _per_elem_rel(terms, ref_terms) <= RTOL
    assert _per_elem_rel(eta2, ref_eta2) <= RTOL


@pytest.mark.parametrize("level,deg,inc,curved,quad_type", [(1, 3, 0, False, 0), (1, 7, 0, False, 0), (1, 4, 1, True, 0), (1, 2, 1, True, 0),
                                                          (1, 3, 1, True, 1), (1, 5, 0, True, 1), (0, 15, 2, True, 0)])
def test_parity_brick(gpu, hiplib, level, deg, inc, curved, quad_type):
    """uniform bricks, affine and curved, Gauss and Lobatto quadrature; p = 15 with deg_quad = 17 (the residual kernel's LDS above 64 KB)"""
    from disco4est_amd import mesh as M
    m = M.BrickMesh(level, deg, deg_quad_inc=inc, quad_type=quad_type)
    mp = M.SineMap(0.05) if curved else None
    J, rst = m.geometry(mp)
    sides = m.build_sides(mp)
    bx = sides["bndry_xyz"]
    g = np.sin(bx[0]) + bx[1] * bx[2]
    e, t, rt, re, plan = _run(gpu, m, J, rst, sides, g=g, mp=mp)
    _check(e, t, rt, re)
    assert np.abs(rt[3]).min() > 0 and (level == 0 or np.abs(rt[1:3]).min() > 0)   # every term is exercised
    plan.destroy()


def test_parity_graded_mixed_p(gpu, hiplib):
    """graded p = 3 ... 9 (p >= 8 buckets among them), curved, over-integrated"""
    from disco4est_amd import mesh as M
    m = M.BrickMesh(1, np.array([3, 4, 5, 6, 7, 8, 9, 5]), deg_quad_inc=1)
    mp = M.SineMap(0.04)
    J, rst = m.geometry(mp)
    sides = m.build_sides(mp)
    bx = sides["bndry_xyz"]
    e, t, rt, re, plan = _run(gpu, m, J, rst, sides, g=bx[0] * bx[1] - bx[2], mp=mp)
    _check(e, t, rt, re)
    plan.destroy()


@pytest.mark.parametrize("hp_split", [0, 1])
def test_parity_hanging_mixed(gpu, hiplib, hp_split):
    from disco4est_amd import mesh as M
    m, _ = _hanging([2, 5], 3)
    mp = M.SineMap(0.04)
    J, rst = m.geometry(mp)
    sides = m.build_sides(mp)
    assert (sides["side_hang"] == 1).sum() > 0
    bx = sides["bndry_xyz"]
    e, t, rt, re, plan = _run(gpu, m, J, rst, sides, g=np.cos(bx[0]) + bx[2], mp=mp, setup=lambda p: p.set_tuning(13, hp_split))
    _check(e, t, rt, re)
    plan.destroy()


def test_parity_cubed_sphere(gpu, hiplib):
    """the 7-tree cubed sphere: faces between trees with p4est orientations != 0, curved"""
    from disco4est_amd import forest as F
    fm = F.ForestMesh(F.cubed_sphere_7tree_connectivity(), 0, 3, F.CubedSphere7Map(1.0, 2.0))
    J, rst = fm.geometry()
    sides = fm.build_sides()
    assert (np.asarray(sides["side_reorder"]) != 0).any()
    bx = sides["bndry_xyz"]
    e, t, rt, re, plan = _run(gpu, fm, J, rst, sides, g=bx[0] * bx[2], u=fm.field())
    _check(e, t, rt, re)
    plan.destroy()


def test_robin_plan_keeps_the_dirichlet_term(gpu, hiplib):
    """a Robin-configured operator: the estimator still evaluates the Dirichlet boundary term, and the plan's Robin state is untouched"""
    import torch
    from disco4est_amd import mesh as M
    m = M.BrickMesh(1, 3, deg_quad_inc=1)
    mp = M.SineMap(0.05)
    J, rst = m.geometry(mp)
    sides = m.build_sides(mp)
    tm = int(sides["total_mortar_nodes"])
    coeff = 0.5 + M.splitmix64_uniform(11, tm)
    rhs = M.splitmix64_uniform(12, tm) - 0.5
    bx = sides["bndry_xyz"]
    g = np.sin(bx[1]) + bx[0]
    u = m.field(mp)
    e, t, rt, re, plan = _run(gpu, m, J, rst, sides, g=g, mp=mp, u=u, plan_hook=lambda p: p.set_robin_values(coeff, rhs))
    _check(e, t, rt, re)
    assert rt[3].min() > 0
    # the operator is still the Robin one: same apply_aij as a fresh Robin plan without the estimator
    from disco4est_amd import Plan
    ref = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, 0)
    ref.set_geometry(J, rst); ref.set_faces(sides, 10.0, 0); ref.set_robin_values(coeff, rhs)
    du = _t(u, gpu)
    a, b = torch.empty_like(du), torch.empty_like(du)
    plan.apply_aij(du, a); ref.apply_aij(du, b)
    assert torch.equal(a, b)
    plan.destroy(); ref.destroy()


def test_penalty_ids_in_every_role(gpu, hiplib):
    from disco4est_amd import mesh as M
    m = M.BrickMesh(1, 2 + (np.arange(8) * 3) % 3, deg_quad_inc=1)
    mp = M.SineMap(0.05)
    J, rst = m.geometry(mp)
    sides = m.build_sides(mp)
    bx = sides["bndry_xyz"]
    g = bx[0] + bx[1] * bx[2]
    for i in range(10):
        for fcns in ((i, 8, 9), (7, i, 9), (7, 8, i)):
            e, t, rt, re, plan = _run(gpu, m, J, rst, sides, fcns=fcns, pref=7.5, g=g, mp=mp)
            _check(e, t, rt, re)
            plan.destroy()


def test_deterministic_and_face_path_independent(gpu, hiplib):
    import torch
    from disco4est_amd import Plan, mesh as M
    m, _ = _hanging([1, 6], 5, inc=0, mixed=False)
    mp = M.SineMap(0.04)
    J, rst = m.geometry(mp)
    sides = m.build_sides(mp)
    u, r = _t(m.field(mp), gpu), _t(M.splitmix64_uniform(3, m.local_nodes), gpu)
    diam = 0.5 + M.splitmix64_uniform(4, m.n_elements)
    out, paths = [], []
    for hybrid in (-1, 0):
        plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, 0)
        plan.set_geometry(J, rst)
        plan.set_tuning(14, hybrid)
        plan.set_estimator(7, 8, 9, 10.0)
        plan.set_faces(sides, 10.0, 0)
        e1 = torch.empty(m.n_elements, dtype=torch.float64, device=gpu)
        e2 = torch.empty_like(e1)
        plan.estimator_bi(u, r, diam, e1)
        Au = torch.empty_like(u)
        plan.apply_aij(u, Au)                 # an operator apply in between changes nothing
        plan.estimator_bi(u, r, diam, e2)
        assert torch.equal(e1, e2)
        out.append(e1.cpu().numpy())
        paths.append(plan.face_path())
        plan.destroy()
    assert paths[0].startswith("hybrid") and paths[1] == "two-phase", paths   # two different operator paths really were compared
    assert np.abs(out[0] - out[1]).max() <= 1e-14 * np.abs(out[1]).max()


@pytest.mark.parametrize("deg,hanging", [(7, False), (3, True)])
def test_plans_without_the_estimator_unchanged(gpu, hiplib, deg, hanging):
    import torch
    from disco4est_amd import Plan, mesh as M
    if hanging:
        m, _ = _hanging([2, 5], deg)
    else:
        m = M.BrickMesh(2, deg)
    mp = M.SineMap(0.04)
    J, rst = m.geometry(mp)
    sides = m.build_sides(mp)
    u = _t(m.field(mp), gpu)
    res = []
    for est in (False, True):
        plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, 0)
        plan.set_geometry(J, rst)
        if est:
            plan.set_estimator(7, 8, 9, 10.0)
        plan.set_faces(sides, 10.0, 0)
        Au = torch.empty_like(u)
        plan.apply_aij(u, Au)
        res.append((Au.clone(), plan.face_path()))
        plan.destroy()
    assert torch.equal(res[0][0], res[1][0]) and res[0][1] == res[1][1]


class _Mailbox:
    def __init__(self):
        self.box = {}


class _LocalTransport:
    def __init__(self, rank, mailbox):
        self.rank, self.mb = rank, mailbox

    def start(self, send_buf, recv_buf):
        for p, t in send_buf.items():
            self.mb.box[(self.rank, p)] = t.clone()
        return recv_buf

    def finish(self, recv_buf):
        for p, t in recv_buf.items():
            t.copy_(self.mb.box[(p, self.rank)])


@pytest.mark.parametrize("world,hooks", [(2, False), (3, False), (2, True), (3, True)])
def test_shards_match_one_plan(gpu, hiplib, world, hooks):
    """2 / 3 virtual ranks on a hanging + mixed mesh (shard boundaries cut hanging faces), ghost traces through an in-process exchange --
    handed over by the caller, or (hooks) exchanged by the estimator itself through the plan_set_comm hooks with ghost_trace = None:
    the ranks' eta2 concatenated is the one-plan result"""
    import torch
    from disco4est_amd import Plan, mesh as M, parallel as P
    mg, deg_global = _hanging([2, 5], 3)
    mp = M.SineMap(0.04)
    Jg, rstg = mg.geometry(mp)
    sg = mg.build_sides(mp)
    ug = mg.field(mp)
    rg = M.splitmix64_uniform(21, mg.local_nodes) - 0.5
    diam_g = 0.5 + M.splitmix64_uniform(22, mg.n_elements)
    bxg = sg["bndry_xyz"]
    pg = Plan(mg.deg, mg.deg_quad, mg.nodal_stride, mg.quad_stride, 0)
    pg.set_geometry(Jg, rstg); pg.set_estimator(7, 8, 9, 10.0); pg.set_faces(sg, 10.0, 0)
    one = torch.empty(mg.n_elements, dtype=torch.float64, device=gpu)
    pg.estimator_bi(_t(ug, gpu), _t(rg, gpu), diam_g, one, g=bxg[0] + bxg[1])
    one = one.cpu().numpy()
    pg.destroy()
    parts = P.partition_by_dofs(deg_global, world)
    mb = _Mailbox()
    ranks = []
    for rk, (first, count) in enumerate(parts):
        m, _ = _hanging([2, 5], 3, first=first, count=count, deg_global=deg_global)
        J, rst = m.geometry(mp); s = m.build_sides(mp)
        plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, 0)
        plan.set_geometry(J, rst); plan.set_estimator(7, 8, 9, 10.0); plan.set_faces(s, 10.0, 0)
        if hooks:
            ex = P.attach(plan, m, s, parts, _LocalTransport(rk, mb), gpu)
        else:
            ex = P.TraceExchange(P.plan_schedule(plan, m, s, parts), _LocalTransport(rk, mb), plan.copy_blocks, gpu)
        lo, n = m.global_nodal_offset, m.local_nodes
        bx = s["bndry_xyz"]
        st = {"m": m, "plan": plan, "ex": ex, "u": _t(ug[lo:lo + n], gpu), "r": _t(rg[lo:lo + n], gpu), "g": bx[0] + bx[1],
              "diam": diam_g[first:first + count], "tr": torch.empty(plan.trace_size, dtype=torch.float64, device=gpu),
              "gt": torch.full((max(plan.ghost_trace_size, 1),), float("nan"), dtype=torch.float64, device=gpu)}
        assert plan.ghost_trace_size > 0
        ranks.append(st)
    # every rank's traces posted up front (with the hooks, each estimator call re-posts its own in phase 0 and collects in phase 1)
    for st in ranks:
        st["plan"].compute_face_traces(st["u"], st["tr"])
        st["ex"].begin(st["tr"])
    got = []
    for st in ranks:
        e = torch.empty(st["m"].n_elements, dtype=torch.float64, device=gpu)
        if hooks:
            st["plan"].estimator_bi(st["u"], st["r"], st["diam"], e, g=st["g"])
        else:
            st["ex"].end(st["gt"])
            st["plan"].estimator_bi(st["u"], st["r"], st["diam"], e, ghost_trace=st["gt"], g=st["g"])
        got.append(e.cpu().numpy())
        st["plan"].destroy()
    got = np.concatenate(got)
    assert np.abs(got - one).max() <= 1e-14 * np.abs(one).max()
