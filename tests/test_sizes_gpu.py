"""GPU tests of the device element size parameters and of face_h_type / volume_h_type in the device mortar geometry
(csrc/d4est_hip_sizes.hip; d4est_hip_plan_set_h_types, _compute_size_parameters_*, _compute_diameters, _size_parameter) against the
numpy restatement tests/dense_sizes.py.

Two places where the cases differ from a literal reading of their specification, both because no implementation could meet it:
  * "plan A differs from a plan left at the default by more than 1e-6" is asserted for every type on the hanging mesh, and on the
    conforming anisotropic brick for TREE_H, VOLUME_DIV_AREA, FACE_DIAM and TOTAL_VOLUME_DIV_TOTAL_AREA.  For J_DIV_SJ_MIN / MEAN / MAX on
    a conforming brick J / sj is one constant per face, so these three ARE the default there; the test asserts that instead (1e-12).
  * the rotated two-tree pair of forest.py is a trilinear-map geometry, for which the engine has no device mortar form (brick and the
    four sphere maps only), so there is no plan A to build on it.  Sides with f_p != f_m ^ 1 and a non-zero orientation, where hp must
    take face f_p of the (+) element, are exercised on the 13-tree sphere, and the test asserts that the mesh has them."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import dense_sizes as DS

pytestmark = pytest.mark.gpu
NAMES = DS.PER_ELEMENT + DS.PER_FACE
ANISO = (0.0, 1.0, 0.0, 2.0, 0.0, 0.5)
R_COMPACT = (1.0, 2.0, 20.0)


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max())


def _arrays(plan):
    return {k: plan.size_parameter(k).clone() for k in NAMES}


def _sphere(deg):
    from disco4est_amd import forest as F
    mp = F.CubedSphere13Map(*R_COMPACT, compactify_outer=True)
    conn = F.cubed_sphere_13tree_connectivity()
    if deg == "mixed":
        deg = np.array([(1, 3, 7, 9)[i % 4] for i in range(13)])
    return F.ForestMesh(conn, 0, deg, mp), mp


def _plan(m):
    from disco4est_amd import Plan
    return Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, m.quad_type)


@pytest.mark.parametrize("deg", [1, 2, 3, 7, 9, 19, "mixed"])
def test_sphere_size_parameters(gpu, hiplib, deg):
    """13-tree sphere, compactified outer shell: all seven arrays against the restatement fed the device's own coordinates
    (diameters 1e-14: one three-term sum of squares under FMA contraction; the rest 1e-12, the single-apply tolerance); the
    coordinates-only entry gives diam_volume and diam_face bit for bit; a second call repeats every array bit for bit.
    p = 1, 2, 3: several elements per workgroup; 9: around one tile; 19: several tiles; mixed {1, 3, 7, 9}: bucket strides."""
    import torch
    m, mp = _sphere(deg)
    tree, q, dq = m.cells()
    plan = _plan(m)
    xyz = torch.full((3 * m.local_nodes,), float("nan"), dtype=torch.float64, device=gpu)
    plan.compute_xyz_analytic(2, mp.params, tree, q, dq, m.nf, xyz, None)
    assert plan.size_parameter("diam_volume") is None and plan.size_parameter("area") is None
    plan.compute_size_parameters(analytic=(2, mp.params, tree, q, dq, m.nf))
    got = _arrays(plan)
    plan.compute_size_parameters(analytic=(2, mp.params, tree, q, dq, m.nf))
    again = _arrays(plan)
    for k in NAMES:
        assert got[k].numel() == (1 if k in DS.PER_ELEMENT else 6) * m.n_elements
        assert torch.equal(got[k], again[k]), k
    plan.compute_diameters(xyz)
    assert torch.equal(plan.size_parameter("diam_volume"), got["diam_volume"])
    assert torch.equal(plan.size_parameter("diam_face"), got["diam_face"])
    assert plan.size_parameter("volume") is None
    plan.destroy()
    xh = xyz.cpu().numpy().reshape(3, -1)
    ref = DS.size_parameters_analytic(2, mp.params, tree, q, dq, float(m.nf), m.deg, xyz=xh, nodal_stride=m.nodal_stride)
    for k in NAMES:
        e = _rel(got[k].cpu().numpy(), ref[k])
        print("%-14s %.3e" % (k, e))
        assert e <= (1e-14 if k.startswith("diam") else 1e-12), (k, e)


@pytest.mark.parametrize("deg", [1, 2, 3, 7, 9, 19, "mixed"])
def test_sinemap_brick_diameters(gpu, hiplib, deg):
    """level-1 brick under SineMap (a geometry the engine has no map for): diam_volume / diam_face from the uploaded node coordinates"""
    from disco4est_amd import mesh as M
    if deg == "mixed":
        deg = np.array([(1, 3, 7, 9)[i % 4] for i in range(8)])
    m = M.BrickMesh(1, deg)
    xyz = np.concatenate(m.nodal_coords(M.SineMap(0.05)))
    plan = _plan(m)
    plan.compute_diameters(_t(xyz, gpu))
    dv, df = plan.size_parameter("diam_volume").cpu().numpy(), plan.size_parameter("diam_face").cpu().numpy()
    plan.destroy()
    rv, rf = DS.diameters(xyz.reshape(3, -1), m.deg, m.nodal_stride)
    print("diam_volume %.3e diam_face %.3e" % (_rel(dv, rv), _rel(df, rf)))
    assert _rel(dv, rv) <= 1e-14 and _rel(df, rf) <= 1e-14


@pytest.mark.parametrize("volume_h_type", [0, 1])
def test_anisotropic_brick_size_parameters(gpu, hiplib, volume_h_type):
    """brick (0,1) x (0,2) x (0,0.5), locally refined (two element sizes), degrees 2 and 4: the closed form"""
    m, dq, root_len = _hanging_brick()
    plan = _plan(m)
    plan.set_h_types(0, volume_h_type)
    plan.compute_size_parameters(brick=(dq, root_len, ANISO))
    got = {k: v.cpu().numpy() for k, v in _arrays(plan).items()}
    plan.destroy()
    ref = DS.size_parameters_brick(dq, root_len, ANISO, volume_h_type=volume_h_type)
    for k in NAMES:
        e = _rel(got[k], ref[k])
        print("%-14s %.3e" % (k, e))
        assert e <= (1e-14 if k.startswith("diam") else 1e-12), (k, e)


# ---- hm / hp through the operator ------------------------------------------------------------------------------------------------
def _hanging_brick():
    from disco4est_amd import mesh as M
    refine = np.zeros(8, dtype=bool)
    refine[0] = True                                   # the hanging faces of cell 0 towards its three neighbours
    deg = np.array([2] * 8 + [4] * 7)                  # p = 2 on the small elements, 4 on the big ones: mixed across every hanging face
    m = M.HangingBrickMesh(1, refine, deg)
    return m, m.size.astype(np.int32), 4.0


def _case(kind):
    """(mesh, J, rst, host side list, device form (brick= / analytic= of Plan.set_faces), size parameters, tree_h)"""
    from disco4est_amd import mesh as M
    if kind == "conforming":
        m = M.BrickMesh(1, 3)
        mp = DS.ScaleMap(ANISO)
        dq = np.ones(8, dtype=np.int32)
        J, rst = m.geometry(mp)
        return m, J, rst, m.build_sides(mp), dict(brick=(dq, 2.0, ANISO)), DS.size_parameters_brick(dq, 2.0, ANISO), dq / 2.0
    if kind == "hanging":
        m, dq, root_len = _hanging_brick()
        mp = DS.ScaleMap(ANISO)
        J, rst = m.geometry(mp)
        return m, J, rst, m.build_sides(mp), dict(brick=(dq, root_len, ANISO)), DS.size_parameters_brick(dq, root_len, ANISO), dq / root_len
    m, mp = _sphere(3)
    tree, q, dq = m.cells()
    J, rst = m.geometry()
    s = m.build_sides()
    turned = (s["side_nbr"] >= 0) & (s["side_nbr_face"] != (np.arange(6 * m.n_elements) % 6 ^ 1)) & (s["side_reorder"] != 0)
    assert turned.any()                                # hp must take face f_p of the (+) element through an orientation
    sp = DS.size_parameters_analytic(2, mp.params, tree, q, dq, float(m.nf), m.deg)
    return m, J, rst, s, dict(analytic=(2, mp.params, tree, q, dq, m.nf, None)), sp, dq / float(m.nf)


_CASES = {}


def _cached_case(kind):
    if kind not in _CASES:
        _CASES[kind] = _case(kind)
    return _CASES[kind]


def _apply(gpu, m, J, rst, sides, u, h_type=None, **device_form):
    import torch
    plan = _plan(m)
    plan.set_geometry(J, rst)
    if h_type is not None:
        plan.set_h_types(h_type, 0)
    plan.set_faces(sides, 10.0, 1, **device_form)      # penalty meanp_sqr_over_meanh: sensitive to hm AND hp (min h hides the larger)
    Au = torch.full_like(u, float("nan"))
    plan.apply_aij(u, Au)
    out = Au.cpu().numpy()
    plan.destroy()
    return out


@pytest.mark.parametrize("name", sorted(DS.FACE_H, key=DS.FACE_H.get))
@pytest.mark.parametrize("kind", ["conforming", "hanging", "sphere"])
def test_face_h_type_through_the_operator(gpu, hiplib, kind, name):
    """plan A = set_h_types + the device mortar form against plan B = host mortar arrays whose hm / hp are the restatement's:
    apply_aij of a random vector to 1e-12 |Au|_inf; and plan A against a plan left at the default (see the module docstring)"""
    from disco4est_amd import mesh as M
    ht = DS.FACE_H[name]
    m, J, rst, sides, form, sp, tree_h = _cached_case(kind)
    u = _t(M.splitmix64_uniform(11, m.local_nodes) - 0.5, gpu)
    hm, hp = DS.mortar_h_arrays(m, sides, sp, tree_h, ht)
    A = _apply(gpu, m, J, rst, sides, u, h_type=ht, **form)
    B = _apply(gpu, m, J, rst, dict(sides, hm=hm, hp=hp), u)
    scale = np.abs(B).max()
    print("%s %s: |A - B| / |B| = %.3e" % (kind, name, np.abs(A - B).max() / scale))
    assert np.isfinite(A).all() and np.abs(A - B).max() <= 1e-12 * scale
    if ht != 0 and kind != "sphere":
        D = _apply(gpu, m, J, rst, sides, u, **form)
        diff = np.abs(A - D).max() / scale
        print("against the default: %.3e" % diff)
        if kind == "conforming" and name in ("FACE_H_EQ_J_DIV_SJ_MIN_LOBATTO", "FACE_H_EQ_J_DIV_SJ_MEAN_LOBATTO", "FACE_H_EQ_J_DIV_SJ_MAX_LOBATTO"):
            assert diff <= 1e-12      # J / sj is constant on the faces of a conforming brick: these three are the default there
        else:
            assert diff > 1e-6


# ---- ghost sides -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["FACE_H_EQ_VOLUME_DIV_AREA", "FACE_H_EQ_J_DIV_SJ_MIN_LOBATTO"])
def test_two_shards_match_one_rank(gpu, hiplib, name):
    """a level-1 brick of mixed degree on two virtual ranks (tests/test_parallel_gpu.py's kind): the gathered apply_lhs of the
    device mortar form with this face_h_type equals the one-rank result to 1e-12 -- hp of a ghost side comes from the ghost element's
    own size parameters"""
    import torch
    from disco4est_amd import Plan, mesh as M, parallel as P
    from tests.test_parallel_gpu import _LocalTransport, _Mailbox
    ht = DS.FACE_H[name]
    deg_global = np.array([(2, 3, 4)[i % 3] for i in range(8)])
    mg = M.BrickMesh(1, deg_global)
    ug = M.splitmix64_uniform(3, mg.local_nodes) - 0.5

    def make(m):
        plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, 0)
        dq = np.ones(m.n_elements, dtype=np.int32)
        plan.set_geometry_brick(dq, 2.0, ANISO)
        plan.set_h_types(ht, 0)
        s = m.build_sides(geometry=False)
        plan.set_faces(s, 10.0, 0, brick=(dq, 2.0, ANISO))
        return plan, s

    plan, _ = make(mg)
    ref = torch.full((mg.local_nodes,), float("nan"), dtype=torch.float64, device=gpu)
    plan.apply_lhs(_t(ug, gpu), ref)
    ref = ref.cpu().numpy()
    plan.destroy()
    parts = P.partition_by_dofs(deg_global, 2)
    mb = _Mailbox()
    got = np.full_like(ref, np.nan)
    ranks = []
    for r, (first, count) in enumerate(parts):
        m = M.BrickMesh(1, deg_global, first=first, count=count)
        plan, s = make(m)
        assert len(s["ghost_deg"]) > 0
        ex = P.TraceExchange(P.plan_schedule(plan, m, s, parts), _LocalTransport(r, mb), plan.copy_blocks, gpu)
        u = _t(ug[m.global_nodal_offset:m.global_nodal_offset + m.local_nodes], gpu)
        tr = torch.empty(plan.trace_size, dtype=torch.float64, device=gpu)
        gt = torch.full((max(plan.ghost_trace_size, 1),), float("nan"), dtype=torch.float64, device=gpu)
        ranks.append((m, plan, ex, u, tr, gt))
    for m, plan, ex, u, tr, gt in ranks:       # the steps of apply_lhs on every rank: traces + exchange, then volume + flux
        plan.compute_face_traces(u, tr)
        ex.begin(tr)
    for m, plan, ex, u, tr, gt in ranks:
        ex.end(gt)
        Au = torch.full_like(u, float("nan"))
        plan.apply_stiffness_matrix(u, Au)
        plan.apply_flux(tr, gt, Au)
        got[m.global_nodal_offset:m.global_nodal_offset + m.local_nodes] = Au.cpu().numpy()
        plan.destroy()
    assert np.isfinite(got).all() and np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()


_ABORT_CHILD = """
import numpy as np
from disco4est_amd import Plan, mesh as M
m = M.BrickMesh(1, 2, first=0, count=4)
plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, 0)
plan.set_h_types("FACE_H_EQ_FACE_DIAM", 0)
s = m.build_sides(geometry=False)
assert len(s["ghost_deg"]) > 0
plan.set_faces(s, 10.0, 0, brick=(np.ones(4, dtype=np.int32), 2.0, (0., 1., 0., 1., 0., 1.)))
print("NOT REACHED")
"""


def test_face_diam_on_a_plan_with_ghost_sides_aborts(gpu, hiplib):
    """the reference reads diam_face without the ghost offset (src/Mesh/d4est_mesh.c:841): rejected, with a message that says so --
    a host-side check before any launch, seen from a child process"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-c", _ABORT_CHILD], capture_output=True, text=True, timeout=120, cwd=root, env=env)
    assert p.returncode != 0 and "NOT REACHED" not in p.stdout
    assert "[D4EST_HIP_ABORT]" in p.stderr and "FACE_H_EQ_FACE_DIAM" in p.stderr and "without the ghost offset" in p.stderr, p.stderr


# ---- estimator -------------------------------------------------------------------------------------------------------------------
def test_estimator_takes_the_plan_diameters(gpu, hiplib):
    """estimator_bi(diam = None) after compute_size_parameters equals the call with the explicit array bit for bit, for both
    volume_h_types; with CUBE_APPROX the residual term is one third of its DIAM value (1e-15 relative)"""
    import torch
    from disco4est_amd import mesh as M
    m, dq, root_len = _hanging_brick()
    mp = DS.ScaleMap(ANISO)
    J, rst = m.geometry(mp)
    sides = m.build_sides(mp)
    u = _t(m.field(mp), gpu)
    r = _t(M.splitmix64_uniform(5, m.local_nodes) - 0.5, gpu)
    term0 = []
    for vht in (0, 1):
        plan = _plan(m)
        plan.set_geometry(J, rst)
        plan.set_h_types(0, vht)
        plan.set_estimator(7, 8, 9, 10.0)
        plan.set_faces(sides, 10.0, 0)
        plan.compute_size_parameters(brick=(dq, root_len, ANISO))
        out = []
        for diam in (None, plan.size_parameter("diam_volume").clone()):
            eta2 = torch.full((m.n_elements,), float("nan"), dtype=torch.float64, device=gpu)
            terms = torch.full((4 * m.n_elements,), float("nan"), dtype=torch.float64, device=gpu)
            plan.estimator_bi(u, r, diam, eta2, terms=terms)
            out.append((eta2, terms))
        assert torch.isfinite(out[0][0]).all()
        assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
        term0.append(out[0][1][:m.n_elements].cpu().numpy())
        plan.destroy()
    e = np.abs(term0[1] - term0[0] / 3.0).max() / np.abs(term0[0] / 3.0).max()
    print("term0(CUBE_APPROX) vs term0(DIAM) / 3: %.3e" % e)
    assert (term0[0] > 0).all() and e <= 1e-15
