"""GPU tests of the device geometry of the 13-tree and holed cubed spheres (geometry types 2, 3, 4 of
d4est_hip_plan_set_geometry_analytic): volume and mortar factors generated on the device against the oracle fed the Python map's
host arrays, node coordinates from d4est_hip_plan_compute_xyz_analytic against the Python map, and the order of the boundary
coordinates that d4est_hip_plan_boundary_gather makes of them.  Radii as in tests/test_sphere_maps.py."""
import numpy as np
import pytest

from disco4est_amd import forest as F
from disco4est_amd.mesh import quad_nodes

pytestmark = pytest.mark.gpu
RTOL = 1e-12                      # tests/test_forest_gpu.py: one fp64 operator apply, re-association only
R_PLAIN = (1.0, 2.0, 6.0)
R_COMPACT = (1.0, 2.0, 20.0)      # compactified outer shell


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _geometry(gtype, outer=False, inner=False):
    """(connectivity, map, params) of a geometry type"""
    R = R_COMPACT if outer else R_PLAIN
    if gtype == 1:
        return F.cubed_sphere_7tree_connectivity(), F.CubedSphere7Map(1.0, 2.0, inner), (1.0, 2.0, float(inner))
    if gtype == 2:
        mp = F.CubedSphere13Map(*R, compactify_outer=outer)
        return F.cubed_sphere_13tree_connectivity(), mp, mp.params
    mp = F.SphereWithHoleMap(*R, compactify_outer=outer, compactify_inner=inner, cube_hole=(gtype == 4))
    return F.sphere_with_hole_connectivity(), mp, mp.params


def _trees(nt, *trees):
    r = np.zeros(nt, dtype=bool)
    r[list(trees)] = True
    return r


@pytest.mark.parametrize("gtype,deg,inc,level,refine,outer,inner,world", [
    (2, 3, 0, 0, None, False, False, 1),
    (2, 2, 1, 0, (0, 7, 12), True, False, 1),          # one outer wedge + one inner wedge + the cube refined
    (2, 7, 0, 0, None, False, False, 1),               # the one-wavefront whole-operator path
    (2, 9, 0, 0, (8,), False, False, 1),               # multi-wave kernels, hanging faces
    (2, 4, 0, 0, (2, 12), False, False, 3),            # ghost cells through m.cells(ghost ids)
    (3, 3, 0, 0, (9,), True, True, 1),
    (3, 4, 0, 0, None, False, False, 2),
    (4, 2, 0, 1, None, True, False, 1),
])
def test_sphere_factors_generated_on_the_device(gpu, hiplib, oracle, gtype, deg, inc, level, refine, outer, inner, world):
    """volume AND mortar factors from the analytic map on the device -- through oriented tree faces, shell-shell and wedge-cube
    interfaces, hanging faces and ghost elements -- against the oracle fed with the Python map's arrays: the stiffness term alone
    first (volume factors), then with the flux terms on top (mortar factors).  Structure and bound of
    tests/test_forest_gpu.py::test_cubed_sphere_factors_generated_on_the_device."""
    import torch
    from disco4est_amd import Plan, parallel as P
    from tests.test_forest_gpu import _LocalTransport, _Mailbox
    conn, mp, params = _geometry(gtype, outer, inner)
    rf = None if refine is None else _trees(conn.num_trees, *refine)
    mg = F.ForestMesh(conn, level, deg, mp, refine=rf, deg_quad_inc=inc)
    parts = P.partition_by_dofs(mg.deg_global, world)
    ug = mg.field()
    Jg, rstg = mg.geometry(); sg = mg.build_sides()
    ref_full = oracle.apply_aij(mg, Jg, rstg, sg, ug, penalty_prefactor=7.5, nthreads=8)
    mb = _Mailbox()
    ranks = []
    for r, (first, count) in enumerate(parts):
        m = F.ForestMesh(conn, level, deg, mp, refine=rf, deg_quad_inc=inc, first=first, count=count)
        s = m.build_sides()
        tree, q, dq = m.cells()
        plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, m.quad_type)
        plan.set_geometry_analytic(gtype, params, tree, q, dq, m.nf)
        plan.set_faces(s, 7.5, 0, analytic=(gtype, params, tree, q, dq, m.nf, m.cells(s["ghost_global_ids"])))
        ex = P.TraceExchange(P.plan_schedule(plan, m, s, parts), _LocalTransport(r, mb), plan.copy_blocks, gpu)
        du = _t(m.field(), gpu)
        tr = torch.empty(plan.trace_size, dtype=torch.float64, device=gpu)
        gt = torch.full((max(plan.ghost_trace_size, 1),), float("nan"), dtype=torch.float64, device=gpu)
        ranks.append((m, plan, ex, du, tr, gt))
    for m, plan, ex, du, tr, gt in ranks:
        plan.compute_face_traces(du, tr)
        ex.begin(tr)
    errs = []
    for m, plan, ex, du, tr, gt in ranks:
        ex.end(gt)
        dAu = torch.full_like(du, float("nan"))
        plan.apply_stiffness_matrix(du, dAu)
        J, rst = m.geometry()
        e_vol = _rel(dAu.cpu().numpy(), oracle.apply_stiffness(m, J, rst, m.field(), nthreads=8))
        plan.apply_flux(tr, gt, dAu)
        sl = slice(m.global_nodal_offset, m.global_nodal_offset + m.local_nodes)
        e_all = _rel(dAu.cpu().numpy(), ref_full[sl])
        plan.destroy()
        print("rank %d: stiffness %.3e, stiffness + flux %.3e" % (len(errs), e_vol, e_all))
        errs.append((e_vol, e_all))
    for e_vol, e_all in errs:
        assert e_vol <= RTOL, e_vol
        assert e_all <= RTOL, e_all


@pytest.mark.parametrize("quad_type", [0, 1])
@pytest.mark.parametrize("gtype,outer,inner", [(1, False, True), (2, True, False), (3, True, True), (4, False, False)])
def test_node_coordinates_on_the_device(gpu, hiplib, gtype, outer, inner, quad_type):
    """compute_xyz_analytic against ForestMesh.nodal_coords() and against the map at the quadrature nodes (Gauss and Lobatto), all four
    types, degrees 2 and 5 mixed over a mesh with hanging faces, both outputs and each alone.  Bound 1e-13 R2: a handful of roundings
    through tan, one sqrt and 1/(c - t).  On the host, the same C++ (d4est_hip_tree_map) is within 1e-14 R2 of numpy
    (tests/test_sphere_maps.py::test_host_map_matches_python_map; measured over its points: 1.5e-16 R2).  The outputs are pre-filled
    with NaN and carry a guard tail: every entry must be finite, nothing may be written past 3 * local_nodes."""
    import torch
    from disco4est_amd import Plan
    conn, mp, params = _geometry(gtype, outer, inner)
    R2 = params[2] if gtype != 1 else params[1]
    nt = conn.num_trees
    rf = _trees(nt, 0, nt - 1)
    probe = F.ForestMesh(conn, 0, 2, mp, refine=rf)
    deg = np.where(np.arange(probe.global_elements) % 3 == 1, 5, 2)
    m = F.ForestMesh(conn, 0, deg, mp, refine=rf, deg_quad_inc=1, quad_type=quad_type)
    assert m.build_sides()["side_hang"].max() > 0 and set(m.deg.tolist()) == {2, 5}
    ref_l = np.concatenate(m.nodal_coords())
    ref_q = [np.empty(m.local_nodes_quad) for _ in range(3)]
    for e in range(m.n_elements):
        pq = int(m.deg_quad[e])
        X = mp.x(int(m.tree[e]), m._cell_xi(m.org[e], m.size[e], m._tensor_ref(quad_nodes(quad_type, pq))))
        for d in range(3):
            ref_q[d][m.quad_stride[e]:m.quad_stride[e] + (pq + 1) ** 3] = X[:, d]
    ref_q = np.concatenate(ref_q)
    tree, q, dq = m.cells()
    plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, m.quad_type)
    guard = 64
    worst = 0.0
    for want_l, want_q in ((True, True), (True, False), (False, True), (True, True)):     # the last: a second call re-uses the plan's staging
        xl = torch.full((3 * m.local_nodes + guard,), float("nan"), dtype=torch.float64, device=gpu)
        xq = torch.full((3 * m.local_nodes_quad + guard,), float("nan"), dtype=torch.float64, device=gpu)
        plan.compute_xyz_analytic(gtype, params, tree, q, dq, m.nf, xl if want_l else None, xq if want_q else None)
        torch.cuda.synchronize()
        for want, got, ref in ((want_l, xl.cpu().numpy(), ref_l), (want_q, xq.cpu().numpy(), ref_q)):
            assert np.isnan(got[ref.size:]).all()                   # nothing past 3 * local_nodes
            if not want:
                assert np.isnan(got).all()
                continue
            assert np.isfinite(got[:ref.size]).all()
            worst = max(worst, np.abs(got[:ref.size] - ref).max() / R2)
    plan.destroy()
    print("worst |x_dev - x_numpy| / R2 = %.3e" % worst)
    assert worst <= 1e-13


def test_boundary_gather_orders_the_device_coordinates(gpu, hiplib, oracle):
    """boundary_gather of the three device Lobatto components == the Lobatto coordinates of the boundary faces in the order
    plan_set_dirichlet_values expects (sides["bndry_xyz"]), to the coordinate bound 1e-13 R2.  Then g = x^2 + y^2 + z^2 built ON THE
    DEVICE from them is fed as Dirichlet data: A(x^2 + y^2 + z^2) equals the oracle's with host-built g to RTOL, and the consistency
    error against M(-6) -- exact only on affine elements -- falls with p by the factor
    tests/test_forest.py::test_cubed_sphere_oracle_symmetry_and_convergence demands of the 7-tree sphere (0.05 from p = 3 to p = 6,
    deg_quad = deg + 2); a boundary block in the wrong order leaves an O(1) error at every p.  13-tree sphere, level 0."""
    import torch
    from disco4est_amd import Plan
    conn, mp, params = _geometry(2)
    errs = []
    for p in (3, 6):
        m = F.ForestMesh(conn, 0, p, mp, deg_quad_inc=2)
        s = m.build_sides()
        tree, q, dq = m.cells()
        plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, m.quad_type)
        plan.set_geometry_analytic(2, params, tree, q, dq, m.nf)
        plan.set_faces(s, 10.0, 0, analytic=(2, params, tree, q, dq, m.nf, None))
        xyz = torch.full((3 * m.local_nodes,), float("nan"), dtype=torch.float64, device=gpu)
        plan.compute_xyz_analytic(2, params, tree, q, dq, m.nf, xyz, None)
        nb = int(s["total_bndry_nodes"])
        b = torch.full((3, nb), float("nan"), dtype=torch.float64, device=gpu)
        for d in range(3):
            plan.boundary_gather(xyz[d * m.local_nodes:(d + 1) * m.local_nodes], b[d])
        bx = np.stack([np.asarray(a) for a in s["bndry_xyz"]])
        assert np.abs(b.cpu().numpy() - bx).max() <= 1e-13 * R_PLAIN[2]
        g = (b * b).sum(dim=0).contiguous()
        plan.set_dirichlet_values(g)
        x, y, z = (xyz[d * m.local_nodes:(d + 1) * m.local_nodes] for d in range(3))
        u = (x * x + y * y + z * z).contiguous()
        Au = torch.full_like(u, float("nan"))
        plan.apply_aij(u, Au)
        rhs = torch.full_like(u, float("nan"))
        plan.apply_mass_matrix(torch.full_like(u, -6.0), rhs)
        Au, rhs = Au.cpu().numpy(), rhs.cpu().numpy()
        plan.destroy()
        J, rst = m.geometry()
        ref = oracle.apply_aij(m, J, rst, s, u.cpu().numpy(), bndry_lobatto=bx[0] ** 2 + bx[1] ** 2 + bx[2] ** 2, penalty_prefactor=10.0, nthreads=8)
        assert _rel(Au, ref) <= RTOL, _rel(Au, ref)
        errs.append(np.abs(Au - rhs).sum() / np.abs(rhs).sum())
    print("consistency error p = 3, 6:", errs)
    assert errs[1] < 0.05 * errs[0], errs
