"""GPU tests of the device point probes (d4est_hip_probe_*, csrc/d4est_hip_probe.hip) against the numpy restatement tests/dense_probe.py.

Tolerance, derived and not fitted: per point |device - restatement| <= (N^3 + 6 N) eps S with S = sum |l_k l_j l_i u_ijk| from the
restatement -- N^3 for any order of the N^3-term sum, 6 N for the roundings of the three basis products.  The reference-space gradient
uses the same bound per component with S formed from |l'|; the physical gradient the largest of the three S times the infinity norm of
the inverse Jacobian as it is applied (max over x_d of sum_i |dr_i/dx_d|).  Every point is held to it.  err, the element id and rst
must be the restatement's exactly (the same roundings in the same order).  xyz is no sum: a map evaluation is some ten operations of at
most one ulp and two tangents of at most two, so 32 eps max|xyz| bounds it.  The CPU side checks that no probed point makes the
restatement's own 3 x 3 inverse worse than that: cond_inf(dx/dr) <= (N^3 + 6 N) / 8."""
import numpy as np
import pytest

from tests import dense_probe as dp

pytestmark = pytest.mark.gpu

DEGS = np.array([1, 2, 3, 4, 7, 8, 19, 1, 2, 3, 4, 7, 8, 19, 5], dtype=np.int32)
EXTENTS = (0., 2., 0., 1., -1., 3.)


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _smooth(x, y, z):
    return np.sin(2.0 * x) * np.cos(y) + z ** 3 + x * y * z


class _BrickCase:
    """the 2 x 2 x 2 brick with its last octant refined once (15 elements, hanging faces, two dq), three fields with a padded stride, and
    the restatement's answers for the special points followed by 1000 random ones -- computed once for the whole module"""

    def __init__(self):
        from disco4est_amd import mesh as M
        refine = np.zeros(8, dtype=bool)
        refine[7] = True
        self.m = m = M.HangingBrickMesh(1, refine, DEGS)
        x, y, z = m.nodal_coords()
        self.stride = m.local_nodes + 5
        self.u = np.full(3 * self.stride, np.nan)
        self.u[:m.local_nodes] = _smooth(x, y, z)
        self.u[self.stride:self.stride + m.local_nodes] = np.cos(3.0 * x * y) - z
        self.u[2 * self.stride:2 * self.stride + m.local_nodes] = M.splitmix64_uniform(9, m.local_nodes) - 0.5
        inside = (m.org + m.size[:, None] * np.array([0.37, 0.52, 0.71])[None, :]) / m.root_len     # strictly inside every element
        special = np.array([
            [0.5, 0.25, 0.25],      # on the face between elements 0 and 1
            [0.5, 0.5, 0.25],       # on an edge of four coarse elements
            [0.5, 0.5, 0.5],        # the centre corner: seven coarse elements and a fine one
            [0.75, 0.75, 0.6],      # on an edge between four children of the refined octant
            [0.75, 0.6, 0.5],       # on a hanging face: coarse element 3 below, two children above
            [0.0, 0.0, 0.0], [1.0, 1.0, 1.0],
            [0.75, 0.25, 0.25],     # centre of element 1 (degree 2): the Lobatto node (1, 1, 1)
            [0.75, 0.75, 0.25],     # centre of element 3 (degree 4)
            [0.25, 0.75, 0.75],     # centre of element 6 (degree 19 has no centre node: an ordinary point)
            [0.3, 0.3, 0.3],        # tree out of range (1)
            [0.3, 0.3, 0.3],        # tree out of range (-1)
            [1.5, 0.5, 0.5],        # abc outside the tree
            [0.3, 0.3, 0.3],        # a valid neighbour of the three
        ])
        tree_special = np.zeros(special.shape[0], dtype=np.int32)
        tree_special[10], tree_special[11] = 1, -1
        self.n_special = inside.shape[0] + special.shape[0]
        rnd = M.splitmix64_uniform(2024, 3000).reshape(1000, 3)
        self.abc = np.concatenate([inside, special, rnd])
        self.tree = np.concatenate([np.zeros(inside.shape[0], dtype=np.int32), tree_special, np.zeros(1000, dtype=np.int32)])
        self.bad = inside.shape[0] + np.array([10, 11, 12])
        self.err, self.elem, self.rst = dp.locate(self.tree, self.abc, m.cells(), m.root_len)
        ok = self.ok = self.err == 0
        e = self.elem[ok]
        self.deg = np.zeros(self.tree.size, dtype=np.int32)
        self.ns = np.zeros(self.tree.size, dtype=np.int32)
        self.deg[ok], self.ns[ok] = m.deg[e], m.nodal_stride[e]
        n = self.tree.size
        self.val = np.full((3, n), np.nan)
        self.S = np.full((3, n), np.nan)
        for f in range(3):
            self.val[f, ok], self.S[f, ok] = dp.evaluate(self.u[f * self.stride:], self.ns[ok], self.deg[ok], self.rst[ok])
        self.g = np.full((n, 3), np.nan)
        self.gS = np.full((n, 3), np.nan)
        self.g[ok], self.gS[ok] = dp.gradient_ref(self.u, self.ns[ok], self.deg[ok], self.rst[ok])
        R = dp.drdx_brick(EXTENTS, m.size[e], m.root_len)
        self.gx = np.full((n, 3), np.nan)
        self.norm = np.full(n, np.nan)
        self.gx[ok], self.norm[ok] = dp.physical(self.g[ok], R)

    def probe(self, gpu, sel):
        from disco4est_amd import Plan, Probe
        m = self.m
        plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, 0)
        return plan, Probe(plan, self.tree[sel], self.abc[sel], m.cells(), m.root_len)


@pytest.fixture(scope="module")
def brick(hiplib):
    return _BrickCase()


def _assert_values(case, sel, got, n_fields):
    n = len(sel)
    for f in range(n_fields):
        dev, ref, S = got[f * n:(f + 1) * n], case.val[f, sel], case.S[f, sel]
        ok = case.ok[sel]
        assert np.isnan(dev[~ok]).all()
        tol = dp.bound(case.deg[sel][ok], S[ok])
        diff = np.abs(dev[ok] - ref[ok])
        print("field %d: %d points, max |device - restatement| / bound = %.3e" % (f, ok.sum(), np.max(diff / np.maximum(tol, 1e-300)) if ok.any() else 0.0))
        assert (diff <= tol).all()


def test_locate_special_points_and_every_degree(gpu, brick):
    """err, element and rst of the points inside every element, on faces, edges and corners (lowest matching id), at abc = 0 and 1, at a
    Lobatto node, and of the three err = 1 points -- exactly the restatement's"""
    sel = np.arange(brick.n_special)
    plan, pr = brick.probe(gpu, sel)
    err, elem, rst = pr.info()
    ns, deg = pr.element_info()
    assert err.tolist() == brick.err[sel].tolist() and err[brick.bad].tolist() == [1, 1, 1] and err.sum() == 3
    assert elem.tolist() == brick.elem[sel].tolist()
    assert elem[:15].tolist() == list(range(15)) and set(deg[:15]) == set(DEGS)
    assert elem[15:22].tolist() == [0, 0, 0, 7, 3, 0, 14]
    np.testing.assert_array_equal(rst, brick.rst[sel])
    np.testing.assert_array_equal(rst[22], [0.0, 0.0, 0.0])   # the degree-2 element's middle node
    assert ns.tolist() == brick.ns[sel].tolist() and deg.tolist() == brick.deg[sel].tolist()
    pr.destroy()
    plan.destroy()


def test_values_at_the_special_points(gpu, brick):
    import torch
    sel = np.arange(brick.n_special)
    plan, pr = brick.probe(gpu, sel)
    out = torch.zeros(len(sel), dtype=torch.float64, device=gpu)
    pr.eval(_t(brick.u, gpu), out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    _assert_values(brick, sel, got, 1)
    assert np.isnan(got[brick.bad]).all() and not np.isnan(got[brick.bad[-1] + 1])   # the valid neighbour is unaffected
    # at the Lobatto node the nodal value itself comes back (every other term of the sum is an exact zero)
    assert got[22] == brick.u[brick.m.nodal_stride[1] + 13]
    pr.destroy()
    plan.destroy()


@pytest.mark.parametrize("n_fields", [1, 3])
@pytest.mark.parametrize("n_points", [1, 63, 64, 65, 1000])
def test_batch_shapes(gpu, brick, n_points, n_fields):
    import torch
    sel = brick.n_special + np.arange(n_points)
    plan, pr = brick.probe(gpu, sel)
    err, elem, rst = pr.info()
    assert (err == 0).all() and elem.tolist() == brick.elem[sel].tolist()
    np.testing.assert_array_equal(rst, brick.rst[sel])
    out = torch.full((n_fields * n_points + 3,), -7.0, dtype=torch.float64, device=gpu)
    pr.eval(_t(brick.u, gpu), out, n_fields=n_fields, field_stride=brick.stride)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[n_fields * n_points:] == -7.0).all()
    _assert_values(brick, sel, got, n_fields)
    pr.destroy()
    plan.destroy()


def test_gradients_on_the_brick(gpu, brick):
    """reference-space and physical gradient (brick map with unequal extents) at the special points and 65 random ones"""
    import torch
    from disco4est_amd import capi
    sel = np.arange(brick.n_special + 65)
    n = len(sel)
    plan, pr = brick.probe(gpu, sel)
    du = _t(brick.u, gpu)
    g = torch.zeros(3 * n, dtype=torch.float64, device=gpu)
    pr.eval_gradient(du, g)
    torch.cuda.synchronize()
    got = g.cpu().numpy().reshape(3, n).T
    ok = brick.ok[sel]
    assert np.isnan(got[~ok]).all()
    tol = dp.bound(brick.deg[sel][ok][:, None], brick.gS[sel][ok])
    diff = np.abs(got[ok] - brick.g[sel][ok])
    print("reference-space gradient: max |device - restatement| / bound = %.3e" % np.max(diff / np.maximum(tol, 1e-300)))
    assert (diff <= tol).all()
    pr.set_map(capi.GEOM_BRICK, EXTENTS)
    pr.eval_gradient(du, g, physical=True)
    torch.cuda.synchronize()
    got = g.cpu().numpy().reshape(3, n).T
    assert np.isnan(got[~ok]).all()
    tol = dp.bound(brick.deg[sel][ok], brick.gS[sel][ok].max(axis=1)) * brick.norm[sel][ok]
    diff = np.abs(got[ok] - brick.gx[sel][ok])
    print("physical gradient: max |device - restatement| / bound = %.3e" % np.max(diff / tol[:, None]))
    assert (diff <= tol[:, None]).all()
    xyz = pr.xyz()
    ex = np.array(EXTENTS)
    want = ex[0::2][None, :] + (ex[1::2] - ex[0::2])[None, :] * brick.abc[sel]
    assert np.isnan(xyz[~ok]).all()
    assert (np.abs(xyz[ok] - want[ok]) <= 32 * dp.EPS * np.abs(want[ok]).max()).all()
    pr.destroy()
    plan.destroy()


def test_no_points_is_a_no_op(gpu, brick):
    import torch
    plan, pr = brick.probe(gpu, np.arange(0))
    assert pr.n_points == 0 and pr.info()[0].size == 0
    out = torch.full((4,), 3.0, dtype=torch.float64, device=gpu)
    du = _t(brick.u, gpu)
    pr.eval(du, out)
    pr.eval_gradient(du, out)
    pr.lib.d4est_hip_probe_eval(pr.handle, 1, None, 0, None)   # the C entry itself returns before it looks at the pointers
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 3.0).all()
    pr.destroy()
    plan.destroy()


def test_run_to_run_bits(gpu, brick):
    import torch
    from disco4est_amd import capi
    sel = np.arange(brick.n_special + 200)
    n = len(sel)
    plan, pr = brick.probe(gpu, sel)
    pr.set_map(capi.GEOM_BRICK, EXTENTS)
    du = _t(brick.u, gpu)
    outs = []
    for _ in range(2):
        v = torch.zeros(3 * n, dtype=torch.float64, device=gpu)
        g = torch.zeros(3 * n, dtype=torch.float64, device=gpu)
        pr.eval(du, v, n_fields=3, field_stride=brick.stride)
        pr.eval_gradient(du, g, physical=True)
        torch.cuda.synchronize()
        outs.append((v.cpu().numpy(), g.cpu().numpy()))
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes()
    plan2, pr2 = brick.probe(gpu, sel)   # and a second locate gives the same points
    for a, b in zip(pr.info(), pr2.info()):
        assert a.tobytes() == b.tobytes()
    for o in (pr, pr2, plan, plan2):
        o.destroy()


def test_13_tree_sphere_with_compactified_outer_shell(gpu, hiplib):
    """level 0, p = 3: the drivers' points (two_punctures_cactus_13tree_with_opt_puncture_finder.c:960-975: the box points x = 0 and
    x = 3 of tree 12, the inner-wedge point r = 10 of tree 9, the outer-wedge point r = 100 of tree 3) and one point in every tree:
    value, xyz and the physical gradient of a smooth field interpolated to the nodes"""
    import torch
    from disco4est_amd import Plan, Probe, forest as F
    R0, R1, R2 = 6.0, 20.0, 1000.0
    mp = F.CubedSphere13Map(R0, R1, R2, compactify_outer=True)
    m = F.ForestMesh(F.cubed_sphere_13tree_connectivity(), 0, 3, mp)
    x, y, z = m.nodal_coords()
    r = np.sqrt(x * x + y * y + z * z)
    u = 1.0 / (1.0 + r / R0) + 0.01 * x / (1.0 + r) + 0.02 * np.sin(y / (1.0 + r))
    a = R0 / np.sqrt(3.0)
    # get_inverted_box_point(R0, x) = (x + a) / (2 a); get_inverted_inner_wedge_point(R0, R1, 10, 0): its closed form; the outer point solves
    # R(c) = m / (c - t) = 100 in closed form where the driver bisects
    inner = (2 * R0 ** 2 - 3 * R0 * R1 + R1 ** 2 - 10.0 ** 2 + np.sqrt(10.0 ** 2 * (R0 ** 2 - 4 * R0 * R1 + 3 * R1 ** 2 + 10.0 ** 2))) / (R0 - R1) ** 2 - 1
    mm, tt = 1.0 / (1.0 / R2 - 1.0 / R1), (R1 - 2.0 * R2) / (R1 - R2)
    outer = tt + mm / 100.0 - 1.0
    assert 0.0 < inner < 1.0 and 0.0 < outer < 1.0
    abc = [[(0.0 + a) / (2 * a), 0.5, 0.5], [(3.0 + a) / (2 * a), 0.5, 0.5], [0.5, 0.5, inner], [0.5, 0.5, outer]]
    tree = [12, 12, 9, 3]
    for t in range(13):
        tree.append(t)
        abc.append([0.31, 0.62, 0.45])
    tree, abc = np.array(tree, dtype=np.int32), np.array(abc)
    n = tree.size
    err, elem, rst = dp.locate(tree, abc, m.cells(), m.nf)
    assert (err == 0).all() and elem.tolist() == tree.tolist()
    deg, ns = m.deg[elem], m.nodal_stride[elem]
    val, S = dp.evaluate(u, ns, deg, rst)
    g_ref, gS = dp.gradient_ref(u, ns, deg, rst)
    dxdr = dp.dxdr_map(mp, tree, abc, m.size[elem], m.nf)
    assert (np.linalg.cond(dxdr, np.inf) <= (4 ** 3 + 6 * 4) / 8.0).all()   # the restatement's own inverse stays inside the bound
    gx, norm = dp.physical(g_ref, np.linalg.inv(dxdr))
    xyz_ref = np.stack([mp.x(int(t), abc[k:k + 1])[0] for k, t in enumerate(tree)])
    np.testing.assert_allclose(np.linalg.norm(xyz_ref[:4], axis=1), [0.0, 3.0, 10.0, 100.0], atol=1e-12)

    plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, 0)
    pr = Probe(plan, tree, abc, m.cells(), m.nf)
    pr.set_map(mp.GEOM_TYPE, mp.params)
    e2, el2, rst2 = pr.info()
    assert (e2 == 0).all() and el2.tolist() == elem.tolist()
    np.testing.assert_array_equal(rst2, rst)
    du = _t(u, gpu)
    out = torch.zeros(n, dtype=torch.float64, device=gpu)
    g = torch.zeros(3 * n, dtype=torch.float64, device=gpu)
    pr.eval(du, out)
    pr.eval_gradient(du, g, physical=True)
    torch.cuda.synchronize()
    got, gg = out.cpu().numpy(), g.cpu().numpy().reshape(3, n).T
    tol = dp.bound(deg, S)
    print("sphere values: max |device - restatement| / bound = %.3e" % np.max(np.abs(got - val) / tol))
    assert (np.abs(got - val) <= tol).all()
    gtol = dp.bound(deg, gS.max(axis=1)) * norm
    print("sphere physical gradient: max |device - restatement| / bound = %.3e" % np.max(np.abs(gg - gx) / gtol[:, None]))
    assert (np.abs(gg - gx) <= gtol[:, None]).all()
    xyz = pr.xyz()
    xtol = 32 * dp.EPS * np.maximum(np.abs(xyz_ref).max(axis=1), a)
    print("sphere xyz: max |device - restatement| / bound = %.3e" % np.max(np.abs(xyz - xyz_ref) / xtol[:, None]))
    assert (np.abs(xyz - xyz_ref) <= xtol[:, None]).all()
    pr.destroy()
    plan.destroy()
