"""CPU pins of tests/dense_probe.py, the numpy restatement the device point probes are held to (tests/test_probe_gpu.py): identities that
need no device, each within the bound of the issue, (N^3 + 6 N) eps S per point with S the sum of the absolute values of the terms."""
import numpy as np

from disco4est_amd import forest as F, mesh as M, table
from tests import dense_probe as dp

DEGS = np.array([1, 2, 3, 4, 7, 8, 19, 1, 2, 3, 4, 7, 8, 19, 5], dtype=np.int32)


def _hanging_brick():
    refine = np.zeros(8, dtype=bool)
    refine[7] = True
    return M.HangingBrickMesh(1, refine, DEGS)


def _random_points(n, seed):
    return M.splitmix64_uniform(seed, 3 * n).reshape(n, 3)


def test_locate_takes_the_first_element_in_traversal_order(hiplib):
    m = _hanging_brick()
    pts = np.array([[0.5, 0.25, 0.25], [0.5, 0.5, 0.25], [0.5, 0.5, 0.5], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0.75, 0.75, 0.6], [1.5, 0.5, 0.5]])
    tree = np.array([0, 0, 0, 0, 0, 0, 0])
    err, elem, rst = dp.locate(tree, pts, m.cells(), m.root_len)
    assert err.tolist() == [0, 0, 0, 0, 0, 0, 1]
    assert elem.tolist() == [0, 0, 0, 0, 14, 7, -1]   # (0.75, 0.75, 0.6): on the edge between four children of the refined octant, the first is 7
    np.testing.assert_array_equal(rst[0], [1.0, 0.0, 0.0])
    np.testing.assert_array_equal(rst[2], [1.0, 1.0, 1.0])
    np.testing.assert_array_equal(rst[4], [1.0, 1.0, 1.0])
    assert np.isnan(rst[6]).all()
    err, elem, _ = dp.locate([1], [[0.5, 0.5, 0.5]], m.cells(), m.root_len)
    assert err[0] == 1 and elem[0] == -1


def test_polynomials_of_the_element_degree_are_reproduced(hiplib):
    """u = (x y z)^p on an element of degree p (discontinuous between elements: every point sees its own element only)"""
    m = _hanging_brick()
    x, y, z = m.nodal_coords()
    pw = np.repeat(m.deg, (m.deg.astype(np.int64) + 1) ** 3).astype(np.float64)
    u = (x * y * z) ** pw
    abc = _random_points(200, 11)
    err, elem, rst = dp.locate(np.zeros(200, dtype=int), abc, m.cells(), m.root_len)
    assert (err == 0).all() and set(m.deg[elem]) == set(DEGS)
    val, S = dp.evaluate(u, m.nodal_stride[elem], m.deg[elem], rst)
    want = (abc[:, 0] * abc[:, 1] * abc[:, 2]) ** m.deg[elem]
    assert (np.abs(val - want) <= dp.bound(m.deg[elem], S)).all(), np.max(np.abs(val - want) / dp.bound(m.deg[elem], S))


def test_the_value_at_a_lobatto_node_is_the_nodal_value_exactly(hiplib):
    for p in (1, 2, 3, 4, 7, 8, 19):
        N = p + 1
        u = M.splitmix64_uniform(5 + p, N ** 3) - 0.5
        lgl = table("lobatto_nodes", p)
        idx = np.array([[0, 0, 0], [p, p, p], [p // 2, 0, p], [1, p - 1, p // 2]])
        rst = lgl[idx]
        val, _ = dp.evaluate(u, np.zeros(4, dtype=int), np.full(4, p), rst)
        np.testing.assert_array_equal(val, u[(idx[:, 2] * N + idx[:, 1]) * N + idx[:, 0]])


def test_reference_gradient_of_monomials(hiplib):
    for p, (a, b, c) in ((1, (1, 1, 0)), (2, (2, 1, 2)), (3, (3, 0, 2)), (4, (4, 4, 4)), (7, (7, 3, 5)), (8, (2, 8, 6)), (19, (19, 17, 11))):
        lgl = table("lobatto_nodes", p)
        t = F.ForestMesh._tensor_ref(lgl)
        u = t[:, 0] ** a * t[:, 1] ** b * t[:, 2] ** c
        rst = 2.0 * _random_points(25, 100 + p) - 1.0
        r, s, tt = rst[:, 0], rst[:, 1], rst[:, 2]
        g, S = dp.gradient_ref(u, np.zeros(25, dtype=int), np.full(25, p), rst)
        want = np.stack([a * r ** max(a - 1, 0) * s ** b * tt ** c, b * r ** a * s ** max(b - 1, 0) * tt ** c,
                         c * r ** a * s ** b * tt ** max(c - 1, 0)], axis=1)
        tol = dp.bound(np.full(25, p), S.max(axis=1))
        assert (np.abs(g - want) <= tol[:, None]).all(), (p, np.max(np.abs(g - want) / tol[:, None]))


def test_physical_gradient_of_r_squared_on_the_13_tree_sphere(hiplib):
    """x^2 + y^2 + z^2 is a polynomial of degree 2 in the element's rst on the centre cube (affine map) and on the outer wedges without
    compactification (R(c)^2 with R linear in c), so p = 3 holds it exactly and its physical gradient is 2 (x, y, z) to rounding"""
    mp = F.CubedSphere13Map(1.0, 2.0, 3.0, compactify_outer=False)
    m = F.ForestMesh(F.cubed_sphere_13tree_connectivity(), 1, 3, mp)
    u = m.field(noise=0.0)
    trees = np.array([0, 1, 2, 3, 4, 5, 12, 12, 12])
    abc = _random_points(trees.size, 77)
    err, elem, rst = dp.locate(trees, abc, m.cells(), m.nf)
    assert (err == 0).all()
    g_ref, S = dp.gradient_ref(u, m.nodal_stride[elem], m.deg[elem], rst)
    dxdr = dp.dxdr_map(mp, trees, abc, m.size[elem], m.nf)
    assert (np.linalg.cond(dxdr, np.inf) <= 11.0).all()   # (N^3 + 6 N) / 8 at N = 4: eight roundings of a well-conditioned 3 x 3 inverse fit the bound
    g, norm = dp.physical(g_ref, np.linalg.inv(dxdr))
    xyz = np.stack([mp.x(int(t), abc[k:k + 1])[0] for k, t in enumerate(trees)])
    tol = dp.bound(m.deg[elem], S.max(axis=1)) * norm
    assert (np.abs(g - 2.0 * xyz) <= tol[:, None]).all(), np.max(np.abs(g - 2.0 * xyz) / tol[:, None])
    # and the brick's inverse Jacobian is the diagonal one
    R = dp.drdx_brick((0., 2., 0., 1., -1., 3.), np.array([1, 2]), 4)
    np.testing.assert_allclose(R[:, [0, 1, 2], [0, 1, 2]], [[4.0, 8.0, 2.0], [2.0, 4.0, 1.0]], rtol=1e-15)
