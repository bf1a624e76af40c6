"""CPU tests of the 13-tree and holed cubed spheres: the two connectivity fixtures, continuity of the maps across every kind of tree
interface (with hanging faces), the chain-rule Jacobian -- forest.CubedSphere13Map / SphereWithHoleMap and the library's own C++ map
through d4est_hip_tree_map -- against a complex-step derivative of X restated here from the reference
(src/Geometry/d4est_geometry_cubed_sphere.c:316-403, :407-497), and the return codes of d4est_hip_tree_map.  No GPU."""
import json
import os

import numpy as np
import pytest

from disco4est_amd import forest as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
R_PLAIN = (1.0, 2.0, 6.0)
R_COMPACT = (1.0, 2.0, 20.0)      # compactified outer shell


# ---- X restated in complex numpy (shares no code with forest.py) ---------------------------------------------------
def _ref_radius(Ra, Rb, compactify, c):
    if compactify:
        m = (2.0 - 1.0) / ((1.0 / Rb) - (1.0 / Ra))
        t = (1.0 * Ra - 2.0 * Rb) / (Ra - Rb)
        return m / (c - t)
    return Ra * (2.0 - c) + Rb * (c - 1.0)


def _ref_X(gtype, R, c_outer, c_inner, tree, xi):
    """reference X of cubed_sphere (gtype 2; 4 is the same on trees < 12) and cubed_sphere_with_sphere_hole (3), xi complex [3]"""
    R0, R1, R2 = R
    if tree == 12:
        return (2.0 * xi - 1.0) * (R0 / np.sqrt(3.0))
    a, b, c = 2.0 * xi[0] - 1.0, 2.0 * xi[1] - 1.0, xi[2] + 1.0
    tx, ty = np.tan(a * np.pi / 4.0), np.tan(b * np.pi / 4.0)
    if tree < 6:
        x, y = tx, ty
        q = _ref_radius(R1, R2, c_outer, c) / np.sqrt(x * x + y * y + 1.0)
    elif gtype == 3:
        x, y = tx, ty
        q = _ref_radius(R0, R1, c_inner, c) / np.sqrt(x * x + y * y + 1.0)
    else:
        p = 2.0 - c
        x = p * a + (1.0 - p) * tx
        y = p * b + (1.0 - p) * ty
        q = (R0 * (2.0 - c) + R1 * (c - 1.0)) / np.sqrt(1.0 + (1.0 - p) * (tx * tx + ty * ty) + 2.0 * p)
    return np.array([[+q * x, -q, +q * y], [+q * x, +q * y, +q], [+q * x, +q, -q * y],
                     [+q, -q * x, -q * y], [-q * y, -q * x, -q], [-q, -q * x, +q * y]][tree % 6])


def _complex_step(gtype, R, c_outer, c_inner, tree, xi, h=1e-30):
    D = np.empty((3, 3))
    for k in range(3):
        z = xi.astype(np.complex128)
        z[k] += 1j * h
        D[:, k] = _ref_X(gtype, R, c_outer, c_inner, tree, z).imag / h
    return D


def _points(tree, n=20):
    """n seeded points of [0,1]^3, the first ones on corners, edges and faces of the tree"""
    xi = np.random.default_rng(1000 + tree).random((n, 3))
    xi[0] = (0, 0, 0); xi[1] = (1, 1, 1); xi[2] = (1, 0, 1); xi[3] = (0, 1, 0)
    xi[4, :2] = (0, 1); xi[5, 1:] = (1, 0)
    xi[6, 0] = 0; xi[7, 1] = 1; xi[8, 2] = 0; xi[9, 2] = 1
    return xi


def _maps():
    """(map, geom_type, radii) of every case: each type with both flags off and with each flag it supports on"""
    out = [(F.CubedSphere13Map(*R_PLAIN), 2, R_PLAIN), (F.CubedSphere13Map(*R_COMPACT, compactify_outer=True), 2, R_COMPACT),
           (F.SphereWithHoleMap(*R_PLAIN), 3, R_PLAIN), (F.SphereWithHoleMap(*R_COMPACT, compactify_outer=True), 3, R_COMPACT),
           (F.SphereWithHoleMap(*R_PLAIN, compactify_inner=True), 3, R_PLAIN),
           (F.SphereWithHoleMap(*R_PLAIN, cube_hole=True), 4, R_PLAIN),
           (F.SphereWithHoleMap(*R_COMPACT, compactify_outer=True, cube_hole=True), 4, R_COMPACT)]
    return out


# ---- 1. fixtures ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nt", [("cubed_sphere_13tree_connectivity", 13), ("sphere_with_hole_connectivity", 12)])
def test_fixture_is_a_consistent_connectivity(name, nt):
    """tree counts; every inter-tree face is pointed back at with the same orientation; the boundary faces are exactly face 5 of the
    outer wedges and, on the holed sphere, face 4 of the inner wedges"""
    with open(os.path.join(GOLDEN, name + ".json")) as fh:
        d = json.load(fh)
    assert d["num_trees"] == nt and len(d["tree_to_vertex"]) == 8 * nt and len(d["vertices"]) % 3 == 0
    assert set(d) == {"source", "num_trees", "vertices", "tree_to_vertex", "tree_to_tree", "tree_to_face"}
    conn = F.cubed_sphere_13tree_connectivity() if nt == 13 else F.sphere_with_hole_connectivity()
    assert conn.num_trees == nt
    boundary = set()
    for t in range(nt):
        for f in range(6):
            tp, c = int(conn.tree_to_tree[t, f]), int(conn.tree_to_face[t, f])
            if tp == t and c == f:
                boundary.add((t, f))
                continue
            fp, o = c % 6, c // 6
            assert 0 <= tp < nt and 0 <= o < 4
            assert int(conn.tree_to_tree[tp, fp]) == t and int(conn.tree_to_face[tp, fp]) == f + 6 * o
            assert F.reference_reorientation_is_consistent(f, fp, o)
    want = {(t, 5) for t in range(6)}
    if nt == 12:
        want |= {(t, 4) for t in range(6, 12)}
    assert boundary == want


# ---- 2. continuity -------------------------------------------------------------------------------------------------
def _refine(nt, cells):
    r = np.zeros(nt * 8, dtype=bool)
    for t, b in cells:
        r[8 * t + b] = True
    return r


def _hanging_tree_pairs(m, s):
    """kinds of tree interface crossed by a hanging face: 'ww' wedge-wedge in one shell, 'ss' shell-shell, 'wc' wedge-cube"""
    kinds = set()
    hang, nbr = np.asarray(s["side_hang"]).reshape(-1), np.asarray(s["side_nbr"]).reshape(-1)
    for sd in np.nonzero(hang == 2)[0]:
        ta, tb = int(m.tree[sd // 6]), int(m.tree[nbr[sd]])
        if ta == tb:
            continue
        lo, hi = min(ta, tb), max(ta, tb)
        kinds.add("wc" if hi == 12 else "ss" if (lo < 6 <= hi) else "ww")
    return kinds


@pytest.mark.parametrize("case", range(7))
def test_maps_are_continuous_across_tree_interfaces(case):
    """level 1, degree 2, one outer-wedge cell, one inner-wedge cell and (13 trees) one cube cell split: hanging faces cross
    wedge-wedge, shell-shell and wedge-cube interfaces; the two sides of every mortar see the same points (the 7-tree bounds)"""
    mp, gtype, _ = _maps()[case]
    nt = mp.num_trees
    conn = F.cubed_sphere_13tree_connectivity() if nt == 13 else F.sphere_with_hole_connectivity()
    cells = [(0, 0), (7, 4)] + ([(12, 7)] if nt == 13 else [])      # (tree, Morton cell): corners touching three tree faces each
    m = F.ForestMesh(conn, 1, 2, mp, refine=_refine(nt, cells))
    s = m.build_sides()
    assert s["mortar_xyz_mismatch"] <= 1e-12, s["mortar_xyz_mismatch"]
    assert s["hanging_order_mismatch"] == 0
    assert _hanging_tree_pairs(m, s) == ({"ww", "ss", "wc"} if nt == 13 else {"ww", "ss"})
    J, _ = m.geometry()
    assert J.min() > 0


# ---- 3. Jacobian against the complex step ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(7))
def test_jacobian_against_complex_step(hiplib, case):
    """Map.jacobian (numpy chain rule) and d4est_hip_tree_map (the C++ the kernels run, host side) against the complex-step derivative
    (h = 1e-30) of the restated reference X, 20 seeded points per tree with corners, edges and faces among them, bound
    2e-14 max(1, |D|max) -- the 7-tree test's.  Compactified outer shell at R2/R1 = 10 (R = (1, 2, 20)): 1/(c - t) loses about
    log2(R2/(R2-R1) R2/R1) = 3.5 bits at the outer boundary; the bound holds there with numpy alone, so R2 = 20 stays.  Measured
    worst error / bound, numpy and C++ together: 0.039 (plain cases), 0.037 (R2 = 20 compactified) -- printed by the test."""
    from disco4est_amd import capi
    mp, gtype, R = _maps()[case]
    worst = 0.0
    for t in range(mp.num_trees):
        xi = _points(t)
        D_py = mp.jacobian(t, xi)
        rc, X_c, D_c = capi.tree_map(gtype, mp.params, t, xi)
        assert rc == 0
        for k in range(xi.shape[0]):
            ref = _complex_step(gtype, R, mp.compactify_outer, mp.compactify_inner, t, xi[k])
            bound = 2e-14 * max(1.0, np.abs(ref).max())
            e_py, e_c = np.abs(D_py[k] - ref).max(), np.abs(D_c[k] - ref).max()
            worst = max(worst, e_py / bound, e_c / bound)
            assert e_py <= bound, ("numpy", t, xi[k], e_py, bound)
            assert e_c <= bound, ("C++", t, xi[k], e_c, bound)
    print("case %d worst error / bound = %.3f" % (case, worst))


# ---- 4. host map against the Python map -----------------------------------------------------------------------------
def test_host_map_matches_python_map(hiplib):
    """x of d4est_hip_tree_map == Map.x within 1e-14 R2 (and against the restated reference X), all four types"""
    from disco4est_amd import capi
    cases = [(m, g, m.params, R[2], m.num_trees) for m, g, R in _maps()]
    for comp in (False, True):
        m7 = F.CubedSphere7Map(1.0, 2.0, comp)
        cases.append((m7, 1, (1.0, 2.0, float(comp)), 2.0, 7))
    for mp, gtype, params, R2, nt in cases:
        for t in range(nt):
            xi = _points(t)
            rc, X_c, D_c = capi.tree_map(gtype, params, t, xi)
            assert rc == 0
            assert np.abs(X_c - mp.x(t, xi)).max() <= 1e-14 * R2
            assert np.abs(D_c - mp.jacobian(t, xi)).max() <= 2e-14 * max(1.0, np.abs(D_c).max())
            if gtype != 1:
                ref = np.array([_ref_X(gtype, (mp.R0, mp.R1, mp.R2), mp.compactify_outer, mp.compactify_inner, t, x.astype(np.complex128)).real
                                for x in xi])
                assert np.abs(X_c - ref).max() <= 1e-14 * R2


# ---- 5. return codes ------------------------------------------------------------------------------------------------
def test_tree_map_return_codes(hiplib):
    from disco4est_amd import capi
    xi = np.array([[0.25, 0.5, 0.75]])
    ok = (1.0, 2.0, 6.0, 0.0, 0.0)
    for gtype in (0, 5, -1):
        assert capi.tree_map(gtype, ok, 0, xi)[0] != 0
    assert capi.tree_map(2, ok, 12, xi)[0] == 0 and capi.tree_map(2, ok, 13, xi)[0] != 0
    assert capi.tree_map(4, ok, 11, xi)[0] == 0 and capi.tree_map(4, ok, 12, xi)[0] != 0
    assert capi.tree_map(3, ok, 11, xi)[0] == 0 and capi.tree_map(3, ok, 12, xi)[0] != 0
    assert capi.tree_map(1, (1.0, 2.0, 0.0), 6, xi)[0] == 0 and capi.tree_map(1, (1.0, 2.0, 0.0), 7, xi)[0] != 0
    assert capi.tree_map(2, ok, -1, xi)[0] != 0
    inner = (1.0, 2.0, 6.0, 0.0, 1.0)
    assert capi.tree_map(2, inner, 0, xi)[0] != 0 and capi.tree_map(4, inner, 0, xi)[0] != 0
    assert capi.tree_map(3, inner, 0, xi)[0] == 0
    assert capi.tree_map(2, (2.0, 1.0, 6.0, 0.0, 0.0), 0, xi)[0] != 0      # radii out of order
