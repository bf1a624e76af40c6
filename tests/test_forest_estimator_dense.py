"""Closed-form pins of the dense estimator and the dense energy norm (tests/dense_estimator.py: _mortar_est, tests/dense_norms.py:
_mortar_norm) on faces BETWEEN trees, which tests/test_forest_estimator_gpu.py holds the device kernels to: two affine trees glued
through the (f_m, f_p, orientation) triples of tests/forest_whole_operator_cases.py.  A continuous quadratic has no jump wherever the
reference's re-orientation is the geometric one -- and a visible one on the 36 triples where it is not (forest.
reference_reorientation_is_consistent: the dense forms follow the reference there, as the engine does); a piecewise-constant field has
the value jump of known size on all 144 triples.  And the case lists of the GPU module are not vacuous: every one covers the eight
reorder codes and the six neighbour faces."""
import numpy as np
import pytest

from disco4est_amd import forest as F
from tests import dense_estimator as DE, dense_norms as DN
from tests import forest_estimator_cases as E, forest_whole_operator_cases as C
from tests.test_estimator_dense import _rfo

ALL_CODES, ALL_FACES = set(range(8)), set(range(6))
ZERO, VISIBLE = 1e-13, 1e-6      # of terms[0].max(): the bound of test_estimator_dense.py::test_continuous_field_has_no_jump_terms, and
#                                  what a non-geometric pairing of the nodes must exceed

# the quadratic of tests/test_estimator_dense.py: unequal coefficients, so no flip or transpose of the face maps it to itself
QUADRATIC = lambda x, y, z: 1.0 + x * y - 0.5 * z * z + 0.3 * x


def _affine(rots, level=0, deg=1, **kw):
    conn = F.Connectivity.rotated_pair(*rots)
    return F.ForestMesh(conn, level, deg, F.TrilinearMap(conn), **kw)


def _jumps(m):
    """(term 1, term 2, the energy norm's interface term) per element over terms[0].max(), of the interpolated quadratic"""
    J, rst = m.geometry()
    s = m.build_sides()
    u = DE.nodal_polynomial(m, QUADRATIC)
    bx = s["bndry_xyz"]
    terms, _ = DE.DenseEstimator(m, J, rst, s, _rfo(), (7, 8, 9), 10.0).compute(u, u, DE.element_diameters(m), g=QUADRATIC(bx[0], bx[1], bx[2]))
    eterms, _ = DN.DenseNorms(m, J, rst, s, _rfo(), 0, 10.0).energy(u)
    scale = terms[0].max()
    assert scale > 1e-6 and np.abs(terms[3]).max() <= ZERO * scale
    return np.stack([terms[1], terms[2], eterms[2]]) / scale


@pytest.mark.parametrize("deg", [2, 3])
def test_continuous_field_conforming(hiplib, deg):
    """level 0, all 144 triples, p = 2 and 3 with deg_quad = deg + 1: each element's jump terms vanish where ITS view of the face is
    geometric and are visible where it is not -- so a triple has no jump at all exactly when C.geometric_both holds"""
    n_other = 0
    for trip, rots in C.ALL:
        j = _jumps(_affine(rots, 0, deg, deg_quad_inc=1))
        assert j.shape == (3, 2)
        if C.geometric_both(trip):
            assert np.abs(j).max() <= ZERO, (trip, j)
            continue
        n_other += 1
        assert np.abs(j).max() > VISIBLE, (trip, j)
        for tree in range(2):
            if E.view_geometric(trip, tree):
                assert np.abs(j[:, tree]).max() <= ZERO, (trip, tree, j)
            else:
                assert j[:, tree].min() > VISIBLE, (trip, tree, j)      # all three of them
    assert n_other == 36


@pytest.mark.parametrize("refine", C.HANGING_REFINES, ids=["tree0-refined", "tree1-refined"])
def test_continuous_field_hanging(hiplib, refine):
    """the hanging face ON the tree boundary (off_p, the sub-face permutation, the 1/2 on the big side's gradient), either tree refined"""
    n_other = 0
    for trip, rots in C.HANGING:
        m = _affine(rots, 0, 2, deg_quad_inc=1, refine=refine)
        assert m.n_elements == 9
        j = _jumps(m)
        if C.geometric_both(trip):
            assert np.abs(j).max() <= ZERO, (trip, j)
        else:
            n_other += 1
            assert np.abs(j).max() > VISIBLE, (trip, j)
    assert 0 < n_other < len(C.HANGING)


def test_piecewise_constant_field(hiplib):
    """u = c_e on the element e, p = 3, all 144 triples: no gradient jump, and across the one interior face (a unit square)
    term 2 = pi_u^2 (c_e - c_n)^2 area with pi_u^2 = c p^2 / (2 h) (houston_u_prefactor_maxp_minh, id 8); the energy norm's interface
    term is 3 pen (c_e - c_n)^2 area with pen = c p^2 / h (SIPG id 0, added once per direction)"""
    pref, p, area = 10.0, 3, 1.0
    c_e = np.array([1.0, 1.37])
    for trip, rots in C.ALL:
        m = _affine(rots, 0, p)
        J, rst = m.geometry()
        s = m.build_sides()
        u = np.repeat(c_e, (p + 1) ** 3)
        terms, _ = DE.DenseEstimator(m, J, rst, s, _rfo(), (7, 8, 9), pref).compute(u, u, DE.element_diameters(m), g=None)
        eterms, _ = DN.DenseNorms(m, J, rst, s, _rfo(), 0, pref).energy(u)
        expect, expect_norm = np.zeros(2), np.zeros(2)
        sides = C.interior_sides(m, s)
        assert len(sides) == 2
        for sd, nbr in sides:
            h = s["hm"][int(s["side_mortar_stride"][sd])]
            assert abs(h - 0.5) <= 1e-14            # h = J / sj of a unit cube as the image of [-1, 1]^3: (1 / 8) / (1 / 4)
            expect[sd // 6] += .5 * pref * p * p / h * (c_e[sd // 6] - c_e[nbr]) ** 2 * area
            expect_norm[sd // 6] += 3.0 * pref * p * p / h * (c_e[sd // 6] - c_e[nbr]) ** 2 * area
        assert np.abs(terms[1]).max() <= 1e-13 * np.abs(terms[2]).max(), trip
        assert np.abs(terms[2] - expect).max() <= 1e-13 * np.abs(expect).max(), trip
        assert np.abs(eterms[2] - expect_norm).max() <= 1e-13 * np.abs(expect_norm).max(), trip


# ---- what the level-0 face can and cannot show ---------------------------------------------------------------------------------------------------
def _drst_p_change_under_the_code(rots, warp, nq=4):
    """largest change of the (+) side's dr/dx block on the glued face (tree 0's side) when it is re-ordered with the face's code, over its
    largest entry"""
    conn = F.Connectivity.rotated_pair(*rots)
    m = F.ForestMesh(conn, 0, nq - 1, F.TrilinearMap(conn, warp))
    s = m.build_sides()
    sd, _ = C.tree_face_sides(m, s)[0]
    S, T, code = int(s["side_mortar_stride"][sd]), nq * nq, int(s["side_reorder"][sd])
    blk = np.asarray(s["drst_p"])[9 * S:9 * S + 9 * T].reshape(9, T)
    return max(np.abs(F.ForestMesh.reorient(b, code, nq) - b).max() for b in blk) / np.abs(blk).max()


def test_the_sine_map_is_symmetric_on_the_level0_face(hiplib):
    """why tests/forest_estimator_cases.py has the ASYMMETRIC families: under mesh.SineMap the mortar factors of the face between two
    level-0 trees are the same in all eight orders, under SkewSineMap every code but 0 moves them"""
    from disco4est_amd import mesh as M
    codes = set()
    for trip, rots in C.FIFTH:
        assert _drst_p_change_under_the_code(rots, M.SineMap(0.03)) <= 1e-12, trip
        change = _drst_p_change_under_the_code(rots, E.SkewSineMap(0.03))
        if C.code_of(trip) == 0:
            assert change == 0.0
        else:
            codes.add(C.code_of(trip))
            assert change > 1e-3, (trip, change)
    assert codes == ALL_CODES - {0}


def test_skew_sine_map_jacobian_is_the_derivative_of_its_x():
    """complex-step derivative of SkewSineMap.x against SkewSineMap.jacobian, and the map stays invertible on the two trees"""
    w = E.SkewSineMap(0.03)
    X, Y, Z = (a.ravel() for a in np.meshgrid(np.linspace(0, 2, 9), np.linspace(0, 1, 5), np.linspace(0, 1, 5), indexing="ij"))
    DF = w.jacobian(X, Y, Z)
    h = 1e-30
    for j, p in enumerate(([X + 1j * h, Y, Z], [X, Y + 1j * h, Z], [X, Y, Z + 1j * h])):
        col = np.stack([np.imag(v) / h for v in w.x(*p)], axis=-1)
        assert np.abs(col - DF[:, :, j]).max() <= 1e-15
    assert np.linalg.det(DF).min() > 0.8 and np.abs(DF - np.eye(3)).max() < 0.12


# ---- the lists of tests/test_forest_estimator_gpu.py ------------------------------------------------------------------------------------------
def test_the_families_name_lists_that_exist():
    assert {name for _, _, name, _ in E.CONFORMING + E.ASYMMETRIC} | {"LEVEL1", "HANGING", "GHOST"} == set(E.LISTS_USED)
    assert all(entry[:2] in [c[:2] for c in E.CONFORMING] for entry in E.ASYMMETRIC)      # degrees of CONFORMING, on another warp
    assert all(len(getattr(C, name)) > 0 for name in E.LISTS_USED)
    degs = [d for d, _, _, _ in E.CONFORMING]
    assert [2, 3] in degs and [3, 2] in degs and any(np.isscalar(d) and d >= 8 for d in degs)
    assert any(inc > 0 for _, inc, _, _ in E.CONFORMING)


@pytest.mark.parametrize("name", ["ALL", "FIFTH"])
def test_level0_lists_cover_every_code_and_face(hiplib, name):
    total = {}
    for trip, rots in getattr(C, name):
        m = _affine(rots)
        s = m.build_sides()
        face = C.tree_face_sides(m, s)
        assert len(face) == 2 and {int(s["side_reorder"][sd]) for sd, _ in face} == {C.code_of(trip)}
        C.merge(total, C.coverage(m, s, face))
    assert total["codes"] == ALL_CODES and total["f_p"] == ALL_FACES


def test_level1_list_covers_every_code_and_face(hiplib):
    total = {}
    for trip, rots in C.LEVEL1:
        m = _affine(rots, level=1)
        s = m.build_sides()
        face = C.tree_face_sides(m, s)
        assert m.n_elements == 16 and len(face) == 8 and {int(s["side_reorder"][sd]) for sd, _ in face} == {C.code_of(trip)}
        assert any(int(s["side_reorder"][sd]) == 0 for sd, n in C.interior_sides(m, s) if (sd, n) not in face)
        C.merge(total, C.coverage(m, s, face))
    assert total["codes"] == ALL_CODES and total["f_p"] == ALL_FACES


@pytest.mark.parametrize("refine", C.HANGING_REFINES, ids=["tree0-refined", "tree1-refined"])
def test_hanging_list_covers_every_code_face_and_orientation(hiplib, refine):
    """with either tree refined: the big side and the four small sides carry the triple's code, between them every code, every
    neighbour face and the orientations 0..3 occur; mixed degrees (the small sides' view geometric) and one degree both occur"""
    total, seen_o, layouts = {}, set(), set()
    for trip, rots in C.HANGING:
        m = _affine(rots, refine=refine)
        s = m.build_sides()
        face = C.tree_face_sides(m, s)
        assert (s["side_hang"] == 1).sum() == 1 and (s["side_hang"] == 2).sum() == 4 and len(face) == 5
        assert {int(s["side_hang"][sd]) for sd, _ in face} == {1, 2}
        assert {int(s["side_reorder"][sd]) for sd, _ in face} == {C.code_of(trip)}
        assert int(s["side_orientation"].max()) == trip[2]
        seen_o.add(trip[2])
        layouts.add(len(set(E.hanging_degrees(trip, refine, m.n_elements).tolist())))
        C.merge(total, C.coverage(m, s, face))
    assert total["codes"] == ALL_CODES and total["f_p"] == ALL_FACES and seen_o == {0, 1, 2, 3}
    assert layouts == {1, 3}


def test_ghost_list_covers_every_code_and_face_on_ghost_sides(hiplib):
    total = {}
    for trip, rots in C.GHOST:
        for first, count in E.GHOST_PARTS:
            m = _affine(rots, level=1, first=first, count=count)
            s = m.build_sides()
            ghost = E.ghost_sides(s)
            assert len(ghost) == 4 and {int(s["side_reorder"][sd]) for sd, _ in ghost} == {C.code_of(trip)}
            C.merge(total, C.coverage(m, s, ghost))
    assert total["codes"] == ALL_CODES and total["f_p"] == ALL_FACES
