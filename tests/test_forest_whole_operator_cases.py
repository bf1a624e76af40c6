"""The case lists of tests/test_forest_whole_operator_gpu.py are not vacuous: the side tables of their meshes, built on the CPU, hold every
reorder code 0..7, every neighbour face 0..5, all nine (d, dn) pairs of own / neighbour face direction and both face ends where the
GPU module says so, orientations 0..3 on the hanging list, and the clean elements the hybrid forms' guards count on.  (The side tables
do not depend on the degree: degree 1 here.)"""
import numpy as np
import pytest

from disco4est_amd import forest as F, mesh as M
from tests import forest_whole_operator_cases as C

ALL_CODES, ALL_FACES = set(range(8)), set(range(6))
ALL_PAIRS = {(d, dn) for d in range(3) for dn in range(3)}


def _mesh(rots, level=0, deg=1, **kw):
    conn = F.Connectivity.rotated_pair(*rots)
    return F.ForestMesh(conn, level, deg, F.TrilinearMap(conn), **kw)


def test_the_lists_are_not_empty():
    for name in ("ALL", "FIFTH", "TENTH", "LEVEL1", "CHEBY", "GHOST", "MIXED", "HANGING"):
        assert len(getattr(C, name)) > 0, name
    assert len(C.ALL) == 144 and C.FIFTH == C.SORTED[::5]
    assert C.TENTH[:15] == C.SORTED[::10] and len(C.TENTH) < len(C.FIFTH)      # every 10th, and the few triples that complete the codes
    assert {deg for deg, _, _ in C.SINGLE_WAVE} == {1, 3, 7} and {deg for deg, _, _ in C.MULTI_WAVE} == {8, 11, 15}
    assert [(deg + 1, deg + inc + 1) for deg, inc, _ in C.SINGLE_WAVE if inc] == [(4, 6)]     # one of D4EST_HIP_DIRECT_PAIRS with NQ > N


@pytest.mark.parametrize("name", ["ALL", "FIFTH", "TENTH"])
def test_kind1_lists_cover_every_code_face_and_direction_pair(hiplib, name):
    """level 0, two elements, both views of the glued face: the two interior sides of each mesh"""
    total = {}
    for trip, rots in getattr(C, name):
        m = _mesh(rots)
        s = m.build_sides()
        sides = C.interior_sides(m, s)
        assert len(sides) == 2 and sides == C.tree_face_sides(m, s)
        assert {sd % 6 for sd, _ in sides} == {trip[0], trip[1]} or trip[0] == trip[1]
        assert {int(s["side_reorder"][sd]) for sd, _ in sides} == {C.code_of(trip)}
        C.merge(total, C.coverage(m, s, sides))
    assert total["codes"] == ALL_CODES and total["f_p"] == ALL_FACES and total["d_dn"] == ALL_PAIRS
    assert total["h"] == {0, 1} and total["h_p"] == {0, 1}


def test_level1_list_has_oriented_and_code0_sides_in_every_mesh(hiplib):
    total = {}
    for trip, rots in C.LEVEL1:
        m = _mesh(rots, level=1)
        s = m.build_sides()
        assert m.n_elements == 16
        face = C.tree_face_sides(m, s)
        inside = [x for x in C.interior_sides(m, s) if x not in face]
        assert len(face) == 8 and len(inside) == 48
        assert {int(s["side_reorder"][sd]) for sd, _ in face} == {C.code_of(trip)}
        assert {int(s["side_reorder"][sd]) for sd, _ in inside} == {0}
        C.merge(total, C.coverage(m, s, face))
    assert total["codes"] == ALL_CODES and total["f_p"] == ALL_FACES


def test_cheby_list_has_the_codes_the_cubed_sphere_lacks(hiplib):
    codes = set()
    for trip, rots in C.CHEBY:
        m = _mesh(rots, level=1)
        s = m.build_sides()
        codes |= C.coverage(m, s, C.tree_face_sides(m, s))["codes"]
    assert codes == {4, 5, 6}


def test_ghost_list_covers_every_code_and_face_on_ghost_sides(hiplib):
    """one tree per rank: every ghost side lies on the tree face, seen from tree 0 the re-orientation is geometric"""
    codes, faces = set(), set()
    for trip, rots in C.GHOST:
        assert C.geometric(trip)
        for first in (0, 8):
            m = _mesh(rots, level=1, first=first, count=8)
            s = m.build_sides()
            ghost = np.nonzero(s["side_nbr"] <= -2)[0]
            assert ghost.size == 4 and len(s["ghost_global_ids"]) == 4
            codes |= {int(c) for c in s["side_reorder"][ghost]}
            faces |= {int(f) for f in s["side_nbr_face"][ghost]}
    assert codes == ALL_CODES and faces == ALL_FACES


def test_mixed_list_has_clean_owners_of_oriented_lower_degree_sides(hiplib):
    codes = set()
    for k, (trip, rots) in enumerate(C.MIXED):
        conn = F.Connectivity.rotated_pair(*rots)
        m = F.ForestMesh(conn, 1, C.level1_degrees(conn.num_trees, k % 2, 5), F.TrilinearMap(conn))
        s = m.build_sides()
        got = C.mixed_aware_tree_face_codes(m, s)
        assert got == {C.code_of(trip)}, (trip, got)
        clean = C.clean_without_higher_neighbour(m, s)
        assert 0 < sum(clean) < m.n_elements
        # degrees differ across the tree face and inside either tree
        assert all(len({int(m.deg[e]) for e in range(16) if m.tree[e] == t}) == 2 for t in range(2))
        codes |= got
    assert codes == ALL_CODES


def test_hanging_list_covers_the_orientations_on_either_side(hiplib):
    seen = {(r, g): set() for r in range(2) for g in (False, True)}
    for trip, rots in C.HANGING:
        for r, refine in enumerate(C.HANGING_REFINES):
            m = _mesh(rots, refine=refine)
            s = m.build_sides()
            assert m.n_elements == 9 and (s["side_hang"] == 1).sum() == 1 and (s["side_hang"] == 2).sum() == 4
            assert int(s["side_orientation"].max()) == trip[2]
            seen[(r, C.geometric(C.hanging_small_view(trip, refine)))].add(trip[2])
            for big_higher in (False, True):
                deg = C.hanging_degrees(s, m.n_elements, 4, big_higher)
                assert sorted(set(deg)) == ([3, 4, 5] if big_higher else [3, 4]) and deg.count(4) == (4 if big_higher else 5)
    # where the reference's re-orientation is geometric -- the small sides can take the kind-2 override -- every orientation occurs with the
    # refined tree on either side; the non-geometric views (one degree only in the GPU module) occur too
    assert seen[(0, True)] == seen[(1, True)] == {0, 1, 2, 3}
    assert seen[(0, False)] | seen[(1, False)]
