"""CPU: (1) the dense long-double forms of tests/dense_mgmatrix.py pinned to the oracle's restatement of the reference's matrix operator
on the hierarchies of tests/test_mgmatrix_gpu.py and on a p = 1 brick; (2) proof that the case lists of tests/mgmatrix_cases.py reach
every launch shape of the five kernels of csrc/d4est_hip_mgmatrix.hip.  If (2) goes red after a change of the library's rules for
cutting rows or columns into workgroups: restate the rule in dense_mgmatrix.py and RE-PICK THE CASES so that every shape is reached."""
import numpy as np
import pytest

from disco4est_amd import mesh as M
from tests import dense_mgmatrix as D
from tests import mgmatrix_cases as C
from tests.mgmatrix_cases import RTOL, hierarchy as _hierarchy


def _p1_hierarchy():
    m1, m0 = M.BrickMesh(1, 1, deg_quad_inc=1), M.BrickMesh(0, 1, deg_quad_inc=1)
    return [m1, m0], [(np.ones(1, np.int32), np.ones(1, np.int32), np.ones(8, np.int32))]


@pytest.mark.parametrize("kind", ["hp3", "hanging2", "p1"])
def test_dense_forms_are_the_oracles(oracle, kind):
    mp = M.SineMap(0.04)
    meshes, items = _p1_hierarchy() if kind == "p1" else _hierarchy(kind)
    mf = meshes[0]
    Jf, _ = mf.geometry(mp)
    coeff = 0.5 + 2.0 * M.splitmix64_uniform(17, mf.local_nodes_quad)
    for c in (coeff, None):
        ref = oracle.mg_matrix_setup(mf, Jf, c)
        got = D.mass_blocks(mf, Jf, c)
        assert np.abs(got - ref).max() <= RTOL * np.abs(ref).max()
    blocks = [oracle.mg_matrix_setup(mf, Jf, coeff)]
    for lvl, (h, dH, dh) in enumerate(items):
        for literal in (False, True):
            ref = oracle.mg_matrix_restriction(h, dH, dh, blocks[-1], literal_window=literal)
            got = D.restrict_blocks(h, dH, dh, blocks[-1], literal_window=literal)
            assert np.abs(got - ref).max() <= RTOL * np.abs(ref).max(), (lvl, literal)
        blocks.append(oracle.mg_matrix_restriction(h, dH, dh, blocks[-1]))
    for lvl, m in enumerate(meshes):
        if m.n_elements < 8 or type(m) is not M.BrickMesh:
            continue                                   # (the operator needs faces: the whole bricks)
        J, rst = m.geometry(mp)
        sides = m.build_sides(mp)
        oracle.set_operator(m, J, rst, sides, 10.0, 0, threads=4)
        oracle.set_lhs_coefficient(None)
        oracle.set_lhs_element_blocks(blocks[lvl])
        u = m.field(mp)
        lhs = oracle.apply_lhs(u)
        oracle.set_lhs_element_blocks(None)
        term = lhs - oracle.apply_aij(m, J, rst, sides, u)
        got = D.block_term(m, blocks[lvl], u)
        assert np.abs(got - term).max() <= RTOL * np.abs(lhs).max(), lvl


def test_block_offset_forms():
    """explicit offsets: the reversed and the shared layout read the blocks they say"""
    m = M.BrickMesh(1, np.array([1, 2, 1, 2, 2, 1, 1, 2], np.int32))
    u = M.splitmix64_uniform(3, m.local_nodes) - 0.5
    per = [M.splitmix64_uniform(10 + e, (int(m.deg[e]) + 1) ** 6) - 0.5 for e in range(8)]
    ref = np.concatenate([per[e].reshape((int(m.deg[e]) + 1) ** 3, -1) @ u[m.nodal_stride[e]:m.nodal_stride[e] + (int(m.deg[e]) + 1) ** 3]
                          for e in range(8)])
    assert np.abs(D.block_term(m, np.concatenate(per), u) - ref).max() <= 1e-15
    off, n = C.block_layout(m.deg, "reversed")
    assert n == sum(p.size for p in per)
    assert np.abs(D.block_term(m, np.concatenate(per[::-1]), u, off) - ref).max() <= 1e-15
    m3 = M.BrickMesh(1, 1)
    off, n = C.block_layout(m3.deg, "shared")
    assert n == 4 * 64 and off.tolist() == [0, 0, 64, 64, 128, 128, 192, 192]


def test_sliced_product_is_the_long_double_product():
    """the large literal-window products go through exact float64 slice products: the same numbers as numpy's long-double matmul"""
    A = ((M.splitmix64_uniform(5, 90 * 300) - 0.5) * np.exp(8.0 * M.splitmix64_uniform(6, 90 * 300))).reshape(90, 300).astype(D.LD)
    B = ((M.splitmix64_uniform(7, 300 * 70) - 0.5) * np.exp(8.0 * M.splitmix64_uniform(8, 300 * 70))).reshape(300, 70).astype(D.LD)
    A, B = A * (1 + D.LD(2) ** -60), B * (1 - D.LD(2) ** -58)        # (mantissas beyond float64)
    ref = np.matmul(A, B)
    scale = np.abs(A).max(axis=1)[:, None] * np.abs(B).max(axis=0)[None, :]
    assert float((np.abs(D._sliced_matmul(A, B) - ref) / scale).max()) <= 300 * 2.0 ** -63


# ---- the case lists reach every launch shape -------------------------------------------------------------------------------------
def _matvec_shapes():
    out = []
    for name, level, deg, layout in C.MATVEC_CASES:
        for p, n_elem in C.buckets(level, deg):
            N3 = (p + 1) ** 3
            rows = D.rows_per_wg(n_elem, N3)
            out.append((name, N3, rows, D.last_chunk_rows(N3, rows)))
    return out


def test_matvec_cases_reach_every_row_split():
    shapes = _matvec_shapes()
    assert {rows for _, _, rows, _ in shapes} == {8, 16, 32, 64}, "re-pick the cases: " + repr(shapes)
    for want in (16, 32, 64):
        # several trips in the last chunk, and in its last trip a wavefront without a second row
        assert any(rows == want and last > 8 and D.second_row_missing(last) for _, _, rows, last in shapes), \
            "re-pick the cases: no ragged multi-trip last chunk at rows = %d in %r" % (want, shapes)
    assert any(rows == 8 and D.second_row_missing(last) for _, _, rows, last in shapes), "re-pick the cases: " + repr(shapes)
    assert any(N3 < 64 for _, N3, _, _ in shapes), "re-pick the cases: " + repr(shapes)
    assert any(N3 < rows for _, N3, rows, _ in shapes), "re-pick the cases: " + repr(shapes)
    assert sum(len(C.buckets(level, deg)) > 1 for _, level, deg, _ in C.MATVEC_CASES) >= 1
    assert {layout for _, _, _, layout in C.MATVEC_CASES} == {"consecutive", "reversed", "shared"}
    # the starting points of the list, as the host rule sees them
    by_name = {name: rows for name, _, rows, _ in shapes}
    assert (by_name["l4-p1"], by_name["l4-p2"], by_name["l3-p4"], by_name["l3-p6"]) == (64, 64, 16, 32)


def test_mass_cases_reach_every_column_split():
    shapes = []
    for level, deg, inc in C.MASS_CASES:
        for p, n_elem in C.buckets(level, deg):
            N3 = (p + 1) ** 3
            cols, chunks = D.mass_cols_per_wg(n_elem, N3)
            shapes.append((level, p, inc, N3, cols, chunks))
    assert any(cols == 1 for *_, cols, _ in shapes), "re-pick the cases: " + repr(shapes)
    assert any(cols > 1 and chunks > 1 and N3 % cols != 0 for _, _, _, N3, cols, chunks in shapes), "re-pick the cases: no ragged last chunk"
    assert any(cols > 1 and chunks > 1 and N3 % cols == 0 for _, _, _, N3, cols, chunks in shapes), "re-pick the cases: no full last chunk"
    assert any(chunks == 1 and cols == N3 for _, _, _, N3, cols, chunks in shapes), "re-pick the cases: no single chunk"
    assert {inc for _, _, inc in C.MASS_CASES} == {0, 1, 2, 3}
    assert {p for lv, p, _ in C.MASS_CASES if lv == 1} == {1, 2, 3, 5, 6, 7, 8, 9, 11}


def test_galerkin_cases_reach_every_split():
    seen_small_child = seen_cols = seen_rows = False
    for name in C.GALERKIN_CASES:
        n_items, n_children, n3, nh3 = C.galerkin_shape(name)
        rows, _ = D.galerkin_split(n_children, n3)
        cols, chunks = D.galerkin_split(n_items, n3)
        # a child smaller than the transfer's max_n^3 by more than one chunk of rows: whole workgroups of the rows kernel with nothing to do
        seen_small_child |= any(n3 - k > rows for k in nh3)
        seen_cols |= cols > 1 and chunks > 1 and n3 % cols != 0
        seen_rows |= rows > 1
    assert seen_small_child and seen_cols and seen_rows, "re-pick the cases"
    _, n_children, n3, nh3 = C.galerkin_shape("h-p2-with-copied-p8")
    assert n3 == 729 and min(nh3) == 27
    assert D.galerkin_split(512, 27)[0] > 1          # 512 items at p = 2: more than one column per workgroup
    assert D.galerkin_split(64, 27)[0] == 1          # (64 items, a level-3 fine brick, would still get one column each)
    # every case keeps the sum over the children in the LDS; the other branch (max_n >= 19) is not reached (profiles/mgmatrix_tests.md)
    assert all(D.galerkin_acc_in_lds(C.galerkin_shape(name)[2]) for name in C.GALERKIN_CASES), "re-pick the cases"
