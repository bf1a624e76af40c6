"""CPU pins of tests/dense_transfer.py (the independent dense statement of the inter-grid transfers, long double inside) to the oracle's
restatement of d4est_operators_apply_p_prolong / _hp_prolong, their transposes and apply_p_restrict / _hp_restrict, and of its Galerkin term
to the oracle's dense element blocks.  The GPU sweep (tests/test_transfer_sweep_gpu.py) then compares the kernels with the dense reference.

Tolerance 1e-13, every element relative to its own largest entry: both sides apply the same three 1-D operators of at most 20 columns;
the oracle works in double with operators from an inverted Vandermonde matrix, the dense reference in long double from the node tables."""
import ctypes

import numpy as np
import pytest

from tests import dense_transfer as DT

RTOL = 1e-13
dp = ctypes.POINTER(ctypes.c_double)
ip = ctypes.POINTER(ctypes.c_int)

# (dH, children's offsets dh - dH): the pairs dH in {1, 7, 15} x offsets 0 .. 3 and 18 -> 19, as p-items, as hp-items whose eight children
# all have that pair (they differ by position: eight different operators on a random input), and mixed hp-items
_PAIRS = [(dH, off) for dH in (1, 2, 7, 15) for off in (0, 1, 2, 3)] + [(18, 0), (18, 1)]
_MIXED = [(dH, [0, 1, 2, 3, 3, 2, 1, 0][r:] + [0, 1, 2, 3, 3, 2, 1, 0][:r]) for dH, r in ((1, 0), (7, 3), (15, 5))] + [(18, [0, 1, 1, 0, 1, 0, 0, 1])]


def _item_list():
    hrefine, degH, degh = [], [], []
    for dH, off in _PAIRS:
        hrefine += [0, 1]
        degH += [dH, dH]
        degh += [dH + off] + [0] * 7 + [dH + off] * 8
    for dH, offs in _MIXED:
        hrefine.append(1)
        degH.append(dH)
        degh += [dH + o for o in offs]
    return np.array(hrefine, np.int32), np.array(degH, np.int32), np.array(degh, np.int32)


def _oracle_walk(oracle, hrefine, degH, degh, x, kind):
    """the item loop of the reference's callbacks with the oracle's element functions; kind: prolong / transpose / restrict"""
    lib = oracle.lib
    lib.oracle_apply_p_prolong.argtypes = [dp, ctypes.c_int, ctypes.c_int, ctypes.c_int, dp]
    lib.oracle_apply_hp_prolong.argtypes = [dp, ctypes.c_int, ctypes.c_int, ip, dp]
    for name in ("prolong_transpose", "restrict"):
        getattr(lib, "oracle_apply_p_" + name).argtypes = [dp, ctypes.c_int, ctypes.c_int, ctypes.c_int, dp]
        getattr(lib, "oracle_apply_hp_" + name).argtypes = [dp, ip, ctypes.c_int, ctypes.c_int, dp]
    d = DT.DenseTransfer(hrefine, degH, degh)
    out = np.zeros(d.fine_nodes if kind == "prolong" else d.coarse_nodes)
    fe = 0
    for k in range(len(hrefine)):
        dH, nc = int(degH[k]), (8 if hrefine[k] else 1)
        dh = np.ascontiguousarray(degh[8 * k:8 * k + 8], dtype=np.int32)
        c0, c1 = int(d.coarse_bounds[k]), int(d.coarse_bounds[k + 1])
        f0, f1 = int(d.fine_bounds[fe]), int(d.fine_bounds[fe + nc])
        fe += nc
        if kind == "prolong":
            src, dst = np.ascontiguousarray(x[c0:c1]), np.zeros(f1 - f0)
            if nc == 1:
                lib.oracle_apply_p_prolong(src.ctypes.data_as(dp), dH, 3, int(dh[0]), dst.ctypes.data_as(dp))
            else:
                lib.oracle_apply_hp_prolong(src.ctypes.data_as(dp), dH, 3, dh.ctypes.data_as(ip), dst.ctypes.data_as(dp))
            out[f0:f1] = dst
        else:
            name = "prolong_transpose" if kind == "transpose" else "restrict"
            src, dst = np.ascontiguousarray(x[f0:f1]), np.zeros(c1 - c0)
            if nc == 1:
                getattr(lib, "oracle_apply_p_" + name)(src.ctypes.data_as(dp), int(dh[0]), 3, dH, dst.ctypes.data_as(dp))
            else:
                getattr(lib, "oracle_apply_hp_" + name)(src.ctypes.data_as(dp), dh.ctypes.data_as(ip), 3, dH, dst.ctypes.data_as(dp))
            out[c0:c1] = dst
    return out


@pytest.fixture(scope="module")
def pinned(oracle):
    from disco4est_amd import mesh as M
    hrefine, degH, degh = _item_list()
    d = DT.DenseTransfer(hrefine, degH, degh)
    xc = M.splitmix64_uniform(41, d.coarse_nodes) - 0.5
    xf = M.splitmix64_uniform(43, d.fine_nodes) - 0.5
    return d, xc, xf, {k: _oracle_walk(oracle, hrefine, degH, degh, (xc if k == "prolong" else xf), k) for k in ("prolong", "transpose", "restrict")}


def test_item_grid_is_the_one_asked_for():
    pairs = set(_PAIRS)
    for dH in (1, 7, 15):
        for off in range(4):
            assert (dH, off) in pairs
    assert (18, 1) in pairs


def test_prolong_matches_oracle(pinned):
    d, xc, xf, ref = pinned
    err = DT.elementwise_rel_err(d.prolong(xc), ref["prolong"], d.fine_bounds)
    print("dense prolong vs oracle, worst element: %.3e" % err)
    assert err <= RTOL


def test_prolong_transpose_matches_oracle(pinned):
    d, xc, xf, ref = pinned
    err = DT.elementwise_rel_err(d.restrict(xf), ref["transpose"], d.coarse_bounds)
    print("dense restrict (sum P^T) vs oracle, worst element: %.3e" % err)
    assert err <= RTOL


def test_projection_matches_oracle(pinned):
    d, xc, xf, ref = pinned
    err = DT.elementwise_rel_err(d.project(xf), ref["restrict"], d.coarse_bounds)
    print("dense L2 projection vs oracle, worst element: %.3e" % err)
    assert err <= RTOL


def test_all_eight_children_differ(pinned):
    """an hp-item whose eight children have ONE degree: eight different operators -- no two children's prolongations agree, and handing
    child c the operator of any other child c' moves the result far outside the tolerance"""
    d, xc, xf, ref = pinned
    got = d.prolong(xc)
    for k, (dH, off) in enumerate(_PAIRS):
        e0 = 9 * k + 1                                      # items alternate p, hp: fine elements 9 k (p) and 9 k + 1 .. 9 k + 8
        blocks = [got[d.fine_bounds[e0 + c]:d.fine_bounds[e0 + c + 1]] for c in range(8)]
        for a in range(8):
            for b in range(a + 1, 8):
                assert np.abs(blocks[a] - blocks[b]).max() > 1e-3 * np.abs(blocks[a]).max(), (dH, off, a, b)


def test_identities():
    """partition of unity, exactness on the coarse space (project o prolong = 1) and adjointness, in the dense reference itself"""
    from disco4est_amd import mesh as M
    hrefine, degH, degh = _item_list()
    d = DT.DenseTransfer(hrefine, degH, degh)
    assert np.abs(d.prolong(np.ones(d.coarse_nodes)) - 1.0).max() <= 1e-15
    xc = M.splitmix64_uniform(47, d.coarse_nodes) - 0.5
    xf = M.splitmix64_uniform(49, d.fine_nodes) - 0.5
    assert np.abs(d.project(d.prolong(xc)) - xc).max() <= 1e-13
    a, b = np.dot(d.prolong(xc), xf), np.dot(xc, d.restrict(xf))
    assert abs(a - b) <= 1e-13 * max(abs(a), abs(b))


def test_batched_application_is_fast():
    """65537 p-items and 8193 hp-items (the list-size cases of the GPU sweep) in well under a second each"""
    import time
    for hrefine, degH, degh in ((np.zeros(65537, np.int32), np.ones(65537, np.int32), np.tile([1, 0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0], 32769)[:8 * 65537]),
                                (np.ones(8193, np.int32), np.full(8193, 2, np.int32), np.tile([2, 3, 4, 2, 3, 4, 4, 3], 8193))):
        d = DT.DenseTransfer(hrefine, degH, degh.astype(np.int32))
        xf = np.linspace(-1.0, 1.0, d.fine_nodes)
        t0 = time.perf_counter()
        d.restrict(xf)
        assert time.perf_counter() - t0 < 1.0


@pytest.mark.parametrize("quad_type", [0, 1])
@pytest.mark.parametrize("hp", [False, True])
def test_galerkin_term_matches_oracle_blocks(hiplib, oracle, hp, quad_type):
    """the dense Galerkin term of one coarse element against the oracle's route: dense fine blocks V^T W J c V (mg_matrix_setup),
    restricted as sum_c P_c^T M_c P_c (mg_matrix_restriction), applied as a block.  1e-12 of the term's largest entry: the oracle's
    dense products are dot products of up to 125 double terms of one sign pattern (about 125 eps = 1.4e-14 each, three of them chained)."""
    from disco4est_amd import mesh as M
    mp = M.SineMap(0.04)
    if hp:
        degf = np.array([2, 3, 2, 4, 3, 2, 4, 3], np.int32)
        mf = M.BrickMesh(1, degf, deg_quad_inc=1, quad_type=quad_type)
        hrefine, dH, degh = np.array([1], np.int32), 2, degf
    else:
        mf = M.BrickMesh(0, 4, deg_quad_inc=2, quad_type=quad_type)
        hrefine, dH, degh = np.array([0], np.int32), 2, np.array([4, 0, 0, 0, 0, 0, 0, 0], np.int32)
    J, _ = mf.geometry(mp)
    coeff = 0.5 + 2.0 * M.splitmix64_uniform(17, mf.local_nodes_quad)
    fine = oracle.mg_matrix_setup(mf, J, coeff)
    n3 = (dH + 1) ** 3
    block = oracle.mg_matrix_restriction(hrefine, np.array([dH], np.int32), degh, fine).reshape(n3, n3)
    uH = M.splitmix64_uniform(19, n3) - 0.5
    ref = block @ uH
    jc = [(J * coeff)[mf.quad_stride[e]:mf.quad_stride[e] + (mf.deg_quad[e] + 1) ** 3] for e in range(mf.n_elements)]
    got = DT.galerkin_term(quad_type, hp, dH, [int(p) for p in mf.deg], [int(q) for q in mf.deg_quad], jc, uH)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print("dense Galerkin term vs oracle blocks: %.3e" % err)
    assert err <= 1e-12
