"""Pins of tests/dense_norms.py (the numpy restatement of the error norms of d4est_norms_save that the device norms are held to) by
values that can be computed by hand on BrickMesh(1, p): 8 elements of side 1/2 in the unit cube, 12 interior faces, 24 boundary
faces of area 1/4."""
import numpy as np
import pytest

from disco4est_amd import mesh as M
from tests import dense_norms as DN
from tests.dense_sipg import quad_rule


def _norms(m, mp=None, fcn=0, pref=10.0):
    from disco4est_amd import capi
    lib = capi.load_library()
    J, rst = m.geometry(mp)
    sides = m.build_sides(mp)
    return DN.DenseNorms(m, J, rst, sides, lambda a, b, c, d: int(lib.d4est_hip_reorient_face_order(a, b, c, d)), fcn, pref), J, sides


def _volume(m, J):
    tot = 0.0
    for e in range(m.n_elements):
        pq = int(m.deg_quad[e])
        w = quad_rule(m.quad_type, pq)[1]
        q0 = int(m.quad_stride[e])
        tot += np.sum(np.kron(w, np.kron(w, w)) * J[q0:q0 + (pq + 1) ** 3])
    return tot


@pytest.mark.parametrize("p,curved", [(2, False), (3, True)])
def test_l2_of_one_is_the_volume(hiplib, p, curved):
    m = M.BrickMesh(1, p, deg_quad_inc=1)
    mp = M.SineMap(0.05) if curved else None
    dn, J, _ = _norms(m, mp)
    arr, tot = dn.l2_sqr(np.ones(m.local_nodes))
    vol = _volume(m, J)
    assert abs(tot - vol) <= 1e-13 * vol
    if not curved:
        assert abs(tot - 1.0) <= 1e-13 and np.abs(arr - 0.125).max() <= 1e-14


@pytest.mark.parametrize("p", [1, 3])
def test_energy_of_x_on_the_affine_brick(hiplib, p):
    """u = x: |grad u|^2 = 1, so the volume term is the volume; u is continuous, so the interface term vanishes; the boundary term
    is sum over the boundary faces of pen int x^2: the face x = 1 gives 1, the four faces y, z = 0, 1 give 1/3 each, x = 0 nothing;
    pen = c p^2 / h with the mortar's h (penalty id 0)"""
    m = M.BrickMesh(1, p)
    pref = 7.0
    dn, J, sides = _norms(m, None, 0, pref)
    u = m.nodal_coords()[0].copy()
    terms, sums = dn.energy(u)
    assert abs(sums[0] - 1.0) <= 1e-12
    assert abs(sums[2]) <= 1e-24 * max(1.0, sums[1])
    h = float(sides["hm"][0])
    assert np.ptp(sides["hm"]) == 0.0
    pen = pref * p * p / h
    assert abs(sums[1] - pen * (1.0 + 4.0 / 3.0)) <= 1e-12 * sums[1]
    assert sums[3] == (sums[0] + sums[1]) + sums[2]


def test_interface_term_of_a_jump(hiplib):
    """piecewise constants with a jump across the plane x = 1/2: each of the 4 interior faces in that plane gives, from each of its
    two sides, 3 pen jump^2 area; the other 8 interior faces give nothing.  The penalty enters once: the term is linear in it"""
    p, jump = 2, 0.75
    m = M.BrickMesh(1, p)
    u = np.zeros(m.local_nodes)
    for e in range(m.n_elements):
        if m.ijk[e][0] == 1:
            s0 = int(m.nodal_stride[e])
            u[s0:s0 + (p + 1) ** 3] = jump
    res = []
    for pref in (3.0, 12.0):
        dn, J, sides = _norms(m, None, 0, pref)
        h = float(sides["hm"][0])
        terms, sums = dn.energy(u)
        pen = pref * p * p / h
        assert abs(sums[2] - 4 * 3 * 2 * pen * jump ** 2 * 0.25) <= 1e-12 * sums[2]
        assert np.abs(terms[2] - 3 * pen * jump ** 2 * 0.25).max() <= 1e-12 * terms[2].max()   # one such face per element
        assert abs(sums[0]) <= 1e-20
        res.append(sums[2])
    assert abs(res[1] / res[0] - 4.0) <= 1e-13     # 12 / 3, not its square


def test_linfty_of_negative_values_is_zero(hiplib):
    m = M.BrickMesh(1, 2)
    dn, _, _ = _norms(m)
    assert dn.linfty(-1.0 - np.arange(m.local_nodes, dtype=float)) == 0.0
    v = -np.ones(m.local_nodes); v[40] = 0.5; v[3] = -7.0
    assert dn.linfty(v) == 0.5
    skip = np.zeros(m.n_elements, dtype=np.int32); skip[40 // 27] = 1
    assert dn.linfty(v, skip) == 0.0


def test_l2_array_is_filled_for_skipped_elements(hiplib):
    m = M.BrickMesh(1, 2, deg_quad_inc=1)
    dn, _, _ = _norms(m, M.SineMap(0.05))
    v = m.field()
    skip = np.array([0, 1, 0, 0, 1, 1, 0, 0], dtype=np.int32)
    arr, tot = dn.l2_sqr(v, skip)
    arr0, tot0 = dn.l2_sqr(v)
    assert np.array_equal(arr, arr0) and arr.min() > 0
    assert abs(tot - arr[skip == 0].sum()) <= 1e-15 * tot and tot < tot0
    assert DN.masked_sum(arr, skip) == tot
    assert np.array_equal(DN.error_field(v, 2 * v), np.abs(v))
