"""CPU pins of tests/dense_sizes.py, the numpy restatement of the reference's element size parameters and mortar h
(src/Mesh/d4est_mesh.c:1620-1827, :3400-3468, :689-856) that the GPU tests of csrc/d4est_hip_sizes.hip compare against."""
import numpy as np
import pytest

from disco4est_amd import capi, forest as F
from tests import dense_sizes as DS


@pytest.mark.parametrize("volume_h_type", [0, 1])
def test_anisotropic_brick_cell(hiplib, volume_h_type):
    """widths (a, b, c): the all-pairs / quadrature path on the cell's own Lobatto nodes gives the closed form"""
    a = np.array([1.0, 2.0, 0.5]) / 4
    p = 4
    t = capi.table("lobatto_nodes", p)
    X = 0.5 * a[None, :] * (DS.tensor_ref(t) + 1.0) + np.array([0.25, 0.5, 0.0])[None, :]
    dxdr_at = lambda ref: np.broadcast_to(np.diag(0.5 * a), (ref.shape[0], 3, 3))
    e = DS._element(dxdr_at, X, p, volume_h_type)
    cf = DS.size_parameters_brick([1], 4, (0, 1, 0, 2, 0, 0.5), volume_h_type=volume_h_type)
    assert abs(e["volume"] - a.prod()) <= 1e-14 * a.prod()
    diam = np.sqrt((a * a).sum()) / (np.sqrt(3.) if volume_h_type else 1.0)
    assert abs(e["diam_volume"] - diam) <= 1e-14 * diam
    for f in range(6):
        o = [i for i in range(3) if i != f // 2]
        assert abs(e["area"][f] - a[o[0]] * a[o[1]]) <= 1e-14
        assert abs(e["diam_face"][f] - np.hypot(a[o[0]], a[o[1]])) <= 1e-14
        for k in ("j_div_sj_min", "j_div_sj_mean", "j_div_sj_max"):
            assert abs(e[k][f] - 0.5 * a[f // 2]) <= 1e-15
    for k in DS.PER_ELEMENT:
        assert abs(cf[k][0] - e[k]) <= 1e-14
    for k in DS.PER_FACE:
        assert np.abs(cf[k] - e[k]).max() <= 1e-14


def test_sphere_volume_and_area_converge(hiplib):
    """13-tree sphere, outer shell not compactified: the volumes of trees 0 ... 5 sum to 4 pi (R2^3 - R1^3) / 3 and the areas of their
    outer faces (face 5: xi_2 = 1) to 4 pi R2^2, the error falling monotonically over p = 3, 7, 11 and below 1e-8 at p = 11"""
    R0, R1, R2 = 1.0, 2.0, 6.0
    mp = F.CubedSphere13Map(R0, R1, R2)
    ev, ea = [], []
    for p in (3, 7, 11):
        sp = DS.size_parameters_analytic(2, mp.params, np.arange(6), np.zeros((6, 3), dtype=int), np.full(6, 2), 2.0, np.full(6, p))
        ev.append(abs(sp["volume"].sum() - 4 * np.pi * (R2 ** 3 - R1 ** 3) / 3) / (4 * np.pi * (R2 ** 3 - R1 ** 3) / 3))
        ea.append(abs(sp["area"][5::6].sum() - 4 * np.pi * R2 ** 2) / (4 * np.pi * R2 ** 2))
    print("volume errors", ev, "area errors", ea)
    assert ev[0] > ev[1] > ev[2] and ea[0] > ea[1] > ea[2]
    assert ev[2] < 1e-8 and ea[2] < 1e-8


def _fake_params(n):
    """distinct numbers per (array, element, face)"""
    sp = {"volume": 100.0 + np.arange(n), "diam_volume": 200.0 + np.arange(n)}
    for i, k in enumerate(DS.PER_FACE):
        sp[k] = 1000.0 * (i + 1) + np.arange(6 * n)
    return sp


@pytest.mark.parametrize("name", sorted(DS.FACE_H, key=DS.FACE_H.get))
def test_calculate_mortar_h_on_a_hanging_pair(hiplib, name):
    """big element 0 (face 1) against small elements 1 ... 4 (face 0): which element's parameter lands on which of the four mortar
    faces, for the side of one and the side of four, for all eight types"""
    ht = DS.FACE_H[name]
    sp = _fake_params(5)
    tree_h = np.array([0.5, 0.25, 0.25, 0.25, 0.25])
    quad = ["q0", "q1", "q2", "q3"]
    big = DS.calculate_mortar_h(ht, [0], 1, 4, sp, tree_h, quad)
    small = DS.calculate_mortar_h(ht, [1, 2, 3, 4], 0, 4, sp, tree_h, quad)
    per_face = {"FACE_H_EQ_J_DIV_SJ_MIN_LOBATTO": "j_div_sj_min", "FACE_H_EQ_J_DIV_SJ_MEAN_LOBATTO": "j_div_sj_mean",
                "FACE_H_EQ_J_DIV_SJ_MAX_LOBATTO": "j_div_sj_max", "FACE_H_EQ_FACE_DIAM": "diam_face"}
    if name == "FACE_H_EQ_J_DIV_SJ_QUAD":
        assert big is quad and small is quad
    elif name == "FACE_H_EQ_TREE_H":
        assert big == [0.5] * 4 and small == [0.25] * 4
    elif name in per_face:
        k = per_face[name]
        assert big == [sp[k][6 * 0 + 1]] * 4                        # the big element's own parameter on all four
        assert small == [sp[k][6 * e + 0] for e in (1, 2, 3, 4)]    # each small element's own
    elif name == "FACE_H_EQ_VOLUME_DIV_AREA":
        assert big == [sp["volume"][0] / sp["area"][1]] * 4
        assert small == [sp["volume"][e] / sp["area"][6 * e] for e in (1, 2, 3, 4)]
    else:
        assert big == [sp["volume"][0] / sp["area"][1]] * 4
        assert small == [sp["volume"][1:5].sum() / sp["area"][[6, 12, 18, 24]].sum()] * 4


def test_mortar_h_arrays_layout_on_a_hanging_brick(hiplib):
    """the hm / hp arrays on a locally refined brick: every mortar face constant, the big side's block carries its own parameter in hm
    and the four small elements' in hp, a small side the reverse"""
    from disco4est_amd import mesh as M
    refine = np.zeros(8, dtype=bool)
    refine[0] = True
    m = M.HangingBrickMesh(1, refine, 2)
    s = m.build_sides()
    n = m.n_elements
    sp = _fake_params(n)
    tree_h = m.size / 4.0
    hm, hp = DS.mortar_h_arrays(m, s, sp, tree_h, DS.FACE_H["FACE_H_EQ_J_DIV_SJ_MIN_LOBATTO"])
    T = 9
    seen = 0
    for sd in range(6 * n):
        e, f = divmod(sd, 6)
        S = int(s["side_mortar_stride"][sd])
        if s["side_hang"][sd] == 1:
            for i in range(4):
                ep = int(s["side_nbr4"][4 * sd + i])
                assert (hm[S + i * T:S + (i + 1) * T] == sp["j_div_sj_min"][6 * e + f]).all()
                assert (hp[S + i * T:S + (i + 1) * T] == sp["j_div_sj_min"][6 * ep + (f ^ 1)]).all()
            seen += 1
        elif s["side_hang"][sd] == 2:
            i, big = int(s["side_sub"][sd]), int(s["side_nbr"][sd])
            assert (hm[S + i * T:S + (i + 1) * T] == sp["j_div_sj_min"][6 * e + f]).all()
            assert (hp[S + i * T:S + (i + 1) * T] == sp["j_div_sj_min"][6 * big + (f ^ 1)]).all()
            seen += 1
    assert seen == 3 + 12
    hm4, _ = DS.mortar_h_arrays(m, s, sp, tree_h, DS.FACE_H["FACE_H_EQ_TREE_H"])
    assert set(np.unique(hm4)) == {0.25, 0.5}
