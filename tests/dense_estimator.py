"""Independent DENSE evaluation of d4est's residual-based a-posteriori error estimator (d4est_estimator_bi_compute,
src/Estimators/d4est_estimator_bi.c) in numpy, in the style of tests/dense_sipg.py.  TEST INFRASTRUCTURE.

The traces are formed by the same explicit selection / prolongation / interpolation matrices as tests/dense_sipg.py (its tables and
helpers are imported, the file is not changed), and the terms follow the reference's formulas literally:
  term0  (h^2 / p^2) sum_q w J (V r)^2 at deg_quad                            d4est_estimator_bi.c:395-441, Mesh/d4est_mesh.c:2299-2370
  term1  Je1 = pi_grad sum_d n_d (dudx_m - dudx_p)_d;  sum_k w sj Je1^2          :150-340 (x 1/2 on the gradient of a half-size mortar's
                                                                                 big side: d4est_laplacian_flux.c:905-915)
  term2  Je2_d = pi_u n_d (u_m - u_p);  sum_d sum_k w sj Je2_d^2
  term3  Je2_d = pi_D n_d (u_m - g), g interpolated from the Lobatto face nodes; sum_d sum_k w sj Je2_d^2          :15-148
Prefactor degrees: the two elements of the mortar (:212-228); pi_D(p, h_m, p, h_m).  Inputs: the arrays mesh.* / forest.* produce."""
import numpy as np

from tests.dense_sipg import DenseLaplacian, face_select, kron3, lobatto, quad_interp_1d, quad_rule, reorient_matrix


def est_penalty(fid, deg_m, h_m, deg_p, h_p, c):
    """the ten penalty functions of d4est_estimator_bi.h by id (include/d4est_hip.h, D4EST_HIP_EST_*), vectorised over h"""
    h_m, h_p = np.asarray(h_m, dtype=float), np.asarray(h_p, dtype=float)
    max_p = float(max(deg_m, deg_p))
    min_h = np.minimum(h_m, h_p)
    max_h_over_p = np.maximum(h_m / deg_m, h_p / deg_p)
    max_p2_over_h = np.maximum(deg_m * deg_m / h_m, deg_p * deg_p / h_p)
    return {
        0: lambda: np.sqrt(min_h / max_p),
        1: lambda: np.sqrt(c * max_p * max_p / min_h),
        2: lambda: np.sqrt(max_h_over_p),
        3: lambda: np.sqrt(c * max_p2_over_h),
        4: lambda: np.sqrt(.5 * max_h_over_p),
        5: lambda: np.sqrt(.5 * c * max_p2_over_h),
        6: lambda: np.sqrt(c * max_p2_over_h),
        7: lambda: np.sqrt(.5 * min_h / max_p),
        8: lambda: np.sqrt(.5 * c * max_p * max_p / min_h),
        9: lambda: np.sqrt(c * max_p * max_p / min_h),
    }[int(fid)]()


class DenseEstimator(DenseLaplacian):
    def __init__(self, mesh, J, rst, sides, reorient_face_order, fcns=(7, 8, 9), penalty_prefactor=10.0):
        super().__init__(mesh, J, rst, sides, reorient_face_order)
        self.fcns, self.c = tuple(int(v) for v in fcns), float(penalty_prefactor)

    def residual_term(self, r, diam):
        m = self.m
        out = np.zeros(m.n_elements)
        for e in range(m.n_elements):
            p, pq = int(m.deg[e]), int(m.deg_quad[e])
            n, nq = p + 1, pq + 1
            V1 = quad_interp_1d(self.qt, p, pq)
            w = quad_rule(self.qt, pq)[1]
            s0, q0 = int(m.nodal_stride[e]), int(m.quad_stride[e])
            v = kron3(V1, V1, V1) @ r[s0:s0 + n ** 3]
            W = np.kron(w, np.kron(w, w))
            h = float(diam[e])
            out[e] = np.sum(W * self.J[q0:q0 + nq ** 3] * v * v) * (h * h / (p * p))
        return out

    def _mortar_est(self, e, f, ep, f_p, code, child_m, child_p, S, Ttot, off, off_p, u, u_ghost, half_m, half_p):
        deg_m, deg_p = self._deg(e), self._deg(ep)
        deg_mq = max(self._degq(e), self._degq(ep))
        nq = deg_mq + 1
        T = nq * nq
        sj, hm, hp, nrm, rm = self._geom(S, T, Ttot, off)
        rp = self._rp(S, T, Ttot, off_p)
        um, up = self._vals(e, u, u_ghost), self._vals(ep, u, u_ghost)
        Sm, Sp = face_select(f, deg_m + 1), face_select(f_p, deg_p + 1)
        Cm = self._side_to_mortar(deg_m, deg_mq, child_m)
        Gm, Gp = self._grad_ops(deg_m), self._grad_ops(deg_p)
        u_m = Cm @ (Sm @ um)
        dudx_m = [sum(rm[i][j] * (Cm @ (Sm @ (Gm[i] @ um))) for i in range(3)) for j in range(3)]
        u_p = self._side_to_mortar(deg_p, deg_mq, child_p[0]) @ (reorient_matrix(code, deg_p + 1) @ (Sp @ up))
        Cp_own = self._side_to_mortar(deg_p, deg_mq, child_p[1])
        Rq = reorient_matrix(code, nq)
        dudx_p = [Rq @ sum(rp[i][j] * (Cp_own @ (Sp @ (Gp[i] @ up))) for i in range(3)) for j in range(3)]
        if half_m:
            dudx_m = [0.5 * v for v in dudx_m]
        if half_p:
            dudx_p = [0.5 * v for v in dudx_p]
        w = quad_rule(self.qt, deg_mq)[1]
        W = np.kron(w, w)
        pg = est_penalty(self.fcns[0], deg_m, hm, deg_p, hp, self.c)
        pu = est_penalty(self.fcns[1], deg_m, hm, deg_p, hp, self.c)
        je1 = pg * sum(nrm[d] * (dudx_m[d] - dudx_p[d]) for d in range(3))
        t1 = np.sum(W * sj * je1 * je1)
        t2 = sum(np.sum(W * sj * (pu * nrm[d] * (u_m - u_p)) ** 2) for d in range(3))
        return t1, t2

    def _boundary_est(self, e, f, u, g):
        s = self.s
        sd = 6 * e + f
        deg, degq = self._deg(e), self._degq(e)
        nq = degq + 1
        T = nq * nq
        S = int(s["side_mortar_stride"][sd])
        sj, hm, _, nrm, _ = self._geom(S, T, T, 0)
        I = quad_interp_1d(self.qt, deg, degq)
        C = np.kron(I, I)
        u_m = C @ (face_select(f, deg + 1) @ self._vals(e, u, None))
        B0 = int(s["side_bndry_stride"][sd])
        gq = C @ g[B0:B0 + (deg + 1) ** 2] if g is not None else np.zeros(T)
        w = quad_rule(self.qt, degq)[1]
        W = np.kron(w, w)
        pd = est_penalty(self.fcns[2], deg, hm, deg, hm, self.c)
        return sum(np.sum(W * sj * (pd * nrm[d] * (u_m - gq)) ** 2) for d in range(3))

    def compute(self, u, r, diam, g=None, u_ghost=None):
        """(terms[4, n_elements], eta2[n_elements])"""
        m, s = self.m, self.s
        terms = np.zeros((4, m.n_elements))
        terms[0] = self.residual_term(r, diam)
        hang = s.get("side_hang")
        nodes2 = lambda a, b: (max(self._degq(a), self._degq(b)) + 1) ** 2
        for e in range(m.n_elements):
            for f in range(6):
                sd = 6 * e + f
                nbr, f_p, code = int(s["side_nbr"][sd]), int(s["side_nbr_face"][sd]), int(s["side_reorder"][sd])
                S = int(s["side_mortar_stride"][sd])
                h = 0 if hang is None else int(hang[sd])
                if nbr == -1:
                    terms[3, e] += self._boundary_est(e, f, u, g)
                    continue
                if h == 0:
                    T = nodes2(e, nbr)
                    parts = [self._mortar_est(e, f, nbr, f_p, code, None, (None, None), S, T, 0, 0, u, u_ghost, False, False)]
                elif h == 1:      # big side: its 4 sub-mortars, all added to e
                    o = int(s["side_orientation"][sd])
                    n4 = [int(v) for v in s["side_nbr4"][4 * sd:4 * sd + 4]]
                    Tm = [nodes2(e, n4[i]) for i in range(4)]
                    Tp = [0] * 4
                    for i in range(4):
                        Tp[self.rfo(f, f_p, o, i)] = Tm[i]
                    parts = []
                    for i in range(4):
                        j = self.rfo(f, f_p, o, i)
                        parts.append(self._mortar_est(e, f, n4[i], f_p, code, i, (None, None), S, sum(Tm), sum(Tm[:i]), sum(Tp[:j]), u,
                                                      u_ghost, True, False))
                else:             # small side: its own sub-mortar
                    o = int(s["side_orientation"][sd])
                    c = int(s["side_sub"][sd])
                    grp = [int(v) for v in s["side_nbr4"][4 * sd:4 * sd + 4]]
                    Tm = [nodes2(grp[i], nbr) for i in range(4)]
                    Tp = [0] * 4
                    for i in range(4):
                        Tp[self.rfo(f, f_p, o, i)] = Tm[i]
                    j = self.rfo(f, f_p, o, c)
                    parts = [self._mortar_est(e, f, nbr, f_p, code, None, (c, j), S, sum(Tm), sum(Tm[:c]), sum(Tp[:j]), u, u_ghost, False,
                                              True)]
                for t1, t2 in parts:
                    terms[1, e] += t1
                    terms[2, e] += t2
        eta2 = ((terms[0] + terms[1]) + terms[2]) + terms[3]
        return terms, eta2


def element_diameters(mesh, mapping=None):
    """a per-element size for the tests: the diagonal of the bounding box of the element's Lobatto nodes"""
    x = mesh.nodal_coords(mapping)
    out = np.zeros(mesh.n_elements)
    for e in range(mesh.n_elements):
        s0, n3 = int(mesh.nodal_stride[e]), (int(mesh.deg[e]) + 1) ** 3
        out[e] = np.sqrt(sum((c[s0:s0 + n3].max() - c[s0:s0 + n3].min()) ** 2 for c in x))
    return out


def nodal_polynomial(mesh, fn, mapping=None):
    """fn(x, y, z) at the Lobatto nodes, element-ordered"""
    x, y, z = mesh.nodal_coords(mapping)
    return fn(x, y, z)


__all__ = ["DenseEstimator", "est_penalty", "element_diameters", "nodal_polynomial", "lobatto"]
