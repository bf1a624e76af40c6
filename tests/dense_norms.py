"""Independent DENSE evaluation of the error norms of d4est_norms_save (src/IO/d4est_norms.c) in numpy, in the style of
tests/dense_estimator.py, whose traces, geometry access and side walk it reuses.  TEST INFRASTRUCTURE.

The terms follow the reference's formulas literally:
  error      |u - u_compare| at the Lobatto nodes                                                       d4est_norms.c:467-468
  L2         per element sum_q w J (V v_e)^2 at deg_quad; the sum leaves out skipped elements          Mesh/d4est_mesh.c:2299-2374
  Linfty     running maximum of the VALUES, starting at 0, over the non-skipped elements               d4est_norms.c:64-117
  energy     volume:    sum_d sum_q w J (sum_i rst_xyz[i][d] V (D_i u))^2                                dGMath/d4est_gradient.c:12-124
             interface: ip[k] = sum_d (n_d u_m - n_d u_p)^2, then sum_k w sj pen ip ADDED ONCE PER DIRECTION d (x 3)
                                                                                                        dGMath/d4est_ip_energy_norm.c:210-270
             boundary:  ip[k] = sum_d (n_d u_m)^2, sum_k w sj pen(deg, h, deg, h) ip, once              :70-102
             pen = u_penalty_fcn (a penalty_calc_t of d4est_laplacian_flux_sipg.c:945-1005), NOT squared; degrees as at :216-218
             total = (volume + boundary) + interface                                                    :440-443
Every local side adds to its own element (a face is visited from both of its sides)."""
import numpy as np

from tests.dense_estimator import DenseEstimator
from tests.dense_sipg import diff_matrix, face_select, kron3, lobatto, penalty, quad_interp_1d, quad_rule, reorient_matrix


def error_field(u, u_compare=None):
    return np.abs(u if u_compare is None else u - u_compare)


class DenseNorms(DenseEstimator):
    def __init__(self, mesh, J, rst, sides, reorient_face_order, penalty_fcn=0, penalty_prefactor=10.0):
        super().__init__(mesh, J, rst, sides, reorient_face_order, penalty_prefactor=penalty_prefactor)
        self.pfcn = int(penalty_fcn)

    # ---- L2 / Linfty
    def l2_array(self, v):
        """v_e^T M_e v_e of every element: the estimator's residual term without h^2 / p^2"""
        m = self.m
        return self.residual_term(v, np.asarray(m.deg, dtype=float))   # (h = p: the factor h^2 / p^2 is exactly 1)

    def l2_sqr(self, v, skip=None):
        arr = self.l2_array(v)
        keep = np.ones(self.m.n_elements, dtype=bool) if skip is None else (np.asarray(skip) == 0)
        return arr, float(np.sum(arr[keep]))

    def linfty(self, v, skip=None):
        m = self.m
        out = 0.0
        for e in range(m.n_elements):
            if skip is not None and skip[e]:
                continue
            s0, n3 = int(m.nodal_stride[e]), (int(m.deg[e]) + 1) ** 3
            for x in v[s0:s0 + n3]:
                if x > out:
                    out = float(x)
        return out

    # ---- IP energy norm
    def volume_term(self, u):
        m = self.m
        out = np.zeros(m.n_elements)
        for e in range(m.n_elements):
            p, pq = int(m.deg[e]), int(m.deg_quad[e])
            n, nq = p + 1, pq + 1
            D = diff_matrix(lobatto(p)[0])
            I = np.eye(n)
            Dl = [kron3(I, I, D), kron3(I, D, I), kron3(D, I, I)]
            V1 = quad_interp_1d(self.qt, p, pq)
            V = kron3(V1, V1, V1)
            w = quad_rule(self.qt, pq)[1]
            W = np.kron(w, np.kron(w, w))
            s0, q0 = int(m.nodal_stride[e]), int(m.quad_stride[e])
            ue = u[s0:s0 + n ** 3]
            Jq = self.J[q0:q0 + nq ** 3]
            r = self.rst[:, q0:q0 + nq ** 3]          # r[3 i + j] = d r_i / d x_j
            dq = [V @ (Dl[i] @ ue) for i in range(3)]
            for d in range(3):
                gd = sum(r[3 * i + d] * dq[i] for i in range(3))
                out[e] += np.sum(W * gd * gd * Jq)
        return out

    def _mortar_norm(self, e, f, ep, f_p, code, child_m, child_p0, S, Ttot, off, u, u_ghost):
        deg_m, deg_p = self._deg(e), self._deg(ep)
        deg_mq = max(self._degq(e), self._degq(ep))
        T = (deg_mq + 1) ** 2
        sj, hm, hp, nrm, _ = self._geom(S, T, Ttot, off)
        um, up = self._vals(e, u, u_ghost), self._vals(ep, u, u_ghost)
        u_m = self._side_to_mortar(deg_m, deg_mq, child_m) @ (face_select(f, deg_m + 1) @ um)
        u_p = self._side_to_mortar(deg_p, deg_mq, child_p0) @ (reorient_matrix(code, deg_p + 1) @ (face_select(f_p, deg_p + 1) @ up))
        w = quad_rule(self.qt, deg_mq)[1]
        W = np.kron(w, w)
        pen = penalty(self.pfcn, deg_m, hm, deg_p, hp, self.c)
        ip = sum((nrm[d] * u_m - nrm[d] * u_p) ** 2 for d in range(3))
        one = np.sum(W * pen * ip * sj)
        return one + one + one          # (added once per direction, d4est_ip_energy_norm.c:251-268)

    def _boundary_norm(self, e, f, u):
        s = self.s
        sd = 6 * e + f
        deg, degq = self._deg(e), self._degq(e)
        T = (degq + 1) ** 2
        S = int(s["side_mortar_stride"][sd])
        sj, hm, _, nrm, _ = self._geom(S, T, T, 0)
        I = quad_interp_1d(self.qt, deg, degq)
        u_m = np.kron(I, I) @ (face_select(f, deg + 1) @ self._vals(e, u, None))
        w = quad_rule(self.qt, degq)[1]
        W = np.kron(w, w)
        pen = penalty(self.pfcn, deg, hm, deg, hm, self.c)
        ip = sum(nrm[d] * u_m * nrm[d] * u_m for d in range(3))
        return np.sum(W * pen * ip * sj)

    def energy(self, u, u_ghost=None):
        """(terms[3, n_elements] = volume, boundary, interface; sums[4] = their sums and the total)"""
        m, s = self.m, self.s
        terms = np.zeros((3, m.n_elements))
        terms[0] = self.volume_term(u)
        hang = s.get("side_hang")
        nodes2 = lambda a, b: (max(self._degq(a), self._degq(b)) + 1) ** 2
        for e in range(m.n_elements):
            for f in range(6):
                sd = 6 * e + f
                nbr, f_p, code = int(s["side_nbr"][sd]), int(s["side_nbr_face"][sd]), int(s["side_reorder"][sd])
                S = int(s["side_mortar_stride"][sd])
                h = 0 if hang is None else int(hang[sd])
                if nbr == -1:
                    terms[1, e] += self._boundary_norm(e, f, u)
                elif h == 0:
                    terms[2, e] += self._mortar_norm(e, f, nbr, f_p, code, None, None, S, nodes2(e, nbr), 0, u, u_ghost)
                elif h == 1:      # big side: its 4 sub-mortars, all added to e
                    n4 = [int(v) for v in s["side_nbr4"][4 * sd:4 * sd + 4]]
                    Tm = [nodes2(e, n4[i]) for i in range(4)]
                    for i in range(4):
                        terms[2, e] += self._mortar_norm(e, f, n4[i], f_p, code, i, None, S, sum(Tm), sum(Tm[:i]), u, u_ghost)
                else:             # small side: its own sub-mortar
                    c = int(s["side_sub"][sd])
                    grp = [int(v) for v in s["side_nbr4"][4 * sd:4 * sd + 4]]
                    Tm = [nodes2(grp[i], nbr) for i in range(4)]
                    terms[2, e] += self._mortar_norm(e, f, nbr, f_p, code, None, c, S, sum(Tm), sum(Tm[:c]), u, u_ghost)
        sums = np.array([terms[0].sum(), terms[1].sum(), terms[2].sum(), 0.0])
        sums[3] = (sums[0] + sums[1]) + sums[2]
        return terms, sums


def masked_sum(elem, skip=None):
    keep = np.ones(len(elem), dtype=bool) if skip is None else (np.asarray(skip) == 0)
    return float(np.sum(np.asarray(elem)[keep]))


__all__ = ["DenseNorms", "error_field", "masked_sum"]
