"""Independent DENSE statement of the hp-multigrid inter-grid transfers in numpy, in the style of tests/dense_sipg.py.
TEST INFRASTRUCTURE.

Nothing here shares code with oracle/*.c or with the library.  The 1-D operators are rebuilt in np.longdouble from the reference's
tabulated Gauss-Lobatto / Gauss nodes and weights (tests/golden/reference_nodes_weights.json):
  p-prolongation    Lagrange interpolation from the dH + 1 coarse Lobatto nodes to the dh + 1 fine ones; the identity at dh = dH
                                                                                     dGMath/d4est_operators.c:995-1012, :1107-1132
  hp-prolongation   the same onto the fine nodes of a half interval, r -> r / 2 -/+ 1 / 2 for child bit 0 / 1; child c of a parent has
                    bits (cx, cy, cz), c = cx + 2 cy + 4 cz                          :944-993, :376-404, d4est_reference.c:14-47
  L2 projection     R = M_H^-1 P^T M_h (p) and R_c = M_H^-1 (P_c / 2)^T M_h per half (hp) with the EXACT 1-D mass matrices of the
                    Lagrange bases (a 20-point Gauss rule integrates the products of two degree <= 19 polynomials exactly); what
                    d4est_operators_apply_p_restrict / _hp_restrict compute           :1134-1185, :1205-1297
  restriction       sum over the children of P_c^T (the transposes of the prolongations)   :1689-1749
  Galerkin term     sum_c (B_c P_c)^T diag(w J c)_c (B_c P_c) u_H of one coarse element, B_c the interpolation to child c's quadrature
                    nodes (Gauss or Lobatto)              Solver/d4est_solver_multigrid_matrix_operator.c:6-48, d4est_operators.c:608-667
The 3-D application is batched: all (item, child) pairs of one shape (children, dH, dh, child position) go through one einsum per
direction, so tens of thousands of items take a fraction of a second.  Arithmetic is np.longdouble inside, results are float64."""
import json
import os

import numpy as np

LD = np.longdouble
_HERE = os.path.dirname(os.path.abspath(__file__))
_TAB = json.load(open(os.path.join(_HERE, "golden", "reference_nodes_weights.json")))
_CACHE = {}


def _rule(kind, n):
    d = _TAB[kind][str(n)]
    return np.array(d["x"], dtype=LD), np.array(d["w"], dtype=LD)


def lagrange(x_from, x_to):
    """L[a, i] = l_i(x_to[a]) for the Lagrange basis on x_from: the product formula, in long double"""
    n = x_from.size
    L = np.ones((x_to.size, n), dtype=LD)
    for i in range(n):
        for j in range(n):
            if j != i:
                L[:, i] *= (x_to - x_from[j]) / (x_from[i] - x_from[j])
    return L


def prolong_1d(hp, dH, dh, bit=0):
    """(dh + 1) x (dH + 1), long double"""
    key = ("P", hp, dH, dh, bit)
    if key not in _CACHE:
        xH, xh = _rule("lobatto", dH + 1)[0], _rule("lobatto", dh + 1)[0]
        if hp:
            _CACHE[key] = lagrange(xH, LD(0.5) * xh + (LD(0.5) if bit else -LD(0.5)))
        else:
            _CACHE[key] = np.eye(dH + 1, dtype=LD) if dh == dH else lagrange(xH, xh)
    return _CACHE[key]


def mass_1d(d):
    """exact M_ij = int_-1^1 l_i l_j of the Lagrange basis on the d + 1 Lobatto nodes"""
    key = ("M", d)
    if key not in _CACHE:
        xg, wg = _rule("gauss", 20)
        L = lagrange(_rule("lobatto", d + 1)[0], xg)
        _CACHE[key] = (L * wg[:, None]).T @ L
    return _CACHE[key]


def _solve(A, B):
    """A^-1 B by Gaussian elimination with partial pivoting (numpy.linalg has no long double)"""
    A, B = A.copy(), B.copy()
    n = A.shape[0]
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]] = A[[p, k]]
            B[[k, p]] = B[[p, k]]
        for r in range(k + 1, n):
            f = A[r, k] / A[k, k]
            A[r, k:] -= f * A[k, k:]
            B[r] -= f * B[k]
    for k in range(n - 1, -1, -1):
        B[k] = (B[k] - A[k, k + 1:] @ B[k + 1:]) / A[k, k]
    return B


def project_1d(hp, dH, dh, bit=0):
    """(dH + 1) x (dh + 1): the 1-D factor of the L2 projection onto the coarse space"""
    key = ("R", hp, dH, dh, bit)
    if key not in _CACHE:
        P = prolong_1d(hp, dH, dh, bit)
        rhs = (P * (LD(0.5) if hp else LD(1.0))).T @ mass_1d(dh)
        _CACHE[key] = _solve(mass_1d(dH), rhs)
    return _CACHE[key]


def quad_interp_1d(quad_type, d, dq):
    """(dq + 1) x (d + 1): Lobatto nodes of degree d -> the quadrature nodes (0: Gauss, 1: Lobatto) of degree dq"""
    key = ("B", quad_type, d, dq)
    if key not in _CACHE:
        _CACHE[key] = lagrange(_rule("lobatto", d + 1)[0], _rule("gauss" if quad_type == 0 else "lobatto", dq + 1)[0])
    return _CACHE[key]


def apply3(Az, Ay, Ax, x):
    """x: [n, cz, cy, cx] (x fastest, d4est_operators.c:1318-1323) -> [n, rz, ry, rx], one einsum per direction"""
    y = np.einsum("ia,ncba->ncbi", Ax, x)
    y = np.einsum("jb,ncbi->ncji", Ay, y)
    return np.einsum("kc,ncji->nkji", Az, y)


class DenseTransfer:
    """the item list of a Transfer (hrefine, degH, degh[8 k + c]) with both vectors element-ordered and contiguous in item order"""

    def __init__(self, hrefine, degH, degh):
        hrefine, degH = np.asarray(hrefine, dtype=np.int64), np.asarray(degH, dtype=np.int64)
        degh = np.asarray(degh, dtype=np.int64).reshape(-1, 8)
        n = hrefine.size
        nc = np.where(hrefine == 1, 8, 1)
        item = np.repeat(np.arange(n), nc)                                   # per (item, child) record, in traversal order
        first = np.concatenate([[0], np.cumsum(nc)])
        pos = np.arange(item.size) - first[item]                             # child position c
        dh = degh[item, pos]
        nH3, nh3 = (degH + 1) ** 3, (dh + 1) ** 3
        self.coarse_bounds = np.concatenate([[0], np.cumsum(nH3)])           # element e of the coarse vector: [b[e], b[e + 1])
        self.fine_bounds = np.concatenate([[0], np.cumsum(nh3)])
        self.coarse_nodes, self.fine_nodes = int(self.coarse_bounds[-1]), int(self.fine_bounds[-1])
        self.n_items, self.n_children = n, int(item.size)
        co, fo = self.coarse_bounds[:-1][item], self.fine_bounds[:-1]
        hp = (nc == 8)[item]
        key = ((hp.astype(np.int64) * 32 + degH[item]) * 32 + dh) * 8 + pos
        order = np.argsort(key, kind="stable")
        cuts = np.nonzero(np.diff(key[order]))[0] + 1
        self.groups = []
        for idx in np.split(order, cuts):
            r = idx[0]
            self.groups.append((bool(hp[r]), int(degH[item[r]]), int(dh[r]), int(pos[r]), co[idx], fo[idx]))

    def _ops(self, table, hp, dH, dh, c):
        return [table(hp, dH, dh, (c >> d) & 1) for d in (2, 1, 0)]         # z, y, x

    def prolong(self, xc):
        xc = np.asarray(xc, dtype=LD)
        out = np.zeros(self.fine_nodes, dtype=LD)
        for hp, dH, dh, c, co, fo in self.groups:
            NH, Nh = dH + 1, dh + 1
            x = xc[co[:, None] + np.arange(NH ** 3)].reshape(-1, NH, NH, NH)
            Pz, Py, Px = self._ops(prolong_1d, hp, dH, dh, c)
            out[(fo[:, None] + np.arange(Nh ** 3)).ravel()] = apply3(Pz, Py, Px, x).ravel()
        return out.astype(np.float64)

    def _down(self, xf, table, transpose):
        xf = np.asarray(xf, dtype=LD)
        out = np.zeros(self.coarse_nodes, dtype=LD)
        for hp, dH, dh, c, co, fo in self.groups:
            NH, Nh = dH + 1, dh + 1
            x = xf[fo[:, None] + np.arange(Nh ** 3)].reshape(-1, Nh, Nh, Nh)
            Oz, Oy, Ox = [(o.T if transpose else o) for o in self._ops(table, hp, dH, dh, c)]
            # one record per coarse element in a group (a child position occurs once per item): plain indexed addition is safe
            out[(co[:, None] + np.arange(NH ** 3)).ravel()] += apply3(Oz, Oy, Ox, x).ravel()
        return out.astype(np.float64)

    def restrict(self, xf):
        """sum over the children of P_c^T x_c"""
        return self._down(xf, prolong_1d, True)

    def project(self, xf):
        """the L2 projection onto the coarse space: sum over the children of R_c x_c"""
        return self._down(xf, project_1d, False)


def galerkin_term(quad_type, hp, dH, dh, dq, w_j_c, uH):
    """sum_c (B_c P_c)^T diag(w J c)_c (B_c P_c) u_H for ONE coarse element.  dh, dq: the children's degrees and quadrature degrees (eight
    entries if hp, else one); w_j_c[c]: the product J c at child c's (dq_c + 1)^3 quadrature nodes, x fastest -- the weights are applied
    here from the tabulated rule."""
    NH = dH + 1
    u = np.asarray(uH, dtype=LD).reshape(1, NH, NH, NH)
    out = np.zeros((NH, NH, NH), dtype=LD)
    for c in range(8 if hp else 1):
        T = [quad_interp_1d(quad_type, dh[c], dq[c]) @ prolong_1d(hp, dH, dh[c], (c >> d) & 1) for d in (2, 1, 0)]
        w = _rule("gauss" if quad_type == 0 else "lobatto", dq[c] + 1)[1]
        W = (w[:, None, None] * w[None, :, None] * w[None, None, :]) * np.asarray(w_j_c[c], dtype=LD).reshape((dq[c] + 1,) * 3)
        v = apply3(T[0], T[1], T[2], u) * W[None]
        out += apply3(T[0].T, T[1].T, T[2].T, v)[0]
    return out.ravel().astype(np.float64)


def elementwise_rel_err(got, ref, bounds):
    """max over the elements [bounds[e], bounds[e + 1]) of max |got - ref| / max |ref| -- every element against its OWN scale, so a wrong
    small element cannot hide behind a large one.  NaN (an entry that was never written) counts as infinite."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    d = np.abs(got - ref)
    d[~np.isfinite(got)] = np.inf
    starts = np.asarray(bounds[:-1], dtype=np.int64)
    err = np.maximum.reduceat(d, starts)
    scale = np.maximum.reduceat(np.abs(ref), starts)
    assert (scale > 0).all(), "an element of the reference is identically zero: choose another input"
    return float((err / scale).max())
