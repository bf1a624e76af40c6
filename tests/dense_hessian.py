"""Independent DENSE evaluation of the Laplacian of a DG field at the quadrature nodes -- a numpy restatement of
src/dGMath/d4est_hessian.c (d4est_hessian_compute_hessian_trace_of_field_on_quadrature_points, :270-368) -- and of the pointwise
residual term of d4est_estimator_bi_new_compute (src/Estimators/d4est_estimator_bi_new.c:471-487).  TEST INFRASTRUCTURE.

The 1-D tables D (collocation derivative) and B (Lobatto -> quadrature nodes) are built here, with the formulas of
tests/dense_sipg.py, on nodes this module computes itself (``nodes_1d``): the roots of P_p' (Lobatto) and of P_n (Gauss) by Newton's
method in long double, started from the committed node fixture and rounded to float64.  Nothing comes from the library.  The fixture's
own values are not used as they stand because its 12 Lobatto points (p = 11) are off by 9e-15 -- a 1.5e-14 relative error in D, which
second derivatives amplify past the rounding of a float64 evaluation; tests/test_hessian_dense.py measures this.
Per element, in the reference's loop order (``order="reference"``):
    d2rdrdx[m][n][k] -= drdx[m][l] drdx[a][n] d2xdrdr[l][a][k]          over a, then l                      :43-58
    du_q[b] = V(D_b u),  d2u_q[b][a] = V(D_a (D_b u))                   all nine                            :77-110
    trace += drdx[a][i] (d2rdrdx[b][i][a] du_q[b] + drdx[b][i] d2u_q[b][a])   over i, a, b                  :127-138
``order="folded"`` is the form the device kernel uses: c_b = sum_i sum_a drdx[a][i] d2rdrdx[b][i][a], G_ab = sum_i drdx[a][i] drdx[b][i],
trace = sum_b c_b du_q[b] + sum_{a <= b} (2 - delta_ab) G_ab d2u_q[a][b].  The two differ by rounding only.

Where drdx and d2xdrdr come from (``form``):
    "brick"      drdx = diag(2 / h), d2xdrdr = 0                                  (d4est_geometry_brick.c:8)
    "analytic"   HESSIAN_ANALYTICAL: the numpy tree map's jacobian (inverted) and second_derivatives at the quadrature nodes
    "numerical"  HESSIAN_NUMERICAL (:227-262): d2xdrdr[d1][d2][d3] = V(D_d3 D_d2 x_d1) from the node coordinates; drdx from the
                 rst_xyz_quad given, or from V(D x) inverted
``dtype`` (numpy.float64 or numpy.longdouble) is the precision of every operation after the float64 inputs (tables, coordinates,
field) have been cast: the long-double run measures the rounding error of the float64 runs."""
import numpy as np

from numpy.polynomial import legendre as _leg

from tests.dense_sipg import diff_matrix, gauss, lagrange_matrix, lobatto, quad_rule

_NODES = {}


def nodes_1d(kind, deg):
    """the deg + 1 Lobatto ("lobatto": -1, the roots of P_deg', 1) or Gauss ("gauss": the roots of P_{deg+1}) nodes, correctly rounded:
    four Newton steps in long double from the committed fixture's values, then rounded to float64"""
    if (kind, deg) not in _NODES:
        ld = np.longdouble
        x = (lobatto(deg)[0] if kind == "lobatto" else gauss(deg)[0]).astype(ld)
        c = np.zeros(deg + 2, dtype=ld)
        c[deg if kind == "lobatto" else deg + 1] = 1
        f = _leg.legder(c) if kind == "lobatto" else c
        df = _leg.legder(f)
        inner = slice(1, -1) if kind == "lobatto" else slice(None)
        for _ in range(4):
            xi = x[inner]
            x[inner] = xi - _leg.legval(xi, f) / _leg.legval(xi, df)
        _NODES[(kind, deg)] = x.astype(np.float64)
    return _NODES[(kind, deg)]


def _apply(M, v, axis, n):
    """the 1-D matrix M along `axis` (0 = x, the fastest) of the n x n x n tensor v"""
    t = v.reshape(n, n, n)          # [k, j, i]
    if axis == 0:
        out = np.einsum("ai,kji->kja", M, t)
    elif axis == 1:
        out = np.einsum("aj,kji->kai", M, t)
    else:
        out = np.einsum("ak,kji->aji", M, t)
    return out.reshape(-1)


def _interp(B, v, n):
    """V v: Lobatto nodes -> quadrature nodes, x then y then z"""
    nq = B.shape[0]
    t = np.einsum("ai,kji->kja", B, v.reshape(n, n, n))
    t = np.einsum("bj,kja->kba", B, t)
    t = np.einsum("ck,kba->cba", B, t)
    return t.reshape(nq ** 3)


def inv3(A):
    """inverse of A[n, 3, 3] by cofactors (numpy.linalg has no long double)"""
    c = np.empty_like(A)
    for i in range(3):
        for j in range(3):
            i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
            c[:, j, i] = A[:, i1, j1] * A[:, i2, j2] - A[:, i1, j2] * A[:, i2, j1]
    det = A[:, 0, 0] * c[:, 0, 0] + A[:, 0, 1] * c[:, 1, 0] + A[:, 0, 2] * c[:, 2, 0]
    return c / det[:, None, None]


def _tensor_ref(x1):
    n = x1.size
    ref = np.empty((n, n, n, 3), dtype=x1.dtype)
    ref[..., 0] = x1[None, None, :]
    ref[..., 1] = x1[None, :, None]
    ref[..., 2] = x1[:, None, None]
    return ref.reshape(-1, 3)


class DenseHessian:
    def __init__(self, mesh, form, dtype=np.float64, mapping=None, xyz=None, rst=None):
        """mesh: mesh.BrickMesh / HangingBrickMesh ("brick", "numerical") or forest.ForestMesh ("analytic", mapping = its tree map, and
        "numerical"); xyz = (x, y, z) at the Lobatto nodes and rst = rst_xyz_quad or None for the numerical form"""
        self.m, self.form, self.dt = mesh, form, np.dtype(dtype)
        self.qt = int(mesh.quad_type)
        self.R, self.X2 = [], []           # per element: drdx[a][i] as [nq3, 3, 3], d2xdrdr[l][a][k] as [nq3, 3, 3, 3]
        self._ops = {}
        for e in range(mesh.n_elements):
            p, pq = int(mesh.deg[e]), int(mesh.deg_quad[e])
            n, nq3 = p + 1, (pq + 1) ** 3
            D, B = self.ops(p, pq)
            if form == "brick":
                h = self._brick_h(e)
                R = np.zeros((nq3, 3, 3), dtype=self.dt)
                for d in range(3):
                    R[:, d, d] = self.dt.type(2.0) / self.dt.type(h)
                X2 = np.zeros((nq3, 3, 3, 3), dtype=self.dt)
            elif form == "analytic":
                xq = nodes_1d("gauss" if self.qt == 0 else "lobatto", pq).astype(self.dt)
                org = np.asarray(mesh.org[e]).astype(self.dt)
                size, nf = self.dt.type(int(mesh.size[e])), self.dt.type(int(mesh.nf))
                xi = (org[None, :] + self.dt.type(0.5) * size * (_tensor_ref(xq) + self.dt.type(1.0))) / nf
                s = self.dt.type(0.5) * size / nf
                tree = int(mesh.tree[e])
                R = inv3(mapping.jacobian(tree, xi) * s)
                X2 = mapping.second_derivatives(tree, xi) * (s * s)
            elif form == "numerical":
                s0, q0 = int(mesh.nodal_stride[e]), int(mesh.quad_stride[e])
                xs = [np.asarray(c[s0:s0 + n ** 3]).astype(self.dt) for c in xyz]
                X2 = np.empty((nq3, 3, 3, 3), dtype=self.dt)
                for d1 in range(3):
                    for d2 in range(3):
                        dr = _apply(D, xs[d1], d2, n)
                        for d3 in range(3):
                            X2[:, d1, d2, d3] = _interp(B, _apply(D, dr, d3, n), n)
                if rst is not None:
                    r9 = np.asarray(rst).reshape(9, -1)
                    R = np.stack([np.stack([r9[3 * a + i, q0:q0 + nq3] for i in range(3)], axis=1) for a in range(3)], axis=1).astype(self.dt)
                else:
                    dxdr = np.empty((nq3, 3, 3), dtype=self.dt)
                    for d in range(3):
                        for d1 in range(3):
                            dxdr[:, d, d1] = _interp(B, _apply(D, xs[d], d1, n), n)
                    R = inv3(dxdr)
            else:
                raise ValueError(form)
            self.R.append(R)
            self.X2.append(X2)

    def _brick_h(self, e):
        m = self.m
        return float(m.h_elem[e]) if hasattr(m, "h_elem") else float(m.h)

    def ops(self, p, pq):
        if (p, pq) not in self._ops:
            xl = nodes_1d("lobatto", p)
            xq = nodes_1d("gauss" if self.qt == 0 else "lobatto", pq)
            self._ops[(p, pq)] = (diff_matrix(xl).astype(self.dt), lagrange_matrix(xl, xq).astype(self.dt))
        return self._ops[(p, pq)]

    def trace(self, u, order="reference"):
        """the Laplacian of u[local_nodes] at the quadrature nodes, [local_nodes_quad], in self.dt"""
        m = self.m
        out = np.zeros(m.local_nodes_quad, dtype=self.dt)
        for e in range(m.n_elements):
            p, pq = int(m.deg[e]), int(m.deg_quad[e])
            n, nq3 = p + 1, (pq + 1) ** 3
            s0, q0 = int(m.nodal_stride[e]), int(m.quad_stride[e])
            D, B = self.ops(p, pq)
            ue = np.asarray(u[s0:s0 + n ** 3]).astype(self.dt)
            R, X2 = self.R[e], self.X2[e]
            d2r = np.zeros((nq3, 3, 3, 3), dtype=self.dt)
            for mm in range(3):
                for nn in range(3):
                    for k in range(3):
                        for a in range(3):
                            for l in range(3):
                                d2r[:, mm, nn, k] -= R[:, mm, l] * R[:, a, nn] * X2[:, l, a, k]
            du = [_apply(D, ue, b, n) for b in range(3)]
            du_q = [_interp(B, du[b], n) for b in range(3)]
            tr = np.zeros(nq3, dtype=self.dt)
            if order == "reference":
                d2u_q = [[_interp(B, _apply(D, du[b], a, n), n) for a in range(3)] for b in range(3)]
                for i in range(3):
                    for a in range(3):
                        for b in range(3):
                            tr += R[:, a, i] * (d2r[:, b, i, a] * du_q[b] + R[:, b, i] * d2u_q[b][a])
            elif order == "folded":
                for b in range(3):
                    c = np.zeros(nq3, dtype=self.dt)
                    for i in range(3):
                        for a in range(3):
                            c += R[:, a, i] * d2r[:, b, i, a]
                    tr += c * du_q[b]
                for a in range(3):
                    for b in range(a, 3):
                        G = R[:, a, 0] * R[:, b, 0] + R[:, a, 1] * R[:, b, 1] + R[:, a, 2] * R[:, b, 2]
                        d2 = _interp(B, _apply(D, du[a], b, n), n)
                        tr += (G if a == b else self.dt.type(2.0) * G) * d2
            else:
                raise ValueError(order)
            out[q0:q0 + nq3] = tr
        return out

    def pointwise_term0(self, r_quad, J, diam):
        """h^2 / deg^2 sum_q w_q J_q r_q^2 per element (d4est_estimator_bi_new.c:471-487)"""
        m = self.m
        out = np.zeros(m.n_elements, dtype=self.dt)
        for e in range(m.n_elements):
            p, pq = int(m.deg[e]), int(m.deg_quad[e])
            q0, nq3 = int(m.quad_stride[e]), (pq + 1) ** 3
            w = quad_rule(self.qt, pq)[1].astype(self.dt)
            W = np.kron(w, np.kron(w, w))
            r = np.asarray(r_quad[q0:q0 + nq3]).astype(self.dt)
            h = self.dt.type(float(diam[e]))
            out[e] = np.sum(W * np.asarray(J[q0:q0 + nq3]).astype(self.dt) * r * r) * (h * h / self.dt.type(p * p))
        return out


def quad_coords(mesh, mapping=None):
    """physical (x, y, z) at the quadrature nodes of a mesh.BrickMesh (optionally through a smooth map) or a forest.ForestMesh"""
    out = [np.empty(mesh.local_nodes_quad) for _ in range(3)]
    for e in range(mesh.n_elements):
        pq = int(mesh.deg_quad[e])
        xq = nodes_1d("gauss" if int(mesh.quad_type) == 0 else "lobatto", pq)
        q0, nq3 = int(mesh.quad_stride[e]), (pq + 1) ** 3
        if hasattr(mesh, "tree"):
            X = (mapping or mesh.mapping).x(int(mesh.tree[e]), mesh._cell_xi(mesh.org[e], mesh.size[e], _tensor_ref(xq)))
            X = (X[:, 0], X[:, 1], X[:, 2])
        else:
            X = mesh._ref_coords(e, xq)
            if mapping is not None:
                X = mapping.x(*X)
        for d in range(3):
            out[d][q0:q0 + nq3] = X[d]
    return out


def error_bound(dense64, dense_ld, u):
    """the GPU tests' bound for one case: 4 x the larger float64 error (reference order, folded order) against the long-double
    result, with a floor of 64 eps max|Lap u|; returns (bound, long-double reference as float64, the two float64 errors)"""
    ref = dense_ld.trace(u, "reference")
    errs = [float(np.abs(dense64.trace(u, o).astype(np.longdouble) - ref).max()) for o in ("reference", "folded")]
    floor = 64.0 * np.finfo(np.float64).eps * float(np.abs(ref).max())
    return max(4.0 * max(errs), floor), ref.astype(np.float64), errs
