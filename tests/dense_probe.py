"""numpy restatement of the point probes (include/d4est_hip.h "point probes"): the element search and rst of
d4est_mesh_interpolate_at_tree_coord (src/Mesh/d4est_mesh.c:3294-3362), the product-form Lagrange basis of d4est_lgl_lagrange_1d
(src/dGMath/d4est_lgl.c:59-68) with its derivative, the tensor sums of d4est_operators_interpolate (src/dGMath/d4est_operators.c:2289-2340)
and the inverse Jacobian of the tree map at the point.  Independent of the device code: plain loops over elements and factors, vectorised
over points only (elementwise numpy operations round like the scalar ones).  Pinned without a device by tests/test_probe_dense.py.

The basis is evaluated operation for operation as the reference writes it, so it can be compared bit for bit; the tensor sums are not
order-faithful -- their bound is below."""
import numpy as np

from disco4est_amd import table

EPS = float(np.finfo(np.float64).eps)


def locate(tree, abc, cells, root_len):
    """(err[n], elem[n], rst[n,3]): first element in traversal order whose closed box contains abc (d4est_mesh.c:3317-3328), rst at :3339"""
    etree, eq, edq = (np.asarray(c) for c in cells)
    eq = eq.reshape(-1, 3)
    tree = np.asarray(tree).reshape(-1)
    abc = np.asarray(abc, dtype=np.float64).reshape(-1, 3)
    n = tree.size
    err = np.ones(n, dtype=np.int32)
    elem = -np.ones(n, dtype=np.int32)
    rst = np.full((n, 3), np.nan)
    rl = float(root_len)
    for p in range(n):
        for e in range(etree.size):
            if etree[e] != tree[p]:
                continue
            check = 0
            for d in range(3):
                amin = float(eq[e, d]) / rl
                amax = float(int(eq[e, d]) + int(edq[e])) / rl
                check += (abc[p, d] <= amax) and (abc[p, d] >= amin)
            if check == 3:
                for d in range(3):
                    amin = float(eq[e, d]) / rl
                    amax = float(int(eq[e, d]) + int(edq[e])) / rl
                    rst[p, d] = 2 * (abc[p, d] - amin) / (amax - amin) - 1
                err[p], elem[p] = 0, e
                break
    return err, elem, rst


def lagrange(x, lgl, j):
    """d4est_lgl_lagrange_1d: l = 1; for i != j: l *= (x - lgl[i]) / (lgl[j] - lgl[i]); x an array of points"""
    l = np.ones_like(x)
    for i in range(lgl.size):
        if i != j:
            l = l * ((x - lgl[i]) / (lgl[j] - lgl[i]))
    return l


def lagrange_deriv(x, lgl, j):
    """d/dx of the product above: the sum over the left-out factor m (ascending) of 1 / (lgl[j] - lgl[m]) times the remaining product"""
    d = np.zeros_like(x)
    for m in range(lgl.size):
        if m == j:
            continue
        l = np.full_like(x, 1.0 / (lgl[j] - lgl[m]))
        for i in range(lgl.size):
            if i != j and i != m:
                l = l * ((x - lgl[i]) / (lgl[j] - lgl[i]))
        d = d + l
    return d


def basis(deg, rst):
    """L[n, 3, N], D[n, 3, N]: l_i and l'_i at rst[n, d] on the engine's Lobatto nodes of degree deg"""
    lgl = table("lobatto_nodes", int(deg))
    rst = np.asarray(rst, dtype=np.float64).reshape(-1, 3)
    N = lgl.size
    L = np.empty((rst.shape[0], 3, N))
    D = np.empty((rst.shape[0], 3, N))
    for d in range(3):
        x = np.ascontiguousarray(rst[:, d])
        for i in range(N):
            L[:, d, i] = lagrange(x, lgl, i)
            D[:, d, i] = lagrange_deriv(x, lgl, i)
    return L, D


def _element_values(u, ns, N):
    idx = np.asarray(ns, dtype=np.int64)[:, None] + np.arange(N ** 3)[None, :]
    return u[idx].reshape(-1, N, N, N)     # [n, k, j, i], i fastest


def evaluate(u, ns, deg, rst):
    """value[n] = sum_kji l_k(t) l_j(s) l_i(r) u[ns + (k N + j) N + i] and S[n] = the same sum of absolute values, for points whose
    elements have nodal strides ns[n] and degrees deg[n]"""
    ns, deg = np.asarray(ns), np.asarray(deg)
    rst = np.asarray(rst, dtype=np.float64).reshape(-1, 3)
    val = np.empty(ns.size)
    S = np.empty(ns.size)
    for p in np.unique(deg):
        sel = np.nonzero(deg == p)[0]
        L, _ = basis(p, rst[sel])
        U = _element_values(u, ns[sel], int(p) + 1)
        T = np.einsum("nk,nj,ni->nkji", L[:, 2], L[:, 1], L[:, 0]) * U
        val[sel] = T.sum(axis=(1, 2, 3))
        S[sel] = np.abs(T).sum(axis=(1, 2, 3))
    return val, S


def gradient_ref(u, ns, deg, rst):
    """g[n, 3] = (du/dr, du/ds, du/dt) from l'_i(r) l_j(s) l_k(t) etc. and S[n, 3], the sums of absolute values"""
    ns, deg = np.asarray(ns), np.asarray(deg)
    rst = np.asarray(rst, dtype=np.float64).reshape(-1, 3)
    g = np.empty((ns.size, 3))
    S = np.empty((ns.size, 3))
    for p in np.unique(deg):
        sel = np.nonzero(deg == p)[0]
        L, D = basis(p, rst[sel])
        U = _element_values(u, ns[sel], int(p) + 1)
        for d in range(3):
            f = [D[:, a] if a == d else L[:, a] for a in range(3)]
            T = np.einsum("nk,nj,ni->nkji", f[2], f[1], f[0]) * U
            g[sel, d] = T.sum(axis=(1, 2, 3))
            S[sel, d] = np.abs(T).sum(axis=(1, 2, 3))
    return g, S


def drdx_brick(extents, dq, root_len):
    """R[n, i, d] = dr_i/dx_d of the brick: the inverse of diag((X1 - X0) dq / root_len / 2)"""
    ex = np.asarray(extents, dtype=np.float64)
    half = np.asarray(dq, dtype=np.float64) / float(root_len) / 2.0
    R = np.zeros((half.size, 3, 3))
    for d in range(3):
        R[:, d, d] = 1.0 / ((ex[2 * d + 1] - ex[2 * d]) * half)
    return R


def dxdr_map(mapping, tree, abc, dq, root_len):
    """dx_i/dr_j [n, 3, 3] of an analytic tree map (forest.*Map.jacobian) at the points: dx/d(abc) dq / root_len / 2"""
    tree = np.asarray(tree).reshape(-1)
    abc = np.asarray(abc, dtype=np.float64).reshape(-1, 3)
    out = np.empty((tree.size, 3, 3))
    for p in range(tree.size):
        out[p] = mapping.jacobian(int(tree[p]), abc[p:p + 1])[0] * (0.5 * float(dq[p]) / float(root_len))
    return out


def physical(g_ref, R):
    """du/dx_d = sum_i du/dr_i dr_i/dx_d; also the infinity norm of the matrix applied, max_d sum_i |R[i, d]|"""
    g = np.einsum("ni,nid->nd", g_ref, R)
    return g, np.abs(R).sum(axis=1).max(axis=1)


def bound(deg, S):
    """|device - restatement| <= (N^3 + 6 N) eps S: N^3 for any order of the N^3-term sum, 6 N for the roundings of the three basis products"""
    N = np.asarray(deg, dtype=np.float64) + 1.0
    return (N ** 3 + 6.0 * N) * EPS * S
