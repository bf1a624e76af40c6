"""Independent DENSE statement of the multigrid MATRIX OPERATOR (csrc/d4est_hip_mgmatrix.hip) in numpy, in the style of
tests/dense_transfer.py and tests/dense_nonlinear.py.  TEST INFRASTRUCTURE.

Nothing here shares code with oracle/*.c or with the kernels.  The 1-D tables (interpolation to the quadrature nodes, quadrature weights,
p- and hp-prolongation) are the library's own float64 tables (d4est_hip_table); everything built from them is accumulated in
np.longdouble and rounded to float64 once at the end:
  mass_blocks      V^T diag(w (x) w (x) w . J . c) V per element, V = B (x) B (x) B       Quadrature/d4est_quadrature.c:1143-1186
  restrict_blocks  sum_c P_c^T M_c P_c per coarse element, or the reference's literal window      dGMath/d4est_operators.c:608-667
  block_term       M_e u_e per element                          Problems/ConstantDensityStar/constant_density_star_fcns.h:485-527
The three *_per_wg / *_split functions restate HOW THE HOST CUTS THE WORK INTO WORKGROUPS.  They are not expected values of anything:
they exist so that tests/test_mgmatrix_dense.py can prove that the case lists of tests/mgmatrix_cases.py reach every launch shape."""
import numpy as np

from disco4est_amd import capi

LD = np.longdouble
_CACHE = {}


def interp_1d(quad_type, deg, deg_quad):
    """(deg_quad + 1) x (deg + 1), long double: Lobatto nodes of degree deg -> the quadrature nodes (0: Gauss, 1: Lobatto)"""
    key = ("B", quad_type, deg, deg_quad)
    if key not in _CACHE:
        t = capi.table("lobatto_to_gauss" if quad_type == 0 else "p_prolong", deg, deg_quad)
        _CACHE[key] = t.reshape(deg_quad + 1, deg + 1).astype(LD)
    return _CACHE[key]


def weights_1d(quad_type, deg_quad):
    key = ("w", quad_type, deg_quad)
    if key not in _CACHE:
        _CACHE[key] = capi.table("gauss_weights" if quad_type == 0 else "lobatto_weights", deg_quad).astype(LD)
    return _CACHE[key]


def prolong_1d(hp, degH, degh, bit=0):
    """(degh + 1) x (degH + 1), long double: p-prolongation, or the half `bit` of the hp-prolongation"""
    key = ("P", bool(hp), degH, degh, bit)
    if key not in _CACHE:
        if hp:
            _CACHE[key] = capi.table("hp_prolong", degH, degh).reshape(2, degh + 1, degH + 1)[bit].astype(LD)
        else:
            _CACHE[key] = capi.table("p_prolong", degH, degh).reshape(degh + 1, degH + 1).astype(LD)
    return _CACHE[key]


def matrix_nodes(deg):
    return int(((np.asarray(deg, dtype=np.int64) + 1) ** 6).sum())


def consecutive_offsets(deg):
    n6 = (np.asarray(deg, dtype=np.int64) + 1) ** 6
    return np.concatenate([[0], np.cumsum(n6)[:-1]]).astype(np.int64)


# ---- V^T W V ----------------------------------------------------------------------------------------------------------------------
def mass_blocks(mesh, J, coeff=None):
    """blocks of every element, consecutive in element order (x fastest inside an element); coeff None: the plain mass matrix.
    Sum-factorised: entry ((iz, iy, ix), (jz, jy, jx)) = sum_q W[qz, qy, qx] B[qz, iz] B[qz, jz] B[qy, iy] B[qy, jy] B[qx, ix] B[qx, jx],
    one direction at a time, all elements of one (deg, deg_quad) pair at once."""
    J = np.asarray(J, dtype=np.float64)
    out = np.empty(matrix_nodes(mesh.deg))
    off = consecutive_offsets(mesh.deg)
    pairs = sorted(set(zip(mesh.deg.tolist(), mesh.deg_quad.tolist())))
    for d, dq in pairs:
        el = np.nonzero((mesh.deg == d) & (mesh.deg_quad == dq))[0]
        N, Q = d + 1, dq + 1
        B = interp_1d(mesh.quad_type, d, dq)
        BB = (B[:, :, None] * B[:, None, :]).reshape(Q, N * N)                         # [q, (i, j)]
        w = weights_1d(mesh.quad_type, dq)
        idx = np.asarray(mesh.quad_stride)[el][:, None] + np.arange(Q ** 3)
        W = J[idx].astype(LD)
        if coeff is not None:
            W = W * np.asarray(coeff, dtype=np.float64)[idx].astype(LD)
        W = W.reshape(-1, Q, Q, Q) * (w[:, None, None] * w[None, :, None] * w[None, None, :])
        for lo in range(0, el.size, 64):
            Wc = W[lo:lo + 64]
            n = Wc.shape[0]
            t = Wc.reshape(n * Q * Q, Q) @ BB                                           # [(e, qz, qy), (ix, jx)]
            t = np.moveaxis(t.reshape(n, Q, Q, N * N), 2, -1).reshape(n * Q * N * N, Q) @ BB   # [(e, qz, ix, jx), (iy, jy)]
            t = np.moveaxis(t.reshape(n, Q, N * N, N * N), 1, -1).reshape(n * N ** 4, Q) @ BB  # [(e, ix, jx, iy, jy), (iz, jz)]
            t = t.reshape(n, N, N, N, N, N, N)                                          # [e, ix, jx, iy, jy, iz, jz]
            blk = np.transpose(t, (0, 5, 3, 1, 6, 4, 2)).reshape(n, N ** 6)             # [e, iz, iy, ix, jz, jy, jx]
            for k, e in enumerate(el[lo:lo + 64]):
                out[off[e]:off[e] + N ** 6] = blk[k]
    return out


# ---- sum_c P_c^T M_c P_c ------------------------------------------------------------------------------------------------------------
def _dense_prolong(hp, dH, dh, c):
    """(dh + 1)^3 x (dH + 1)^3, long double: child c = (cx, cy, cz) bits, x fastest (d4est_operators.c:394-404)"""
    Px, Py, Pz = (prolong_1d(hp, dH, dh, (c >> d) & 1) for d in (0, 1, 2))
    return np.kron(Pz, np.kron(Py, Px))


def _two_sided(M, Pz, Py, Px):
    """P^T M P for P = Pz (x) Py (x) Px, M: [g, nh^3, nh^3] -> [g, nH^3, nH^3], one index at a time"""
    g = M.shape[0]
    nh, nH = Px.shape
    t = M.reshape(g, nh, nh, nh, nh, nh, nh)
    for axis, P in zip((1, 2, 3, 4, 5, 6), (Pz, Py, Px, Pz, Py, Px)):
        t = np.moveaxis(np.tensordot(t, P, axes=([axis], [0])), -1, axis)
    return t.reshape(g, nH ** 3, nH ** 3)


def _right_sided(M, Pz, Py, Px):
    """M P, M: [g, nh^3, nh^3] -> [g, nh^3, nH^3]"""
    g = M.shape[0]
    nh, nH = Px.shape
    t = M.reshape(g, nh ** 3, nh, nh, nh)
    for axis, P in zip((2, 3, 4), (Pz, Py, Px)):
        t = np.moveaxis(np.tensordot(t, P, axes=([axis], [0])), -1, axis)
    return t.reshape(g, nh ** 3, nH ** 3)


def _sliced_matmul(A, B, bits=17, parts=4):
    """A @ B for long-double A [m, k], B [k, n] where numpy's long-double matmul (no BLAS) would take minutes: the rows of A and the
    columns of B are cut into `parts` slices of `bits`-bit integers times a power of two; a product of two slices is a sum of k
    integers below 2^(2 bits) -- exact in float64 (BLAS) up to k = 2^(52 - 2 bits) = 2^18 -- and the slice products are added up in
    long double.  What is dropped (slice pairs of joint order >= parts) is below 2^(-bits parts) = 3e-21 of (row maximum) x (column maximum) per term."""
    def slices(X, axis):
        mx = np.abs(X).max(axis=axis, keepdims=True).astype(np.float64)
        mx[mx == 0.0] = 1.0
        e = (np.ceil(np.log2(mx)) + 1).astype(np.int64)
        out, r = [], X.copy()
        for k in range(parts):
            s = np.ldexp(LD(1.0), e - bits * (k + 1))
            p = np.rint(r / s)
            out.append((p.astype(np.float64), s))
            r = r - p * s
        return out
    assert A.shape[1] <= 1 << (52 - 2 * bits)
    sa, sb = slices(A, 1), slices(B, 0)
    acc = np.zeros((A.shape[0], B.shape[1]), dtype=LD)
    for k, (pa, ka) in enumerate(sa):
        for l, (pb, kb) in enumerate(sb):
            if k + l < parts:
                acc += (pa @ pb).astype(LD) * ka * kb
    return acc


def restrict_blocks(hrefine, degH, degh, fine_blocks, literal_window=False):
    """coarse blocks of a transfer's item list (hrefine[k], degH[k], degh[8 k + c]); the fine blocks are consecutive in traversal order.
    literal_window: on items with eight children the left factor of child c is not P_c^T but the window
    PT.ravel()[s_c : s_c + nH^3 nh_c^3] read as an nH^3 x nh_c^3 matrix, PT the transpose of the STACKED prolongation and
    s_c = nH^3 sum_{c' < c} nh_c'^3 (d4est_operators.c:637, :651; build_windows of the library describes the same window)."""
    hrefine = np.asarray(hrefine, dtype=np.int64)
    degH = np.asarray(degH, dtype=np.int64)
    degh = np.asarray(degh, dtype=np.int64).reshape(-1, 8)
    fine_blocks = np.asarray(fine_blocks, dtype=np.float64)
    nc = np.where(hrefine == 1, 8, 1)
    n6 = np.concatenate([((degh[k, :nc[k]] + 1) ** 6) for k in range(hrefine.size)])
    foff = np.concatenate([[0], np.cumsum(n6)])
    first = np.concatenate([[0], np.cumsum(nc)])
    assert foff[-1] == fine_blocks.size
    coff = consecutive_offsets(degH)
    out = np.empty(matrix_nodes(degH))
    groups = {}
    for k in range(hrefine.size):
        groups.setdefault((int(nc[k]), int(degH[k]), tuple(degh[k, :nc[k]].tolist())), []).append(k)
    for (children, dH, dhs), items in groups.items():
        items = np.asarray(items)
        hp = children == 8
        nH3 = (dH + 1) ** 3
        acc = np.zeros((items.size, nH3, nH3), dtype=LD)
        PT_flat = None
        if hp and literal_window:
            PT_flat = np.ascontiguousarray(np.vstack([_dense_prolong(True, dH, dhs[c], c) for c in range(8)]).T).ravel()
        s = 0
        for c in range(children):
            nh3 = (dhs[c] + 1) ** 3
            M = fine_blocks[foff[first[items] + c][:, None] + np.arange(nh3 * nh3)].reshape(-1, nh3, nh3).astype(LD)
            Pz, Py, Px = (prolong_1d(hp, dH, dhs[c], (c >> d) & 1) for d in (2, 1, 0))
            if PT_flat is None:
                acc += _two_sided(M, Pz, Py, Px)
            else:
                Wc = PT_flat[s:s + nH3 * nh3].reshape(nH3, nh3)
                T = _right_sided(M, Pz, Py, Px)
                if nH3 * nh3 * nH3 <= 1 << 25:
                    acc += np.matmul(Wc, T)
                else:
                    for k in range(items.size):
                        acc[k] += _sliced_matmul(Wc, T[k])
                s += nH3 * nh3
        for k, it in enumerate(items):
            out[coff[it]:coff[it] + nH3 * nH3] = acc[k].ravel()
    return out


# ---- M_e u_e --------------------------------------------------------------------------------------------------------------------
def block_term(mesh, blocks, u, block_offset=None):
    """the zeroth-order term alone: out_e = M_e u_e, M_e the (deg_e + 1)^3 square block at block_offset[e] (None: consecutive)"""
    blocks = np.asarray(blocks, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64)
    off = consecutive_offsets(mesh.deg) if block_offset is None else np.asarray(block_offset, dtype=np.int64)
    out = np.empty(mesh.local_nodes)
    for d in sorted(set(mesh.deg.tolist())):
        el = np.nonzero(mesh.deg == d)[0]
        n3 = (d + 1) ** 3
        per = max(1, (1 << 22) // (n3 * n3))                                            # at most 64 MB of long doubles at a time
        for lo in range(0, el.size, per):
            e = el[lo:lo + per]
            M = blocks[off[e][:, None] + np.arange(n3 * n3)].reshape(-1, n3, n3).astype(LD)
            x = u[np.asarray(mesh.nodal_stride)[e][:, None] + np.arange(n3)].astype(LD)
            y = np.einsum("eij,ej->ei", M, x)
            out[(np.asarray(mesh.nodal_stride)[e][:, None] + np.arange(n3)).ravel()] = y.ravel()
    return out


# ---- how the host cuts the work into workgroups (restatements, NOT expected values) --------------------------------------------------
def rows_per_wg(n_elem, N3):
    """add_lhs_blocks_term, d4est_hip_mgmatrix.hip: `int rows = 64; while (rows > 8 && n_elem * ceil(N3 / rows) < 4096) rows >>= 1;`
    per bucket; a wavefront then takes rows r and r + 4 per trip, r += 8, the second row guarded by rb < r1"""
    rows = 64
    while rows > 8 and n_elem * ((N3 + rows - 1) // rows) < 4096:
        rows >>= 1
    return rows


def last_chunk_rows(N3, rows):
    """rows of the last (possibly ragged) chunk"""
    return N3 - ((N3 + rows - 1) // rows - 1) * rows


def second_row_missing(n_rows):
    """does the LAST trip of a chunk of n_rows rows have a wavefront whose second row (r + 4) is cut off by the guard?  The waves
    w = 0 .. 3 of trip t hold rows 8 t + w and 8 t + w + 4: some second row is missing exactly when n_rows is no multiple of 8."""
    return n_rows % 8 != 0


def mass_cols_per_wg(n_elem, N3):
    """d4est_hip_compute_weighted_mass_blocks: `chunks = max(1, min(N3, ceil(4096 / n_elem))); cols = ceil(N3 / chunks);
    chunks = ceil(N3 / cols)` per bucket -> (cols, chunks)"""
    chunks = max(1, min(N3, (4096 + n_elem - 1) // n_elem))
    cols = (N3 + chunks - 1) // chunks
    return cols, (N3 + cols - 1) // cols


def galerkin_split(n, max_n3):
    """d4est_hip_transfer_galerkin_blocks: `per = max(1, min(n3, ceil(4096 / n))); rows = ceil(n3 / per)` with n = n_children for the
    rows kernel and n = n_items for the two column kernels, n3 = the transfer-wide max_n^3 -> (rows or cols per workgroup, chunks)"""
    per = max(1, min(max_n3, (4096 + n - 1) // n))
    r = (max_n3 + per - 1) // per
    return r, (max_n3 + r - 1) // r


def galerkin_acc_in_lds(max_n3):
    """d4est_hip_transfer_galerkin_blocks: `acc_in_lds = 3 * n3 * sizeof(double) <= 160 * 1024`: galerkin_cols_kernel keeps the sum over
    the children in a third LDS field where it fits (max_n <= 18), in the output column itself otherwise"""
    return 3 * max_n3 * 8 <= 160 * 1024
