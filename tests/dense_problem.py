"""Independent numpy restatement of the problem functions csrc/d4est_hip_problem.hip evaluates on the device, in the reference's own loop
order (written from the formulas, citing lines only):

  compute_confAij / compute_confAij_sqr and the coefficients of the two power callbacks
      (src/Problems/TwoPunctures/two_punctures_fcns.h:180-320): the i, j, k, l loops with levi_civita, the eps rules, pow(psi0 psi0, 3.5)
  the Robin callbacks (two_punctures_fcns.h:612-673, src/Problems/ConstantDensityStar/constant_density_star_fcns.h:9-57)
  u_alpha, psi_fcn, rho_fcn (constant_density_star_fcns.h:88-111, :246-301)
  the boundary mortar coordinates (src/Mesh/d4est_mesh.c:514-640) from forest.py's numpy maps and mesh.py's brick

K2 also comes with a per-point forward error bound gamma * sum|terms| (k2_with_bound).
"""
import numpy as np

U = 2.0 ** -53


def levi_civita(a, b, c):
    if (a, b, c) in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
        return 1.0
    if (a, b, c) in ((1, 0, 2), (0, 2, 1), (2, 1, 0)):
        return -1.0
    return 0.0


def split_puncture_params(params):
    p = np.asarray(params, dtype=np.float64)
    n = int(p[0])
    t = p[2:2 + 10 * n].reshape(n, 10)
    return n, float(p[1]), t[:, 0:3], t[:, 3:6], t[:, 6:9], t[:, 9]


def conf_aij(i, j, x, y, z, params, absolute=False):
    """compute_confAij (:180-228) for arrays of points; absolute=True: the same sum with every term replaced by its magnitude (the
    sum|terms| of the error bound)"""
    n_p, eps, C, P, S, M = split_puncture_params(params)
    ab = np.abs if absolute else (lambda v: v)
    x, y, z = (np.asarray(a, dtype=np.float64) for a in (x, y, z))
    out = np.zeros_like(x)
    with np.errstate(all="ignore"):
        for n in range(n_p):
            d = [x - C[n, 0], y - C[n, 1], z - C[n, 2]]
            rn = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
            rn = np.where(rn == 0., rn + eps, rn)                       # :202-203
            nv = [d[0] / rn, d[1] / rn, d[2] / rn]
            s_ij = np.zeros_like(x)
            s_ji = np.zeros_like(x)
            pn = np.zeros_like(x)
            for k in range(3):
                pn = pn + ab(P[n, k] * nv[k])
                for l in range(3):
                    s_ij = s_ij + ab(levi_civita(i, k, l) * S[n, k] * nv[l] * nv[j])
                    s_ji = s_ji + ab(levi_civita(j, k, l) * S[n, k] * nv[l] * nv[i])
            kron = 1.0 if i == j else 0.0
            if absolute:
                a = np.abs(nv[i] * P[n, j]) + np.abs(nv[j] * P[n, i]) + (kron + np.abs(nv[i] * nv[j])) * pn
            else:
                a = nv[i] * P[n, j] + nv[j] * P[n, i] - (kron - nv[i] * nv[j]) * pn
            b = s_ij + s_ji
            out = out + (1. / (rn * rn)) * (a + (2. / rn) * b)
        return out * (3. / 2.)


def conf_aij_sqr(x, y, z, params):
    """compute_confAij_sqr (:230-248)"""
    out = np.zeros_like(np.asarray(x, dtype=np.float64))
    with np.errstate(all="ignore"):
        for i in range(3):
            for j in range(3):
                a = conf_aij(i, j, x, y, z, params)
                out = out + a * a
    return out


# Longest path of one A_ij, in roundings (each <= u relative to the magnitude sum): d = x - C (1), r (3 products / sums + sqrt: 5), n = d / r
# (1), one term S n n of the 18 (3), their sums (9 + 1), 2 / r and its product (2), a + ... (1), 1 / (r r) and its product (3), the sum
# over <= 9 punctures (9), 3/2 (1): 36.  Squaring doubles it and adds one (73), the sum over the nine (i, j) adds 9: 82.  The device
# takes another order of the same terms, bounded by the same count, so the two results differ by at most 2 * 82 u sum|terms|.
K2_GAMMA = 2 * 82 * U


def k2_with_bound(x, y, z, params):
    """(K2, bound): |K2_any_order - K2| <= bound = K2_GAMMA * sum_ij (sum|terms of A_ij|)^2 per point"""
    k2 = conf_aij_sqr(x, y, z, params)
    s = np.zeros_like(k2)
    with np.errstate(all="ignore"):
        for i in range(3):
            for j in range(3):
                a = conf_aij(i, j, x, y, z, params, absolute=True)
                s = s + a * a
    return k2, K2_GAMMA * s


def _mass_sum(x, y, z, params):
    n_p, eps, C, P, S, M = split_puncture_params(params)
    x, y, z = (np.asarray(a, dtype=np.float64) for a in (x, y, z))
    s = np.zeros_like(x)
    r = np.zeros_like(x)
    with np.errstate(all="ignore"):
        for n in range(n_p):
            dx, dy, dz = x - C[n, 0], y - C[n, 1], z - C[n, 2]
            r = np.sqrt(dx * dx + dy * dy + dz * dz)
            s = s + M[n] / (2. * r)
    return s, r, eps


def puncture_b(x, y, z, params):
    """1 + sum_n m_n / (2 r_n) (:263-274): psi_0 = b + u"""
    return 1. + _mass_sum(x, y, z, params)[0]


def puncture_a(x, y, z, params):
    """-K2 / 8 where the r of the LAST puncture exceeds puncture_eps, else 0 (:264-283)"""
    _, r, eps = _mass_sum(x, y, z, params)
    return np.where(r > eps, (-1. / 8.) * conf_aij_sqr(x, y, z, params), 0.)


def neg_1o8_k2_psi_neg7(x, y, z, u, params):
    """two_punctures_neg_1o8_K2_psi_neg7 (:252-284) with pow(psi0 psi0, 3.5)"""
    s, r, eps = _mass_sum(x, y, z, params)
    psi0 = 1. + u + s
    with np.errstate(all="ignore"):
        return np.where(r > eps, (-1. / 8.) * conf_aij_sqr(x, y, z, params) / np.power(psi0 * psi0, 3.5), 0.)


def split_cds_params(params):
    cx, cy, cz, R, rho0, C0, alpha, beta = (float(v) for v in params)
    return cx, cy, cz, R, rho0, C0, alpha, beta


def u_alpha(x, y, z, params):
    cx, cy, cz, R, rho0, C0, alpha, beta = split_cds_params(params)
    dx, dy, dz = x - cx, y - cy, z - cz
    r2 = dx * dx + dy * dy + dz * dz
    return np.sqrt(alpha * R) / np.sqrt(r2 + alpha * R * alpha * R)


def cds_psi(x, y, z, params):
    cx, cy, cz, R, rho0, C0, alpha, beta = split_cds_params(params)
    x, y, z = (np.asarray(a, dtype=np.float64) for a in (x, y, z))
    dx, dy, dz = x - cx, y - cy, z - cz
    r2 = dx * dx + dy * dy + dz * dz
    with np.errstate(all="ignore"):
        return np.where(r2 > R * R, 1. + beta / np.sqrt(r2), C0 * u_alpha(x, y, z, params))


def cds_rho(x, y, z, params):
    cx, cy, cz, R, rho0, C0, alpha, beta = split_cds_params(params)
    dx, dy, dz = x - cx, y - cy, z - cz
    r2 = dx * dx + dy * dy + dz * dz
    return np.where(r2 > R * R, 0., rho0)


def cds_a(x, y, z, params):
    return (-2. * np.pi) * cds_rho(x, y, z, params)


def inv_r(x, y, z):
    r2 = x * x + y * y + z * z
    with np.errstate(all="ignore"):
        return 1 / np.sqrt(r2)


def robin_coeff_brick(x, y, z, normal):
    """two_punctures_robin_coeff_brick_fcn (:612-638); normal[3, n]"""
    r2 = x * x + y * y + z * z
    return np.where(np.abs(normal[0]) > 0., normal[0] * x / r2, np.where(np.abs(normal[1]) > 0., normal[1] * y / r2, normal[2] * z / r2))


FIELDS = {"PUNCTURE_K2": conf_aij_sqr, "PUNCTURE_A": puncture_a, "PUNCTURE_B": puncture_b, "CDS_A": cds_a, "CDS_PSI": cds_psi,
          "INV_R": lambda x, y, z, params=None: inv_r(x, y, z)}


# ---- coordinates ---------------------------------------------------------------------------------------------------------------------
def _quad_nodes(quad_type, deg_quad):
    from disco4est_amd import capi
    return capi.table("gauss_nodes" if quad_type == 0 else "lobatto_nodes", deg_quad)


def _tensor_ref(t):
    n = t.size
    ref = np.empty((n, n, n, 3))
    ref[..., 0] = t[None, None, :]
    ref[..., 1] = t[None, :, None]
    ref[..., 2] = t[:, None, None]
    return ref.reshape(-1, 3)


def _face_ref(f, t):
    d, sgn = f // 2, (1.0 if f % 2 else -1.0)
    ax = [a for a in range(3) if a != d]
    n = t.size
    ref = np.zeros((n * n, 3))
    ref[:, d] = sgn
    ref[:, ax[0]] = np.tile(t, n)
    ref[:, ax[1]] = np.repeat(t, n)
    return ref


def brick_point(q, dq, root_len, extents, ref):
    """the single-tree brick at reference points ref[n, 3] of the cell (q, dq)"""
    ex = np.asarray(extents, dtype=np.float64)
    xi = (np.asarray(q, dtype=np.float64)[None, :] + 0.5 * dq * (ref + 1.0)) / root_len
    return ex[0::2][None, :] + (ex[1::2] - ex[0::2])[None, :] * xi


def _point_fn(m, extents):
    """x(e, ref) of a mesh: forest.ForestMesh through its numpy map, a mesh.py brick through brick_point"""
    tree, q, dq = m.cells()
    if extents is not None:
        return lambda e, ref: brick_point(q[e], dq[e], m.root_len, extents, ref)
    return lambda e, ref: m.mapping.x(int(tree[e]), m._cell_xi(m.org[e], m.size[e], ref))


def quad_xyz(m, extents=None):
    """x, y, z at the quadrature nodes of every element (quad_stride layout): [3, local_nodes_quad]"""
    out = np.empty((3, m.local_nodes_quad))
    fn = _point_fn(m, extents)
    for e in range(m.n_elements):
        pq = int(m.deg_quad[e])
        X = fn(e, _tensor_ref(_quad_nodes(m.quad_type, pq)))
        s = int(m.quad_stride[e])
        out[:, s:s + (pq + 1) ** 3] = X.T
    return out


def boundary_xyz(m, sides, extents=None, fill=np.nan):
    """x, y, z at the mortar quadrature nodes of every boundary side, indexed like sj: [3, total_mortar_nodes] (d4est_mesh.c:604-625:
    the map AT the face's quadrature points); the other sides' entries hold `fill`"""
    out = np.full((3, int(sides["total_mortar_nodes"])), fill)
    fn = _point_fn(m, extents)
    for s in range(6 * m.n_elements):
        if sides["side_nbr"][s] != -1:
            continue
        e, f = divmod(s, 6)
        pq = int(m.deg_quad[e])
        X = fn(e, _face_ref(f, _quad_nodes(m.quad_type, pq)))
        S = int(sides["side_mortar_stride"][s])
        out[:, S:S + (pq + 1) ** 2] = X.T
    return out
