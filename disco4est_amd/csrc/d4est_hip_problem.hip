// Problem data of the reference's shipped nonlinear drivers evaluated on the device: the puncture and star source fields by id, the
// power term set on a plan from forest coordinates in one kernel, the boundary mortar coordinates and Robin data by id.
//
// Replaces, per mesh change:
//   compute_confAij / compute_confAij_sqr and the coefficients of two_punctures_neg_1o8_K2_psi_neg7 / _plus_7o8_K2_psi_neg8
//                                                  (src/Problems/TwoPunctures/two_punctures_fcns.h:180-320)
//   two_punctures_robin_coeff_brick_fcn / _sphere_fcn / _robin_bc_rhs_fcn                          (two_punctures_fcns.h:612-673)
//   the three Robin callbacks, u_alpha, psi_fcn, rho_fcn and the coefficient of the power callbacks
//                                                  (src/Problems/ConstantDensityStar/constant_density_star_fcns.h:9-57, :88-111, :246-357)
//   xyz_m_mortar_quad on boundary faces            (src/Mesh/d4est_mesh.c:514-640; consumer src/dGMath/d4est_laplacian_flux.c:47-112, :200-204)
//
// Design (gfx950): the fields are a few hundred flops per point and read three doubles, so every kernel here is one thread per point
// with the parameters in the kernel argument segment (scalar loads, wave-uniform loops over the punctures).  The term kernel gets the
// point from the element's cell description and the 1-D abscissae -- no coordinate array -- and writes a and b straight into the
// plan-owned arrays of d4est_hip_nonlinear.hip.  Everything below the includes is compiled with floating-point contraction OFF: a
// field's bits then do not depend on which kernel it was inlined into, which is what lets the one-kernel term equal
// d4est_hip_field_eval on d4est_hip_plan_compute_xyz_* bit for bit.  (The tree maps of d4est_hip_maps.h keep the contraction they have
// in every other unit: the coordinates equal those of d4est_hip_plan_compute_xyz_analytic.)
#include <algorithm>
#include <cmath>
#include <vector>

#include "d4est_hip_internal.h"
#include "d4est_hip_maps.h"
#include "d4est_hip_pointwise.h"

#pragma clang fp contract(off)

namespace d4est_hip {

constexpr int kFieldParamsMax = 2 + 10 * (D4EST_HIP_MAX_PUNCTURES - 1);

struct FieldParams {
  int n_punctures;
  int pad;
  double p[kFieldParamsMax];
};

// ---- the fields ------------------------------------------------------------------------------------------------------------------
// puncture params: p[0] = num_punctures, p[1] = puncture_eps, puncture n at p + 2 + 10 n: C[3], P[3], S[3], M

// sum_ij (3/2 A_ij)^2 (two_punctures_fcns.h:180-248) from the six independent components of the symmetric A_ij
__device__ __forceinline__ double puncture_k2(const FieldParams& F, double x, double y, double z) {
  const double eps = F.p[1];
  double A00 = 0., A01 = 0., A02 = 0., A11 = 0., A12 = 0., A22 = 0.;
  for (int n = 0; n < F.n_punctures; ++n) {
    const double* q = F.p + 2 + 10 * n;
    const double dx = x - q[0], dy = y - q[1], dz = z - q[2];
    double r = sqrt(dx * dx + dy * dy + dz * dz);
    if (r == 0.) r += eps;                                     // :202-203
    const double n0 = dx / r, n1 = dy / r, n2 = dz / r;
    const double P0 = q[3], P1 = q[4], P2 = q[5], S0 = q[6], S1 = q[7], S2 = q[8];
    const double Pn = P0 * n0 + P1 * n1 + P2 * n2;
    const double w0 = S1 * n2 - S2 * n1, w1 = S2 * n0 - S0 * n2, w2 = S0 * n1 - S1 * n0;   // S x n = eps_ikl S_k n_l
    const double ir2 = 1. / (r * r), tr = 2. / r;
    A00 += ir2 * ((n0 * P0 + n0 * P0 - (1. - n0 * n0) * Pn) + tr * (w0 * n0 + w0 * n0));
    A11 += ir2 * ((n1 * P1 + n1 * P1 - (1. - n1 * n1) * Pn) + tr * (w1 * n1 + w1 * n1));
    A22 += ir2 * ((n2 * P2 + n2 * P2 - (1. - n2 * n2) * Pn) + tr * (w2 * n2 + w2 * n2));
    A01 += ir2 * ((n0 * P1 + n1 * P0 + n0 * n1 * Pn) + tr * (w0 * n1 + w1 * n0));
    A02 += ir2 * ((n0 * P2 + n2 * P0 + n0 * n2 * Pn) + tr * (w0 * n2 + w2 * n0));
    A12 += ir2 * ((n1 * P2 + n2 * P1 + n1 * n2 * Pn) + tr * (w1 * n2 + w2 * n1));
  }
  A00 *= 1.5; A01 *= 1.5; A02 *= 1.5; A11 *= 1.5; A12 *= 1.5; A22 *= 1.5;   // :226
  return (A00 * A00 + A11 * A11 + A22 * A22) + 2. * (A01 * A01 + A02 * A02 + A12 * A12);
}

// sum_n m_n / (2 r_n) and the r the reference's test reads: that of the LAST puncture (:264-277)
__device__ __forceinline__ double puncture_mass_sum(const FieldParams& F, double x, double y, double z, double& r_last) {
  double sum = 0., r = 0.;
  for (int n = 0; n < F.n_punctures; ++n) {
    const double* q = F.p + 2 + 10 * n;
    const double dx = x - q[0], dy = y - q[1], dz = z - q[2];
    r = sqrt(dx * dx + dy * dy + dz * dz);
    sum += q[9] / (2. * r);
  }
  r_last = r;
  return sum;
}

__device__ __forceinline__ double puncture_a(const FieldParams& F, double x, double y, double z) {
  double r_last;
  (void)puncture_mass_sum(F, x, y, z, r_last);
  const double k2 = puncture_k2(F, x, y, z);
  return r_last > F.p[1] ? (-1. / 8.) * k2 : 0.;
}

__device__ __forceinline__ double puncture_b(const FieldParams& F, double x, double y, double z) {
  double r_last;
  return 1. + puncture_mass_sum(F, x, y, z, r_last);
}

// star params: p = {cx, cy, cz, R, rho0, C0, alpha, beta}
__device__ __forceinline__ double cds_r2(const FieldParams& F, double x, double y, double z) {
  const double dx = x - F.p[0], dy = y - F.p[1], dz = z - F.p[2];
  return dx * dx + dy * dy + dz * dz;
}

__device__ __forceinline__ double cds_a(const FieldParams& F, double x, double y, double z) {
  const double kPi = 3.14159265358979323846;
  const double R = F.p[3];
  const double rho = cds_r2(F, x, y, z) > R * R ? 0. : F.p[4];   // constant_density_star_fcns.h:295-300
  return (-2. * kPi) * rho;                                       // :356
}

__device__ __forceinline__ double cds_psi(const FieldParams& F, double x, double y, double z) {
  const double R = F.p[3], C0 = F.p[5], alpha = F.p[6], beta = F.p[7];
  const double r2 = cds_r2(F, x, y, z);
  if (r2 > R * R) return 1. + beta / sqrt(r2);                                   // :269-270
  return C0 * (sqrt(alpha * R) / sqrt(r2 + alpha * R * alpha * R));              // :272 with :110
}

__device__ __forceinline__ double inv_r(double x, double y, double z) {
  const double r2 = x * x + y * y + z * z;
  return 1 / sqrt(r2);
}

// ---- the fields of the remaining problem families ------------------------------------------------------------------------------------
// okendon_analytic_solution, the DIM == 3 branch (src/Problems/Okendon/okendon_fcns.h:70-96); params {p}
__device__ __forceinline__ double okendon_u(const FieldParams& F, double x, double y, double z) {
  const double p = F.p[0];
  const double M = 1. / (pow((2. / (1. - p)) * (1 + (2. / (1. - p))), (1. / (1. - p))));
  const double r2 = x * x + y * y + z * z;
  return M * pow(r2, 1 / (1 - p));
}

// boyen_york_model_analytic_solution (src/Problems/BoyenYorkModel/boyen_york_model_fcns.h:67-95); params {a, P}
__device__ __forceinline__ double by_psi(const FieldParams& F, double x, double y, double z) {
  const double r2 = x * x + y * y + z * z;
  const double r = sqrt(r2);
  const double r3 = r * r2;
  const double r4 = r2 * r2;
  const double a = F.p[0], P = F.p[1];
  const double E = sqrt(P * P + 4 * a * a);
  const double t1 = 1.;
  const double t2 = 2. * E / r;
  const double t3 = 6 * a * a / (r2);
  const double t4 = 2 * a * a * E / (r3);
  const double t5 = a * a * a * a / (r4);
  return pow((t1 + t2 + t3 + t4 + t5), .25);
}

// boyen_york_model_helmholtz_fcn (:110-128)
__device__ __forceinline__ double by_a(const FieldParams& F, double x, double y, double z) {
  const double a = F.p[0], P = F.p[1];
  const double r2 = x * x + y * y + z * z;
  const double r4 = r2 * r2;
  const double a2 = a * a;
  const double P2 = P * P;
  return .75 * (P2 / r4) * (1 - (a2 / r2)) * (1 - (a2 / r2));
}

// poisson_lorentzian_analytic_solution / _rhs_fcn / _robin_coeff_fcn (src/Problems/Poisson/poisson_lorentzian_fcns.h:55-67, :71-82, :22-36)
__device__ __forceinline__ double lorentzian_u(double x, double y, double z) {
  const double r = sqrt(x * x + y * y + z * z);
  return 1. / sqrt(1. + r * r);
}
__device__ __forceinline__ double lorentzian_rhs(double x, double y, double z) { return 3. / pow((1. + x * x + y * y + z * z), 2.5); }
__device__ __forceinline__ double lorentzian_robin(double x, double y, double z) {
  const double r2 = x * x + y * y + z * z;
  return sqrt(r2) / (1. + r2);
}

// stamm_analytic_solution, the DIM == 3 branch (src/Problems/Stamm/stamm_fcns.h:78-114); params {c2x, c2y, c2z}.
// d4est_util_dbl_pow_int(rp, 3) is (rp rp) rp (src/Utilities/d4est_util.c:157-185)
__device__ __forceinline__ double stamm_u(const FieldParams& F, double x, double y, double z) {
  const double xp = x - F.p[0], yp = y - F.p[1], zp = z - F.p[2];
  const double rp = sqrt(xp * xp + yp * yp + zp * zp);
  return x * (1. - x) * y * (1. - y) * z * (1. - z) * ((rp * rp) * rp);
}

// stamm_rhs_fcn, the DIM == 3 branch (:149-208), term by term in the reference's order; S = |c2 - x|^2, pow_int(., 2) is one product
__device__ __forceinline__ double stamm_rhs(const FieldParams& F, double x, double y, double z) {
  const double c2x = F.p[0], c2y = F.p[1], c2z = F.p[2];
  if (x == c2x && y == c2y && z == c2z) return 0.;
  const double dx2 = (c2x - x) * (c2x - x), dy2 = (c2y - y) * (c2y - y), dz2 = (c2z - z) * (c2z - z);
  const double S = dx2 + dy2 + dz2;
  const double S2 = S * S;
  double ret = (-2 * (1 - x) * x * (1 - y) * y * S2 +
                9 * (1 - x) * x * (1 - y) * y * S * (1 - z) * z +
                6 * (1 - x) * (-c2x + x) * (1 - y) * y * S * (1 - z) * z -
                6 * x * (-c2x + x) * (1 - y) * y * S * (1 - z) * z +
                6 * (1 - x) * x * (1 - y) * (-c2y + y) * S * (1 - z) * z -
                6 * (1 - x) * x * y * (-c2y + y) * S * (1 - z) * z -
                2 * (1 - x) * x * S2 * (1 - z) * z -
                2 * (1 - y) * y * S2 * (1 - z) * z -
                3 * dx2 * (-1 + x) * x * (-1 + y) * y * (-1 + z) * z -
                3 * (-1 + x) * x * dy2 * (-1 + y) * y * (-1 + z) * z -
                3 * (-1 + x) * x * (-1 + y) * y * dz2 * (-1 + z) * z +
                6 * (1 - x) * x * (1 - y) * y * S * (1 - z) * (-c2z + z) -
                6 * (1 - x) * x * (1 - y) * y * S * z * (-c2z + z)) /
               sqrt(S);
  ret *= -1;
  return ret;
}

__device__ __forceinline__ double field_value(int id, const FieldParams& F, double x, double y, double z) {
  switch (id) {   // wave-uniform
    case D4EST_HIP_FIELD_PUNCTURE_K2: return puncture_k2(F, x, y, z);
    case D4EST_HIP_FIELD_PUNCTURE_A: return puncture_a(F, x, y, z);
    case D4EST_HIP_FIELD_PUNCTURE_B: return puncture_b(F, x, y, z);
    case D4EST_HIP_FIELD_CDS_A: return cds_a(F, x, y, z);
    case D4EST_HIP_FIELD_CDS_PSI: return cds_psi(F, x, y, z);
    case D4EST_HIP_FIELD_OKENDON_U: return okendon_u(F, x, y, z);
    case D4EST_HIP_FIELD_BY_PSI: return by_psi(F, x, y, z);
    case D4EST_HIP_FIELD_BY_A: return by_a(F, x, y, z);
    case D4EST_HIP_FIELD_LORENTZIAN_U: return lorentzian_u(x, y, z);
    case D4EST_HIP_FIELD_LORENTZIAN_RHS: return lorentzian_rhs(x, y, z);
    case D4EST_HIP_FIELD_LORENTZIAN_ROBIN: return lorentzian_robin(x, y, z);
    case D4EST_HIP_FIELD_STAMM_U: return stamm_u(F, x, y, z);
    case D4EST_HIP_FIELD_STAMM_RHS: return stamm_rhs(F, x, y, z);
    default: return inv_r(x, y, z);
  }
}

__global__ __launch_bounds__(256) void field_eval_kernel(int id, FieldParams F, const double* __restrict__ xyz, long long n,
                                                         double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = field_value(id, F, xyz[i], xyz[n + i], xyz[2 * n + i]);
}

// ---- where a node is ---------------------------------------------------------------------------------------------------------------
struct CoordSrc {
  int kind;              // 0 brick, 1 analytic map, 2 the caller's coordinate array
  int pad;
  TreeMapParams P;
  const CellDesc* cells;
  double root_len;
  double x0[3], ex[3];   // brick: origin and extents
  const double* xyz;     // kind 2: x | y | z, components `total` apart
  size_t total;
};

// d4est_geometry_brick_X on one tree (src/Geometry/d4est_geometry_brick.c:119-149)
__device__ __forceinline__ void brick_x(const CoordSrc& S, const CellDesc& cell, const double r[3], double x[3]) {
  for (int d = 0; d < 3; ++d) {
    const double xi = ((double)cell.q[d] + 0.5 * (double)cell.dq * (r[d] + 1.0)) / S.root_len;
    x[d] = S.x0[d] + S.ex[d] * xi;
  }
}

__device__ __forceinline__ void cell_point(const CoordSrc& S, const CellDesc& cell, const double r[3], double x[3]) {
  if (S.kind == 0) brick_x(S, cell, r, x);
  else cell_x(S.P, cell, S.root_len, r, x);
}

// up to MAXB degree buckets of a plan in one launch: bucket j serves the entries [elem_end[j-1], elem_end[j]) of the plan's
// bucket-ordered element lists, Nn nodes per direction at nodes + node_off[j]
struct BucketList {
  static constexpr int MAXB = 16;
  int n;
  int first;             // entry of the element lists the launch starts at
  int elem_end[MAXB];
  int Nn[MAXB];
  int node_off[MAXB];
};

// one workgroup per element, one thread per node; mode 0: coordinates (x | y | z, `total` apart) into out_a; mode 1: the puncture
// term's a and b; mode 2: the star term's a; mode 3: the Okendon term's a; mode 4: the Boyen-York term's a
__global__ __launch_bounds__(128) void node_kernel(int mode, CoordSrc S, BucketList B, const int* __restrict__ elem_ids,
                                                   const int* __restrict__ s_list, const double* __restrict__ nodes, FieldParams F,
                                                   double* __restrict__ out_a, double* __restrict__ out_b, size_t total) {
  const int n_entries = B.elem_end[B.n - 1] - B.first;
  for (int i = blockIdx.x; i < n_entries; i += gridDim.x) {
    const int ei = B.first + i;
    int bi = 0;
    while (bi + 1 < B.n && ei >= B.elem_end[bi]) ++bi;
    const int Nn = B.Nn[bi], N3 = Nn * Nn * Nn;
    const double* t = nodes + B.node_off[bi];
    const size_t s0 = (size_t)s_list[ei];
    CellDesc cell = {};
    if (S.kind != 2) cell = S.cells[elem_ids[ei]];
    for (int n = threadIdx.x; n < N3; n += blockDim.x) {
      double x[3];
      if (S.kind == 2) {
        x[0] = S.xyz[s0 + n]; x[1] = S.xyz[S.total + s0 + n]; x[2] = S.xyz[2 * S.total + s0 + n];
      } else {
        const double r[3] = {t[n % Nn], t[(n / Nn) % Nn], t[n / (Nn * Nn)]};
        cell_point(S, cell, r, x);
      }
      if (mode == 0) {
        out_a[s0 + n] = x[0]; out_a[total + s0 + n] = x[1]; out_a[2 * total + s0 + n] = x[2];
      } else if (mode == 1) {
        out_a[s0 + n] = puncture_a(F, x[0], x[1], x[2]);
        out_b[s0 + n] = puncture_b(F, x[0], x[1], x[2]);
      } else if (mode == 2) {
        out_a[s0 + n] = cds_a(F, x[0], x[1], x[2]);
      } else if (mode == 3) {
        out_a[s0 + n] = 1.;   // okendon_build_residual adds + V^T W J |u|^p to A u (okendon_fcns.h:377-403)
      } else {
        out_a[s0 + n] = by_a(F, x[0], x[1], x[2]);
      }
    }
  }
}

// a boundary side: its element and face, the offset S of its mortar nodes (side_mortar_stride), NQ nodes per direction at nodes + node_off
struct BoundaryUnit {
  int elem, face, S, NQ, node_off, pad;
};

// the reference point of face node (ta, tb): the face's two axes in increasing order, the first fastest
__device__ __forceinline__ void face_point(int f, double ta, double tb, double r[3]) {
  const int dir = f >> 1;
  r[dir] = (f & 1) ? 1.0 : -1.0;
  r[dir == 0 ? 1 : 0] = ta;
  r[dir == 2 ? 1 : 2] = tb;
}

// one workgroup per boundary side, one thread per mortar node.  mode 0: x | y | z (`total` apart) into out_a; mode 1: sj coeff into
// out_a, sj rhs into out_b
__global__ __launch_bounds__(64) void boundary_kernel(int mode, int coeff_id, int rhs_id, CoordSrc S,
                                                      const BoundaryUnit* __restrict__ units, int n_units,
                                                      const double* __restrict__ nodes, const double* __restrict__ sj,
                                                      double* __restrict__ out_a, double* __restrict__ out_b, size_t total) {
  for (int ui = blockIdx.x; ui < n_units; ui += gridDim.x) {
    const BoundaryUnit un = units[ui];
    const CellDesc cell = S.cells[un.elem];
    const double* t = nodes + un.node_off;
    const int T = un.NQ * un.NQ;
    for (int k = threadIdx.x; k < T; k += blockDim.x) {
      double r[3], x[3];
      face_point(un.face, t[k % un.NQ], t[k / un.NQ], r);
      cell_point(S, cell, r, x);
      const size_t at = (size_t)un.S + k;
      if (mode == 0) {
        out_a[at] = x[0]; out_a[total + at] = x[1]; out_a[2 * total + at] = x[2];
        continue;
      }
      double c;
      if (coeff_id == D4EST_HIP_ROBIN_COEFF_BRICK) {   // two_punctures_fcns.h:626-633 with n = sign(f) e_axis
        const int dir = un.face >> 1;
        const double r2 = x[0] * x[0] + x[1] * x[1] + x[2] * x[2];
        const double xa = dir == 0 ? x[0] : dir == 1 ? x[1] : x[2];
        c = (((un.face & 1) ? 1.0 : -1.0) * xa) / r2;
      } else if (coeff_id == D4EST_HIP_ROBIN_COEFF_LORENTZIAN) {
        c = lorentzian_robin(x[0], x[1], x[2]);
      } else {
        c = inv_r(x[0], x[1], x[2]);
      }
      const double rhs = rhs_id == D4EST_HIP_ROBIN_RHS_INV_R ? inv_r(x[0], x[1], x[2]) : 0.;
      out_a[at] = sj[at] * c;      // the products of faces_set_robin's kernel
      out_b[at] = sj[at] * rhs;
    }
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
static FieldParams field_params(int field_id, const double* params, int n_params, const char* who) {
  FieldParams F = {};
  if (field_id < D4EST_HIP_FIELD_PUNCTURE_K2 || field_id > D4EST_HIP_FIELD_STAMM_RHS) D4EST_HIP_ABORT("%s: unknown field id %d", who, field_id);
  if (field_id == D4EST_HIP_FIELD_INV_R || (field_id >= D4EST_HIP_FIELD_LORENTZIAN_U && field_id <= D4EST_HIP_FIELD_LORENTZIAN_ROBIN)) return F;
  if (!params) D4EST_HIP_ABORT("%s: params is NULL", who);
  if (field_id == D4EST_HIP_FIELD_OKENDON_U) {
    if (n_params != 1 || !(params[0] > 0. && params[0] < 1.))   // okendon_params_init asserts the range (okendon_fcns.h:65)
      D4EST_HIP_ABORT("%s: the Okendon field takes the 1 param {p}, 0 < p < 1; n_params = %d", who, n_params);
  } else if (field_id == D4EST_HIP_FIELD_BY_PSI || field_id == D4EST_HIP_FIELD_BY_A) {
    if (n_params != 2) D4EST_HIP_ABORT("%s: the Boyen-York fields take the 2 params {a, P}, n_params = %d", who, n_params);
  } else if (field_id >= D4EST_HIP_FIELD_STAMM_U) {
    if (n_params != 3) D4EST_HIP_ABORT("%s: the Stamm fields take the 3 params {c2x, c2y, c2z}, n_params = %d", who, n_params);
  } else if (field_id <= D4EST_HIP_FIELD_PUNCTURE_B) {
    if (n_params < 2) D4EST_HIP_ABORT("%s: the puncture fields take {num_punctures, puncture_eps, per puncture C[3], P[3], S[3], M}", who);
    if (!(params[0] >= 1. && params[0] < (double)D4EST_HIP_MAX_PUNCTURES) || params[0] != std::floor(params[0]))
      D4EST_HIP_ABORT("%s: num_punctures = %g (1 .. %d)", who, params[0], D4EST_HIP_MAX_PUNCTURES - 1);
    const int np = (int)params[0];
    if (n_params != 2 + 10 * np) D4EST_HIP_ABORT("%s: n_params = %d for %d punctures (2 + 10 num_punctures)", who, n_params, np);
    F.n_punctures = np;
  } else if (n_params != 8) {
    D4EST_HIP_ABORT("%s: the star fields take the 8 params {cx, cy, cz, R, rho0, C0, alpha, beta}, n_params = %d", who, n_params);
  }
  std::copy(params, params + n_params, F.p);
  return F;
}

static std::vector<CellDesc> brick_cells(const d4est_hip_plan* plan, const int* elem_q, const int* elem_dq, double root_len,
                                         const double* extents, const char* who) {
  if (plan->n_elements > 0 && (!elem_q || !elem_dq)) D4EST_HIP_ABORT("%s: NULL element array", who);
  if (!extents || !(root_len > 0.) || !(extents[1] > extents[0]) || !(extents[3] > extents[2]) || !(extents[5] > extents[4]))
    D4EST_HIP_ABORT("%s: bad brick extents / root length", who);
  std::vector<CellDesc> c((size_t)plan->n_elements);
  for (int e = 0; e < plan->n_elements; ++e) {
    if (elem_dq[e] <= 0) D4EST_HIP_ABORT("%s: element %d has dq %d", who, e, elem_dq[e]);
    c[e] = CellDesc{0, {elem_q[3 * e], elem_q[3 * e + 1], elem_q[3 * e + 2]}, elem_dq[e], 0};
  }
  return c;
}

static std::vector<CellDesc> analytic_cells(const d4est_hip_plan* plan, int geom_type, const int* tree, const int* q, const int* dq,
                                            double root_len, const char* who) {
  if (plan->n_elements > 0 && (!tree || !q || !dq)) D4EST_HIP_ABORT("%s: NULL element array", who);
  if (!(root_len > 0.)) D4EST_HIP_ABORT("%s: root_len", who);
  const int max_tree = tree_map_num_trees(geom_type) - 1;
  std::vector<CellDesc> c((size_t)plan->n_elements);
  for (int e = 0; e < plan->n_elements; ++e) {
    if (tree[e] < 0 || tree[e] > max_tree || dq[e] <= 0) D4EST_HIP_ABORT("%s: element %d has tree %d / dq %d", who, e, tree[e], dq[e]);
    c[e] = CellDesc{tree[e], {q[3 * e], q[3 * e + 1], q[3 * e + 2]}, dq[e], 0};
  }
  return c;
}

static CoordSrc brick_src(double root_len, const double* extents) {
  CoordSrc S = {};
  S.kind = 0;
  S.root_len = root_len;
  for (int d = 0; d < 3; ++d) { S.x0[d] = extents[2 * d]; S.ex[d] = extents[2 * d + 1] - extents[2 * d]; }
  return S;
}

static CoordSrc analytic_src(int geom_type, const double* geom_params, double root_len, const char* who) {
  CoordSrc S = {};
  S.kind = 1;
  S.root_len = root_len;
  d4est_hipi_tree_map_params(geom_type, geom_params, who, &S.P);
  return S;
}

// node_kernel over every bucket of the plan: which = 0 the Lobatto nodes (nodal_stride), 1 the quadrature nodes (quad_stride)
static void launch_nodes(d4est_hip_plan* plan, int mode, CoordSrc S, const NodeTables* nt, int which, const FieldParams& F, double* out_a,
                         double* out_b) {
  const size_t total = (size_t)(which ? plan->local_nodes_quad : plan->local_nodes);
  const int* s_list = which ? plan->d_qs_list : plan->d_ns_list;
  BucketList B = {};
  auto flush = [&]() {
    if (B.n == 0) return;
    const int n_entries = B.elem_end[B.n - 1] - B.first;
    if (n_entries > 0)
      hipLaunchKernelGGL(node_kernel, dim3(std::min(n_entries, 1 << 20)), dim3(128), 0, plan->stream, mode, S, B, plan->d_elem_ids, s_list,
                         nt ? nt->d_nodes : nullptr, F, out_a, out_b, total);
    B = BucketList{};
  };
  for (size_t bi = 0; bi < plan->buckets.size(); ++bi) {   // the buckets are consecutive ranges of the bucket-ordered lists
    const Bucket& bk = plan->buckets[bi];
    if (bk.n_elem == 0) continue;
    if (B.n > 0 && B.elem_end[B.n - 1] != bk.elem_offset) flush();
    if (B.n == 0) B.first = bk.elem_offset;
    const int j = B.n++;
    B.elem_end[j] = bk.elem_offset + bk.n_elem;
    B.Nn[j] = which ? bk.NQ : bk.N;
    B.node_off[j] = nt ? (int)(2 * bi + which) * nt->stride : 0;
    if (B.n == BucketList::MAXB) flush();
  }
  flush();
  HIP_CHECK(hipGetLastError());
}

// the problem families with a term setter: node_kernel's mode
enum Term { kTermPuncture = 1, kTermCds = 2, kTermOkendon = 3, kTermBoyenYork = 4 };

static void set_term(d4est_hip_plan* plan, Term term, const double* params, int n_params, CoordSrc S,
                     const std::vector<CellDesc>* cells, const char* who) {
  const int field = term == kTermPuncture ? D4EST_HIP_FIELD_PUNCTURE_A : term == kTermCds ? D4EST_HIP_FIELD_CDS_A
                  : term == kTermOkendon ? D4EST_HIP_FIELD_OKENDON_U : D4EST_HIP_FIELD_BY_A;
  const FieldParams F = field_params(field, params, n_params, who);
  double *a = nullptr, *b = nullptr;
  if (term == kTermOkendon) nonlinear_term_arrays_real(plan, params[0], false, &a, &b);   // |u|^p: s = p
  else nonlinear_term_arrays(plan, term == kTermCds ? 5 : -7, term == kTermPuncture, &a, &b);
  if (plan->n_elements == 0) return;
  if (cells) {
    const NodeTables nt = stage_cells_and_nodes(plan, *cells);
    S.cells = nt.d_cells;
    launch_nodes(plan, term, S, &nt, 1, F, a, b);
  } else {
    launch_nodes(plan, term, S, nullptr, 1, F, a, b);
  }
}

static CoordSrc xyz_src(const d4est_hip_plan* plan, const double* xyz_quad_dev, const char* who) {
  if (!xyz_quad_dev && plan->local_nodes_quad > 0) D4EST_HIP_ABORT("%s: xyz_quad_dev is NULL", who);
  CoordSrc S = {};
  S.kind = 2;
  S.xyz = xyz_quad_dev;
  S.total = (size_t)plan->local_nodes_quad;
  return S;
}

// mode 0: coordinates into xyz_out; mode 1: the plan's Robin arrays
static void boundary_launch(d4est_hip_plan* plan, int mode, int coeff_id, int rhs_id, CoordSrc S, const std::vector<CellDesc>& cells,
                            double* xyz_out, const char* who) {
  if (!plan->has_faces) D4EST_HIP_ABORT("%s: call d4est_hip_plan_set_faces first", who);
  const double* sj = nullptr;
  double *out_a = xyz_out, *out_b = nullptr;
  if (mode == 1) {
    if (coeff_id != D4EST_HIP_ROBIN_COEFF_INV_R && coeff_id != D4EST_HIP_ROBIN_COEFF_BRICK && coeff_id != D4EST_HIP_ROBIN_COEFF_LORENTZIAN)
      D4EST_HIP_ABORT("%s: unknown coeff_id %d", who, coeff_id);
    if (rhs_id != D4EST_HIP_ROBIN_RHS_ZERO && rhs_id != D4EST_HIP_ROBIN_RHS_INV_R) D4EST_HIP_ABORT("%s: unknown rhs_id %d", who, rhs_id);
    if (coeff_id == D4EST_HIP_ROBIN_COEFF_BRICK && S.kind != 0)
      D4EST_HIP_ABORT("%s: ROBIN_COEFF_BRICK needs the brick source (the face normal is +-e_axis on a brick only)", who);
    sj = faces_sj(plan, who);
  } else if (!xyz_out && plan->total_mortar_nodes > 0) {
    D4EST_HIP_ABORT("%s: xyz_mortar_dev is NULL", who);
  }
  const NodeTables nt = stage_cells_and_nodes(plan, cells);
  S.cells = nt.d_cells;
  std::vector<int> bucket_of((size_t)plan->n_elements, 0);
  for (size_t bi = 0; bi < plan->buckets.size(); ++bi)
    for (int i = 0; i < plan->buckets[bi].n_elem; ++i) bucket_of[plan->elem_ids[plan->buckets[bi].elem_offset + i]] = (int)bi;
  std::vector<BoundaryUnit> units;
  for (int e = 0; e < plan->n_elements; ++e)
    for (int f = 0; f < 6; ++f) {
      const size_t s = 6 * (size_t)e + f;
      if (plan->side_nbr[s] != -1) continue;
      const int NQ = plan->deg_quad[e] + 1;   // a boundary side's mortar has the element's own quadrature degree
      const long long S0 = plan->side_mortar_stride[s];
      if (S0 < 0 || S0 + (long long)NQ * NQ > plan->total_mortar_nodes) D4EST_HIP_ABORT("%s: side %zu mortar data exceeds total_mortar_nodes", who, s);
      units.push_back(BoundaryUnit{e, f, (int)S0, NQ, (2 * bucket_of[e] + 1) * nt.stride, 0});
    }
  if (mode == 1) {   // every side is validated: now the boundary data changes what the operator computes
    plan_operator_changed(plan);
    faces_robin_arrays(plan, who, &out_a, &out_b);
  }
  if (units.empty()) return;
  BoundaryUnit* d_units = nullptr;
  HIP_CHECK(hipMalloc(&d_units, units.size() * sizeof(BoundaryUnit)));
  HIP_CHECK(hipMemcpy(d_units, units.data(), units.size() * sizeof(BoundaryUnit), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(boundary_kernel, dim3((unsigned)std::min<size_t>(units.size(), 1 << 20)), dim3(64), 0, plan->stream, mode, coeff_id, rhs_id, S,
                     d_units, (int)units.size(), nt.d_nodes, sj, out_a, out_b, (size_t)plan->total_mortar_nodes);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(plan->stream));
  HIP_CHECK(hipFree(d_units));
}

// ---- the load vector V^T W J f(x_quad) of a field id ----------------------------------------------------------------------------------
// The pointwise function of nonlin_body (d4est_hip_pointwise.h) without a forward half: the node's point from the element's cell
// description and the bucket's quadrature abscissae (or the caller's coordinates), then the field.  elem_ids and nodes are the
// launch's bucket's: entry ei of its element lists, NQ abscissae
struct LoadField {
  static constexpr bool kForward = false;
  int beta;
  int id;
  const int* elem_ids;
  const double* nodes;
  CoordSrc S;
  FieldParams F;
  __device__ __forceinline__ double term(int ei, int q, int a, int b, int kq, double) const {
    double x[3];
    if (S.kind == 2) {
      x[0] = S.xyz[q]; x[1] = S.xyz[S.total + q]; x[2] = S.xyz[2 * S.total + q];
    } else {
      const CellDesc cell = S.cells[elem_ids[ei]];
      const double r[3] = {nodes[a], nodes[b], nodes[kq]};
      cell_point(S, cell, r, x);
    }
    return field_value(id, F, x[0], x[1], x[2]);
  }
};

// out = beta out + V^T W J f(x_quad): one kernel per bucket where d4est_hip_apply_galerkin_integral has a one-kernel path (every
// bucket a built pair: plan_pairs_built, the nonlinear term's own condition), else coordinates, field_eval and the integral through
// plan-owned temporaries
static void build_load(d4est_hip_plan* plan, int field_id, const double* params, int n_params, CoordSrc S,
                       const std::vector<CellDesc>* cells, int beta, double* out, const char* who) {
  const FieldParams F = field_params(field_id, params, n_params, who);
  if (beta != 0 && beta != 1) D4EST_HIP_ABORT("%s: beta = %d (0 or 1)", who, beta);
  if (!out && plan->local_nodes > 0) D4EST_HIP_ABORT("%s: out_dev is NULL", who);
  if (!plan->has_geometry) D4EST_HIP_ABORT("%s: d4est_hip_plan_set_geometry was not called", who);
  if (plan->n_elements == 0 || plan->local_nodes == 0) return;
  NodeTables nt = {};
  if (cells) {
    nt = stage_cells_and_nodes(plan, *cells);
    S.cells = nt.d_cells;
  }
  if (plan_pairs_built(plan)) {
    for (size_t bi = 0; bi < plan->buckets.size(); ++bi) {
      const Bucket& bk = plan->buckets[bi];
      if (bk.n_elem == 0) continue;
      LoadField P = {};
      P.beta = beta;
      P.id = field_id;
      P.elem_ids = plan->d_elem_ids + bk.elem_offset;
      P.nodes = cells ? nt.d_nodes + (2 * bi + 1) * (size_t)nt.stride : nullptr;
      P.S = S;
      P.F = F;
      for_built_pair(bk.N, bk.NQ, [&](auto n, auto nq) {
        constexpr int N = decltype(n)::value, NQ = decltype(nq)::value;
        using C = WaveCfg<N, NQ>;
        set_lds_limit(nonlin_kernel<N, NQ, false, LoadField>, C::LDS_BYTES);
        hipLaunchKernelGGL((nonlin_kernel<N, NQ, false, LoadField>), dim3((bk.n_elem + C::EPB - 1) / C::EPB), dim3(C::THREADS), C::LDS_BYTES,
                           plan->stream, nullptr, out, plan->d_J, plan->d_ns_list + bk.elem_offset, plan->d_qs_list + bk.elem_offset, bk.n_elem,
                           bk.d_EBb, bk.d_EBf, bk.d_w, P, nullptr, nullptr);
      });
    }
    HIP_CHECK(hipGetLastError());
    return;
  }
  // composed: the three calls a caller would make, through plan-owned temporaries (no allocation after the first call, no
  // synchronisation: the load is rebuilt on every AMR level)
  const size_t nq = (size_t)plan->local_nodes_quad, n = (size_t)plan->local_nodes;
  double *d_f = nullptr, *d_xyz = nullptr;
  nonlinear_load_scratch(plan, S.kind != 2, &d_f, &d_xyz);
  const double* xyz = S.xyz;
  if (S.kind != 2) {
    launch_nodes(plan, 0, S, &nt, 1, F, d_xyz, nullptr);
    xyz = d_xyz;
  }
  hipLaunchKernelGGL(field_eval_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, plan->stream, field_id, F, xyz, (long long)nq, d_f);
  if (!beta) {
    launch_mass_like(plan, 1, d_f, out);
  } else {
    if (!plan->d_work_m) HIP_CHECK(hipMalloc(&plan->d_work_m, n * sizeof(double)));
    launch_mass_like(plan, 1, d_f, plan->d_work_m);
    launch_add(plan, (int)n, plan->d_work_m, out);
  }
  HIP_CHECK(hipGetLastError());
}

}  // namespace d4est_hip

using namespace d4est_hip;

extern "C" {

void d4est_hip_field_eval(void* hip_stream, int field_id, const double* params, int n_params, const double* xyz_dev, long long n,
                          double* out_dev) {
  const FieldParams F = field_params(field_id, params, n_params, "field_eval");
  if (n < 0) D4EST_HIP_ABORT("field_eval: n = %lld", n);
  if (n == 0) return;
  if (!xyz_dev || !out_dev) D4EST_HIP_ABORT("field_eval: NULL array");
  const long long blocks = (n + 255) / 256;
  if (blocks > 0x7fffffffLL) D4EST_HIP_ABORT("field_eval: n = %lld is too many points for one launch", n);
  hipLaunchKernelGGL(field_eval_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(hip_stream), field_id, F, xyz_dev,
                     n, out_dev);
  HIP_CHECK(hipGetLastError());
}

void d4est_hip_plan_compute_xyz_brick(d4est_hip_plan_t* plan, const int* elem_q, const int* elem_dq, double root_len,
                                      const double* extents, double* xyz_lobatto_dev, double* xyz_quad_dev) {
  const char* who = "plan_compute_xyz_brick";
  if (!plan) D4EST_HIP_ABORT("%s: NULL plan", who);
  const std::vector<CellDesc> cells = brick_cells(plan, elem_q, elem_dq, root_len, extents, who);
  if (plan->n_elements == 0) return;
  CoordSrc S = brick_src(root_len, extents);
  const NodeTables nt = stage_cells_and_nodes(plan, cells);
  S.cells = nt.d_cells;
  const FieldParams F = {};
  if (xyz_lobatto_dev) launch_nodes(plan, 0, S, &nt, 0, F, xyz_lobatto_dev, nullptr);
  if (xyz_quad_dev) launch_nodes(plan, 0, S, &nt, 1, F, xyz_quad_dev, nullptr);
}

void d4est_hip_plan_set_puncture_term_brick(d4est_hip_plan_t* plan, const double* params, int n_params, const int* elem_q,
                                            const int* elem_dq, double root_len, const double* extents) {
  const char* who = "plan_set_puncture_term_brick";
  if (!plan) D4EST_HIP_ABORT("%s: NULL plan", who);
  const std::vector<CellDesc> cells = brick_cells(plan, elem_q, elem_dq, root_len, extents, who);
  set_term(plan, kTermPuncture, params, n_params, brick_src(root_len, extents), &cells, who);
}

void d4est_hip_plan_set_puncture_term_analytic(d4est_hip_plan_t* plan, const double* params, int n_params, int geom_type,
                                               const double* geom_params, const int* elem_tree, const int* elem_q, const int* elem_dq,
                                               double root_len) {
  const char* who = "plan_set_puncture_term_analytic";
  if (!plan) D4EST_HIP_ABORT("%s: NULL plan", who);
  const CoordSrc S = analytic_src(geom_type, geom_params, root_len, who);
  const std::vector<CellDesc> cells = analytic_cells(plan, geom_type, elem_tree, elem_q, elem_dq, root_len, who);
  set_term(plan, kTermPuncture, params, n_params, S, &cells, who);
}

void d4est_hip_plan_set_puncture_term_xyz(d4est_hip_plan_t* plan, const double* params, int n_params, const double* xyz_quad_dev) {
  const char* who = "plan_set_puncture_term_xyz";
  if (!plan) D4EST_HIP_ABORT("%s: NULL plan", who);
  set_term(plan, kTermPuncture, params, n_params, xyz_src(plan, xyz_quad_dev, who), nullptr, who);
}

void d4est_hip_plan_set_cds_term_brick(d4est_hip_plan_t* plan, const double* params, int n_params, const int* elem_q, const int* elem_dq,
                                       double root_len, const double* extents) {
  const char* who = "plan_set_cds_term_brick";
  if (!plan) D4EST_HIP_ABORT("%s: NULL plan", who);
  const std::vector<CellDesc> cells = brick_cells(plan, elem_q, elem_dq, root_len, extents, who);
  set_term(plan, kTermCds, params, n_params, brick_src(root_len, extents), &cells, who);
}

void d4est_hip_plan_set_cds_term_analytic(d4est_hip_plan_t* plan, const double* params, int n_params, int geom_type,
                                          const double* geom_params, const int* elem_tree, const int* elem_q, const int* elem_dq,
                                          double root_len) {
  const char* who = "plan_set_cds_term_analytic";
  if (!plan) D4EST_HIP_ABORT("%s: NULL plan", who);
  const CoordSrc S = analytic_src(geom_type, geom_params, root_len, who);
  const std::vector<CellDesc> cells = analytic_cells(plan, geom_type, elem_tree, elem_q, elem_dq, root_len, who);
  set_term(plan, kTermCds, params, n_params, S, &cells, who);
}

void d4est_hip_plan_set_cds_term_xyz(d4est_hip_plan_t* plan, const double* params, int n_params, const double* xyz_quad_dev) {
  const char* who = "plan_set_cds_term_xyz";
  if (!plan) D4EST_HIP_ABORT("%s: NULL plan", who);
  set_term(plan, kTermCds, params, n_params, xyz_src(plan, xyz_quad_dev, who), nullptr, who);
}

void d4est_hip_plan_set_okendon_term_brick(d4est_hip_plan_t* plan, const double* params, int n_params, const int* elem_q,
                                           const int* elem_dq, double root_len, const double* extents) {
  const char* who = "plan_set_okendon_term_brick";
  if (!plan) D4EST_HIP_ABORT("%s: NULL plan", who);
  const std::vector<CellDesc> cells = brick_cells(plan, elem_q, elem_dq, root_len, extents, who);
  set_term(plan, kTermOkendon, params, n_params, brick_src(root_len, extents), &cells, who);
}

void d4est_hip_plan_set_okendon_term_analytic(d4est_hip_plan_t* plan, const double* params, int n_params, int geom_type,
                                              const double* geom_params, const int* elem_tree, const int* elem_q, const int* elem_dq,
                                              double root_len) {
  const char* who = "plan_set_okendon_term_analytic";
  if (!plan) D4EST_HIP_ABORT("%s: NULL plan", who);
  const CoordSrc S = analytic_src(geom_type, geom_params, root_len, who);
  const std::vector<CellDesc> cells = analytic_cells(plan, geom_type, elem_tree, elem_q, elem_dq, root_len, who);
  set_term(plan, kTermOkendon, params, n_params, S, &cells, who);
}

void d4est_hip_plan_set_okendon_term_xyz(d4est_hip_plan_t* plan, const double* params, int n_params, const double* xyz_quad_dev) {
  const char* who = "plan_set_okendon_term_xyz";
  if (!plan) D4EST_HIP_ABORT("%s: NULL plan", who);
  set_term(plan, kTermOkendon, params, n_params, xyz_src(plan, xyz_quad_dev, who), nullptr, who);
}

void d4est_hip_plan_set_boyen_york_term_brick(d4est_hip_plan_t* plan, const double* params, int n_params, const int* elem_q,
                                              const int* elem_dq, double root_len, const double* extents) {
  const char* who = "plan_set_boyen_york_term_brick";
  if (!plan) D4EST_HIP_ABORT("%s: NULL plan", who);
  const std::vector<CellDesc> cells = brick_cells(plan, elem_q, elem_dq, root_len, extents, who);
  set_term(plan, kTermBoyenYork, params, n_params, brick_src(root_len, extents), &cells, who);
}

void d4est_hip_plan_set_boyen_york_term_analytic(d4est_hip_plan_t* plan, const double* params, int n_params, int geom_type,
                                                 const double* geom_params, const int* elem_tree, const int* elem_q, const int* elem_dq,
                                                 double root_len) {
  const char* who = "plan_set_boyen_york_term_analytic";
  if (!plan) D4EST_HIP_ABORT("%s: NULL plan", who);
  const CoordSrc S = analytic_src(geom_type, geom_params, root_len, who);
  const std::vector<CellDesc> cells = analytic_cells(plan, geom_type, elem_tree, elem_q, elem_dq, root_len, who);
  set_term(plan, kTermBoyenYork, params, n_params, S, &cells, who);
}

void d4est_hip_plan_set_boyen_york_term_xyz(d4est_hip_plan_t* plan, const double* params, int n_params, const double* xyz_quad_dev) {
  const char* who = "plan_set_boyen_york_term_xyz";
  if (!plan) D4EST_HIP_ABORT("%s: NULL plan", who);
  set_term(plan, kTermBoyenYork, params, n_params, xyz_src(plan, xyz_quad_dev, who), nullptr, who);
}

void d4est_hip_plan_build_load_by_id_brick(d4est_hip_plan_t* plan, int field_id, const double* params, int n_params, const int* elem_q,
                                           const int* elem_dq, double root_len, const double* extents, int beta, double* out_dev) {
  const char* who = "plan_build_load_by_id_brick";
  if (!plan) D4EST_HIP_ABORT("%s: NULL plan", who);
  const std::vector<CellDesc> cells = brick_cells(plan, elem_q, elem_dq, root_len, extents, who);
  build_load(plan, field_id, params, n_params, brick_src(root_len, extents), &cells, beta, out_dev, who);
}

void d4est_hip_plan_build_load_by_id_analytic(d4est_hip_plan_t* plan, int field_id, const double* params, int n_params, int geom_type,
                                              const double* geom_params, const int* elem_tree, const int* elem_q, const int* elem_dq,
                                              double root_len, int beta, double* out_dev) {
  const char* who = "plan_build_load_by_id_analytic";
  if (!plan) D4EST_HIP_ABORT("%s: NULL plan", who);
  const CoordSrc S = analytic_src(geom_type, geom_params, root_len, who);
  const std::vector<CellDesc> cells = analytic_cells(plan, geom_type, elem_tree, elem_q, elem_dq, root_len, who);
  build_load(plan, field_id, params, n_params, S, &cells, beta, out_dev, who);
}

void d4est_hip_plan_build_load_by_id_xyz(d4est_hip_plan_t* plan, int field_id, const double* params, int n_params,
                                         const double* xyz_quad_dev, int beta, double* out_dev) {
  const char* who = "plan_build_load_by_id_xyz";
  if (!plan) D4EST_HIP_ABORT("%s: NULL plan", who);
  build_load(plan, field_id, params, n_params, xyz_src(plan, xyz_quad_dev, who), nullptr, beta, out_dev, who);
}

void d4est_hip_plan_compute_boundary_xyz_brick(d4est_hip_plan_t* plan, const int* elem_q, const int* elem_dq, double root_len,
                                               const double* extents, double* xyz_mortar_dev) {
  const char* who = "plan_compute_boundary_xyz_brick";
  if (!plan) D4EST_HIP_ABORT("%s: NULL plan", who);
  const std::vector<CellDesc> cells = brick_cells(plan, elem_q, elem_dq, root_len, extents, who);
  boundary_launch(plan, 0, 0, 0, brick_src(root_len, extents), cells, xyz_mortar_dev, who);
}

void d4est_hip_plan_compute_boundary_xyz_analytic(d4est_hip_plan_t* plan, int geom_type, const double* geom_params, const int* elem_tree,
                                                  const int* elem_q, const int* elem_dq, double root_len, double* xyz_mortar_dev) {
  const char* who = "plan_compute_boundary_xyz_analytic";
  if (!plan) D4EST_HIP_ABORT("%s: NULL plan", who);
  const CoordSrc S = analytic_src(geom_type, geom_params, root_len, who);
  const std::vector<CellDesc> cells = analytic_cells(plan, geom_type, elem_tree, elem_q, elem_dq, root_len, who);
  boundary_launch(plan, 0, 0, 0, S, cells, xyz_mortar_dev, who);
}

void d4est_hip_plan_set_robin_by_id_brick(d4est_hip_plan_t* plan, int coeff_id, int rhs_id, const int* elem_q, const int* elem_dq,
                                          double root_len, const double* extents) {
  const char* who = "plan_set_robin_by_id_brick";
  if (!plan) D4EST_HIP_ABORT("%s: NULL plan", who);
  const std::vector<CellDesc> cells = brick_cells(plan, elem_q, elem_dq, root_len, extents, who);
  boundary_launch(plan, 1, coeff_id, rhs_id, brick_src(root_len, extents), cells, nullptr, who);
}

void d4est_hip_plan_set_robin_by_id_analytic(d4est_hip_plan_t* plan, int coeff_id, int rhs_id, int geom_type, const double* geom_params,
                                             const int* elem_tree, const int* elem_q, const int* elem_dq, double root_len) {
  const char* who = "plan_set_robin_by_id_analytic";
  if (!plan) D4EST_HIP_ABORT("%s: NULL plan", who);
  const CoordSrc S = analytic_src(geom_type, geom_params, root_len, who);
  const std::vector<CellDesc> cells = analytic_cells(plan, geom_type, elem_tree, elem_q, elem_dq, root_len, who);
  boundary_launch(plan, 1, coeff_id, rhs_id, S, cells, nullptr, who);
}

}  // extern "C"
