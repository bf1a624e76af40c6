// The Laplacian of a DG field at the quadrature nodes, d4est_hessian_compute_hessian_trace_of_field_on_quadrature_points
// (src/dGMath/d4est_hessian.c:270-368), on a plan.
//
// Written out from d4est_hessian.c:41-58 and :127-138, with R_ai = dr_a/dx_i and X_lak = d^2 x_l / dr_a dr_k:
//   Lap u (q) = sum_b c_b(q) V(D_b u)(q) + sum_ab G_ab(q) V(D_a D_b u)(q)
//   G_ab = sum_i R_ai R_bi                        (symmetric: 6 values)
//   c_b  = sum_i sum_a R_ai d2rdrdx[b][i][a],     d2rdrdx[m][n][k] = - sum_a sum_l R_ml R_an X_lak
// The nine coefficients depend on the mesh only: d4est_hip_plan_set_hessian_* forms them once, 9 local_nodes_quad doubles, element-blocked
// like the metric: coef[9 quad_stride_e + c NQ^3 + n], c in (c_0, c_1, c_2, G_00, G_01, G_02, G_11, G_12, G_22).
//   brick      X = 0 (d4est_geometry_brick.c:8), R diagonal and constant per element: c = 0, G diagonal.
//   analytic   HESSIAN_ANALYTICAL (:180-226): one thread per quadrature node evaluates dx/dr and d^2x/dr dr of the tree map
//              (d4est_hip_maps.h) at the node and inverts dx/dr, which is how the analytic factors get rst_xyz.
//   numerical  HESSIAN_NUMERICAL (:227-262): X_{d1 d2 d3} = V(D_d3 D_d2 x_d1) from the node coordinates, through the plan's own
//              apply_dij and interpolation kernels; R from the caller's rst_xyz_quad or, without it, from V(D x) inverted with the
//              cofactor expressions of the numerical volume factors.  Its scratch (36 local_nodes_quad doubles) is parked and released
//              by the first apply that finds the set-up kernels finished, by the next set-up or by plan_destroy: no form waits.
//
// The apply (hessian_trace_kernel): one workgroup per element, per (deg, deg_quad) bucket.  With the 1-D tables B (interpolation),
// G = B D and G2 = B D D, V(D_a D_b u) is a tensor product of three of them applied to u (D along different directions commutes with
// the interpolation along the others), so nothing of N^3 size beside u is kept: for every quadrature plane kq
//   (1) three N x N planes  w_M(j, i) = sum_k M(kq, k) u(i, j, k),  M in (B, G, G2),
//   (2) six N x NQ planes   t(j, iq) = sum_i M'(iq, i) w_M(j, i)    for the pairs (z, x) in (B,B) (B,G) (B,G2) (G,B) (G,G) (G2,B),
//   (3) per node (iq, jq) the nine line products along y, each times its coefficient, summed in a fixed order and stored once.
// The symmetric pairs are folded (G_ab holds a != b once, the kernel doubles it).  No atomics: the same bits on every call.
// Dynamic LDS: 8 (N^3 + 3 N^2 + 9 N NQ) bytes, which must not exceed 160 KB (163840 bytes); every deg <= 19 fits with
// any deg_quad a plan accepts (N = NQ = 20: 102400 bytes; N = 20, NQ = 24: 108160 bytes); deg = deg_quad = 23 does not (165888).  d4est_hip_plan_hessian_supported reports it; the setters and the apply abort beyond it.
// The one-wavefront form of d4est_hip_wave.h for p <= 7 is not built: every bucket takes this body (workgroups of 64 to 256 threads).
// That header's line-product bodies take one table kind per pass and keep one field per lane set; nine fields from three table kinds
// (B, B D, B D D) need new contraction bodies next to it, which were not written and verified in this change.
#include <algorithm>
#include <cmath>

#include "d4est_hip_internal.h"
#include "d4est_hip_maps.h"
#include "d4est_hip_tables.h"

namespace d4est_hip {

constexpr size_t kHessMaxLds = 160 * 1024;   // gfx950: 160 KB of LDS per workgroup

static size_t hess_lds_bytes(int N, int NQ) { return (size_t)(N * N * N + 3 * N * N + 9 * N * NQ) * sizeof(double); }

struct HessHost {
  int form = 0;                    // 1 brick, 2 analytic, 3 numerical
  double* d_coef = nullptr;        // 9 local_nodes_quad
  std::vector<double*> d_G2T;      // per bucket: (B D D)^T, N x NQ
  // what the set-up kernels read (kept until the next set-up or plan_destroy, so that no set-up waits for its kernels)
  int* d_dq = nullptr;
  CellDesc* d_cells = nullptr;
  double* d_nodes = nullptr;
  // the numerical form's scratch: released by the first apply that finds the set-up kernels finished (scratch_done), else here too
  double* d_scratch[4] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t scratch_done = nullptr;
};

static HessHost* hess_of(const d4est_hip_plan* plan) { return static_cast<HessHost*>(plan->hess); }

// the nine coefficients of one node from R[a][i] = dr_a/dx_i and X[l][a][k] = d^2 x_l / dr_a dr_k (d4est_hessian.c:41-58, :127-138)
__device__ inline void hess_coefficients(const double R[3][3], const double X[3][3][3], double out[9]) {
  double d2r[3][3][3];
  for (int m = 0; m < 3; ++m)
    for (int n = 0; n < 3; ++n)
      for (int k = 0; k < 3; ++k) {
        double s = 0.0;
        for (int a = 0; a < 3; ++a)
          for (int l = 0; l < 3; ++l) s -= R[m][l] * R[a][n] * X[l][a][k];
        d2r[m][n][k] = s;
      }
  for (int b = 0; b < 3; ++b) {
    double s = 0.0;
    for (int i = 0; i < 3; ++i)
      for (int a = 0; a < 3; ++a) s += R[a][i] * d2r[b][i][a];
    out[b] = s;
  }
  int c = 3;
  for (int a = 0; a < 3; ++a)
    for (int b = a; b < 3; ++b) out[c++] = R[a][0] * R[b][0] + R[a][1] * R[b][1] + R[a][2] * R[b][2];
}

__global__ __launch_bounds__(256) void hess_coef_brick_kernel(const int* __restrict__ elem_ids, const int* __restrict__ qs_list, int n_bucket,
                                                              int NQ, const int* __restrict__ elem_dq, double root_len, double ex, double ey,
                                                              double ez, double* __restrict__ coef) {
  const int NQ3 = NQ * NQ * NQ;
  for (int ei = blockIdx.x; ei < n_bucket; ei += gridDim.x) {
    const double half = (double)elem_dq[elem_ids[ei]] / root_len / 2.;
    const double rx = 1. / (ex * half), ry = 1. / (ey * half), rz = 1. / (ez * half);   // dr_d/dx_d (brick_metric_kernel)
    const double g[9] = {0., 0., 0., rx * rx, 0., 0., ry * ry, 0., rz * rz};
    double* out = coef + (size_t)9 * qs_list[ei];
    for (int n = threadIdx.x; n < NQ3; n += blockDim.x) {
#pragma unroll
      for (int c = 0; c < 9; ++c) out[(size_t)c * NQ3 + n] = g[c];
    }
  }
}

__global__ __launch_bounds__(256) void hess_coef_analytic_kernel(const int* __restrict__ elem_ids, const int* __restrict__ qs_list, int n_bucket,
                                                                 int NQ, const double* __restrict__ xq, const CellDesc* __restrict__ cells,
                                                                 TreeMapParams P, double root_len, double* __restrict__ coef) {
  const int NQ3 = NQ * NQ * NQ;
  for (int ei = blockIdx.x; ei < n_bucket; ei += gridDim.x) {
    const CellDesc cell = cells[elem_ids[ei]];
    double* out = coef + (size_t)9 * qs_list[ei];
    for (int n = threadIdx.x; n < NQ3; n += blockDim.x) {
      const int iq = n % NQ, jq = (n / NQ) % NQ, kq = n / (NQ * NQ);
      const double r[3] = {xq[iq], xq[jq], xq[kq]};
      double dxdr[3][3], R[3][3], X[3][3][3], c9[9];
      cell_dxdr(P, cell, root_len, r, dxdr);
      cell_d2xdr(P, cell, root_len, r, X);
      invert3(dxdr, R);   // R[a][i] = dr_a/dx_i
      hess_coefficients(R, X, c9);
#pragma unroll
      for (int c = 0; c < 9; ++c) out[(size_t)c * NQ3 + n] = c9[c];
    }
  }
}

// numerical form: rst[(3 a + i) nq + n] = dr_a/dx_i (inverse != 0: it holds dx_a/dr_i and is inverted here with the cofactor expressions
// of the numerical volume factors), x2[(9 l + 3 a + k) nq + n] = V(D_k D_a x_l)
__global__ __launch_bounds__(256) void hess_coef_numerical_kernel(const int* __restrict__ qs_list, int n_bucket, int NQ,
                                                                  const double* __restrict__ rst, int inverse, const double* __restrict__ x2,
                                                                  size_t nq, double* __restrict__ coef) {
  const int NQ3 = NQ * NQ * NQ;
  for (int ei = blockIdx.x; ei < n_bucket; ei += gridDim.x) {
    const size_t qs = (size_t)qs_list[ei];
    double* out = coef + 9 * qs;
    for (int n = threadIdx.x; n < NQ3; n += blockDim.x) {
      const size_t at = qs + n;
      double R[3][3], X[3][3][3], c9[9];
      if (inverse) {
        const double xr = rst[0 * nq + at], xs = rst[1 * nq + at], xt = rst[2 * nq + at];
        const double yr = rst[3 * nq + at], ys = rst[4 * nq + at], yt = rst[5 * nq + at];
        const double zr = rst[6 * nq + at], zs = rst[7 * nq + at], zt = rst[8 * nq + at];
        const double J = xr * (ys * zt - zs * yt) - yr * (xs * zt - zs * xt) + zr * (xs * yt - ys * xt);
        R[0][0] = (ys * zt - zs * yt) / J;  R[0][1] = -(xs * zt - zs * xt) / J; R[0][2] = (xs * yt - ys * xt) / J;
        R[1][0] = -(yr * zt - zr * yt) / J; R[1][1] = (xr * zt - zr * xt) / J;  R[1][2] = -(xr * yt - yr * xt) / J;
        R[2][0] = (yr * zs - zr * ys) / J;  R[2][1] = -(xr * zs - zr * xs) / J; R[2][2] = (xr * ys - yr * xs) / J;
      } else {
        for (int a = 0; a < 3; ++a)
          for (int i = 0; i < 3; ++i) R[a][i] = rst[(size_t)(3 * a + i) * nq + at];
      }
      for (int l = 0; l < 3; ++l)
        for (int a = 0; a < 3; ++a)
          for (int k = 0; k < 3; ++k) X[l][a][k] = x2[(size_t)(9 * l + 3 * a + k) * nq + at];
      hess_coefficients(R, X, c9);
#pragma unroll
      for (int c = 0; c < 9; ++c) out[(size_t)c * NQ3 + n] = c9[c];
    }
  }
}

// Lap u at the quadrature nodes of the elements of one bucket (see the head of the file).  BT, GT, G2T: N x NQ transposes.
__global__ __launch_bounds__(256) void hessian_trace_kernel(const double* __restrict__ u, const double* __restrict__ coef,
                                                            const int* __restrict__ ns_list, const int* __restrict__ qs_list, int n_elem,
                                                            const double* __restrict__ BT, const double* __restrict__ GT,
                                                            const double* __restrict__ G2T, int N, int NQ, double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int N2 = N * N, N3 = N2 * N, T = N * NQ, NQ2 = NQ * NQ, NQ3 = NQ2 * NQ;
  double* U = smem;           // N^3
  double* W = U + N3;         // 3 planes of N^2: z-variant B, G, G2
  double* P = W + 3 * N2;     // 6 planes of N NQ: (z, x) = (B,B) (B,G) (B,G2) (G,B) (G,G) (G2,B)
  double* Ms = P + 6 * T;     // BT | GT | G2T, each N x NQ
  for (int i = threadIdx.x; i < T; i += blockDim.x) {
    Ms[i] = BT[i];
    Ms[T + i] = GT[i];
    Ms[2 * T + i] = G2T[i];
  }
  for (int el = blockIdx.x; el < n_elem; el += gridDim.x) {
    const double* ue = u + ns_list[el];
    const size_t qs = (size_t)qs_list[el];
    const double* ce = coef + 9 * qs;
    for (int i = threadIdx.x; i < N3; i += blockDim.x) U[i] = ue[i];
    __syncthreads();
    for (int kq = 0; kq < NQ; ++kq) {
      // (1) the three z-contractions of this plane
      for (int idx = threadIdx.x; idx < 3 * N2; idx += blockDim.x) {
        const int v = idx / N2, ji = idx - v * N2;
        const double* M = Ms + v * T + kq;
        double t = 0.0;
        for (int k = 0; k < N; ++k) t = fma(M[k * NQ], U[ji + N2 * k], t);
        W[idx] = t;
      }
      __syncthreads();
      // (2) the six x-contractions
      for (int idx = threadIdx.x; idx < 6 * T; idx += blockDim.x) {
        const int v = idx / T, r = idx - v * T, j = r / NQ, iq = r - j * NQ;
        const int zv = v < 3 ? 0 : (v < 5 ? 1 : 2), xv = v < 3 ? v : (v < 5 ? v - 3 : 0);
        const double* M = Ms + xv * T + iq;
        const double* w = W + zv * N2 + j * N;
        double t = 0.0;
        for (int i = 0; i < N; ++i) t = fma(M[i * NQ], w[i], t);
        P[idx] = t;
      }
      __syncthreads();
      // (3) the nine y-contractions of every node of the plane, each times its coefficient
      for (int n = threadIdx.x; n < NQ2; n += blockDim.x) {
        const int jq = n / NQ, iq = n - jq * NQ;
        const double *b = Ms + jq, *g = Ms + T + jq, *g2 = Ms + 2 * T + jq;
        double d0 = 0.0, d1 = 0.0, d2 = 0.0, d00 = 0.0, d01 = 0.0, d02 = 0.0, d11 = 0.0, d12 = 0.0, d22 = 0.0;
        for (int j = 0; j < N; ++j) {
          const double bj = b[j * NQ], gj = g[j * NQ], g2j = g2[j * NQ];
          const double* p = P + j * NQ + iq;
          const double pBB = p[0], pBG = p[T], pBG2 = p[2 * T], pGB = p[3 * T], pGG = p[4 * T], pG2B = p[5 * T];
          d0 = fma(bj, pBG, d0);      // (z, y, x) = (B, B, G)
          d1 = fma(gj, pBB, d1);      // (B, G, B)
          d2 = fma(bj, pGB, d2);      // (G, B, B)
          d00 = fma(bj, pBG2, d00);   // (B, B, G2)
          d01 = fma(gj, pBG, d01);    // (B, G, G)
          d02 = fma(bj, pGG, d02);    // (G, B, G)
          d11 = fma(g2j, pBB, d11);   // (B, G2, B)
          d12 = fma(gj, pGB, d12);    // (G, G, B)
          d22 = fma(bj, pG2B, d22);   // (G2, B, B)
        }
        const size_t q = (size_t)kq * NQ2 + n;
        double s = ce[q] * d0;
        s = fma(ce[(size_t)NQ3 + q], d1, s);
        s = fma(ce[(size_t)2 * NQ3 + q], d2, s);
        s = fma(ce[(size_t)3 * NQ3 + q], d00, s);
        s = fma(2.0 * ce[(size_t)4 * NQ3 + q], d01, s);
        s = fma(2.0 * ce[(size_t)5 * NQ3 + q], d02, s);
        s = fma(ce[(size_t)6 * NQ3 + q], d11, s);
        s = fma(2.0 * ce[(size_t)7 * NQ3 + q], d12, s);
        s = fma(ce[(size_t)8 * NQ3 + q], d22, s);
        out[qs + q] = s;
      }
      // (the next plane's (1) writes W, which (2) has finished reading; its (2) writes P after the barrier that follows (1))
    }
    __syncthreads();
  }
}

static void release_setup_arrays(HessHost* x) {
  (void)hipFree(x->d_dq); (void)hipFree(x->d_cells); (void)hipFree(x->d_nodes);
  x->d_dq = nullptr; x->d_cells = nullptr; x->d_nodes = nullptr;
  for (double*& p : x->d_scratch) { (void)hipFree(p); p = nullptr; }
}

void hessian_destroy(d4est_hip_plan* plan) {
  HessHost* x = hess_of(plan);
  if (!x) return;
  release_setup_arrays(x);
  (void)hipFree(x->d_coef);
  if (x->scratch_done) (void)hipEventDestroy(x->scratch_done);
  for (double* p : x->d_G2T) (void)hipFree(p);
  delete x;
  plan->hess = nullptr;
}

int hessian_info(const d4est_hip_plan* plan) { return hess_of(plan) ? hess_of(plan)->form : 0; }

int hessian_supported(const d4est_hip_plan* plan) {
  for (const Bucket& bk : plan->buckets)
    if (bk.n_elem > 0 && hess_lds_bytes(bk.N, bk.NQ) > kHessMaxLds) return 0;
  return 1;
}

// the plan's HessHost with its coefficient array and G2 tables, ready for a set-up kernel to fill
static HessHost* hess_prepare(d4est_hip_plan* plan, const char* who) {
  for (const Bucket& bk : plan->buckets)
    if (bk.n_elem > 0 && hess_lds_bytes(bk.N, bk.NQ) > kHessMaxLds)
      D4EST_HIP_ABORT("%s: (deg, deg_quad) = (%d, %d) needs %zu bytes of LDS, more than %zu (d4est_hip_plan_hessian_supported)", who, bk.deg,
                      bk.deg_quad, hess_lds_bytes(bk.N, bk.NQ), kHessMaxLds);
  HessHost* x = hess_of(plan);
  if (x) {
    HIP_CHECK(hipStreamSynchronize(plan->stream));   // a second set-up: the first one's kernels may still read these
    release_setup_arrays(x);
    return x;
  }
  x = new HessHost();
  plan->hess = x;
  HIP_CHECK(hipMalloc(&x->d_coef, std::max<size_t>(9 * (size_t)plan->local_nodes_quad, 1) * sizeof(double)));
  size_t lds = 0;
  for (const Bucket& bk : plan->buckets) {
    const std::vector<double> B = Tables1D::quad_interp(plan->quad_type, bk.deg, bk.deg_quad), D = Tables1D::dij(bk.deg);
    const std::vector<double> G = Tables1D::matmul(B, D, bk.NQ, bk.N, bk.N);
    const std::vector<double> G2T = Tables1D::transpose(Tables1D::matmul(G, D, bk.NQ, bk.N, bk.N), bk.NQ, bk.N);
    double* d = nullptr;
    HIP_CHECK(hipMalloc(&d, G2T.size() * sizeof(double)));
    HIP_CHECK(hipMemcpy(d, G2T.data(), G2T.size() * sizeof(double), hipMemcpyHostToDevice));
    x->d_G2T.push_back(d);
    if (bk.n_elem > 0) lds = std::max(lds, hess_lds_bytes(bk.N, bk.NQ));
  }
  // the apply kernel's LDS beyond the default 64 KB.  The attribute belongs to the kernel on the current device, not to a plan, so it
  // is set to the one fixed limit: nothing a smaller plan could lower
  if (lds > 64 * 1024) set_lds_limit(hessian_trace_kernel, kHessMaxLds);
  return x;
}

void hessian_set_brick(d4est_hip_plan* plan, const int* elem_dq, double root_len, const double* extents) {
  HessHost* x = hess_prepare(plan, "plan_set_hessian_brick");
  const int ne = plan->n_elements;
  HIP_CHECK(hipMalloc(&x->d_dq, std::max<size_t>((size_t)ne, 1) * sizeof(int)));
  if (ne > 0) HIP_CHECK(hipMemcpy(x->d_dq, elem_dq, (size_t)ne * sizeof(int), hipMemcpyHostToDevice));
  for (const Bucket& bk : plan->buckets) {
    if (bk.n_elem == 0) continue;
    hipLaunchKernelGGL(hess_coef_brick_kernel, dim3(std::min(bk.n_elem, 4096)), dim3(256), 0, plan->stream, plan->d_elem_ids + bk.elem_offset,
                       plan->d_qs_list + bk.elem_offset, bk.n_elem, bk.NQ, x->d_dq, root_len, extents[1] - extents[0],
                       extents[3] - extents[2], extents[5] - extents[4], x->d_coef);
    HIP_CHECK(hipGetLastError());
  }
  x->form = 1;
}

void hessian_set_analytic(d4est_hip_plan* plan, const TreeMapParams& P, const std::vector<CellDesc>& cells, double root_len) {
  HessHost* x = hess_prepare(plan, "plan_set_hessian_analytic");
  HIP_CHECK(hipMalloc(&x->d_cells, std::max<size_t>(cells.size(), 1) * sizeof(CellDesc)));
  if (!cells.empty()) HIP_CHECK(hipMemcpy(x->d_cells, cells.data(), cells.size() * sizeof(CellDesc), hipMemcpyHostToDevice));
  // the 1-D quadrature nodes of every bucket, one row of `stride` each
  int stride = 1;
  for (const Bucket& bk : plan->buckets) stride = std::max(stride, bk.NQ);
  std::vector<double> tab(std::max<size_t>(plan->buckets.size() * stride, 1), 0.0);
  for (size_t bi = 0; bi < plan->buckets.size(); ++bi) {
    std::vector<double> xq, w;
    if (plan->quad_type == QUAD_LEGENDRE) Tables1D::gauss(plan->buckets[bi].deg_quad, xq, w);
    else Tables1D::lobatto(plan->buckets[bi].deg_quad, xq, w);
    std::copy(xq.begin(), xq.end(), tab.begin() + bi * stride);
  }
  HIP_CHECK(hipMalloc(&x->d_nodes, tab.size() * sizeof(double)));
  HIP_CHECK(hipMemcpy(x->d_nodes, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
  for (size_t bi = 0; bi < plan->buckets.size(); ++bi) {
    const Bucket& bk = plan->buckets[bi];
    if (bk.n_elem == 0) continue;
    hipLaunchKernelGGL(hess_coef_analytic_kernel, dim3(std::min(bk.n_elem, 4096)), dim3(256), 0, plan->stream,
                       plan->d_elem_ids + bk.elem_offset, plan->d_qs_list + bk.elem_offset, bk.n_elem, bk.NQ, x->d_nodes + bi * stride,
                       x->d_cells, P, root_len, x->d_coef);
    HIP_CHECK(hipGetLastError());
  }
  x->form = 2;
}

void hessian_set_numerical(d4est_hip_plan* plan, const double* xyz_lobatto, const double* rst_xyz_quad, int on_device) {
  HessHost* x = hess_prepare(plan, "plan_set_hessian_numerical");
  const size_t ln = (size_t)plan->local_nodes, nq = (size_t)plan->local_nodes_quad;
  double *d_xyz_own = nullptr, *d_rst_own = nullptr, *d_tmp = nullptr, *d_x2 = nullptr;
  const double* d_xyz = xyz_lobatto;
  const double* d_rst = rst_xyz_quad;
  if (!on_device) {
    HIP_CHECK(hipMalloc(&d_xyz_own, std::max<size_t>(3 * ln, 1) * sizeof(double)));
    HIP_CHECK(hipMemcpy(d_xyz_own, xyz_lobatto, 3 * ln * sizeof(double), hipMemcpyHostToDevice));
    d_xyz = d_xyz_own;
    if (rst_xyz_quad) {
      HIP_CHECK(hipMalloc(&d_rst_own, std::max<size_t>(9 * nq, 1) * sizeof(double)));
      HIP_CHECK(hipMemcpy(d_rst_own, rst_xyz_quad, 9 * nq * sizeof(double), hipMemcpyHostToDevice));
      d_rst = d_rst_own;
    }
  }
  HIP_CHECK(hipMalloc(&d_tmp, std::max<size_t>(4 * ln, 1) * sizeof(double)));
  HIP_CHECK(hipMalloc(&d_x2, std::max<size_t>(27 * nq, 1) * sizeof(double)));
  int inverse = 0;
  if (!rst_xyz_quad) {   // dx_d/dr_d1 = V(D_d1 x_d), as launch_numerical_geometry forms it; inverted in the coefficient kernel
    HIP_CHECK(hipMalloc(&d_rst_own, std::max<size_t>(9 * nq, 1) * sizeof(double)));
    for (int d = 0; d < 3; ++d) {
      launch_dudr(plan, d_xyz + d * ln, d_tmp, d_tmp + ln, d_tmp + 2 * ln);
      for (int d1 = 0; d1 < 3; ++d1) launch_mass_like(plan, 2, d_tmp + d1 * ln, d_rst_own + (size_t)(3 * d + d1) * nq);
    }
    d_rst = d_rst_own;
    inverse = 1;
  }
  double *dr = d_tmp, *drdr = d_tmp + ln;
  for (int d1 = 0; d1 < 3; ++d1)
    for (int d2 = 0; d2 < 3; ++d2) {
      launch_dij(plan, d_xyz + d1 * ln, dr, d2, 0);
      for (int d3 = 0; d3 < 3; ++d3) {
        launch_dij(plan, dr, drdr, d3, 0);
        launch_mass_like(plan, 2, drdr, d_x2 + (size_t)(9 * d1 + 3 * d2 + d3) * nq);
      }
    }
  for (const Bucket& bk : plan->buckets) {
    if (bk.n_elem == 0) continue;
    hipLaunchKernelGGL(hess_coef_numerical_kernel, dim3(std::min(bk.n_elem, 4096)), dim3(256), 0, plan->stream,
                       plan->d_qs_list + bk.elem_offset, bk.n_elem, bk.NQ, d_rst, inverse, d_x2, nq, x->d_coef);
    HIP_CHECK(hipGetLastError());
  }
  // no wait: the scratch is parked and goes away once the kernels above have finished (hessian_trace, the next set-up, plan_destroy)
  x->d_scratch[0] = d_xyz_own; x->d_scratch[1] = d_rst_own; x->d_scratch[2] = d_tmp; x->d_scratch[3] = d_x2;
  if (!x->scratch_done) HIP_CHECK(hipEventCreateWithFlags(&x->scratch_done, hipEventDisableTiming));
  HIP_CHECK(hipEventRecord(x->scratch_done, plan->stream));
  x->form = 3;
}

void hessian_trace(d4est_hip_plan* plan, const double* u, double* del2u_quad) {
  HessHost* x = hess_of(plan);
  if (!x || x->form == 0) D4EST_HIP_ABORT("hessian_trace: the plan has no Hessian coefficients (d4est_hip_plan_set_hessian_*)");
  if (!u || !del2u_quad) D4EST_HIP_ABORT("hessian_trace: NULL u / del2u_quad");
  if (x->d_scratch[3] && hipEventQuery(x->scratch_done) == hipSuccess)   // the numerical set-up has finished: its scratch is idle
    for (double*& p : x->d_scratch) { HIP_CHECK(hipFree(p)); p = nullptr; }
  for (size_t bi = 0; bi < plan->buckets.size(); ++bi) {
    const Bucket& bk = plan->buckets[bi];
    if (bk.n_elem == 0) continue;
    const size_t lds = hess_lds_bytes(bk.N, bk.NQ);
    if (lds > kHessMaxLds) D4EST_HIP_ABORT("hessian_trace: (deg, deg_quad) = (%d, %d) needs %zu bytes of LDS", bk.deg, bk.deg_quad, lds);
    // the widest stage is (2) with 6 N NQ products per plane
    const int work = 6 * bk.N * bk.NQ, threads = work <= 64 ? 64 : (work <= 128 ? 128 : 256);
    hipLaunchKernelGGL(hessian_trace_kernel, dim3(std::min(bk.n_elem, 65536)), dim3(threads), lds, plan->stream, u, x->d_coef,
                       plan->d_ns_list + bk.elem_offset, plan->d_qs_list + bk.elem_offset, bk.n_elem, bk.d_BT, bk.d_GT, x->d_G2T[bi], bk.N,
                       bk.NQ, del2u_quad);
    HIP_CHECK(hipGetLastError());
  }
}

}  // namespace d4est_hip
