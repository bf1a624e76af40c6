// The residual-based a-posteriori error estimator of d4est_estimator_bi_compute (src/Estimators/d4est_estimator_bi.c:343-560) on a plan.
//
// Per local element e, eta2[e] = term0 + term1 + term2 + term3 (the reference's estimator_vtk order, :373-378, :437):
//   term0  (h_e^2 / p_e^2) r_e^T M_e r_e at the element's deg_quad          :395-441, src/Mesh/d4est_mesh.c:2299-2370
//   term1  sum over the interior mortars of e of  sum_k w_k sj_k (pi_grad n.(grad u_m - grad u_p))^2     :150-340
//   term2  sum over the interior mortars of e of  sum_d sum_k w_k sj_k (pi_u n_d (u_m - u_p))^2
//   term3  sum over the boundary sides of e of    sum_d sum_k w_k sj_k (pi_D n_d (u_m - g))^2            :15-148
// Every local side adds to its own element only (a face is visited from both of its sides), a big hanging side adds its four
// sub-mortars, a small side its own.
//
// Kernels (one stream, no host synchronisation, no floating-point atomics: fixed-order reductions, bit-identical from call to call):
//   (1) the full trace kernel of the plan (every side's / every mortar record's block of u and du/dr at the mortar quadrature nodes --
//       the operator path's kernels do not write every block on hybrid and direct plans), into an estimator-owned buffer; ghost blocks
//       from the caller or through the plan's exchange hooks;
//   (2) est_residual_kernel per (deg, deg_quad) bucket: interpolate r to the quadrature nodes (three tensor passes in LDS), sum w J (V r)^2
//       with a fixed tree reduction, times h^2 / p^2;
//   (3) est_face_kernel: one wavefront per element walks the element's mortars and sums terms 1 - 3 from the trace blocks and 8
//       per-node factors formed at set-up, then eta2 = ((term0 + term1) + term2) + term3.
// Set-up (est_geom_kernel, from the reference-layout mortar factors inside faces_set_geometry, so every geometry entry point reaches
// it): per mortar quadrature node  bm_i = fm sum_x n_x (dr_i/dx_x)^-,  bp_i = fp sum_x n_x (dr_i/dx_x)^+ (re-ordered to the (-) side),
// c1 = w sj pi_grad^2,  c2 = w sj pi_u^2 |n|^2 (boundary: w sj pi_D^2 |n|^2), so that term1 = sum c1 (bm.dudr_m - bp.dudr_p)^2 and
// term2 / term3 = sum c2 (u_m - u_p)^2.  fm / fp = 1/2 on the big element's gradient across a hanging face: the reference scales
// dudx before it calls the estimator's interface function (src/dGMath/d4est_laplacian_flux.c:905-915).
#include <algorithm>
#include <cmath>

#include "d4est_hip_elem_l2.h"
#include "d4est_hip_internal.h"
#include "d4est_hip_tables.h"
#include "d4est_hip_wave.h"

namespace d4est_hip {

struct EstHost {
  EstMortar* d_mortars = nullptr;
  int n_mortars = 0;
  int* d_elem_first = nullptr;
  double* d_fac = nullptr;       // 8 per mortar quadrature node at 8 gidx: bm[3], bp[3], c1, c2 (each a T block)
  double* d_trace = nullptr;     // the estimator's own local / ghost trace buffers (the operator's stay untouched)
  double* d_ghost = nullptr;
  double* d_terms = nullptr;     // 4 n_elements scratch when the caller wants no terms
  const double* face_ops = nullptr;
  const double* hp_ops = nullptr;
};

static EstHost* est_of(d4est_hip_plan* plan) { return static_cast<EstHost*>(plan->est); }

// the ten penalty functions of d4est_estimator_bi.h (ids D4EST_HIP_EST_*), evaluated as the reference writes them
__device__ inline double est_penalty(int id, int deg_m, double h_m, int deg_p, double h_p, double c) {
  const double max_p = (double)(deg_m > deg_p ? deg_m : deg_p);
  const double min_h = (h_m < h_p) ? h_m : h_p;
  const double mhp = h_m / (double)deg_m, phq = h_p / (double)deg_p;
  const double max_h_over_p = (mhp > phq) ? mhp : phq;
  const double mp2 = (double)(deg_m * deg_m) / h_m, pp2 = (double)(deg_p * deg_p) / h_p;
  const double max_p2_over_h = (mp2 > pp2) ? mp2 : pp2;
  switch (id) {
    case 0: return sqrt(min_h / max_p);                          // bi_gradu_prefactor_maxp_minh
    case 1: return sqrt(c * max_p * max_p / min_h);              // bi_u_prefactor_conforming_maxp_minh
    case 2: return sqrt(max_h_over_p);                           // bi_gradu_prefactor_max_h_over_p
    case 3: return sqrt(c * max_p2_over_h);                      // bi_u_prefactor_conforming_max_p2_over_h
    case 4: return sqrt(.5 * max_h_over_p);                      // houston_gradu_prefactor_max_h_over_p
    case 5: return sqrt(.5 * c * max_p2_over_h);                 // houston_u_prefactor_max_p2_over_h
    case 6: return sqrt(c * max_p2_over_h);                      // houston_u_dirichlet_prefactor_max_p2_over_h
    case 7: return sqrt(.5 * min_h / max_p);                     // houston_gradu_prefactor_maxp_minh
    case 8: return sqrt(.5 * c * max_p * max_p / min_h);         // houston_u_prefactor_maxp_minh
    default: return sqrt(c * max_p * max_p / min_h);             // houston_u_dirichlet_prefactor_maxp_minh
  }
}

__global__ __launch_bounds__(64) void est_geom_kernel(const EstMortar* __restrict__ md, int n_m, const double* __restrict__ sj,
                                                      const double* __restrict__ nrm, const double* __restrict__ drst_m,
                                                      const double* __restrict__ drst_p, const double* __restrict__ hm,
                                                      const double* __restrict__ hp, const double* __restrict__ wt, int wt_ld, int f_grad,
                                                      int f_u, int f_dir, double c, double* __restrict__ fac) {
  for (int r = blockIdx.x; r < n_m; r += gridDim.x) {
    const EstMortar m = md[r];
    const int NQ = m.NQ, T = NQ * NQ;
    const size_t S = (size_t)m.S, TT = (size_t)m.Ttot;
    const double* w = wt + (size_t)(NQ - 1) * wt_ld;
    double* out = fac + 8 * (size_t)m.gidx;
    for (int k = threadIdx.x; k < T; k += blockDim.x) {
      const int a = k % NQ, b = k / NQ;
      const int kp = (m.kind == 0) ? k : reorder_index(m.code, NQ - 1, a, b);
      const double sjk = sj[S + m.off + k];
      double nx[3], nn = 0.0;
      for (int x = 0; x < 3; ++x) {
        nx[x] = nrm[3 * S + (size_t)x * TT + m.off + k];
        nn += nx[x] * nx[x];
      }
      for (int i = 0; i < 3; ++i) {
        double bm = 0.0, bp = 0.0;
        for (int x = 0; x < 3; ++x) {
          bm += nx[x] * drst_m[9 * S + (size_t)(i + 3 * x) * TT + m.off + k];
          // (+) side factors are stored in the (+) side's sub-mortar order and orientation, as for the SIPG factors
          if (m.kind != 0) bp += nx[x] * drst_p[9 * S + (size_t)(i + 3 * x) * TT + m.off_p + kp];
        }
        out[(size_t)i * T + k] = m.fm * bm;
        out[(size_t)(3 + i) * T + k] = m.fp * bp;
      }
      const double wsj = w[a] * w[b] * sjk;
      const double hmk = hm[S + m.off + k];
      if (m.kind == 0) {
        const double pd = est_penalty(f_dir, m.deg_m, hmk, m.deg_m, hmk, c);
        out[(size_t)6 * T + k] = 0.0;
        out[(size_t)7 * T + k] = wsj * pd * pd * nn;
      } else {
        const double hpk = hp[S + m.off + k];
        const double pg = est_penalty(f_grad, m.deg_m, hmk, m.deg_p, hpk, c);
        const double pu = est_penalty(f_u, m.deg_m, hmk, m.deg_p, hpk, c);
        out[(size_t)6 * T + k] = wsj * pg * pg;
        out[(size_t)7 * T + k] = wsj * pu * pu * nn;
      }
    }
  }
}

// term0 of the elements of one (deg, deg_quad) bucket: one 256-thread workgroup per element
__global__ __launch_bounds__(256) void est_residual_kernel(const double* __restrict__ r, const double* __restrict__ J,
                                                           const int* __restrict__ elem_ids, const int* __restrict__ ns_list,
                                                           const int* __restrict__ qs_list, int n_elem, const double* __restrict__ B,
                                                           const double* __restrict__ w, int N, int NQ, int deg,
                                                           const double* __restrict__ diam, double* __restrict__ term0) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const ElemL2Lds lds = elem_l2_lds(smem, B, w, N, NQ);
  for (int el = blockIdx.x; el < n_elem; el += gridDim.x) {
    const int e = elem_ids[el];
    const double sum = elem_l2_sqr(lds, r + ns_list[el], J + qs_list[el], N, NQ);   // (d4est_hip_elem_l2.h: shared with the L2 norm)
    if (threadIdx.x == 0) {
      const double h = diam[e];
      term0[e] = sum * (h * h / (double)(deg * deg));   // (d4est_estimator_bi.c:420-433: estimator *= h*h/(deg*deg))
    }
    __syncthreads();
  }
}

// term0 of d4est_estimator_bi_new_compute with use_pointwise_residual (src/Estimators/d4est_estimator_bi_new.c:471-487): the residual is
// given at the quadrature nodes, term0 = h^2 / deg^2 sum_q w_q J_q r_q^2 (d4est_quadrature_innerproduct: no interpolation).  One
// 256-thread workgroup per element, strided partial sums and a fixed tree reduction.
__global__ __launch_bounds__(256) void est_pointwise_residual_kernel(const double* __restrict__ rq, const double* __restrict__ J,
                                                                     const int* __restrict__ elem_ids, const int* __restrict__ qs_list,
                                                                     int n_elem, const double* __restrict__ w, int NQ, int deg,
                                                                     const double* __restrict__ diam, double* __restrict__ term0) {
  __shared__ double red[256];
  const int NQ2 = NQ * NQ, NQ3 = NQ2 * NQ;
  for (int el = blockIdx.x; el < n_elem; el += gridDim.x) {
    const int e = elem_ids[el], qs = qs_list[el];
    double acc = 0.0;
    for (int idx = threadIdx.x; idx < NQ3; idx += blockDim.x) {
      const int ab = idx % NQ2, c = idx / NQ2;
      const double r = rq[qs + idx];
      acc += w[ab % NQ] * w[ab / NQ] * w[c] * J[qs + idx] * r * r;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
      if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      const double h = diam[e];
      term0[e] = red[0] * (h * h / (double)(deg * deg));
    }
    __syncthreads();
  }
}

// terms 1 - 3 and eta2: one wavefront per element, lanes over the mortar quadrature nodes, mortars in sequence
__global__ __launch_bounds__(64) void est_face_kernel(const double* __restrict__ qtrace, const double* __restrict__ ghost_qtrace,
                                                      const EstMortar* __restrict__ md, const int* __restrict__ elem_first,
                                                      const double* __restrict__ fac, const double* __restrict__ face_ops,
                                                      const double* __restrict__ hp_ops, const double* __restrict__ g_lobatto, int n_elem,
                                                      double* __restrict__ terms, double* __restrict__ eta2) {
  for (int e = blockIdx.x; e < n_elem; e += gridDim.x) {
    double t1 = 0.0, t2 = 0.0, t3 = 0.0;
    for (int r = elem_first[e]; r < elem_first[e + 1]; ++r) {
      const EstMortar m = md[r];
      const int NQ = m.NQ, T = NQ * NQ;
      const double* f = fac + 8 * (size_t)m.gidx;
      const double* qm = qtrace + m.qoff;
      if (m.kind == 0) {
        const double* C = (m.ops_hp ? hp_ops : face_ops) + m.offC;
        const double* g = g_lobatto ? g_lobatto + m.bstride : nullptr;
        const int N = m.N;
        for (int k = threadIdx.x; k < T; k += blockDim.x) {
          double gq = 0.0;
          if (g) {   // Lobatto face nodes -> mortar quadrature nodes, as bndry_interp_kernel (d4est_estimator_bi.c:83-96)
            const int ap = k % NQ, bp = k / NQ;
            for (int b = 0; b < N; ++b) {
              double s = 0.0;
              for (int a = 0; a < N; ++a) s = fma(C[ap * N + a], g[a + N * b], s);
              gq = fma(C[bp * N + b], s, gq);
            }
          }
          const double d = qm[k] - gq;
          t3 += f[(size_t)7 * T + k] * d * d;
        }
        continue;
      }
      const double* qp = ((m.kind == 2) ? ghost_qtrace : qtrace) + m.nbr_qoff;
      for (int k = threadIdx.x; k < T; k += blockDim.x) {
        const int kp = reorder_index(m.code, NQ - 1, k % NQ, k / NQ);
        double gm = 0.0, gp = 0.0;
        for (int i = 0; i < 3; ++i) {
          gm = fma(f[(size_t)i * T + k], qm[(size_t)(1 + i) * T + k], gm);
          gp = fma(f[(size_t)(3 + i) * T + k], qp[(size_t)(1 + i) * T + kp], gp);
        }
        const double dg = gm - gp, du = qm[k] - qp[kp + m.u_shift];
        t1 += f[(size_t)6 * T + k] * dg * dg;
        t2 += f[(size_t)7 * T + k] * du * du;
      }
    }
    // fixed-order butterfly over the wavefront (lane 0's sums are the same on every call)
    for (int s = 32; s > 0; s >>= 1) {
      t1 += __shfl_xor(t1, s, 64);
      t2 += __shfl_xor(t2, s, 64);
      t3 += __shfl_xor(t3, s, 64);
    }
    if (threadIdx.x == 0) {
      terms[(size_t)n_elem + e] = t1;
      terms[2 * (size_t)n_elem + e] = t2;
      terms[3 * (size_t)n_elem + e] = t3;
      eta2[e] = ((terms[e] + t1) + t2) + t3;
    }
  }
}

static size_t residual_lds_bytes(int N, int NQ) { return elem_l2_lds_bytes(N, NQ); }   // dynamic LDS of est_residual_kernel for one bucket

void estimator_destroy(d4est_hip_plan* plan) {
  EstHost* x = est_of(plan);
  if (!x) return;
  (void)hipFree(x->d_mortars); (void)hipFree(x->d_elem_first); (void)hipFree(x->d_fac);
  (void)hipFree(x->d_trace); (void)hipFree(x->d_ghost); (void)hipFree(x->d_terms);
  delete x;
  plan->est = nullptr;
}

MortarRecords mortar_records_upload(d4est_hip_plan* plan, const char* who, const double** face_ops, const double** hp_ops) {
  std::vector<EstMortar> mort;
  std::vector<int> first;
  faces_estimator_mortars(plan, mort, first, face_ops, hp_ops);
  int max_nq = 1;
  std::vector<char> used(64, 0);
  for (const EstMortar& m : mort) {
    if (m.NQ < 2 || m.NQ > 63) D4EST_HIP_ABORT("%s: mortar with %d quadrature nodes per direction", who, m.NQ);
    max_nq = std::max(max_nq, m.NQ);
    used[m.NQ] = 1;
  }
  // tensor quadrature weights of the plan's mortar degrees: row NQ - 1 holds the NQ weights of degree NQ - 1
  std::vector<double> wt((size_t)max_nq * max_nq, 0.0);
  for (int q = 2; q <= max_nq; ++q) {
    if (!used[q]) continue;
    const std::vector<double> w = Tables1D::quad_weights(plan->quad_type, q - 1);
    std::copy(w.begin(), w.end(), wt.begin() + (size_t)(q - 1) * max_nq);
  }
  auto up = [](const void* src, size_t bytes) {
    void* d = nullptr;
    HIP_CHECK(hipMalloc(&d, std::max<size_t>(bytes, 8)));
    if (bytes) HIP_CHECK(hipMemcpy(d, src, bytes, hipMemcpyHostToDevice));
    return d;
  };
  MortarRecords r;
  r.n_mortars = (int)mort.size();
  r.max_nq = max_nq;
  r.d_mortars = (EstMortar*)up(mort.data(), mort.size() * sizeof(EstMortar));
  r.d_elem_first = (int*)up(first.data(), first.size() * sizeof(int));
  r.d_wt = (double*)up(wt.data(), wt.size() * sizeof(double));
  return r;
}

void estimator_setup(d4est_hip_plan* plan, const double* sj, const double* n, const double* drst_m, const double* drst_p, const double* hm,
                     const double* hp) {
  estimator_destroy(plan);
  EstHost* x = new EstHost();
  plan->est = x;
  const MortarRecords rec = mortar_records_upload(plan, "plan_set_estimator", &x->face_ops, &x->hp_ops);
  const int max_nq = rec.max_nq;
  x->n_mortars = rec.n_mortars;
  x->d_mortars = rec.d_mortars;
  x->d_elem_first = rec.d_elem_first;
  double* d_wt = rec.d_wt;
  const size_t tm = std::max<size_t>((size_t)plan->total_mortar_nodes, 1);
  HIP_CHECK(hipMalloc(&x->d_fac, 8 * tm * sizeof(double)));
  HIP_CHECK(hipMemsetAsync(x->d_fac, 0, 8 * tm * sizeof(double), plan->stream));
  HIP_CHECK(hipMalloc(&x->d_trace, std::max<size_t>((size_t)plan->local_trace_doubles, 1) * sizeof(double)));
  if (plan->ghost_trace_doubles > 0) HIP_CHECK(hipMalloc(&x->d_ghost, (size_t)plan->ghost_trace_doubles * sizeof(double)));
  HIP_CHECK(hipMalloc(&x->d_terms, std::max<size_t>(4 * (size_t)plan->n_elements, 1) * sizeof(double)));
  if (x->n_mortars > 0)
    hipLaunchKernelGGL(est_geom_kernel, dim3(std::min(x->n_mortars, 8192)), dim3(64), 0, plan->stream, x->d_mortars, x->n_mortars, sj, n, drst_m,
                       drst_p, hm, hp, d_wt, max_nq, plan->est_fcn[0], plan->est_fcn[1], plan->est_fcn[2], plan->est_prefactor, x->d_fac);
  HIP_CHECK(hipGetLastError());
  // the residual kernel's LDS beyond the default 64 KB: raised once here, for the plan's largest bucket (at most 160 KB: see estimator_compute)
  size_t lds = 0;
  for (const Bucket& bk : plan->buckets) lds = std::max(lds, residual_lds_bytes(bk.N, bk.NQ));
  if (lds <= 160 * 1024) set_lds_limit(est_residual_kernel, lds);
  HIP_CHECK(hipStreamSynchronize(plan->stream));   // (set-up: the caller's factor arrays may be freed after it)
  HIP_CHECK(hipFree(d_wt));
}

void estimator_compute(d4est_hip_plan* plan, const double* u, const double* ghost_trace, const double* residual, const double* diam,
                       const double* g_lobatto, double* eta2, double* terms, bool pointwise) {
  EstHost* x = est_of(plan);
  if (!plan->est_requested) D4EST_HIP_ABORT("estimator_bi: the plan has no estimator set-up (d4est_hip_plan_set_estimator)");
  if (!x) D4EST_HIP_ABORT("estimator_bi: call d4est_hip_plan_set_estimator before the mortar factors (plan_set_mortar_geometry)");
  if (!plan->has_geometry) D4EST_HIP_ABORT("estimator_bi: the plan has no volume geometry (plan_set_geometry)");
  if (!u || !residual || !diam || !eta2) D4EST_HIP_ABORT("estimator_bi: NULL u / residual / diam / eta2");
  const int ne = plan->n_elements;
  if (ne == 0) return;
  // (1) every side's trace block; ghost blocks from the caller or through the exchange hooks (as apply_lhs)
  launch_traces_all(plan, u, x->d_trace);
  const double* gt = ghost_trace;
  if (!gt && plan->ghost_trace_doubles > 0) {
    if (!plan->exchange_fn) D4EST_HIP_ABORT("estimator_bi: plan has ghost sides but neither a ghost trace nor an exchange callback (plan_set_comm)");
    plan->exchange_fn(plan->comm_ctx, 0, x->d_trace, x->d_ghost);
    plan->exchange_fn(plan->comm_ctx, 1, x->d_trace, x->d_ghost);
    gt = x->d_ghost;
  }
  double* t = terms ? terms : x->d_terms;
  // (2) term0 per bucket
  for (const Bucket& bk : plan->buckets) {
    if (bk.n_elem == 0) continue;
    const int N = bk.N, NQ = bk.NQ;
    if (pointwise) {
      hipLaunchKernelGGL(est_pointwise_residual_kernel, dim3(std::min(bk.n_elem, 16384)), dim3(256), 0, plan->stream, residual, plan->d_J,
                         plan->d_elem_ids + bk.elem_offset, plan->d_qs_list + bk.elem_offset, bk.n_elem, bk.d_w, NQ, bk.deg, diam, t);
      HIP_CHECK(hipGetLastError());
      continue;
    }
    const size_t lds = residual_lds_bytes(N, NQ);
    if (lds > 160 * 1024) D4EST_HIP_ABORT("estimator_bi: (deg, deg_quad) = (%d, %d) needs %zu bytes of LDS", bk.deg, bk.deg_quad, lds);
    hipLaunchKernelGGL(est_residual_kernel, dim3(std::min(bk.n_elem, 16384)), dim3(256), lds, plan->stream, residual, plan->d_J,
                       plan->d_elem_ids + bk.elem_offset, plan->d_ns_list + bk.elem_offset, plan->d_qs_list + bk.elem_offset, bk.n_elem, bk.d_B,
                       bk.d_w, N, NQ, bk.deg, diam, t);
    HIP_CHECK(hipGetLastError());
  }
  // (3) terms 1 - 3 and the sum
  hipLaunchKernelGGL(est_face_kernel, dim3(std::min(ne, 65536)), dim3(64), 0, plan->stream, x->d_trace, gt, x->d_mortars, x->d_elem_first,
                     x->d_fac, x->face_ops, x->hp_ops, g_lobatto, ne, t, eta2);
  HIP_CHECK(hipGetLastError());
}

}  // namespace d4est_hip
