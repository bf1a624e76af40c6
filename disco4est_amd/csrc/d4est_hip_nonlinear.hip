// The nonlinear power term f(x, u) = a(x) (b(x) + u)^k of the reference's shipped nonlinear problems on a plan: the residual term, its
// linearisation and the Newton loop around the device FCG solve.
//
// Replaces, for all local elements at once:
//   d4est_quadrature_apply_fofufofvlj + axpy 1.0   (src/Quadrature/d4est_quadrature.c:776-936, as called from
//                                                   src/Problems/ConstantDensityStar/constant_density_star_fcns.h:360-437)
//   the callbacks neg_2pi_rho_up1_neg5 / neg_10pi_rho_up1_neg4 (constant_density_star_fcns.h:334-357) and
//   two_punctures_neg_1o8_K2_psi_neg7 / two_punctures_plus_7o8_K2_psi_neg8 (src/Problems/TwoPunctures/two_punctures_fcns.h:252-320)
//   constant_density_star_build_residual           (constant_density_star_fcns.h:439-482)
//   d4est_solver_newton_solve                      (src/Solver/d4est_solver_newton.c:135-365)
//
// Design (gfx950): one kernel body, templated on {term, coefficient}.  Both start with V u in registers -- the forward half of
// mass_like_body (d4est_hip_volume.hip): NQ*NQ threads own one element, every thread ends with the NQ values of its (a, b) column at the
// quadrature nodes.  The term form multiplies by w J a (b + V u)^k there and runs the three transposed contractions back to the nodes
// (out = beta out + V^T W J f): u in, out out, J / a / b streamed once -- 8 + 8 + 24 r bytes per DoF, r = (NQ / N)^3, no
// quadrature-sized temporary.  The coefficient form stops at the quadrature nodes and writes c = k a (b + V u0)^(k-1) and w J c, the two
// arrays d4est_hip_plan_set_lhs_coefficient and the first apply_lhs after it would have produced in a copy and a second pass.
// The power is a product of |k| factors (k < 0: one division of 1 by the product); k is wave-uniform, the loop does not diverge.
// The body (d4est_hip_pointwise.h) takes the pointwise function as a template parameter: PowArgs is the integer form above, AbsPowArgs
// the real form a |b + u|^s of Okendon's callbacks (src/Problems/Okendon/okendon_fcns.h:114-145), evaluated with pow as they are.
#include <algorithm>
#include <cmath>

#include "d4est_hip_internal.h"
#include "d4est_hip_wave.h"
#include "d4est_hip_mwave.h"
#include "d4est_hip_pointwise.h"

namespace d4est_hip {

struct NonlinHost {
  double* d_a = nullptr;     // plan-owned copies of the caller's arrays (local_nodes_quad each); d_a == nullptr: the term is off
  double* d_b = nullptr;     // nullptr: b = 0
  int k = 0;
  bool real = false;         // the real form a |b + u|^s (d4est_hip_plan_set_nonlinear_abs_power); then k = 0
  double s = 0.;
  double* d_xyzq = nullptr;  // composed load vector only: x | y | z at the quadrature nodes (nonlinear_load_scratch)
  double* d_uq = nullptr;   // composed path only: V u at the quadrature nodes
  // Newton loop: F(u), the step, the Krylov solver's A u; one device scalar and its pinned host mirror
  double *d_f = nullptr, *d_step = nullptr, *d_Au = nullptr, *d_norm = nullptr, *h_norm = nullptr;
};

static NonlinHost* host_of(const d4est_hip_plan* plan) { return static_cast<NonlinHost*>(plan->nonlin); }

// Mixed-degree plans: all buckets with deg_quad = deg <= 7 in ONE launch (the rule of mass_like_multi_kernel): one 64-lane workgroup
// per work unit, which looks its bucket up (wave-uniform) and runs that degree's body
struct NonlinMulti {
  static constexpr int MAXB = 7;
  int n = 0;
  int wg_end[MAXB] = {};       // exclusive prefix of the buckets' workgroup counts
  int N[MAXB] = {};
  int n_elem[MAXB] = {};
  int elem_offset[MAXB] = {};  // into the plan's bucket-ordered ns / qs lists
  const double* EBf[MAXB] = {};
  const double* EBb[MAXB] = {};
  const double* wq[MAXB] = {};
};

template <bool COEFF, class F>
__global__ __launch_bounds__(64) void nonlin_multi_kernel(const double* __restrict__ u, double* __restrict__ out,
                                                          const double* __restrict__ Jq, const int* __restrict__ ns_list_all,
                                                          const int* __restrict__ qs_list_all, F P, double* __restrict__ c_out,
                                                          double* __restrict__ wjc_out, NonlinMulti A) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int blk = blockIdx.x;
  int bi = 0;
  while (bi + 1 < A.n && blk >= A.wg_end[bi]) ++bi;
  const int wg = blk - (bi > 0 ? A.wg_end[bi - 1] : 0);
  const int off = A.elem_offset[bi], nb = A.n_elem[bi];
  const double* EBb = A.EBb[bi];
  const double* EBf = A.EBf[bi];
  const double* wq = A.wq[bi];
#define D4EST_CASE(N_)                                                                                                              \
  case N_:                                                                                                                          \
    nonlin_body<N_, N_, COEFF, F>(smem, wg, u, out, Jq, ns_list_all + off, qs_list_all + off, nb, EBb, EBf, wq, P, c_out, wjc_out); \
    break;
  switch (A.N[bi]) {
    D4EST_CASE(2) D4EST_CASE(3) D4EST_CASE(4) D4EST_CASE(5) D4EST_CASE(6) D4EST_CASE(7) D4EST_CASE(8)
    default: break;
  }
#undef D4EST_CASE
}

// composed path (a bucket without a compiled pair): the pointwise step between d4est_hip_interpolate and the integral / the w J c pass
template <bool COEFF, class F>
__global__ __launch_bounds__(256) void nonlin_pointwise_kernel(long long n, double* __restrict__ uq, F P) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    uq[i] = COEFF ? P.coeff(0, i, 0, 0, 0, uq[i]) : P.term(0, i, 0, 0, 0, uq[i]);
}

__global__ __launch_bounds__(256) void nonlin_negate_kernel(int n, double* __restrict__ x) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) x[i] = -1. * x[i];
}

static bool plan_fused(const d4est_hip_plan* plan) { return plan_pairs_built(plan); }

// every bucket of a plan for which plan_fused() holds
template <bool COEFF, class F>
static void launch_fused(d4est_hip_plan* plan, const double* u, double* out, F P, double* c_out, double* wjc_out) {
  unsigned covered = 0u;
  NonlinMulti A;   // mixed-degree plans: one launch for the deg_quad = deg <= 7 buckets
  size_t lds = 0;
  for (size_t i = 0; i < plan->buckets.size(); ++i) {
    const Bucket& bk = plan->buckets[i];
    if (!bucket_single_wave(bk)) continue;
    const WaveCfgSquare w = wave_cfg_square(bk.N);
    if (!multi_append(A, covered, i, bk, (bk.n_elem + w.epb - 1) / w.epb)) continue;
    lds = std::max(lds, w.lds_bytes);
  }
  if (A.n >= 2)
    hipLaunchKernelGGL((nonlin_multi_kernel<COEFF, F>), dim3(multi_workgroups(A)), dim3(64), lds, plan->stream, u, out, plan->d_J,
                       plan->d_ns_list, plan->d_qs_list, P, c_out, wjc_out, A);
  else
    covered = 0u;
  for_each_uncovered_bucket(plan, covered, [&](const Bucket& bk) {
    const bool built = for_built_pair(bk.N, bk.NQ, [&](auto n, auto nq) {
      constexpr int N = decltype(n)::value, NQ = decltype(nq)::value;
      using C = WaveCfg<N, NQ>;
      set_lds_limit(nonlin_kernel<N, NQ, COEFF, F>, C::LDS_BYTES);
      hipLaunchKernelGGL((nonlin_kernel<N, NQ, COEFF, F>), dim3((bk.n_elem + C::EPB - 1) / C::EPB), dim3(C::THREADS), C::LDS_BYTES, plan->stream,
                         u, out, plan->d_J, plan->d_ns_list + bk.elem_offset, plan->d_qs_list + bk.elem_offset, bk.n_elem, bk.d_EBb,
                         bk.d_EBf, bk.d_w, P, c_out, wjc_out);
    });
    if (!built) D4EST_HIP_ABORT("nonlinear term: no kernel for (N, NQ) = (%d, %d)", bk.N, bk.NQ);   // plan_fused() excludes this
  });
  HIP_CHECK(hipGetLastError());
}

static NonlinHost* need_term(d4est_hip_plan* plan, const char* who) {
  NonlinHost* h = host_of(plan);
  if (!h || !h->d_a) D4EST_HIP_ABORT("%s: no power term is set (d4est_hip_plan_set_nonlinear_power / _abs_power)", who);
  if (!plan->has_geometry) D4EST_HIP_ABORT("%s: d4est_hip_plan_set_geometry was not called", who);
  return h;
}

static size_t nq_alloc(const d4est_hip_plan* plan) { return std::max<size_t>((size_t)plan->local_nodes_quad, 1) * sizeof(double); }

static void ensure_uq(d4est_hip_plan* plan, NonlinHost* h) {
  if (!h->d_uq) HIP_CHECK(hipMalloc(&h->d_uq, nq_alloc(plan)));
}

static void term_arrays(d4est_hip_plan* plan, bool real, int k, double s, bool with_b, double** a, double** b) {
  NonlinHost* h = host_of(plan);
  if (!h) { h = new NonlinHost; plan->nonlin = h; }
  if (!h->d_a) HIP_CHECK(hipMalloc(&h->d_a, nq_alloc(plan)));
  if (with_b) {
    if (!h->d_b) HIP_CHECK(hipMalloc(&h->d_b, nq_alloc(plan)));
  } else {
    (void)hipFree(h->d_b); h->d_b = nullptr;
  }
  h->k = k;         // setting either form clears the other
  h->real = real;
  h->s = s;
  *a = h->d_a;
  *b = h->d_b;
}

void nonlinear_term_arrays(d4est_hip_plan* plan, int k, bool with_b, double** a, double** b) {
  term_arrays(plan, false, k, 0., with_b, a, b);
}

void nonlinear_term_arrays_real(d4est_hip_plan* plan, double s, bool with_b, double** a, double** b) {
  term_arrays(plan, true, 0, s, with_b, a, b);
}

// the term switched off (a == NULL of either setter)
static void term_off(d4est_hip_plan* plan) {
  NonlinHost* h = host_of(plan);
  if (!h) { h = new NonlinHost; plan->nonlin = h; }
  (void)hipFree(h->d_a); h->d_a = nullptr;
  (void)hipFree(h->d_b); h->d_b = nullptr;
  h->k = 0;
  h->real = false;
  h->s = 0.;
}

// f(P) with the pointwise function of the form that is set
template <class Fn>
static void with_form(const NonlinHost* h, int beta, Fn&& f) {
  if (h->real) f(AbsPowArgs{h->d_a, h->d_b, h->s, beta});
  else f(PowArgs{h->d_a, h->d_b, h->k, beta});
}

void nonlinear_load_scratch(d4est_hip_plan* plan, bool want_xyz, double** f_quad, double** xyz_quad) {
  NonlinHost* h = host_of(plan);
  if (!h) { h = new NonlinHost; plan->nonlin = h; }
  ensure_uq(plan, h);
  if (want_xyz && !h->d_xyzq) HIP_CHECK(hipMalloc(&h->d_xyzq, 3 * nq_alloc(plan)));
  *f_quad = h->d_uq;
  *xyz_quad = want_xyz ? h->d_xyzq : nullptr;
}

void nonlinear_destroy(d4est_hip_plan* plan) {
  NonlinHost* h = host_of(plan);
  if (!h) return;
  (void)hipFree(h->d_a); (void)hipFree(h->d_b); (void)hipFree(h->d_uq); (void)hipFree(h->d_xyzq);
  (void)hipFree(h->d_f); (void)hipFree(h->d_step); (void)hipFree(h->d_Au); (void)hipFree(h->d_norm);
  if (h->h_norm) (void)hipHostFree(h->h_norm);
  delete h;
  plan->nonlin = nullptr;
}

}  // namespace d4est_hip

using d4est_hip::NonlinHost;

extern "C" {

void d4est_hip_plan_set_nonlinear_power(d4est_hip_plan_t* plan, const double* a_quad_dev, const double* b_quad_dev, int k) {
  if (!plan) D4EST_HIP_ABORT("plan_set_nonlinear_power: NULL plan");
  if (k < -16 || k > 16) D4EST_HIP_ABORT("plan_set_nonlinear_power: k = %d is outside [-16, 16]", k);
  const size_t bytes = (size_t)plan->local_nodes_quad * sizeof(double);
  if (!a_quad_dev) {   // the term is off
    d4est_hip::term_off(plan);
    return;
  }
  // the values are CAPTURED here, as d4est_hip_plan_set_lhs_coefficient captures its coefficient
  double *d_a = nullptr, *d_b = nullptr;
  d4est_hip::nonlinear_term_arrays(plan, k, b_quad_dev != nullptr, &d_a, &d_b);
  HIP_CHECK(hipMemcpyAsync(d_a, a_quad_dev, bytes, hipMemcpyDeviceToDevice, plan->stream));
  if (b_quad_dev) HIP_CHECK(hipMemcpyAsync(d_b, b_quad_dev, bytes, hipMemcpyDeviceToDevice, plan->stream));
}

void d4est_hip_plan_set_nonlinear_abs_power(d4est_hip_plan_t* plan, const double* a_quad_dev, const double* b_quad_dev, double s) {
  if (!plan) D4EST_HIP_ABORT("plan_set_nonlinear_abs_power: NULL plan");
  if (!std::isfinite(s)) D4EST_HIP_ABORT("plan_set_nonlinear_abs_power: s = %g", s);
  const size_t bytes = (size_t)plan->local_nodes_quad * sizeof(double);
  if (!a_quad_dev) {   // the term is off
    d4est_hip::term_off(plan);
    return;
  }
  double *d_a = nullptr, *d_b = nullptr;
  d4est_hip::nonlinear_term_arrays_real(plan, s, b_quad_dev != nullptr, &d_a, &d_b);
  HIP_CHECK(hipMemcpyAsync(d_a, a_quad_dev, bytes, hipMemcpyDeviceToDevice, plan->stream));
  if (b_quad_dev) HIP_CHECK(hipMemcpyAsync(d_b, b_quad_dev, bytes, hipMemcpyDeviceToDevice, plan->stream));
}

int d4est_hip_plan_nonlinear_coefficients(const d4est_hip_plan_t* plan, const double** a_dev, const double** b_dev, int* k) {
  if (!plan) D4EST_HIP_ABORT("plan_nonlinear_coefficients: NULL plan");
  const NonlinHost* h = d4est_hip::host_of(plan);
  if (!h || !h->d_a) return 0;
  if (a_dev) *a_dev = h->d_a;
  if (b_dev) *b_dev = h->d_b;
  if (k) *k = h->k;   // 0 while the real form is set (d4est_hip_plan_nonlinear_exponent)
  return 1;
}

int d4est_hip_plan_nonlinear_exponent(const d4est_hip_plan_t* plan, double* s) {
  if (!plan) D4EST_HIP_ABORT("plan_nonlinear_exponent: NULL plan");
  const NonlinHost* h = d4est_hip::host_of(plan);
  if (!h || !h->d_a || !h->real) return 0;
  if (s) *s = h->s;
  return 1;
}

void d4est_hip_apply_nonlinear_term(d4est_hip_plan_t* plan, const double* u_dev, int beta, double* out_dev) {
  if (!plan) D4EST_HIP_ABORT("apply_nonlinear_term: NULL plan");
  if (beta != 0 && beta != 1) D4EST_HIP_ABORT("apply_nonlinear_term: beta = %d (0 or 1)", beta);
  if (!u_dev || !out_dev) D4EST_HIP_ABORT("apply_nonlinear_term: NULL vector");
  NonlinHost* h = d4est_hip::host_of(plan);
  const int n = plan->local_nodes;
  if (!h || !h->d_a) {   // the term is off: out = beta out
    if (!beta && n > 0) HIP_CHECK(hipMemsetAsync(out_dev, 0, (size_t)n * sizeof(double), plan->stream));
    return;
  }
  if (!plan->has_geometry) D4EST_HIP_ABORT("apply_nonlinear_term: d4est_hip_plan_set_geometry was not called");
  if (n == 0) return;
  if (d4est_hip::plan_fused(plan)) {
    d4est_hip::with_form(h, beta, [&](auto P) { d4est_hip::launch_fused<false>(plan, u_dev, out_dev, P, nullptr, nullptr); });
    return;
  }
  // composed: interpolate, pointwise, integrate (+ axpy 1.0)
  d4est_hip::ensure_uq(plan, h);
  d4est_hip::launch_mass_like(plan, 2, u_dev, h->d_uq);
  const long long nq = plan->local_nodes_quad;
  d4est_hip::with_form(h, beta, [&](auto P) {
    hipLaunchKernelGGL((d4est_hip::nonlin_pointwise_kernel<false, decltype(P)>), dim3(d4est_hip::grid_for(nq)), dim3(256), 0, plan->stream, nq,
                       h->d_uq, P);
  });
  if (!beta) {
    d4est_hip::launch_mass_like(plan, 1, h->d_uq, out_dev);
  } else {
    if (!plan->d_work_m) HIP_CHECK(hipMalloc(&plan->d_work_m, (size_t)n * sizeof(double)));
    d4est_hip::launch_mass_like(plan, 1, h->d_uq, plan->d_work_m);
    d4est_hip::launch_add(plan, n, plan->d_work_m, out_dev);
  }
  HIP_CHECK(hipGetLastError());
}

void d4est_hip_plan_linearise(d4est_hip_plan_t* plan, const double* u0_dev) {
  if (!plan) D4EST_HIP_ABORT("plan_linearise: NULL plan");
  if (!u0_dev) D4EST_HIP_ABORT("plan_linearise: NULL vector");
  NonlinHost* h = d4est_hip::need_term(plan, "plan_linearise");
  // the state d4est_hip_plan_set_lhs_coefficient(plan, c) leaves: a captured graph is dropped, the operator generation bumped, the
  // coefficient form selected (it replaces element blocks / a Galerkin chain), the plan-owned copy holds c
  if (plan->cheby_graph) { (void)hipGraphExecDestroy(plan->cheby_graph); plan->cheby_graph = nullptr; }
  ++plan->op_generation;
  plan->lhs_wjc_valid = false;
  plan->d_lhs_blocks = nullptr;
  d4est_hip::lhs_chain_destroy(plan);
  if (!plan->d_lhs_c) HIP_CHECK(hipMalloc(&plan->d_lhs_c, d4est_hip::nq_alloc(plan)));
  if (!plan->d_lhs_wjc) HIP_CHECK(hipMalloc(&plan->d_lhs_wjc, d4est_hip::nq_alloc(plan)));
  plan->d_lhs_coeff = plan->d_lhs_c;   // non-null = the term is on (the caller's array is never read after the capture)
  if (plan->local_nodes == 0) return;
  if (d4est_hip::plan_fused(plan)) {
    d4est_hip::with_form(h, 0, [&](auto P) { d4est_hip::launch_fused<true>(plan, u0_dev, nullptr, P, plan->d_lhs_c, plan->d_lhs_wjc); });
    plan->lhs_wjc_valid = true;   // ... and w J c is already formed (set_lhs_coefficient leaves it to the first apply)
    return;
  }
  // composed: V u0 into the coefficient array, c in place; w J c by the first apply (ensure_lhs_wjc)
  d4est_hip::launch_mass_like(plan, 2, u0_dev, plan->d_lhs_c);
  const long long nq = plan->local_nodes_quad;
  d4est_hip::with_form(h, 0, [&](auto P) {
    hipLaunchKernelGGL((d4est_hip::nonlin_pointwise_kernel<true, decltype(P)>), dim3(d4est_hip::grid_for(nq)), dim3(256), 0, plan->stream, nq,
                       plan->d_lhs_c, P);
  });
  HIP_CHECK(hipGetLastError());
}

int d4est_hip_plan_nonlinear_fused(const d4est_hip_plan_t* plan) {
  if (!plan) D4EST_HIP_ABORT("plan_nonlinear_fused: NULL plan");
  return d4est_hip::plan_fused(plan) ? 1 : 0;
}

void d4est_hip_build_residual(d4est_hip_plan_t* plan, const double* u_dev, const double* ghost_trace_dev, const double* rhs_dev,
                              double* out_dev) {
  if (!plan) D4EST_HIP_ABORT("build_residual: NULL plan");
  d4est_hip_apply_aij(plan, u_dev, ghost_trace_dev, out_dev);
  d4est_hip_apply_nonlinear_term(plan, u_dev, 1, out_dev);
  if (rhs_dev) d4est_hip::launch_residual_inplace_sub(plan, plan->local_nodes, rhs_dev, out_dev);
}

int d4est_hip_newton_solve(d4est_hip_plan_t* plan, double* u_dev, const double* rhs_dev, const double* g_lobatto_dev, double atol,
                           double rtol, int imin, int imax, int krylov_imax, double krylov_atol, double krylov_rtol, d4est_hip_pc_fn pc,
                           void* pc_ctx, d4est_hip_linearise_fn on_linearise, void* cb_ctx, double* fnrm_history_host, int* its_host) {
  if (!plan) D4EST_HIP_ABORT("newton_solve: NULL plan");
  if (!u_dev) D4EST_HIP_ABORT("newton_solve: NULL vector");
  if (plan->n_ghost > 0 || plan->ghost_trace_doubles > 0) D4EST_HIP_ABORT("newton_solve: the plan has ghost sides (single-rank plans only)");
  if (!plan->has_faces) D4EST_HIP_ABORT("newton_solve: the plan has no faces (plan_set_faces)");
  if (imin < 0 || imax < 0 || krylov_imax < 0) D4EST_HIP_ABORT("newton_solve: imin = %d, imax = %d, krylov_imax = %d", imin, imax, krylov_imax);
  NonlinHost* h = d4est_hip::need_term(plan, "newton_solve");
  const int n = plan->local_nodes;
  const size_t bytes = std::max<size_t>((size_t)n, 1) * sizeof(double);
  if (!h->d_f) {
    HIP_CHECK(hipMalloc(&h->d_f, bytes));
    HIP_CHECK(hipMalloc(&h->d_step, bytes));
    HIP_CHECK(hipMalloc(&h->d_Au, bytes));
    HIP_CHECK(hipMalloc(&h->d_norm, sizeof(double)));
    HIP_CHECK(hipHostMalloc((void**)&h->h_norm, sizeof(double), hipHostMallocDefault));
  }
  const int g = d4est_hip::grid_for(n);
  // the residual carries the inhomogeneous boundary values, the Jacobian the zeroed ones (d4est_solver_newton.c:120-123)
  auto residual_norm = [&]() {
    d4est_hip_plan_set_dirichlet_values(plan, g_lobatto_dev, 1);
    d4est_hip_build_residual(plan, u_dev, nullptr, rhs_dev, h->d_f);
    d4est_hip_plan_set_dirichlet_values(plan, nullptr, 1);
    d4est_hip::launch_dot(plan, n, h->d_f, h->d_f, h->d_norm);
    if (plan->allreduce_fn) plan->allreduce_fn(plan->comm_ctx, h->d_norm, 1);
    HIP_CHECK(hipMemcpyAsync(h->h_norm, h->d_norm, sizeof(double), hipMemcpyDeviceToHost, plan->stream));
    HIP_CHECK(hipStreamSynchronize(plan->stream));   // the one host read per Newton iteration
    return std::sqrt(*h->h_norm);
  };
  double fnrm = residual_norm();                                             // :196-223
  if (fnrm_history_host) fnrm_history_host[0] = fnrm;
  const double stop_tol = atol + rtol * fnrm;                                // :226
  int itc = 0;
  while ((fnrm > stop_tol || itc < imin) && itc < imax) {                    // :234
    if (n > 0) hipLaunchKernelGGL(d4est_hip::nonlin_negate_kernel, dim3(g), dim3(256), 0, plan->stream, n, h->d_f);   // :238
    HIP_CHECK(hipMemsetAsync(h->d_step, 0, bytes, plan->stream));            // :246
    d4est_hip_plan_linearise(plan, u_dev);
    if (on_linearise) on_linearise(cb_ctx, u_dev);
    (void)d4est_hip::fcg_solve(plan, h->d_step, h->d_f, h->d_Au, krylov_imax, krylov_atol, krylov_rtol, pc, pc_ctx, nullptr);   // :248-263
    d4est_hip::launch_add(plan, n, h->d_step, u_dev);   // :266, the full step
    fnrm = residual_norm();                                                  // :269-305
    ++itc;
    if (fnrm_history_host) fnrm_history_host[itc] = fnrm;
  }
  if (its_host) *its_host = itc;
  return fnrm > stop_tol ? 1 : 0;                                            // :346-348
}

}  // extern "C"
