// Krylov solves on one plan: d4est_solver_cg_solve (src/Solver/d4est_solver_cg.c:76-197) and the FCG the reference builds,
// d4est_solver_fcg_solve of src/Solver/d4est_solver_fcg_improved.c:97-346.
//
// The scalars (alpha, beta, rho, gamma, the stop test) never leave the device: one-thread kernels form them from device memory, as
// cg_alpha_kernel does for cg_eigs (d4est_hip_solver.hip).  The vector work per CG iteration is three passes -- d.Ad partial sums; u += a d,
// r -= a Ad with the r.r partial sums; d = r + b d -- and per FCG iteration two: the four partial sums of v.r, v.w, v.q, r.r, then one
// update of d, q, u, r.  Reductions are two-stage (fixed grid, fixed LDS tree, no atomics), so a solve is bit-identical from run to run.
// CG iterations are enqueued in batches; a device flag raised by the scalar kernel turns every later vector update into a no-op, and the
// host reads that flag once per batch.  Products and sums are rounded one by one, like the reference's BLAS-1 loops (no contraction).
#include <algorithm>
#include <cmath>
#include <cstddef>

#include "d4est_hip_internal.h"

namespace d4est_hip {

namespace {

constexpr int kBlocks = 1024;     // reduction grid cap (the grid depends on n only: the summation order does not depend on the batch)
constexpr int kThreads = 256;
constexpr int kDefaultCheck = 8;  // D4EST_HIP_TUNE_KRYLOV_CHECK default

// device scalars of one solve
struct KState {
  double dot[4];      // reduced sums (after the allreduce hook)
  double delta, delta_old, delta0, thr;   // CG
  double alpha, beta;                     // CG step lengths
  double rho, coef, a, na, tol;           // FCG: rho_k, -gamma_k / rho_{k-1}, alpha_k / rho_k, -alpha_k / rho_k, atol + rtol |r_0|
  int done, count;    // stop flag, iterations made (copied to pinned host memory together)
};

struct KrylovWork {
  size_t n_alloc = 0;
  double* vec[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // r, d, w, v, q
  double* partial = nullptr;   // 4 * kBlocks
  KState* st = nullptr;
  double* hist = nullptr;      // device history (grown on demand)
  int hist_cap = 0;
  int* flags_host = nullptr;   // pinned: done, count
};

int grid_for(int n) { return std::max(1, std::min((n + kThreads - 1) / kThreads, kBlocks)); }

KrylovWork* work(d4est_hip_plan* plan, int hist_len) {
  KrylovWork* w = static_cast<KrylovWork*>(plan->krylov);
  if (!w) {
    w = new KrylovWork();
    plan->krylov = w;
    HIP_CHECK(hipMalloc(&w->partial, 4 * (size_t)kBlocks * sizeof(double)));
    HIP_CHECK(hipMalloc(&w->st, sizeof(KState)));
    HIP_CHECK(hipHostMalloc((void**)&w->flags_host, 2 * sizeof(int), hipHostMallocDefault));
  }
  const size_t n = std::max<size_t>((size_t)plan->local_nodes, 1);
  if (w->n_alloc < n) {
    for (double*& v : w->vec) {
      if (v) HIP_CHECK(hipFree(v));
      HIP_CHECK(hipMalloc(&v, n * sizeof(double)));
    }
    w->n_alloc = n;
  }
  if (hist_len > w->hist_cap) {
    if (w->hist) HIP_CHECK(hipFree(w->hist));
    HIP_CHECK(hipMalloc(&w->hist, (size_t)hist_len * sizeof(double)));
    w->hist_cap = hist_len;
  }
  return w;
}

// NS dot products x_s . y_s over one grid-stride range, block sums to partial[s * kBlocks + block] (the order of dot_partial_kernel)
template <int NS>
__device__ inline void block_store(double (&s)[NS], double* __restrict__ partial) {
  __shared__ double sm[NS][kThreads];
  for (int k = 0; k < NS; ++k) sm[k][threadIdx.x] = s[k];
  __syncthreads();
  for (int w = kThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w)
      for (int k = 0; k < NS; ++k) sm[k][threadIdx.x] += sm[k][threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0)
    for (int k = 0; k < NS; ++k) partial[k * kBlocks + blockIdx.x] = sm[k][0];
}

__global__ __launch_bounds__(kThreads) void dot1_kernel(int n, const double* __restrict__ x, const double* __restrict__ y,
                                                         double* __restrict__ partial) {
  double s[1] = {0.0};
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) s[0] = fma(x[i], y[i], s[0]);
  block_store<1>(s, partial);
}

// sum the nsums block partials in a fixed tree, into st->dot[0 .. nsums)
__global__ __launch_bounds__(kThreads) void reduce_kernel(int nblocks, int nsums, const double* __restrict__ partial, KState* st) {
  __shared__ double sm[kThreads];
  for (int k = 0; k < nsums; ++k) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += kThreads) s += partial[k * kBlocks + i];
    sm[threadIdx.x] = s;
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
      if ((int)threadIdx.x < w) sm[threadIdx.x] += sm[threadIdx.x + w];
      __syncthreads();
    }
    if (threadIdx.x == 0) st->dot[k] = sm[0];
    __syncthreads();
  }
}

// ---- CG (d4est_solver_cg.c) ----
// r = rhs - Au (copy + xpby(rhs, -1, r), :129-132); d = r (:133)
__global__ __launch_bounds__(kThreads) void cg_init_vec_kernel(int n, const double* __restrict__ rhs, const double* __restrict__ Au,
                                                               double* __restrict__ r, double* __restrict__ d) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const double v = __dadd_rn(rhs[i], __dmul_rn(-1.0, Au[i]));
    r[i] = v;
    d[i] = v;
  }
}
// delta_0 = delta_new (:142-143); the loop test of :148 before the first iteration
__global__ void cg_init_scalar_kernel(KState* st, double* hist, double atol, double rtol) {
  const double delta = st->dot[0];
  st->delta = delta;
  st->delta0 = delta;
  st->thr = __dadd_rn(__dmul_rn(atol, atol), __dmul_rn(__dmul_rn(delta, rtol), rtol));
  st->count = 0;
  st->done = !(delta > st->thr);
  if (hist) hist[0] = delta;
}
// alpha = delta_new / d.Au (:169); delta_old = delta_new (:176)
__global__ void cg_alpha_step_kernel(KState* st) {
  if (st->done) return;
  st->alpha = st->delta / st->dot[0];
  st->delta_old = st->delta;
}
// u += alpha d ; r -= alpha Au (:171-174), with the block sums of r.r (:177)
__global__ __launch_bounds__(kThreads) void cg_update_kernel(int n, const KState* __restrict__ st, const double* __restrict__ d,
                                                             const double* __restrict__ Au, double* __restrict__ u, double* __restrict__ r,
                                                             double* __restrict__ partial) {
  if (st->done) return;
  const double a = st->alpha;
  double s[1] = {0.0};
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    u[i] = __dadd_rn(u[i], __dmul_rn(a, d[i]));
    const double ri = __dadd_rn(r[i], __dmul_rn(-a, Au[i]));
    r[i] = ri;
    s[0] = fma(ri, ri, s[0]);
  }
  block_store<1>(s, partial);
}
// beta = delta_new / delta_old (:183); the loop test of :148 for the next iteration
__global__ void cg_beta_step_kernel(KState* st, double* hist) {
  if (st->done) return;
  const double delta = st->dot[0];
  st->delta = delta;
  st->beta = delta / st->delta_old;
  st->count += 1;
  if (hist) hist[st->count] = delta;
  st->done = !(delta > st->thr);
}
// d = r + beta d (:184) -- skipped once the stop flag is up: d is internal, and A d of the later no-op iterations then reproduces the
// caller's Au of the last real iteration bit for bit
__global__ __launch_bounds__(kThreads) void cg_xpby_kernel(int n, const KState* __restrict__ st, const double* __restrict__ r,
                                                           double* __restrict__ d) {
  if (st->done) return;
  const double b = st->beta;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) d[i] = __dadd_rn(r[i], __dmul_rn(b, d[i]));
}

// ---- FCG (d4est_solver_fcg_improved.c) ----
// r_0 = rhs - Au_0 (axpyeqz(-1, Au, rhs, r), :177)
__global__ __launch_bounds__(kThreads) void fcg_init_vec_kernel(int n, const double* __restrict__ rhs, const double* __restrict__ Au,
                                                                double* __restrict__ r) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) r[i] = __dadd_rn(__dmul_rn(-1.0, Au[i]), rhs[i]);
}
// tol = atol + rtol sqrt(|r_0|^2) (:192)
__global__ void fcg_init_scalar_kernel(KState* st, double atol, double rtol) {
  st->delta0 = st->dot[0];
  st->tol = __dadd_rn(atol, __dmul_rn(rtol, sqrt(st->dot[0])));
  st->count = 0;
  st->done = 0;
}
// v.r, v.w (:236-238) and from k = 1 on v.q, r.r (:240-243), one pass; v may alias r (the identity preconditioner)
template <int NS>
__global__ __launch_bounds__(kThreads) void fcg_dots_kernel(int n, const double* v, const double* r, const double* __restrict__ w,
                                                            const double* __restrict__ q, double* __restrict__ partial) {
  double s[NS];
  for (int k = 0; k < NS; ++k) s[k] = 0.0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const double vi = v[i], ri = r[i];
    s[0] = fma(vi, ri, s[0]);
    s[1] = fma(vi, w[i], s[1]);
    if constexpr (NS == 4) {
      s[2] = fma(vi, q[i], s[2]);
      s[3] = fma(ri, ri, s[3]);
    }
  }
  block_store<NS>(s, partial);
}
// :255-283: alpha_k, beta_k, gamma_k from the reduced dots; rho; the stop test on |r_k| (taken after this iteration's update)
__global__ void fcg_step_kernel(KState* st, double* hist, int k) {
  const double alpha_k = st->dot[0], beta_k = st->dot[1];
  if (k > 0) {
    const double gamma_k = st->dot[2];
    st->coef = -gamma_k / st->rho;                                   // -gamma_k / rho_{k-1} (:262, :264)
    st->rho = __dadd_rn(beta_k, -(__dmul_rn(gamma_k, gamma_k) / st->rho));   // rho_k = beta_k - gamma_k^2 / rho_{k-1} (:266)
  } else {
    st->rho = beta_k;                                                  // :269
  }
  st->a = alpha_k / st->rho;     // :279
  st->na = -alpha_k / st->rho;   // :281
  const double rk = (k > 0) ? sqrt(st->dot[3]) : sqrt(st->delta0);
  if (hist) hist[k] = rk;
  st->count = k + 1;
  st->done = (k > 0 && rk <= st->tol) ? 1 : 0;   // :283
}
// k > 0: d = coef d + v, q = coef q + w (:262-264); k = 0: d = v, q = w (:272-275); then u = a d + u, r = na q + r (:279-281).
// v may alias r: both are read before r is written.
__global__ __launch_bounds__(kThreads) void fcg_update_kernel(int n, int first, const KState* __restrict__ st, const double* v,
                                                              const double* __restrict__ w, double* __restrict__ d, double* __restrict__ q,
                                                              double* __restrict__ u, double* r) {
  const double c = st->coef, a = st->a, na = st->na;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const double vi = v[i], wi = w[i], ri = r[i];
    const double di = first ? vi : __dadd_rn(__dmul_rn(c, d[i]), vi);
    const double qi = first ? wi : __dadd_rn(__dmul_rn(c, q[i]), wi);
    d[i] = di;
    q[i] = qi;
    u[i] = __dadd_rn(__dmul_rn(a, di), u[i]);
    r[i] = __dadd_rn(__dmul_rn(na, qi), ri);
  }
}

// the reduced sums into st->dot, through the plan's allreduce hook (one call, nsums scalars)
void reduce(d4est_hip_plan* plan, KrylovWork* w, int nblocks, int nsums) {
  hipLaunchKernelGGL(reduce_kernel, dim3(1), dim3(kThreads), 0, plan->stream, nblocks, nsums, w->partial, w->st);
  if (plan->allreduce_fn) plan->allreduce_fn(plan->comm_ctx, reinterpret_cast<double*>(w->st), nsums);   // st->dot is at offset 0
}

void read_flags(d4est_hip_plan* plan, KrylovWork* w) {
  HIP_CHECK(hipMemcpyAsync(w->flags_host, &w->st->done, 2 * sizeof(int), hipMemcpyDeviceToHost, plan->stream));
  HIP_CHECK(hipStreamSynchronize(plan->stream));
}

void read_history(d4est_hip_plan* plan, KrylovWork* w, int len, double* hist_out) {
  if (!hist_out || len <= 0) return;
  HIP_CHECK(hipMemcpyAsync(hist_out, w->hist, (size_t)len * sizeof(double), hipMemcpyDeviceToHost, plan->stream));
  HIP_CHECK(hipStreamSynchronize(plan->stream));
}

}  // namespace

static_assert(offsetof(KState, dot) == 0, "the allreduce hook reduces st->dot in place");
static_assert(offsetof(KState, count) == offsetof(KState, done) + sizeof(int), "done and count are read together");

int cg_solve(d4est_hip_plan* plan, double* u, const double* rhs, double* Au, int imax, double atol, double rtol, double* hist_out) {
  if (!u || !rhs || !Au) D4EST_HIP_ABORT("cg_solve: NULL vector");
  if (imax < 0) D4EST_HIP_ABORT("cg_solve: imax = %d", imax);
  ensure_solver_workspace(plan);
  KrylovWork* w = work(plan, imax + 1);
  const int n = plan->local_nodes, g = grid_for(n);
  double *r = w->vec[0], *d = w->vec[1];
  double* hist = hist_out ? w->hist : nullptr;
  const int check = plan->tuning[D4EST_HIP_TUNE_KRYLOV_CHECK] >= 1 ? plan->tuning[D4EST_HIP_TUNE_KRYLOV_CHECK] : kDefaultCheck;
  apply_operator(plan, u, Au);                                                                     // :116-127
  if (n > 0) hipLaunchKernelGGL(cg_init_vec_kernel, dim3(g), dim3(kThreads), 0, plan->stream, n, rhs, Au, r, d);
  hipLaunchKernelGGL(dot1_kernel, dim3(g), dim3(kThreads), 0, plan->stream, n, r, r, w->partial);  // :134
  reduce(plan, w, g, 1);                                                                           // :139-142
  hipLaunchKernelGGL(cg_init_scalar_kernel, dim3(1), dim3(1), 0, plan->stream, w->st, hist, atol, rtol);
  HIP_CHECK(hipGetLastError());
  int enqueued = 0;
  w->flags_host[0] = 0;
  w->flags_host[1] = 0;
  if (imax > 0) read_flags(plan, w);   // a start that already meets the test costs no operator apply
  while (!w->flags_host[0] && enqueued < imax) {
    const int batch = std::min(check, imax - enqueued);
    for (int b = 0; b < batch; ++b) {
      apply_operator(plan, d, Au);                                                                  // :150-161 (vecs->u = d)
      hipLaunchKernelGGL(dot1_kernel, dim3(g), dim3(kThreads), 0, plan->stream, n, d, Au, w->partial);   // :163
      reduce(plan, w, g, 1);                                                                        // :165-168
      hipLaunchKernelGGL(cg_alpha_step_kernel, dim3(1), dim3(1), 0, plan->stream, w->st);
      hipLaunchKernelGGL(cg_update_kernel, dim3(g), dim3(kThreads), 0, plan->stream, n, w->st, d, Au, u, r, w->partial);
      reduce(plan, w, g, 1);                                                                        // :177-181
      hipLaunchKernelGGL(cg_beta_step_kernel, dim3(1), dim3(1), 0, plan->stream, w->st, hist);
      if (n > 0) hipLaunchKernelGGL(cg_xpby_kernel, dim3(g), dim3(kThreads), 0, plan->stream, n, w->st, r, d);
    }
    HIP_CHECK(hipGetLastError());
    enqueued += batch;
    read_flags(plan, w);
  }
  const int count = w->flags_host[1];
  read_history(plan, w, count + 1, hist_out);
  return count;
}

int fcg_solve(d4est_hip_plan* plan, double* u, const double* rhs, double* Au, int imax, double atol, double rtol, d4est_hip_pc_fn pc,
              void* pc_ctx, double* hist_out) {
  if (!u || !rhs || !Au) D4EST_HIP_ABORT("fcg_solve: NULL vector");
  if (imax < 0) D4EST_HIP_ABORT("fcg_solve: imax = %d", imax);
  ensure_solver_workspace(plan);
  KrylovWork* w = work(plan, std::max(imax, 1));
  const int n = plan->local_nodes, g = grid_for(n);
  double *r = w->vec[0], *d = w->vec[1], *wk = w->vec[2], *q = w->vec[4];
  double* v = pc ? w->vec[3] : r;   // the identity preconditioner copies r to v (:215): reading r itself gives the same numbers
  double* hist = hist_out ? w->hist : nullptr;
  apply_operator(plan, u, Au);                                                                     // :163-174
  if (n > 0) hipLaunchKernelGGL(fcg_init_vec_kernel, dim3(g), dim3(kThreads), 0, plan->stream, n, rhs, Au, r);
  hipLaunchKernelGGL(dot1_kernel, dim3(g), dim3(kThreads), 0, plan->stream, n, r, r, w->partial);  // :180
  reduce(plan, w, g, 1);                                                                           // :182-190
  hipLaunchKernelGGL(fcg_init_scalar_kernel, dim3(1), dim3(1), 0, plan->stream, w->st, atol, rtol);
  HIP_CHECK(hipGetLastError());
  int count = 0;
  for (int k = 0; k < imax; ++k) {
    if (pc) pc(pc_ctx, r, v);                                                                      // :206-212
    apply_operator(plan, v, wk);                                                                   // :219-233
    if (k > 0) hipLaunchKernelGGL(fcg_dots_kernel<4>, dim3(g), dim3(kThreads), 0, plan->stream, n, v, r, wk, q, w->partial);
    else hipLaunchKernelGGL(fcg_dots_kernel<2>, dim3(g), dim3(kThreads), 0, plan->stream, n, v, r, wk, q, w->partial);
    reduce(plan, w, g, k > 0 ? 4 : 2);                                                             // :245-253
    hipLaunchKernelGGL(fcg_step_kernel, dim3(1), dim3(1), 0, plan->stream, w->st, hist, k);
    if (n > 0) hipLaunchKernelGGL(fcg_update_kernel, dim3(g), dim3(kThreads), 0, plan->stream, n, k == 0 ? 1 : 0, w->st, v, wk, d, q, u, r);
    HIP_CHECK(hipGetLastError());
    read_flags(plan, w);
    count = w->flags_host[1];
    if (w->flags_host[0]) break;                                                                   // :283-285
  }
  read_history(plan, w, count, hist_out);
  return count;
}

void krylov_destroy(d4est_hip_plan* plan) {
  KrylovWork* w = static_cast<KrylovWork*>(plan->krylov);
  if (!w) return;
  for (double* v : w->vec) (void)hipFree(v);
  (void)hipFree(w->partial);
  (void)hipFree(w->st);
  (void)hipFree(w->hist);
  if (w->flags_host) (void)hipHostFree(w->flags_host);
  delete w;
  plan->krylov = nullptr;
}

}  // namespace d4est_hip
