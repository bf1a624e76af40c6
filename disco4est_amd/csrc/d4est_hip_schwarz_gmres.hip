// Restarted GMRES as the subdomain solver of the additive Schwarz smoother, batched over all subdomains of a rank.
//
// Reference: d4est_solver_schwarz_subdomain_solver_gmres (src/Solver/d4est_solver_schwarz_subdomain_solver_gmres.c:165-443), selected
// by subdomain_solver = gmres with subdomain_inner_iter (the restart length mr).  The reference solves one subdomain after another; here
// all subdomains advance in lock-step: every inner step is ONE d4est_hip_schwarz_apply_over_subdomains on basis vector k of every
// subdomain, followed by one workgroup per subdomain that does the reference's arithmetic for that subdomain in the reference's order
// (:320-394).  k, rho, rho_tol, the Hessenberg column, the rotations and the stop flag of every subdomain live on the device; a
// subdomain that has met the stop test (rho <= rho_tol && rho <= tol_abs, :391 -- the AND is the reference's) is a no-op until its
// cycle's update kernel, as a finished subdomain of the CG is.  The host looks at the "still iterating" counter once per restart cycle.
//
// Three kernels:
//   start    (:246-296)  r = rhs - A x, rho = |r|, rho_tol in cycle 0, v_0 = r / rho, g = (rho, 0, ...); cycle 0 restricts the mesh
//                        residual the way schwarz_cg_init_kernel does (x = 0, so r = rhs and no apply is made)
//   arnoldi  (:320-394)  av, modified Gram-Schmidt against v_0 .. v_k (each h[j][k] after the previous subtraction), the conditional
//                        second pass, the normalisation, then one lane: earlier rotations on the column, the new rotation, g, rho, the flag
//   update   (:397-421)  back-substitution by one lane in the reference's order, then x += sum_j v_j y_j, j ascending
// Fields over the subdomains are stored at full element size with zeros outside the overlap, so the vector passes walk the flat list of
// a subdomain's restricted nodes (d_box_off) and give the sums of the reference's restricted vectors.  Reductions have a fixed shape
// (wave butterfly, then the four wave sums in a fixed order) and use no floating-point atomics: two runs give the same bits.
//
// Deviation: the reference divides by rho unguarded (:281); a subdomain with rho == 0 at a cycle start is treated as finished here
// (x unchanged, final_res = 0, final_iter as reached).
#include <algorithm>
#include <cmath>

#include "d4est_hip_schwarz_internal.h"

#ifndef D4EST_HIP_SCHWARZ_GMRES_MAX_MR
#error "include/d4est_hip.h must define D4EST_HIP_SCHWARZ_GMRES_MAX_MR"
#endif

namespace d4est_hip {

namespace {

constexpr int kThreads = 256;
constexpr int kRegNodes = 8;   // nodes per thread of the register-resident Arnoldi kernel: subdomains up to 2048 restricted nodes

// doubles per subdomain in d_gm_small: h ((mr + 1) x mr, row-major), c (mr), s (mr), g (mr + 1)
__host__ __device__ inline long long small_stride(int mr) { return (long long)(mr + 1) * mr + 2 * mr + (mr + 1); }

// fixed-shape sum over a workgroup of 256: xor butterfly inside each wavefront (every lane ends with the same bits), then the four
// wave sums in a fixed order
__device__ inline double wg_sum(double v, double* red4) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = v;
  __syncthreads();
  const double r = (red4[0] + red4[1]) + (red4[2] + red4[3]);
  __syncthreads();
  return r;
}

// mult_givens (:150-163), every product and sum rounded on its own
__device__ inline void mult_givens(double c, double s, int k, double* g) {
  const double g1 = __dsub_rn(__dmul_rn(c, g[k]), __dmul_rn(s, g[k + 1]));
  const double g2 = __dadd_rn(__dmul_rn(s, g[k]), __dmul_rn(c, g[k + 1]));
  g[k] = g1;
  g[k + 1] = g2;
}

// one lane, after the vector work of step k: :360-394.  hcol (LDS) holds h[0..k][k]; hk1 is h[k+1][k].
__device__ inline void givens_step(double* hcol, double hk1, int k, int mr, double* sm, double* rho_arr, int* state, int* final_iter,
                                   int s, int n_sub, double tol_abs) {
  double* h = sm;
  double* c = sm + (long long)(mr + 1) * mr;
  double* sn = c + mr;
  double* g = sn + mr;
  hcol[k + 1] = hk1;
  for (int j = 0; j < k; ++j) mult_givens(c[j], sn[j], j, hcol);                                   // :360-374
  const double hkk = hcol[k], hk1k = hcol[k + 1];
  const double mu = sqrt(__dadd_rn(__dmul_rn(hkk, hkk), __dmul_rn(hk1k, hk1k)));                   // :376
  const double ck = hkk / mu, sk = -hk1k / mu;                                                     // :377-378
  c[k] = ck;
  sn[k] = sk;
  hcol[k] = __dsub_rn(__dmul_rn(ck, hkk), __dmul_rn(sk, hk1k));                                    // :379
  hcol[k + 1] = 0.0;                                                                               // :380
  mult_givens(ck, sk, k, g);                                                                       // :381
  const double rho = fabs(g[k + 1]);                                                               // :383
  for (int i = 0; i <= k + 1; ++i) h[(long long)i * mr + k] = hcol[i];
  rho_arr[s] = rho;
  state[s] = k + 1;                                                                                // columns of this cycle: k_copy + 1
  final_iter[s] += 1;                                                                              // itr_used, :385
  if (rho <= rho_arr[n_sub + s] && rho <= tol_abs) state[n_sub + s] = 1;                           // :391, left alone until the update
}

}  // namespace

// Start of restart cycle `itr` for every subdomain.  itr == 0: the restricted residual is taken from the mesh vectors (FUSED: rhs - A u
// formed node by node, the one rounded operation of schwarz_cg_init_kernel<true>), x = 0 and r = rhs.  itr > 0: Ax holds A x.
template <bool FUSED>
__global__ __launch_bounds__(kThreads) void schwarz_gmres_start_kernel(const VirtDesc* __restrict__ vd, const int* __restrict__ sub_first,
                                                                       const int* __restrict__ box_first, const int* __restrict__ box_off,
                                                                       const double* __restrict__ r_mesh, const double* __restrict__ Au_mesh,
                                                                       double* __restrict__ x, double* __restrict__ rhs, double* __restrict__ v0,
                                                                       const double* __restrict__ Ax, int mr, double* __restrict__ small,
                                                                       double* __restrict__ rho_arr, int* __restrict__ state,
                                                                       int* __restrict__ final_iter, int* __restrict__ n_active, int n_sub,
                                                                       int itr, double tol_rel) {
  __shared__ double red4[4];
  const int s = blockIdx.x;
  if (itr > 0 && state[n_sub + s] == 2) return;
  const int first = box_first[s], cnt = box_first[s + 1] - first;
  double acc = 0.0;
  if (itr == 0) {
    for (int v = sub_first[s]; v < sub_first[s + 1]; ++v) {
      const VirtDesc q = vd[v];
      const int n3 = q.N * q.N * q.N;
      for (int n = threadIdx.x; n < n3; n += blockDim.x) {
        int i, j, k;
        double val = 0.0;
        if (in_overlap(q, n, i, j, k))
          val = FUSED ? __dadd_rn(r_mesh[q.src + n], __dmul_rn(-1.0, Au_mesh[q.src + n])) : r_mesh[q.src + n];
        x[q.dst + n] = 0.0;
        rhs[q.dst + n] = val;
        v0[q.dst + n] = val;
        acc += val * val;
      }
    }
  } else {
    for (int t = threadIdx.x; t < cnt; t += blockDim.x) {
      const int o = box_off[first + t];
      const double r = __dsub_rn(rhs[o], Ax[o]);                                                   // :263-266
      v0[o] = r;
      acc += r * r;
    }
  }
  const double rho = sqrt(wg_sum(acc, red4));                                                      // :268 (the sums order the writes above, too)
  if (rho != 0.0)
    for (int t = threadIdx.x; t < cnt; t += blockDim.x) {
      const int o = box_off[first + t];
      v0[o] = v0[o] / rho;                                                                         // :279-282
    }
  double* g = small + small_stride(mr) * s + (long long)(mr + 1) * mr + 2 * mr;
  for (int i = threadIdx.x; i <= mr; i += blockDim.x) g[i] = i == 0 ? rho : 0.0;                   // :284-288 (h: every entry read later is written first)
  if (threadIdx.x == 0) {
    rho_arr[s] = rho;
    state[s] = 0;
    if (itr == 0) {
      rho_arr[n_sub + s] = rho * tol_rel;                                                          // :274-277
      final_iter[s] = 0;
    }
    if (rho == 0.0) {   // nothing to solve (the reference would form 0 / 0 at :281): finished, x as it is
      state[n_sub + s] = 2;
      if (itr > 0) atomicSub(n_active, 1);
    } else {
      state[n_sub + s] = 0;
      if (itr == 0) atomicAdd(n_active, 1);
    }
  }
}

// Inner step k with the new vector w = v_{k+1} = A v_k held in registers (PT restricted nodes per thread) over all passes.
template <int PT>
__global__ __launch_bounds__(kThreads) void schwarz_gmres_arnoldi_kernel(const int* __restrict__ box_first, const int* __restrict__ box_off,
                                                                         double* __restrict__ V, long long vstride, int k, int mr,
                                                                         double* __restrict__ small, double* __restrict__ rho_arr,
                                                                         int* __restrict__ state, int* __restrict__ final_iter, int n_sub,
                                                                         double tol_abs) {
  __shared__ double red4[4];
  extern __shared__ double hcol[];   // mr + 1: column k of h, touched by lane 0 only
  const int s = blockIdx.x;
  if (state[n_sub + s] != 0) return;
  const int first = box_first[s], cnt = box_first[s + 1] - first;
  double* __restrict__ wp = V + (long long)(k + 1) * vstride;
  int o[PT];
  double w[PT], vj[PT];
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < PT; ++j) {
    const int t = threadIdx.x + kThreads * j;
    o[j] = (t < cnt) ? box_off[first + t] : -1;
    w[j] = (o[j] >= 0) ? wp[o[j]] : 0.0;
    acc += w[j] * w[j];
  }
  const double av = sqrt(wg_sum(acc, red4));                                                       // :321
  for (int jj = 0; jj <= k; ++jj) {                                                                // :323-331
    const double* __restrict__ vp = V + (long long)jj * vstride;
    acc = 0.0;
#pragma unroll
    for (int j = 0; j < PT; ++j) {
      vj[j] = (o[j] >= 0) ? vp[o[j]] : 0.0;
      acc += w[j] * vj[j];
    }
    const double hjk = wg_sum(acc, red4);
#pragma unroll
    for (int j = 0; j < PT; ++j) w[j] = w[j] - hjk * vj[j];
    if (threadIdx.x == 0) hcol[jj] = hjk;
  }
  acc = 0.0;
#pragma unroll
  for (int j = 0; j < PT; ++j) acc += w[j] * w[j];
  double hk1 = sqrt(wg_sum(acc, red4));                                                            // :334
  if (__dadd_rn(av, __dmul_rn(1.0e-03, hk1)) == av) {                                              // :336-350 (uniform over the workgroup)
    for (int jj = 0; jj <= k; ++jj) {
      const double* __restrict__ vp = V + (long long)jj * vstride;
      acc = 0.0;
#pragma unroll
      for (int j = 0; j < PT; ++j) {
        vj[j] = (o[j] >= 0) ? vp[o[j]] : 0.0;
        acc += w[j] * vj[j];
      }
      const double htmp = wg_sum(acc, red4);
#pragma unroll
      for (int j = 0; j < PT; ++j) w[j] = w[j] - htmp * vj[j];
      if (threadIdx.x == 0) hcol[jj] = hcol[jj] + htmp;
    }
    acc = 0.0;
#pragma unroll
    for (int j = 0; j < PT; ++j) acc += w[j] * w[j];
    hk1 = sqrt(wg_sum(acc, red4));
  }
#pragma unroll
  for (int j = 0; j < PT; ++j)
    if (o[j] >= 0) wp[o[j]] = (hk1 != 0.0) ? w[j] / hk1 : w[j];                                    // :352-358
  if (threadIdx.x == 0) givens_step(hcol, hk1, k, mr, small + small_stride(mr) * s, rho_arr, state, final_iter, s, n_sub, tol_abs);
}

// The same step for subdomains of any size: w stays in its basis slot and is re-read by every pass (each thread touches its own nodes only).
__global__ __launch_bounds__(kThreads) void schwarz_gmres_arnoldi_any_kernel(const int* __restrict__ box_first, const int* __restrict__ box_off,
                                                                             double* __restrict__ V, long long vstride, int k, int mr,
                                                                             double* __restrict__ small, double* __restrict__ rho_arr,
                                                                             int* __restrict__ state, int* __restrict__ final_iter, int n_sub,
                                                                             double tol_abs) {
  __shared__ double red4[4];
  extern __shared__ double hcol[];
  const int s = blockIdx.x;
  if (state[n_sub + s] != 0) return;
  const int* __restrict__ off = box_off + box_first[s];
  const int cnt = box_first[s + 1] - box_first[s];
  double* wp = V + (long long)(k + 1) * vstride;
  auto norm_w = [&]() {
    double a = 0.0;
    for (int t = threadIdx.x; t < cnt; t += kThreads) {
      const double wv = wp[off[t]];
      a += wv * wv;
    }
    return sqrt(wg_sum(a, red4));
  };
  auto project = [&](int jj) {   // returns w . v_jj and subtracts that multiple of v_jj from w
    const double* __restrict__ vp = V + (long long)jj * vstride;
    double a = 0.0;
    for (int t = threadIdx.x; t < cnt; t += kThreads) a += wp[off[t]] * vp[off[t]];
    const double hv = wg_sum(a, red4);
    for (int t = threadIdx.x; t < cnt; t += kThreads) wp[off[t]] = wp[off[t]] - hv * vp[off[t]];
    return hv;
  };
  const double av = norm_w();
  for (int jj = 0; jj <= k; ++jj) {
    const double hjk = project(jj);
    if (threadIdx.x == 0) hcol[jj] = hjk;
  }
  double hk1 = norm_w();
  if (__dadd_rn(av, __dmul_rn(1.0e-03, hk1)) == av) {
    for (int jj = 0; jj <= k; ++jj) {
      const double htmp = project(jj);
      if (threadIdx.x == 0) hcol[jj] = hcol[jj] + htmp;
    }
    hk1 = norm_w();
  }
  if (hk1 != 0.0)
    for (int t = threadIdx.x; t < cnt; t += kThreads) wp[off[t]] = wp[off[t]] / hk1;
  if (threadIdx.x == 0) givens_step(hcol, hk1, k, mr, small + small_stride(mr) * s, rho_arr, state, final_iter, s, n_sub, tol_abs);
}

// End of a restart cycle (:397-421): y by back-substitution with the columns reached, x += sum_j v_j y_j; a subdomain whose flag is up
// leaves the restart loop (:418-421).
__global__ __launch_bounds__(kThreads) void schwarz_gmres_update_kernel(const int* __restrict__ box_first, const int* __restrict__ box_off,
                                                                        const double* __restrict__ V, long long vstride, double* __restrict__ x,
                                                                        int mr, const double* __restrict__ small, int* __restrict__ state,
                                                                        int* __restrict__ n_active, int n_sub) {
  extern __shared__ double lds[];   // one row of h (mr), y (mr)
  const int s = blockIdx.x;
  if (state[n_sub + s] == 2) return;
  const int kk = state[s];          // columns of this cycle (>= 1: the subdomain was iterating at step 0)
  if (kk <= 0) return;
  double* row = lds;
  double* y = lds + mr;
  const double* sm = small + small_stride(mr) * s;
  const double* g = sm + (long long)(mr + 1) * mr + 2 * mr;
  // :399-408, one row at a time: the workgroup stages row i of the rotated h in LDS, one lane subtracts in the reference's order
  // (j ascending) -- the chain is serial by nature, and one row keeps the LDS need at 2 mr doubles whatever the restart length
  for (int i = kk - 1; i >= 0; --i) {
    for (int j = i + threadIdx.x; j < kk; j += kThreads) row[j] = sm[(long long)i * mr + j];
    __syncthreads();
    if (threadIdx.x == 0) {
      double yi = g[i];
      for (int j = i + 1; j < kk; ++j) yi = __dsub_rn(yi, __dmul_rn(row[j], y[j]));
      y[i] = yi / row[i];
    }
    __syncthreads();
  }
  const int* __restrict__ off = box_off + box_first[s];
  const int cnt = box_first[s + 1] - box_first[s];
  for (int t = threadIdx.x; t < cnt; t += kThreads) {                                              // :410-416
    const int o = off[t];
    double xv = x[o];
    for (int j = 0; j < kk; ++j) xv = __dadd_rn(xv, __dmul_rn(V[(long long)j * vstride + o], y[j]));
    x[o] = xv;
  }
  if (threadIdx.x == 0 && state[n_sub + s] == 1) {
    state[n_sub + s] = 2;
    atomicSub(n_active, 1);
  }
}

void schwarz_gmres_release(d4est_hip_schwarz* sz) {
  void* ptrs[] = {sz->d_gm_V, sz->d_gm_small, sz->d_gm_rho, sz->d_gm_state};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  sz->d_gm_V = sz->d_gm_small = sz->d_gm_rho = nullptr;
  sz->d_gm_state = nullptr;
  sz->gmres_bytes = 0;
  sz->gmres_mr = 0;
  sz->solver_kind = 0;
  sz->last_solver = 0;   // (get_info must not look for the rho array any more)
}

int schwarz_gmres_solve(d4est_hip_schwarz* sz, const double* r_mesh, const double* Au_mesh, int itr_max, double tol_abs, double tol_rel) {
  if (!sz->d_gm_V) D4EST_HIP_ABORT("schwarz: the GMRES workspace is missing (d4est_hip_schwarz_set_subdomain_solver)");
  hipStream_t st = sz->plan->stream;
  const int mr = sz->gmres_mr, ns = sz->n_sub;
  const long long vs = sz->nodal_size;
  double* V = sz->d_gm_V;
  const dim3 grid(ns), block(kThreads);
  const size_t lds_col = (size_t)(mr + 2) * sizeof(double), lds_upd = 2 * (size_t)mr * sizeof(double);
  int applies = 0;
  for (int itr = 0; itr < itr_max; ++itr) {                                                        // :243
    if (itr > 0) {
      // one look at the "still iterating" counter per restart cycle; in cycle 0 every subdomain with a non-zero residual iterates
      int n_active = 0;
      HIP_CHECK(hipMemcpyAsync(&n_active, sz->d_n_active, sizeof(int), hipMemcpyDeviceToHost, st));
      HIP_CHECK(hipStreamSynchronize(st));
      sz->host_reads++;
      if (n_active == 0) break;
      d4est_hip_schwarz_apply_over_subdomains(sz, sz->d_du, V + vs);                               // :246-261 (v_1 is free until step 0)
      ++applies;
    }
    if (Au_mesh)
      hipLaunchKernelGGL(schwarz_gmres_start_kernel<true>, grid, block, 0, st, sz->d_vd, sz->d_sub_first, sz->d_box_first, sz->d_box_off, r_mesh,
                         Au_mesh, sz->d_du, sz->d_r, V, V + vs, mr, sz->d_gm_small, sz->d_gm_rho, sz->d_gm_state, sz->d_final_iter,
                         sz->d_n_active, ns, itr, tol_rel);
    else
      hipLaunchKernelGGL(schwarz_gmres_start_kernel<false>, grid, block, 0, st, sz->d_vd, sz->d_sub_first, sz->d_box_first, sz->d_box_off, r_mesh,
                         (const double*)nullptr, sz->d_du, sz->d_r, V, V + vs, mr, sz->d_gm_small, sz->d_gm_rho, sz->d_gm_state,
                         sz->d_final_iter, sz->d_n_active, ns, itr, tol_rel);
    HIP_CHECK(hipGetLastError());
    for (int k = 0; k < mr; ++k) {                                                                 // :298
      d4est_hip_schwarz_apply_over_subdomains(sz, V + (long long)k * vs, V + (long long)(k + 1) * vs);   // :302-317
      ++applies;
      if (sz->max_box_nodes <= kThreads * kRegNodes)
        hipLaunchKernelGGL(schwarz_gmres_arnoldi_kernel<kRegNodes>, grid, block, lds_col, st, sz->d_box_first, sz->d_box_off, V, vs, k, mr,
                           sz->d_gm_small, sz->d_gm_rho, sz->d_gm_state, sz->d_final_iter, ns, tol_abs);
      else
        hipLaunchKernelGGL(schwarz_gmres_arnoldi_any_kernel, grid, block, lds_col, st, sz->d_box_first, sz->d_box_off, V, vs, k, mr,
                           sz->d_gm_small, sz->d_gm_rho, sz->d_gm_state, sz->d_final_iter, ns, tol_abs);
      HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(schwarz_gmres_update_kernel, grid, block, lds_upd, st, sz->d_box_first, sz->d_box_off, V, vs, sz->d_du, mr,
                       sz->d_gm_small, sz->d_gm_state, sz->d_n_active, ns);
    HIP_CHECK(hipGetLastError());
  }
  return applies;
}

}  // namespace d4est_hip

using namespace d4est_hip;

extern "C" {

int d4est_hip_schwarz_set_subdomain_solver(d4est_hip_schwarz_t* sz, int kind, int subdomain_inner_iter) {
  if (!sz || !sz->plan) D4EST_HIP_ABORT("schwarz_set_subdomain_solver: NULL schwarz handle");
  if (kind == 0) {
    HIP_CHECK(hipStreamSynchronize(sz->plan->stream));
    schwarz_gmres_release(sz);
    return 0;
  }
  if (kind != 1) return 1;
  const int mr = subdomain_inner_iter;
  if (mr <= 0) return 2;
  if (sz->n_sub > 0 && mr > sz->min_box_nodes) return 3;   // "nodes < mr", subdomain_solver_gmres.c:203-205
  if (mr > D4EST_HIP_SCHWARZ_GMRES_MAX_MR) return 4;
  if (!sz->d_box_off) D4EST_HIP_ABORT("schwarz_set_subdomain_solver: the restricted node lists exceed 32-bit offsets");
  HIP_CHECK(hipStreamSynchronize(sz->plan->stream));
  schwarz_gmres_release(sz);
  const size_t ns = (size_t)sz->n_sub;
  const size_t nV = (size_t)(mr + 1) * (size_t)sz->nodal_size, nsmall = ns * (size_t)small_stride(mr);
  auto alloc0 = [](size_t bytes) {   // zero-filled: a subdomain that is a no-op from the start leaves its slots as they are
    void* p = nullptr;
    HIP_CHECK(hipMalloc(&p, std::max<size_t>(bytes, 8)));
    HIP_CHECK(hipMemset(p, 0, std::max<size_t>(bytes, 8)));
    return p;
  };
  sz->d_gm_V = (double*)alloc0(nV * sizeof(double));
  sz->d_gm_small = (double*)alloc0(nsmall * sizeof(double));
  sz->d_gm_rho = (double*)alloc0(2 * ns * sizeof(double));
  sz->d_gm_state = (int*)alloc0(2 * ns * sizeof(int));
  sz->gmres_bytes = (long long)((nV + nsmall + 2 * ns) * sizeof(double) + 2 * ns * sizeof(int));
  sz->gmres_mr = mr;
  sz->solver_kind = 1;
  return 0;
}

void d4est_hip_schwarz_subdomain_solver(const d4est_hip_schwarz_t* sz, int* kind, int* subdomain_inner_iter, long long* workspace_bytes) {
  if (!sz || !sz->plan) D4EST_HIP_ABORT("schwarz_subdomain_solver: NULL schwarz handle");
  if (kind) *kind = sz->solver_kind;
  if (subdomain_inner_iter) *subdomain_inner_iter = sz->solver_kind == 1 ? sz->gmres_mr : 0;
  if (workspace_bytes) *workspace_bytes = sz->gmres_bytes;
}

}  // extern "C"
