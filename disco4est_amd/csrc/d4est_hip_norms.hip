// The error norms of d4est_norms_save (src/IO/d4est_norms.c:380-560) on a plan: L2, L-infinity, the IP energy norm and the masked sum
// that also gives the energy_estimator column.  Results are this rank's local sums / maxima, left on the device; the reduction over
// ranks and the square root stay with the caller (the reference's sc_reduce sits outside the compute functions).
//
//   error field  err = |u - u_compare| at the Lobatto nodes (d4est_norms.c:467-468): the absolute value BEFORE any interpolation
//   L2           norm2_e = v_e^T M_e v_e = sum_q w J (V v_e)^2 at the element's deg_quad (d4est_mesh_compute_l2_norm_sqr,
//                src/Mesh/d4est_mesh.c:2299-2374); l2_array[e] is written for every element, the sum leaves out the skipped ones
//   L-infinity   max(0, max_i v_i) over the nodes of the non-skipped elements (d4est_norms_fcn_Linfty, d4est_norms.c:64-117): the
//                maximum of the VALUES, not of their magnitudes, and the running maximum starts at 0 -- as the reference has it
//   IP energy    d4est_ip_energy_norm_compute (src/dGMath/d4est_ip_energy_norm.c:286-448), squared, total = (volume + boundary) + interface
//     volume     sum_d sum_q w J (du/dx_d)^2, du/dx_d = sum_i rst_xyz[i][d] V(D_i u)   (d4est_gradient_l2_norm, d4est_gradient.c:71-124)
//     interface  per local side with an interior mortar: 3 sum_k w_k sj_k pen_k sum_d n_d^2 (u_m - u_p)^2   (:210-270)
//     boundary   per boundary side: sum_k w_k sj_k pen(deg, h_k, deg, h_k) sum_d n_d^2 u_m^2, no Dirichlet data   (:70-102)
//
// Quirks of the reference that are reproduced:
//   * the factor 3 of the interface term: the node value already sums over d, and is then added once more per direction (:251-268);
//   * pen = u_penalty_fcn(...) enters ONCE (a penalty_calc_t of d4est_laplacian_flux_sipg.c:945-1005), where the estimator squares its
//     prefactors;
//   * a face is visited from both of its local sides, so an interior face between two local elements counts twice; a ghost side adds
//     from the local side only; a big hanging side adds its four sub-mortars, a small side its own (the estimator's side walk).
// One deviation in rounding only: the plan keeps the volume geometry as the combined symmetric metric G_ij = w J sum_d rst_xyz[i][d]
// rst_xyz[j][d] (every geometry entry point produces it; rst_xyz itself is not kept), so the volume term is evaluated as
// sum_q sum_ij G_ij g_i g_j with g_i = V(D_i u) -- the same quadratic form, expanded.
//
// Kernels (the plan's stream, no host synchronisation, no floating-point atomics; every reduction has a fixed order, so every output
// is bit-identical from call to call):
//   norms_error_kernel     elementwise
//   norms_l2_kernel        per (deg, deg_quad) bucket, one 256-thread workgroup per element: the body of the estimator's residual term
//                          (d4est_hip_elem_l2.h)
//   norms_elem_max_kernel  per bucket, one wavefront per element: max(0, max_i v_i)
//   norms_gradient_kernel  per bucket, one 256-thread workgroup per element, all in LDS: u_e and D_0 u, D_1 u, D_2 u (4 N^3), then per
//                          z-slab c of the quadrature nodes the z- and x-interpolation of the three (N^2, NQ N each), the
//                          y-interpolation in registers and the metric sum; fixed tree reduction.
//                          LDS LIMIT: (4 N^3 + 3 (N^2 + NQ N) + NQ N + N^2 + 256) doubles <= 160 KB, which holds for p <= 15 at
//                          every deg_quad a plan can have (p = 15, deg_quad = 17: 147 KB); a bucket beyond it aborts with a message.
//   norms_face_kernel      one wavefront per element walks the element's mortar records (faces_estimator_mortars) over trace blocks
//                          from launch_traces_all in a buffer the norms own, with ONE factor per mortar quadrature node formed at
//                          set-up (norms_geom_kernel, inside faces_set_geometry: given, brick and analytic geometry all reach it):
//                          c = w sj pen |n|^2
//   norms_reduce_kernel    one 1024-thread workgroup: masked fixed-order sum (or maximum) of per-element arrays
#include <algorithm>
#include <cmath>

#include "d4est_hip_elem_l2.h"
#include "d4est_hip_internal.h"
#include "d4est_hip_penalty.h"
#include "d4est_hip_tables.h"
#include "d4est_hip_wave.h"

namespace d4est_hip {

struct NormHost {
  double* d_elem = nullptr;      // 4 n_elements scratch: per-element values when the caller wants none (3 terms) / per-element maxima
  // IP energy norm only (norms_setup)
  bool has_faces = false;
  EstMortar* d_mortars = nullptr;
  int n_mortars = 0;
  int* d_elem_first = nullptr;
  double* d_fac = nullptr;       // w sj pen |n|^2 per mortar quadrature node, at gidx
  double* d_trace = nullptr;     // the norms' own local / ghost trace buffers
  double* d_ghost = nullptr;
};

static NormHost* norms_of(d4est_hip_plan* plan) {
  if (!plan->norms) {
    NormHost* x = new NormHost();
    HIP_CHECK(hipMalloc(&x->d_elem, std::max<size_t>(4 * (size_t)plan->n_elements, 1) * sizeof(double)));
    plan->norms = x;
  }
  return static_cast<NormHost*>(plan->norms);
}

__global__ __launch_bounds__(256) void norms_error_kernel(int n, const double* __restrict__ u, const double* __restrict__ uc,
                                                          double* __restrict__ err) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) err[i] = fabs(uc ? u[i] - uc[i] : u[i]);
}

__global__ __launch_bounds__(256) void norms_l2_kernel(const double* __restrict__ v, const double* __restrict__ J,
                                                       const int* __restrict__ elem_ids, const int* __restrict__ ns_list,
                                                       const int* __restrict__ qs_list, int n_elem, const double* __restrict__ B,
                                                       const double* __restrict__ w, int N, int NQ, double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const ElemL2Lds lds = elem_l2_lds(smem, B, w, N, NQ);
  for (int el = blockIdx.x; el < n_elem; el += gridDim.x) {
    const double sum = elem_l2_sqr(lds, v + ns_list[el], J + qs_list[el], N, NQ);
    if (threadIdx.x == 0) out[elem_ids[el]] = sum;
    __syncthreads();
  }
}

__global__ __launch_bounds__(64) void norms_elem_max_kernel(const double* __restrict__ v, const int* __restrict__ elem_ids,
                                                            const int* __restrict__ ns_list, int n_elem, int N3,
                                                            double* __restrict__ out) {
  for (int el = blockIdx.x; el < n_elem; el += gridDim.x) {
    const double* ve = v + ns_list[el];
    double m = 0.0;   // (d4est_norms.c:74: the running maximum starts at 0)
    for (int i = threadIdx.x; i < N3; i += blockDim.x) {
      const double t = ve[i];
      m = (t > m) ? t : m;
    }
    for (int s = 32; s > 0; s >>= 1) {
      const double o = __shfl_xor(m, s, 64);
      m = (o > m) ? o : m;
    }
    if (threadIdx.x == 0) out[elem_ids[el]] = m;
  }
}

// dynamic LDS of norms_gradient_kernel for one bucket
static size_t gradient_lds_bytes(int N, int NQ) {
  return (size_t)(4 * N * N * N + 3 * (N * N + NQ * N) + NQ * N + N * N + 256) * sizeof(double);
}

// the volume term of the elements of one (deg, deg_quad) bucket: one 256-thread workgroup per element
__global__ __launch_bounds__(256) void norms_gradient_kernel(const double* __restrict__ u, const double* __restrict__ metric,
                                                             const int* __restrict__ elem_ids, const int* __restrict__ ns_list,
                                                             const int* __restrict__ qs_list, int n_elem, const double* __restrict__ B,
                                                             const double* __restrict__ D, int N, int NQ, double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int N2 = N * N, N3 = N2 * N, NQ2 = NQ * NQ, NQ3 = NQ2 * NQ;
  double* U = smem;                 // u_e
  double* T = U + N3;               // D_0 u, D_1 u, D_2 u at the Lobatto nodes (N3 each)
  double* Z = T + 3 * N3;           // per direction, slab c: (i, j) after the z-interpolation
  double* Y = Z + 3 * N2;           // (a, j) after the x-interpolation
  double* Bs = Y + 3 * NQ * N;      // NQ x N
  double* Ds = Bs + NQ * N;         // N x N
  double* red = Ds + N2;            // 256
  for (int i = threadIdx.x; i < NQ * N; i += blockDim.x) Bs[i] = B[i];
  for (int i = threadIdx.x; i < N2; i += blockDim.x) Ds[i] = D[i];
  for (int el = blockIdx.x; el < n_elem; el += gridDim.x) {
    const double* ue = u + ns_list[el];
    const double* M = metric + (size_t)6 * qs_list[el];   // [c][q], c in (rr, rs, rt, ss, st, tt), weights and J folded in
    for (int i = threadIdx.x; i < N3; i += blockDim.x) U[i] = ue[i];
    __syncthreads();
    for (int idx = threadIdx.x; idx < 3 * N3; idx += blockDim.x) {   // d4est_operators_apply_dij, directions 0 (fastest index) .. 2
      const int dir = idx / N3, n = idx % N3;
      const int i = n % N, j = (n / N) % N, k = n / N2;
      const int row = (dir == 0) ? i : (dir == 1) ? j : k;
      const int stride = (dir == 0) ? 1 : (dir == 1) ? N : N2;
      const int base = n - row * stride;
      double t = 0.0;
      for (int l = 0; l < N; ++l) t = fma(Ds[row * N + l], U[base + l * stride], t);
      T[idx] = t;
    }
    __syncthreads();
    double acc = 0.0;
    for (int c = 0; c < NQ; ++c) {
      for (int idx = threadIdx.x; idx < 3 * N2; idx += blockDim.x) {        // z: Z(i, j) = sum_k B(c, k) T(i, j, k)
        const int dir = idx / N2, ij = idx % N2;
        const double* Td = T + dir * N3;
        double t = 0.0;
        for (int k = 0; k < N; ++k) t = fma(Bs[c * N + k], Td[ij + N2 * k], t);
        Z[idx] = t;
      }
      __syncthreads();
      for (int idx = threadIdx.x; idx < 3 * NQ * N; idx += blockDim.x) {    // x: Y(a, j) = sum_i B(a, i) Z(i, j)
        const int dir = idx / (NQ * N), aj = idx % (NQ * N);
        const int a = aj % NQ, j = aj / NQ;
        const double* Zd = Z + dir * N2;
        double t = 0.0;
        for (int i = 0; i < N; ++i) t = fma(Bs[a * N + i], Zd[i + N * j], t);
        Y[idx] = t;
      }
      __syncthreads();
      for (int ab = threadIdx.x; ab < NQ2; ab += blockDim.x) {              // y, then the metric sum
        const int a = ab % NQ, b = ab / NQ;
        double g[3];
        for (int dir = 0; dir < 3; ++dir) {
          const double* Yd = Y + dir * NQ * N;
          double t = 0.0;
          for (int j = 0; j < N; ++j) t = fma(Bs[b * N + j], Yd[a + NQ * j], t);
          g[dir] = t;
        }
        const size_t q = (size_t)ab + (size_t)NQ2 * c;
        acc += M[q] * g[0] * g[0] + M[3 * (size_t)NQ3 + q] * g[1] * g[1] + M[5 * (size_t)NQ3 + q] * g[2] * g[2] +
               2.0 * (M[(size_t)NQ3 + q] * g[0] * g[1] + M[2 * (size_t)NQ3 + q] * g[0] * g[2] + M[4 * (size_t)NQ3 + q] * g[1] * g[2]);
      }
      // (no barrier here: the next slab's z pass writes Z, last read before the barrier above, and its x pass, which writes Y, comes
      // after that slab's first barrier)
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) out[elem_ids[el]] = red[0];
    __syncthreads();
  }
}

__global__ __launch_bounds__(64) void norms_geom_kernel(const EstMortar* __restrict__ md, int n_m, const double* __restrict__ sj,
                                                        const double* __restrict__ nrm, const double* __restrict__ hm,
                                                        const double* __restrict__ hp, const double* __restrict__ wt, int wt_ld, int fcn,
                                                        double c, double* __restrict__ fac) {
  for (int r = blockIdx.x; r < n_m; r += gridDim.x) {
    const EstMortar m = md[r];
    const int NQ = m.NQ, T = NQ * NQ;
    const size_t S = (size_t)m.S, TT = (size_t)m.Ttot;
    const double* w = wt + (size_t)(NQ - 1) * wt_ld;
    double* out = fac + (size_t)m.gidx;
    for (int k = threadIdx.x; k < T; k += blockDim.x) {
      double nn = 0.0;
      for (int x = 0; x < 3; ++x) {
        const double nx = nrm[3 * S + (size_t)x * TT + m.off + k];
        nn += nx * nx;
      }
      const double hmk = hm[S + m.off + k];
      // boundary: pen(deg, h, deg, h) (d4est_ip_energy_norm.c:70-79); interface: the two elements of the mortar (:214-221)
      const double pen = (m.kind == 0) ? sipg_penalty(fcn, m.deg_m, hmk, m.deg_m, hmk, c)
                                       : sipg_penalty(fcn, m.deg_m, hmk, m.deg_p, hp[S + m.off + k], c);
      out[k] = w[k % NQ] * w[k / NQ] * sj[S + m.off + k] * pen * nn;
    }
  }
}

// boundary and interface terms: one wavefront per element, lanes over the mortar quadrature nodes, mortars in sequence
__global__ __launch_bounds__(64) void norms_face_kernel(const double* __restrict__ qtrace, const double* __restrict__ ghost_qtrace,
                                                        const EstMortar* __restrict__ md, const int* __restrict__ elem_first,
                                                        const double* __restrict__ fac, int n_elem, double* __restrict__ terms) {
  for (int e = blockIdx.x; e < n_elem; e += gridDim.x) {
    double tb = 0.0, ti = 0.0;
    for (int r = elem_first[e]; r < elem_first[e + 1]; ++r) {
      const EstMortar m = md[r];
      const int T = m.NQ * m.NQ;
      const double* f = fac + (size_t)m.gidx;
      const double* qm = qtrace + m.qoff;
      if (m.kind == 0) {
        for (int k = threadIdx.x; k < T; k += blockDim.x) tb += f[k] * qm[k] * qm[k];
        continue;
      }
      const double* qp = ((m.kind == 2) ? ghost_qtrace : qtrace) + m.nbr_qoff;
      for (int k = threadIdx.x; k < T; k += blockDim.x) {
        const int kp = reorder_index(m.code, m.NQ - 1, k % m.NQ, k / m.NQ);
        const double du = qm[k] - qp[kp + m.u_shift];
        ti += f[k] * du * du;
      }
    }
    for (int s = 32; s > 0; s >>= 1) {   // fixed-order butterfly over the wavefront
      tb += __shfl_xor(tb, s, 64);
      ti += __shfl_xor(ti, s, 64);
    }
    if (threadIdx.x == 0) {
      terms[(size_t)n_elem + e] = tb;
      terms[2 * (size_t)n_elem + e] = 3.0 * ti;   // (d4est_ip_energy_norm.c:251-268: the node sum once per direction)
    }
  }
}

// out[a] = the masked fixed-order sum (is_max: maximum, from 0) of in[a n .. a n + n), a < n_arrays; with_total: out[n_arrays] = the sum
// of the n_arrays results in order.  One workgroup: thread t takes elements t, t + 1024, ... in order, then a tree over the threads.
__global__ __launch_bounds__(1024) void norms_reduce_kernel(const double* __restrict__ in, const int* __restrict__ skip, int n, int n_arrays,
                                                            int is_max, int with_total, double* __restrict__ out) {
  __shared__ double red[1024];
  double total = 0.0;
  for (int a = 0; a < n_arrays; ++a) {
    const double* x = in + (size_t)a * n;
    double acc = 0.0;
    for (int e = threadIdx.x; e < n; e += blockDim.x) {
      if (skip && skip[e]) continue;
      const double t = x[e];
      acc = is_max ? ((t > acc) ? t : acc) : acc + t;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) {
        const double o = red[threadIdx.x + s], me = red[threadIdx.x];
        red[threadIdx.x] = is_max ? ((o > me) ? o : me) : me + o;
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      out[a] = red[0];
      total += red[0];
    }
    __syncthreads();
  }
  if (with_total && threadIdx.x == 0) out[n_arrays] = total;
}

static void launch_reduce(d4est_hip_plan* plan, const double* in, const int* skip, int n_arrays, int is_max, int with_total, double* out) {
  hipLaunchKernelGGL(norms_reduce_kernel, dim3(1), dim3(1024), 0, plan->stream, in, skip, plan->n_elements, n_arrays, is_max, with_total, out);
  HIP_CHECK(hipGetLastError());
}

void norms_destroy(d4est_hip_plan* plan) {
  NormHost* x = static_cast<NormHost*>(plan->norms);
  if (!x) return;
  (void)hipFree(x->d_elem); (void)hipFree(x->d_mortars); (void)hipFree(x->d_elem_first); (void)hipFree(x->d_fac);
  (void)hipFree(x->d_trace); (void)hipFree(x->d_ghost);
  delete x;
  plan->norms = nullptr;
}

void norms_setup(d4est_hip_plan* plan, const double* sj, const double* n, const double* hm, const double* hp) {
  norms_destroy(plan);
  NormHost* x = norms_of(plan);
  const double *face_ops, *hp_ops;
  const MortarRecords rec = mortar_records_upload(plan, "plan_set_energy_norm", &face_ops, &hp_ops);
  const int max_nq = rec.max_nq;
  x->n_mortars = rec.n_mortars;
  x->d_mortars = rec.d_mortars;
  x->d_elem_first = rec.d_elem_first;
  double* d_wt = rec.d_wt;
  const size_t tm = std::max<size_t>((size_t)plan->total_mortar_nodes, 1);
  HIP_CHECK(hipMalloc(&x->d_fac, tm * sizeof(double)));
  HIP_CHECK(hipMemsetAsync(x->d_fac, 0, tm * sizeof(double), plan->stream));
  HIP_CHECK(hipMalloc(&x->d_trace, std::max<size_t>((size_t)plan->local_trace_doubles, 1) * sizeof(double)));
  if (plan->ghost_trace_doubles > 0) HIP_CHECK(hipMalloc(&x->d_ghost, (size_t)plan->ghost_trace_doubles * sizeof(double)));
  if (x->n_mortars > 0)
    hipLaunchKernelGGL(norms_geom_kernel, dim3(std::min(x->n_mortars, 8192)), dim3(64), 0, plan->stream, x->d_mortars, x->n_mortars, sj, n, hm,
                       hp, d_wt, max_nq, plan->norm_fcn, plan->norm_prefactor, x->d_fac);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(plan->stream));   // (set-up: the caller's factor arrays may be freed after it)
  HIP_CHECK(hipFree(d_wt));
  x->has_faces = true;
}

void norms_error(d4est_hip_plan* plan, const double* u, const double* u_compare, double* err) {
  if (!u || !err) D4EST_HIP_ABORT("norms_error: NULL u / err");
  const int n = plan->local_nodes;
  if (n == 0) return;
  hipLaunchKernelGGL(norms_error_kernel, dim3(std::max(1, std::min((n + 255) / 256, 4096))), dim3(256), 0, plan->stream, n, u, u_compare, err);
  HIP_CHECK(hipGetLastError());
}

// the two kernels below may need more dynamic LDS than the default 64 KB.  The attribute belongs to the kernel, not to a plan, so it is
// raised once per device (set_lds_limit), to the kernel's own limit (kElemL2MaxLds), the first time a bucket beyond 64 KB is launched: no
// runtime call on the later launches, and no plan can lower what another plan needs.

void norms_l2_sqr(d4est_hip_plan* plan, const double* v, const int* skip, double* l2_array, double* sum) {
  if (!plan->has_geometry) D4EST_HIP_ABORT("norm_l2_sqr: the plan has no volume geometry (plan_set_geometry)");
  if (!v || !sum) D4EST_HIP_ABORT("norm_l2_sqr: NULL v / sum");
  NormHost* x = norms_of(plan);
  double* arr = l2_array ? l2_array : x->d_elem;
  for (const Bucket& bk : plan->buckets) {
    if (bk.n_elem == 0) continue;
    const size_t lds = elem_l2_lds_bytes(bk.N, bk.NQ);
    if (lds > kElemL2MaxLds) D4EST_HIP_ABORT("norm_l2_sqr: (deg, deg_quad) = (%d, %d) needs %zu bytes of LDS", bk.deg, bk.deg_quad, lds);
    if (lds > 64 * 1024) set_lds_limit(norms_l2_kernel, kElemL2MaxLds);
    hipLaunchKernelGGL(norms_l2_kernel, dim3(std::min(bk.n_elem, 16384)), dim3(256), lds, plan->stream, v, plan->d_J,
                       plan->d_elem_ids + bk.elem_offset, plan->d_ns_list + bk.elem_offset, plan->d_qs_list + bk.elem_offset, bk.n_elem, bk.d_B,
                       bk.d_w, bk.N, bk.NQ, arr);
    HIP_CHECK(hipGetLastError());
  }
  launch_reduce(plan, arr, skip, 1, 0, 0, sum);
}

void norms_linfty(d4est_hip_plan* plan, const double* v, const int* skip, double* max_out) {
  if (!v || !max_out) D4EST_HIP_ABORT("norm_linfty: NULL v / max");
  NormHost* x = norms_of(plan);
  for (const Bucket& bk : plan->buckets) {
    if (bk.n_elem == 0) continue;
    hipLaunchKernelGGL(norms_elem_max_kernel, dim3(std::min(bk.n_elem, 65536)), dim3(64), 0, plan->stream, v, plan->d_elem_ids + bk.elem_offset,
                       plan->d_ns_list + bk.elem_offset, bk.n_elem, bk.N * bk.N * bk.N, x->d_elem);
    HIP_CHECK(hipGetLastError());
  }
  launch_reduce(plan, x->d_elem, skip, 1, 1, 0, max_out);
}

void norms_masked_sum(d4est_hip_plan* plan, const double* elem, const int* skip, double* sum) {
  if (!elem || !sum) D4EST_HIP_ABORT("masked_sum: NULL elem / sum");
  launch_reduce(plan, elem, skip, 1, 0, 0, sum);
}

void norms_ip_energy_sqr(d4est_hip_plan* plan, const double* v, const double* ghost_trace, double* elem_terms, double* sums) {
  if (!plan->norm_requested) D4EST_HIP_ABORT("ip_energy_norm_sqr: the plan has no energy-norm set-up (d4est_hip_plan_set_energy_norm)");
  NormHost* x = static_cast<NormHost*>(plan->norms);
  if (!x || !x->has_faces) D4EST_HIP_ABORT("ip_energy_norm_sqr: call d4est_hip_plan_set_energy_norm before the mortar factors (plan_set_mortar_geometry)");
  if (!plan->has_geometry) D4EST_HIP_ABORT("ip_energy_norm_sqr: the plan has no volume geometry (plan_set_geometry)");
  if (!v || !sums) D4EST_HIP_ABORT("ip_energy_norm_sqr: NULL v / sums");
  const int ne = plan->n_elements;
  double* t = elem_terms ? elem_terms : x->d_elem;
  if (ne > 0) {
    // every side's trace block; ghost blocks from the caller or through the exchange hooks (as estimator_compute)
    launch_traces_all(plan, v, x->d_trace);
    const double* gt = ghost_trace;
    if (!gt && plan->ghost_trace_doubles > 0) {
      if (!plan->exchange_fn) D4EST_HIP_ABORT("ip_energy_norm_sqr: plan has ghost sides but neither a ghost trace nor an exchange callback (plan_set_comm)");
      plan->exchange_fn(plan->comm_ctx, 0, x->d_trace, x->d_ghost);
      plan->exchange_fn(plan->comm_ctx, 1, x->d_trace, x->d_ghost);
      gt = x->d_ghost;
    }
    for (const Bucket& bk : plan->buckets) {
      if (bk.n_elem == 0) continue;
      const size_t lds = gradient_lds_bytes(bk.N, bk.NQ);
      if (lds > kElemL2MaxLds) D4EST_HIP_ABORT("ip_energy_norm_sqr: (deg, deg_quad) = (%d, %d) needs %zu bytes of LDS", bk.deg, bk.deg_quad, lds);
      if (lds > 64 * 1024) set_lds_limit(norms_gradient_kernel, kElemL2MaxLds);
      hipLaunchKernelGGL(norms_gradient_kernel, dim3(std::min(bk.n_elem, 16384)), dim3(256), lds, plan->stream, v, plan->d_metric,
                         plan->d_elem_ids + bk.elem_offset, plan->d_ns_list + bk.elem_offset, plan->d_qs_list + bk.elem_offset, bk.n_elem, bk.d_B,
                         bk.d_D, bk.N, bk.NQ, t);
      HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(norms_face_kernel, dim3(std::min(ne, 65536)), dim3(64), 0, plan->stream, x->d_trace, gt, x->d_mortars, x->d_elem_first,
                       x->d_fac, ne, t);
    HIP_CHECK(hipGetLastError());
  }
  // volume, boundary, interface and total = (volume + boundary) + interface (d4est_ip_energy_norm.c:440-443)
  launch_reduce(plan, t, nullptr, 3, 0, 1, sums);
}

}  // namespace d4est_hip
