// The one-kernel "V u -> pointwise at the quadrature nodes -> V^T W J" body, templated on the pointwise function, and the pointwise
// functions of the two power forms.  Shared by d4est_hip_nonlinear.hip (the integer and the real power term, their linearisation) and
// d4est_hip_problem.hip (the load vector of a field id: no forward half, the pointwise function is map + field).
//
// A pointwise function F is a trivially copyable struct (it travels in the kernel argument segment) with
//   static constexpr bool kForward   the body interpolates u first (false: the function does not read u, `u` may be null)
//   int beta                         term form: 0 overwrite, 1 accumulate
//   double term(ei, q, a, b, kq, u)  f at the quadrature node q = qs + a + NQ (b + NQ kq) of entry ei of the launch's element
//                                    lists, u = (V u)(q).  q is an int here and a long long in the composed path's flat kernel
//   double coeff(ei, q, a, b, kq, u) df/du there (the coefficient form)
#pragma once

#include "d4est_hip_internal.h"
#include "d4est_hip_wave.h"
#include "d4est_hip_mwave.h"

namespace d4est_hip {

// base^k by repeated multiplication (the reference's callbacks multiply out; no pow)
__device__ __forceinline__ double pow_int(double base, int k) {
  const int m = k < 0 ? -k : k;
  double p = 1.0;
  for (int i = 0; i < m; ++i) p *= base;
  return k < 0 ? 1.0 / p : p;
}
__device__ __forceinline__ double power_term(double a, double b, double u, int k) { return a * pow_int(b + u, k); }
// d/du of the above: k a (b + u)^(k-1); k = 0: exactly 0 (not 0 * (b + u)^-1)
__device__ __forceinline__ double power_coeff(double a, double b, double u, int k) {
  return k == 0 ? 0.0 : ((double)k * a) * pow_int(b + u, k - 1);
}

// f = a (b + u)^k, integer k
struct PowArgs {
  static constexpr bool kForward = true;
  const double* a;
  const double* b;   // may be null
  int k;
  int beta;
  template <class I>
  __device__ __forceinline__ double term(int, I q, int, int, int, double u) const { return power_term(a[q], b ? b[q] : 0.0, u, k); }
  template <class I>
  __device__ __forceinline__ double coeff(int, I q, int, int, int, double u) const { return power_coeff(a[q], b ? b[q] : 0.0, u, k); }
};

// f = a |b + u|^s, real s, evaluated the way the reference's callbacks are written (src/Problems/Okendon/okendon_fcns.h:114-145):
// pow(t t, s / 2) and s / pow(t t, (1 - s) / 2), t = b + u.  Nothing is clamped at t = 0: the IEEE result stands
struct AbsPowArgs {
  static constexpr bool kForward = true;
  const double* a;
  const double* b;   // may be null
  double s;
  int beta;
  template <class I>
  __device__ __forceinline__ double term(int, I q, int, int, int, double u) const {
    const double t = (b ? b[q] : 0.0) + u;
    return a[q] * pow(t * t, .5 * s);
  }
  template <class I>
  __device__ __forceinline__ double coeff(int, I q, int, int, int, double u) const {
    const double t = (b ? b[q] : 0.0) + u;
    return (s * a[q]) / pow(t * t, .5 * (1. - s));
  }
};

// dst += the LDS image (store_element_image of d4est_hip_wave.h with the reference's axpy 1.0)
template <int N, int PL, int PN>
__device__ __forceinline__ void add_element_image(double* __restrict__ dst, const double* R, int te) {
  constexpr int N3 = N * N * N, NL = (N3 + PL - 1) / PL;
#pragma unroll
  for (int q = 0; q < NL; ++q) {
    const int idx = te + PL * q;
    const int i = idx % N, j = (idx / N) % N, k = idx / (N * N);
    if (N3 % PL == 0 || idx < N3) dst[idx] = dst[idx] + R[i + PN * (j + N * k)];
  }
}

// Bop / BopT: the even-odd tables of B^T / B (Bucket::d_EBb / d_EBf), as mass_like_body takes them with EO = true
template <int N, int NQ, bool COEFF, class F>
__device__ __forceinline__ void nonlin_body(double* smem, int wg, const double* __restrict__ u, double* __restrict__ out,
                                            const double* __restrict__ Jq, const int* __restrict__ ns_list,
                                            const int* __restrict__ qs_list, int n_bucket, const double* __restrict__ Bop,
                                            const double* __restrict__ BopT, const double* __restrict__ wq, F P,
                                            double* __restrict__ c_out, double* __restrict__ wjc_out) {
  using C = WaveCfg<N, NQ>;
  constexpr int PL = C::PL, PN = C::PN, PQ = C::PQ;

  const int tid = threadIdx.x;
  const int slot = tid / PL;
  const int te = tid - slot * PL;
  const int a = te % NQ, b = te / NQ;
  const int ei = wg * C::EPB + slot;
  const bool active = (slot < C::EPB) && (ei < n_bucket);
  double* R0 = smem + (active ? slot : 0) * C::LDS_PER_ELEM;
  double* R1 = R0 + C::FS;

  int ns = 0, qs = 0;
  if (active) {
    ns = ns_list[ei];
    qs = qs_list[ei];
  }

  // ---- forward: g = (V u)(a, b, :) ----
  double g[NQ];
  if constexpr (F::kForward) {
    if (active) load_element_image<N, PL, PN>(R0, u + ns, te);
    __syncthreads();
    if (active && a < N && b < N) {  // r
      double x[N], y[NQ];
#pragma unroll
      for (int i = 0; i < N; ++i) x[i] = lds_ld(&R0[i + PN * (a + N * b)]);
      fwd<N, NQ, true, false>(BopT, x, y);
#pragma unroll
      for (int iq = 0; iq < NQ; ++iq) R1[a + PN * (iq + NQ * b)] = y[iq];
    }
    __syncthreads();
    if (active && b < N) {  // s
      double x[N], y[NQ];
#pragma unroll
      for (int j = 0; j < N; ++j) x[j] = lds_ld(&R1[j + PN * (a + NQ * b)]);
      fwd<N, NQ, true, false>(BopT, x, y);
#pragma unroll
      for (int jq = 0; jq < NQ; ++jq) R0[b + PN * (a + NQ * jq)] = y[jq];
    }
    __syncthreads();
    if (active) {  // t
      double x[N];
#pragma unroll
      for (int k = 0; k < N; ++k) x[k] = lds_ld(&R0[k + PN * (a + NQ * b)]);
      fwd<N, NQ, true, false>(BopT, x, g);
    }
  } else if (active) {
    // no forward half: f does not read u.  Such a function is large (a map and a field), so it is evaluated in a ROLLED loop and parked
    // in the thread's own NQ slots of the LDS image, which nothing else uses before the backward half
#pragma unroll 1
    for (int kq = 0; kq < NQ; ++kq) R0[te + PL * kq] = P.term(ei, qs + a + NQ * (b + NQ * kq), a, b, kq, 0.0);
#pragma unroll
    for (int kq = 0; kq < NQ; ++kq) g[kq] = R0[te + PL * kq];
  }

  // ---- pointwise, at the thread's NQ quadrature nodes ----
  if constexpr (COEFF) {
    if (active) {
      const double wab = wq[b] * wq[a];
#pragma unroll
      for (int kq = 0; kq < NQ; ++kq) {
        const int q = qs + a + NQ * (b + NQ * kq);
        const double c = P.coeff(ei, q, a, b, kq, g[kq]);
        c_out[q] = c;
        wjc_out[q] = (wq[kq] * wab) * (Jq[q] * c);   // the rounding of lhs_wjc_kernel (d4est_hip_solver.hip)
      }
    }
    return;
  } else {
    double c[N];
    if (active) {
      const double wab = wq[a] * wq[b];
#pragma unroll
      for (int kq = 0; kq < NQ; ++kq) {
        const int q = qs + a + NQ * (b + NQ * kq);
        const double sc = (wq[kq] * wab) * Jq[q];
        if constexpr (F::kForward) g[kq] = P.term(ei, q, a, b, kq, g[kq]) * sc;
        else g[kq] *= sc;
      }
      bwd<NQ, N, true, false, false>(Bop, g, c);
    }
    // ---- backward: V^T, as mass_like_body ----
    __syncthreads();
    if (active) {
#pragma unroll
      for (int k = 0; k < N; ++k) R0[b + PQ * (a + NQ * k)] = c[k];
    }
    __syncthreads();
    if (active && b < N) {
      double x[NQ], y[N];
#pragma unroll
      for (int jq = 0; jq < NQ; ++jq) x[jq] = lds_ld(&R0[jq + PQ * (a + NQ * b)]);
      bwd<NQ, N, true, false, false>(Bop, x, y);
#pragma unroll
      for (int j = 0; j < N; ++j) R1[a + PQ * (j + N * b)] = y[j];
    }
    __syncthreads();
    if (active && a < N && b < N) {
      double x[NQ], o[N];
#pragma unroll
      for (int iq = 0; iq < NQ; ++iq) x[iq] = lds_ld(&R1[iq + PQ * (a + N * b)]);
      bwd<NQ, N, true, false, false>(Bop, x, o);
#pragma unroll
      for (int i = 0; i < N; ++i) R0[i + PN * (a + N * b)] = o[i];
    }
    __syncthreads();
    if (active) {
      if (P.beta) add_element_image<N, PL, PN>(out + ns, R0, te);
      else store_element_image<N, PL, PN>(out + ns, R0, te);
    }
  }
}

template <int N, int NQ, bool COEFF, class F>
__global__ __launch_bounds__((WaveCfg<N, NQ>::THREADS)) void nonlin_kernel(
    const double* __restrict__ u, double* __restrict__ out, const double* __restrict__ Jq, const int* __restrict__ ns_list,
    const int* __restrict__ qs_list, int n_bucket, const double* __restrict__ Bop, const double* __restrict__ BopT,
    const double* __restrict__ wq, F P, double* __restrict__ c_out, double* __restrict__ wjc_out) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  nonlin_body<N, NQ, COEFF, F>(smem, blockIdx.x, u, out, Jq, ns_list, qs_list, n_bucket, Bop, BopT, wq, P, c_out, wjc_out);
}

// every bucket has a compiled (deg + 1, deg_quad + 1) pair (pair_built, d4est_hip_wave.h: the pairs for which
// d4est_hip_apply_galerkin_integral launches a compiled kernel, d4est_hip_volume.hip): the ONE condition under which the nonlinear term,
// its linearisation and the load vector by id take their one-kernel form
inline bool plan_pairs_built(const d4est_hip_plan* plan) {
  for (const Bucket& bk : plan->buckets)
    if (bk.n_elem > 0 && !pair_built(bk.N, bk.NQ)) return false;
  return true;
}

}  // namespace d4est_hip
