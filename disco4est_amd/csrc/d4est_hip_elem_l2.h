// v_e^T M_e v_e = sum_q w J (V v_e)^2 of one element at its deg_quad (d4est_mesh_compute_l2_norm_sqr, src/Mesh/d4est_mesh.c:2299-2374):
// the body shared by the estimator's residual term (d4est_hip_estimator.hip) and the L2 norm (d4est_hip_norms.hip).  One 256-thread
// workgroup per element; three tensor passes in LDS, then a fixed tree reduction (the same value on every call).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

namespace d4est_hip {

// dynamic LDS of a kernel built on elem_l2_sqr for one (N, NQ): X, Y, the interpolation matrix, the weights, the reduction buffer
inline size_t elem_l2_lds_bytes(int N, int NQ) {
  return (size_t)(std::max(N * N * N, NQ * NQ * N) + NQ * N * N + NQ * N + NQ + 256) * sizeof(double);
}
constexpr size_t kElemL2MaxLds = 160 * 1024;   // gfx950: 160 KB of LDS per workgroup

struct ElemL2Lds {
  double *X, *Y, *Bs, *ws, *red;
};

// carve the workgroup's dynamic LDS and load the bucket's tables (no barrier: elem_l2_sqr's first one covers it)
__device__ inline ElemL2Lds elem_l2_lds(double* smem, const double* __restrict__ B, const double* __restrict__ w, int N, int NQ) {
  const int N3 = N * N * N, xs = (N3 > NQ * NQ * N) ? N3 : NQ * NQ * N, ys = NQ * N * N;
  ElemL2Lds s;
  s.X = smem;           // v_e, then the (a, b, k) partial
  s.Y = s.X + xs;       // the (a, j, k) partial
  s.Bs = s.Y + ys;      // NQ x N
  s.ws = s.Bs + NQ * N;
  s.red = s.ws + NQ;    // 256
  for (int i = threadIdx.x; i < NQ * N; i += blockDim.x) s.Bs[i] = B[i];
  for (int i = threadIdx.x; i < NQ; i += blockDim.x) s.ws[i] = w[i];
  return s;
}

// the sum, valid on thread 0 (every thread of the 256 calls; the caller puts a barrier before the next element's call)
__device__ inline double elem_l2_sqr(const ElemL2Lds& s, const double* __restrict__ v, const double* __restrict__ Jq, int N, int NQ) {
  double *X = s.X, *Y = s.Y, *red = s.red;
  const double *Bs = s.Bs, *ws = s.ws;
  const int N3 = N * N * N;
  for (int i = threadIdx.x; i < N3; i += blockDim.x) X[i] = v[i];
  __syncthreads();
  for (int idx = threadIdx.x; idx < NQ * N * N; idx += blockDim.x) {   // x: Y(a, j, k) = sum_i B(a, i) X(i, j, k)
    const int a = idx % NQ, jk = idx / NQ;
    double t = 0.0;
    for (int i = 0; i < N; ++i) t = fma(Bs[a * N + i], X[i + N * jk], t);
    Y[idx] = t;
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < NQ * NQ * N; idx += blockDim.x) {  // y: X(a, b, k) = sum_j B(b, j) Y(a, j, k)
    const int a = idx % NQ, b = (idx / NQ) % NQ, k = idx / (NQ * NQ);
    double t = 0.0;
    for (int j = 0; j < N; ++j) t = fma(Bs[b * N + j], Y[a + NQ * (j + N * k)], t);
    X[idx] = t;
  }
  __syncthreads();
  double acc = 0.0;
  for (int idx = threadIdx.x; idx < NQ * NQ * NQ; idx += blockDim.x) {  // z, then w J v^2
    const int ab = idx % (NQ * NQ), c = idx / (NQ * NQ);
    double t = 0.0;
    for (int k = 0; k < N; ++k) t = fma(Bs[c * N + k], X[ab + NQ * NQ * k], t);
    acc += ws[ab % NQ] * ws[ab / NQ] * ws[c] * Jq[idx] * t * t;
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
    __syncthreads();
  }
  return red[0];
}

}  // namespace d4est_hip
