// Face (mortar) part of the weak Laplacian: SIPG flux on conforming mortars and Dirichlet boundaries.
//
// Replaces, for all local (element, face) sides at once,
//   d4est_laplacian_compute_dudr              (src/dGMath/d4est_laplacian.c:237-282)  -> only face TRACES are formed
//   d4est_laplacian_flux_interface/_boundary  (src/dGMath/d4est_laplacian_flux.c:232-1014, :23-230)
//   d4est_laplacian_flux_sipg_interface/_dirichlet (src/dGMath/d4est_laplacian_flux_sipg.c:494-942, :15-336)
//   d4est_mortars_compute_flux_on_local_elements   (src/Mesh/d4est_mortars.c:601-840; the serial p4est_iterate walk)
//
// Design: element-centric and two-phase.
//  (1) trace kernel: every element writes, for each of its six sides, the traces of u and of du/dr_{0,1,2}
//      ALREADY INTERPOLATED to the side's mortar quadrature nodes (4 T doubles per side, T = (deg_mortar_quad+1)^2).
//      The reference interpolates every side twice per apply -- once as the (-) side of its own flux call and once as
//      the (+) side of the neighbour's -- here it happens once, and the mortar-node trace is also the only thing a
//      neighbouring GPU needs (instead of the reference's whole ghost elements).
//  (2) flux kernel: one workgroup per element walks its six sides, reads its own and the neighbour's mortar-node
//      traces (the neighbour's re-ordered by the p4est flip/transpose code), evaluates the three SIPG terms,
//      integrates and projects back (one tensor apply), scatters the four lifted fields into LDS volume fields and
//      applies  W_0 + sum_l D_l^T W_l  into Au_e once: race-free and deterministic, no atomics.
// The reference's 24 doubles of mortar geometry per quadrature node are pre-combined at set-up into 7:
//   am_i = sum_d sj n_d (dr_i/dx_d)^-,  ap_i = sum_d sj n_d (dr_i/dx_d)^+ (re-ordered to the (-) side),  s3 = sj sigma.
//
// This unit holds the trace / flux kernels and their launchers.  The descriptor structs the kernels read and FaceHost, the set-up's
// findings per plan, are in d4est_hip_faces_host.h; d4est_hip_faces_setup.hip builds them, d4est_hip_faces_geometry.hip fills the
// geometric factors and the boundary data.
#include <algorithm>

#include "d4est_hip_faces_host.h"
#include "d4est_hip_maps.h"
#include "d4est_hip_penalty.h"
#include "d4est_hip_wave.h"

namespace d4est_hip {

// value c (0: u, 1..3: du/dr_{c-1}) at face node (a,b) of face f from the element values ue (N^3, x fastest)
__device__ inline double nodal_trace(const double* ue, const double* D /* row-major, leading dim ldD */, int ldD, int N, int f,
                                     int a, int b, int c) {
  const int v = face_vol_index(f, N, a, b);
  if (c == 0) return ue[v];
  const int d = c - 1;
  const int stride = (d == 0) ? 1 : (d == 1 ? N : N * N);
  const int pos = (v / stride) % N;
  const int base = v - pos * stride;
  double val = 0.0;
  for (int i = 0; i < N; ++i) val = fma(D[pos * ldD + i], ue[base + i * stride], val);
  return val;
}

// ---------------------------------------------------------------------------
// generic tensor apply (runtime sizes, whole workgroup): out (rows x rows) = (op (x) op) in (cols x cols)
// ---------------------------------------------------------------------------
__device__ inline void apply2d(const double* __restrict__ op, int rows, int cols, const double* in, double* tmp, double* out,
                               int nfields, int in_stride, int out_stride, int tmp_stride) {
  for (int idx = threadIdx.x; idx < nfields * rows * cols; idx += blockDim.x) {
    const int fld = idx / (rows * cols), r = idx % (rows * cols), ap = r % rows, b = r / rows;
    const double* x = in + fld * in_stride + cols * b;
    double s = 0.0;
    for (int a = 0; a < cols; ++a) s = fma(op[ap * cols + a], x[a], s);
    tmp[fld * tmp_stride + ap + rows * b] = s;
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < nfields * rows * rows; idx += blockDim.x) {
    const int fld = idx / (rows * rows), r = idx % (rows * rows), ap = r % rows, bp = r / rows;
    const double* x = tmp + fld * tmp_stride + ap;
    double s = 0.0;
    for (int b = 0; b < cols; ++b) s = fma(op[bp * cols + b], x[rows * b], s);
    out[fld * out_stride + ap + rows * bp] = s;
  }
  __syncthreads();
}

// ---------------------------------------------------------------------------
// (1) generic trace kernel: any degree, one 256-thread workgroup per element
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void trace_generic_kernel(const double* __restrict__ u, double* __restrict__ qtrace,
                                                            const SideDesc* __restrict__ sd, const ElemDesc* __restrict__ ed,
                                                            const double* __restrict__ face_ops, int n_elem, int fld_stride) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* A = smem;                     // 4 nodal fields
  double* tmp = A + 4 * fld_stride;
  double* Q = tmp + 4 * fld_stride;     // 4 fields at the mortar nodes
  double* ue = Q + 4 * fld_stride;
  for (int e = blockIdx.x; e < n_elem; e += gridDim.x) {
    const ElemDesc el = ed[e];
    const int N = el.N, N2 = N * N, N3 = N2 * N;
    double* Ds = ue + N3;
    for (int i = threadIdx.x; i < N3; i += blockDim.x) ue[i] = u[el.ns + i];
    for (int i = threadIdx.x; i < N2; i += blockDim.x) Ds[i] = face_ops[el.offD + i];
    __syncthreads();
    for (int f = 0; f < 6; ++f) {
      const SideDesc d = sd[6 * e + f];
      const int NQ = d.NQ, T = NQ * NQ;
      for (int idx = threadIdx.x; idx < 4 * N2; idx += blockDim.x) {
        const int c = idx / N2, ab = idx % N2;
        A[c * fld_stride + ab] = nodal_trace(ue, Ds, N, N, f, ab % N, ab / N, c);
      }
      __syncthreads();
      apply2d(face_ops + d.offC, NQ, N, A, tmp, Q, 4, fld_stride, fld_stride, fld_stride);
      for (int idx = threadIdx.x; idx < 4 * T; idx += blockDim.x) qtrace[d.qoff + idx] = Q[(idx / T) * fld_stride + idx % T];
      __syncthreads();
    }
  }
}

// ghost sides: the same for face f of a ghost element given as a whole element (reference-style ghost data)
__global__ __launch_bounds__(256) void ghost_trace_kernel(const double* __restrict__ u_ghost, double* __restrict__ ghost_qtrace,
                                                          const GhostSideDesc* __restrict__ gd, const double* __restrict__ face_ops,
                                                          int n_ghost_sides, int fld_stride) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* A = smem;
  double* tmp = A + 4 * fld_stride;
  double* Q = tmp + 4 * fld_stride;
  double* ue = Q + 4 * fld_stride;
  for (int s = blockIdx.x; s < n_ghost_sides; s += gridDim.x) {
    const GhostSideDesc g = gd[s];
    const int N = g.N, N2 = N * N, N3 = N2 * N, T = g.NQ * g.NQ;
    double* Ds = ue + N3;
    for (int i = threadIdx.x; i < N3; i += blockDim.x) ue[i] = u_ghost[g.u_off + i];
    for (int i = threadIdx.x; i < N2; i += blockDim.x) Ds[i] = face_ops[g.offD + i];
    __syncthreads();
    for (int idx = threadIdx.x; idx < 4 * N2; idx += blockDim.x) {
      const int c = idx / N2, ab = idx % N2;
      A[c * fld_stride + ab] = nodal_trace(ue, Ds, N, N, g.f, ab % N, ab / N, c);
    }
    __syncthreads();
    apply2d(face_ops + g.offC, g.NQ, N, A, tmp, Q, 4, fld_stride, fld_stride, fld_stride);
    for (int idx = threadIdx.x; idx < 4 * T; idx += blockDim.x) ghost_qtrace[g.goff + idx] = Q[(idx / T) * fld_stride + idx % T];
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// (2) generic flux kernel: any degree, one 256-thread workgroup per element, sides in sequence
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void flux_generic_kernel(const double* __restrict__ qtrace, const double* __restrict__ ghost_qtrace,
                                                           double* __restrict__ Au, const SideDesc* __restrict__ sd,
                                                           const ElemDesc* __restrict__ ed, const double* __restrict__ face_ops,
                                                           const double* __restrict__ geom, const double* __restrict__ bndry_q,
                                                           const double* __restrict__ robin_c, const double* __restrict__ robin_r,
                                                           int n_elem, int fld_stride) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* A = smem;                     // 4 term fields at the mortar nodes
  double* tmp = A + 4 * fld_stride;
  double* R = tmp + 4 * fld_stride;     // 4 fields on the side's nodes
  double* acc = R + 4 * fld_stride;
  for (int e = blockIdx.x; e < n_elem; e += gridDim.x) {
    const ElemDesc el = ed[e];
    const int N = el.N, N2 = N * N, N3 = N2 * N;
    double* Ds = acc + N3;
    for (int i = threadIdx.x; i < N3; i += blockDim.x) acc[i] = 0.0;
    for (int i = threadIdx.x; i < N2; i += blockDim.x) Ds[i] = face_ops[el.offD + i];
    __syncthreads();
    for (int f = 0; f < 6; ++f) {
      const SideDesc d = sd[6 * e + f];
      const int NQ = d.NQ, T = NQ * NQ;
      const double* g = geom + (size_t)7 * d.geom;
      const double* qm = qtrace + d.qoff;
      const double* qp = ((d.kind == 2) ? ghost_qtrace : qtrace) + d.nbr_qoff;
      for (int k = threadIdx.x; k < T; k += blockDim.x) {
        if (d.kind == 0 && robin_c) {
          // Robin boundary (d4est_laplacian_flux_sipg.c:339-489): only  sj (coeff u_m - rhs), integrated and lifted
          A[k] = robin_c[d.geom + k] * qm[k] - robin_r[d.geom + k];
          for (int l = 0; l < 3; ++l) A[(1 + l) * fld_stride + k] = 0.0;
          continue;
        }
        const int kp = (d.kind == 0) ? k : reorder_index(d.code, NQ - 1, k % NQ, k / NQ);
        const double um = qm[k];
        const double up = (d.kind == 0) ? bndry_q[d.geom + k] : qp[kp];
        double t1 = 0.0, am[3];
        for (int i = 0; i < 3; ++i) {
          am[i] = g[i * T + k];
          t1 += am[i] * qm[(1 + i) * T + k];
          if (d.kind != 0) t1 += g[(3 + i) * T + k] * qp[(1 + i) * T + kp];
        }
        const double jump = um - up;
        // interface: t1 = -1/2 sj n.(grad u_m + grad u_p), t2_l = -1/2 am_l [u]; boundary: t1 = -sj n.grad u_m, t2_l = -am_l (u - g)
        const double w1 = (d.kind != 0) ? -0.5 : -1.0;
        A[k] = w1 * t1 + g[6 * T + k] * jump;
        for (int l = 0; l < 3; ++l) A[(1 + l) * fld_stride + k] = w1 * am[l] * jump;
      }
      __syncthreads();
      apply2d(face_ops + d.offE, N, NQ, A, tmp, R, 4, fld_stride, fld_stride, fld_stride);
      // lift (+ D_l^T for the term-2 fields) into the element accumulator
      const int dir = f >> 1, fix = face_fix(f, N);
      const int sdir = (dir == 0) ? 1 : (dir == 1 ? N : N2);
      for (int idx = threadIdx.x; idx < N3; idx += blockDim.x) {
        const int pos = (idx / sdir) % N;
        int a, b;
        if (dir == 0) { a = (idx / N) % N; b = idx / N2; }
        else if (dir == 1) { a = idx % N; b = idx / N2; }
        else { a = idx % N; b = (idx / N) % N; }
        double v = Ds[fix * N + pos] * R[(1 + dir) * fld_stride + a + N * b];
        if (pos == fix) {
          v += R[a + N * b];
          const int t0 = (dir == 0) ? 1 : 0, t1d = (dir == 2) ? 1 : 2;  // tangential reference directions of a and b
          double s0 = 0.0, s1 = 0.0;
          for (int q = 0; q < N; ++q) {
            s0 = fma(Ds[q * N + a], R[(1 + t0) * fld_stride + q + N * b], s0);
            s1 = fma(Ds[q * N + b], R[(1 + t1d) * fld_stride + a + N * q], s1);
          }
          v += s0 + s1;
        }
        acc[idx] += v;
      }
      __syncthreads();
    }
    for (int i = threadIdx.x; i < N3; i += blockDim.x) Au[el.ns + i] += acc[i];
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// Non-conforming (hanging 1 <-> 4) meshes: mortar-record path.  Every side owns 1 record (conforming, boundary, or the
// hanging "small" side: faces_m = 4, faces_p = 1, seen from one of the four small elements) or 4 records (the "big" side:
// faces_m = 1, faces_p = 4).  A record's mortar-node trace block is produced by its own element with
//   conforming / small:  p-prolong + interpolation              (Mesh/d4est_mortars.c:556-566, d4est_laplacian_flux.c:659-694)
//   big, sub-mortar i:   hp-prolong child (i & 1, i >> 1) + interpolation   (Mesh/d4est_mortars.c:568-579)
// and consumed by the element itself and by the element across the mortar.  du/dr in a block is with respect to the
// producing element's own reference coordinates; the mortar's metric (given on the mortar-sized cell) is twice the big
// element's, hence the factors fm / fp = 1/2 on the big element's gradient and w2 = 1/2 on the big side's term 2
// (d4est_laplacian_flux.c:905-915, d4est_laplacian_flux_sipg.c:806-808).
// ---------------------------------------------------------------------------
// out (rows x rows) = (opb (x) opa) in (cols x cols): opa contracts the fast face index a, opb the slow index b
__device__ inline void apply2d_ab(const double* __restrict__ opa, const double* __restrict__ opb, int rows, int cols, const double* in,
                                  double* tmp, double* out, int nfields, int in_stride, int out_stride, int tmp_stride, bool accumulate) {
  for (int idx = threadIdx.x; idx < nfields * rows * cols; idx += blockDim.x) {
    const int fld = idx / (rows * cols), r = idx % (rows * cols), ap = r % rows, b = r / rows;
    const double* x = in + fld * in_stride + cols * b;
    double s = 0.0;
    for (int a = 0; a < cols; ++a) s = fma(opa[ap * cols + a], x[a], s);
    tmp[fld * tmp_stride + ap + rows * b] = s;
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < nfields * rows * rows; idx += blockDim.x) {
    const int fld = idx / (rows * rows), r = idx % (rows * rows), ap = r % rows, bp = r / rows;
    const double* x = tmp + fld * tmp_stride + ap;
    double s = 0.0;
    for (int b = 0; b < cols; ++b) s = fma(opb[bp * cols + b], x[rows * b], s);
    if (accumulate) out[fld * out_stride + ap + rows * bp] += s;
    else out[fld * out_stride + ap + rows * bp] = s;
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void trace_hp_kernel(const double* __restrict__ u, double* __restrict__ qtrace,
                                                       const HpMortar* __restrict__ md, const int* __restrict__ elem_first,
                                                       const ElemDesc* __restrict__ ed, const double* __restrict__ face_ops,
                                                       const double* __restrict__ hp_ops, int n_elem, int fld_stride) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* A = smem;                     // 4 nodal fields of the current side
  double* tmp = A + 4 * fld_stride;
  double* Q = tmp + 4 * fld_stride;     // 4 fields at the mortar nodes
  double* ue = Q + 4 * fld_stride;
  for (int e = blockIdx.x; e < n_elem; e += gridDim.x) {
    const ElemDesc el = ed[e];
    const int N = el.N, N2 = N * N, N3 = N2 * N;
    double* Ds = ue + N3;
    for (int i = threadIdx.x; i < N3; i += blockDim.x) ue[i] = u[el.ns + i];
    for (int i = threadIdx.x; i < N2; i += blockDim.x) Ds[i] = face_ops[el.offD + i];
    __syncthreads();
    for (int r = elem_first[e]; r < elem_first[e + 1]; ++r) {
      const HpMortar m = md[r];
      const int NQ = m.NQ, T = NQ * NQ;
      if (m.first) {
        for (int idx = threadIdx.x; idx < 4 * N2; idx += blockDim.x) {
          const int c = idx / N2, ab = idx % N2;
          A[c * fld_stride + ab] = nodal_trace(ue, Ds, N, N, m.face, ab % N, ab / N, c);
        }
        __syncthreads();
      }
      apply2d_ab(hp_ops + m.offCa, hp_ops + m.offCb, NQ, N, A, tmp, Q, 4, fld_stride, fld_stride, fld_stride, false);
      for (int idx = threadIdx.x; idx < 4 * T; idx += blockDim.x) qtrace[m.qoff + idx] = Q[(idx / T) * fld_stride + idx % T];
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(256) void flux_hp_kernel(const double* __restrict__ qtrace, const double* __restrict__ ghost_qtrace,
                                                      double* __restrict__ Au,
                                                      const HpMortar* __restrict__ md, const int* __restrict__ elem_first,
                                                      const ElemDesc* __restrict__ ed, const double* __restrict__ face_ops,
                                                      const double* __restrict__ hp_ops, const double* __restrict__ geom,
                                                      const double* __restrict__ bndry_q, const double* __restrict__ robin_c,
                                                      const double* __restrict__ robin_r, int n_elem, int fld_stride) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* A = smem;                     // 4 term fields at the mortar nodes
  double* tmp = A + 4 * fld_stride;
  double* R = tmp + 4 * fld_stride;     // 4 fields on the side's nodes, summed over the side's mortars
  double* acc = R + 4 * fld_stride;
  for (int e = blockIdx.x; e < n_elem; e += gridDim.x) {
    const ElemDesc el = ed[e];
    const int N = el.N, N2 = N * N, N3 = N2 * N;
    double* Ds = acc + N3;
    for (int i = threadIdx.x; i < N3; i += blockDim.x) acc[i] = 0.0;
    for (int i = threadIdx.x; i < N2; i += blockDim.x) Ds[i] = face_ops[el.offD + i];
    __syncthreads();
    for (int r = elem_first[e]; r < elem_first[e + 1]; ++r) {
      const HpMortar m = md[r];
      const int NQ = m.NQ, T = NQ * NQ, f = m.face;
      const double* g = geom + (size_t)7 * m.gidx;
      const double* qm = qtrace + m.qoff;
      const double* qp = ((m.kind == 2) ? ghost_qtrace : qtrace) + m.nbr_qoff;
      for (int k = threadIdx.x; k < T; k += blockDim.x) {
        if (m.kind == 0 && robin_c) {
          A[k] = robin_c[m.gidx + k] * qm[k] - robin_r[m.gidx + k];
          for (int l = 0; l < 3; ++l) A[(1 + l) * fld_stride + k] = 0.0;
          continue;
        }
        const int kp = (m.kind == 0) ? k : reorder_index(m.code, NQ - 1, k % NQ, k / NQ);
        const double um = qm[k];
        const double up = (m.kind == 0) ? bndry_q[m.gidx + k] : qp[kp + m.u_shift];
        double tm = 0.0, tp = 0.0, am[3];
        for (int i = 0; i < 3; ++i) {
          am[i] = g[i * T + k];
          tm += am[i] * qm[(1 + i) * T + k];
          if (m.kind != 0) tp += g[(3 + i) * T + k] * qp[(1 + i) * T + kp];
        }
        const double jump = um - up;
        const double w1 = (m.kind != 0) ? -0.5 : -1.0;
        A[k] = w1 * (tm + tp) + g[6 * T + k] * jump;   // (fm, fp, w2: folded into the factors by face_geom_hp_kernel)
        for (int l = 0; l < 3; ++l) A[(1 + l) * fld_stride + k] = w1 * am[l] * jump;
      }
      __syncthreads();
      apply2d_ab(hp_ops + m.offEa, hp_ops + m.offEb, N, NQ, A, tmp, R, 4, fld_stride, fld_stride, fld_stride, !m.first);
      if (!m.last) continue;
      const int dir = f >> 1, fix = face_fix(f, N);
      const int sdir = (dir == 0) ? 1 : (dir == 1 ? N : N2);
      for (int idx = threadIdx.x; idx < N3; idx += blockDim.x) {
        const int pos = (idx / sdir) % N;
        int a, b;
        if (dir == 0) { a = (idx / N) % N; b = idx / N2; }
        else if (dir == 1) { a = idx % N; b = idx / N2; }
        else { a = idx % N; b = (idx / N) % N; }
        double v = Ds[fix * N + pos] * R[(1 + dir) * fld_stride + a + N * b];
        if (pos == fix) {
          v += R[a + N * b];
          const int t0 = (dir == 0) ? 1 : 0, t1d = (dir == 2) ? 1 : 2;
          double s0 = 0.0, s1 = 0.0;
          for (int q = 0; q < N; ++q) {
            s0 = fma(Ds[q * N + a], R[(1 + t0) * fld_stride + q + N * b], s0);
            s1 = fma(Ds[q * N + b], R[(1 + t1d) * fld_stride + a + N * q], s1);
          }
          v += s0 + s1;
        }
        acc[idx] += v;
      }
      __syncthreads();
    }
    for (int i = threadIdx.x; i < N3; i += blockDim.x) Au[el.ns + i] += acc[i];
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// fast path (every N, Np, NQ <= 8, i.e. p <= 7): workgroup of six wavefronts per element, wavefront f <-> side f,
// lane <-> node of a fixed 8 x 8 grid (index a + 8 b).  Operators are zero-padded to 8 x 8 in LDS so the tensor
// applies are branch-free and fully unrolled (the padding multiplies zeros).
// ---------------------------------------------------------------------------
constexpr int kFW = 8;

// out_c(a',b') = sum_{a,b} op[a'][a] op[b'][b] in_c(a,b); lane = a' + 8 b'; result in registers
// the buffer handed to wave_apply2d belongs to the calling WAVE only (each wave of flux_wave_kernel owns s_in[f]), so its hand-offs
// through LDS need a wave-level fence, not a workgroup barrier
__device__ __forceinline__ void wave_private_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// two-buffer form of wave_apply2d (first pass in -> tmp): one wave-level fence less per pass than the in-place form
template <int NF>
__device__ __forceinline__ void wave_apply2d_tmp(const double* op /*[8][8] padded*/, const double* in /*[NF][64]*/,
                                                 double* tmp /*[NF][64]*/, int lane, double* out /*[NF]*/) {
  const int lo = lane & 7, hi = lane >> 3;
  double c[kFW];
#pragma unroll
  for (int a = 0; a < kFW; ++a) c[a] = op[lo * 8 + a];
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    double s = 0.0;
#pragma unroll
    for (int a = 0; a < kFW; ++a) s = fma(c[a], in[f * 64 + a + 8 * hi], s);
    tmp[f * 64 + lane] = s;
  }
  wave_private_lds_fence();
#pragma unroll
  for (int b = 0; b < kFW; ++b) c[b] = op[hi * 8 + b];
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    double s = 0.0;
#pragma unroll
    for (int b = 0; b < kFW; ++b) s = fma(c[b], tmp[f * 64 + lo + 8 * b], s);
    out[f] = s;
  }
  wave_private_lds_fence();
}

template <int NF>
__device__ __forceinline__ void wave_apply2d(const double* op /*[8][8] padded*/, double* buf /*[NF][64], overwritten*/, int lane,
                                             double* out /*[NF]*/) {
  // both passes work in place: a wave executes in lockstep, so every lane has its row / column in registers before the
  // (fenced) stores of the pass overwrite the buffer
  const int lo = lane & 7, hi = lane >> 3;
  double c[kFW], t[NF];
#pragma unroll
  for (int a = 0; a < kFW; ++a) c[a] = op[lo * 8 + a];
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    double s = 0.0;
#pragma unroll
    for (int a = 0; a < kFW; ++a) s = fma(c[a], buf[f * 64 + a + 8 * hi], s);
    t[f] = s;
  }
  wave_private_lds_fence();
#pragma unroll
  for (int f = 0; f < NF; ++f) buf[f * 64 + lane] = t[f];
  wave_private_lds_fence();
#pragma unroll
  for (int b = 0; b < kFW; ++b) c[b] = op[hi * 8 + b];
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    double s = 0.0;
#pragma unroll
    for (int b = 0; b < kFW; ++b) s = fma(c[b], buf[f * 64 + lo + 8 * b], s);
    out[f] = s;
  }
  wave_private_lds_fence();
}

__global__ __launch_bounds__(384, 6) void trace_wave_kernel(const double* __restrict__ u, double* __restrict__ qtrace,
                                                         const SideDesc* __restrict__ sd, const ElemDesc* __restrict__ ed,
                                                         const double* __restrict__ face_ops, int n_elem, TraceUniform uni) {
  // Per side only TWO nodal fields are formed -- the trace tr(a,b) of u and the normal derivative n(a,b) -- because the
  // tangential derivatives commute with the interpolation:  (C (x) C)(D_a tr) = ((C D) (x) C) tr.  Pass 1 contracts the
  // face index a with C and CD, pass 2 the index b: 56 FMAs and ~90 LDS reads per lane instead of 152 / 130.
  __shared__ double s_u[512];
  __shared__ double s_D[64];          // zero-padded 8 x 8
  __shared__ double s_in[6][2][64];   // tr, n
  __shared__ double s_tmp[6][3][64];  // C tr, CD tr, C n
  __shared__ double s_C[6][2][64];    // C, CD zero-padded 8 x 8
  const int f = threadIdx.x >> 6, lane = threadIdx.x & 63, lo = lane & 7, hi = lane >> 3;
  const int dir = f >> 1;
  const int t0 = (dir == 0) ? 1 : 0, t1d = (dir == 2) ? 1 : 2;  // reference directions of the face indices a and b
  int e = blockIdx.x;
  ElemDesc edn{};
  SideDesc dn{};
  auto uniform_desc = [&](int e_, ElemDesc& el_, SideDesc& d_) {
    el_.N = uni.N; el_.ns = uni.ns0 + e_ * uni.ns_stride; el_.offD = uni.offD;
    d_.NQ = uni.NQ; d_.offC = uni.offC; d_.offCD = uni.offCD; d_.qoff = uni.q0 + (long long)(6 * e_ + f) * uni.q_stride;
  };
  if (uni.N > 0) uniform_desc(e < n_elem ? e : 0, edn, dn);
  else {
    edn = ed[e < n_elem ? e : 0];
    dn = sd[6 * (e < n_elem ? e : 0) + f];
  }
  for (; e < n_elem; e += gridDim.x) {
    const ElemDesc el = edn;
    const SideDesc d = dn;
    {
      const int en = e + gridDim.x;
      if (en < n_elem) {
        if (uni.N > 0) uniform_desc(en, edn, dn);
        else {
          edn = ed[en];
          dn = sd[6 * en + f];
        }
      }
    }
    const int N = el.N, N2 = N * N, N3 = N2 * N, NQ = d.NQ, T = NQ * NQ;
    double uv0 = 0.0, uv1 = 0.0;
    if ((int)threadIdx.x < N3) uv0 = u[el.ns + threadIdx.x];
    if ((int)threadIdx.x + 384 < N3) uv1 = u[el.ns + threadIdx.x + 384];
    const bool opl = hi < NQ && lo < N;
    const double opc = opl ? face_ops[d.offC + hi * N + lo] : 0.0;
    const double opcd = opl ? face_ops[d.offCD + hi * N + lo] : 0.0;
    const double dval = (threadIdx.x < 64) ? face_ops[el.offD + threadIdx.x] : 0.0;
    if ((int)threadIdx.x < N3) s_u[threadIdx.x] = uv0;
    if ((int)threadIdx.x + 384 < N3) s_u[threadIdx.x + 384] = uv1;
    if (threadIdx.x < 64) s_D[threadIdx.x] = dval;
    s_C[f][0][lane] = opc;
    s_C[f][1][lane] = opcd;
    __syncthreads();
    // ---- nodal trace and normal derivative at lane (a = lo, b = hi)
    {
      const int sn = (dir == 0) ? 1 : (dir == 1 ? N : N2);
      const int sa = (dir == 0) ? N : 1, sb = (dir == 2) ? N : N2;
      const int fix = face_fix(f, N);
      double tr = 0.0, nd = 0.0;
      if (lo < N && hi < N) {
        const int base = lo * sa + hi * sb;
        tr = s_u[base + fix * sn];
#pragma unroll
        for (int i = 0; i < kFW; ++i) nd = fma(s_D[fix * 8 + i], s_u[base + (i < N ? i : N - 1) * sn], nd);  // padded D columns are 0
      }
      s_in[f][0][lane] = tr;
      s_in[f][1][lane] = nd;
    }
    __syncthreads();
    // ---- pass 1: lane (a' = lo, b = hi): contract the face index a
    {
      double c1[kFW], c2[kFW];
#pragma unroll
      for (int a = 0; a < kFW; ++a) { c1[a] = s_C[f][0][lo * 8 + a]; c2[a] = s_C[f][1][lo * 8 + a]; }
      double P = 0.0, R = 0.0, S = 0.0;
#pragma unroll
      for (int a = 0; a < kFW; ++a) {
        const double t = s_in[f][0][a + 8 * hi], n = s_in[f][1][a + 8 * hi];
        P = fma(c1[a], t, P);
        R = fma(c2[a], t, R);
        S = fma(c1[a], n, S);
      }
      s_tmp[f][0][lane] = P;
      s_tmp[f][1][lane] = R;
      s_tmp[f][2][lane] = S;
    }
    __syncthreads();
    // ---- pass 2: lane (a' = lo, b' = hi): contract the face index b
    {
      double c1[kFW], c2[kFW];
#pragma unroll
      for (int b = 0; b < kFW; ++b) { c1[b] = s_C[f][0][hi * 8 + b]; c2[b] = s_C[f][1][hi * 8 + b]; }
      double qu = 0.0, qtb = 0.0, qta = 0.0, qn = 0.0;
#pragma unroll
      for (int b = 0; b < kFW; ++b) {
        const double P = s_tmp[f][0][lo + 8 * b], R = s_tmp[f][1][lo + 8 * b], S = s_tmp[f][2][lo + 8 * b];
        qu = fma(c1[b], P, qu);
        qtb = fma(c2[b], P, qtb);
        qta = fma(c1[b], R, qta);
        qn = fma(c1[b], S, qn);
      }
      if (lo < NQ && hi < NQ) {
        double* out = qtrace + d.qoff + lo + NQ * hi;
        out[0] = qu;
        out[(1 + dir) * T] = qn;
        out[(1 + t0) * T] = qta;
        out[(1 + t1d) * T] = qtb;
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// MFMA form of the trace kernel.  The two interpolation passes of a face are 8 x 8 x 8 matrix products; on the vector ALU
// every lane re-reads its operator row and its data column from LDS (45 KB of LDS traffic per wave and element: the kernel was
// LDS-bound, tools/pmc_faces.sh).  v_mfma_f64_16x16x4 takes the stacked operator [C; CD] (16 x 8) as a 2-register operand that
// never leaves the lane, so per element a lane only moves its own few values through LDS to re-shape them into MFMA operands:
//   pass 1:  Y (16 x 16) = [C; CD] (16 x 8) . [tr | nd] (8 x 16)         rows 0-7: C.tr | C.nd,  rows 8-15: CD.tr | (unused)
//   pass 2:  Z1 = [C.tr; CD.tr] (16 x 8) . [C^T | CD^T] (8 x 16)          -> qu | qtb ;  qta | (unused)
//            Z2 = [C.nd; 0]     (16 x 8) . [C^T | CD^T]                    -> qn
// Operand layouts (cdna_hip_programming.md): A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15],
// C/D reg r: row (lane >> 4) + 4 r, col lane & 15.  [C^T | CD^T] as a B operand holds the same values as [C; CD] as an A operand.
// ---------------------------------------------------------------------------
typedef double mfma_d4 __attribute__((ext_vector_type(4)));


// one workgroup = 3 waves = the three reference directions of one element; wave `dir` serves the two faces 2 dir, 2 dir + 1,
// which share the same lines of u (trace = first / last entry, normal derivative = row 0 / row N-1 of D)
__global__ __launch_bounds__(192) void trace_mfma_kernel(const double* __restrict__ u, double* __restrict__ qtrace,
                                                         const SideDesc* __restrict__ sd, const ElemDesc* __restrict__ ed,
                                                         const double* __restrict__ face_ops, int n_elem,
                                                         const int* __restrict__ elist = nullptr) {
  // elist: the kernel works on the listed elements only (n_elem = length of the list): the elements with a ghost (+) side, whose traces
  // feed the exchange while the interior elements' operator kernel forms its traces from u itself (apply_operator)
  auto EL = [&](int i) { return elist ? elist[i] : i; };
  constexpr int LDM = 18;                 // padded row length of the 8 x 16 re-shaping buffer (<= 2-way bank conflicts)
  constexpr int UJ = 9, UK = 72;          // padded strides of the LDS copy of u: conflict-free face reads in all three directions
  constexpr int TPB = 192;
  __shared__ double s_u[8 * UK];
  __shared__ double s_x[3][2][8 * LDM];   // per wave and face: [a][(field, b)]
  // the direction is wave-uniform: with it in an SGPR the descriptor loads become scalar loads and cost no VGPRs
  const int dir = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63, lo = lane & 7, hi = lane >> 3;
  const int mi = lane & 15, mk = lane >> 4;   // MFMA operand coordinates of this lane
  const int t0 = (dir == 0) ? 1 : 0, t1d = (dir == 2) ? 1 : 2;
  int cur_off[2][2] = {{-1, -1}, {-1, -1}}, cur_offD = -1, cur_N = -1, cur_NQ[2] = {-1, -1};
  double opA[2][2] = {{0.0, 0.0}, {0.0, 0.0}}, drow[2][kFW];
#pragma unroll
  for (int i = 0; i < kFW; ++i) drow[0][i] = drow[1][i] = 0.0;
  // persistent loop, software-pipelined: descriptors two elements ahead, u (3 values per thread) one element ahead
  int e = blockIdx.x;
  const int e_first = e < n_elem ? EL(e) : (n_elem > 0 ? EL(0) : 0);
  ElemDesc el = ed[e_first];
  SideDesc d0 = sd[6 * e_first + 2 * dir], d1 = sd[6 * e_first + 2 * dir + 1];
  double uv[3] = {0.0, 0.0, 0.0};
  {
    const int n3 = el.N * el.N * el.N;
#pragma unroll
    for (int r = 0; r < 3; ++r)
      if (e < n_elem && (int)threadIdx.x + TPB * r < n3) uv[r] = u[el.ns + threadIdx.x + TPB * r];
  }
  ElemDesc edn = el;
  SideDesc dn0 = d0, dn1 = d1;
  if (e + (int)gridDim.x < n_elem) {
    const int e2 = EL(e + gridDim.x);
    edn = ed[e2];
    dn0 = sd[6 * e2 + 2 * dir];
    dn1 = sd[6 * e2 + 2 * dir + 1];
  }
  for (; e < n_elem; e += gridDim.x) {
    const int N = el.N, N2 = N * N, N3 = N2 * N;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int t = threadIdx.x + TPB * r;
      if (t < N3) s_u[(t % N) + UJ * ((t / N) % N) + UK * (t / N2)] = uv[r];
    }
    const ElemDesc el_next = edn;
    const SideDesc d0_next = dn0, d1_next = dn1;
    {
      const int en = e + gridDim.x;
      if (en < n_elem) {
        const int n3 = el_next.N * el_next.N * el_next.N;
#pragma unroll
        for (int r = 0; r < 3; ++r) uv[r] = ((int)threadIdx.x + TPB * r < n3) ? u[el_next.ns + threadIdx.x + TPB * r] : 0.0;
        const int en2 = en + gridDim.x;
        if (en2 < n_elem) {
          const int e2 = EL(en2);
          edn = ed[e2];
          dn0 = sd[6 * e2 + 2 * dir];
          dn1 = sd[6 * e2 + 2 * dir + 1];
        }
      }
    }
    // operator registers: reloaded only when the side's operators change (wave-uniform test)
#pragma unroll
    for (int s_ = 0; s_ < 2; ++s_) {
      const SideDesc& d = s_ ? d1 : d0;
      if (d.offC != cur_off[s_][0] || d.offCD != cur_off[s_][1] || N != cur_N || d.NQ != cur_NQ[s_]) {
        const int row = mi & 7, off = (mi < 8) ? d.offC : d.offCD;
        opA[s_][0] = (row < d.NQ && mk < N) ? face_ops[off + row * N + mk] : 0.0;
        opA[s_][1] = (row < d.NQ && mk + 4 < N) ? face_ops[off + row * N + mk + 4] : 0.0;
        cur_off[s_][0] = d.offC; cur_off[s_][1] = d.offCD; cur_NQ[s_] = d.NQ;
      }
    }
    if (el.offD != cur_offD || N != cur_N) {
#pragma unroll
      for (int i = 0; i < kFW; ++i) {
        drow[0][i] = face_ops[el.offD + i];                 // zero-padded 8 x 8 image: row 0 and row N-1
        drow[1][i] = face_ops[el.offD + (N - 1) * 8 + i];
      }
      cur_offD = el.offD;
    }
    cur_N = N;
    __syncthreads();
    // ---- nodal traces and normal derivatives of both faces at lane (a = lo, b = hi): one pass over the line of u
    {
      const int sn = (dir == 0) ? 1 : (dir == 1 ? UJ : UK);
      const int sa = (dir == 0) ? UJ : 1, sb = (dir == 2) ? UJ : UK;
      double tr0 = 0.0, nd0 = 0.0, tr1 = 0.0, nd1 = 0.0;
      if (lo < N && hi < N) {
        const int base = lo * sa + hi * sb;
#pragma unroll
        for (int i = 0; i < kFW; ++i) {
          const double ui = s_u[base + (i < N ? i : N - 1) * sn];   // padded D columns are 0
          if (i == 0) tr0 = ui;
          if (i == N - 1) tr1 = ui;
          nd0 = fma(drow[0][i], ui, nd0);
          nd1 = fma(drow[1][i], ui, nd1);
        }
      }
      s_x[dir][0][lo * LDM + hi] = tr0;        // row k = a, column j = b
      s_x[dir][0][lo * LDM + 8 + hi] = nd0;    // column j = 8 + b
      s_x[dir][1][lo * LDM + hi] = tr1;
      s_x[dir][1][lo * LDM + 8 + hi] = nd1;
    }
    wave_lds_fence();
#pragma unroll
    for (int s_ = 0; s_ < 2; ++s_) {
      const SideDesc& d = s_ ? d1 : d0;
      const int NQ = d.NQ, T = NQ * NQ;
      const double* sx = s_x[dir][s_];
      // ---- pass 1, transposed:  Y^T (16 x 16) = [tr | nd]^T (16 x 8) . [C^T | CD^T] (8 x 16)
      //      rows (field, b), columns (operator, a'); the operator B operand holds the same values as the A operand [C; CD]
      mfma_d4 y = {0.0, 0.0, 0.0, 0.0};
      {
        const double a0 = sx[mk * LDM + mi], a1 = sx[(mk + 4) * LDM + mi];   // A[i = (field, b)][k = a]
        y = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, opA[s_][0], y, 0, 0, 0);
        y = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, opA[s_][1], y, 0, 0, 0);
      }
      // ---- pass 2:  Z = [C; CD] (16 x 8, along b) . Y^T rows.  The C/D registers of pass 1 ARE the B operands of pass 2:
      //      reg r holds row (lane >> 4) + 4 r = (field r >> 1, b = (lane >> 4) + 4 (r & 1)), i.e. k-step r & 1 of field r >> 1
      mfma_d4 z1 = {0.0, 0.0, 0.0, 0.0}, z2 = {0.0, 0.0, 0.0, 0.0};
      z1 = __builtin_amdgcn_mfma_f64_16x16x4f64(opA[s_][0], y[0], z1, 0, 0, 0);
      z1 = __builtin_amdgcn_mfma_f64_16x16x4f64(opA[s_][1], y[1], z1, 0, 0, 0);
      z2 = __builtin_amdgcn_mfma_f64_16x16x4f64(opA[s_][0], y[2], z2, 0, 0, 0);
      z2 = __builtin_amdgcn_mfma_f64_16x16x4f64(opA[s_][1], y[3], z2, 0, 0, 0);
      // ---- store: column lane & 15 = (operator along a, a'), reg r: row (lane >> 4) + 4 r = (operator along b, b')
      //      z1 rows C:  cols C -> qu, cols CD -> qta;  z1 rows CD: cols C -> qtb;  z2 rows C, cols C -> qn
      double* out = qtrace + d.qoff;
      const int aq = mi & 7;
      if (aq < NQ) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const int bq = mk + 4 * r;
          if (bq < NQ) {
            out[((mi < 8) ? 0 : (1 + t0) * T) + aq + NQ * bq] = z1[r];
            if (mi < 8) {
              out[(1 + t1d) * T + aq + NQ * bq] = z1[2 + r];
              out[(1 + dir) * T + aq + NQ * bq] = z2[r];
            }
          }
        }
      }
    }
    __syncthreads();
    el = el_next; d0 = d0_next; d1 = d1_next;
  }
}

// The same kernel for 8 < N or NQ <= 16 (p = 8 .. 15): every 16 x 16 operand block is one MFMA tile, the contraction length
// N <= 16 is 4 k-steps.  Per face: pass 1 = 3 tiles (tr.C^T, tr.CD^T, nd.C^T) x 4 k-steps, pass 2 = 4 tiles (qu, qta, qtb, qn) x
// 4 k-steps = 28 MFMAs, all useful at N = 16.  Replaces the generic trace kernel, whose per-node LDS dot products made the
// face path five times more expensive than the volume kernel at p >= 9.
__global__ __launch_bounds__(192) void trace_mfma16_kernel(const double* __restrict__ u, double* __restrict__ qtrace,
                                                           const SideDesc* __restrict__ sd, const ElemDesc* __restrict__ ed,
                                                           const double* __restrict__ face_ops, int n_elem, int max_n,
                                                           const int* __restrict__ elist = nullptr) {
  constexpr int LDM = 34;                  // staging rows: 32 columns (field, b) + padding
  constexpr int UJ = 17, UK = 272;         // padded strides of the LDS copy of u (<= 2-way bank conflicts in all directions)
  constexpr int TPB = 192;
  extern __shared__ __attribute__((aligned(16))) double smem16[];
  double* s_u = smem16;                    // max_n * UK (only the k-planes the plan's largest element needs)
  const int dir = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  double* stage = smem16 + max_n * UK + dir * (2 * 16 * LDM);   // per wave: 2 faces x [a (16)][(field, b) 32]
  const int lane = threadIdx.x & 63;
  const int mi = lane & 15, mk = lane >> 4;
  const int t0 = (dir == 0) ? 1 : 0, t1d = (dir == 2) ? 1 : 2;
  int cur_off[2][2] = {{-1, -1}, {-1, -1}}, cur_offD = -1, cur_N = -1, cur_NQ[2] = {-1, -1};
  double op[2][2][4];   // [face][C / CD][k-step]: OP[row mi][col 4 ks + mk], zero-padded
  double drow[2][16];
#pragma unroll
  for (int i = 0; i < 16; ++i) drow[0][i] = drow[1][i] = 0.0;
#pragma unroll
  for (int a_ = 0; a_ < 2; ++a_)
#pragma unroll
    for (int b_ = 0; b_ < 2; ++b_)
#pragma unroll
      for (int c_ = 0; c_ < 4; ++c_) op[a_][b_][c_] = 0.0;
  // the staging rows / columns beyond N are never written again: zero them once (they meet zero operator entries, but LDS
  // garbage could be NaN)
  for (int i = lane; i < 2 * 16 * LDM; i += 64) stage[i] = 0.0;
  wave_lds_fence();
  for (int ei = blockIdx.x; ei < n_elem; ei += gridDim.x) {
    const int e = elist ? elist[ei] : ei;   // (elist: the listed elements only, see trace_mfma_kernel)
    const ElemDesc el = ed[e];
    const SideDesc d0 = sd[6 * e + 2 * dir], d1 = sd[6 * e + 2 * dir + 1];
    const int N = el.N, N2 = N * N, N3 = N2 * N;
    // (a rolled `for (t = tid; t < N3; t += TPB)` waits for each load in turn: N3 / TPB dependent memory round trips, 21 at p = 15)
    for (int t0 = threadIdx.x; t0 < N3; t0 += 8 * TPB) {
      double uv[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) uv[c] = (t0 + c * TPB < N3) ? u[el.ns + t0 + c * TPB] : 0.0;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int t = t0 + c * TPB;
        if (t < N3) s_u[(t % N) + UJ * ((t / N) % N) + UK * (t / N2)] = uv[c];
      }
    }
#pragma unroll
    for (int s_ = 0; s_ < 2; ++s_) {
      const SideDesc& d = s_ ? d1 : d0;
      if (d.offC != cur_off[s_][0] || d.offCD != cur_off[s_][1] || N != cur_N || d.NQ != cur_NQ[s_]) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const int col = 4 * ks + mk;
          const bool in = mi < d.NQ && col < N;
          op[s_][0][ks] = in ? face_ops[d.offC + mi * N + col] : 0.0;
          op[s_][1][ks] = in ? face_ops[d.offCD + mi * N + col] : 0.0;
        }
        cur_off[s_][0] = d.offC; cur_off[s_][1] = d.offCD; cur_NQ[s_] = d.NQ;
      }
    }
    if (el.offD != cur_offD || N != cur_N) {   // unpadded N x N derivative matrix: rows 0 and N-1
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        drow[0][i] = (i < N) ? face_ops[el.offD + i] : 0.0;
        drow[1][i] = (i < N) ? face_ops[el.offD + (N - 1) * N + i] : 0.0;
      }
      cur_offD = el.offD;
    }
    cur_N = N;
    __syncthreads();
    // ---- nodal traces / normal derivatives of both faces: 256 face nodes in 4 chunks of 64 lanes
    {
      const int sn = (dir == 0) ? 1 : (dir == 1 ? UJ : UK);
      const int sa = (dir == 0) ? UJ : 1, sb = (dir == 2) ? UJ : UK;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (4 * c >= N) continue;   // wave-uniform: this chunk holds only padding
        const int idx = 64 * c + lane, a = idx & 15, b = idx >> 4;
        if (a < N && b < N) {
          double tr0 = 0.0, nd0 = 0.0, tr1 = 0.0, nd1 = 0.0;
          const int base = a * sa + b * sb;
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            if (i >= N) continue;   // wave-uniform
            const double ui = s_u[base + i * sn];
            if (i == 0) tr0 = ui;
            if (i == N - 1) tr1 = ui;
            nd0 = fma(drow[0][i], ui, nd0);
            nd1 = fma(drow[1][i], ui, nd1);
          }
          stage[a * LDM + b] = tr0;
          stage[a * LDM + 16 + b] = nd0;
          stage[16 * LDM + a * LDM + b] = tr1;
          stage[16 * LDM + a * LDM + 16 + b] = nd1;
        }
      }
    }
    wave_lds_fence();
#pragma unroll
    for (int s_ = 0; s_ < 2; ++s_) {
      const SideDesc& d = s_ ? d1 : d0;
      const int NQ = d.NQ, T = NQ * NQ;
      const double* st = stage + s_ * 16 * LDM;
      // pass 1 (transposed): rows (field, b), K = a, columns (operator, a')
      mfma_d4 ytc = {0.0, 0.0, 0.0, 0.0}, ytd = {0.0, 0.0, 0.0, 0.0}, ync = {0.0, 0.0, 0.0, 0.0};
      const int KN = (N + 3) >> 2;   // k-steps that hold data (wave-uniform): the others multiply zero padding
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        if (ks >= KN) continue;
        const double atr = st[(4 * ks + mk) * LDM + mi], and_ = st[(4 * ks + mk) * LDM + 16 + mi];
        ytc = __builtin_amdgcn_mfma_f64_16x16x4f64(atr, op[s_][0][ks], ytc, 0, 0, 0);
        ytd = __builtin_amdgcn_mfma_f64_16x16x4f64(atr, op[s_][1][ks], ytd, 0, 0, 0);
        ync = __builtin_amdgcn_mfma_f64_16x16x4f64(and_, op[s_][0][ks], ync, 0, 0, 0);
      }
      // pass 2: reg r of a pass-1 tile = rows 4 r .. 4 r + 3 (the b index) = B operand of k-step r
      mfma_d4 qu = {0.0, 0.0, 0.0, 0.0}, qta = {0.0, 0.0, 0.0, 0.0}, qtb = {0.0, 0.0, 0.0, 0.0}, qn = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (r >= KN) continue;
        qu = __builtin_amdgcn_mfma_f64_16x16x4f64(op[s_][0][r], ytc[r], qu, 0, 0, 0);
        qta = __builtin_amdgcn_mfma_f64_16x16x4f64(op[s_][0][r], ytd[r], qta, 0, 0, 0);
        qtb = __builtin_amdgcn_mfma_f64_16x16x4f64(op[s_][1][r], ytc[r], qtb, 0, 0, 0);
        qn = __builtin_amdgcn_mfma_f64_16x16x4f64(op[s_][0][r], ync[r], qn, 0, 0, 0);
      }
      // store: column mi = a', reg r: row mk + 4 r = b'
      double* out = qtrace + d.qoff;
      if (mi < NQ) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int bq = mk + 4 * r;
          if (bq < NQ) {
            out[mi + NQ * bq] = qu[r];
            out[(1 + t0) * T + mi + NQ * bq] = qta[r];
            out[(1 + t1d) * T + mi + NQ * bq] = qtb[r];
            out[(1 + dir) * T + mi + NQ * bq] = qn[r];
          }
        }
      }
    }
    __syncthreads();
  }
}

// FUSE: the Chebyshev update of the element (r = alpha (rhs - Au), p = r + beta p, u += p; cheby_update_kernel, same roundings) runs
// in the epilogue, where the element's final Au is in registers -- one kernel and one read of Au less per smoother iteration.  u is
// not an input of this kernel (the faces read traces), so updating it in place is safe.
// INPLACE: the per-wave operator apply works in place (23 KB of LDS per workgroup instead of 35 KB): faster on a mesh plan (config 2
// 41.6 -> 36.9 us, level 5 342 -> 316 us), slower on a Schwarz subdomain plan, where a third of the sides read one cached zero block and
// the kernel is bound by its LDS / issue chain rather than by memory latency (875 -> 962 us on 97 336 copies) -- chosen per plan.
template <bool FUSE, bool INPLACE>
__global__ __launch_bounds__(384, 6) void flux_wave_kernel(const double* __restrict__ qtrace, const double* __restrict__ ghost_qtrace,
                                                        double* __restrict__ Au, const SideDesc* __restrict__ sd,
                                                        const ElemDesc* __restrict__ ed, const double* __restrict__ face_ops,
                                                        const double* __restrict__ geom, const double* __restrict__ bndry_q,
                                                        const double* __restrict__ robin_c, const double* __restrict__ robin_r,
                                                        int n_elem, int xcd_chunk, ChebyFuse cf, const int* __restrict__ elist) {
  __shared__ double s_in[6][4][64];   // per wave: 4 term fields on the 8 x 8 grid
  __shared__ double s_tmp[INPLACE ? 1 : 6][INPLACE ? 1 : 4][64];
  __shared__ double s_E[6][64];       // per wave: E of its side, zero-padded to 8 x 8
  __shared__ double s_W[512];         // lifted face-local part: terms 1+3 and the tangential D^T of term 2
  __shared__ double s_N[6][64];       // per side: term 2 of the normal direction (D^T spreads it along the normal lines)
  __shared__ double s_D[64];          // zero-padded 8 x 8
  // the face index is wave-uniform: in an SGPR it turns the descriptor loads into scalar loads (no VGPRs for descriptors)
  const int f = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63, lo = lane & 7, hi = lane >> 3;
  // persistent workgroups: the descriptors of the NEXT element are requested while this one is computed
  // XCD-aware element order: workgroups are dealt round-robin to the 8 XCDs (each with its own L2), so the virtual index v is
  // mapped to element (v % 8) * chunk + v / 8: every XCD walks one contiguous (Morton-local) eighth of the elements and finds
  // its neighbours' traces in its own L2 more often.  xcd_chunk = 0: identity.
  // elist: the kernel works on the listed elements only (the hybrid operator's dirty elements; n_elem = the list's length)
  auto elem_of = [&](int v) { return elist ? elist[v] : (xcd_chunk > 0 ? (v & 7) * xcd_chunk + (v >> 3) : v); };
  int e = blockIdx.x;
  ElemDesc edn = ed[e < n_elem ? elem_of(e) : 0];
  SideDesc dn = sd[6 * (e < n_elem ? elem_of(e) : 0) + f];
  for (; e < n_elem; e += gridDim.x) {
    const ElemDesc el = edn;
    const SideDesc d = dn;
    {
      const int en = e + gridDim.x;
      if (en < n_elem) {
        edn = ed[elem_of(en)];
        dn = sd[6 * elem_of(en) + f];
      }
    }
    const int N = el.N, N2 = N * N, N3 = N2 * N, NQ = d.NQ, T = NQ * NQ;
    const bool on_m = lo < N && hi < N, on_q = lo < NQ && hi < NQ;
    // ---- every global load of this side up front (independent requests: one memory latency)
    double qm[4] = {0, 0, 0, 0}, qp[4] = {0, 0, 0, 0}, gq[7] = {0, 0, 0, 0, 0, 0, 0};
    if (on_q && d.kind != 3) {   // kind 3: a hanging side of an hp-split plan -- its terms come from the mortar-record kernel (all-zero inputs here)
      const int k = lo + NQ * hi;
      const double* m = qtrace + d.qoff + k;
#pragma unroll
      for (int c = 0; c < 4; ++c) qm[c] = m[c * T];
      if (d.kind != 0) {
        const double* p = ((d.kind == 2) ? ghost_qtrace : qtrace) + d.nbr_qoff + reorder_index(d.code, NQ - 1, lo, hi);
#pragma unroll
        for (int c = 0; c < 4; ++c) qp[c] = p[c * T];
      } else if (robin_c) {
        qp[0] = robin_r[d.geom + k];
      } else {
        qp[0] = bndry_q[d.geom + k];
      }
      if (d.kind == 0 && robin_c) {
        gq[6] = robin_c[d.geom + k];  // am = ap = 0: no term 1 / term 2 on a Robin side
      } else {
        const double* g = geom + (size_t)7 * d.geom + k;
#pragma unroll
        for (int c = 0; c < 7; ++c) gq[c] = g[c * T];
      }
    }
    const double ope = (hi < N && lo < NQ) ? face_ops[d.offE + hi * NQ + lo] : 0.0;
    const double dval = (threadIdx.x < 64) ? face_ops[el.offD + threadIdx.x] : 0.0;
    // Au_e is read now (2 values per thread) so that the final update only stores
    double au0 = 0.0, au1 = 0.0;
    if ((int)threadIdx.x < N3) au0 = Au[el.ns + threadIdx.x];
    if ((int)threadIdx.x + 384 < N3) au1 = Au[el.ns + threadIdx.x + 384];
    for (int i = threadIdx.x; i < 512; i += blockDim.x) s_W[i] = 0.0;
    s_E[f][lane] = ope;
    if (threadIdx.x < 64) s_D[threadIdx.x] = dval;
    // ---- SIPG terms at the quadrature node of this lane (padding lanes carry zeros)
    {
      double t1 = 0.0;
#pragma unroll
      for (int i = 0; i < 3; ++i) t1 += gq[i] * qm[1 + i] + gq[3 + i] * qp[1 + i];  // gq[3..5] = 0 on boundary sides
      const double jump = qm[0] - qp[0];
      const double w1 = (d.kind != 0) ? -0.5 : -1.0;
      // Robin boundary (d4est_laplacian_flux_sipg.c:339-489): sj (coeff u_m - rhs) only
      s_in[f][0][lane] = (d.kind == 0 && robin_c) ? gq[6] * qm[0] - qp[0] : w1 * t1 + gq[6] * jump;
#pragma unroll
      for (int l = 0; l < 3; ++l) s_in[f][1 + l][lane] = w1 * gq[l] * jump;
    }
    __syncthreads();
    // ---- integrate and project onto the (-) side: 4 fields on the N x N face nodes
    double res[4];
    if (INPLACE) wave_apply2d<4>(s_E[f], &s_in[f][0][0], lane, res);
    else wave_apply2d_tmp<4>(s_E[f], &s_in[f][0][0], &s_tmp[INPLACE ? 0 : f][0][0], lane, res);
    // ---- D^T of the two TANGENTIAL term-2 fields stays inside the face: val = t13 + D_a^T t2_a + D_b^T t2_b
    const int dir = f >> 1;
    const int t0 = (dir == 0) ? 1 : 0, t1d = (dir == 2) ? 1 : 2;  // reference directions of the face indices a and b
    s_in[f][0][lane] = res[1 + t0];
    s_in[f][1][lane] = res[1 + t1d];
    s_N[f][lane] = res[1 + dir];
    __syncthreads();
    double val = res[0];
#pragma unroll
    for (int q = 0; q < kFW; ++q) {
      val = fma(s_D[q * 8 + lo], s_in[f][0][q + 8 * hi], val);   // padded rows/columns of D are zero
      val = fma(s_D[q * 8 + hi], s_in[f][1][lo + 8 * q], val);
    }
    // ---- lift the face-local part, opposite faces together (disjoint node sets)
    for (int phase = 0; phase < 3; ++phase) {
      if (dir == phase && on_m) s_W[face_vol_index(f, N, lo, hi)] += val;
      __syncthreads();
    }
    // ---- Au_e += W + sum over the six sides of D[fix][.] (x) N_f  (the normal D^T touches the whole line)
#pragma unroll
    for (int rep = 0; rep < 2; ++rep) {
      const int idx = threadIdx.x + rep * 384;
      if (idx < N3) {
        const int i = idx % N, j = (idx / N) % N, k = idx / N2;
        double v = s_W[idx];
        v = fma(s_D[i], s_N[0][j + 8 * k], v);
        v = fma(s_D[(N - 1) * 8 + i], s_N[1][j + 8 * k], v);
        v = fma(s_D[j], s_N[2][i + 8 * k], v);
        v = fma(s_D[(N - 1) * 8 + j], s_N[3][i + 8 * k], v);
        v = fma(s_D[k], s_N[4][i + 8 * j], v);
        v = fma(s_D[(N - 1) * 8 + k], s_N[5][i + 8 * j], v);
        const double a = (rep == 0 ? au0 : au1) + v;
        Au[el.ns + idx] = a;
        if (FUSE) {
          const size_t o = (size_t)el.ns + idx;
          const double res = __dadd_rn(cf.rhs[o], __dmul_rn(-1.0, a));
          const double ri = __dmul_rn(cf.alpha, res);
          const double pi = __dadd_rn(__dmul_rn(cf.beta, cf.p[o]), ri);
          if (cf.r) cf.r[o] = ri;
          cf.p[o] = pi;
          (cf.u_out ? cf.u_out : cf.u)[o] = __dadd_rn(cf.u[o], pi);   // (u_out: the hybrid operator's second vector -- its clean kernels read the neighbours' u)
        }
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// Tiled MFMA flux kernel for N, NQ <= 16 (the p = 8 .. 15 counterpart of flux_wave_kernel).  One workgroup = 3 waves = the three
// reference directions of one element; wave `dir` serves faces 2 dir and 2 dir + 1.  Per face:
//   terms   lane (mi, mk) evaluates the 4 SIPG term fields at its 4 mortar nodes (a' = mi, b' = 4 ks + mk) -- exactly the values
//           it needs as the A operand of the first contraction, so the term fields never touch LDS
//   pass 1  Y_c = A_c . E^T   (contract b', 4 k-steps, tile: column = side index b, rows = a')
//   pass 2  R_c = E . Y_c     (contract a'; the tile registers of pass 1 are the B operands)            32 MFMAs for 4 fields
//   D^T     val = R_0 + D^T . R_t0  (tile registers again)  +  R_t1 . D  (one tile transposed through LDS)    8 MFMAs
// then the face-local part `val` and the normal term-2 field (whose D^T spreads along the whole normal line) of the six faces
// are combined into Au_e by all threads from LDS tiles.
// ---------------------------------------------------------------------------
template <bool FUSE>   // FUSE: Chebyshev update in the epilogue, see flux_wave_kernel
__global__ __launch_bounds__(192) void flux_mfma16_kernel(const double* __restrict__ qtrace, const double* __restrict__ ghost_qtrace,
                                                          double* __restrict__ Au, const SideDesc* __restrict__ sd,
                                                          const ElemDesc* __restrict__ ed, const double* __restrict__ face_ops,
                                                          const double* __restrict__ geom, const double* __restrict__ bndry_q,
                                                          const double* __restrict__ robin_c, const double* __restrict__ robin_r,
                                                          int n_elem, int xcd_chunk, ChebyFuse cf, const int* __restrict__ elist) {
  constexpr int LT = 17;                    // padded row length of a 16 x 16 tile in LDS
  constexpr int TPB = 192;
  __shared__ double s_tile[6][2][16 * LT];  // per face: val, normal field   (rows a, columns b)
  __shared__ double s_tr[3][16 * LT];       // per wave: transposition buffer
  __shared__ double s_Dfix[6][16];          // per face: row `fix` of D (the normal D^T)
  const int dir = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int mi = lane & 15, mk = lane >> 4;
  const int t0 = (dir == 0) ? 1 : 0, t1d = (dir == 2) ? 1 : 2;   // reference directions of the face indices a and b
  int cur_offE[2] = {-1, -1}, cur_offD = -1, cur_N = -1, cur_NQ[2] = {-1, -1};
  double opE[2][4], opD[4];   // E[mi][4 ks + mk] (N x NQ) per face;  D[4 ks + mk][mi]
#pragma unroll
  for (int i = 0; i < 4; ++i) opE[0][i] = opE[1][i] = opD[i] = 0.0;
  for (int v = blockIdx.x; v < n_elem; v += gridDim.x) {
    const int e = elist ? elist[v] : (xcd_chunk > 0 ? (v & 7) * xcd_chunk + (v >> 3) : v);   // XCD-aware element order / element list, see flux_wave_kernel
    const ElemDesc el = ed[e];
    const int N = el.N, N2 = N * N, N3 = N2 * N;
    if (el.offD != cur_offD || N != cur_N) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) opD[ks] = (4 * ks + mk < N && mi < N) ? face_ops[el.offD + (4 * ks + mk) * N + mi] : 0.0;
      cur_offD = el.offD;
    }
#pragma unroll
    for (int s_ = 0; s_ < 2; ++s_) {
      const int f = 2 * dir + s_;
      const SideDesc d = sd[6 * e + f];
      const int NQ = d.NQ, T = NQ * NQ;
      if (d.offE != cur_offE[s_] || N != cur_N || NQ != cur_NQ[s_]) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) opE[s_][ks] = (mi < N && 4 * ks + mk < NQ) ? face_ops[d.offE + mi * NQ + 4 * ks + mk] : 0.0;
        cur_offE[s_] = d.offE; cur_NQ[s_] = NQ;
      }
      if (lane < 16) s_Dfix[f][lane] = (lane < N) ? face_ops[el.offD + face_fix(f, N) * N + lane] : 0.0;
      // ---- SIPG terms at this lane's 4 mortar nodes (a' = mi, b' = 4 ks + mk): the A operands of pass 1
      double A[4][4];
      const bool robin = (d.kind == 0) && robin_c;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const int bq = 4 * ks + mk;
        A[0][ks] = A[1][ks] = A[2][ks] = A[3][ks] = 0.0;
        if (mi < NQ && bq < NQ && d.kind != 3) {   // kind 3: a hanging side of an hp-split plan -- its terms come from the mortar-record kernels
          const int k = mi + NQ * bq;
          const double* m = qtrace + d.qoff + k;
          const double um = m[0];
          if (robin) {
            A[0][ks] = robin_c[d.geom + k] * um - robin_r[d.geom + k];
          } else {
            const double* g = geom + (size_t)7 * d.geom + k;
            double up, t1 = 0.0, am[3];
            if (d.kind != 0) {
              const double* pp = ((d.kind == 2) ? ghost_qtrace : qtrace) + d.nbr_qoff + reorder_index(d.code, NQ - 1, mi, bq);
              up = pp[0];
#pragma unroll
              for (int i = 0; i < 3; ++i) {
                am[i] = g[i * T];
                t1 += am[i] * m[(1 + i) * T] + g[(3 + i) * T] * pp[(1 + i) * T];
              }
            } else {
              up = bndry_q[d.geom + k];
#pragma unroll
              for (int i = 0; i < 3; ++i) {
                am[i] = g[i * T];
                t1 += am[i] * m[(1 + i) * T];
              }
            }
            const double jump = um - up;
            const double w1 = (d.kind != 0) ? -0.5 : -1.0;
            A[0][ks] = w1 * t1 + g[6 * T] * jump;
            A[1][ks] = w1 * am[t0] * jump;    // field order: tangential a, tangential b, normal
            A[2][ks] = w1 * am[t1d] * jump;
            A[3][ks] = w1 * am[dir] * jump;
          }
        }
      }
      // ---- pass 1 / pass 2 per field
      mfma_d4 R[4];
      const int KQ = (NQ + 3) >> 2, KN = (N + 3) >> 2;   // k-steps that hold data (wave-uniform)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        mfma_d4 y = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
          if (ks < KQ) y = __builtin_amdgcn_mfma_f64_16x16x4f64(A[c][ks], opE[s_][ks], y, 0, 0, 0);
        mfma_d4 rr = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (r < KQ) rr = __builtin_amdgcn_mfma_f64_16x16x4f64(opE[s_][r], y[r], rr, 0, 0, 0);
        R[c] = rr;   // tile: column mi = b, reg r: row mk + 4 r = a
      }
      // ---- val = R_0 + D_a^T R_ta + R_tb D
      mfma_d4 val = R[0];
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (r < KN) val = __builtin_amdgcn_mfma_f64_16x16x4f64(opD[r], R[1][r], val, 0, 0, 0);   // A = D^T: D[4 r + mk][mi]
      {
        double* tb = s_tr[dir];
        wave_lds_fence();
#pragma unroll
        for (int r = 0; r < 4; ++r) tb[(mk + 4 * r) * LT + mi] = R[2][r];
        wave_lds_fence();
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          if (ks >= KN) continue;
          const double a_ = tb[mi * LT + 4 * ks + mk];            // A[i = a][k = q]
          val = __builtin_amdgcn_mfma_f64_16x16x4f64(a_, opD[ks], val, 0, 0, 0);   // B = D[k = q][j = b]
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s_tile[f][0][(mk + 4 * r) * LT + mi] = val[r];
        s_tile[f][1][(mk + 4 * r) * LT + mi] = R[3][r];
      }
    }
    cur_N = N;
    __syncthreads();
    // ---- Au_e += lift(val_f) + D[fix_f][.] (x) Nrm_f over the six faces
    // (Au and the smoother vectors of six nodes per thread are requested before the first is used: the rolled loop waited for its
    // loads every trip)
    for (int idx0 = threadIdx.x; idx0 < N3; idx0 += 6 * TPB) {
      double au_[6], rh_[6], pp_[6], uu_[6];
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        const int idx = idx0 + c * TPB;
        au_[c] = rh_[c] = pp_[c] = uu_[c] = 0.0;
        if (idx < N3) {
          const size_t o = (size_t)el.ns + idx;
          au_[c] = Au[o];
          if (FUSE) {
            rh_[c] = cf.rhs[o];
            pp_[c] = cf.p[o];
            uu_[c] = cf.u[o];
          }
        }
      }
#pragma unroll
      for (int c = 0; c < 6; ++c) {
      const int idx = idx0 + c * TPB;
      if (idx >= N3) continue;
      const int i = idx % N, j = (idx / N) % N, k = idx / N2;
      double v = 0.0;
      v = fma(s_Dfix[0][i], s_tile[0][1][j * LT + k], v);
      v = fma(s_Dfix[1][i], s_tile[1][1][j * LT + k], v);
      v = fma(s_Dfix[2][j], s_tile[2][1][i * LT + k], v);
      v = fma(s_Dfix[3][j], s_tile[3][1][i * LT + k], v);
      v = fma(s_Dfix[4][k], s_tile[4][1][i * LT + j], v);
      v = fma(s_Dfix[5][k], s_tile[5][1][i * LT + j], v);
      if (i == 0) v += s_tile[0][0][j * LT + k];
      if (i == N - 1) v += s_tile[1][0][j * LT + k];
      if (j == 0) v += s_tile[2][0][i * LT + k];
      if (j == N - 1) v += s_tile[3][0][i * LT + k];
      if (k == 0) v += s_tile[4][0][i * LT + j];
      if (k == N - 1) v += s_tile[5][0][i * LT + j];
      const size_t o = (size_t)el.ns + idx;
      const double a = au_[c] + v;
      Au[o] = a;
      if (FUSE) {
        const double res = __dadd_rn(rh_[c], __dmul_rn(-1.0, a));
        const double ri = __dmul_rn(cf.alpha, res);
        const double pi = __dadd_rn(__dmul_rn(cf.beta, pp_[c]), ri);
        if (cf.r) cf.r[o] = ri;
        cf.p[o] = pi;
        (cf.u_out ? cf.u_out : cf.u)[o] = __dadd_rn(uu_[c], pi);
      }
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// Mortar-record (hanging-face) counterparts of the tiled MFMA kernels, N, NQ <= 16: separate 1-D operators along the two
// face axes (the hp-prolongation child of a big side differs per axis), 1 or 4 records per side; the nodal trace of a big
// side is formed once and interpolated onto its four sub-mortars, and the four sub-mortar contributions of a big side are
// summed in the MFMA accumulators before the lift.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(192) void trace_hp_mfma16_kernel(const double* __restrict__ u, double* __restrict__ qtrace,
                                                              const HpMortar* __restrict__ md, const int* __restrict__ side_first,
                                                              const ElemDesc* __restrict__ ed, const double* __restrict__ face_ops,
                                                              const double* __restrict__ hp_ops, int n_elem, int max_n,
                                                              const int* __restrict__ elist = nullptr, int hang_only = 0) {
  // elist / hang_only (hp split, launch_traces): the kernel walks the listed elements -- those with a hanging side -- and serves the
  // records of their HANGING sides only; the conforming sides of the whole mesh are the fast conforming kernel's
  constexpr int LDM = 34;
  constexpr int UJ = 17, UK = 272;
  constexpr int TPB = 192;
  extern __shared__ __attribute__((aligned(16))) double smem16[];
  double* s_u = smem16;
  const int dir = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  double* stage = smem16 + max_n * UK + dir * (2 * 16 * LDM);
  const int lane = threadIdx.x & 63;
  const int mi = lane & 15, mk = lane >> 4;
  const int t0 = (dir == 0) ? 1 : 0, t1d = (dir == 2) ? 1 : 2;
  int cur_offD = -1, cur_N = -1;
  double drow[2][16];
#pragma unroll
  for (int i = 0; i < 16; ++i) drow[0][i] = drow[1][i] = 0.0;
  for (int i = lane; i < 2 * 16 * LDM; i += 64) stage[i] = 0.0;
  wave_lds_fence();
  for (int ei = blockIdx.x; ei < n_elem; ei += gridDim.x) {
    const int e = elist ? elist[ei] : ei;
    const ElemDesc el = ed[e];
    const int N = el.N, N2 = N * N, N3 = N2 * N;
    // (a rolled `for (t = tid; t < N3; t += TPB)` waits for each load in turn: N3 / TPB dependent memory round trips, 21 at p = 15)
    for (int t0 = threadIdx.x; t0 < N3; t0 += 8 * TPB) {
      double uv[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) uv[c] = (t0 + c * TPB < N3) ? u[el.ns + t0 + c * TPB] : 0.0;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int t = t0 + c * TPB;
        if (t < N3) s_u[(t % N) + UJ * ((t / N) % N) + UK * (t / N2)] = uv[c];
      }
    }
    if (el.offD != cur_offD || N != cur_N) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        drow[0][i] = (i < N) ? face_ops[el.offD + i] : 0.0;
        drow[1][i] = (i < N) ? face_ops[el.offD + (N - 1) * N + i] : 0.0;
      }
      cur_offD = el.offD;
      cur_N = N;
    }
    __syncthreads();
    {
      const int sn = (dir == 0) ? 1 : (dir == 1 ? UJ : UK);
      const int sa = (dir == 0) ? UJ : 1, sb = (dir == 2) ? UJ : UK;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (4 * c >= N) continue;
        const int idx = 64 * c + lane, a = idx & 15, b = idx >> 4;
        if (a < N && b < N) {
          double tr0 = 0.0, nd0 = 0.0, tr1 = 0.0, nd1 = 0.0;
          const int base = a * sa + b * sb;
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            if (i >= N) continue;
            const double ui = s_u[base + i * sn];
            if (i == 0) tr0 = ui;
            if (i == N - 1) tr1 = ui;
            nd0 = fma(drow[0][i], ui, nd0);
            nd1 = fma(drow[1][i], ui, nd1);
          }
          stage[a * LDM + b] = tr0;
          stage[a * LDM + 16 + b] = nd0;
          stage[16 * LDM + a * LDM + b] = tr1;
          stage[16 * LDM + a * LDM + 16 + b] = nd1;
        }
      }
    }
    wave_lds_fence();
    const int KN = (N + 3) >> 2;
#pragma unroll
    for (int s_ = 0; s_ < 2; ++s_) {
      const int sidx = 6 * e + 2 * dir + s_;
      const double* st = stage + s_ * 16 * LDM;
      double aval[2][4];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        aval[0][ks] = st[(4 * ks + mk) * LDM + mi];
        aval[1][ks] = st[(4 * ks + mk) * LDM + 16 + mi];
      }
      for (int r_ = side_first[sidx]; r_ < side_first[sidx + 1]; ++r_) {
        const HpMortar m = md[r_];
        if (hang_only && m.hang == 0.0) continue;   // (wave-uniform)
        const int NQ = m.NQ, T = NQ * NQ;
        double oa[2][4], ob[2][4];   // along a: C, CD ; along b: C, CD   -- OP[row mi][col 4 ks + mk]
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const int col = 4 * ks + mk;
          const bool in = mi < NQ && col < N;
          oa[0][ks] = in ? hp_ops[m.offCa + mi * N + col] : 0.0;
          oa[1][ks] = in ? hp_ops[m.offCDa + mi * N + col] : 0.0;
          ob[0][ks] = in ? hp_ops[m.offCb + mi * N + col] : 0.0;
          ob[1][ks] = in ? hp_ops[m.offCDb + mi * N + col] : 0.0;
        }
        mfma_d4 ytc = {0.0, 0.0, 0.0, 0.0}, ytd = {0.0, 0.0, 0.0, 0.0}, ync = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          if (ks >= KN) continue;
          ytc = __builtin_amdgcn_mfma_f64_16x16x4f64(aval[0][ks], oa[0][ks], ytc, 0, 0, 0);
          ytd = __builtin_amdgcn_mfma_f64_16x16x4f64(aval[0][ks], oa[1][ks], ytd, 0, 0, 0);
          ync = __builtin_amdgcn_mfma_f64_16x16x4f64(aval[1][ks], oa[0][ks], ync, 0, 0, 0);
        }
        mfma_d4 qu = {0.0, 0.0, 0.0, 0.0}, qta = {0.0, 0.0, 0.0, 0.0}, qtb = {0.0, 0.0, 0.0, 0.0}, qn = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (r >= KN) continue;
          qu = __builtin_amdgcn_mfma_f64_16x16x4f64(ob[0][r], ytc[r], qu, 0, 0, 0);
          qta = __builtin_amdgcn_mfma_f64_16x16x4f64(ob[0][r], ytd[r], qta, 0, 0, 0);
          qtb = __builtin_amdgcn_mfma_f64_16x16x4f64(ob[1][r], ytc[r], qtb, 0, 0, 0);
          qn = __builtin_amdgcn_mfma_f64_16x16x4f64(ob[0][r], ync[r], qn, 0, 0, 0);
        }
        double* out = qtrace + m.qoff;
        if (mi < NQ) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int bq = mk + 4 * r;
            if (bq < NQ) {
              out[mi + NQ * bq] = qu[r];
              out[(1 + t0) * T + mi + NQ * bq] = qta[r];
              out[(1 + t1d) * T + mi + NQ * bq] = qtb[r];
              out[(1 + dir) * T + mi + NQ * bq] = qn[r];
            }
          }
        }
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(192) void flux_hp_mfma16_kernel(const double* __restrict__ qtrace, const double* __restrict__ ghost_qtrace,
                                                             double* __restrict__ Au,
                                                             const HpMortar* __restrict__ md, const int* __restrict__ side_first,
                                                             const ElemDesc* __restrict__ ed, const double* __restrict__ face_ops,
                                                             const double* __restrict__ hp_ops, const double* __restrict__ geom,
                                                             const double* __restrict__ bndry_q, const double* __restrict__ robin_c,
                                                             const double* __restrict__ robin_r, int n_elem,
                                                             const int* __restrict__ elist = nullptr, int hang_only = 0) {
  // elist / hang_only: see trace_hp_mfma16_kernel (the conforming sides' terms were added by the fast conforming flux kernel)
  constexpr int LT = 17;
  constexpr int TPB = 192;
  __shared__ double s_tile[6][2][16 * LT];
  __shared__ double s_tr[3][16 * LT];
  __shared__ double s_Dfix[6][16];
  const int dir = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int mi = lane & 15, mk = lane >> 4;
  const int t0 = (dir == 0) ? 1 : 0, t1d = (dir == 2) ? 1 : 2;
  int cur_offD = -1, cur_N = -1;
  double opD[4] = {0.0, 0.0, 0.0, 0.0};
  for (int ei = blockIdx.x; ei < n_elem; ei += gridDim.x) {
    const int e = elist ? elist[ei] : ei;
    const ElemDesc el = ed[e];
    const int N = el.N, N2 = N * N, N3 = N2 * N;
    if (el.offD != cur_offD || N != cur_N) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) opD[ks] = (4 * ks + mk < N && mi < N) ? face_ops[el.offD + (4 * ks + mk) * N + mi] : 0.0;
      cur_offD = el.offD;
      cur_N = N;
    }
    const int KN = (N + 3) >> 2;
#pragma unroll
    for (int s_ = 0; s_ < 2; ++s_) {
      const int f = 2 * dir + s_, sidx = 6 * e + f;
      if (lane < 16) s_Dfix[f][lane] = (lane < N) ? face_ops[el.offD + face_fix(f, N) * N + lane] : 0.0;
      mfma_d4 R[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) R[c] = mfma_d4{0.0, 0.0, 0.0, 0.0};
      for (int r_ = side_first[sidx]; r_ < side_first[sidx + 1]; ++r_) {
        const HpMortar m = md[r_];
        if (hang_only && m.hang == 0.0) continue;   // (wave-uniform)
        const int NQ = m.NQ, T = NQ * NQ, KQ = (NQ + 3) >> 2;
        double oea[4], oeb[4];   // E along a / b: E[mi][4 ks + mk]  (N x NQ)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const bool in = mi < N && 4 * ks + mk < NQ;
          oea[ks] = in ? hp_ops[m.offEa + mi * NQ + 4 * ks + mk] : 0.0;
          oeb[ks] = in ? hp_ops[m.offEb + mi * NQ + 4 * ks + mk] : 0.0;
        }
        double A[4][4];
        const bool robin = (m.kind == 0) && robin_c;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const int bq = 4 * ks + mk;
          A[0][ks] = A[1][ks] = A[2][ks] = A[3][ks] = 0.0;
          if (mi < NQ && bq < NQ) {
            const int k = mi + NQ * bq;
            const double* qm = qtrace + m.qoff + k;
            const double um = qm[0];
            if (robin) {
              A[0][ks] = robin_c[m.gidx + k] * um - robin_r[m.gidx + k];
            } else {
              const double* g = geom + (size_t)7 * m.gidx + k;
              double up, tm = 0.0, tp = 0.0, am[3];
#pragma unroll
              for (int i = 0; i < 3; ++i) {
                am[i] = g[i * T];
                tm += am[i] * qm[(1 + i) * T];
              }
              if (m.kind != 0) {
                const double* pp = ((m.kind == 2) ? ghost_qtrace : qtrace) + m.nbr_qoff + reorder_index(m.code, NQ - 1, mi, bq);
                up = pp[m.u_shift];
#pragma unroll
                for (int i = 0; i < 3; ++i) tp += g[(3 + i) * T] * pp[(1 + i) * T];
              } else {
                up = bndry_q[m.gidx + k];
              }
              const double jump = um - up;
              const double w1 = (m.kind != 0) ? -0.5 : -1.0;
              A[0][ks] = w1 * (tm + tp) + g[6 * T] * jump;   // (fm, fp, w2: folded into the factors by face_geom_hp_kernel)
              A[1][ks] = w1 * am[t0] * jump;
              A[2][ks] = w1 * am[t1d] * jump;
              A[3][ks] = w1 * am[dir] * jump;
            }
          }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          mfma_d4 y = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int ks = 0; ks < 4; ++ks)
            if (ks < KQ) y = __builtin_amdgcn_mfma_f64_16x16x4f64(A[c][ks], oeb[ks], y, 0, 0, 0);
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (r < KQ) R[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(oea[r], y[r], R[c], 0, 0, 0);   // summed over the side's mortars
        }
      }
      mfma_d4 val = R[0];
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (r < KN) val = __builtin_amdgcn_mfma_f64_16x16x4f64(opD[r], R[1][r], val, 0, 0, 0);
      {
        double* tb = s_tr[dir];
        wave_lds_fence();
#pragma unroll
        for (int r = 0; r < 4; ++r) tb[(mk + 4 * r) * LT + mi] = R[2][r];
        wave_lds_fence();
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          if (ks >= KN) continue;
          const double a_ = tb[mi * LT + 4 * ks + mk];
          val = __builtin_amdgcn_mfma_f64_16x16x4f64(a_, opD[ks], val, 0, 0, 0);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s_tile[f][0][(mk + 4 * r) * LT + mi] = val[r];
        s_tile[f][1][(mk + 4 * r) * LT + mi] = R[3][r];
      }
    }
    __syncthreads();
    for (int idx0 = threadIdx.x; idx0 < N3; idx0 += 8 * TPB) {
      double au_[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) au_[c] = (idx0 + c * TPB < N3) ? Au[el.ns + idx0 + c * TPB] : 0.0;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
      const int idx = idx0 + c * TPB;
      if (idx >= N3) continue;
      const int i = idx % N, j = (idx / N) % N, k = idx / N2;
      double v = 0.0;
      v = fma(s_Dfix[0][i], s_tile[0][1][j * LT + k], v);
      v = fma(s_Dfix[1][i], s_tile[1][1][j * LT + k], v);
      v = fma(s_Dfix[2][j], s_tile[2][1][i * LT + k], v);
      v = fma(s_Dfix[3][j], s_tile[3][1][i * LT + k], v);
      v = fma(s_Dfix[4][k], s_tile[4][1][i * LT + j], v);
      v = fma(s_Dfix[5][k], s_tile[5][1][i * LT + j], v);
      if (i == 0) v += s_tile[0][0][j * LT + k];
      if (i == N - 1) v += s_tile[1][0][j * LT + k];
      if (j == 0) v += s_tile[2][0][i * LT + k];
      if (j == N - 1) v += s_tile[3][0][i * LT + k];
      if (k == 0) v += s_tile[4][0][i * LT + j];
      if (k == N - 1) v += s_tile[5][0][i * LT + j];
      Au[el.ns + idx] = au_[c] + v;
      }
    }
    __syncthreads();
  }
}


// ---------------------------------------------------------------------------
// hp split, the record kernels' work in its parallel form: a UNIT is one side that stays with the mortar records (a big hanging side: 4
// records; a small side the conforming kernels cannot take: 1), and its records go to the 4 wavefronts of a workgroup side by side
// instead of one after the other.  The two kernels above walk an element's sides in three direction-waves and a side's records in
// a loop: on a locally refined mesh (one hanging side per listed element, a few hundred listed elements) two of the three waves find
// nothing to do and the third runs four dependent chains of descriptor load -> operator / trace loads -> MFMA one after another
// (13.8 + 22.7 us per apply at level 4, p = 7, 350 listed elements: pure latency).  Same arithmetic per record; the four sub-mortar
// contributions of a big side meet in LDS and are summed in record order (deterministic).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void trace_unit_kernel(const double* __restrict__ u, double* __restrict__ qtrace,
                                                         const HpMortar* __restrict__ md, const HangUnit* __restrict__ units,
                                                         const ElemDesc* __restrict__ ed, const double* __restrict__ face_ops,
                                                         const double* __restrict__ hp_ops, int n_units, int max_n) {
  constexpr int LDM = 34;
  constexpr int TPB = 256;
  // the element's u as [i + UJ (j + ...)] with odd row and slab strides sized by the plan's largest degree (a p = 7 plan: 5.3 KB instead of
  // the 17.4 KB of the 16-wide image: workgroups per CU are what bounds this kernel on densely refined meshes)
  const int UJ = max_n | 1, UK = (max_n * UJ) | 1;
  extern __shared__ __attribute__((aligned(16))) double smem16[];
  double* s_u = smem16;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  double* stage = smem16 + ((max_n * UK + 1) & ~1) + wv * (16 * LDM);   // per wave: the side's nodal trace (columns 0..15) and normal derivative (16..31)
  const int lane = threadIdx.x & 63;
  const int mi = lane & 15, mk = lane >> 4;
  for (int i = lane; i < 16 * LDM; i += 64) stage[i] = 0.0;
  for (int ui = blockIdx.x; ui < n_units; ui += gridDim.x) {
    const HangUnit un = units[ui];
    const ElemDesc el = ed[un.e];
    const int N = el.N, N2 = N * N, N3 = N2 * N;
    const int dir = un.f >> 1, hi = un.f & 1;
    const int t0 = (dir == 0) ? 1 : 0, t1d = (dir == 2) ? 1 : 2;
    // this wave's record, requested with the element's data (its operator offsets are needed two round trips later)
    const bool have = wv < un.nrec;
    const HpMortar m = md[un.r0 + (have ? wv : 0)];
    for (int tb = threadIdx.x; tb < N3; tb += 8 * TPB) {
      double uv[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) uv[c] = (tb + c * TPB < N3) ? u[el.ns + tb + c * TPB] : 0.0;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int t = tb + c * TPB;
        if (t < N3) s_u[(t % N) + UJ * ((t / N) % N) + UK * (t / N2)] = uv[c];
      }
    }
    double drow[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) drow[i] = (i < N) ? face_ops[el.offD + (hi ? (N - 1) * N : 0) + i] : 0.0;
    const int NQ = m.NQ, T = NQ * NQ;
    double oa[2][4], ob[2][4];   // along a: C, CD ; along b: C, CD   -- OP[row mi][col 4 ks + mk]
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int col = 4 * ks + mk;
      const bool in = have && mi < NQ && col < N;
      oa[0][ks] = in ? hp_ops[m.offCa + mi * N + col] : 0.0;
      oa[1][ks] = in ? hp_ops[m.offCDa + mi * N + col] : 0.0;
      ob[0][ks] = in ? hp_ops[m.offCb + mi * N + col] : 0.0;
      ob[1][ks] = in ? hp_ops[m.offCDb + mi * N + col] : 0.0;
    }
    __syncthreads();
    if (have) {
      const int sn = (dir == 0) ? 1 : (dir == 1 ? UJ : UK);
      const int sa = (dir == 0) ? UJ : 1, sb = (dir == 2) ? UJ : UK;
      const int fixo = hi ? (N - 1) * sn : 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (4 * c >= N) continue;
        const int idx = 64 * c + lane, a = idx & 15, b = idx >> 4;
        if (a < N && b < N) {
          double nd = 0.0;
          const int base = a * sa + b * sb;
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            if (i >= N) continue;
            nd = fma(drow[i], s_u[base + i * sn], nd);
          }
          stage[a * LDM + b] = s_u[base + fixo];
          stage[a * LDM + 16 + b] = nd;
        }
      }
      wave_lds_fence();
      const int KN = (N + 3) >> 2;
      double aval[2][4];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        aval[0][ks] = stage[(4 * ks + mk) * LDM + mi];
        aval[1][ks] = stage[(4 * ks + mk) * LDM + 16 + mi];
      }
      mfma_d4 ytc = {0.0, 0.0, 0.0, 0.0}, ytd = {0.0, 0.0, 0.0, 0.0}, ync = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        if (ks >= KN) continue;
        ytc = __builtin_amdgcn_mfma_f64_16x16x4f64(aval[0][ks], oa[0][ks], ytc, 0, 0, 0);
        ytd = __builtin_amdgcn_mfma_f64_16x16x4f64(aval[0][ks], oa[1][ks], ytd, 0, 0, 0);
        ync = __builtin_amdgcn_mfma_f64_16x16x4f64(aval[1][ks], oa[0][ks], ync, 0, 0, 0);
      }
      mfma_d4 qu = {0.0, 0.0, 0.0, 0.0}, qta = {0.0, 0.0, 0.0, 0.0}, qtb = {0.0, 0.0, 0.0, 0.0}, qn = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (r >= KN) continue;
        qu = __builtin_amdgcn_mfma_f64_16x16x4f64(ob[0][r], ytc[r], qu, 0, 0, 0);
        qta = __builtin_amdgcn_mfma_f64_16x16x4f64(ob[0][r], ytd[r], qta, 0, 0, 0);
        qtb = __builtin_amdgcn_mfma_f64_16x16x4f64(ob[1][r], ytc[r], qtb, 0, 0, 0);
        qn = __builtin_amdgcn_mfma_f64_16x16x4f64(ob[0][r], ync[r], qn, 0, 0, 0);
      }
      double* out = qtrace + m.qoff;
      if (mi < NQ) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int bq = mk + 4 * r;
          if (bq < NQ) {
            out[mi + NQ * bq] = qu[r];
            out[(1 + t0) * T + mi + NQ * bq] = qta[r];
            out[(1 + t1d) * T + mi + NQ * bq] = qtb[r];
            out[(1 + dir) * T + mi + NQ * bq] = qn[r];
          }
        }
      }
    }
    __syncthreads();
  }
}

// one workgroup per listed element; its units one after the other, a unit's records on the 4 wavefronts.
// FUSE: the Chebyshev update of the listed elements in the epilogue (their A u is final only here: hybrid operator, hanging-aware form;
// roundings of cheby_update_kernel; the new iterate goes to cf.u_out -- the operator kernel reads the neighbours' u)
// TS: tile size of the LDS images (8 where every degree of the plan is <= 7: 15 KB instead of 55 KB per workgroup -- on densely refined
// meshes the workgroups per CU bound this kernel --, else 16)
template <bool FUSE, int TS>
__global__ __launch_bounds__(256) void flux_unit_kernel(const double* __restrict__ qtrace, const double* __restrict__ ghost_qtrace,
                                                        double* __restrict__ Au, const HpMortar* __restrict__ md,
                                                        const HangUnit* __restrict__ units, const int* __restrict__ unit_first,
                                                        const ElemDesc* __restrict__ ed, const double* __restrict__ face_ops,
                                                        const double* __restrict__ hp_ops, const double* __restrict__ geom,
                                                        const double* __restrict__ bndry_q, const double* __restrict__ robin_c,
                                                        const double* __restrict__ robin_r, int n_elem, ChebyFuse cf) {
  constexpr int LT = TS + 1;
  constexpr int TPB = 256;
  constexpr int NAU = (TS <= 8) ? 2 : 8;   // nodes of the element per thread and sweep (N <= 8: 512 nodes = two per thread)
  __shared__ double s_tile[6][2][TS * LT];
  __shared__ double s_part[3][4][TS * LT];   // waves 1..3: their record's four lifted fields
  __shared__ double s_tr[TS * LT];
  __shared__ double s_Dfix[6][16];
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int mi = lane & 15, mk = lane >> 4;
  for (int ei = blockIdx.x; ei < n_elem; ei += gridDim.x) {
    const int u0 = unit_first[ei], u1 = unit_first[ei + 1];
    if (u0 == u1) continue;
    const HangUnit first = units[u0];
    const ElemDesc el = ed[first.e];
    const int N = el.N, N2 = N * N, N3 = N2 * N;
    const int KN = (N + 3) >> 2;
    // A u of the element, requested before anything else: it is added to at the very end
    double au_[NAU], rh_[FUSE ? NAU : 1], pp_[FUSE ? NAU : 1], uu_[FUSE ? NAU : 1];
    {
#pragma unroll
      for (int c = 0; c < NAU; ++c) {
        const bool in = threadIdx.x + c * TPB < N3;
        const size_t o = (size_t)el.ns + threadIdx.x + c * TPB;
        au_[c] = in ? Au[o] : 0.0;
        if constexpr (FUSE) { rh_[c] = in ? cf.rhs[o] : 0.0; pp_[c] = in ? cf.p[o] : 0.0; uu_[c] = in ? cf.u[o] : 0.0; }
      }
    }
    double opD[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) opD[ks] = (4 * ks + mk < N && mi < N) ? face_ops[el.offD + (4 * ks + mk) * N + mi] : 0.0;
    int mask = 0;
    for (int ui = u0; ui < u1; ++ui) {
      const HangUnit un = (ui == u0) ? first : units[ui];
      const int f = un.f, dir = f >> 1;
      const int t0 = (dir == 0) ? 1 : 0, t1d = (dir == 2) ? 1 : 2;
      mask |= 1 << f;
      if (wv == 0 && lane < 16) s_Dfix[f][lane] = (lane < N) ? face_ops[el.offD + face_fix(f, N) * N + lane] : 0.0;
      mfma_d4 R[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) R[c] = mfma_d4{0.0, 0.0, 0.0, 0.0};
      if (wv < un.nrec) {
        const HpMortar m = md[un.r0 + wv];
        const int NQ = m.NQ, T = NQ * NQ, KQ = (NQ + 3) >> 2;
        double oea[4], oeb[4];   // E along a / b: E[mi][4 ks + mk]  (N x NQ)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const bool in = mi < N && 4 * ks + mk < NQ;
          oea[ks] = in ? hp_ops[m.offEa + mi * NQ + 4 * ks + mk] : 0.0;
          oeb[ks] = in ? hp_ops[m.offEb + mi * NQ + 4 * ks + mk] : 0.0;
        }
        double A[4][4];
        const bool robin = (m.kind == 0) && robin_c;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const int bq = 4 * ks + mk;
          A[0][ks] = A[1][ks] = A[2][ks] = A[3][ks] = 0.0;
          if (mi < NQ && bq < NQ) {
            const int k = mi + NQ * bq;
            const double* qm = qtrace + m.qoff + k;
            const double um = qm[0];
            if (robin) {
              A[0][ks] = robin_c[m.gidx + k] * um - robin_r[m.gidx + k];
            } else {
              const double* g = geom + (size_t)7 * m.gidx + k;
              double up, tm = 0.0, tp = 0.0, am[3];
#pragma unroll
              for (int i = 0; i < 3; ++i) {
                am[i] = g[i * T];
                tm += am[i] * qm[(1 + i) * T];
              }
              if (m.kind != 0) {
                const double* pp = ((m.kind == 2) ? ghost_qtrace : qtrace) + m.nbr_qoff + reorder_index(m.code, NQ - 1, mi, bq);
                up = pp[m.u_shift];
#pragma unroll
                for (int i = 0; i < 3; ++i) tp += g[(3 + i) * T] * pp[(1 + i) * T];
              } else {
                up = bndry_q[m.gidx + k];
              }
              const double jump = um - up;
              const double w1 = (m.kind != 0) ? -0.5 : -1.0;
              A[0][ks] = w1 * (tm + tp) + g[6 * T] * jump;   // (fm, fp, w2: folded into the factors by face_geom_hp_kernel)
              A[1][ks] = w1 * am[t0] * jump;
              A[2][ks] = w1 * am[t1d] * jump;
              A[3][ks] = w1 * am[dir] * jump;
            }
          }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          mfma_d4 y = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int ks = 0; ks < 4; ++ks)
            if (ks < KQ) y = __builtin_amdgcn_mfma_f64_16x16x4f64(A[c][ks], oeb[ks], y, 0, 0, 0);
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (r < KQ) R[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(oea[r], y[r], R[c], 0, 0, 0);
        }
        if (wv > 0 && mi < TS) {
#pragma unroll
          for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (mk + 4 * r < TS) s_part[wv - 1][c][(mk + 4 * r) * LT + mi] = R[c][r];
        }
      }
      __syncthreads();
      if (wv == 0) {
        for (int w = 1; w < un.nrec; ++w) {   // the side's mortars, summed in record order
#pragma unroll
          for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (mi < TS && mk + 4 * r < TS) R[c][r] += s_part[w - 1][c][(mk + 4 * r) * LT + mi];
        }
        mfma_d4 val = R[0];
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (r < KN) val = __builtin_amdgcn_mfma_f64_16x16x4f64(opD[r], R[1][r], val, 0, 0, 0);
        wave_lds_fence();
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (mi < TS && mk + 4 * r < TS) s_tr[(mk + 4 * r) * LT + mi] = R[2][r];
        wave_lds_fence();
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          if (ks >= KN) continue;
          const double a_ = (mi < TS && 4 * ks + mk < TS) ? s_tr[mi * LT + 4 * ks + mk] : 0.0;
          val = __builtin_amdgcn_mfma_f64_16x16x4f64(a_, opD[ks], val, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (mi < TS && mk + 4 * r < TS) {
            s_tile[f][0][(mk + 4 * r) * LT + mi] = val[r];
            s_tile[f][1][(mk + 4 * r) * LT + mi] = R[3][r];
          }
        }
      }
      __syncthreads();
    }
    for (int idx0 = threadIdx.x; idx0 < N3; idx0 += NAU * TPB) {
      if (idx0 != (int)threadIdx.x) {   // (N > 12: a second sweep)
#pragma unroll
        for (int c = 0; c < NAU; ++c) {
          const bool in = idx0 + c * TPB < N3;
          const size_t o = (size_t)el.ns + idx0 + c * TPB;
          au_[c] = in ? Au[o] : 0.0;
          if constexpr (FUSE) { rh_[c] = in ? cf.rhs[o] : 0.0; pp_[c] = in ? cf.p[o] : 0.0; uu_[c] = in ? cf.u[o] : 0.0; }
        }
      }
#pragma unroll
      for (int c = 0; c < NAU; ++c) {
        const int idx = idx0 + c * TPB;
        if (idx >= N3) continue;
        const int i = idx % N, j = (idx / N) % N, k = idx / N2;
        double v = 0.0;
        if (mask & 1) { v = fma(s_Dfix[0][i], s_tile[0][1][j * LT + k], v); if (i == 0) v += s_tile[0][0][j * LT + k]; }
        if (mask & 2) { v = fma(s_Dfix[1][i], s_tile[1][1][j * LT + k], v); if (i == N - 1) v += s_tile[1][0][j * LT + k]; }
        if (mask & 4) { v = fma(s_Dfix[2][j], s_tile[2][1][i * LT + k], v); if (j == 0) v += s_tile[2][0][i * LT + k]; }
        if (mask & 8) { v = fma(s_Dfix[3][j], s_tile[3][1][i * LT + k], v); if (j == N - 1) v += s_tile[3][0][i * LT + k]; }
        if (mask & 16) { v = fma(s_Dfix[4][k], s_tile[4][1][i * LT + j], v); if (k == 0) v += s_tile[4][0][i * LT + j]; }
        if (mask & 32) { v = fma(s_Dfix[5][k], s_tile[5][1][i * LT + j], v); if (k == N - 1) v += s_tile[5][0][i * LT + j]; }
        const double a_ = au_[c] + v;
        if (!FUSE || !cf.skip_Au_store) Au[el.ns + idx] = a_;
        if constexpr (FUSE) {
          const size_t o = (size_t)el.ns + idx;
          const double res = __dadd_rn(rh_[c], __dmul_rn(-1.0, a_));
          const double ri = __dmul_rn(cf.alpha, res);
          const double pi = __dadd_rn(__dmul_rn(cf.beta, pp_[c]), ri);
          if (cf.r) cf.r[o] = ri;
          cf.p[o] = pi;
          cf.u_out[o] = __dadd_rn(uu_[c], pi);
        }
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// launch section (the host set-up that produces what these launchers read: d4est_hip_faces_setup.hip; the geometry and
// boundary-data setters: d4est_hip_faces_geometry.hip)
// ---------------------------------------------------------------------------

// resident workgroups per CU assumed by the persistent fast kernels (experiment knob: D4EST_HIP_FACE_WG_PER_CU)
static int face_wg_per_cu() {
  static int v = -1;
  if (v < 0) {
    const char* e = std::getenv("D4EST_HIP_FACE_WG_PER_CU");
    v = e ? std::atoi(e) : 4;
    if (v < 1) v = 4;
  }
  return v;
}

static void debug_occupancy_once() {
  static bool done = false;
  if (done || !std::getenv("D4EST_HIP_DEBUG_OCC")) return;
  done = true;
  int nt = -1, nf = -1;
  (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nt, reinterpret_cast<const void*>(trace_wave_kernel), 384, 0);
  (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nf, reinterpret_cast<const void*>(flux_wave_kernel<false, true>), 384, 0);
  hipFuncAttributes at{}, af{};
  (void)hipFuncGetAttributes(&at, reinterpret_cast<const void*>(trace_wave_kernel));
  (void)hipFuncGetAttributes(&af, reinterpret_cast<const void*>(flux_wave_kernel<false, true>));
  std::fprintf(stderr, "[d4est_hip] occupancy: trace_wave %d wg/CU (regs %d, lds %zu, scratch %zu) flux_wave %d wg/CU (regs %d, lds %zu, scratch %zu)\n",
               nt, at.numRegs, at.sharedSizeBytes, at.localSizeBytes, nf, af.numRegs, af.sharedSizeBytes, af.localSizeBytes);
}

static size_t generic_lds_bytes(const d4est_hip_plan* plan) { return (size_t)plan->max_face_lds_doubles * sizeof(double); }

// ---- which kernels serve a plan.  The one place that decides it: launch_traces, launch_flux, flux_can_fuse_update and the list rules
// below all read it.  Computed per call from the set-up's findings and the tuning keys as they are NOW (keys are flipped on live plans).
enum class FaceFamily {
  HpSplitFast,    // hanging faces, hp split: conforming sides through the p <= 7 kernels, hanging sides through the record kernels
  HpSplitTiled,   // ... conforming sides through the tiled 16 x 16 kernels (or both conforming families on lists)
  HpTiled,        // hanging faces, no split: the tiled record kernels for every side
  HpGeneric,      // hanging faces, any degree
  ConfFastMfma,   // conforming, every N, NQ <= 8: trace_mfma_kernel + flux_wave_kernel
  ConfFastWave,   // ... tuning key 3 = 1: trace_wave_kernel + flux_wave_kernel
  FamilySplit,    // conforming mixed-degree with degrees above 7: p <= 7 kernels and tiled kernels, each on its list
  Tiled,          // conforming, N, NQ <= 16: trace_mfma16_kernel + flux_mfma16_kernel
  Generic,
};
static FaceFamily face_family(const d4est_hip_plan* plan, const FaceHost& fh) {
  const int fast_key = plan->tuning[D4EST_HIP_TUNE_FLUX_FAST];
  if (fh.hp) {
    if (fh.hp_split) return fh.hp_split_fast ? FaceFamily::HpSplitFast : FaceFamily::HpSplitTiled;   // (decided at set-up)
    return (fast_key != 0 && fh.hp_max_N <= 16 && fh.hp_max_NQ <= 16) ? FaceFamily::HpTiled : FaceFamily::HpGeneric;
  }
  if (fast_key == 0) return FaceFamily::Generic;
  if (plan->face_fast) return fast_key != 1 ? FaceFamily::ConfFastMfma : FaceFamily::ConfFastWave;
  if (fh.family_split) return FaceFamily::FamilySplit;   // (set-up takes it only where the tiled kernels apply: N, NQ <= 16)
  return (fh.max_N <= 16 && fh.max_NQ <= 16) ? FaceFamily::Tiled : FaceFamily::Generic;
}
static bool family_hp_split(FaceFamily f) { return f == FaceFamily::HpSplitFast || f == FaceFamily::HpSplitTiled; }
// the trace kernels with an element-list form (the other families compute every element's traces) ...
static bool trace_takes_list(FaceFamily f) { return f != FaceFamily::HpGeneric && f != FaceFamily::ConfFastWave && f != FaceFamily::Generic; }
// ... and the flux kernels with one (the hybrid operator is not set up on the others)
static bool flux_takes_list(FaceFamily f) { return f != FaceFamily::HpGeneric && f != FaceFamily::Generic; }
// the flux kernels whose epilogue can carry the Chebyshev update
static bool flux_family_fuses(FaceFamily f) {
  return f == FaceFamily::ConfFastMfma || f == FaceFamily::ConfFastWave || f == FaceFamily::FamilySplit || f == FaceFamily::Tiled;
}

// the two conforming families' lists of one launch: the whole plan's, or the hybrid operator's ring (traces) / dirty (flux) list split
// the same way; a list without a split of its own goes through the tiled kernels whole
struct FamilyLists {
  bool on;
  const int *small, *big;
  int n_small, n_big;
};
static FamilyLists family_lists(const FaceHost& fh, const int* elist, bool ring) {
  const int* hy = ring ? fh.hy_ring : fh.hy_dirty;
  const ElemList& hy_small = ring ? fh.ring_small : fh.dirty_small;
  const ElemList& small = elist ? hy_small : fh.fam_small;
  const ElemList& big = elist ? (ring ? fh.ring_big : fh.dirty_big) : fh.fam_big;
  FamilyLists l;
  l.on = fh.family_split && (!elist || (elist == hy && hy_small.d));
  l.small = small.d;
  l.big = big.d;
  l.n_small = small.n;
  l.n_big = big.n;
  return l;
}

// ---- one launcher per kernel: it owns the grid, the block, the LDS size and the plan's arguments; the callers pass what varies
static int face_cus(const d4est_hip_plan* plan) { return plan->n_cus > 0 ? plan->n_cus : 256; }
// persistent grid: `resident` workgroups at most, every one with the same number of rounds over the n elements
static int persistent_grid(int n, int resident) {
  const int rounds = (n + resident - 1) / resident;
  return (n + rounds - 1) / rounds;
}
// XCD-aware element order (chunk = n / 8 elements per XCD) on whole-plan launches only: 0 with an element list, the family lists included
static int xcd_chunk(const int* elist, int n, int grid) {
  static const bool no_remap = std::getenv("D4EST_HIP_NO_XCD_REMAP") != nullptr;
  return (!elist && n % 8 == 0 && grid % 8 == 0 && !no_remap) ? n / 8 : 0;
}
static const double* robin_c_of(const FaceHost& fh) { return fh.robin ? fh.d_robin_c : nullptr; }
static const double* robin_r_of(const FaceHost& fh) { return fh.robin ? fh.d_robin_r : nullptr; }

void faces_robin(d4est_hip_plan* plan, const double** robin_c, const double** robin_r) {
  const FaceHost& fh = face_host(plan);
  *robin_c = robin_c_of(fh);
  *robin_r = robin_r_of(fh);
}

// p <= 7, 3 waves.  Inherited: 8 resident workgroups per CU (47 VGPRs, 11.5 KB LDS) where the flux kernels take face_wg_per_cu()
static void run_trace_mfma(d4est_hip_plan* plan, const double* u, double* trace, int n, const int* elist, int wg_per_cu = 8) {
  hipLaunchKernelGGL(trace_mfma_kernel, dim3(persistent_grid(n, wg_per_cu * face_cus(plan))), dim3(192), 0, plan->stream, u, trace,
                     (const SideDesc*)plan->d_side_desc, (const ElemDesc*)plan->d_elem_desc, plan->d_face_ops, n, elist);
}
// p <= 7, 6 waves, no list form
static void run_trace_wave(d4est_hip_plan* plan, const FaceHost& fh, const double* u, double* trace, int n, int wg_per_cu) {
  hipLaunchKernelGGL(trace_wave_kernel, dim3(persistent_grid(n, wg_per_cu * face_cus(plan))), dim3(384), 0, plan->stream, u, trace,
                     (const SideDesc*)plan->d_side_desc, (const ElemDesc*)plan->d_elem_desc, plan->d_face_ops, n, fh.uni);
}
// p = 8 .. 15: tiled MFMA trace kernel (descriptors with unpadded N x N derivative matrices).  Only local elements are copied to LDS:
// the copy of u is sized by the largest LOCAL degree (cached at set-up: no per-launch walk over the elements)
static void run_trace_mfma16(d4est_hip_plan* plan, const FaceHost& fh, const double* u, double* trace, int n, const int* elist) {
  const size_t lds = (size_t)(fh.max_local_N * 272 + 3 * 2 * 16 * 34) * sizeof(double);
  set_lds_limit(trace_mfma16_kernel, lds);
  const int per_cu = (int)std::min<size_t>(8, (160 * 1024) / lds);
  hipLaunchKernelGGL(trace_mfma16_kernel, dim3(std::min(n, per_cu * face_cus(plan))), dim3(192), lds, plan->stream, u, trace,
                     (const SideDesc*)plan->d_side_desc, (const ElemDesc*)fh.d_elem_desc_generic, plan->d_face_ops, n, fh.max_local_N, elist);
}
// both conforming families on their lists; false: this launch's list has no split of its own (the caller sends it through the tiled kernel)
static bool run_trace_families(d4est_hip_plan* plan, const FaceHost& fh, const double* u, double* trace, const int* elist) {
  const FamilyLists l = family_lists(fh, elist, /*ring=*/true);
  if (!l.on) return false;
  if (l.n_small > 0) run_trace_mfma(plan, u, trace, l.n_small, l.small);
  if (l.n_big > 0) run_trace_mfma16(plan, fh, u, trace, l.n_big, l.big);
  return true;
}
// the hanging sides of the hp split, one unit (side with live records) per workgroup round
static void run_trace_unit(d4est_hip_plan* plan, const FaceHost& fh, const double* u, double* trace) {
  const int uj = fh.hp_max_N | 1, uk = (fh.hp_max_N * uj) | 1;
  const size_t lds = (size_t)(((fh.hp_max_N * uk + 1) & ~1) + 4 * 16 * 34) * sizeof(double);
  const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(8, (160 * 1024) / lds));
  hipLaunchKernelGGL(trace_unit_kernel, dim3(std::min(fh.n_units, per_cu * face_cus(plan))), dim3(256), lds, plan->stream, u, trace, fh.d_rec,
                     fh.d_units, (const ElemDesc*)fh.d_elem_desc_generic, plan->d_face_ops, fh.d_hp_ops, fh.n_units, fh.hp_max_N);
}
// tiled record kernel, 4 workgroups per CU.  hang_only = 1: the hanging sides of the listed elements (hp split), 0: every side
static void run_trace_hp_mfma16(d4est_hip_plan* plan, const FaceHost& fh, const double* u, double* trace, int n, const int* elist, int hang_only) {
  const size_t lds = (size_t)(fh.hp_max_N * 272 + 3 * 2 * 16 * 34) * sizeof(double);
  set_lds_limit(trace_hp_mfma16_kernel, lds);
  hipLaunchKernelGGL(trace_hp_mfma16_kernel, dim3(std::min(n, 4 * face_cus(plan))), dim3(192), lds, plan->stream, u, trace, fh.d_rec,
                     fh.d_side_first, (const ElemDesc*)fh.d_elem_desc_generic, plan->d_face_ops, fh.d_hp_ops, n, fh.hp_max_N, elist, hang_only);
}
static void run_trace_hp_generic(d4est_hip_plan* plan, const FaceHost& fh, const double* u, double* trace, int n) {
  const size_t lds = fh.hp_lds_doubles * sizeof(double);
  set_lds_limit(trace_hp_kernel, lds);
  hipLaunchKernelGGL(trace_hp_kernel, dim3(std::min(n, 16384)), dim3(256), lds, plan->stream, u, trace, fh.d_rec, fh.d_elem_first,
                     (const ElemDesc*)fh.d_elem_desc_generic, plan->d_face_ops, fh.d_hp_ops, n, fh.hp_fld_stride);
}
static void run_trace_generic(d4est_hip_plan* plan, const FaceHost& fh, const double* u, double* trace, int n) {
  const size_t lds = generic_lds_bytes(plan);
  set_lds_limit(trace_generic_kernel, lds);
  hipLaunchKernelGGL(trace_generic_kernel, dim3(std::min(n, 16384)), dim3(256), lds, plan->stream, u, trace, (const SideDesc*)plan->d_side_desc,
                     (const ElemDesc*)fh.d_elem_desc_generic, plan->d_face_ops, n, fh.fld_stride);
}

void launch_traces(d4est_hip_plan* plan, const double* u, double* trace, bool ghost, const int* elist, int n_list, int parts) {
  FaceHost& fh = face_host(plan);
  if (ghost) {
    if (fh.hp) D4EST_HIP_ABORT("compute_ghost_traces: plans with hanging faces take their ghost traces from the trace exchange (d4est_hip_plan_*_sub offsets), not from whole ghost elements");
    if (fh.n_ghost_sides == 0) return;
    const size_t lds = generic_lds_bytes(plan);
    set_lds_limit(ghost_trace_kernel, lds);
    hipLaunchKernelGGL(ghost_trace_kernel, dim3(std::min(fh.n_ghost_sides, 16384)), dim3(256), lds, plan->stream, u, trace,
                       fh.d_ghost_sides, plan->d_face_ops, fh.n_ghost_sides, fh.fld_stride);
    HIP_CHECK(hipGetLastError());
    return;
  }
  const FaceFamily fam = face_family(plan, fh);
  // elist: only these elements' traces are needed (inherited: an hp-split plan whose key 3 was set to 0 afterwards computes every element)
  if (!(trace_takes_list(fam) && plan->tuning[D4EST_HIP_TUNE_FLUX_FAST] != 0)) elist = nullptr;
  const int n = elist ? n_list : plan->n_elements;
  if (parts != 3 && !family_hp_split(fam)) D4EST_HIP_ABORT("launch_traces: parts = %d on a plan without the hp split", parts);
  if (n == 0 && !(family_hp_split(fam) && (parts & 2))) return;
  switch (fam) {
    case FaceFamily::HpSplitFast:
    case FaceFamily::HpSplitTiled:
      // every conforming side from the conforming kernels, then the hanging sides of the elements that have one (the record kernel
      // overwrites the blocks the first kernel filled for those sides)
      if (n > 0 && (parts & 1)) {
        if (fam == FaceFamily::HpSplitFast) run_trace_mfma(plan, u, trace, n, elist);
        else if (!run_trace_families(plan, fh, u, trace, elist)) run_trace_mfma16(plan, fh, u, trace, n, elist);
      }
      if ((parts & 2) && fh.n_units > 0) run_trace_unit(plan, fh, u, trace);
      else if ((parts & 2) && fh.hang_elems.n > 0) run_trace_hp_mfma16(plan, fh, u, trace, fh.hang_elems.n, fh.hang_elems.d, 1);
      break;
    case FaceFamily::HpTiled: run_trace_hp_mfma16(plan, fh, u, trace, n, elist, 0); break;
    case FaceFamily::HpGeneric: run_trace_hp_generic(plan, fh, u, trace, n); break;
    case FaceFamily::ConfFastMfma:
    case FaceFamily::ConfFastWave: {
      // resident workgroups per CU: 8 of the 3-wave MFMA kernel, 4 of the 6-wave kernel.  Inherited: D4EST_HIP_FACE_WG_PER_CU overrides
      // the trace grid on this family only
      static const bool wg_override = std::getenv("D4EST_HIP_FACE_WG_PER_CU") != nullptr;   // environment knobs are read once
      const bool mfma = fam == FaceFamily::ConfFastMfma;
      const int wg_per_cu = wg_override ? face_wg_per_cu() : (mfma ? 8 : 4);
      debug_occupancy_once();
      if (mfma) run_trace_mfma(plan, u, trace, n, elist, wg_per_cu);
      else run_trace_wave(plan, fh, u, trace, n, wg_per_cu);
      break;
    }
    case FaceFamily::FamilySplit:
      if (run_trace_families(plan, fh, u, trace, elist)) break;
      if (fh.max_N > 16 || fh.max_NQ > 16) D4EST_HIP_ABORT("launch_traces: family split on a plan beyond the tiled kernels (N, NQ <= 16)");
      [[fallthrough]];
    case FaceFamily::Tiled: run_trace_mfma16(plan, fh, u, trace, n, elist); break;
    case FaceFamily::Generic: run_trace_generic(plan, fh, u, trace, n); break;
  }
  HIP_CHECK(hipGetLastError());
}

// true when launch_flux runs the kernel that can carry the Chebyshev update in its epilogue
static bool flux_can_fuse(d4est_hip_plan* plan, FaceFamily fam) {
  return plan->has_faces && plan->n_elements > 0 && !hybrid_active(plan) && flux_family_fuses(fam);
}
bool flux_can_fuse_update(d4est_hip_plan* plan) { return flux_can_fuse(plan, face_family(plan, face_host(plan))); }

// p <= 7, 6 waves, persistent grid of face_wg_per_cu() workgroups per CU.  INPLACE = false: a Schwarz subdomain plan (see the kernel)
template <bool FUSE, bool INPLACE>
static void run_flux_wave(d4est_hip_plan* plan, const FaceHost& fh, const double* trace, const double* ghost_trace, double* Au, int n,
                          const int* elist, const ChebyFuse& cf) {
  const int grid = persistent_grid(n, face_wg_per_cu() * face_cus(plan));
  hipLaunchKernelGGL((flux_wave_kernel<FUSE, INPLACE>), dim3(grid), dim3(384), 0, plan->stream, trace, ghost_trace, Au,
                     (const SideDesc*)plan->d_side_desc, (const ElemDesc*)plan->d_elem_desc, plan->d_face_ops, plan->d_face_geom, plan->d_bndry,
                     robin_c_of(fh), robin_r_of(fh), n, xcd_chunk(elist, n, grid), cf, elist);
}
static void flux_wave(d4est_hip_plan* plan, const FaceHost& fh, const double* trace, const double* ghost_trace, double* Au, int n,
                      const int* elist, const ChebyFuse* cf, bool inplace = true) {
  if (cf && !inplace) run_flux_wave<true, false>(plan, fh, trace, ghost_trace, Au, n, elist, *cf);
  else if (cf) run_flux_wave<true, true>(plan, fh, trace, ghost_trace, Au, n, elist, *cf);
  else if (!inplace) run_flux_wave<false, false>(plan, fh, trace, ghost_trace, Au, n, elist, ChebyFuse{});
  else run_flux_wave<false, true>(plan, fh, trace, ghost_trace, Au, n, elist, ChebyFuse{});
}
// p = 8 .. 15, 8 workgroups per CU.  Inherited: the XCD-aware order only where the conforming tiled family calls it (xcd), not under the hp split
template <bool FUSE>
static void run_flux_mfma16(d4est_hip_plan* plan, const FaceHost& fh, const double* trace, const double* ghost_trace, double* Au, int n,
                            const int* elist, const ChebyFuse& cf, bool xcd) {
  const int grid = std::min(n, 8 * face_cus(plan));
  hipLaunchKernelGGL(flux_mfma16_kernel<FUSE>, dim3(grid), dim3(192), 0, plan->stream, trace, ghost_trace, Au, (const SideDesc*)plan->d_side_desc,
                     (const ElemDesc*)fh.d_elem_desc_generic, plan->d_face_ops, plan->d_face_geom, plan->d_bndry, robin_c_of(fh), robin_r_of(fh), n,
                     xcd ? xcd_chunk(elist, n, grid) : 0, cf, elist);
}
static void flux_mfma16(d4est_hip_plan* plan, const FaceHost& fh, const double* trace, const double* ghost_trace, double* Au, int n,
                        const int* elist, const ChebyFuse* cf, bool xcd) {
  if (cf) run_flux_mfma16<true>(plan, fh, trace, ghost_trace, Au, n, elist, *cf, xcd);
  else run_flux_mfma16<false>(plan, fh, trace, ghost_trace, Au, n, elist, ChebyFuse{}, xcd);
}
// (cf: the Chebyshev update in both families' epilogues -- every element is on exactly one of the two lists)
static bool flux_families(d4est_hip_plan* plan, const FaceHost& fh, const double* trace, const double* ghost_trace, double* Au,
                          const int* elist, const ChebyFuse* cf) {
  const FamilyLists l = family_lists(fh, elist, /*ring=*/false);
  if (!l.on) return false;
  if (l.n_small > 0) flux_wave(plan, fh, trace, ghost_trace, Au, l.n_small, l.small, cf);
  if (l.n_big > 0) flux_mfma16(plan, fh, trace, ghost_trace, Au, l.n_big, l.big, cf, false);
  return true;
}
// the hanging sides of the hp split, by units: 8 workgroups per CU of the N <= 8 instance, 2 of the N <= 16 one
template <bool FUSE>
static void run_flux_unit(d4est_hip_plan* plan, const FaceHost& fh, const double* trace, const double* ghost_trace, double* Au, const ChebyFuse& cf) {
  auto go = [&](auto kern, int per_cu) {
    hipLaunchKernelGGL(kern, dim3(std::min(fh.hang_elems.n, per_cu * face_cus(plan))), dim3(256), 0, plan->stream, trace, ghost_trace, Au, fh.d_rec,
                       fh.d_units, fh.d_unit_first, (const ElemDesc*)fh.d_elem_desc_generic, plan->d_face_ops, fh.d_hp_ops, plan->d_face_geom,
                       plan->d_bndry, robin_c_of(fh), robin_r_of(fh), fh.hang_elems.n, cf);
  };
  if (fh.hp_max_N <= 8) go(flux_unit_kernel<FUSE, 8>, 8);
  else go(flux_unit_kernel<FUSE, 16>, 2);
}
// tiled record kernel, 8 workgroups per CU; hang_only as in run_trace_hp_mfma16
static void run_flux_hp_mfma16(d4est_hip_plan* plan, const FaceHost& fh, const double* trace, const double* ghost_trace, double* Au, int n,
                               const int* elist, int hang_only) {
  hipLaunchKernelGGL(flux_hp_mfma16_kernel, dim3(std::min(n, 8 * face_cus(plan))), dim3(192), 0, plan->stream, trace, ghost_trace, Au, fh.d_rec,
                     fh.d_side_first, (const ElemDesc*)fh.d_elem_desc_generic, plan->d_face_ops, fh.d_hp_ops, plan->d_face_geom, plan->d_bndry,
                     robin_c_of(fh), robin_r_of(fh), n, elist, hang_only);
}
static void run_flux_hp_generic(d4est_hip_plan* plan, const FaceHost& fh, const double* trace, const double* ghost_trace, double* Au, int n) {
  const size_t lds = fh.hp_lds_doubles * sizeof(double);
  set_lds_limit(flux_hp_kernel, lds);
  hipLaunchKernelGGL(flux_hp_kernel, dim3(std::min(n, 16384)), dim3(256), lds, plan->stream, trace, ghost_trace, Au, fh.d_rec, fh.d_elem_first,
                     (const ElemDesc*)fh.d_elem_desc_generic, plan->d_face_ops, fh.d_hp_ops, plan->d_face_geom, plan->d_bndry, robin_c_of(fh),
                     robin_r_of(fh), n, fh.hp_fld_stride);
}
static void run_flux_generic(d4est_hip_plan* plan, const FaceHost& fh, const double* trace, const double* ghost_trace, double* Au, int n) {
  const size_t lds = generic_lds_bytes(plan);
  set_lds_limit(flux_generic_kernel, lds);
  hipLaunchKernelGGL(flux_generic_kernel, dim3(std::min(n, 16384)), dim3(256), lds, plan->stream, trace, ghost_trace, Au,
                     (const SideDesc*)plan->d_side_desc, (const ElemDesc*)fh.d_elem_desc_generic, plan->d_face_ops, plan->d_face_geom, plan->d_bndry,
                     robin_c_of(fh), robin_r_of(fh), n, fh.fld_stride);
}

void launch_flux(d4est_hip_plan* plan, const double* trace, const double* ghost_trace, double* Au, const ChebyFuse* cf, const int* elist,
                 int n_list, int parts) {
  FaceHost& fh = face_host(plan);
  const FaceFamily fam = face_family(plan, fh);
  if (cf && !(flux_can_fuse(plan, fam) || (elist && hybrid_active(plan) && !fh.hp))) D4EST_HIP_ABORT("launch_flux: fused update requested on a plan whose flux kernel cannot carry it");
  if (!plan->has_faces || !plan->has_face_geometry) D4EST_HIP_ABORT("apply flux: plan_set_faces / plan_set_mortar_geometry were not called");
  if (plan->n_elements == 0) return;
  if (fh.n_ghost_sides > 0 && !ghost_trace) D4EST_HIP_ABORT("apply flux: plan has %d ghost sides but no ghost trace buffer was given", fh.n_ghost_sides);
  const int n = elist ? n_list : plan->n_elements;
  if (parts != 3 && !family_hp_split(fam)) D4EST_HIP_ABORT("launch_flux: parts = %d on a plan without the hp split", parts);
  if (n == 0 && !(family_hp_split(fam) && (parts & 2))) return;
  // (a fused update on a list: the hybrid operator's dirty elements only -- cf->u_out set, see apply_operator)
  if (elist && cf && !(elist == fh.hy_dirty_any && cf->u_out)) D4EST_HIP_ABORT("launch_flux: a fused update cannot ride on this element list");
  if (elist && !flux_takes_list(fam)) D4EST_HIP_ABORT("launch_flux: no list form of this plan's flux kernels (the hybrid operator is not set up for such plans)");
  switch (fam) {
    case FaceFamily::HpSplitFast:
    case FaceFamily::HpSplitTiled:
      // (see launch_traces) the conforming sides' terms from the conforming kernels, then the hanging sides' from the record kernel
      if (n > 0 && (parts & 1)) {
        if (fam == FaceFamily::HpSplitFast) flux_wave(plan, fh, trace, ghost_trace, Au, n, elist, nullptr);
        else if (!flux_families(plan, fh, trace, ghost_trace, Au, elist, nullptr)) flux_mfma16(plan, fh, trace, ghost_trace, Au, n, elist, nullptr, false);
      }
      if ((parts & 2) && fh.n_units > 0) run_flux_unit<false>(plan, fh, trace, ghost_trace, Au, ChebyFuse{});
      else if ((parts & 2) && fh.hang_elems.n > 0) run_flux_hp_mfma16(plan, fh, trace, ghost_trace, Au, fh.hang_elems.n, fh.hang_elems.d, 1);
      break;
    case FaceFamily::HpTiled: run_flux_hp_mfma16(plan, fh, trace, ghost_trace, Au, n, elist, 0); break;
    case FaceFamily::HpGeneric: run_flux_hp_generic(plan, fh, trace, ghost_trace, Au, n); break;
    case FaceFamily::ConfFastMfma:
    case FaceFamily::ConfFastWave:
      flux_wave(plan, fh, trace, ghost_trace, Au, n, elist, cf, /*inplace=*/plan->tuning[D4EST_HIP_TUNE_GHOST_ALIAS] <= 0);
      break;
    case FaceFamily::FamilySplit:
      if (flux_families(plan, fh, trace, ghost_trace, Au, elist, cf)) break;
      if (fh.max_N > 16 || fh.max_NQ > 16) D4EST_HIP_ABORT("launch_flux: family split on a plan beyond the tiled kernels (N, NQ <= 16)");
      [[fallthrough]];
    case FaceFamily::Tiled: flux_mfma16(plan, fh, trace, ghost_trace, Au, n, elist, cf, true); break;
    case FaceFamily::Generic: run_flux_generic(plan, fh, trace, ghost_trace, Au, n); break;
  }
  HIP_CHECK(hipGetLastError());
}

void launch_flux_units(d4est_hip_plan* plan, const double* trace, const double* ghost_trace, double* Au, const ChebyFuse* cf) {
  FaceHost& fh = face_host(plan);
  if (!(fh.hp && fh.hp_split)) D4EST_HIP_ABORT("launch_flux_units: the plan has no hp split");
  if (!cf) { launch_flux(plan, trace, ghost_trace, Au, nullptr, nullptr, 0, 2); return; }
  if (fh.hang_elems.n == 0) return;
  if (fh.n_units == 0) D4EST_HIP_ABORT("launch_flux_units: a fused update needs the unit form of the record kernels");
  if (!cf->u_out || cf->u_out == cf->u) D4EST_HIP_ABORT("launch_flux_units: the fused update needs a second vector");
  run_flux_unit<true>(plan, fh, trace, ghost_trace, Au, *cf);
  HIP_CHECK(hipGetLastError());
}
bool faces_hp(d4est_hip_plan* plan) { return face_host(plan).hp; }
bool faces_hp_split(d4est_hip_plan* plan) {
  FaceHost& fh = face_host(plan);
  return fh.hp && fh.hp_split;
}
bool faces_have_units(d4est_hip_plan* plan) {
  FaceHost& fh = face_host(plan);
  return fh.hp && fh.hp_split && (fh.hang_elems.n == 0 || fh.n_units > 0);
}

// a volume vector's values at the Lobatto face nodes of every boundary side, in the layout of the Dirichlet data (side_bndry_stride)
__global__ __launch_bounds__(64) void bndry_gather_kernel(const double* __restrict__ vol, double* __restrict__ out, const int* __restrict__ is_bndry,
                                                          const int* __restrict__ side_bndry_stride, const ElemDesc* __restrict__ ed, int n_sides) {
  for (int s = blockIdx.x; s < n_sides; s += gridDim.x) {
    if (!is_bndry[s]) continue;
    const ElemDesc el = ed[s / 6];
    const int N = el.N, f = s % 6;
    for (int k = threadIdx.x; k < N * N; k += blockDim.x) out[side_bndry_stride[s] + k] = vol[el.ns + face_vol_index(f, N, k % N, k / N)];
  }
}

void launch_boundary_gather(d4est_hip_plan* plan, const double* vol, double* out) {
  FaceHost& fh = face_host(plan);
  const int n_sides = 6 * plan->n_elements;
  if (n_sides == 0 || plan->total_bndry_nodes == 0) return;
  if (!fh.d_is_bndry) {
    std::vector<int> b(n_sides);
    for (int s_ = 0; s_ < n_sides; ++s_) b[s_] = fh.sd_host[s_].kind == 0;   // (boundary sides; hanging sides are kind 3)
    fh.d_is_bndry = fh.upload(b);
  }
  hipLaunchKernelGGL(bndry_gather_kernel, dim3(std::min(n_sides, 8192)), dim3(64), 0, plan->stream, vol, out, fh.d_is_bndry,
                     fh.d_side_bndry_stride, (const ElemDesc*)fh.d_elem_desc_generic, n_sides);
  HIP_CHECK(hipGetLastError());
}

void launch_traces_all(d4est_hip_plan* plan, const double* u, double* trace) {
  FaceHost& fh = face_host(plan);
  const int n = plan->n_elements;
  if (n == 0) return;
  if (fh.hp) run_trace_hp_generic(plan, fh, u, trace, n);
  else run_trace_generic(plan, fh, u, trace, n);
  HIP_CHECK(hipGetLastError());
}

}  // namespace d4est_hip
