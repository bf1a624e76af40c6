// Geometry and boundary data of the face part: the setters that fill the plan's combined mortar factors (from host- or device-supplied
// reference-layout arrays, from the brick map, from an analytic tree map) and the Dirichlet and Robin data -- with the small set-up
// kernels they launch.  The descriptors and mortar records they read are built by d4est_hip_faces_setup.hip.
#include <algorithm>

#include "d4est_hip_faces_host.h"
#include "d4est_hip_maps.h"
#include "d4est_hip_penalty.h"
#include "d4est_hip_tables.h"

namespace d4est_hip {

// Dirichlet data: Lobatto face nodes -> mortar quadrature nodes (d4est_laplacian_flux_sipg.c:80-107), set-up time
__global__ __launch_bounds__(64) void bndry_interp_kernel(const double* __restrict__ g_lobatto, double* __restrict__ g_quad,
                                                          const SideDesc* __restrict__ sd, const ElemDesc* __restrict__ ed,
                                                          const int* __restrict__ side_bndry_stride,
                                                          const double* __restrict__ face_ops, int n_sides) {
  for (int s = blockIdx.x; s < n_sides; s += gridDim.x) {
    const SideDesc d = sd[s];
    if (d.kind != 0) continue;
    const int N = ed[s / 6].N, NQ = d.NQ;
    const double* C = face_ops + d.offC;
    const double* g = g_lobatto + side_bndry_stride[s];
    for (int k = threadIdx.x; k < NQ * NQ; k += blockDim.x) {
      const int ap = k % NQ, bp = k / NQ;
      double v = 0.0;
      for (int b = 0; b < N; ++b) {
        double r = 0.0;
        for (int a = 0; a < N; ++a) r = fma(C[ap * N + a], g[a + N * b], r);
        v = fma(C[bp * N + b], r, v);
      }
      g_quad[d.geom + k] = v;
    }
  }
}

// ---------------------------------------------------------------------------
// set-up: 7 combined geometric factors per mortar quadrature node
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void face_geom_kernel(const SideDesc* __restrict__ sd, const int* __restrict__ side_deg_m,
                                                       const int* __restrict__ side_deg_p, int n_sides,
                                                       const double* __restrict__ sj, const double* __restrict__ nrm,
                                                       const double* __restrict__ drst_m, const double* __restrict__ drst_p,
                                                       const double* __restrict__ hm, const double* __restrict__ hp,
                                                       double prefactor, int fcn, double* __restrict__ geom) {
  for (int s = blockIdx.x; s < n_sides; s += gridDim.x) {
    const SideDesc d = sd[s];
    const int NQ = d.NQ, T = NQ * NQ;
    const size_t S = (size_t)d.geom;
    for (int k = threadIdx.x; k < T; k += blockDim.x) {
      const int a = k % NQ, b = k / NQ;
      const int kp = (d.kind == 0) ? k : reorder_index(d.code, NQ - 1, a, b);
      const double sjk = sj[S + k];
      double sn[3];
      for (int x = 0; x < 3; ++x) sn[x] = sjk * nrm[3 * S + (size_t)x * T + k];
      for (int i = 0; i < 3; ++i) {
        double am = 0.0, ap = 0.0;
        for (int x = 0; x < 3; ++x) {
          am += sn[x] * drst_m[9 * S + (size_t)(i + 3 * x) * T + k];
          if (d.kind != 0) ap += sn[x] * drst_p[9 * S + (size_t)(i + 3 * x) * T + kp];
        }
        geom[7 * S + (size_t)i * T + k] = am;
        geom[7 * S + (size_t)(3 + i) * T + k] = ap;
      }
      const int dm = side_deg_m[s], dp = (d.kind == 0) ? dm : side_deg_p[s];
      const double hpk = (d.kind == 0) ? hm[S + k] : hp[S + k];
      geom[7 * S + (size_t)6 * T + k] = sjk * sipg_penalty(fcn, dm, hm[S + k], dp, hpk, prefactor);
    }
  }
}

__global__ __launch_bounds__(64) void face_geom_hp_kernel(const HpMortar* __restrict__ md, const HpGeomSrc* __restrict__ gs, int n_rec,
                                                          const double* __restrict__ sj, const double* __restrict__ nrm,
                                                          const double* __restrict__ drst_m, const double* __restrict__ drst_p,
                                                          const double* __restrict__ hm, const double* __restrict__ hp,
                                                          double prefactor, int fcn, double* __restrict__ geom) {
  for (int r = blockIdx.x; r < n_rec; r += gridDim.x) {
    const HpMortar m = md[r];
    const HpGeomSrc g = gs[r];
    const int NQ = m.NQ, T = NQ * NQ;
    const size_t S = (size_t)g.S, TT = (size_t)g.Ttot;
    for (int k = threadIdx.x; k < T; k += blockDim.x) {
      const int a = k % NQ, b = k / NQ;
      const int kp = (m.kind == 0) ? k : reorder_index(m.code, NQ - 1, a, b);
      const double sjk = sj[S + g.off + k];
      double sn[3];
      for (int x = 0; x < 3; ++x) sn[x] = sjk * nrm[3 * S + (size_t)x * TT + g.off + k];
      for (int i = 0; i < 3; ++i) {
        double am = 0.0, ap = 0.0;
        for (int x = 0; x < 3; ++x) {
          am += sn[x] * drst_m[9 * S + (size_t)(i + 3 * x) * TT + g.off + k];
          // (+) side factors are stored in the (+) side's sub-mortar order and orientation (d4est_laplacian_flux.c:858-900)
          if (m.kind != 0) ap += sn[x] * drst_p[9 * S + (size_t)(i + 3 * x) * TT + g.off_p + kp];
        }
        // the hanging-face factors of the reference (d4est_laplacian_flux.c:907-915: x 0.5 on the big element's gradient and term 2 on
        // its half-size mortars, x 0.5 on the big element's gradient seen from a small side) are folded in here -- exact scalings --,
        // so that a record's SIPG terms read like a conforming side's and a small side can go to the conforming flux kernel (hp split)
        geom[7 * (size_t)m.gidx + (size_t)i * T + k] = m.fm * am;
        geom[7 * (size_t)m.gidx + (size_t)(3 + i) * T + k] = m.fp * ap;
      }
      const double hmk = hm[S + g.off + k], hpk = (m.kind == 0) ? hmk : hp[S + g.off + k];
      geom[7 * (size_t)m.gidx + (size_t)6 * T + k] = sjk * sipg_penalty(fcn, g.deg_m, hmk, (m.kind == 0) ? g.deg_m : g.deg_p, hpk, prefactor);
    }
  }
}

void faces_set_geometry(d4est_hip_plan* plan, const double* sj, const double* n, const double* drst_m, const double* drst_p,
                        const double* hm, const double* hp, int on_device) {
  FaceHost& fh = face_host(plan);
  const size_t T = (size_t)plan->total_mortar_nodes;
  const double* src[6] = {sj, n, drst_m, drst_p, hm, hp};
  const size_t mult[6] = {1, 3, 9, 9, 1, 1};
  double* tmp[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  const double* dev[6];
  for (int i = 0; i < 6; ++i) {
    if (!src[i]) D4EST_HIP_ABORT("plan_set_mortar_geometry: NULL array %d", i);
    if (on_device) {
      dev[i] = src[i];
    } else {
      HIP_CHECK(hipMalloc(&tmp[i], std::max<size_t>(mult[i] * T, 1) * sizeof(double)));
      HIP_CHECK(hipMemcpy(tmp[i], src[i], mult[i] * T * sizeof(double), hipMemcpyHostToDevice));
      dev[i] = tmp[i];
    }
  }
  const int n_sides = 6 * plan->n_elements;
  if (fh.hp) {
    if (fh.n_rec > 0)
      hipLaunchKernelGGL(face_geom_hp_kernel, dim3(std::min(fh.n_rec, 8192)), dim3(64), 0, plan->stream, fh.d_rec, fh.d_gsrc, fh.n_rec,
                         dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], plan->sipg_prefactor, plan->sipg_penalty_fcn, plan->d_face_geom);
    HIP_CHECK(hipGetLastError());
  } else if (n_sides > 0) {
    const int grid = n_sides < 8192 ? n_sides : 8192;
    hipLaunchKernelGGL(face_geom_kernel, dim3(grid), dim3(64), 0, plan->stream, (const SideDesc*)plan->d_side_desc,
                       fh.d_side_deg_m, fh.d_side_deg_p, n_sides, dev[0], dev[1], dev[2], dev[3], dev[4], dev[5],
                       plan->sipg_prefactor, plan->sipg_penalty_fcn, plan->d_face_geom);
    HIP_CHECK(hipGetLastError());
  }
  // raw sj is kept for Robin boundary data (faces_set_robin)
  if (!fh.d_sj) fh.d_sj = fh.alloc<double>(T);
  if (T > 0) HIP_CHECK(hipMemcpyAsync(fh.d_sj, dev[0], T * sizeof(double), hipMemcpyDeviceToDevice, plan->stream));
  // the estimator's factors (d4est_hip_plan_set_estimator): only on plans that asked for them
  if (plan->est_requested) estimator_setup(plan, dev[0], dev[1], dev[2], dev[3], dev[4], dev[5]);
  // the IP energy norm's face factor (d4est_hip_plan_set_energy_norm): likewise
  if (plan->norm_requested) norms_setup(plan, dev[0], dev[1], dev[4], dev[5]);
  HIP_CHECK(hipStreamSynchronize(plan->stream));
  for (int i = 0; i < 6; ++i)
    if (tmp[i]) HIP_CHECK(hipFree(tmp[i]));
  plan->has_face_geometry = true;
}

void faces_set_dirichlet(d4est_hip_plan* plan, const double* g_lobatto, int on_device) {
  FaceHost& fh = face_host(plan);
  const size_t tm = std::max<size_t>((size_t)plan->total_mortar_nodes, 1);
  fh.dirichlet_nonzero = (g_lobatto != nullptr);
  plan->bc_inhomogeneous = fh.dirichlet_nonzero || fh.robin;
  if (!g_lobatto) {
    HIP_CHECK(hipMemsetAsync(plan->d_bndry, 0, tm * sizeof(double), plan->stream));
    return;
  }
  const size_t nb = (size_t)plan->total_bndry_nodes;
  if (nb == 0) return;
  const double* dev = g_lobatto;
  double* tmp = nullptr;
  if (!on_device) {
    HIP_CHECK(hipMalloc(&tmp, nb * sizeof(double)));
    HIP_CHECK(hipMemcpy(tmp, g_lobatto, nb * sizeof(double), hipMemcpyHostToDevice));
    dev = tmp;
  }
  const int n_sides = 6 * plan->n_elements;
  hipLaunchKernelGGL(bndry_interp_kernel, dim3(std::min(n_sides, 8192)), dim3(64), 0, plan->stream, dev, plan->d_bndry,
                     (const SideDesc*)plan->d_side_desc, (const ElemDesc*)plan->d_elem_desc, fh.d_side_bndry_stride,
                     plan->d_face_ops, n_sides);
  HIP_CHECK(hipGetLastError());
  if (tmp) {
    HIP_CHECK(hipStreamSynchronize(plan->stream));
    HIP_CHECK(hipFree(tmp));
  }
}

// brick geometry on the mortars (d4est_mesh_compute_mortar_quadrature_quantities on the brick map): constant per mortar;
// the mortar is the face of a cell of the MORTAR's size (half the element on the big side of a hanging face)
__device__ inline void brick_fill_mortar(int f, double hx, double hy, double hz, size_t S, int off, int TT, int T,
                                         double* sj, double* nrm, double* drst_m, double* drst_p, double* hm, double* hp) {
  const int dir = f >> 1;
  const double h[3] = {hx, hy, hz};
  const double J = hx * hy * hz;
  const double sjv = J * (1. / h[dir]);
  for (int k = threadIdx.x; k < T; k += blockDim.x) {
    sj[S + off + k] = sjv;
    hm[S + off + k] = J / sjv;
    hp[S + off + k] = J / sjv;
    for (int d = 0; d < 3; ++d) nrm[3 * S + (size_t)d * TT + off + k] = (d == dir) ? ((f & 1) ? 1. : -1.) : 0.;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        const double v = (i == j) ? 1. / h[i] : 0.;
        drst_m[9 * S + (size_t)(i + 3 * j) * TT + off + k] = v;
        drst_p[9 * S + (size_t)(i + 3 * j) * TT + off + k] = v;
      }
  }
}

__global__ __launch_bounds__(64) void brick_mortar_kernel(const SideDesc* __restrict__ sd, int n_sides, const int* __restrict__ elem_dq,
                                                          double root_len, double ex, double ey, double ez, double* sj, double* nrm,
                                                          double* drst_m, double* drst_p, double* hm, double* hp) {
  for (int s = blockIdx.x; s < n_sides; s += gridDim.x) {
    const SideDesc d = sd[s];
    if (d.kind == 3) continue;   // hanging side: written by the record kernel
    const double half = (double)elem_dq[s / 6] / root_len / 2.;
    const int T = d.NQ * d.NQ;
    brick_fill_mortar(s % 6, ex * half, ey * half, ez * half, (size_t)d.geom, 0, T, T, sj, nrm, drst_m, drst_p, hm, hp);
  }
}

__global__ __launch_bounds__(64) void brick_mortar_hp_kernel(const HpMortar* __restrict__ md, const HpGeomSrc* __restrict__ gs, int n_rec,
                                                             const int* __restrict__ elem_dq, double root_len, double ex, double ey,
                                                             double ez, double* sj, double* nrm, double* drst_m, double* drst_p,
                                                             double* hm, double* hp) {
  for (int r = blockIdx.x; r < n_rec; r += gridDim.x) {
    const HpMortar m = md[r];
    const HpGeomSrc g = gs[r];
    const double half = (double)elem_dq[m.elem] / root_len / 2. * (m.fm < 1.0 ? 0.5 : 1.0);   // big side: half-size mortar
    brick_fill_mortar(m.face, ex * half, ey * half, ez * half, (size_t)g.S, g.off, g.Ttot, m.NQ * m.NQ, sj, nrm, drst_m, drst_p, hm, hp);
  }
}

// The mortar faces of hm / hp with the elements whose size parameters d4est_mesh_calculate_mortar_h reads for them
// (src/Mesh/d4est_mesh.c:689-856 as called at :629-644 and :1071-1103): (-) elements on f_m, (+) elements in (-) order on f_p; on a
// hanging face the side of four gives each mortar face its own small element, the other side its one big element.
// dq: p4est side length of the local elements, then of the ghost elements.
static std::vector<MortarHUnit> mortar_h_units(d4est_hip_plan* plan, const std::vector<int>& dq, double root_len, const char* who) {
  FaceHost& fh = face_host(plan);
  const int ne = plan->n_elements, type = plan->face_h_type;
  if ((type == D4EST_HIP_FACE_H_EQ_FACE_DIAM || type == D4EST_HIP_FACE_H_EQ_TOTAL_VOLUME_DIV_TOTAL_AREA) && plan->n_ghost > 0)
    D4EST_HIP_ABORT("%s: face_h_type %d (%s) is not defined on a plan with ghost sides: the reference reads diam_face / area / volume without "
                    "the ghost offset there (src/Mesh/d4est_mesh.c:801-802, :841)", who, type,
                    type == D4EST_HIP_FACE_H_EQ_FACE_DIAM ? "FACE_H_EQ_FACE_DIAM" : "FACE_H_EQ_TOTAL_VOLUME_DIV_TOTAL_AREA");
  auto idx = [&](int ref) {
    if (ref == -1) D4EST_HIP_ABORT("%s: boundary reference on an interior side", who);
    const int i = ref >= 0 ? ref : ne - (ref + 2);
    if (i >= (int)dq.size()) D4EST_HIP_ABORT("%s: ghost element %d has no cell description", who, i - ne);
    return i;
  };
  std::vector<MortarHUnit> units;
  auto add = [&](int at, int T, int e, int f, int hang, size_t s, int i) {
    MortarHUnit u{};
    u.at = at; u.T = T;
    u.one_m = e; u.f_m = f; u.n_m = 1; u.em[0] = e;
    if (plan->side_nbr[s] == -1) {   // boundary: one h (:629-644)
      u.one_p = e; u.f_p = f; u.n_p = 1; u.ep[0] = e;
    } else {
      u.f_p = plan->side_nbr_face[s];
      if (hang == 0) {
        u.one_p = idx(plan->side_nbr[s]); u.n_p = 1; u.ep[0] = u.one_p;
      } else if (hang == 1) {        // (+) side: the four small elements in (-) order
        u.n_p = 4;
        for (int k = 0; k < 4; ++k) u.ep[k] = idx(plan->side_nbr4[4 * s + k]);
        u.one_p = u.ep[i];
      } else {                       // this element is one of the four (-) elements; (+) side: the big element
        u.n_m = 4;
        for (int k = 0; k < 4; ++k) u.em[k] = idx(plan->side_nbr4[4 * s + k]);
        u.one_p = idx(plan->side_nbr[s]); u.n_p = 1; u.ep[0] = u.one_p;
      }
    }
    u.tree_h_m = (double)dq[u.one_m] / root_len;
    u.tree_h_p = (double)dq[u.one_p] / root_len;
    units.push_back(u);
  };
  if (fh.hp) {
    std::vector<HpMortar> rec((size_t)fh.n_rec);
    std::vector<HpGeomSrc> gs((size_t)fh.n_rec);
    if (fh.n_rec > 0) {
      HIP_CHECK(hipMemcpy(rec.data(), fh.d_rec, rec.size() * sizeof(HpMortar), hipMemcpyDeviceToHost));
      HIP_CHECK(hipMemcpy(gs.data(), fh.d_gsrc, gs.size() * sizeof(HpGeomSrc), hipMemcpyDeviceToHost));
    }
    for (int e = 0; e < ne; ++e)
      for (int f = 0; f < 6; ++f) {
        const size_t s = 6 * (size_t)e + f;
        for (int r = plan->side_first_rec[s]; r < plan->side_first_rec[s + 1]; ++r)
          add(gs[r].S + gs[r].off, rec[r].NQ * rec[r].NQ, e, f, plan->side_hang[s], s, r - plan->side_first_rec[s]);
      }
  } else {
    std::vector<SideDesc> sd(6 * (size_t)ne);
    if (!sd.empty()) HIP_CHECK(hipMemcpy(sd.data(), plan->d_side_desc, sd.size() * sizeof(SideDesc), hipMemcpyDeviceToHost));
    for (size_t s = 0; s < sd.size(); ++s) add(sd[s].geom, sd[s].NQ * sd[s].NQ, (int)(s / 6), (int)(s % 6), 0, s, 0);
  }
  return units;
}

void faces_set_geometry_brick(d4est_hip_plan* plan, const int* d_elem_dq, const int* h_elem_dq, double root_len, const double* extents) {
  FaceHost& fh = face_host(plan);
  const size_t T = std::max<size_t>((size_t)plan->total_mortar_nodes, 1);
  double* a[6];
  const size_t mult[6] = {1, 3, 9, 9, 1, 1};
  for (int i = 0; i < 6; ++i) {
    HIP_CHECK(hipMalloc(&a[i], mult[i] * T * sizeof(double)));
    HIP_CHECK(hipMemsetAsync(a[i], 0, mult[i] * T * sizeof(double), plan->stream));
  }
  const double ex = extents[1] - extents[0], ey = extents[3] - extents[2], ez = extents[5] - extents[4];
  const int n_sides = 6 * plan->n_elements;
  if (fh.hp) {
    if (fh.n_rec > 0)
      hipLaunchKernelGGL(brick_mortar_hp_kernel, dim3(std::min(fh.n_rec, 8192)), dim3(64), 0, plan->stream, fh.d_rec, fh.d_gsrc, fh.n_rec,
                         d_elem_dq, root_len, ex, ey, ez, a[0], a[1], a[2], a[3], a[4], a[5]);
  } else if (n_sides > 0) {
    hipLaunchKernelGGL(brick_mortar_kernel, dim3(std::min(n_sides, 8192)), dim3(64), 0, plan->stream, (const SideDesc*)plan->d_side_desc,
                       n_sides, d_elem_dq, root_len, ex, ey, ez, a[0], a[1], a[2], a[3], a[4], a[5]);
  }
  HIP_CHECK(hipGetLastError());
  if (plan->face_h_type != D4EST_HIP_FACE_H_EQ_J_DIV_SJ_QUAD) {
    // a ghost element's size follows from the side that refers to it (2:1 balance): the same, half (the small elements of a big
    // side) or twice (the big element of a small side) the local element's
    const int ne = plan->n_elements, ng = plan->n_ghost;
    std::vector<int> dq(h_elem_dq, h_elem_dq + ne);
    dq.resize((size_t)ne + ng, ne > 0 ? h_elem_dq[0] : 1);
    auto set = [&](int ref, int v) { if (ref <= -2 && -(ref + 2) < ng) dq[(size_t)ne - (ref + 2)] = v; };
    for (size_t s = 0; s < 6 * (size_t)ne; ++s) {
      const int hang = plan->side_hang.empty() ? 0 : plan->side_hang[s], own = h_elem_dq[s / 6];
      set(plan->side_nbr[s], hang == 2 ? 2 * own : hang == 1 ? own / 2 : own);
      if (hang != 0)
        for (int k = 0; k < 4; ++k) set(plan->side_nbr4[4 * s + k], hang == 1 ? own / 2 : own);
    }
    std::vector<CellDesc> cells(dq.size());
    for (size_t i = 0; i < dq.size(); ++i) cells[i] = CellDesc{0, {0, 0, 0}, dq[i], 0};
    const std::vector<MortarHUnit> units = mortar_h_units(plan, dq, root_len, "plan_set_mortar_geometry_brick");
    if (plan->face_h_type != D4EST_HIP_FACE_H_EQ_TREE_H) sizes_compute(plan, nullptr, extents, cells, ng, root_len);
    sizes_fill_mortar_h(plan, units, a[4], a[5]);
  }
  faces_set_geometry(plan, a[0], a[1], a[2], a[3], a[4], a[5], /*on_device=*/1);
  for (int i = 0; i < 6; ++i) HIP_CHECK(hipFree(a[i]));
}

// ---------------------------------------------------------------------------
// Mortar factors of an analytic tree map on the device (d4est_mesh_compute_mortar_quadrature_quantities with
// DX_compute_method = GEOM_COMPUTE_ANALYTIC, src/Mesh/d4est_mesh.c:858-1108, src/Mesh/d4est_mortars.c:19-190): one unit per
// conforming side / per mortar record.  The (-) cell gives sj, n (COMPUTE_NORMAL_USING_JACOBIAN), dr/dx and hm = J/sj at the
// mortar's quadrature nodes in (-) order; the (+) cell -- evaluated in ITS tree, at ITS nodes -- gives drst_dxyz_p_porder in the
// (+) side's own node and sub-face order and, re-oriented into (-) order, hp.  On the big side of a hanging face the cells are
// the half-size virtual children of the element (d4est_mortars_compute_qcoords_on_mortar, :419-468).  The arrays are written in
// the reference's layout and handed to the same pre-combination as host-supplied factors.
// ---------------------------------------------------------------------------
struct MortarUnit {
  int S, off, off_p, Ttot, NQ, code, boundary, pad;
  CellDesc m, p;
};

__device__ inline void face_ref_point(int f, double ta, double tb, double r[3]) {
  const int dir = f >> 1;
  r[dir] = (f & 1) ? 1.0 : -1.0;
  r[dir == 0 ? 1 : 0] = ta;
  r[dir == 2 ? 1 : 2] = tb;
}

__global__ __launch_bounds__(64) void analytic_mortar_kernel(const MortarUnit* __restrict__ units, int n_units, TreeMapParams P,
                                                             double root_len, const double* __restrict__ quad_nodes /* [NQ][24] */,
                                                             double* sj, double* nrm, double* drst_m, double* drst_p, double* hm, double* hp) {
  for (int ui = blockIdx.x; ui < n_units; ui += gridDim.x) {
    const MortarUnit un = units[ui];
    const int NQ = un.NQ, T = NQ * NQ;
    const double* t = quad_nodes + 24 * NQ;
    const size_t S = (size_t)un.S;
    for (int k = threadIdx.x; k < T; k += blockDim.x) {
      const int a = k % NQ, b = k / NQ;
      double r[3], dxdr[3][3], inv[3][3];
      face_ref_point(un.m.face, t[a], t[b], r);
      cell_dxdr(P, un.m, root_len, r, dxdr);
      const double J = invert3(dxdr, inv);
      const int dir = un.m.face >> 1;
      const double sgn = (un.m.face & 1) ? 1.0 : -1.0;
      double v[3], s2 = 0.0;
      for (int d = 0; d < 3; ++d) { v[d] = sgn * J * inv[dir][d]; s2 += v[d] * v[d]; }
      const double sjv = sqrt(s2);
      sj[S + un.off + k] = sjv;
      hm[S + un.off + k] = J / sjv;
      for (int d = 0; d < 3; ++d) nrm[3 * S + (size_t)d * un.Ttot + un.off + k] = v[d] / sjv;
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) drst_m[9 * S + (size_t)(i + 3 * j) * un.Ttot + un.off + k] = inv[i][j];
      if (un.boundary) {
        hp[S + un.off + k] = J / sjv;
        for (int i = 0; i < 3; ++i)
          for (int j = 0; j < 3; ++j) drst_p[9 * S + (size_t)(i + 3 * j) * un.Ttot + un.off_p + k] = inv[i][j];
        continue;
      }
      // (+) side, its own node k
      face_ref_point(un.p.face, t[a], t[b], r);
      cell_dxdr(P, un.p, root_len, r, dxdr);
      (void)invert3(dxdr, inv);
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) drst_p[9 * S + (size_t)(i + 3 * j) * un.Ttot + un.off_p + k] = inv[i][j];
      // hp at (-) node k = J/sj of the (+) side at its node reorder(k)
      const int kp = reorder_index(un.code, NQ - 1, a, b);
      face_ref_point(un.p.face, t[kp % NQ], t[kp / NQ], r);
      cell_dxdr(P, un.p, root_len, r, dxdr);
      const double Jp = invert3(dxdr, inv);
      const int dirp = un.p.face >> 1;
      double sp = 0.0;
      for (int d = 0; d < 3; ++d) sp += (Jp * inv[dirp][d]) * (Jp * inv[dirp][d]);
      hp[S + un.off + k] = Jp / sqrt(sp);
    }
  }
}

static CellDesc face_child(const CellDesc& c, int face, int child) {
  // half-size virtual child `child` (z-order on the face) of cell c that touches face `face`
  CellDesc r = c;
  const int dir = face >> 1, h = c.dq / 2;
  const int a0 = dir == 0 ? 1 : 0, a1 = dir == 2 ? 1 : 2;
  r.dq = h;
  r.q[a0] += (child & 1) * h;
  r.q[a1] += (child >> 1) * h;
  if (face & 1) r.q[dir] += h;
  r.face = face;
  return r;
}

void faces_set_geometry_analytic(d4est_hip_plan* plan, const TreeMapParams& P, const std::vector<CellDesc>& elem,
                                 const std::vector<CellDesc>& ghost, double root_len) {
  FaceHost& fh = face_host(plan);
  const int ne = plan->n_elements;
  auto cell_of = [&](int ref, int face) {
    if (ref == -1) D4EST_HIP_ABORT("plan_set_mortar_geometry_analytic: boundary reference");
    CellDesc c;
    if (ref >= 0) c = elem[ref];
    else {
      const int g = -(ref + 2);
      if (g >= (int)ghost.size()) D4EST_HIP_ABORT("plan_set_mortar_geometry_analytic: ghost element %d has no cell description", g);
      c = ghost[g];
    }
    c.face = face;
    return c;
  };
  std::vector<MortarUnit> units;
  if (fh.hp) {
    std::vector<HpMortar> rec((size_t)fh.n_rec);
    std::vector<HpGeomSrc> gs((size_t)fh.n_rec);
    HIP_CHECK(hipMemcpy(rec.data(), fh.d_rec, rec.size() * sizeof(HpMortar), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(gs.data(), fh.d_gsrc, gs.size() * sizeof(HpGeomSrc), hipMemcpyDeviceToHost));
    for (int e = 0; e < ne; ++e)
      for (int f = 0; f < 6; ++f) {
        const size_t s = 6 * (size_t)e + f;
        const int hang = plan->side_hang[s], nbr = plan->side_nbr[s], f_p = plan->side_nbr_face[s], o = plan->side_orientation[s];
        const int r0 = plan->side_first_rec[s], r1 = plan->side_first_rec[s + 1];
        for (int r = r0; r < r1; ++r) {
          MortarUnit u{};
          u.S = gs[r].S; u.off = gs[r].off; u.off_p = gs[r].off_p; u.Ttot = gs[r].Ttot; u.NQ = rec[r].NQ; u.code = rec[r].code;
          u.boundary = (rec[r].kind == 0);
          if (hang == 0) {
            u.m = cell_of(e, f);
            u.p = u.boundary ? u.m : cell_of(nbr, f_p);
          } else if (hang == 1) {
            const int i = r - r0;
            u.m = face_child(cell_of(e, f), f, i);
            u.p = cell_of(plan->side_nbr4[4 * s + i], f_p);
          } else {
            const int c = plan->side_sub[s];
            u.m = cell_of(e, f);
            u.p = face_child(cell_of(nbr, f_p), f_p, reorient_face_order(f, f_p, o, c));
          }
          units.push_back(u);
        }
      }
  } else {
    std::vector<SideDesc> sd(6 * (size_t)ne);
    if (!sd.empty()) HIP_CHECK(hipMemcpy(sd.data(), plan->d_side_desc, sd.size() * sizeof(SideDesc), hipMemcpyDeviceToHost));
    for (size_t s = 0; s < sd.size(); ++s) {
      MortarUnit u{};
      const int T = sd[s].NQ * sd[s].NQ;
      u.S = sd[s].geom; u.off = 0; u.off_p = 0; u.Ttot = T; u.NQ = sd[s].NQ; u.code = sd[s].code; u.boundary = (sd[s].kind == 0);
      u.m = cell_of((int)(s / 6), (int)(s % 6));
      u.p = u.boundary ? u.m : cell_of(plan->side_nbr[s], plan->side_nbr_face[s]);
      units.push_back(u);
    }
  }
  // quadrature nodes of every mortar degree in use
  std::vector<double> qn((size_t)25 * 24, 0.0);
  for (const MortarUnit& u : units) {
    if (u.NQ > 24) D4EST_HIP_ABORT("plan_set_mortar_geometry_analytic: mortar degree %d", u.NQ - 1);
    if (qn[(size_t)24 * u.NQ + u.NQ - 1] == 0.0 || u.NQ == 1) {
      std::vector<double> x, w;
      if (plan->quad_type == QUAD_LEGENDRE) Tables1D::gauss(u.NQ - 1, x, w);
      else Tables1D::lobatto(u.NQ - 1, x, w);
      for (int i = 0; i < u.NQ; ++i) qn[(size_t)24 * u.NQ + i] = x[i];
    }
  }
  const size_t T = std::max<size_t>((size_t)plan->total_mortar_nodes, 1);
  double* a[6];
  const size_t mult[6] = {1, 3, 9, 9, 1, 1};
  for (int i = 0; i < 6; ++i) {
    HIP_CHECK(hipMalloc(&a[i], mult[i] * T * sizeof(double)));
    HIP_CHECK(hipMemsetAsync(a[i], 0, mult[i] * T * sizeof(double), plan->stream));
  }
  MortarUnit* d_units = upload_vec(units);
  double* d_qn = upload_vec(qn);
  if (!units.empty())
    hipLaunchKernelGGL(analytic_mortar_kernel, dim3(std::min((int)units.size(), 8192)), dim3(64), 0, plan->stream, d_units, (int)units.size(), P,
                       root_len, d_qn, a[0], a[1], a[2], a[3], a[4], a[5]);
  HIP_CHECK(hipGetLastError());
  if (plan->face_h_type != D4EST_HIP_FACE_H_EQ_J_DIV_SJ_QUAD) {
    std::vector<CellDesc> cells(elem);
    cells.insert(cells.end(), ghost.begin(), ghost.end());
    std::vector<int> dq(cells.size());
    for (size_t i = 0; i < cells.size(); ++i) dq[i] = cells[i].dq;
    const std::vector<MortarHUnit> hunits = mortar_h_units(plan, dq, root_len, "plan_set_mortar_geometry_analytic");
    if (plan->face_h_type != D4EST_HIP_FACE_H_EQ_TREE_H) sizes_compute(plan, &P, nullptr, cells, (int)ghost.size(), root_len);
    sizes_fill_mortar_h(plan, hunits, a[4], a[5]);
  }
  faces_set_geometry(plan, a[0], a[1], a[2], a[3], a[4], a[5], /*on_device=*/1);
  for (int i = 0; i < 6; ++i) HIP_CHECK(hipFree(a[i]));
  HIP_CHECK(hipFree(d_units));
  HIP_CHECK(hipFree(d_qn));
}

__global__ __launch_bounds__(256) void robin_setup_kernel(const double* __restrict__ sj, const double* __restrict__ coeff,
                                                          const double* __restrict__ rhs, double* __restrict__ c,
                                                          double* __restrict__ r, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    c[i] = sj[i] * coeff[i];
    r[i] = sj[i] * rhs[i];
  }
}

// Robin boundary data at the mortar quadrature nodes of the boundary sides (indexed like sj: side stride S + k).
// coeff_quad == NULL switches the boundary sides back to Dirichlet.
void faces_set_robin(d4est_hip_plan* plan, const double* coeff_quad, const double* rhs_quad, int on_device) {
  FaceHost& fh = face_host(plan);
  if (!plan->has_face_geometry) D4EST_HIP_ABORT("plan_set_robin_values: call d4est_hip_plan_set_mortar_geometry first (needs sj)");
  if (!coeff_quad) {
    fh.robin = false;
    plan->bc_inhomogeneous = fh.dirichlet_nonzero;   // back to Dirichlet: the values set earlier are still in d_bndry
    return;
  }
  if (!rhs_quad) D4EST_HIP_ABORT("plan_set_robin_values: rhs_quad is NULL");
  const size_t tm = (size_t)plan->total_mortar_nodes;
  if (!fh.d_robin_c) {
    fh.d_robin_c = fh.alloc<double>(tm);
    fh.d_robin_r = fh.alloc<double>(tm);
  }
  fh.robin = true;
  plan->bc_inhomogeneous = true;
  if (tm == 0) return;
  const double* dc = coeff_quad;
  const double* dr = rhs_quad;
  double *tc = nullptr, *tr = nullptr;
  if (!on_device) {
    HIP_CHECK(hipMalloc(&tc, tm * sizeof(double)));
    HIP_CHECK(hipMalloc(&tr, tm * sizeof(double)));
    HIP_CHECK(hipMemcpy(tc, coeff_quad, tm * sizeof(double), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(tr, rhs_quad, tm * sizeof(double), hipMemcpyHostToDevice));
    dc = tc;
    dr = tr;
  }
  hipLaunchKernelGGL(robin_setup_kernel, dim3(1024), dim3(256), 0, plan->stream, fh.d_sj, dc, dr, fh.d_robin_c, fh.d_robin_r, tm);
  HIP_CHECK(hipGetLastError());
  if (tc) {
    HIP_CHECK(hipStreamSynchronize(plan->stream));
    HIP_CHECK(hipFree(tc));
    HIP_CHECK(hipFree(tr));
  }
}

const double* faces_sj(d4est_hip_plan* plan, const char* who) {
  if (!plan->has_face_geometry) D4EST_HIP_ABORT("%s: call d4est_hip_plan_set_mortar_geometry first (needs sj)", who);
  return face_host(plan).d_sj;
}

void faces_robin_arrays(d4est_hip_plan* plan, const char* who, double** robin_c, double** robin_r) {
  if (!plan->has_face_geometry) D4EST_HIP_ABORT("%s: call d4est_hip_plan_set_mortar_geometry first (needs sj)", who);
  FaceHost& fh = face_host(plan);
  const size_t tm = (size_t)plan->total_mortar_nodes;
  if (!fh.d_robin_c) {
    fh.d_robin_c = fh.alloc<double>(tm);
    fh.d_robin_r = fh.alloc<double>(tm);
  }
  fh.robin = true;
  plan->bc_inhomogeneous = true;
  *robin_c = fh.d_robin_c;
  *robin_r = fh.d_robin_r;
}

}  // namespace d4est_hip
