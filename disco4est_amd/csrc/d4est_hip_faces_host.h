// Private to the three face units: what the face set-up (d4est_hip_faces_setup.hip) uploads and what the geometry setters
// (d4est_hip_faces_geometry.hip) and the trace / flux kernels and their launchers (d4est_hip_faces.hip) read -- the device-visible
// descriptor structs and FaceHost, the set-up's host-side findings per plan.
#pragma once
#include <algorithm>
#include <map>
#include <vector>

#include "d4est_hip_internal.h"
#include "d4est_hip_wave.h"

namespace d4est_hip {

struct SideDesc {
  int kind;           // 0 boundary, 1 interface with local (+), 2 interface with ghost (+)
  int code;           // flip0 | flip1<<1 | transpose<<2   (dGMath/d4est_operators.c:2031-2081)
  int NQ;             // mortar quadrature nodes/dir
  int offC;           // (NQ x N)  side nodes -> mortar quadrature nodes (p-prolong then Lobatto->quadrature)
  int offCD;          // (NQ x N)  C * D: tangential derivative fused with the interpolation (fast trace kernel)
  int pad0;
  int offE;           // (N x NQ)  mortar quadrature -> side operator (P^T I^T W)
  int geom;           // scalar stride S of the side (face_geom at 7*S; Dirichlet data at S)
  long long qoff;     // offset of this side's mortar-node trace block (4 T doubles) in the local buffer
  long long nbr_qoff; // offset of the (+) side's block (local buffer for kind 1, ghost buffer for kind 2)
};

struct ElemDesc {
  int N;     // nodes per direction
  int ns;    // nodal stride
  int offD;  // offset of the zero-padded 8 x 8 (fast path) or N x N (generic) derivative matrix inside face_ops
  int pad;
};

// uniform plans (one degree, one mortar degree, contiguous strides): the trace kernel computes its addresses instead of loading
// descriptors, which removes one dependent global-load latency from every workgroup (the kernel is latency bound)
struct TraceUniform {
  int N, NQ, offC, offCD, offD, ns0, ns_stride, pad;  // N == 0: not uniform
  long long q0, q_stride;                              // qoff of side s = q0 + s * q_stride
};

struct GhostSideDesc {
  int N;       // nodes/dir of the ghost element
  int f;       // its face
  int NQ;
  int offC;    // (NQ x N)
  int offD;    // N x N
  int pad;
  long long u_off;  // offset of the ghost element in the packed ghost vector
  long long goff;   // offset of the block in the ghost trace buffer
};

// volume index of face node (a,b) of face f (a fastest; tangential axes in increasing order)
__device__ inline int face_vol_index(int f, int N, int a, int b) {
  const int dir = f >> 1, fix = face_fix(f, N);
  if (dir == 0) return fix + N * (a + N * b);
  if (dir == 1) return a + N * (fix + N * b);
  return a + N * (b + N * fix);
}

// the mortar records of a mesh with hanging faces (the record path: see d4est_hip_faces.hip)
struct HpMortar {
  int elem, face;
  int kind;          // 0 boundary, 1 interface with a local (+) element, 2 with a ghost (+) element
  int code;          // reorder code applied when reading the (+) block
  int N, NQ;         // side nodes / mortar quadrature nodes per direction
  int offCa, offCb;  // (NQ x N) side -> mortar quadrature nodes along the face axes a, b (hp_ops)
  int offCDa, offCDb; // C . D: tangential derivative fused with the interpolation (MFMA kernels)
  int offEa, offEb;  // (N x NQ) mortar quadrature nodes -> side
  int first, last;   // first / last record of its side
  int gidx;          // scalar index of the mortar's first node in the precombined geometry / boundary arrays (S + off)
  int u_shift;       // offset (doubles) from the (+) block to the block whose u field this mortar reads; 0 except on a small side whose
                     // face pair the reference re-orients non-geometrically (see faces_setup_hp)
  double fm, fp, w2; // hanging-face factors (set-up only: face_geom_hp_kernel folds them into the geometric factors; w2 = fm)
  double hang;       // side_hang of the record's side as a number (0 conforming, 1 big, 2 small): lets the tiled kernels serve the hanging sides only (hp split)
  long long qoff, nbr_qoff;
};

struct HpGeomSrc {   // where the record's factors sit in the reference-layout arrays (set-up only)
  int S, off, Ttot, off_p;
  int deg_m, deg_p, pad0, pad1;
};

// one side of a listed element that stays with the mortar records (trace_unit_kernel / flux_unit_kernel)
struct HangUnit { int e, f, r0, nrec; };

template <typename T>
T* upload_vec(const std::vector<T>& v) {
  T* d = nullptr;
  HIP_CHECK(hipMalloc(&d, std::max<size_t>(v.size(), 1) * sizeof(T)));
  if (!v.empty()) HIP_CHECK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return d;
}

// a device list of element numbers and its length
struct ElemList {
  int* d = nullptr;
  int n = 0;
};

struct FaceHost {
  TraceUniform uni{};            // N == 0: descriptors are loaded
  // hanging-mesh (mortar record) path
  bool hp = false;
  int n_rec = 0;
  HpMortar* d_rec = nullptr;
  HpGeomSrc* d_gsrc = nullptr;
  int* d_elem_first = nullptr;
  int* d_side_first = nullptr;   // first record of side s (6 n_elements + 1 entries)
  int hp_max_N = 1, hp_max_NQ = 1;
  // hp split (deg, deg_quad <= 7): the fast conforming kernels serve every conforming (and small hanging) side of the mesh, the mortar-record
  // kernels only the hanging sides of the elements that have one (hang_elems)
  bool hp_split = false;
  bool hp_split_fast = false;    // ... and every degree <= 7: the p <= 7 kernels take every conforming side; else the tiled 16 x 16 kernels (or both
                                 // families on lists: family_split) do
  ElemList hang_elems;
  HangUnit* d_units = nullptr;   // the sides of the listed elements that stay with the records, element by element (trace_unit_kernel / flux_unit_kernel)
  int* d_unit_first = nullptr;   // per listed element: its first unit (hang_elems.n + 1 entries)
  int n_units = 0;
  std::vector<HpMortar> rec_host;   // host copy of the records (set-up of the split)
  std::vector<HpGeomSrc> gsrc_host;  // host copy of the records' factor sources (set-up of the estimator)
  int* d_is_bndry = nullptr;         // 1 per boundary side (launch_boundary_gather; uploaded on first use)
  std::vector<SideDesc> sd_host;     // host copy of the side descriptors as faces_setup built them, before the hp split (the same)
  double* d_hp_ops = nullptr;
  int hp_fld_stride = 0;
  size_t hp_lds_doubles = 0;
  double* d_sj = nullptr;       // raw sj (for Robin data)
  double* d_robin_c = nullptr;  // sj * coeff, sj * rhs at the mortar nodes of the boundary sides
  double* d_robin_r = nullptr;
  bool robin = false;
  bool dirichlet_nonzero = false;   // non-zero Dirichlet data sits in d_bndry (it survives a Robin on / off cycle)
  std::vector<int> side_deg_m, side_deg_p;
  int* d_side_deg_m = nullptr;
  int* d_side_deg_p = nullptr;
  int* d_side_bndry_stride = nullptr;
  GhostSideDesc* d_ghost_sides = nullptr;
  int n_ghost_sides = 0;
  int fld_stride = 0;   // generic kernels: doubles per field buffer
  int max_N = 1, max_NQ = 1;
  int max_local_N = 1;   // largest deg + 1 among the plan's own elements (sizes the LDS copy of u in trace_mfma16_kernel)
  ElemDesc* d_elem_desc_generic = nullptr;  // offD -> unpadded N x N matrices
  // family split (conforming mixed-degree plans with degrees above 7): the elements whose own degree and six mortars all fit 8 x 8 go
  // through the p <= 7 kernels (trace_mfma_kernel / flux_wave_kernel, 2 - 3 x faster per element than the tiled 16 x 16 kernels), the
  // rest through the tiled ones; both families write the same trace array and add into the same A u
  bool family_split = false;
  ElemList fam_small, fam_big;
  // ... and the hybrid operator's ring / dirty lists of such a plan, split the same way (the list launches of the two families; without them
  // a listed launch sends every listed element through the tiled kernels: level 5, graded p = 3 ... 9, ring traces 396 us)
  const int *hy_ring = nullptr, *hy_dirty = nullptr;   // the hybrid operator's device lists these belong to (matched by pointer)
  const int* hy_dirty_any = nullptr;                   // the hybrid operator's dirty list, family split or not (a fused update may ride on it)
  ElemList ring_small, ring_big, dirty_small, dirty_big;

  // Every device array above comes from alloc() / upload() and is freed by release(): a new array needs no line of its own there.
  // No destructor: the map of these is a static, and a plan still alive at process exit leaks quietly -- no hipFree during static destruction.
  std::vector<void*> owned;
  template <typename T>
  T* alloc(size_t n) {
    T* d = nullptr;
    HIP_CHECK(hipMalloc(&d, std::max<size_t>(n, 1) * sizeof(T)));
    owned.push_back(d);
    return d;
  }
  template <typename T>
  T* upload(const std::vector<T>& v) {
    T* d = upload_vec(v);
    owned.push_back(d);
    return d;
  }
  ElemList upload_list(const std::vector<int>& v) { return ElemList{upload(v), (int)v.size()}; }
  void release() {
    for (void* d : owned) (void)hipFree(d);
    owned.clear();
  }
};

// the plan's entry (created empty on first use); d4est_hip_faces_setup.hip keeps the map and faces_destroy erases the entry
FaceHost& face_host(d4est_hip_plan* plan);

}  // namespace d4est_hip
