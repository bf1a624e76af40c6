// Internal declarations shared by the HIP translation units of libd4est_hip.so.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "../../include/d4est_hip.h"

#define D4EST_HIP_ABORT(...)                                   \
  do {                                                         \
    std::fprintf(stderr, "[D4EST_HIP_ABORT] ");                \
    std::fprintf(stderr, __VA_ARGS__);                         \
    std::fprintf(stderr, " (%s:%d)\n", __FILE__, __LINE__);    \
    std::abort();                                              \
  } while (0)

#define HIP_CHECK(expr)                                                              \
  do {                                                                               \
    hipError_t _e = (expr);                                                          \
    if (_e != hipSuccess) D4EST_HIP_ABORT("%s failed: %s", #expr, hipGetErrorString(_e)); \
  } while (0)

namespace d4est_hip {

// One (deg, deg_quad) bucket of elements; launches are per bucket so N and NQ are
// compile-time constants inside the kernels.
struct Bucket {
  int deg = 0, deg_quad = 0;
  int N = 0, NQ = 0;
  int n_elem = 0;
  int elem_offset = 0;      // offset into Plan::d_elem_ids / d_ns_list / d_qs_list
  // device 1-D tables (row-major)
  double* d_B = nullptr;    // NQ x N  interpolation Lobatto -> quadrature nodes
  double* d_G = nullptr;    // NQ x N  G = B * D  (derivative evaluated at quadrature nodes)
  double* d_D = nullptr;    // N x N   collocation derivative
  double* d_w = nullptr;    // NQ      quadrature weights
  double* d_BT = nullptr;   // N x NQ  transposes (row i = column i of the operator: one scalar load feeds NQ FMA chains)
  double* d_GT = nullptr;
  double* d_DT = nullptr;
  // square N x N tables for the nodal mass applies (d4est_operators.c:891-928) and the Gauss inverse mass
  // (d4est_quadrature.c:1222-1331; only when deg_quad == deg, else null)
  // affine strides of the bucket-ordered element list (ns = ns0 + i*ns_stride); ns_stride < 0: not affine, use the lists
  int ns0 = 0, ns_stride = -1, qs0 = 0, qs_stride = -1;
  bool affine = false;  // every element has a node-independent J (dr/dx)(dr/dx)^T (detected in plan_set_geometry)
  // even-odd tables (see stiffness_wave_eo_kernel), only when N and NQ are even: forward B, G (N/2 rows of NQ) and
  // backward B^T, G^T (NQ/2 rows of N)
  double* d_EBf = nullptr;
  double* d_EGf = nullptr;
  double* d_EBb = nullptr;
  double* d_EGb = nullptr;
  // N = NQ only: even-odd tables of the differentiation matrix ON the quadrature nodes and of its transpose (collocated-gradient form)
  double* d_EDq = nullptr;
  double* d_EDqT = nullptr;
  double* d_M = nullptr;
  double* d_MT = nullptr;
  double* d_Minv = nullptr;
  double* d_MinvT = nullptr;
  double* d_Binv = nullptr;   // (lobatto_to_gauss_interp)^-1
  double* d_BinvT = nullptr;  // its transpose = (lobatto_to_gauss_interp_trans)^-1
  double* d_wGL = nullptr;    // Gauss weights
};

}  // namespace d4est_hip

struct d4est_hip_plan {
  int n_elements = 0;
  int local_nodes = 0;
  int local_nodes_quad = 0;
  int quad_type = 0;
  hipStream_t stream = nullptr;
  int n_cus = 0;  // multiProcessorCount of the device the plan was created on
  char last_kernel[128] = "";  // name of the stiffness kernel selected by the last apply (largest bucket last)

  std::vector<int> deg, deg_quad, nodal_stride, quad_stride;  // host copies
  std::vector<d4est_hip::Bucket> buckets;

  std::vector<int> elem_ids;      // element ids sorted by bucket (host)
  int* d_elem_ids = nullptr;      // same on the device
  int* d_ns_list = nullptr;       // nodal_stride in bucket order (one load, wave-uniform when 1 element/wave)
  int* d_qs_list = nullptr;       // quad_stride in bucket order

  bool has_geometry = false;
  double* d_J = nullptr;          // local_nodes_quad  (reference layout)
  int* d_face_stride = nullptr;       // per element: offset of its N^2 face values in a face vector (apply_slicer / apply_lift)
  int face_nodes = 0;
  double* d_metric = nullptr;
  double* d_metric_affine = nullptr;  // 6 per element (bucket order): J (dr/dx)(dr/dx)^T of node 0
  int* d_nonaffine = nullptr;         // per bucket: set by the precombine kernel when an element is not affine     // 6 * local_nodes_quad, element-blocked: [e][c][n], c in (rr,rs,rt,ss,st,tt)

  // ---- faces (set-up: d4est_hip_faces_setup.hip; kernels and launchers: d4est_hip_faces.hip) ----
  bool has_faces = false, has_face_geometry = false;
  int n_ghost = 0;
  std::vector<int> ghost_deg, ghost_deg_quad;
  std::vector<int> side_nbr, side_nbr_face, side_reorder, side_mortar_stride, side_bndry_stride;  // host copies, 6*n_elements
  std::vector<int> side_hang, side_sub, side_nbr4, side_orientation;  // hanging faces (d4est_hip_plan_set_hanging); empty = conforming
  int total_mortar_nodes = 0, total_bndry_nodes = 0;
  long long local_trace_doubles = 0, ghost_trace_doubles = 0;
  int* d_side_desc = nullptr;        // SideDesc per side (see d4est_hip_faces_host.h)
  void* d_elem_desc = nullptr;       // ElemDesc per element
  // per mortar record (hanging plans; empty on conforming plans where a side has exactly one block)
  std::vector<long long> rec_qoff, rec_goff;
  std::vector<int> rec_len, side_first_rec;
  std::vector<long long> trace_offset, ghost_trace_offset;  // per SIDE: offset of its 4 T mortar-node trace block (ghost: -1 if none)
  double* d_face_ops = nullptr;      // concatenated 1-D face operators (C and E matrices)
  double* d_face_geom = nullptr;     // 7 * total_mortar_nodes: am[3], ap[3], s3 per mortar quadrature node (side-blocked)
  double* d_bndry = nullptr;         // Dirichlet values on boundary Lobatto face nodes (total_bndry_nodes), zero by default
  double* d_trace = nullptr;         // plan-owned local trace buffer
  double sipg_prefactor = 10.0;
  int sipg_penalty_fcn = 0;
  int max_face_lds_doubles = 0;
  bool face_fast = false;  // all sides have N, Np, NQ <= 8: flux_wave_kernel applies
  void* direct = nullptr;  // DirectHost (d4est_hip_direct.hip): conforming uniform-degree plans, deg_quad <= 7
  void* hybrid = nullptr;  // HybridHost (d4est_hip_direct.hip): mixed-degree / locally refined plans -- clean elements through the direct kernels

  // ---- solver workspace / communication hooks (d4est_hip_solver.hip) ----
  double *d_work_p = nullptr, *d_work_d = nullptr, *d_work_r = nullptr, *d_reduce = nullptr, *d_ghost_trace = nullptr;
  const double* d_lhs_coeff = nullptr;   // optional zeroth-order term of apply_lhs: + V^T W J c V u (the caller's array; non-null = term on)
  double* d_lhs_c = nullptr;             // its values as they were at plan_set_lhs_coefficient (plan-owned copy)
  double* d_lhs_wjc = nullptr;           // w J c at the quadrature nodes (one stream for the operator kernels' volume stage)
  bool lhs_wjc_valid = false;
  double* d_work_m = nullptr;            // scratch of that term
  // the same term on a coarse multigrid level (d4est_hip_mgmatrix.hip): dense element blocks (the caller's array; non-null = this form
  // is on) with one offset per element, or the Galerkin chain through transfer objects up to a fine plan's coefficient
  const double* d_lhs_blocks = nullptr;
  long long* d_lhs_block_off = nullptr;
  void* lhs_chain = nullptr;             // d4est_hip::LhsChain
  hipStream_t side_stream = nullptr;  // the trace kernel (and the exchange) run here, concurrently with the volume kernel
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  // D4EST_HIP_TUNE_GRAPH: the last cheby_iterate call captured as a hipGraph (replayed while the arguments stay the same)
  hipGraphExec_t cheby_graph = nullptr;
  struct { const void *u, *rhs, *Au, *r; int iter, flag; double lmin, lmax; hipStream_t stream; } cheby_graph_key = {};
  d4est_hip_exchange_fn exchange_fn = nullptr;
  d4est_hip_allreduce_fn allreduce_fn = nullptr;
  void* comm_ctx = nullptr;

  // bumped by every call that can change what the operator computes (geometry, faces, SIPG parameters, boundary data, the zeroth-order
  // coefficient, tuning): objects that cache something derived from the operator (the Schwarz smoother's condensed blocks) compare it
  unsigned long long op_generation = 0;
  bool quad_aliased = false;      // some elements share a quadrature block (quad_stride repeats)
  int stream_mode = 0;            // 1: non-temporal metric / factor loads and A u stores (capi: update_stream_mode; kernels: with_ld)
  bool bc_inhomogeneous = false;   // non-zero Dirichlet data or Robin data is set (an affine, not linear, operator)

  int tuning[D4EST_HIP_TUNE_COUNT] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};  // -1 = auto  // see d4est_hip_plan_set_tuning

  // Krylov solvers (d4est_hip_krylov.hip): vectors, reduction partials, device scalars and the pinned stop flag, allocated on first use
  void* krylov = nullptr;   // d4est_hip::KrylovWork

  // generic-path scratch (allocated lazily)
  double* d_scratch = nullptr;
  size_t scratch_doubles = 0;

  // a-posteriori error estimator (d4est_hip_estimator.hip): requested by d4est_hip_plan_set_estimator before the mortar factors, whose
  // set-up then also forms the estimator's per-node factors (EstHost); plans without the request allocate nothing for it
  bool est_requested = false;
  int est_fcn[3] = {-1, -1, -1};   // gradu, u, u_dirichlet penalty ids (D4EST_HIP_EST_*)
  double est_prefactor = 0.0;
  void* est = nullptr;             // d4est_hip::EstHost

  // error norms (d4est_hip_norms.hip): the IP energy norm is requested by d4est_hip_plan_set_energy_norm before the mortar factors, whose
  // set-up then also forms its per-node face factor; the other norms allocate their scratch on first use (NormHost)
  bool norm_requested = false;
  int norm_fcn = -1;               // u_penalty_fcn: a SIPG penalty id (d4est_hip_plan_set_sipg)
  double norm_prefactor = 0.0;
  void* norms = nullptr;           // d4est_hip::NormHost

  // host-pointer entry points (d4est_hip_*_host): persistent pinned staging (3 vectors) and device mirrors u, rhs, Au, r,
  // allocated once on first use -- no per-call hipMalloc behind d4est's host double* API
  double* h_stage = nullptr;
  double* d_host[4] = {nullptr, nullptr, nullptr, nullptr};

  void* xyz = nullptr;   // d4est_hip::XyzHost (d4est_hip_volume.hip): what plan_compute_xyz_analytic keeps between calls

  // element size parameters (d4est_hip_sizes.hip): [mesh_parameters] face_h_type / volume_h_type (d4est_hip_plan_set_h_types; the defaults
  // are what the device mortar forms always wrote) and the plan-owned arrays of d4est_mesh_init_element_size_parameters
  int face_h_type = D4EST_HIP_FACE_H_EQ_J_DIV_SJ_QUAD;
  int volume_h_type = D4EST_HIP_VOL_H_EQ_DIAM;
  void* sizes = nullptr;           // d4est_hip::SizeHost

  // Hessian-trace coefficients (d4est_hip_hessian.hip): allocated by d4est_hip_plan_set_hessian_*; plans that never call them keep nullptr
  void* hess = nullptr;            // d4est_hip::HessHost

  // nonlinear power term f(x, u) = a (b + u)^k (d4est_hip_nonlinear.hip): allocated by d4est_hip_plan_set_nonlinear_power
  void* nonlin = nullptr;          // d4est_hip::NonlinHost
};

namespace d4est_hip {
// D4EST_HIP_TUNE_STIFFNESS_WAVE values that select the even-odd single-wavefront kernels (and the kernels built on their body): auto, 11,
// and 12 = the same kernels with the 16-product body where auto / 11 take the collocated-gradient body (deg_quad = deg)
inline bool tune_wave_eo(int tw) { return tw < 0 || tw == 11 || tw == 12; }

// Dynamic LDS beyond `threshold` (64 KB: what a kernel may use without asking): hipFuncSetAttribute(MaxDynamicSharedMemorySize), once per
// (device, kernel) and only ever raised.  The attribute belongs to the kernel on the current device, not to a plan; a driver call per
// launch would sit in the hot path of every smoother iteration, and inside hipGraph capture regions.
inline void raise_lds_limit(const void* fn, size_t bytes) {
  static std::mutex mu;
  static std::map<std::pair<int, const void*>, size_t> done;
  int device = 0;
  HIP_CHECK(hipGetDevice(&device));
  std::lock_guard<std::mutex> lock(mu);
  size_t& set = done[{device, fn}];
  if (set >= bytes) return;
  HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  set = bytes;
}
template <typename K>
inline void set_lds_limit(K kernel, size_t bytes, size_t threshold = 64 * 1024) {
  if (bytes > threshold) raise_lds_limit(reinterpret_cast<const void*>(kernel), bytes);
}

// Mixed-degree plans put several buckets into one launch; its argument struct M (WaveEoMulti, NonlinMulti) lists at most M::MAXB of the
// plan's first 32 buckets (one bit each in `covered`).  multi_append adds bucket i with its `workgroups` -- the fields every such kernel
// reads and the running workgroup prefix -- and returns false, nothing changed, where a limit is reached.
inline bool bucket_single_wave(const Bucket& bk) { return bk.n_elem > 0 && bk.N == bk.NQ && bk.N >= 2 && bk.N <= 8; }   // deg_quad = deg <= 7
template <class M>
inline bool multi_append(M& A, unsigned& covered, size_t i, const Bucket& bk, int workgroups) {
  if (A.n == M::MAXB || i >= 32) return false;
  const int j = A.n++;
  A.wg_end[j] = (j > 0 ? A.wg_end[j - 1] : 0) + workgroups;
  A.N[j] = bk.N; A.n_elem[j] = bk.n_elem; A.elem_offset[j] = bk.elem_offset;
  A.EBf[j] = bk.d_EBf; A.EBb[j] = bk.d_EBb; A.wq[j] = bk.d_w;
  covered |= 1u << i;
  return true;
}
template <class M>
inline int multi_workgroups(const M& A) { return A.n > 0 ? A.wg_end[A.n - 1] : 0; }
// ... and the per-bucket launches take the rest: f(bucket) for every non-empty bucket without a bit in `covered`
template <class F>
inline void for_each_uncovered_bucket(const d4est_hip_plan* plan, unsigned covered, F&& f) {
  for (size_t i = 0; i < plan->buckets.size(); ++i) {
    const Bucket& bk = plan->buckets[i];
    if (bk.n_elem > 0 && !(i < 32 && ((covered >> i) & 1u))) f(bk);
  }
}

// what every setter that changes the plan's state does first (drop_graph of d4est_hip_capi.hip, and the setters of the other units)
inline void plan_operator_changed(d4est_hip_plan* plan) {
  if (plan->cheby_graph) { (void)hipGraphExecDestroy(plan->cheby_graph); plan->cheby_graph = nullptr; }
  ++plan->op_generation;   // (every caller of this function changes the plan's state)
  // w J c of the fused operator kernels is derived from J and the coefficient: every setter that can change either comes through here
  // (plan_set_jacobian included), so the cached stream can never outlive its inputs
  plan->lhs_wjc_valid = false;
}

struct TreeMapParams;
struct CellDesc;
void launch_analytic_geometry(d4est_hip_plan* plan, const TreeMapParams& P, const CellDesc* d_cells, double root_len);
void faces_set_geometry_analytic(d4est_hip_plan* plan, const TreeMapParams& P, const std::vector<CellDesc>& elem,
                                 const std::vector<CellDesc>& ghost, double root_len);
// x | y | z of the analytic map at the Lobatto nodes and / or the quadrature nodes (either output may be null), on the plan's stream
void launch_analytic_xyz(d4est_hip_plan* plan, const TreeMapParams& P, const std::vector<CellDesc>& cells, double root_len,
                         double* xyz_lobatto, double* xyz_quad);
void analytic_xyz_destroy(d4est_hip_plan* plan);
// the staging half of launch_analytic_xyz, for the other units that evaluate a map at the plan's nodes (d4est_hip_problem.hip): the
// cell descriptions copied to the device on the plan's stream (through the plan's pinned buffer) and the cached 1-D node tables --
// bucket bi's Lobatto nodes at d_nodes + (2 bi) stride, its quadrature nodes (Gauss or Lobatto by quad_type) at d_nodes + (2 bi + 1) stride
struct NodeTables {
  const CellDesc* d_cells;
  const double* d_nodes;
  int stride;
};
NodeTables stage_cells_and_nodes(d4est_hip_plan* plan, const std::vector<CellDesc>& cells);

// d4est_hip_sizes.hip: element size parameters (d4est_mesh_init_element_size_parameters_local / _ghost) on the plan's stream.
// cells: the local elements followed by n_ghost ghost elements (n_ghost = 0: local elements only); brick != nullptr: the brick
// geometry with these extents (the cells' tree and q are not used), else the analytic map P
void sizes_compute(d4est_hip_plan* plan, const TreeMapParams* P, const double* brick_extents, const std::vector<CellDesc>& cells,
                   int n_ghost, double root_len);
void sizes_compute_diameters(d4est_hip_plan* plan, const double* xyz_lobatto);
// the plan-owned device array `which` (D4EST_HIP_SIZE_*) and its length; nullptr when it has not been computed
const double* sizes_array(const d4est_hip_plan* plan, int which, long long* count);
void sizes_destroy(d4est_hip_plan* plan);
// one mortar face of the reference-layout hm / hp arrays and the elements whose parameters d4est_mesh_calculate_mortar_h reads for it:
// index e for a local element, n_elements + g for ghost g.  one_m / one_p: the element whose parameter the mortar face takes (its own
// small element on a side of four, else the one element); em / ep: all elements of the side, which enter
// FACE_H_EQ_TOTAL_VOLUME_DIV_TOTAL_AREA.  A boundary side has (+) = (-).
struct MortarHUnit {
  int at, T;                     // hm[at .. at + T), hp likewise
  int one_m, f_m, n_m, em[4];
  int one_p, f_p, n_p, ep[4];
  double tree_h_m, tree_h_p;     // dq / root_len of one_m / one_p
};
// hm / hp of every unit by the plan's face_h_type (any but J_DIV_SJ_QUAD) from the size parameters, which must have been computed
void sizes_fill_mortar_h(d4est_hip_plan* plan, const std::vector<MortarHUnit>& units, double* hm, double* hp);

// d4est_hip_volume.hip
void launch_metric_precombine(d4est_hip_plan* plan, const double* d_J, const double* d_rst);
void launch_stiffness(d4est_hip_plan* plan, const double* u, double* Au);
void launch_stiffness_view(d4est_hip_plan* plan, const double* u, double* Au, int* ns_list_view, int* qs_list_view, const int* view_offset,
                           const int* view_count);
// mode: 0 mass, 1 galerkin, 2 interpolate / square tensor apply, 3 weighted mass, 4 inverse mass;
// which: 0 quadrature interpolation, 1 inverse Gauss interpolation, 2 M (1-D mass), 3 M^-1
void launch_mass_like(d4est_hip_plan* plan, int mode, const double* in, double* out, const double* coeff = nullptr, int which = 0);
void launch_brick_geometry(d4est_hip_plan* plan, const int* d_elem_dq, double root_len, const double* extents);
void launch_numerical_geometry(d4est_hip_plan* plan, const double* d_xyz);
void faces_set_geometry_brick(d4est_hip_plan* plan, const int* d_elem_dq, const int* h_elem_dq, double root_len, const double* extents);
void launch_slicer_lift(d4est_hip_plan* plan, const double* in, double* out, int face, int lift);
void launch_dij(d4est_hip_plan* plan, const double* in, double* out, int dir, int transpose);
void launch_dudr(d4est_hip_plan* plan, const double* u, double* d0, double* d1, double* d2);

// d4est_hip_faces_setup.hip: the host set-up of the face part (also faces_estimator_mortars and faces_destroy below)
void faces_setup(d4est_hip_plan* plan);
int reorient_face_order(int f_m, int f_p, int o, int i);  // dGMath/d4est_reference.c:84-110
int face_reorder_code(int f_m, int f_p, int o);            // dGMath/d4est_operators.c:2031-2050
// d4est_hip_faces_geometry.hip: mortar geometry and boundary data (also faces_set_geometry_brick / _analytic above)
void faces_set_geometry(d4est_hip_plan* plan, const double* sj, const double* n, const double* drst_m, const double* drst_p,
                        const double* hm, const double* hp, int on_device);
void faces_set_dirichlet(d4est_hip_plan* plan, const double* g_lobatto, int on_device);
void faces_set_robin(d4est_hip_plan* plan, const double* coeff_quad, const double* rhs_quad, int on_device);
// raw sj at the mortar nodes (side_mortar_stride[s] + k) and the plan's Robin arrays sj coeff / sj rhs, allocated if need be and switched
// on as faces_set_robin does -- the caller fills the boundary sides' entries on the plan's stream; both abort with `who` without sj
const double* faces_sj(d4est_hip_plan* plan, const char* who);
void faces_robin_arrays(d4est_hip_plan* plan, const char* who, double** robin_c, double** robin_r);
// d4est_hip_faces.hip: the trace / flux kernels and their launchers
// the plan's Robin arrays as the kernels take them: both nullptr while the boundary sides are Dirichlet
void faces_robin(d4est_hip_plan* plan, const double** robin_c, const double** robin_r);
void launch_traces(d4est_hip_plan* plan, const double* u, double* trace, bool ghost, const int* elist = nullptr, int n_list = 0, int parts = 3 /* see launch_flux */);
// Chebyshev update carried by the flux kernel's epilogue (flux_wave_kernel<true>): r = alpha (rhs - Au), p = r + beta p, u += p
struct ChebyFuse {
  const double* rhs = nullptr;
  double* p = nullptr;
  double* u = nullptr;
  double* u_out = nullptr;   // direct face kernel only: where the new iterate goes (it reads the neighbours' u)
  int skip_Au_store = 0;     // whole-operator kernel only: A u is consumed by the update and not stored (every iteration but the last)
  double* r = nullptr;
  double alpha = 0.0, beta = 0.0;
};
bool flux_can_fuse_update(d4est_hip_plan* plan);

// d4est_hip_direct.hip: the face terms straight from u (no trace arrays) on conforming uniform-degree plans
struct DirectFuse {   // Chebyshev update in the epilogue; the new iterate goes to u_out (the kernel reads the neighbours' u)
  const double* rhs = nullptr;
  double* p = nullptr;
  double* u_out = nullptr;
  double* r = nullptr;
  double alpha = 0.0, beta = 0.0;
  int skip_Au_store = 0;   // whole-operator form only: A u feeds the update in registers and is not written
  int pad = 0;
};
void direct_setup(d4est_hip_plan* plan, int N, int NQ, int ns0, int ns_stride, const double* C, const double* CD, const double* E);
void direct_destroy(d4est_hip_plan* plan);
bool direct_active(const d4est_hip_plan* plan);
double* direct_second_vector(d4est_hip_plan* plan);
// the direct kernel works on the listed elements only (the others are still read as neighbours); nullptr: every element.  The list
// (device ints) stays the caller's.  Only while direct_active(plan).
void direct_set_element_list(d4est_hip_plan* plan, const int* list_dev, int n_list);
bool direct_has_element_list(const d4est_hip_plan* plan);
bool direct_fused_ok(const d4est_hip_plan* plan);   // the volume term can ride in the same kernel (N = NQ in {6, 8}, one bucket ...)
// the elements with at least one ghost (+) side / with none (device lists; multi-rank plans: boundary traces feed the exchange,
// the interior elements' operator kernel runs while it is in flight)
void direct_ghost_split(d4est_hip_plan* plan, const int** bnd_list, int* n_bnd, const int** int_list, int* n_int);
// vol_term = 0: Au += face terms of u; 1: Au = (volume + face terms) of u; 2: ... with the zeroth-order term in the volume stage
void launch_direct_faces(d4est_hip_plan* plan, const double* u, const double* ghost_trace, double* Au, const DirectFuse* cf = nullptr,
                         int vol_term = 0);
// elist / n_list: only these elements' face terms (the hybrid operator's dirty elements); the hanging-side record kernels keep their own list
// parts (locally refined plans under the hp split): 1 the conforming kernel only, 2 the record kernel only, 3 both
void launch_flux(d4est_hip_plan* plan, const double* trace, const double* ghost_trace, double* Au, const ChebyFuse* cf = nullptr,
                 const int* elist = nullptr, int n_list = 0, int parts = 3);
// the hybrid operator (d4est_hip_direct.hip): clean elements (all six sides conforming against a local element of the same degree, or
// the boundary) through the one-kernel path of their degree bucket, the rest through the two-phase kernels on lists
bool hybrid_pair_built(int N, int NQ);
// hanging-aware form (locally refined plans under the hp split): what a clean element's hanging side is to the direct kernel --
// kind 3: served by the mortar-record kernels (no contribution); kind 2: a small side, (+) block at goff in the plan's trace array, own
// block exported to export_off, combined factors at geom; kind < 0: an ordinary side
// ghost-aware form (sharded plans, tuning key 14 = 2): kind 4 = a conforming side against a ghost element of the same degree -- (+) block at
// goff in the plan's GHOST trace buffer, no export, combined factors at geom
struct HybridSideOverride { int kind; long long goff; int export_off; int geom; };
void hybrid_setup(d4est_hip_plan* plan, const std::vector<char>& clean, const std::vector<const double*>& C, const std::vector<const double*>& CD,
                  const std::vector<const double*>& E, const std::vector<HybridSideOverride>* ov = nullptr, const char* form = "hanging-aware");
bool hybrid_hanging(const d4est_hip_plan* plan);   // the clean kernels read / write the trace array: record traces before, record flux after them
void hybrid_host_lists(const d4est_hip_plan* plan, const std::vector<int>** dirty, const std::vector<int>** ring);   // host copies of hybrid_lists
void hybrid_destroy(d4est_hip_plan* plan);
bool hybrid_active(const d4est_hip_plan* plan);
const char* hybrid_path(const d4est_hip_plan* plan);
void hybrid_lists(const d4est_hip_plan* plan, const int** dirty, int* n_dirty, const int** ring, int* n_ring);
// phase 0 fork + launches, 1 join; one bucket or a sharded plan: no fork, phase 1 launches on the plan's stream
void launch_hybrid_clean(d4est_hip_plan* plan, const double* u, const double* ghost_trace, double* Au, int phase, const DirectFuse* cf = nullptr);
bool hybrid_can_fuse_update(const d4est_hip_plan* plan);   // the Chebyshev update can ride in the hybrid operator's kernels (hanging-aware form, all clean)
double* hybrid_second_vector(d4est_hip_plan* plan);
// the record flux kernel of an hp-split plan alone, optionally with the Chebyshev update of the elements it serves in its epilogue
void launch_flux_units(d4est_hip_plan* plan, const double* trace, const double* ghost_trace, double* Au, const ChebyFuse* cf);
bool faces_have_units(d4est_hip_plan* plan);   // hp split with the unit record kernels (the form that can carry the update)
bool faces_hp(d4est_hip_plan* plan);         // the plan has hanging faces (mortar records)
bool faces_hp_split(d4est_hip_plan* plan);   // the plan has record kernels beside the conforming ones (launch_traces / launch_flux take `parts`)
void launch_hybrid_dirty_stiffness(d4est_hip_plan* plan, const double* u, double* Au);
// sharded plans: the plan has ghost sides (launch order around the exchange hooks: apply_operator); the clean elements beside a ghost side
// run after exchange phase 1, on the plan's stream (launch_hybrid_clean_ghost)
bool hybrid_sharded(const d4est_hip_plan* plan);
void launch_hybrid_clean_ghost(d4est_hip_plan* plan, const double* u, double* Au, const DirectFuse* cf = nullptr);
void faces_destroy(d4est_hip_plan* plan);
// the estimator's view of the plan's mortars (d4est_hip_faces_setup.hip builds it from its side descriptors / mortar records): one entry per
// conforming or boundary side, per sub-mortar of a big hanging side, per small hanging side; the entries of an element consecutive
struct EstMortar {
  int elem;
  int kind;          // 0 boundary, 1 interface with a local (+) element, 2 with a ghost (+) element
  int code;          // reorder code applied when reading the (+) block
  int NQ;            // mortar quadrature nodes per direction
  int gidx;          // scalar index of the mortar's first node (S + off): the estimator factors sit at 8 gidx
  int S, off, off_p, Ttot;   // where the reference-layout mortar factors of this mortar sit (set-up only)
  int deg_m, deg_p;  // prefactor degrees (d4est_estimator_bi.c:212-228)
  int N;             // boundary: nodes per direction of the element's face (Dirichlet data)
  int offC, ops_hp;  // boundary: (NQ x N) Lobatto face nodes -> mortar quadrature nodes, in face_ops (ops_hp = 0) or hp_ops (1)
  int bstride;       // boundary: side_bndry_stride of the side
  int u_shift;       // see HpMortar::u_shift
  double fm, fp;     // hanging-face factors on the (-) / (+) gradient (d4est_laplacian_flux.c:905-915)
  long long qoff, nbr_qoff;
};
void faces_estimator_mortars(d4est_hip_plan* plan, std::vector<EstMortar>& out, std::vector<int>& elem_first, const double** face_ops,
                             const double** hp_ops);
// every local side's (every mortar record's) trace block, whatever kernels the operator path uses
void launch_traces_all(d4est_hip_plan* plan, const double* u, double* trace);
// out[side_bndry_stride[s] + a + N b] = vol at face node (a, b) of every boundary side s (d4est_hip_plan_boundary_gather)
void launch_boundary_gather(d4est_hip_plan* plan, const double* vol, double* out);
// d4est_hip_estimator.hip
// the mortar records of faces_estimator_mortars and the per-element first-record table on the device, with the tensor quadrature
// weights of the plan's mortar degrees (row NQ - 1 of d_wt holds the NQ weights of degree NQ - 1, row length max_nq): what the set-up of
// the estimator and of the energy norm both start from.  The caller owns the three device arrays (d_wt is freed after its geometry kernel).
struct MortarRecords {
  EstMortar* d_mortars;
  int* d_elem_first;
  double* d_wt;
  int n_mortars, max_nq;
};
MortarRecords mortar_records_upload(d4est_hip_plan* plan, const char* who, const double** face_ops, const double** hp_ops);
void estimator_setup(d4est_hip_plan* plan, const double* sj, const double* n, const double* drst_m, const double* drst_p, const double* hm,
                     const double* hp);
void estimator_destroy(d4est_hip_plan* plan);
// pointwise: `residual` holds local_nodes_quad values at the quadrature nodes and term 0 is h^2 / p^2 sum_q w J r^2 (no interpolation)
void estimator_compute(d4est_hip_plan* plan, const double* u, const double* ghost_trace, const double* residual, const double* diam,
                       const double* g_lobatto, double* eta2, double* terms, bool pointwise = false);

// d4est_hip_hessian.hip: the coefficients of the Hessian trace on a plan and its apply
void hessian_set_brick(d4est_hip_plan* plan, const int* elem_dq, double root_len, const double* extents);
void hessian_set_analytic(d4est_hip_plan* plan, const TreeMapParams& P, const std::vector<CellDesc>& cells, double root_len);
void hessian_set_numerical(d4est_hip_plan* plan, const double* xyz_lobatto, const double* rst_xyz_quad, int on_device);
int hessian_info(const d4est_hip_plan* plan);
int hessian_supported(const d4est_hip_plan* plan);
void hessian_trace(d4est_hip_plan* plan, const double* u, double* del2u_quad);
void hessian_destroy(d4est_hip_plan* plan);

// d4est_hip_norms.hip
void norms_setup(d4est_hip_plan* plan, const double* sj, const double* n, const double* hm, const double* hp);
void norms_destroy(d4est_hip_plan* plan);
void norms_error(d4est_hip_plan* plan, const double* u, const double* u_compare, double* err);
void norms_l2_sqr(d4est_hip_plan* plan, const double* v, const int* skip, double* l2_array, double* sum);
void norms_linfty(d4est_hip_plan* plan, const double* v, const int* skip, double* max_out);
void norms_ip_energy_sqr(d4est_hip_plan* plan, const double* v, const double* ghost_trace, double* elem_terms, double* sums);
void norms_masked_sum(d4est_hip_plan* plan, const double* elem, const int* skip, double* sum);

// d4est_hip_solver.hip
// traces, volume term, (exchange), flux; lhs_term: also the optional zeroth-order term of plan_set_lhs_coefficient
void apply_operator(d4est_hip_plan* plan, const double* u, double* Au, const ChebyFuse* cf = nullptr, bool lhs_term = true);
void launch_residual(d4est_hip_plan* plan, int n, const double* rhs, const double* Au, double* r);   // r = rhs - Au
// grid of the 256-thread grid-stride vector kernels: one thread per entry up to 4096 workgroups
inline int grid_for(long long n) { return (int)std::max<long long>(1, std::min<long long>((n + 255) / 256, 4096)); }
void launch_add(d4est_hip_plan* plan, int n, const double* x, double* y);   // y += x (d4est_linalg_vec_axpy 1.0), on the plan's stream
void launch_residual_inplace(d4est_hip_plan* plan, int n, const double* rhs, double* r);              // r = rhs - r
void launch_residual_inplace_sub(d4est_hip_plan* plan, int n, const double* a, double* r);            // r = r - a
void ensure_solver_workspace(d4est_hip_plan* plan);
void add_lhs_mass_term(d4est_hip_plan* plan, const double* u, double* Au);   // Au += the plan's zeroth-order term, whichever form is set
// d4est_hip_mgmatrix.hip: the term as dense element blocks / as a Galerkin chain (multigrid matrix operator)
void add_lhs_blocks_term(d4est_hip_plan* plan, const double* u, double* Au);
void add_lhs_chain_term(d4est_hip_plan* plan, const double* u, double* Au);
void lhs_chain_destroy(d4est_hip_plan* plan);
// the term has a form that the fused operator kernels do not carry (blocks or chain): the volume kernel runs on its own and the term
// is added before the flux kernel
inline bool lhs_extra_term(const d4est_hip_plan* plan) { return plan->d_lhs_blocks != nullptr || plan->lhs_chain != nullptr; }
const double* ensure_lhs_wjc(d4est_hip_plan* plan);   // w J c at the quadrature nodes (formed on first use after the coefficient / geometry changed)
void launch_copy_blocks(hipStream_t stream, int n_blocks, const double* src, const long long* src_off, double* dst,
                        const long long* dst_off, const int* len);
void launch_dot(d4est_hip_plan* plan, int n, const double* x, const double* y, double* out_dev);
void launch_cheby_update(d4est_hip_plan* plan, int n, const double* rhs, const double* Au, double alpha, double beta, double* r,
                         double* p, double* u);
void cheby_iterate(d4est_hip_plan* plan, double* u, const double* rhs, double* Au, double* r, int iter, double lmin, double lmax,
                   int compute_residual_at_end);
double cg_eigs(d4est_hip_plan* plan, double* u, const double* rhs, double* Au, int imax, int use_new, double* hist_out);

// d4est_hip_krylov.hip
int cg_solve(d4est_hip_plan* plan, double* u, const double* rhs, double* Au, int imax, double atol, double rtol, double* hist_out);
int fcg_solve(d4est_hip_plan* plan, double* u, const double* rhs, double* Au, int imax, double atol, double rtol, d4est_hip_pc_fn pc,
              void* pc_ctx, double* hist_out);
void krylov_destroy(d4est_hip_plan* plan);

// d4est_hip_schwarz.hip: the smoother loop behind the V-cycle object's Smoother interface and the Schwarz preconditioner's loop (the
// handle's layout is private to that file).  check: 0 ok, 1 NULL, 2 the handle's mesh node count is not the plan's, 3 the subdomain plan
// is not on the plan's stream, 4 the plan has ghost sides (or no faces).  A handle with an element exchange (a sharded handle): 2 compares
// with its own node count and 4 only means "no faces".  Neither loop synchronises at the end of an iterate.
int schwarz_smoother_check(const d4est_hip_schwarz* sz, const d4est_hip_plan* mesh_plan);
bool schwarz_fused_residual(const d4est_hip_schwarz* sz);
d4est_hip_plan* schwarz_subdomain_plan(const d4est_hip_schwarz* sz);   // (d4est_hip_comm.hip orders its rounds on that plan's stream)
void schwarz_smoother_run(d4est_hip_schwarz* sz, d4est_hip_plan* mesh_plan, double* u, const double* rhs, double* r,
                          int smoother_iterations, int subdomain_iter, double subdomain_atol, double subdomain_rtol);
void schwarz_pc_run(d4est_hip_schwarz* sz, d4est_hip_plan* mesh_plan, const double* rhs, double* z, double* Au, double* residual,
                    int iterations, int subdomain_iter, double subdomain_atol, double subdomain_rtol);

// d4est_hip_nonlinear.hip
void nonlinear_destroy(d4est_hip_plan* plan);
// the plan-owned a (and, with_b, b; else b is dropped and *b = nullptr) of the power term with exponent k, allocated if need be: the
// state d4est_hip_plan_set_nonlinear_power leaves, for a caller that writes the values itself on the plan's stream
void nonlinear_term_arrays(d4est_hip_plan* plan, int k, bool with_b, double** a, double** b);
// the same for the REAL power term a |b + u|^s; either call clears the other form
void nonlinear_term_arrays_real(d4est_hip_plan* plan, double s, bool with_b, double** a, double** b);
// plan-owned temporaries of the composed load vector (d4est_hip_problem.hip), allocated on first use and freed with the plan:
// local_nodes_quad doubles (shared with the composed nonlinear term) and, with want_xyz, 3 local_nodes_quad more
void nonlinear_load_scratch(d4est_hip_plan* plan, bool want_xyz, double** f_quad, double** xyz_quad);

// d4est_hip_capi.hip (defined among its extern "C" entry points; not in the header: internal): {geom_type, params} of the analytic entry
// points -> TreeMapParams; aborts with `who` on a bad type, radius or flag
extern "C" void d4est_hipi_tree_map_params(int geom_type, const double* params, const char* who, TreeMapParams* out);


}  // namespace d4est_hip
