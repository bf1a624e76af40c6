// The Schwarz handle's layout, shared by d4est_hip_schwarz.hip (set-up, the CG subdomain solver, the exchanges) and
// d4est_hip_schwarz_gmres.hip (the GMRES subdomain solver).  Private to those two files.
#pragma once

#include <vector>

#include "d4est_hip_internal.h"

namespace d4est_hip {

struct VirtDesc {
  int dst;      // offset of the copy in a field over the subdomains
  int src;      // nodal_stride of the mesh element
  int N;        // deg + 1
  int lo[3];    // restricted node range per direction: lo <= index < hi
  int hi[3];
  int woff[3];  // hat weight of node index i in direction d: weights[woff[d] + i]
};

__device__ inline bool in_overlap(const VirtDesc& q, int n, int& i, int& j, int& k) {
  i = n % q.N;
  j = (n / q.N) % q.N;
  k = n / (q.N * q.N);
  return i >= q.lo[0] && i < q.hi[0] && j >= q.lo[1] && j < q.hi[1] && k >= q.lo[2] && k < q.hi[2];
}

}  // namespace d4est_hip

struct d4est_hip_schwarz {
  d4est_hip_plan_t* plan = nullptr;  // the subdomain plan (not owned)
  int n_sub = 0, n_virtual = 0, n_mesh = 0, overlap = 0;
  long long nodal_size = 0, restricted_nodal_size = 0;
  int mesh_nodes = 0;
  d4est_hip::VirtDesc* d_vd = nullptr;
  int* d_sub_first = nullptr;
  int* d_mesh_first = nullptr;    // per mesh element: first entry of its contribution list (n_mesh + 1)
  int* d_mesh_contrib = nullptr;  // subdomain elements that are copies of the mesh element, ascending (= ascending subdomain)
  int* d_mesh_stride = nullptr;
  int* d_mesh_N = nullptr;
  double* d_weights = nullptr;
  // workspace of iterate (lazy)
  double *d_du = nullptr, *d_r = nullptr, *d_d = nullptr, *d_Ad = nullptr, *d_zero_ghost = nullptr;
  double *d_delta = nullptr, *d_tol = nullptr;
  int *d_active = nullptr, *d_final_iter = nullptr, *d_n_active = nullptr;
  // flat list of the restricted nodes of every subdomain (field offsets), for the register-resident CG kernel
  int* d_box_off = nullptr;
  int* d_box_first = nullptr;        // n_sub + 1
  int max_box_nodes = 0;
  int min_box_nodes = 0;             // smallest restricted_nodal_size of a subdomain (0 without subdomains)
  // condensed copies (see ensure_condensed): copies with a handful of restricted nodes whose rows of the subdomain operator are kept as
  // small dense blocks instead of being applied matrix-free
  std::vector<d4est_hip::VirtDesc> h_vd;   // host copy of the copy descriptors
  int condensed_state = 0;           // 0 not looked at yet, 1 in use, -1 not applicable / switched off
  unsigned long long cond_generation = 0;   // the subdomain plan's op_generation the state above belongs to
  int n_cond = 0;
  void* d_cond = nullptr;            // CondDesc per condensed copy
  double* d_cond_blocks = nullptr;
  int* d_keep_list = nullptr;        // the copies that stay matrix-free
  int n_keep = 0;
  int* d_cond_off = nullptr;         // per condensed copy: field offsets of its inputs (own restricted nodes first, then the neighbours')
  long long cond_block_doubles = 0;
  // D4EST_HIP_SCHWARZ_FUSED_RESIDUAL=1 (read at create): the smoother loop (schwarz_smoother_run, schwarz_pc_run) forms rhs - A u
  // inside the CG start instead of writing it to a mesh vector first -- same numbers.  Off by default: on the level-4, p = 7 cycle
  // it measured no faster than the two-kernel sequence; D4EST_HIP_SCHWARZ_UNFUSED_RESIDUAL=1 forces it off.
  bool fused_residual = false;
  long long host_reads = 0;          // blocking reads of the device counters made so far (the "still iterating" looks and the public entry's sweep count)
  // ---- the subdomain solver (d4est_hip_schwarz_set_subdomain_solver): 0 the batched CG, 1 restarted GMRES (d4est_hip_schwarz_gmres.hip)
  int solver_kind = 0;
  int gmres_mr = 0;                  // restart length (subdomain_inner_iter)
  int last_solver = 0;               // the solver of the last iterate: what get_info reads
  long long gmres_bytes = 0;         // size of the GMRES workspace below
  double* d_gm_V = nullptr;          // (mr + 1) basis vectors, each a field over the subdomains
  double* d_gm_small = nullptr;      // per subdomain: h ((mr + 1) x mr, row-major), c (mr), s (mr), g (mr + 1)
  double* d_gm_rho = nullptr;        // per subdomain: rho, then (n_sub further on) rho_tol
  int* d_gm_state = nullptr;         // per subdomain: columns done in this restart cycle, then (n_sub further on) the flag
  // ---- whole-element exchange of a SHARDED handle (d4est_hip_schwarz_set_element_exchange); ex_fn == nullptr: one rank, nothing below is used.
  // The mesh handed to create() is the rank's extended mesh; u / r of iterate, smooth and the pc are vectors of the own nodes, the prefix.
  d4est_hip_element_exchange_fn ex_fn = nullptr;
  void* ex_ctx = nullptr;
  int n_own = 0, n_peers = 0;
  long long own_nodes = 0;
  std::vector<int> ex_peer;
  std::vector<long long> own_first, ghost_first;   // per peer (+ total): first double of its segment among the own-element / ghost-layer blocks
  double *d_r_ext = nullptr, *d_u_ext = nullptr;   // residual and correction on the extended mesh
  // packed buffers: direction 0 sends `own` and receives `ghost`, direction 1 sends `ghost_back` and receives `own_back`
  double *d_own_pack = nullptr, *d_ghost_pack = nullptr, *d_ghost_back = nullptr, *d_own_back = nullptr;
  int* d_own_blk_first = nullptr;    // per own element (n_own + 1): its entries of d_own_blk_off, in ascending peer rank
  int* d_own_blk_off = nullptr;      // offset of the element's block in the own-element packed layout of that peer
  int n_ghost_blocks = 0;
  int* d_ghost_blk_elem = nullptr;   // per ghost-layer block, peer after peer: its element ...
  int* d_ghost_blk_off = nullptr;    // ... and the block's offset in the ghost-layer packed layout
  std::vector<int> h_mesh_stride, h_mesh_N;
};

namespace d4est_hip {

// d4est_hip_schwarz_gmres.hip.  schwarz_gmres_solve: the subdomain solves of one iterate under GMRES -- sz->d_du receives the solutions
// (zero start), sz->d_r the restricted right-hand sides; r_mesh / Au_mesh as schwarz_cg_init_kernel takes them (Au_mesh != nullptr:
// the residual r_mesh - Au_mesh is formed in the start kernel).  Returns the number of batched operator applies made.
int schwarz_gmres_solve(d4est_hip_schwarz* sz, const double* r_mesh, const double* Au_mesh, int itr_max, double tol_abs, double tol_rel);
void schwarz_gmres_release(d4est_hip_schwarz* sz);   // frees the workspace (destroy, kind = 0)

}  // namespace d4est_hip
