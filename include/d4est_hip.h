/*
 * d4est_hip.h -- C-ABI of the MI355X (gfx950) matrix-free DG operator-apply engine.
 *
 * Drop-in boundary for d4est's element hot path.  Plain C:
 * pointers, ints and sizes only.  Vectors are ELEMENT-ORDERED exactly like d4est's
 * (element e occupies [nodal_stride[e], nodal_stride[e] + (deg[e]+1)^3), x fastest;
 * reference: src/Mesh/d4est_mesh.c:2395-2470, src/dGMath/d4est_operators.c:1318-1323).
 *
 * Error convention follows the reference: every entry point is void / returns a
 * handle, and invalid input or a HIP failure prints "[D4EST_HIP_ABORT] ..." and
 * abort()s, as D4EST_ABORT does (src/Utilities/d4est_util.h:171).
 *
 * Unless a function says "host", every double* / int* argument named *_dev is a
 * DEVICE pointer (hipMalloc / d4est_hip_malloc / a torch CUDA tensor's data_ptr).
 * All launches go to the plan's stream (default: the null stream).
 */
#ifndef D4EST_HIP_H
#define D4EST_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct d4est_hip_plan d4est_hip_plan_t;
typedef struct d4est_hip_transfer d4est_hip_transfer_t;   /* hp-multigrid inter-grid transfer, see below */
typedef struct d4est_hip_schwarz d4est_hip_schwarz_t;     /* additive Schwarz smoother, see below */
typedef struct d4est_hip_amr d4est_hip_amr_t;             /* one rank's hp-AMR bookkeeping, see below */

/* quadrature types (reference: [quadrature] name = legendre | lobatto,
 * src/Quadrature/d4est_quadrature_legendre.c:6-20, d4est_quadrature_lobatto.c:6-21) */
#define D4EST_HIP_QUAD_LEGENDRE 0
#define D4EST_HIP_QUAD_LOBATTO 1

/* ---- library info ---------------------------------------------------------- */
const char* d4est_hip_version(void);
int d4est_hip_device_count(void);

/* ---- 1-D operator tables (host) -------------------------------------------------
 * Replaces the lazily built cache of d4est_operators_t
 * (src/dGMath/d4est_operators.h:9-51, d4est_operators.c:196-304).  `out` is a HOST
 * buffer, row-major.  Returns the number of doubles written; with out == NULL only
 * returns the size.  deg_b is ignored by one-degree tables. */
enum d4est_hip_table_id {
  D4EST_HIP_TABLE_LOBATTO_NODES = 0,     /* deg_a+1            d4est_operators.c:727-733  */
  D4EST_HIP_TABLE_LOBATTO_WEIGHTS = 1,   /* deg_a+1            d4est_operators.c:735-741  */
  D4EST_HIP_TABLE_GAUSS_NODES = 2,       /* deg_a+1            d4est_operators.c:790-796  */
  D4EST_HIP_TABLE_GAUSS_WEIGHTS = 3,     /* deg_a+1            d4est_operators.c:798-805  */
  D4EST_HIP_TABLE_DIJ = 4,               /* N x N              d4est_operators.c:855-872  */
  D4EST_HIP_TABLE_MIJ = 5,               /* N x N              d4est_operators.c:712-724  */
  D4EST_HIP_TABLE_INVMIJ = 6,            /* N x N              d4est_operators.c:849-853  */
  D4EST_HIP_TABLE_LOBATTO_TO_GAUSS = 7,  /* (deg_b+1)x(deg_a+1) deg_a=lobatto, deg_b=gauss  d4est_operators.c:411-438 */
  D4EST_HIP_TABLE_P_PROLONG = 8,         /* (deg_b+1)x(deg_a+1) deg_a=degH, deg_b=degh      d4est_operators.c:995-1012 */
  D4EST_HIP_TABLE_HP_PROLONG = 9,        /* 2x(deg_b+1)x(deg_a+1)                            d4est_operators.c:944-993 */
  D4EST_HIP_TABLE_P_RESTRICT = 10,       /* (deg_a+1)x(deg_b+1)                              d4est_operators.c:1165-1185 */
  D4EST_HIP_TABLE_HP_RESTRICT = 11       /* 2x(deg_a+1)x(deg_b+1)                            d4est_operators.c:1232-1259 */
};
int d4est_hip_table(int table_id, int deg_a, int deg_b, double* out_host);

/* ---- device memory helpers for C hosts ------------------------------------------ */
void* d4est_hip_malloc(size_t bytes);
void d4est_hip_free(void* ptr_dev);
void d4est_hip_memcpy_h2d(void* dst_dev, const void* src_host, size_t bytes);
void d4est_hip_memcpy_d2h(void* dst_host, const void* src_dev, size_t bytes);
void d4est_hip_memset(void* dst_dev, int value, size_t bytes);
void d4est_hip_device_synchronize(void);

/* ---- plan -----------------------------------------------------------------------
 * One plan per (mesh, rank): mirrors what d4est_mesh_update produces
 * (src/Mesh/d4est_mesh.c:2790) -- per element deg, deg_quad, nodal_stride,
 * quad_stride (src/Mesh/d4est_element_data.h:13-48) -- all HOST int arrays of
 * length n_elements.  Elements are bucketed by (deg, deg_quad) internally. */
d4est_hip_plan_t* d4est_hip_plan_create(int n_elements, const int* deg, const int* deg_quad,
                                        const int* nodal_stride, const int* quad_stride, int quad_type);
void d4est_hip_plan_destroy(d4est_hip_plan_t* plan);
/* hipStream_t passed as void*; NULL = null stream */
void d4est_hip_plan_set_stream(d4est_hip_plan_t* plan, void* hip_stream);
/* Performance knobs (never change results beyond fp64 re-association).  Value -1 (default) = auto. */
enum d4est_hip_tuning_key {
  D4EST_HIP_TUNE_STIFFNESS_PREFETCH = 0, /* 1: request the metric at kernel entry (deg_quad <= 7), 0: at the point of use */
  D4EST_HIP_TUNE_STIFFNESS_WAVE = 1,     /* where (deg_quad+1)^2 <= 64: 0 multi-buffer kernel, 1 single-wavefront kernel, 2 two-wavefront kernel with metric prefetch, 3 single-wavefront kernel with pipelined operator loads (auto default for odd N), 11 even-odd single-wavefront kernel (auto default for even N, NQ; with deg_quad = deg in the collocated-gradient form, 12 one-dimensional products per thread), 12 the same kernel with the 16-product body at deg_quad = deg too (A/B runs; the whole operator then runs as volume kernel + face kernel); every value computes the same stiffness apply (tests/test_volume_gpu.py, tests/test_volume_cg_gpu.py) */
  D4EST_HIP_TUNE_STIFFNESS_STAGGER = 2,  /* single-wave kernel: delay (units of 1024 cycles) of every other resident workgroup row */
  D4EST_HIP_TUNE_FLUX_FAST = 3,          /* 0: always the generic flux kernel; else the wave-per-face kernel where all degrees <= 7 */
  D4EST_HIP_TUNE_STIFFNESS_BIGP = 4,     /* p >= 8: 0 three-field kernel, 1 two-field multi-wave kernel (default except p = 15), 2 at p = 12 ... 15 (deg_quad = deg): the FP64 matrix-core kernel (v_mfma_f64_16x16x4; default at p = 15, where no padding is needed) */
  D4EST_HIP_TUNE_OVERLAP_TRACES = 5,     /* 1: the trace kernel runs on a side stream beside the volume kernel (default off: the event waits cost more) */
  D4EST_HIP_TUNE_STIFFNESS_EO = 6,       /* multi-buffer / multi-wave kernels: 0 plain contractions, else (default) even-odd contractions where deg+1 and deg_quad+1 are even */
  D4EST_HIP_TUNE_AFFINE = 7,             /* 0: always stream the per-node metric (the reference's general path); else (default) buckets whose elements all have a node-independent J (dr/dx)(dr/dx)^T (detected in plan_set_geometry, 4 ulp) rebuild the metric from 6 numbers per element */
  D4EST_HIP_TUNE_GHOST_ALIAS = 8,        /* set before plan_set_faces; 1: all ghost sides of a conforming plan share block 0 of the ghost trace buffer (for a ghost trace that is the same on every side: the zero trace of a Schwarz subdomain plan); compute_ghost_traces is then meaningless */
  D4EST_HIP_TUNE_GRAPH = 9,              /* 1: d4est_hip_cheby_iterate is captured into a hipGraph on its first call and replayed while its arguments (pointers, iteration count, eigenvalue window) stay the same -- for launch-bound meshes (multigrid coarse levels); needs a non-null plan stream and no exchange callback (single rank); default off */
  D4EST_HIP_TUNE_FUSE_UPDATE = 10,       /* 0: cheby_iterate runs its update as a separate kernel; else (default) on conforming meshes up to p = 15 the update rides in the epilogue of the flux kernel (same roundings, bit-identical) */
  D4EST_HIP_TUNE_FACE_DIRECT = 11,       /* 0: apply_aij / apply_lhs / the smoothers always run the two-phase face kernels (traces, then flux); default: conforming plans with one degree, deg_quad <= 7 and at least 768 elements (below that the two-phase kernels, with several wavefronts per element, are faster on the mostly empty chip) run the single-wavefront kernel that forms both sides' traces from u itself (no trace arrays; with ghost sides the trace kernel still feeds the exchange); 1: that kernel for the face terms only, the volume kernel separately, whatever the size; 2: the whole operator in that one kernel where deg_quad = deg (else as 1), whatever the size -- the default picks this form too.  Conforming plans with one degree deg = deg_quad = 8 ... 15 have the multi-wave form of that kernel (one workgroup per element: volume term, then the trace-free face terms; d4est_hip_direct_mw.hip), which is the default at EVERY size; values 0 / 1 / 2 select as above */
  D4EST_HIP_TUNE_STREAM = 12,            /* stream mode of the volume kernels with more than 8192 elements or deg >= 8, and of the p = 8 ... 15 whole-operator kernel: the data an apply reads or writes exactly once (metric, mortar factors, A u) moves with the non-temporal hint. default (-1): on when metric + u + A u of one apply exceed 320 MB (they then do not fit the 256 MB Infinity Cache, and keeping them out of the caches leaves those to u: level 5, p = 7 stiffness 191 -> 156 us); 0 / 1 force it off / on.  Same numbers either way */
  D4EST_HIP_TUNE_HP_SPLIT = 13,          /* set before plan_set_faces.  Plans with hanging faces, every deg and deg_quad <= 7 (any number of ranks): 0 every side through the tiled mortar-record kernels; 1 the conforming sides of the whole mesh AND the small sides of the hanging faces (one mortar each, the hanging factor folded into the geometric factors) through the fast conforming face kernels, only the big sides (four mortars) through the record kernels; default (-1): that split unless more than half of the elements would stay with the record kernels (level-4 brick, p = 7, every 64th ... every 3rd octant refined: apply_aij 203 -> 139 ... 661 -> 448 us).  Round 4: plans with degrees up to 15 take the split too (their conforming sides through the tiled conforming kernels, on the two family lists where the plan has them), and the record kernels run in their unit form (a side's sub-mortar records on four wavefronts); environment D4EST_HIP_HP_SPLIT_FAST_ONLY=1 / D4EST_HIP_NO_HANG_UNITS=1 restore round 3's forms */
  D4EST_HIP_TUNE_HYBRID = 14,            /* set before plan_set_faces.  Mixed-degree and locally refined plans; on one rank by default, on a shard (a plan with ghost sides) by opting in with value 2: 0 every element through the two-phase kernels; CLEAN elements -- deg_quad = deg <= 15 and all six sides conforming against a local element of the same degree or the domain boundary -- get the whole operator from the trace-free one-kernel path of their degree (faces_direct_kernel / operator_mw_kernel over an element list), only the rest runs traces + volume + flux, on lists.  default (-1): where that was measured to pay -- the clean elements are one degree bucket and at least half of the mesh (locally refined meshes of one degree: level 4, p = 7, every 64th octant refined, apply_aij 144 -> 125 us); with several clean buckets the largest one is kept where it holds at least half of the mesh (one dominant degree; the others' elements stay two-phase) -- or, at size (at least 2048 clean elements per clean bucket), every bucket --, else every bucket would be its own latency-structured launch and the two-phase kernels win at these sizes; 1: whenever there is a clean element.  Same operator either way (tests/test_hybrid_gpu.py).  Hanging-aware form (plans under the hp split, elements with deg <= 7; environment D4EST_HIP_HYBRID_NO_HANGING=1 switches it off; mixed-aware form likewise for a conforming side against a lower-degree neighbour, D4EST_HIP_HYBRID_NO_MIXED=1): a hanging side does not make an element dirty -- big sides stay with the record kernels, small sides read the big element's sub-mortar block from the trace array and export their own; on a locally refined mesh of one degree EVERY element then takes the one-kernel path (level 4, p = 7, every 64th octant refined: 125 -> 81 us) and cheby_iterate carries its update in the operator kernel and the record flux kernel.  2: as 1, and also on plans with ghost sides (values -1, 0 and 1 leave such plans on the two-phase kernels, or on the one-degree direct kernel of key 11): ghost-aware form -- a conforming side against a GHOST element of the same deg and deg_quad does not make an element (deg <= 7) dirty either, the kernel reads the (+) block from the exchanged ghost trace buffer as the two-phase flux kernel does; a ghost neighbour of another degree, a hanging face cut by the shard boundary and every ghost side of a deg >= 8 element leave the element with the two-phase kernels.  Launch order on the plan's stream: trace kernels of the elements whose blocks are sent or read, exchange phase 0, clean elements without a ghost side, exchange phase 1, clean elements beside a ghost side, dirty flux; cheby_iterate keeps its fused update (bit-identical to key 10 = 0).  Environment D4EST_HIP_HYBRID_NO_GHOST=1 switches the form off.  Not yet measured on several GPUs, hence opt-in (tests/test_hybrid_ghost_gpu.py) */
  D4EST_HIP_TUNE_KRYLOV_CHECK = 15,      /* d4est_hip_cg_solve: iterations enqueued between two host reads of the device stop flag (default -1 = 8); every value gives the same iterates, bit for bit, and the same count (iterations after the stop are no-ops on the device) */
  D4EST_HIP_TUNE_STIFFNESS_ENTRY = 16,   /* schedule of the metric stream in the collocated-gradient single-wavefront kernels of key 1 (deg_quad = deg <= 7, streamed metric; stiffness_wave_eo_kernel, stiffness_wave_eo_multi_kernel): 0 the first metric plane is requested before the last forward contraction; 1 the first planes of a thread's quadrature line are requested at kernel entry, right behind the element's own loads, and wait in registers under the forward contractions; default (-1): 1 in the one-bucket kernel at deg = 7, else 0.  The same arithmetic in the same order: bit-identical results (tests/test_volume_entry_prefetch_gpu.py) */
  D4EST_HIP_TUNE_COUNT = 17
};
void d4est_hip_plan_set_tuning(d4est_hip_plan_t* plan, int key, int value);
/* name of the stiffness kernel the last d4est_hip_apply_stiffness_matrix selected (for reports / profiles) */
const char* d4est_hip_plan_last_kernel(const d4est_hip_plan_t* plan);
/* Which face kernels apply_aij / apply_lhs / the smoothers run on this plan (after plan_set_faces, with the current tuning):
 * "direct" (one kernel, traces formed from u in place: conforming plans with one degree, deg_quad <= 7 or deg = deg_quad <= 15),
 * "direct+volume" (the same kernel also applies the element's volume term and writes A u once: deg_quad = deg <= 15, after
 * plan_set_geometry), "two-phase" (trace kernel, then flux kernel) or "hybrid: direct+volume on C clean elements, two-phase on D"
 * (mixed-degree / locally refined plans, tuning key D4EST_HIP_TUNE_HYBRID); on a plan with ghost sides under value 2 of that key
 * "hybrid: direct+volume on C clean elements (G beside ghost sides), two-phase on D". */
const char* d4est_hip_plan_face_path(const d4est_hip_plan_t* plan);
int d4est_hip_plan_local_nodes(const d4est_hip_plan_t* plan);
int d4est_hip_plan_local_nodes_quad(const d4est_hip_plan_t* plan);
/* 1 when the plan runs in stream mode (tuning key D4EST_HIP_TUNE_STREAM: forced, or chosen from the plan's size), else 0 */
int d4est_hip_plan_stream_mode(const d4est_hip_plan_t* plan);
int d4est_hip_plan_n_elements(const d4est_hip_plan_t* plan);

/* Geometric factors in the reference's SoA layout (src/Mesh/d4est_mesh.h:123-169,
 * d4est_mesh.c:2757-2776): J_quad[local_nodes_quad];
 * rst_xyz_quad[(3*i+j)*local_nodes_quad + quad_stride[e] + n] = d r_i / d x_j.
 * on_device != 0: the two pointers are device pointers, else host pointers.
 * The plan keeps J and the pre-combined symmetric metric  W J (dr/dx)(dr/dx)^T
 * (6 entries per quadrature node, element-blocked); the inputs are not retained. */
void d4est_hip_plan_set_geometry(d4est_hip_plan_t* plan, const double* J_quad, const double* rst_xyz_quad, int on_device);

/* Volume factors with DX_compute_method = GEOM_COMPUTE_NUMERICAL (src/Mesh/d4est_mesh.c:2637-2671): the caller hands over only the
 * physical coordinates of the Lobatto nodes, xyz_lobatto = x[local_nodes] | y[local_nodes] | z[local_nodes] (d4est_factors->xyz, any
 * geometry: cubed sphere, disk, ...; 24 B/node instead of the 80 B per quadrature node of plan_set_geometry); the device forms
 * dx_d/dr_d1 = interpolate(D_d1 x_d) at the quadrature nodes, J and dr/dx (src/Geometry/d4est_geometry.c:877-976) and the
 * pre-combined metric.  Mortar factors still come through plan_set_mortar_geometry. */
void d4est_hip_plan_set_geometry_numerical(d4est_hip_plan_t* plan, const double* xyz_lobatto, int on_device);
/* Geometric factors generated ON THE DEVICE for the reference's `brick` geometry ([geometry] name = brick, X0..Z1;
 * src/Geometry/d4est_geometry_brick.c:140-206: dx_d/dr_d = (X1_d - X0_d) (dq / P4EST_ROOT_LEN) / 2, diagonal, constant per element) --
 * SURVEY.md section 8f rank 4, brick only.  Replaces d4est_hip_plan_set_geometry / _set_mortar_geometry on a brick: no J_quad /
 * rst_xyz_quad / mortar arrays are formed on the host or uploaded.  elem_dq[e] = the quadrant's side length in p4est integer
 * coordinates (d4est_element_data_t::dq), root_len = P4EST_ROOT_LEN, extents = {X0, X1, Y0, Y1, Z0, Z1}.  The mortar variant is
 * called where d4est_hip_plan_set_mortar_geometry would be (after plan_set_faces / plan_set_sipg); hanging faces use the mortar-sized
 * cell (src/Mesh/d4est_mortars.c:420-470); hm / hp by the plan's face_h_type (d4est_hip_plan_set_h_types; default FACE_H_EQ_J_DIV_SJ_QUAD). */
void d4est_hip_plan_set_geometry_brick(d4est_hip_plan_t* plan, const int* elem_dq, double root_len, const double* extents);
void d4est_hip_plan_set_mortar_geometry_brick(d4est_hip_plan_t* plan, const int* elem_dq, double root_len, const double* extents);

/* Geometric factors of an ANALYTIC tree map generated on the device (DX_compute_method =
 * GEOM_COMPUTE_ANALYTIC, JAC_compute_method = GEOM_COMPUTE_NUMERICAL as the reference requires, src/Mesh/d4est_mesh.c:2637-2680,
 * :858-1108): the host hands over only where every element sits in the forest -- d4est_element_data_t::tree, ::q[3], ::dq
 * (src/Mesh/d4est_element_data.h:13-48), p4est integer coordinates, root_len = P4EST_ROOT_LEN -- instead of 96 B per quadrature node
 * and 24 doubles per mortar node.  geom_type / params:
 *   D4EST_HIP_GEOM_CUBED_SPHERE_7TREE  [geometry] name = cubed_sphere_7tree (src/Geometry/d4est_geometry_cubed_sphere.c:498-580,
 *                                      :1884-1899): params = {R0, R1, compactify_inner_shell}; trees 0..5 wedges, 6 the centre cube
 *   D4EST_HIP_GEOM_CUBED_SPHERE        [geometry] name = cubed_sphere (:316-403, :2070-2100): the 13 trees of
 *                                      p8est_connectivity_new_sphere -- 0..5 outer wedges on (R1, R2), 6..11 inner wedges on
 *                                      (R0, R1), 12 the centre cube
 *   D4EST_HIP_GEOM_CUBED_SPHERE_WITH_SPHERE_HOLE  name = cubed_sphere_with_sphere_hole (:407-497): the 12 trees of
 *                                      d4est_connectivity_new_sphere_with_hole, both shells equiangular
 *   D4EST_HIP_GEOM_CUBED_SPHERE_WITH_CUBE_HOLE    name = cubed_sphere_with_cube_hole (:2243-2260): the 13-tree map on those 12 trees
 *     params of these three = {R0, R1 > R0, R2 > R1, compactify_outer_shell, compactify_inner_shell} (flags: zero / non-zero).
 *     compactify_inner_shell != 0 is REJECTED for cubed_sphere and cubed_sphere_with_cube_hole (abort; d4est_hip_tree_map returns
 *     non-zero): the reference's map of those trees ignores the flag while its analytic Jacobian honours it, so the factors would
 *     not be the Jacobian of the map.  cubed_sphere_with_sphere_hole takes both flags.
 * The mortar variant is called where d4est_hip_plan_set_mortar_geometry would be (after plan_set_hanging / plan_set_faces /
 * plan_set_sipg), needs the same three arrays for the ghost elements (order of ghost_deg), follows faces between trees through
 * side_reorder / side_orientation and hanging faces through the half-size virtual children of the big element
 * (src/Mesh/d4est_mortars.c:419-468); hm / hp by the plan's face_h_type (d4est_hip_plan_set_h_types; default FACE_H_EQ_J_DIV_SJ_QUAD). */
#define D4EST_HIP_GEOM_CUBED_SPHERE_7TREE 1
#define D4EST_HIP_GEOM_CUBED_SPHERE 2
#define D4EST_HIP_GEOM_CUBED_SPHERE_WITH_SPHERE_HOLE 3
#define D4EST_HIP_GEOM_CUBED_SPHERE_WITH_CUBE_HOLE 4
void d4est_hip_plan_set_geometry_analytic(d4est_hip_plan_t* plan, int geom_type, const double* params, const int* elem_tree,
                                          const int* elem_q, const int* elem_dq, double root_len);
void d4est_hip_plan_set_mortar_geometry_analytic(d4est_hip_plan_t* plan, int geom_type, const double* params, const int* elem_tree,
                                                 const int* elem_q, const int* elem_dq, const int* ghost_tree, const int* ghost_q,
                                                 const int* ghost_dq, double root_len);

/* Node coordinates of the same maps on the device: xyz_lobatto_dev = x[local_nodes] | y | z at every element's Lobatto nodes
 * (d4est_factors->xyz, what d4est_hip_plan_set_geometry_numerical takes), xyz_quad_dev = x[local_nodes_quad] | y | z at its quadrature
 * nodes (Gauss or Lobatto by the plan's quad_type; d4est_factors->xyz_quad) -- for the right-hand side, the coefficient of a
 * linearised term, boundary data.  Either pointer may be NULL.  One thread per node on the plan's stream, no host synchronisation;
 * the plan allocates its small staging on the first call and nothing afterwards.  Boundary-face coordinates need no entry of their
 * own: d4est_hip_plan_boundary_gather of each of the three Lobatto components gives them in the order
 * d4est_hip_plan_set_dirichlet_values expects.  Aborts like plan_set_geometry_analytic on a bad type, tree or flag. */
void d4est_hip_plan_compute_xyz_analytic(d4est_hip_plan_t* plan, int geom_type, const double* params, const int* elem_tree,
                                         const int* elem_q, const int* elem_dq, double root_len, double* xyz_lobatto_dev,
                                         double* xyz_quad_dev);
/* The same map evaluated on the HOST (the host side of the inline functions the kernels call; no HIP call, works without a GPU):
 * x_out[3] = x(tree, xi) and dxdxi_out[9] = d x_i / d xi_j (row-major) at tree coordinates xi[3] in [0,1]^3; either output may be
 * NULL.  Returns 0, or non-zero -- without aborting -- for an unknown type, bad radii, a rejected flag or a tree out of range. */
int d4est_hip_tree_map(int geom_type, const double* params, int tree, const double* xi, double* x_out, double* dxdxi_out);
/* The map's second derivatives on the HOST, likewise without a HIP call: d2_out[9 i + 3 j + k] = d^2 x_i / d xi_j d xi_k at xi[3], the
 * chain rule through the functions that give x and dx/dxi (what d4est_geometry_cubed_sphere_D2X, src/Geometry/
 * d4est_geometry_cubed_sphere.c:585-790, gives for the 13-tree sphere from machine-generated closed forms; those are not transcribed,
 * and that file's `c` is built from s instead of t at :629).  Exactly symmetric in (j, k); zero on the centre cube.  Return codes:
 * those of d4est_hip_tree_map. */
int d4est_hip_tree_map_d2(int geom_type, const double* params, int tree, const double* xi, double* d2_out /*27*/);

/* ---- volume kernels (device vectors of local_nodes doubles) ---------------------- */
/* Au = K u : replaces d4est_laplacian_apply_stiffness_matrix (src/dGMath/d4est_laplacian.c:198-234)
 * = loop of d4est_quadrature_apply_stiffness_matrix (src/Quadrature/d4est_quadrature.c:263-382).
 * Au is OVERWRITTEN (as the reference's zero-fill at :337). */
void d4est_hip_apply_stiffness_matrix(d4est_hip_plan_t* plan, const double* u_dev, double* Au_dev);
/* Mu = M u : loop of d4est_quadrature_apply_mass_matrix (src/Quadrature/d4est_quadrature.c:385-477) */
void d4est_hip_apply_mass_matrix(d4est_hip_plan_t* plan, const double* u_dev, double* Mu_dev);
/* out = V^T W J f_quad : d4est_quadrature_apply_galerkin_integral (d4est_quadrature.c:142-213);
 * f_quad_dev has local_nodes_quad doubles (element e at quad_stride[e]) */
void d4est_hip_apply_galerkin_integral(d4est_hip_plan_t* plan, const double* f_quad_dev, double* out_dev);
/* u_quad = V u : d4est_quadrature_interpolate (d4est_quadrature.c:966-1016) */
void d4est_hip_interpolate(d4est_hip_plan_t* plan, const double* u_dev, double* u_quad_dev);
/* out = V^T (W J c) V u : d4est_quadrature_apply_fofufofvlilj with QUAD_APPLY_MATRIX (d4est_quadrature.c:593-774) =
 * d4est_quadrature_apply_mass_matrix with jac_quad replaced by jac_quad * f(u) f(v).  The reference evaluates the
 * callbacks f(u), f(v) on the host at the quadrature nodes (:661-683); here the caller hands their product
 * coeff_quad_dev (local_nodes_quad doubles, element e at quad_stride[e]) -- e.g. d4est_hip_interpolate + one
 * elementwise kernel of its own. */
void d4est_hip_apply_weighted_mass_matrix(d4est_hip_plan_t* plan, const double* u_dev, const double* coeff_quad_dev, double* out_dev);
/* out = V^-1 (W J)^-1 V^-T in : d4est_quadrature_apply_inverse_mass_matrix (d4est_quadrature.c:1222-1331).  As in the
 * reference this is always Gauss-Legendre and needs deg_quad == deg on every element (the assert at :1233); aborts
 * otherwise. */
void d4est_hip_apply_inverse_mass_matrix(d4est_hip_plan_t* plan, const double* in_dev, double* out_dev);
/* out = (M (x) M (x) M) in and (M^-1 (x) M^-1 (x) M^-1) in per element, M the 1-D reference mass matrix:
 * d4est_operators_apply_mij / d4est_operators_apply_invmij (d4est_operators.c:891-928), batched over the plan. */
void d4est_hip_apply_mij(d4est_hip_plan_t* plan, const double* in_dev, double* out_dev);
void d4est_hip_apply_invmij(d4est_hip_plan_t* plan, const double* in_dev, double* out_dev);
/* out = D_dir in and out = D_dir^T in per element, dir = 0, 1, 2 = r, s, t: d4est_operators_apply_dij / _dij_transpose
 * (d4est_operators.c:1385-1410, :2259-2284), batched over the plan; in and out must not alias. */
void d4est_hip_apply_dij(d4est_hip_plan_t* plan, const double* in_dev, int dir, double* out_dev);
void d4est_hip_apply_dij_transpose(d4est_hip_plan_t* plan, const double* in_dev, int dir, double* out_dev);
/* Trace of a volume field on face `face` of every element and its inverse scatter: d4est_operators_apply_slicer / _apply_lift
 * (d4est_operators.c:1521-1582, :1454-1519), batched.  A face vector holds N_e^2 values per element (tangential axes in increasing
 * order, the first fastest), element e at sum_{e' < e} N_{e'}^2; d4est_hip_plan_face_nodes = its length.  The lift zero-fills. */
int d4est_hip_plan_face_nodes(const d4est_hip_plan_t* plan);
void d4est_hip_apply_slicer(d4est_hip_plan_t* plan, const double* in_dev, int face, double* out_face_dev);
void d4est_hip_apply_lift(d4est_hip_plan_t* plan, const double* in_face_dev, int face, double* out_dev);
/* dudr_i = D_i u, i = 0..2 : d4est_laplacian_compute_dudr (d4est_laplacian.c:237-282), 3 applies of
 * d4est_operators_apply_dij (d4est_operators.c:1385-1410) per element. */
void d4est_hip_compute_dudr(d4est_hip_plan_t* plan, const double* u_dev, double* dudr0_dev, double* dudr1_dev, double* dudr2_dev);

/* ---- faces: SIPG mortar terms (conforming mortars, Dirichlet boundaries) ------------------------------
 * Flat side list, side s = 6*e + f ((-) element e, face f = 0..5 = -x,+x,-y,+y,-z,+z), HOST int arrays of 6*n_elements:
 * what the reference's face iteration hands to its flux callback (src/Mesh/d4est_mortars.c:601-803):
 *   side_nbr[s]        >= 0: local (+) element; -1: domain boundary; <= -2: ghost element g = -(v+2)
 *   side_nbr_face[s]   face of the (+) element
 *   side_reorder[s]    flip0 | flip1<<1 | transpose<<2, the result of p4est_expand_face_transform as used by
 *                      d4est_operators_reorient_face_data (src/dGMath/d4est_operators.c:2031-2081); 0 inside one tree
 *   side_mortar_stride[s]  scalar offset S of the side's mortar quadrature data (d4est_laplacian_flux.c:417-449)
 *   side_bndry_stride[s]   offset of the side's Dirichlet values (boundary sides)
 * Ghost elements: ghost_deg / ghost_deg_quad (n_ghost), as p4est_ghost_exchange_data ships them (Mesh/d4est_ghost.c:52). */
void d4est_hip_plan_set_faces(d4est_hip_plan_t* plan, const int* side_nbr, const int* side_nbr_face, const int* side_reorder,
                              const int* side_mortar_stride, const int* side_bndry_stride, int total_mortar_nodes,
                              int total_bndry_nodes, int n_ghost, const int* ghost_deg, const int* ghost_deg_quad);
/* The side arrays of d4est_hip_plan_set_faces / _set_hanging built on the HOST from a p8est connectivity and the list of quadrants
 * alone -- for hosts without p4est_iterate; a d4est build records the same numbers from its face callback.
 * tree_to_tree / tree_to_face: p8est connectivity (6 per tree; face + 6 * orientation; a boundary face points at itself).  Local
 * elements: tree, q (3 per element, p4est integer coordinates in [0, root_len)), dq (side length), deg, deg_quad -- in the rank's element
 * order; ghost quadrants (the off-rank face neighbours the rank knows) likewise, referenced as -(g + 2).  The mesh must be 2:1
 * balanced across faces.  Outputs (caller-allocated: 6 n_local ints each, side_nbr4 24 n_local): everything set_faces / set_hanging
 * take, with mortar strides assigned in side order (the small sides of a hanging face share the block of their group's first local
 * member, src/Mesh/d4est_mesh.c:956-962) -- to be used with device-generated factors (plan_set_mortar_geometry_brick / _analytic) or
 * with host arrays laid out by the same strides.  Returns 1 when the mesh has hanging faces (then call plan_set_hanging). */
int d4est_hip_build_sides(int n_trees, const int* tree_to_tree, const int* tree_to_face, int root_len, int n_local, const int* tree,
                          const int* q, const int* dq, const int* deg, const int* deg_quad, int n_ghost, const int* ghost_tree,
                          const int* ghost_q, const int* ghost_dq, const int* ghost_deg_quad, int* side_nbr, int* side_nbr_face,
                          int* side_reorder, int* side_orientation, int* side_hang, int* side_sub, int* side_nbr4,
                          int* side_mortar_stride, int* side_bndry_stride, int* total_mortar_nodes, int* total_bndry_nodes);
/* The integer topology tables the library works with (csrc/d4est_hip_topology.h), for hosts that want the same numbers and for the
 * pin against the reference's own data (tests/test_topology_tables.py): id 0 p8est_face_corners [6][4], 1 p8est_face_dual [6],
 * 2 p8est_face_permutations [8][4], 3 p8est_face_permutation_sets [3][4], 4 p8est_face_permutation_refs [6][6], 5 p8est_corner_faces [8][3]
 * (p4est-2.8 src/p8est_connectivity.c:29-63, :145-152); 10 / 11 / 12 d4est_reference_p8est_FToF_code [6][6] / _code_to_perm [3][4] /
 * _perm_to_order [8][4] (src/dGMath/d4est_reference.c:3-12).  Returns the entry count (row-major ints written to out; out == NULL: count
 * only), -1 for an unknown id. */
int d4est_hip_topology_table(int id, int* out);
/* Non-conforming (hanging, 1 <-> 4) faces of a 2:1 balanced mesh; call BEFORE d4est_hip_plan_set_faces (conforming meshes skip it).
 * HOST int arrays over the sides s = 6*e + f, mirroring the two calls the reference's face iteration makes per hanging face
 * (src/Mesh/d4est_mortars.c:700-803: (e_m[4], faces_m = 4 | e_p[1]) and (e_m[1] | e_p[4], faces_p = 4)):
 *   side_hang[s]        0 conforming or boundary; 1 "big" side: this face is split, (+) side = 4 small elements;
 *                       2 "small" side: this element is one of the 4 hanging elements, (+) side = the big element (side_nbr[s])
 *   side_sub[s]         small side: index of this element among the 4 (p4est order of the hanging quadrants = z-order on the face)
 *   side_nbr4[4s..4s+3] big side: the four (+) elements in (-) order (e_p_oriented, src/Mesh/d4est_element_data.c:130-150);
 *                       small side: the four members e_m[0..3] of its own group
 *   side_orientation[s] p4est face orientation 0..3 (selects d4est_reference_reorient_face_order, dGMath/d4est_reference.c:84-110)
 * Mortar data layout as the reference allocates it (src/Mesh/d4est_mesh.c:956-979): the block of a hanging face holds its 4
 * sub-mortars one after another (scalars), vector / matrix components are strided by the block's TOTAL node count, the four small
 * sides share ONE block (the same side_mortar_stride), and drst_dxyz_p_porder is stored in the (+) side's sub-face order.
 * Element references (side_nbr, side_nbr4) are local ids or ghost codes -(g + 2), as in side_nbr.  Plans with hanging faces
 * and ghost elements take the ghost traces from the trace exchange (the *_sub block accessors below); d4est_hip_compute_ghost_traces
 * (whole ghost elements) serves conforming plans only.
 * Faces between trees: side_orientation / side_reorder as p4est reports them; every (f_m, f_p, orientation) triple is followed as the
 * reference computes it.  For transposed pairs with exactly one flip seen from the lower-numbered face (reorder codes 5, 6 -- none in
 * the reference's own connectivities) d4est_operators_reorient_face_data is not the geometric map; on a SMALL side of such a pair the
 * reference takes u and du/dx from different children of the big face, which the engine reproduces when the four sub-mortars share one
 * quadrature degree and the big element is local, and aborts otherwise. */
void d4est_hip_plan_set_hanging(d4est_hip_plan_t* plan, const int* side_hang, const int* side_sub, const int* side_nbr4,
                                const int* side_orientation);
/* SIPG parameters ([flux] sipg_penalty_prefactor, sipg_penalty_fcn; d4est_laplacian_flux_sipg.c:945-1005):
 * fcn 0 maxp_sqr_over_minh (default), 1 meanp_sqr_over_meanh, 2 maxpp1_sqr_over_minh, 3 mean_p_sqr_over_h.
 * Call BEFORE d4est_hip_plan_set_mortar_geometry (the penalty is folded into the face factors). */
void d4est_hip_plan_set_sipg(d4est_hip_plan_t* plan, double penalty_prefactor, int penalty_fcn);
/* Mortar geometric factors in the reference's layout (src/Mesh/d4est_mesh.c:946-1108): with T nodes on the side's mortar,
 * sj[S+k], n[3S + d*T + k], drst_dxyz_m / drst_dxyz_p_porder[9S + (i+3j)*T + k] = d r_i/d x_j, hm[S+k], hp[S+k]. */
void d4est_hip_plan_set_mortar_geometry(d4est_hip_plan_t* plan, const double* sj, const double* n, const double* drst_dxyz_m,
                                        const double* drst_dxyz_p_porder, const double* hm, const double* hp, int on_device);
/* ---- a-posteriori error estimator (csrc/d4est_hip_estimator.hip) -----------------------------------------------------------------
 * d4est_estimator_bi_compute (src/Estimators/d4est_estimator_bi.c:343-560), which the hp-adaptive drivers call once per AMR level after
 * the solve (e.g. src/Problems/ConstantDensityStar/constant_density_star_mgpc_newton_petsc.c:306-324).  Per local element e,
 * eta2[e] = term0 + term1 + term2 + term3, summed in that order:
 *   term0  (h_e^2 / p_e^2) r_e^T M_e r_e, M_e = V^T W J V at deg_quad (:395-441; d4est_mesh_compute_l2_norm_sqr, src/Mesh/d4est_mesh.c:2299-2370)
 *   term1  sum over the interior mortars of e of sum_k w_k sj_k (pi_grad n.(grad u_m - grad u_p))^2   (d4est_estimator_bi_interface, :150-340)
 *   term2  sum over the interior mortars of e of sum_d sum_k w_k sj_k (pi_u n_d (u_m - u_p))^2
 *   term3  sum over the boundary sides of e of sum_d sum_k w_k sj_k (pi_D n_d (u_m - g))^2              (d4est_estimator_bi_dirichlet, :15-148)
 * Every local side adds to its own element only; a big hanging side adds its four sub-mortars, a small side its own; the prefactor
 * degrees are those of the mortar's two elements (:212-228); pi_D is evaluated as pi_D(p, h_m, p, h_m).  The boundary term is always
 * the Dirichlet one, with g given here, whatever Dirichlet / Robin data the plan's operator holds (the reference forces BC_DIRICHLET,
 * :491-496).  The penalty functions of d4est_estimator_bi.h, by id (any id in any role; c = penalty_prefactor): */
#define D4EST_HIP_EST_BI_GRADU_MAXP_MINH 0              /* sqrt(min_h / max_p)                      bi_gradu_prefactor_maxp_minh */
#define D4EST_HIP_EST_BI_U_MAXP_MINH 1                  /* sqrt(c max_p^2 / min_h)                  bi_u_prefactor_conforming_maxp_minh */
#define D4EST_HIP_EST_BI_GRADU_MAX_H_OVER_P 2           /* sqrt(max(h_m/p_m, h_p/p_p))              bi_gradu_prefactor_max_h_over_p */
#define D4EST_HIP_EST_BI_U_MAX_P2_OVER_H 3              /* sqrt(c max(p_m^2/h_m, p_p^2/h_p))        bi_u_prefactor_conforming_max_p2_over_h */
#define D4EST_HIP_EST_HOUSTON_GRADU_MAX_H_OVER_P 4      /* sqrt(.5 max(h_m/p_m, h_p/p_p))           houston_gradu_prefactor_max_h_over_p */
#define D4EST_HIP_EST_HOUSTON_U_MAX_P2_OVER_H 5         /* sqrt(.5 c max(p_m^2/h_m, p_p^2/h_p))     houston_u_prefactor_max_p2_over_h */
#define D4EST_HIP_EST_HOUSTON_U_DIRICHLET_MAX_P2_OVER_H 6 /* sqrt(c max(p_m^2/h_m, p_p^2/h_p))      houston_u_dirichlet_prefactor_max_p2_over_h */
#define D4EST_HIP_EST_HOUSTON_GRADU_MAXP_MINH 7         /* sqrt(.5 min_h / max_p)                   houston_gradu_prefactor_maxp_minh */
#define D4EST_HIP_EST_HOUSTON_U_MAXP_MINH 8             /* sqrt(.5 c max_p^2 / min_h)               houston_u_prefactor_maxp_minh */
#define D4EST_HIP_EST_HOUSTON_U_DIRICHLET_MAXP_MINH 9   /* sqrt(c max_p^2 / min_h)                  houston_u_dirichlet_prefactor_maxp_minh */
/* Config 4 uses (7, 8, 9) with c = sipg_penalty_prefactor (constant_density_star_mgpc_newton_petsc.c:195-199).  Call BEFORE
 * d4est_hip_plan_set_mortar_geometry or its brick / analytic forms (the estimator's per-node factors are formed there from the mortar
 * factors, as the SIPG penalty is: the same rule as d4est_hip_plan_set_sipg).  Plans without this call allocate nothing for the
 * estimator and run as before.  Aborts ([D4EST_HIP_ABORT]) on a NULL plan or an id outside 0..9. */
void d4est_hip_plan_set_estimator(d4est_hip_plan_t* plan, int gradu_fcn, int u_fcn, int u_dirichlet_fcn, double penalty_prefactor);
/* eta2_dev[n_elements] (and terms_dev[4 n_elements], term-major: term t of element e at t n_elements + e, the reference's estimator_vtk
 * layout; NULL = not wanted) from device vectors u_dev and residual_dev (local_nodes: the residual d4est_elliptic_eqns_build_residual
 * leaves in Au) and diam_dev[n_elements] (d4est_mesh_data_t::diam_volume; NULL = the plan's own diam_volume,
 * d4est_hip_plan_compute_size_parameters_* / _compute_diameters, and an abort if that has not been computed).  ghost_trace_dev: the ghost trace buffer of plans with ghost
 * sides (d4est_hip_plan_ghost_trace_size doubles, filled by the caller's exchange of u's traces), or NULL -- then the traces are
 * exchanged through the plan_set_comm hooks, as apply_lhs does (on plans with hanging faces the *_sub blocks included).
 * g_lobatto_dev: Dirichlet data on the boundary sides' Lobatto face nodes in the layout of d4est_hip_plan_set_dirichlet_values, NULL =
 * g = 0.  Needs plan_set_geometry (or a form of it), plan_set_faces, the mortar factors and d4est_hip_plan_set_estimator before them;
 * aborts otherwise.  Everything runs on the plan's stream, without host synchronisation; no atomics: bit-identical from call to call,
 * the same on every face path of the operator (the estimator forms every side's trace itself).  Limit: the residual term holds one
 * element's interpolated residual in LDS, (max(N^3, NQ^2 N) + NQ N^2) doubles, N = deg + 1, NQ = deg_quad + 1 -- up to deg_quad = deg + 2
 * at p = 19 (160 KB); a plan beyond it aborts here. */
void d4est_hip_estimator_bi(d4est_hip_plan_t* plan, const double* u_dev, const double* ghost_trace_dev, const double* residual_dev,
                            const double* diam_dev, const double* g_lobatto_dev, double* eta2_dev, double* terms_dev);
/* The estimator with the POINTWISE (strong-form) residual: d4est_estimator_bi_new_compute(..., use_pointwise_residual = 1)
 * (src/Estimators/d4est_estimator_bi_new.c:386-567), what the *_anares drivers call (src/Problems/cds_anares.c:303-343).  Identical to
 * d4est_hip_estimator_bi except for term 0: residual_quad_dev holds local_nodes_quad values r_q at the quadrature nodes and
 * term 0 = h^2 / deg^2 sum_q w_q J_q r_q^2 (:471-487, d4est_quadrature_innerproduct; no interpolation, no LDS limit).  Terms 1 - 3 and
 * eta2 take the same kernels as d4est_hip_estimator_bi.  Out of scope: a compactified factor set distinct from the physical one
 * (d4est_factors_compactified != d4est_factors_physical) and estimator_vtk_per_face. */
void d4est_hip_estimator_bi_pointwise(d4est_hip_plan_t* plan, const double* u_dev, const double* ghost_trace_dev,
                                      const double* residual_quad_dev, const double* diam_dev, const double* g_lobatto_dev,
                                      double* eta2_dev, double* terms_dev);
/* 1 and the three ids and the prefactor of d4est_hip_plan_set_estimator (either output may be NULL) when the plan has the estimator,
 * else 0 -- for hosts that check a caller's penalty functions against the plan (the compat library's d4est_estimator_bi_compute) */
int d4est_hip_plan_estimator_info(const d4est_hip_plan_t* plan, int* ids, double* penalty_prefactor);
/* ---- the Laplacian of a field at the quadrature nodes (csrc/d4est_hip_hessian.hip) ---------------------------------------------------
 * d4est_hessian_compute_hessian_trace_of_field_on_quadrature_points (src/dGMath/d4est_hessian.c:270-368).  With R_ai = dr_a/dx_i,
 *   Lap u (q) = sum_b c_b(q) V(D_b u)(q) + sum_ab G_ab(q) V(D_a D_b u)(q),   G_ab = sum_i R_ai R_bi,
 *   c_b = sum_i sum_a R_ai d2rdrdx[b][i][a],   d2rdrdx[m][n][k] = - sum_al R_ml R_an d^2 x_l / dr_a dr_k      (:41-58, :127-138).
 * The nine coefficients per quadrature node depend on the mesh only; one of the three set-up calls forms them once, into plan-owned
 * storage of 9 local_nodes_quad doubles that plan_destroy frees.  Plans that never call them allocate nothing and run as before.
 *   _brick      d^2x/dr dr = 0 (src/Geometry/d4est_geometry_brick.c:8): c = 0, G diagonal; arguments as plan_set_geometry_brick.
 *   _analytic   HESSIAN_ANALYTICAL (:180-226): dx/dr and d^2x/dr dr of the analytic tree map at every quadrature node (Gauss or Lobatto
 *               by the plan's quad_type), dx/dr inverted to R; arguments, flag rules and rejections as plan_set_geometry_analytic.
 *   _numerical  HESSIAN_NUMERICAL (:227-262): d^2 x_d1 / dr_d2 dr_d3 = V(D_d3 D_d2 x_d1) from xyz_lobatto (x | y | z, 3 local_nodes);
 *               R from rst_xyz_quad (the reference's SoA layout, 9 local_nodes_quad) or, when that is NULL, from V(D x) inverted as
 *               plan_set_geometry_numerical forms it.  on_device: both arrays are device (1) or host (0) pointers.
 * All run on the plan's stream with no host synchronisation after the uploads (device arrays handed over with on_device = 1 must
 * stay valid until the stream has passed the call); the numerical form's scratch is released later, by the first apply that finds the
 * set-up kernels finished.  A later set-up call replaces the coefficients (it waits for the earlier one's kernels).  Aborts ([D4EST_HIP_ABORT]) on a NULL plan, a bad
 * type / tree / flag / extent, or a (deg, deg_quad) bucket beyond the apply kernel's LDS: ask d4est_hip_plan_hessian_supported first. */
void d4est_hip_plan_set_hessian_brick(d4est_hip_plan_t* plan, const int* elem_dq, double root_len, const double* extents);
void d4est_hip_plan_set_hessian_analytic(d4est_hip_plan_t* plan, int geom_type, const double* params, const int* elem_tree,
                                         const int* elem_q, const int* elem_dq, double root_len);
void d4est_hip_plan_set_hessian_numerical(d4est_hip_plan_t* plan, const double* xyz_lobatto, const double* rst_xyz_quad, int on_device);
/* 0 none, 1 brick, 2 analytic, 3 numerical */
int d4est_hip_plan_hessian_info(const d4est_hip_plan_t* plan);
/* 1 if every (deg, deg_quad) bucket of the plan fits the apply kernel's LDS, else 0; never aborts on a valid plan.  The kernel holds
 * one element's u, three N x N and six N x NQ planes and three N x NQ tables: 8 (N^3 + 3 N^2 + 9 N NQ) bytes <= 163840 (160 KB),
 * N = deg + 1, NQ = deg_quad + 1.  Every deg <= 19 fits with any deg_quad a plan accepts (N = 20, NQ = 24: 108160 bytes);
 * the first that does not is deg = deg_quad = 23 (165888 bytes). */
int d4est_hip_plan_hessian_supported(const d4est_hip_plan_t* plan);
/* del2u_quad_dev[local_nodes_quad] (OVERWRITTEN) <- u_dev[local_nodes]: replaces the element loop of :291-359, 9 apply_dij and 12
 * interpolations per element.  One workgroup per element per (deg, deg_quad) bucket on the plan's stream, no host synchronisation, no
 * atomics: bit-identical from call to call.  The symmetric pairs D_a D_b = D_b D_a are folded (the reference sums all nine) and the
 * 1-D tables B D and B D D are formed once, so the result differs from the reference's by rounding.  Aborts without a set-up call. */
void d4est_hip_hessian_trace(d4est_hip_plan_t* plan, const double* u_dev, double* del2u_quad_dev);
/* ---- element size parameters and [mesh_parameters] face_h_type / volume_h_type (csrc/d4est_hip_sizes.hip) ----------------------------
 * The ids follow the reference's enums d4est_mesh_face_h_t / d4est_mesh_volume_h_t (src/Mesh/d4est_mesh.h:33-48). */
#define D4EST_HIP_FACE_H_EQ_J_DIV_SJ_QUAD 0                 /* J / sj at every mortar quadrature node (the default) */
#define D4EST_HIP_FACE_H_EQ_J_DIV_SJ_MIN_LOBATTO 1          /* min of J / sj over the face's Lobatto nodes */
#define D4EST_HIP_FACE_H_EQ_J_DIV_SJ_MEAN_LOBATTO 2
#define D4EST_HIP_FACE_H_EQ_J_DIV_SJ_MAX_LOBATTO 3
#define D4EST_HIP_FACE_H_EQ_TREE_H 4                        /* dq / P4EST_ROOT_LEN */
#define D4EST_HIP_FACE_H_EQ_VOLUME_DIV_AREA 5               /* volume of the element / area of its face */
#define D4EST_HIP_FACE_H_EQ_FACE_DIAM 6                     /* largest node distance on the face */
#define D4EST_HIP_FACE_H_EQ_TOTAL_VOLUME_DIV_TOTAL_AREA 7   /* summed over the side's one or four elements */
#define D4EST_HIP_VOL_H_EQ_DIAM 0
#define D4EST_HIP_VOL_H_EQ_CUBE_APPROX 1                    /* diam_volume / sqrt(3) */
/* Which h the device mortar forms (plan_set_mortar_geometry_brick / _analytic) write into hm / hp, and whether diam_volume is scaled:
 * d4est_mesh_calculate_mortar_h (src/Mesh/d4est_mesh.c:689-856, called at :629-644 and :1071-1103) and
 * d4est_mesh_data_compute_volume_diam (:3414-3468).  Call BEFORE the mortar geometry, like d4est_hip_plan_set_sipg; aborts on an id out
 * of range.  A plan without the call behaves as before (J_DIV_SJ_QUAD, DIAM).  With any other face type the mortar forms first compute
 * the size parameters below themselves (ghost elements included), then fill hm with the parameter of the (-) element(s) on face f_m
 * and hp with that of the (+) element(s), in (-) order, on face f_p -- constant over a mortar face; on a hanging face each of the four
 * mortar faces takes the parameter of its own small element on the side that has four and of the one big element (its own parameter,
 * not a half-size child's) on the other.  FACE_H_EQ_FACE_DIAM and FACE_H_EQ_TOTAL_VOLUME_DIV_TOTAL_AREA index the reference's arrays
 * without the ghost offset (:801-802, :841), so what the reference computes across ranks is not defined: on a plan with ghost sides
 * the mortar forms abort for these two.  Host-array factors (d4est_hip_plan_set_mortar_geometry) carry their own hm / hp. */
void d4est_hip_plan_set_h_types(d4est_hip_plan_t* plan, int face_h_type, int volume_h_type);
/* d4est_mesh_init_element_size_parameters_local / _ghost (src/Mesh/d4est_mesh.c:1620-1827) on the device, everything on the Lobatto
 * nodes of the element's own deg; index e for local element e, n_elements + g for ghost g, faces at 6 * index + f: */
#define D4EST_HIP_SIZE_DIAM_VOLUME 0     /* n: max over all node pairs of |x_i - x_j| (:3446-3467), / sqrt(3) with VOL_H_EQ_CUBE_APPROX */
#define D4EST_HIP_SIZE_VOLUME 1          /* n: Lobatto inner product of 1 with J (:1736-1749) */
#define D4EST_HIP_SIZE_AREA 2            /* 6n: the same with sj on the face's Lobatto nodes (:1778-1791) */
#define D4EST_HIP_SIZE_DIAM_FACE 3       /* 6n: max pair distance over the face's nodes (:1794-1807) */
#define D4EST_HIP_SIZE_J_DIV_SJ_MIN 4    /* 6n: min / mean / max of J / sj over the face's Lobatto nodes (:1808-1812), J and sj as */
#define D4EST_HIP_SIZE_J_DIV_SJ_MEAN 5   /*     d4est_mortars_compute_geometric_data_on_mortar gives them with */
#define D4EST_HIP_SIZE_J_DIV_SJ_MAX 6    /*     COMPUTE_NORMAL_USING_JACOBIAN */
/* Brick geometry: elem_dq / root_len / extents as d4est_hip_plan_set_geometry_brick; ghost_dq (order of ghost_deg, needs plan_set_faces)
 * or NULL = local elements only.  Analytic tree maps: the arguments of d4est_hip_plan_set_mortar_geometry_analytic; the three ghost
 * arrays may be NULL likewise.  One launch per degree on the plan's stream, no host synchronisation after the first call's
 * allocations, no atomics: bit-identical from call to call.  Degrees 1 ... 23. */
void d4est_hip_plan_compute_size_parameters_brick(d4est_hip_plan_t* plan, const int* elem_dq, const int* ghost_dq, double root_len,
                                                  const double* extents);
void d4est_hip_plan_compute_size_parameters_analytic(d4est_hip_plan_t* plan, int geom_type, const double* params, const int* elem_tree,
                                                     const int* elem_q, const int* elem_dq, const int* ghost_tree, const int* ghost_q,
                                                     const int* ghost_dq, double root_len);
/* diam_volume and diam_face alone, of the local elements, from their node coordinates xyz_lobatto_dev = x[local_nodes] | y | z
 * (d4est_factors->xyz, any geometry): all the estimator's h needs on a geometry the engine has no map for (:1673-1690, :1794-1807). */
void d4est_hip_plan_compute_diameters(d4est_hip_plan_t* plan, const double* xyz_lobatto_dev);
/* The plan-owned device array `which` (D4EST_HIP_SIZE_*) and its length in doubles; returns 1, or 0 -- leaving the outputs alone --
 * when that array has not been computed.  The pointer stays valid until the plan is destroyed or a later call covers more elements. */
int d4est_hip_plan_size_parameter(const d4est_hip_plan_t* plan, int which, const double** array_dev, long long* count);
/* ---- error norms (csrc/d4est_hip_norms.hip) -----------------------------------------------------------------------------------------
 * The columns of d4est_norms_save (src/IO/d4est_norms.c:380-560), which the drivers write once per AMR level (e.g.
 * src/Problems/ConstantDensityStar/constant_density_star_mgpc_newton_petsc.c:266-287, :453-473): L_2, L_infty, energy_norm and
 * energy_estimator.  Every result is this rank's LOCAL sum / maximum, left on the device: the reduction over ranks stays with the
 * caller (the reference's sc_reduce sits outside the compute functions) and no square root is taken.  skip_dev: int[n_elements], 1 =
 * skip the element (the reference's skip_element_fcn, evaluated by the caller), NULL = skip none.  Everything runs on the plan's
 * stream without host synchronisation; no floating-point atomics, every reduction has a fixed order: bit-identical from call to call.
 *
 * The IP energy norm must be requested BEFORE d4est_hip_plan_set_mortar_geometry or its brick / analytic forms (its per-node face
 * factor w sj pen |n|^2 is formed there, as the estimator's factors are).  penalty_fcn: u_penalty_fcn of d4est_ip_energy_norm_data_t,
 * a penalty_calc_t by the ids of d4est_hip_plan_set_sipg (d4est_laplacian_flux_sipg.c:945-1005); penalty_prefactor: its last
 * argument.  Plans without this call allocate nothing for it and behave as before.  Aborts on an id outside 0..3. */
void d4est_hip_plan_set_energy_norm(d4est_hip_plan_t* plan, int penalty_fcn, double penalty_prefactor);
/* 1 and the id and prefactor of d4est_hip_plan_set_energy_norm (either output may be NULL) when the plan has the request, else 0 */
int d4est_hip_plan_energy_norm_info(const d4est_hip_plan_t* plan, int* penalty_fcn, double* penalty_prefactor);
/* err = |u - u_compare| at the Lobatto nodes (d4est_norms_save, d4est_norms.c:467-468: the absolute value is taken at the nodes, before
 * any interpolation).  u_compare_dev == NULL: err = |u|.  err_dev may alias u_dev. */
void d4est_hip_norms_error(d4est_hip_plan_t* plan, const double* u_dev, const double* u_compare_dev, double* err_dev);
/* d4est_mesh_compute_l2_norm_sqr (src/Mesh/d4est_mesh.c:2299-2374): l2_array_dev[e] = v_e^T M_e v_e = sum_q w J (V v_e)^2 at the
 * element's deg_quad, written for EVERY element (NULL = not wanted); *sum_dev = the sum over the elements that are not skipped.
 * Needs the volume geometry.  Limit: the estimator's residual term's (d4est_hip_estimator_bi). */
void d4est_hip_norm_l2_sqr(d4est_hip_plan_t* plan, const double* v_dev, const int* skip_dev, double* l2_array_dev, double* sum_dev);
/* d4est_norms_fcn_Linfty (d4est_norms.c:64-117): *max_dev = max(0, max_i v_i) over the nodes of the elements that are not skipped --
 * the maximum of the values, not of their magnitudes, from a running maximum that starts at 0, as the reference has it (the drivers
 * pass the error field, which is non-negative). */
void d4est_hip_norm_linfty(d4est_hip_plan_t* plan, const double* v_dev, const int* skip_dev, double* max_dev);
/* d4est_ip_energy_norm_compute (src/dGMath/d4est_ip_energy_norm.c:286-448), squared: sums_dev[4] = volume, boundary, interface and
 * total = (volume + boundary) + interface (:440-443); elem_terms_dev[3 n_elements], term-major in the same order, each local side's
 * part added to its own element (NULL = not wanted).
 *   volume     sum_d sum_q w J (du/dx_d)^2, du/dx_d = sum_i rst_xyz[i][d] V(D_i u)      (d4est_gradient_l2_norm, d4est_gradient.c:71-124)
 *   interface  per local side with an interior mortar: 3 sum_k w_k sj_k pen_k sum_d n_d^2 (u_m - u_p)^2        (:210-270)
 *   boundary   per boundary side: sum_k w_k sj_k pen(deg, h_k, deg, h_k) sum_d n_d^2 u_m^2, no Dirichlet data  (:70-102)
 * As in the reference: the factor 3 (the node value already sums over d and is added once more per direction, :251-268); pen is not
 * squared; a face is visited from both of its local sides (an interior face between local elements counts twice), a ghost side from
 * the local side only; a big hanging side adds its four sub-mortars, a small side its own; degrees as at :216-218.
 * ghost_trace_dev: as for d4est_hip_estimator_bi (NULL = exchanged through the plan_set_comm hooks).  Needs the volume geometry,
 * plan_set_faces, the mortar factors and d4est_hip_plan_set_energy_norm before them; aborts otherwise.  The same on every face path
 * of the operator (the norm forms every side's trace itself, in a buffer of its own).  Limit: the volume term holds u_e and its
 * three derivatives in LDS, (4 N^3 + 3 (N^2 + NQ N) + NQ N + N^2 + 256) doubles <= 160 KB, N = deg + 1, NQ = deg_quad + 1 --
 * p <= 15; a plan beyond it aborts here. */
void d4est_hip_ip_energy_norm_sqr(d4est_hip_plan_t* plan, const double* v_dev, const double* ghost_trace_dev, double* elem_terms_dev,
                                  double* sums_dev);
/* *sum_dev = the fixed-order sum of elem_dev[n_elements] over the elements that are not skipped: with eta2 of d4est_hip_estimator_bi,
 * d4est_norms_fcn_energy_estimator (d4est_norms.c:249-297) */
void d4est_hip_masked_sum(d4est_hip_plan_t* plan, const double* elem_dev, const int* skip_dev, double* sum_dev);
/* total_bndry_nodes of plan_set_faces, and a device volume vector's values at the Lobatto face nodes of every boundary side in the layout
 * of d4est_hip_plan_set_dirichlet_values (side_bndry_stride; d4est_operators_apply_slicer order): where a host evaluates Dirichlet data
 * from the node coordinates (the three coordinate vectors gathered one by one).  On the device: d4est_hip_field_eval (e.g. CDS_PSI) on
 * the three gathered vectors stored x | y | z gives the array d4est_hip_plan_set_dirichlet_values(on_device = 1) takes */
int d4est_hip_plan_bndry_nodes(const d4est_hip_plan_t* plan);
void d4est_hip_plan_boundary_gather(d4est_hip_plan_t* plan, const double* vol_dev, double* bndry_dev);
/* Dirichlet values on the Lobatto face nodes of every boundary side (EVAL_BNDRY_FCN_ON_LOBATTO,
 * d4est_laplacian_flux_sipg.c:80-112); NULL resets to zero (the homogeneous operator used by apply_lhs). */
void d4est_hip_plan_set_dirichlet_values(d4est_hip_plan_t* plan, const double* g_lobatto, int on_device);
/* Robin boundary condition on ALL boundary sides instead of Dirichlet (BC_ROBIN of d4est_laplacian_flux_new;
 * d4est_laplacian_flux_sipg_robin, d4est_laplacian_flux_sipg.c:339-489): the side adds  V^T W sj (coeff u_m - rhs), lifted.
 * The reference evaluates the callbacks robin_coeff / robin_rhs at the boundary mortar quadrature nodes (:388-412); here the
 * caller hands the two arrays, indexed like sj (side_mortar_stride[s] + k, total_mortar_nodes doubles; only the boundary
 * sides' entries are read).  coeff_quad == NULL switches back to Dirichlet.  Call after plan_set_mortar_geometry. */
void d4est_hip_plan_set_robin_values(d4est_hip_plan_t* plan, const double* coeff_quad, const double* rhs_quad, int on_device);
/* Trace buffers.  For every side s the engine keeps u and du/dr_{0,1,2} INTERPOLATED TO THE SIDE'S MORTAR QUADRATURE
 * NODES (what d4est_laplacian_flux_interface forms at src/dGMath/d4est_laplacian_flux.c:635-815, once per side instead
 * of once per flux call): a block of 4 T doubles, T = (deg_mortar_quad+1)^2, field c at c*T, node a + NQ*b in the
 * side's own face ordering.  Local blocks are in side order; the ghost buffer holds one block per local side whose (+)
 * element is a ghost (the (+) element's trace on ITS face), also in side order. */
long long d4est_hip_plan_trace_size(const d4est_hip_plan_t* plan);
long long d4est_hip_plan_ghost_trace_size(const d4est_hip_plan_t* plan);
/* ghost blocks from whole-element ghost data packed in ghost order (what d4est_ghost_data_exchange delivers,
 * src/Mesh/d4est_ghost_data.c:143-256); a trace exchange (RCCL) fills the same buffer directly. */
void d4est_hip_compute_ghost_traces(d4est_hip_plan_t* plan, const double* u_ghost_dev, double* ghost_trace_dev);
/* local traces of u into trace_dev (d4est_hip_plan_trace_size doubles) */
void d4est_hip_compute_face_traces(d4est_hip_plan_t* plan, const double* u_dev, double* trace_dev);
/* Au += mortar terms, given local (and ghost) traces: d4est_laplacian_apply_mortar_matrices (d4est_laplacian.c:285-315) */
void d4est_hip_apply_flux(d4est_hip_plan_t* plan, const double* trace_dev, const double* ghost_trace_dev, double* Au_dev);
/* Au = A u : d4est_laplacian_apply_aij (src/dGMath/d4est_laplacian.c:318-417) = stiffness + traces + flux.
 * ghost_trace_dev may be NULL when the plan has no ghost elements. */
void d4est_hip_apply_aij(d4est_hip_plan_t* plan, const double* u_dev, const double* ghost_trace_dev, double* Au_dev);

/* rhs = M f - A(0): d4est_laplacian_build_rhs_with_strong_bc (src/dGMath/d4est_laplacian.c:16-140), which every Problem calls once per
 * solve: the source term integrated against the test functions -- f given at the Lobatto nodes (f_on_quad = 0: M f,
 * d4est_quadrature_apply_mass_matrix per element, INIT_FIELD_ON_LOBATTO) or at the quadrature nodes (f_on_quad = 1: V^T W J f,
 * d4est_quadrature_apply_galerkin_integral, INIT_FIELD_ON_QUAD) -- minus the Laplacian applied to u = 0 WITH the inhomogeneous boundary
 * data currently set on the plan (d4est_hip_plan_set_dirichlet_values / _set_robin_values: the reference's
 * flux_fcn_data_for_build_rhs; reset them to the homogeneous data of apply_lhs afterwards).  Needs plan_set_faces; on plans with ghost
 * sides the exchange hooks of plan_set_comm.  f_dev / rhs_dev: device arrays; the _host form takes the reference's host vectors. */
void d4est_hip_build_rhs_with_strong_bc(d4est_hip_plan_t* plan, const double* f_dev, int f_on_quad, double* rhs_dev);
void d4est_hip_build_rhs_with_strong_bc_host(d4est_hip_plan_t* plan, const double* f_host, int f_on_quad, double* rhs_host);

/* Linearised nonlinear problems: the reference's apply_lhs is d4est_laplacian_apply_aij plus, per element,
 * d4est_quadrature_apply_fofufofvlilj(u_e; f(x, u0)) added with axpy 1.0 (e.g. constant_density_star_apply_jac,
 * src/Problems/ConstantDensityStar/constant_density_star_fcns.h:777-850 with :528-603).  coeff_quad_dev[local_nodes_quad] = f at
 * the quadrature nodes (device array; its values are CAPTURED by this call -- a plan-owned copy, and w J c pre-combined for the operator
 * kernels, whose volume stage then carries the term for one extra stream of 8 B per node -- so call it again whenever u0, i.e. f,
 * changes; the caller's array is not read afterwards); NULL = pure Laplacian.
 * The term then is part of d4est_hip_apply_lhs, _cheby_iterate, _cg_eigs and _schwarz_smooth; set on a Schwarz subdomain plan
 * (same array: the copies' quad_stride alias it) it is part of the subdomain operator.  d4est_hip_apply_aij stays the Laplacian. */
void d4est_hip_plan_set_lhs_coefficient(d4est_hip_plan_t* plan, const double* coeff_quad_dev);
/* The coefficient form as the plan holds it (read-only, for checks and diagnostics): *c_dev = the plan-owned copy of c, *wjc_dev = the
 * pre-combined w J c of the operator kernels (device, local_nodes_quad doubles each, element e at quad_stride[e]), or NULL while w J c is
 * not formed -- d4est_hip_plan_set_lhs_coefficient and a d4est_hip_plan_linearise on the composed path leave it to the first apply that
 * needs it.  Returns 0 and writes nothing when no coefficient form is set, else 1.  Either output pointer may be NULL.  The arrays live
 * until the plan is destroyed; their contents change with every set_lhs_coefficient / plan_linearise, on the plan's stream. */
int d4est_hip_plan_lhs_coefficient_arrays(const d4est_hip_plan_t* plan, const double** c_dev, const double** wjc_dev);
/* ---- the multigrid MATRIX OPERATOR: the zeroth-order term on the coarse levels (csrc/d4est_hip_mgmatrix.hip) -------------------------
 * With use_matrix_operator = 1 (e.g. constant_density_star_mgpc_newton_petsc.c:591-602) the reference holds the term
 * V^T W J f(x, u0) V as ONE DENSE BLOCK PER ELEMENT on the finest level (d4est_solver_multigrid_matrix_setup_fofufofvlilj_operator,
 * src/Solver/d4est_solver_multigrid_matrix_operator.c:160-245: d4est_quadrature_apply_fofufofvlilj with QUAD_COMPUTE_MATRIX), restricts
 * the blocks level by level with the Galerkin product  sum_children P_c^T M_c P_c  (the restriction callback :6-48 ->
 * d4est_operators_compute_PT_mat_P, src/dGMath/d4est_operators.c:608-667), and the smoother's apply_lhs on every level below the finest
 * adds M_e u_e per element (constant_density_star_apply_jac_add_nonlinear_term_using_matrix,
 * src/Problems/ConstantDensityStar/constant_density_star_fcns.h:485-527, selected at :806-850 when matrix_op->matrix != matrix_at0).
 * Block layout = the reference's matrix_op->matrix: element e's (deg_e+1)^3 x (deg_e+1)^3 row-major block, blocks consecutive in
 * element order (d4est_mesh_get_local_matrix_nodes doubles in all).
 * The plan carries the term in ONE of three forms (each setter replaces the others; NULL switches its own form off):
 *   d4est_hip_plan_set_lhs_coefficient     the coefficient field (finest level; fused into the operator kernels)
 *   d4est_hip_plan_set_lhs_element_blocks  dense blocks (the reference's coarse-level form; 8 (deg+1)^3 bytes per DoF per apply)
 *   d4est_hip_plan_set_lhs_galerkin_chain  the same Galerkin operator applied matrix-free through the transfer objects and the FINE
 *                                          plan's coefficient: T_0^T .. T_{k-1}^T (V^T W J c V) T_{k-1} .. T_0 u -- 8 bytes per fine
 *                                          quadrature node per apply instead of the blocks (cheaper than blocks while
 *                                          fine quadrature nodes < (deg+1)^6 coarse entries, i.e. for up to two h-levels at equal p)
 * all three are part of d4est_hip_apply_lhs, _cheby_iterate, _cg_eigs; coefficient and blocks also of the Schwarz subdomain operator
 * (on a subdomain plan pass block_offset_host: the block of copy k is the block of its mesh element). */
/* d4est_mesh_get_local_matrix_nodes: sum over the elements of (deg+1)^6 */
long long d4est_hip_plan_matrix_nodes(const d4est_hip_plan_t* plan);
/* QUAD_COMPUTE_MATRIX for every element (d4est_quadrature.c:748-760, :1143-1186: the weighted mass matrix applied to the unit vectors,
 * column by column): blocks_dev[d4est_hip_plan_matrix_nodes] = V^T (W J coeff) V per element; coeff_quad_dev == NULL: the mass matrix */
void d4est_hip_compute_weighted_mass_blocks(d4est_hip_plan_t* plan, const double* coeff_quad_dev, double* blocks_dev);
/* blocks_dev stays the caller's (read at every apply); block_offset_host (n_elements, in doubles) or NULL = consecutive */
void d4est_hip_plan_set_lhs_element_blocks(d4est_hip_plan_t* plan, const double* blocks_dev, const long long* block_offset_host);
/* transfers[0]: this plan's level <-> the next finer level, ..., transfers[n-1]: <-> fine_plan's level; fine_plan has its geometry and
 * its coefficient (d4est_hip_plan_set_lhs_coefficient) set; the objects stay the caller's and must outlive the plan's use of them;
 * n_transfers = 0 switches the form off.  Runs on this plan's stream. */
void d4est_hip_plan_set_lhs_galerkin_chain(d4est_hip_plan_t* plan, int n_transfers, d4est_hip_transfer_t* const* transfers,
                                           d4est_hip_plan_t* fine_plan);
/* ---- smoother inner loops (device resident) -----------------------------------------------------------
 * Communication hooks for plans with ghost elements / several ranks (replace the reference's MPI calls:
 * d4est_ghost_data_exchange, src/Mesh/d4est_ghost_data.c:143-256, and sc_allreduce, d4est_solver_cg_eigs.c:181-243).
 * exchange(ctx, phase, trace_dev, ghost_trace_dev): phase 0 = post the face-trace exchange (the local trace buffer is
 * complete on the plan's stream), phase 1 = make the plan's stream wait until ghost_trace_dev is filled.
 * allreduce(ctx, scalars_dev, n): in-place SUM over ranks of n device doubles, ordered on the plan's stream. */
typedef void (*d4est_hip_exchange_fn)(void* ctx, int phase, const double* trace_dev, double* ghost_trace_dev);
typedef void (*d4est_hip_allreduce_fn)(void* ctx, double* scalars_dev, int n);
void d4est_hip_plan_set_comm(d4est_hip_plan_t* plan, d4est_hip_exchange_fn exchange, d4est_hip_allreduce_fn allreduce, void* ctx);
/* Au = A u using the plan-owned trace buffers and the communication hooks (apply_lhs of the Poisson problems,
 * src/Problems/Poisson/poisson_sinx_fcns.h:110-128). */
void d4est_hip_apply_lhs(d4est_hip_plan_t* plan, const double* u_dev, double* Au_dev);
/* d4est_solver_multigrid_smoother_cheby_iterate_aux (src/Solver/d4est_solver_multigrid_smoother_cheby.c:81-176):
 * iter Chebyshev iterations on u for A u = rhs with eigenvalue window [lmin, lmax]; r receives the residual
 * rhs - A u when compute_residual_at_end == 1 (else alpha (rhs - A u) of the last iteration, as in the reference).
 * u, rhs, Au (work), r are device vectors of local_nodes doubles. */
void d4est_hip_cheby_iterate(d4est_hip_plan_t* plan, double* u_dev, const double* rhs_dev, double* Au_dev, double* r_dev, int iter,
                             double lmin, double lmax, int compute_residual_at_end);
/* one fused Chebyshev update  r = alpha (rhs - Au); p = r + beta p; u += p  (smoother_cheby.c:135-153) */
void d4est_hip_cheby_update(d4est_hip_plan_t* plan, int n, const double* rhs_dev, const double* Au_dev, double alpha, double beta,
                            double* r_dev, double* p_dev, double* u_dev);
/* cg_eigs (src/Solver/d4est_solver_cg_eigs.c:116-275): imax CG iterations started from u (which they advance, as in the
 * reference), returns the Gershgorin bound of the Lanczos tridiagonal (use_new selects :36-64 over :9-33).
 * history_host (optional, 2*imax doubles) receives alpha_0..alpha_{imax-1}, beta_0..beta_{imax-1}. */
double d4est_hip_cg_eigs(d4est_hip_plan_t* plan, double* u_dev, const double* rhs_dev, double* Au_dev, int imax, int use_new,
                         double* history_host);
/* ---- Krylov solves on one plan (csrc/d4est_hip_krylov.hip) ---------------------------------------------------------------------
 * The operator is the plan's apply_lhs (zeroth-order term and communication hooks included).  u_dev is the start and receives the
 * solution; Au_dev is work that is left as the reference leaves vecs->Au.  The arithmetic is the reference's, statement for statement;
 * the scalars never leave the device (one-thread kernels form them from device memory), the dot products are two-stage reductions in a
 * fixed order without atomics (bit-identical from run to run), and each reduction point calls the plan's allreduce hook once, with the
 * scalar count of the reference's sc_allreduce.  Vectors and scalars live on the plan (allocated on the first call).
 *
 * d4est_solver_cg_solve (src/Solver/d4est_solver_cg.c:76-197): r = rhs - A u, d = r, delta_0 = r.r; while i < imax and
 * delta > atol^2 + delta_0 rtol^2: alpha = delta / d.Ad, u += alpha d, r -= alpha Ad, beta = r.r / delta, d = r + beta d.  Returns the
 * iteration count; history_host (optional, imax + 1 doubles) receives delta_0, delta_1, ... (count + 1 values); Au_dev ends as A d of the
 * last iteration (A u of the start when no iteration ran).  Iterations are enqueued in batches of D4EST_HIP_TUNE_KRYLOV_CHECK: the
 * scalar kernel raises a device flag when the stop test holds, every vector update after it is a no-op, and the host reads the flag
 * and the count from pinned memory once per batch -- the only host synchronisations.  The allreduce hook is called for every
 * enqueued iteration (1 + 2 per iteration; exactly the reference's count with D4EST_HIP_TUNE_KRYLOV_CHECK = 1).
 * The _host form takes host vectors (u_host in / out, Au_host optional) through the plan's pinned staging, as the other *_host entries. */
int d4est_hip_cg_solve(d4est_hip_plan_t* plan, double* u_dev, const double* rhs_dev, double* Au_dev, int imax, double atol, double rtol,
                       double* history_host);
int d4est_hip_cg_solve_host(d4est_hip_plan_t* plan, double* u_host, const double* rhs_host, double* Au_host, int imax, double atol,
                            double rtol, double* history_host);
/* preconditioner z = B r: device vectors of local_nodes doubles, work ordered on the plan's stream (the reference's pc_apply,
 * src/LinearAlgebra/d4est_krylov_pc.h) */
typedef void (*d4est_hip_pc_fn)(void* ctx, const double* r_dev, double* z_dev);
/* d4est_solver_fcg_solve as the reference builds it (src/Solver/d4est_solver_fcg_improved.c:97-346; CMakeLists.txt:127): r = rhs - A u,
 * tol = atol + rtol |r_0|; for k < imax: v = B r (pc == NULL: the identity, do_not_use_preconditioner = 1), w = A v, one pass for
 * v.r, v.w (and from k = 1 on v.q, r.r; one allreduce of 2 or 4 scalars), the improved-FCG recurrences of rho, gamma, d, q in one
 * scalar kernel and one pass for d, q, u, r; stop when k > 0 and |r_k| <= tol AFTER the update (r_k: the residual before it).  Returns
 * the iteration count (updates made); history_host (optional, imax doubles) receives |r_k| of every iteration (|r_0| at k = 0).  One
 * host synchronisation per iteration (the preconditioner dominates).  Au_dev ends as A u of the start, as in the reference. */
int d4est_hip_fcg_solve(d4est_hip_plan_t* plan, double* u_dev, const double* rhs_dev, double* Au_dev, int imax, double atol, double rtol,
                        d4est_hip_pc_fn pc, void* pc_ctx, double* history_host);
/* ---- nonlinear problems -Laplace(u) + f(x, u) = 0 on one plan (csrc/d4est_hip_nonlinear.hip) -----------------------------------------
 * The reference takes f as a host callback (d4est_xyzu_fcn_t), which a device cannot call.  The callbacks of its shipped nonlinear
 * problems have one shape, f(x, u) = a(x) (b(x) + u)^k with a small integer k, and the Jacobian callback is k a (b + u)^(k-1):
 *   neg_2pi_rho_up1_neg5 / neg_10pi_rho_up1_neg4 (src/Problems/ConstantDensityStar/constant_density_star_fcns.h:347-357 / :334-344):
 *     a = -2 pi rho(x), b = 0, k = 5
 *   two_punctures_neg_1o8_K2_psi_neg7 / two_punctures_plus_7o8_K2_psi_neg8 (src/Problems/TwoPunctures/two_punctures_fcns.h:252-284 /
 *     :288-320): a = -K^2 / 8 (0 inside puncture_eps), b = 1 + sum_n m_n / (2 r_n), k = -7
 * a and b depend on the mesh only: the caller evaluates them once per mesh at the quadrature nodes (d4est_hip_plan_compute_xyz_analytic
 * gives xyz_quad on the device), or leaves it to d4est_hip_plan_set_puncture_term_* / _set_cds_term_* (below, "problem data on the
 * device"), which write a and b of the two shipped problems into the plan from forest coordinates in one kernel.
 *
 * d4est_hip_plan_set_nonlinear_power registers the term.  a_quad_dev, b_quad_dev: local_nodes_quad doubles each, element e at
 * quad_stride[e] (device arrays; their values are CAPTURED by this call into plan-owned copies, as d4est_hip_plan_set_lhs_coefficient
 * captures its coefficient -- call it again when a or b changes; the caller's arrays are not read afterwards).  b_quad_dev == NULL: b = 0.
 * a_quad_dev == NULL switches the term off (it then contributes zero; plan_linearise and newton_solve abort).  |k| <= 16, else abort.
 * The power is |k| multiplications (k < 0: one division of 1 by the product), never pow: the ConstantDensityStar callbacks multiply out,
 * and TwoPunctures' pow(psi^2, 3.5) differs from the product in the last bits only. */
void d4est_hip_plan_set_nonlinear_power(d4est_hip_plan_t* plan, const double* a_quad_dev, const double* b_quad_dev, int k);
/* The real form f(x, u) = a |b + u|^s with Jacobian s a |b + u|^(s-1): Okendon's callbacks pow(u*u, .5*p) and p / pow(u*u, .5*(1.-p)),
 * 0 < p < 1 (src/Problems/Okendon/okendon_fcns.h:114-145).  Capture semantics as set_nonlinear_power (plan-owned copies, b == NULL: 0,
 * a == NULL: the term is off).  Evaluated the reference's way with t = b + V u: a * pow(t*t, 0.5*s) and s * a / pow(t*t, 0.5*(1.-s));
 * nothing is clamped at t = 0, the IEEE result stands (s < 1: the Jacobian is +-inf there, as in the reference).  Setting either form
 * clears the other.  d4est_hip_apply_nonlinear_term, _plan_linearise, _plan_nonlinear_fused, _build_residual and _newton_solve take
 * whichever form is set, with the same one-kernel instances, mixed-degree launch and three-call fallback.  s must be finite. */
void d4est_hip_plan_set_nonlinear_abs_power(d4est_hip_plan_t* plan, const double* a_quad_dev, const double* b_quad_dev, double s);
/* returns 1 and writes s (s may be NULL) when the real form is set, else 0 */
int d4est_hip_plan_nonlinear_exponent(const d4est_hip_plan_t* plan, double* s);
/* out = beta out + V^T W J f(x, V u) per element, beta = 0 or 1: the loop of d4est_quadrature_apply_fofufofvlj followed by axpy 1.0
 * (constant_density_star_fcns.h:360-437 with src/Quadrature/d4est_quadrature.c:776-936).  ONE kernel -- interpolate, pointwise,
 * integrate, no quadrature-sized temporary -- for every (deg, deg_quad) pair d4est_hip_apply_galerkin_integral serves with a one-kernel
 * path (deg_quad = deg <= 19, and deg_quad - deg in {1, 2, 3} at the compiled pairs; mixed-degree plans: the deg_quad = deg <= 7
 * buckets in one launch).  A plan with an element outside these pairs runs d4est_hip_interpolate, a pointwise kernel and
 * d4est_hip_apply_galerkin_integral instead; d4est_hip_plan_nonlinear_fused returns 1 when the plan takes the one-kernel form. */
void d4est_hip_apply_nonlinear_term(d4est_hip_plan_t* plan, const double* u_dev, int beta, double* out_dev);
int d4est_hip_plan_nonlinear_fused(const d4est_hip_plan_t* plan);
/* Sets the plan's zeroth-order coefficient to c = k a (b + V u0)^(k-1) (k = 0: c = 0), the Jacobian callback at u0
 * (constant_density_star_fcns.h:528-603): one kernel writes the plan-owned coefficient and the pre-combined w J c of the operator
 * kernels.  Afterwards the plan is in the state d4est_hip_plan_set_lhs_coefficient(plan, c) leaves, with w J c already formed: the
 * coefficient form replaces element blocks / a Galerkin chain, and the term is part of d4est_hip_apply_lhs, _cheby_iterate, _cg_eigs,
 * the Krylov solves.  d4est_hip_plan_set_lhs_coefficient(plan, NULL) switches it off again.  Aborts if no power term is set. */
void d4est_hip_plan_linearise(d4est_hip_plan_t* plan, const double* u0_dev);
/* out = A u + N(u) - rhs: the reference's build_residual (constant_density_star_fcns.h:439-482) -- d4est_hip_apply_aij with the boundary
 * data currently set on the plan, the nonlinear term with beta = 1, one axpy.  rhs_dev == NULL: no right-hand side; ghost_trace_dev as
 * in d4est_hip_apply_aij. */
void d4est_hip_build_residual(d4est_hip_plan_t* plan, const double* u_dev, const double* ghost_trace_dev, const double* rhs_dev,
                              double* out_dev);
/* called by d4est_hip_newton_solve after every d4est_hip_plan_linearise(plan, u0): where the caller refreshes its preconditioner
 * (d4est_hip_plan_linearise on the coarse plans with the projected u0, block rebuilds, eigenvalue reuse flags) */
typedef void (*d4est_hip_linearise_fn)(void* ctx, const double* u0_dev);
/* d4est_solver_newton_solve (src/Solver/d4est_solver_newton.c:135-365) with d4est_hip_fcg_solve as its Krylov function:
 * F = A u + N(u) - rhs with the Dirichlet data g_lobatto_dev (layout of d4est_hip_plan_set_dirichlet_values, device array, NULL =
 * homogeneous); stop_tol = atol + rtol |F(u)| at the initial guess; while (|F| > stop_tol || itc < imin) && itc < imax: linearise at u,
 * on_linearise(cb_ctx, u) if non-NULL, solve J step = -F from step = 0 by FCG (krylov_imax, krylov_atol, krylov_rtol, pc / pc_ctx as in
 * d4est_hip_fcg_solve), u += step (always the full step, no line search), new F.  Returns 1 if |F| > stop_tol at exit, else 0.
 * The residual carries the inhomogeneous boundary values and the Jacobian the zeroed ones (:120-123): the routine switches the plan's
 * Dirichlet data between g_lobatto_dev and homogeneous and leaves the plan homogeneous, linearised at the last-but-one iterate.
 * |F| comes from the plan's dot product and allreduce hook and is read to the host once per Newton iteration; fnrm_history_host
 * (optional, imax + 1 doubles) receives its + 1 norms, its_host (optional) the iteration count.
 * Single-rank plans only: aborts if the plan has ghost sides.
 * Known limit: a coarse plan that reads this plan's w J c through d4est_hip_plan_set_lhs_galerkin_chain and replays a Chebyshev hipGraph
 * captured under D4EST_HIP_TUNE_GRAPH would replay the previous linearisation; newton_solve is unsupported with that tuning key on chain
 * plans. */
int d4est_hip_newton_solve(d4est_hip_plan_t* plan, double* u_dev, const double* rhs_dev, const double* g_lobatto_dev, double atol,
                           double rtol, int imin, int imax, int krylov_imax, double krylov_atol, double krylov_rtol, d4est_hip_pc_fn pc,
                           void* pc_ctx, d4est_hip_linearise_fn on_linearise, void* cb_ctx, double* fnrm_history_host, int* its_host);
/* pack / unpack of face-trace blocks for the ghost exchange: dst[dst_off[b]+i] = src[src_off[b]+i], i < len[b];
 * the three index arrays are DEVICE arrays of n_blocks entries; runs on the plan's stream.  Replaces the per-mirror
 * memcpy loop of d4est_ghost_data_exchange (src/Mesh/d4est_ghost_data.c:196-236). */
void d4est_hip_copy_blocks(d4est_hip_plan_t* plan, int n_blocks, const double* src_dev, const long long* src_off_dev,
                           double* dst_dev, const long long* dst_off_dev, const int* len_dev);
/* offset / length (in doubles) of side s' block in the local trace buffer, and the offset of the block that side s
 * RECEIVES in the ghost buffer (-1 when its (+) element is not a ghost): the send / receive lists of an exchange */
long long d4est_hip_plan_trace_offset(const d4est_hip_plan_t* plan, int side);
long long d4est_hip_plan_ghost_trace_offset(const d4est_hip_plan_t* plan, int side);
int d4est_hip_plan_trace_block_len(const d4est_hip_plan_t* plan, int side);
/* Plans with hanging faces: a big side owns FOUR blocks (one per sub-mortar, in (-) order), every other side one.  Block `sub` of
 * side `side`: where it sits in the local trace buffer, how long it is, and -- if the element across that mortar is a ghost --
 * where its counterpart is expected in the ghost trace buffer (-1 otherwise).  The counterpart of a big side's block i is the single
 * block of small element i's side; the counterpart of a small side's block is the big element's block
 * d4est_reference_reorient_face_order(f_m, f_p, orientation, side_sub).  With sub = 0 these equal the three functions above on
 * conforming plans. */
int d4est_hip_plan_side_blocks(const d4est_hip_plan_t* plan, int side);
/* d4est_reference_reorient_face_order (dGMath/d4est_reference.c:84-110), face_dim = 2: index in the (+) side's own order of the
 * sub-face that is i in (-) order */
int d4est_hip_reorient_face_order(int f_m, int f_p, int orientation, int i);
/* The side_reorder code of a tree-boundary face pair: what d4est_operators_reorient_face_data derives through
 * p4est_expand_face_transform(min(f_m, f_p), 6*orientation + max(f_m, f_p)) (dGMath/d4est_operators.c:2031-2050):
 * flip0 | flip1 << 1 | (not aligned) << 2.  orientation = p4est's tree_to_face[.] / 6 = p4est_iter_face_info_t::orientation
 * (0 inside a tree).  Lets a C host fill side_reorder without p4est's transform tables. */
int d4est_hip_face_reorder_code(int f_m, int f_p, int orientation);
long long d4est_hip_plan_trace_offset_sub(const d4est_hip_plan_t* plan, int side, int sub);
long long d4est_hip_plan_ghost_trace_offset_sub(const d4est_hip_plan_t* plan, int side, int sub);
int d4est_hip_plan_trace_block_len_sub(const d4est_hip_plan_t* plan, int side, int sub);
/* deterministic device dot product; result_dev is a device double */
void d4est_hip_vec_dot(d4est_hip_plan_t* plan, int n, const double* x_dev, const double* y_dev, double* result_dev);

/* ---- RCCL transport of the ghost exchange (csrc/d4est_hip_comm.hip) --------------------------------------------------------------
 * The C replacement of d4est_ghost_data_exchange (src/Mesh/d4est_ghost_data.c:143-256) and of the sc_allreduce calls of cg_eigs
 * (src/Solver/d4est_solver_cg_eigs.c:181-243), one process per GPU, RCCL over xGMI.  librccl is opened at run time.
 * Communicator: rank 0 calls d4est_hip_comm_get_unique_id, the host broadcasts the d4est_hip_comm_unique_id_bytes() bytes by whatever
 * it has (MPI_Bcast in a d4est build, torch.distributed in the tests), every rank calls d4est_hip_comm_create (ncclCommInitRank;
 * collective; the calling thread's current HIP device is the rank's GPU).
 * One communicator, ONE stream: every RCCL operation of a communicator (the grouped send / receive of the trace exchange, the all-reduce
 * of the CG scalars, d4est_hip_comm_sendrecv / _allreduce_sum) is issued on a stream the communicator owns, with an event in from and an
 * event out to the calling plan's stream -- the order RCCL sees is the host's issue order on every rank, whatever streams the plans use. */
typedef struct d4est_hip_comm d4est_hip_comm_t;
typedef struct d4est_hip_rccl_exchange d4est_hip_rccl_exchange_t;
int d4est_hip_comm_unique_id_bytes(void);
void d4est_hip_comm_get_unique_id(void* id_out);
d4est_hip_comm_t* d4est_hip_comm_create(const void* unique_id, int rank, int world);
/* as above, but returns NULL (and prints the RCCL error) when ncclCommInitRank fails, instead of aborting */
d4est_hip_comm_t* d4est_hip_comm_try_create(const void* unique_id, int rank, int world);
void d4est_hip_comm_destroy(d4est_hip_comm_t* comm);
int d4est_hip_comm_rank(const d4est_hip_comm_t* comm);
int d4est_hip_comm_size(const d4est_hip_comm_t* comm);
/* ncclCommCount of the communicator: the rank count RCCL itself reports (reports / self-checks) */
int d4est_hip_comm_nccl_count(const d4est_hip_comm_t* comm);
/* Wire a plan (faces set) to the communicator: installs C exchange / allreduce hooks (no callback into the host language), so that
 * d4est_hip_apply_lhs, _cheby_iterate, _cg_eigs run on N ranks.  Per neighbouring rank p (peer_rank[p]) the blocks
 * [send_first[p], send_first[p+1]) of (send_off, send_len): offsets / lengths in doubles into the plan's LOCAL trace buffer
 * (d4est_hip_plan_trace_offset_sub / _trace_block_len_sub), and [recv_first[p], recv_first[p+1]) of (recv_off, recv_len) into the GHOST
 * trace buffer (d4est_hip_plan_ghost_trace_offset_sub); both ends list the shared faces in the same canonical order, the totals per
 * peer pair must agree.  Per apply: one pack kernel, one grouped ncclSend / ncclRecv round on a communication stream (beside the
 * volume kernel), one unpack kernel.  All arrays are HOST arrays, copied.  The returned object must outlive the plan's use of it. */
d4est_hip_rccl_exchange_t* d4est_hip_plan_set_rccl_exchange(d4est_hip_plan_t* plan, d4est_hip_comm_t* comm, int n_peers, const int* peer_rank,
                                                            const int* send_first, const long long* send_off, const int* send_len,
                                                            const int* recv_first, const long long* recv_off, const int* recv_len);
void d4est_hip_rccl_exchange_destroy(d4est_hip_rccl_exchange_t* x);
long long d4est_hip_rccl_exchange_count(const d4est_hip_rccl_exchange_t* x);          /* exchanges posted so far */
long long d4est_hip_rccl_exchange_send_doubles(const d4est_hip_rccl_exchange_t* x);   /* doubles sent / received per exchange */
long long d4est_hip_rccl_exchange_recv_doubles(const d4est_hip_rccl_exchange_t* x);
/* one grouped point-to-point round on already packed device buffers (peer p: send_dev[send_first[p]..send_first[p+1]), likewise
 * recv), ordered on the plan's stream -- the whole-element exchanges of the Schwarz smoother; and an in-place SUM over ranks */
void d4est_hip_comm_sendrecv(d4est_hip_comm_t* comm, d4est_hip_plan_t* plan, int n_peers, const int* peer_rank, const double* send_dev,
                             const long long* send_first, double* recv_dev, const long long* recv_first);
void d4est_hip_comm_allreduce_sum(d4est_hip_comm_t* comm, d4est_hip_plan_t* plan, double* scalars_dev, int n);

/* ---- host-pointer entries: the drop-in behind d4est's host double* API (SURVEY.md section 7 "hard part") -----------------------
 * Every reference caller hands over HOST vectors.  These entries take host pointers, move the data through plan-owned
 * persistent pinned staging and device mirrors (allocated once on first use -- no per-call hipMalloc), run the device-resident
 * routine and copy the results back: ONE upload and ONE download per call, however many operator applies happen inside
 * (a 15-iteration Chebyshev smoother call moves 2 vectors up and 2 down for 16 applies).  They return after the results are
 * in the host arrays.  PCIe-inclusive: not the measured path. */
void d4est_hip_apply_stiffness_matrix_host(d4est_hip_plan_t* plan, const double* u_host, double* Au_host);
/* d4est_laplacian_apply_aij on host vectors (the Laplacian alone) / apply_lhs (+ the zeroth-order term, exchange hooks) */
void d4est_hip_apply_aij_host(d4est_hip_plan_t* plan, const double* u_host, double* Au_host);
void d4est_hip_apply_lhs_host(d4est_hip_plan_t* plan, const double* u_host, double* Au_host);
/* d4est_hip_cheby_iterate on host vectors: u_host in/out, r_host out; Au_host (optional, may be NULL) receives the last A u */
void d4est_hip_cheby_iterate_host(d4est_hip_plan_t* plan, double* u_host, const double* rhs_host, double* Au_host, double* r_host,
                                  int iter, double lmin, double lmax, int compute_residual_at_end);
/* d4est_hip_cg_eigs on host vectors: u_host in/out (advanced by the CG iterations, as in the reference) */
double d4est_hip_cg_eigs_host(d4est_hip_plan_t* plan, double* u_host, const double* rhs_host, double* Au_host, int imax, int use_new,
                              double* history_host);
/* only J_quad (mass / galerkin / weighted-mass / inverse-mass kernels need no dr/dx) */
void d4est_hip_plan_set_jacobian(d4est_hip_plan_t* plan, const double* J_quad, int on_device);
/* pinned host memory and stream-ordered copies for C hosts that keep their own staging */
void* d4est_hip_host_alloc(size_t bytes);
void d4est_hip_host_free(void* ptr_host);
void d4est_hip_memcpy_h2d_async(d4est_hip_plan_t* plan, void* dst_dev, const void* src_host, size_t bytes);
void d4est_hip_memcpy_d2h_async(d4est_hip_plan_t* plan, void* dst_host, const void* src_dev, size_t bytes);
void d4est_hip_plan_synchronize(d4est_hip_plan_t* plan);

/* ---- hp-multigrid inter-grid transfer ---------------------------------------------------
 * The V-cycle's restriction / prolongation callbacks (src/Solver/d4est_solver_multigrid_callbacks.h:100-200, :245-330) walk the
 * coarse grid and call, per coarse element, d4est_operators_apply_p_prolong / _hp_prolong (prolongation) or their transposes
 * (restriction of residuals; src/dGMath/d4est_operators.c:1091-1132, :1689-1749).  A transfer object is that walk as a flat list:
 * item k has hrefine[k] = 0 (one fine element of degree degh[8k] <-> coarse element of degree degH[k]; equal degrees copy) or 1
 * (eight children in z-order with degrees degh[8k..8k+7] <-> their parent); d4est's third case (an element that is not coarsened,
 * copied child by child) is hrefine = 0 with degh = degH.  Both vectors are element-ordered and contiguous in item order, like the
 * reference's fine_stride / coarse_stride.  degh >= degH as the reference asserts (d4est_operators.c:379).  Degrees up to 17: the
 * restriction kernels hold three (deg+1)^3 fields in the 160 KB LDS; d4est_hip_transfer_create aborts above that. */
d4est_hip_transfer_t* d4est_hip_transfer_create(int n_items, const int* hrefine, const int* degH, const int* degh);
void d4est_hip_transfer_destroy(d4est_hip_transfer_t* t);
void d4est_hip_transfer_set_stream(d4est_hip_transfer_t* t, void* hip_stream);
long long d4est_hip_transfer_coarse_nodes(const d4est_hip_transfer_t* t);
long long d4est_hip_transfer_fine_nodes(const d4est_hip_transfer_t* t);
/* x_fine = P x_coarse (d4est_operators_apply_p_prolong / _hp_prolong per item) */
void d4est_hip_transfer_prolong(d4est_hip_transfer_t* t, const double* x_coarse_dev, double* x_fine_dev);
/* u_fine += P x_coarse in ONE kernel: the coarse-grid correction of the V-cycle (d4est_solver_multigrid.c:1182-1250: copy err -> rres,
 * prolong into the fine rres, axpy 1.0 into u) without the fine-level intermediate.  Every entry of P x_coarse is rounded to a double
 * before it is added, so the result is bit-identical to d4est_hip_transfer_prolong into a scratch vector followed by u_fine += scratch. */
void d4est_hip_transfer_prolong_add(d4est_hip_transfer_t* t, const double* x_coarse_dev, double* u_fine_dev);
/* x_coarse = P^T x_fine (d4est_operators_apply_p_prolong_transpose / _hp_prolong_transpose per item; overwrites x_coarse) */
void d4est_hip_transfer_restrict(d4est_hip_transfer_t* t, const double* x_fine_dev, double* x_coarse_dev);
/* x_coarse = L2 projection of x_fine (d4est_operators_apply_p_restrict / _hp_restrict per item, src/dGMath/d4est_operators.c:1205-1230,
 * :1275-1297: M_H^-1 P^T M_h, children summed; the restriction of FIELDS, e.g. of the solution when the mesh is coarsened) */
void d4est_hip_transfer_project(d4est_hip_transfer_t* t, const double* x_fine_dev, double* x_coarse_dev);
/* Which kernels serve this transfer (read-only; launches nothing): the work lists of the prolongation (which = 0), of the restriction and
 * projection (1) and of the fused Galerkin term (2: built when a one-transfer chain is set on a plan, empty before and when the chain runs
 * unfused), one text line "NH dmax nc n cg" per list.  NH: coarse nodes per direction of the compile-time kernel, 0 for the generic
 * runtime-size kernels; dmax: the list's largest fine-minus-coarse size (instances exist for 0, 1 and 3: a list with 2 runs the 3);
 * nc: children per coarse element (restriction / Galerkin lists: 1 or 8); n: entries; cg: child groups per workgroup the launch uses.
 * Writes at most len - 1 characters and a NUL into buf (may be NULL), returns the full length. */
int d4est_hip_transfer_describe(const d4est_hip_transfer_t* t, int which, char* buf, int len);

/* The restriction of the multigrid matrix operator's element blocks through this transfer's item list (the restriction callback of
 * src/Solver/d4est_solver_multigrid_matrix_operator.c:6-48 for every coarse element): coarse block k = sum_c P_c^T M_c P_c over the item's
 * children (d4est_operators_compute_PT_mat_P, src/dGMath/d4est_operators.c:608-667); blocks consecutive in traversal order on both grids
 * (fine_matrix_stride / coarse_matrix_stride); an item that is a copy (hrefine 0, degh = degH) copies its block.
 * literal_window = 0: the Galerkin product as written above.  literal_window = 1: the reference's arithmetic to the letter -- at :651 it
 * takes child c's left factor as a window of the transposed STACKED prolongation (&PT[stride_P] read as (degH+1)^3 x (degh_c+1)^3), which
 * equals P_c^T for one child but interleaves rows of different children for eight; a d4est build therefore holds THAT block on
 * h-coarsened levels (non-symmetric).  The chain form above is the exact product by construction. */
long long d4est_hip_transfer_fine_matrix_nodes(const d4est_hip_transfer_t* t);
long long d4est_hip_transfer_coarse_matrix_nodes(const d4est_hip_transfer_t* t);
void d4est_hip_transfer_galerkin_blocks(d4est_hip_transfer_t* t, const double* fine_blocks_dev, double* coarse_blocks_dev, int literal_window);

/* ---- the hp-multigrid V-cycle, solve and preconditioner (csrc/d4est_hip_multigrid.hip) ---------------------------------------------
 * d4est_solver_multigrid_vcycle / d4est_solver_multigrid_solve (src/Solver/d4est_solver_multigrid.c:751-1348, :1420-1506) with the
 * Chebyshev smoother driver (d4est_solver_multigrid_smoother_cheby.c:222-376), the CG and Chebyshev bottom solvers
 * (d4est_solver_multigrid_bottom_solver_cg.c:48-198, _cheby.c:59-113) and d4est_krylov_pc_multigrid_apply
 * (src/Solver/d4est_krylov_pc_multigrid.c:40-77) on a device-resident hierarchy.  Levels as in the reference: 0 = bottom (coarsest) ...
 * n_levels - 1 = top (finest).  plans[l] is level l's operator -- geometry, faces, the zeroth-order term in whichever form
 * (coefficient on the top, element blocks or Galerkin chain below), communication hooks: all the caller's, with homogeneous boundary
 * data on every level (build_rhs_with_strong_bc moved g into rhs) -- and transfers[l] connects level l (coarse) and l + 1 (fine).  A d4est
 * host builds transfers[l] from coarse_grid_refinement[] of the reference's V-cycle (hrefine, degH, degh per coarse element; hrefine = 2,
 * an element that is not coarsened, is a copied item: hrefine 0 with degh = degH).  The objects stay the caller's and must outlive this
 * one.  create propagates the finest plan's stream to every plan and transfer (ordering between levels is stream order and nothing else)
 * and allocates the workspace once: one arena per vector kind (Ae, err, res below the top; rres on every level) laid out like the
 * reference's *_at0 arrays with stride_to_fine_data.  It aborts, with the message of the code, unless d4est_hip_multigrid_check
 * returns 0: 1 n_levels < 2 (the reference's abort at :1435-1438), 2 a NULL entry, 3 a transfer whose coarse / fine node counts are not
 * those of its two plans.
 * The smoother is the Chebyshev driver or the Schwarz smoother (d4est_solver_multigrid_smoother_schwarz.c:89-204, the caller's Schwarz
 * handle per level); the bottom solver is CG, Chebyshev or reuse_smoother (d4est_solver_multigrid_bottom_solver_reuse_smoother.c:20-39).
 * On plans with ghost sides the Schwarz handles must carry an element exchange (d4est_hip_schwarz_set_element_exchange).
 * Not part of the object: the PETSc bottom solver, the reference-named compat entry points, hierarchies coarsened across ranks (every level's hooks
 * are simply used).  The object never changes a plan's tuning: a caller may set D4EST_HIP_TUNE_GRAPH (key 9) on launch-bound coarse
 * plans itself. */
typedef struct d4est_hip_multigrid d4est_hip_multigrid_t;
int d4est_hip_multigrid_check(int n_levels, d4est_hip_plan_t* const* plans, d4est_hip_transfer_t* const* transfers);
d4est_hip_multigrid_t* d4est_hip_multigrid_create(int n_levels, d4est_hip_plan_t* const* plans, d4est_hip_transfer_t* const* transfers);
void d4est_hip_multigrid_destroy(d4est_hip_multigrid_t* mg);
/* every plan and transfer of the hierarchy onto this stream (hipStream_t as void*) */
void d4est_hip_multigrid_set_stream(d4est_hip_multigrid_t* mg, void* hip_stream);
/* The [mg_smoother_cheby] keys of the reference's input file, same meaning.  Per smoother call: when eigs_compute is set -- at PRE_V it
 * is 0 only if reuse_fromlastvcycle and vcycle_index != 0, at UPV_PRE_SMOOTH it is 0 if reuse_fromdownvcycle or (reuse_fromlastvcycle
 * and vcycle_index != 0) -- cg_eigs runs cheby_eigs_cg_imax iterations FROM THE CURRENT ITERATE, WHICH IT ADVANCES (as in the reference;
 * with cheby_use_zero_guess_for_eigs from a zero scratch vector instead) and eigs[level] = bound * cheby_eigs_max_multiplier; then
 * cheby_imax iterations on the window [eigs[level] / ratio, eigs[level]], the residual rhs - A u left for the restriction.
 * Returns 0, or -- leaving the object without a smoother -- 1 for cheby_use_zero_guess_for_eigs = 1 without
 * cheby_eigs_reuse_fromdownvcycle = 1 (the reference's abort at smoother_cheby.c:313-318), 2 for a negative cheby_imax,
 * cheby_eigs_cg_imax < 1 or a ratio that is not positive. */
int d4est_hip_multigrid_set_smoother_cheby(d4est_hip_multigrid_t* mg, int cheby_imax, int cheby_eigs_cg_imax, double cheby_eigs_lmax_lmin_ratio,
                                           double cheby_eigs_max_multiplier, int cheby_eigs_reuse_fromdownvcycle,
                                           int cheby_eigs_reuse_fromlastvcycle, int cheby_use_new_cg_eigs, int cheby_use_zero_guess_for_eigs);
/* [mg_smoother_schwarz] smoother_iterations and the three [d4est_solver_schwarz] CG options (as d4est_hip_schwarz_smooth takes them).
 * schwarz_on_level[l] (n_levels entries) is the caller's Schwarz handle for plans[l], built as for d4est_hip_schwarz_smooth; it stays
 * the caller's and must outlive the object.  Entry 0 may be NULL unless the reuse_smoother bottom solver is selected.  Per smoother
 * call: smoother_iterations times { r = rhs - A u; schwarz_iterate(u, r) }, then r = rhs - A u; r is the operator's output vector as
 * in the reference (vecs->Au = r), the cycle's Au is left alone.  Inside this loop no iterate ends with a host read; what remains is
 * the look at the "still iterating" counter before the first and then every 8th subdomain sweep.  Environment
 * D4EST_HIP_SCHWARZ_FUSED_RESIDUAL=1, read when the Schwarz handle is created, forms the residual of the intermediate iterations in
 * the subdomain CG's start kernel instead of writing it to r first (same numbers, bit for bit; off by default because it measured no
 * faster; D4EST_HIP_SCHWARZ_UNFUSED_RESIDUAL=1 forces the two kernels).
 * d4est_hip_schwarz_get_info works after a cycle.  The smoother has no eigenvalue state: d4est_hip_multigrid_get_info reports -1.
 * Returns 0, or -- leaving the object without a smoother -- 1 for a NULL entry on a level >= 1, 2 for a handle whose mesh node count is
 * not plans[l]'s (a sharded handle: its own node count), 3 for a handle whose subdomain plan is not on the hierarchy's stream, 4 for a
 * plan with ghost sides and a handle without an element exchange (or a plan without faces), 5 for subdomain options <= 0 (d4est_solver_schwarz_subdomain_solver_cg.c:86-92) or a negative smoother_iterations. */
int d4est_hip_multigrid_set_smoother_schwarz(d4est_hip_multigrid_t* mg, d4est_hip_schwarz_t* const* schwarz_on_level, int smoother_iterations,
                                             int subdomain_iter, double subdomain_atol, double subdomain_rtol);
/* One call of the current smoother on one level, as the V-cycle makes it: smooth A_level u = rhs, r = rhs - A u of the final iterate on
 * exit (u, rhs, Au, r: device vectors of plans[level]'s local_nodes; Au is work).  For a host that drives its own cycle and for tests. */
void d4est_hip_multigrid_smooth_level(d4est_hip_multigrid_t* mg, int level, double* u_dev, const double* rhs_dev, double* Au_dev,
                                      double* r_dev);
/* [mg_bottom_solver_reuse_smoother]: the bottom solve is the current smoother on level 0 (smoother->smooth(..., r, 0)).  The Chebyshev
 * smoother takes eigs[0] by its own rules (eigs_compute as PRE_V left it); the Schwarz smoother needs schwarz_on_level[0]. */
void d4est_hip_multigrid_set_bottom_solver_reuse_smoother(d4est_hip_multigrid_t* mg);
/* [mg_bottom_solver_cg]: d4est_hip_cg_solve on plans[0] from err = 0 */
void d4est_hip_multigrid_set_bottom_solver_cg(d4est_hip_multigrid_t* mg, int bottom_imax, double bottom_atol, double bottom_rtol);
/* [mg_bottom_solver_cheby]: cg_eigs from the current iterate on every call, the multiplier, cheby_imax iterations */
void d4est_hip_multigrid_set_bottom_solver_cheby(d4est_hip_multigrid_t* mg, int cheby_imax, int cheby_eigs_cg_imax, double lmax_lmin_ratio,
                                                 double max_multiplier, int use_new_cg_eigs);
/* 1 once a smoother and a bottom solver are set (reuse_smoother: and the smoother covers level 0), else 0; vcycle / solve / pc_apply
 * abort while it is 0 */
int d4est_hip_multigrid_ready(const d4est_hip_multigrid_t* mg);
/* One V-cycle on A u = rhs (device vectors of the top level's local_nodes; Au is work, left as the last smoother call leaves it).
 * vcycle_index is vcycle_num_finished as the eigenvalue-reuse rules see it.  Down, level = top ... 1: err = 0, smooth (u, rhs, Au) on
 * the top / (err, res, Ae) below it, res_{level-1} = P^T (rhs - A u).  Bottom: err_0 = 0, the bottom solver.  Up, level = 0 ... top - 1:
 * u_{level+1} += P err_level (d4est_hip_transfer_prolong_add; environment D4EST_HIP_MG_UNFUSED_CORRECTION=1, read at create: prolong
 * and add as two kernels, same numbers), smooth.  No host synchronisation beyond those of cg_eigs / cg_solve. */
void d4est_hip_multigrid_vcycle(d4est_hip_multigrid_t* mg, double* u_dev, const double* rhs_dev, double* Au_dev, int vcycle_index);
/* vcycle_r2_local of the last V-cycle: |rhs - A u|^2 of the top level's final smoother call (:1330-1332), a fixed-order two-stage
 * reduction without atomics (bit-identical from run to run); reads the device scalar (synchronises the stream) */
double d4est_hip_multigrid_vcycle_r2(d4est_hip_multigrid_t* mg);
/* d4est_solver_multigrid_solve: r2_0 = |rhs - A u|^2 (one apply, one call of the finest plan's allreduce hook with 1 scalar), stoptol =
 * rtol^2 r2_0 + atol^2; while n < vcycle_imax and r2 > stoptol: one V-cycle with index n, r2 = allreduce(vcycle_r2) (one hook call),
 * n++, break if sqrt(r2 / r2_last) >= 0.99, else r2_last = r2.  The host reads r2 once per cycle.  Returns the V-cycles done;
 * history_host (optional, vcycle_imax + 1 doubles) receives the global r2 before the first and after each cycle. */
int d4est_hip_multigrid_solve(d4est_hip_multigrid_t* mg, double* u_dev, const double* rhs_dev, double* Au_dev, int vcycle_imax,
                              double vcycle_atol, double vcycle_rtol, double* history_host);
/* d4est_krylov_pc_multigrid_apply as a d4est_hip_pc_fn (ctx = the multigrid object): z = 0, an Au of the object's own, then
 * d4est_hip_multigrid_solve(z, rhs = r) with the parameters stored by d4est_hip_multigrid_set_pc (default: one V-cycle, atol = rtol = 0).
 * A d4est host binds d4est_krylov_pc_t.pc_apply to it; d4est_hip_fcg_solve takes it as pc with pc_ctx = the object. */
void d4est_hip_multigrid_set_pc(d4est_hip_multigrid_t* mg, int vcycle_imax, double vcycle_atol, double vcycle_rtol);
void d4est_hip_multigrid_pc_apply(void* mg, const double* r_dev, double* z_dev);
/* eigs_host[n_levels]: the spectral bound last used per level, after the multiplier (-1: none yet, and on every level with the
 * Schwarz smoother; level 0 holds the bottom Chebyshev solver's bound when that solver is set, the smoother's own under
 * reuse_smoother); the V-cycles of the last solve; the bottom solver's iterations in the last cycle (CG: iterations made; Chebyshev:
 * cheby_imax; reuse_smoother: 0).  Any output may be NULL. */
void d4est_hip_multigrid_get_info(const d4est_hip_multigrid_t* mg, double* eigs_host, int* vcycles, int* bottom_iterations);

/* ---- additive Schwarz smoother ------------------------------------------------------------
 * Replaces d4est_solver_schwarz_iterate (src/Solver/d4est_solver_schwarz.c:172-285) with its CG subdomain solver
 * (src/Solver/d4est_solver_schwarz_subdomain_solver_cg.c:101-249) and the Laplacian subdomain operator
 * (src/Solver/d4est_solver_schwarz_laplacian_ext.c:167-358), all subdomains of the rank at once.
 *
 * Metadata in the reference's terms (src/Solver/d4est_solver_schwarz_metadata.h:19-62), flattened: subdomain i owns the entries
 * [sub_first[i], sub_first[i+1]) of sub_elem (local element id of each subdomain element, sorted by (tree, quadid) like
 * d4est_solver_schwarz_metadata.c:447-455), sub_faces[3k..3k+2] (element_metadata.faces: the faces of the subdomain element that
 * touch the core, -1 = none; all -1 on the core) and sub_core_faces[3k..3k+2] (element_metadata.core_faces, the mirrored faces).
 * num_nodes_overlap is the [d4est_solver_schwarz] input of that name (1 .. min deg + 1).
 *
 * subdomain_plan is a plan whose elements are the subdomain elements in that order (deg / deg_quad of the mesh element; quad_stride
 * and the mortar strides of the mesh element, so the geometric factors are the mesh's own arrays; neighbours = the copies inside the
 * same subdomain; a face whose neighbour is outside the subdomain = a ghost side, which the smoother feeds with a zero trace: the
 * reference's zero_and_skip rule, src/dGMath/d4est_laplacian_flux.c:486-520, :944-962; domain boundary = -1 with homogeneous
 * Dirichlet data).  disco4est_amd/schwarz.py builds it; the plan stays owned by the caller and must outlive the handle.
 * Hanging 1 <-> 4 faces: the copies carry the mesh's plan_set_hanging arrays, group / neighbour entries remapped the same way.
 * Several ranks: the mesh handed over is the rank's EXTENDED mesh (own elements followed by the ghost layer, P4EST_CONNECT_FULL), subdomains
 * exist for the own elements only; the residual of the ghost-layer elements arrives by a whole-element exchange before the subdomain solves
 * and their part of u (the corrections) is sent back to the owners afterwards.  With d4est_hip_schwarz_set_element_exchange (below) the
 * handle makes both exchanges itself and every entry that takes mesh vectors works on the rank's OWN nodes; without it the entries are
 * extended-mesh entries and the exchanges are the host's (disco4est_amd/schwarz.py: SchwarzShard, parallel.ElementSchedule). */
d4est_hip_schwarz_t* d4est_hip_schwarz_create(d4est_hip_plan_t* subdomain_plan, int n_subdomains, const int* sub_first,
                                              const int* sub_elem, const int* sub_faces, const int* sub_core_faces,
                                              int num_nodes_overlap, int n_mesh_elements, const int* mesh_deg,
                                              const int* mesh_nodal_stride);
void d4est_hip_schwarz_destroy(d4est_hip_schwarz_t* sz);
/* schwarz_metadata->nodal_size / ->restricted_nodal_size (d4est_solver_schwarz_metadata.c:459-520) */
long long d4est_hip_schwarz_nodal_size(const d4est_hip_schwarz_t* sz);
long long d4est_hip_schwarz_restricted_nodal_size(const d4est_hip_schwarz_t* sz);
/* How many element copies have their rows of the subdomain operator kept as small dense blocks (read off the matrix-free operator by
 * probing, once, on first use) instead of being applied element by element: on a conforming one-degree mesh with a small overlap
 * the corner copies (8 of 27 per subdomain; 8 restricted nodes of 512 at overlap 2, p = 7).  0 when the optimisation does not apply
 * (mixed degrees, hanging faces, blocks above 8 KB) or is switched off (D4EST_HIP_SCHWARZ_CONDENSE=0); results agree to rounding. */
int d4est_hip_schwarz_condensed_copies(d4est_hip_schwarz_t* sz);
/* d4est_solver_schwarz_convert_nodal_field_to_restricted_field_over_subdomains (src/Solver/d4est_solver_schwarz_helpers.c:123-155).
 * Fields over the subdomains have nodal_size entries (whole elements); the restricted field is stored in place, zero outside the
 * overlap nodes (restrict-transpose, helpers.c:210-239, is then the identity). */
void d4est_hip_schwarz_restrict_field(d4est_hip_schwarz_t* sz, const double* field_dev, double* out_over_subdomains_dev);
/* d4est_solver_schwarz_laplacian_ext_apply_over_subdomain for every subdomain: out = R A R^T in (in must be zero outside the overlap) */
void d4est_hip_schwarz_apply_over_subdomains(d4est_hip_schwarz_t* sz, const double* in_dev, double* out_dev);
/* d4est_solver_schwarz_compute_correction + ..._add_corrections (helpers.c:421-451, transfer_ghost_data.c:97-120):
 * u += sum over subdomains of weights * du, added in ascending subdomain order */
void d4est_hip_schwarz_add_correction(d4est_hip_schwarz_t* sz, const double* du_over_subdomains_dev, double* u_dev);
/* d4est_solver_schwarz_iterate: u += correction of the residual r = rhs - A u (both mesh vectors on the device); the three
 * [d4est_solver_schwarz] CG options as arguments.  Returns the number of batched CG sweeps (= the largest iteration count) of this
 * rank.  On a sharded handle (element exchange set) u and r are vectors of the rank's OWN nodes and the call is collective. */
int d4est_hip_schwarz_iterate(d4est_hip_schwarz_t* sz, double* u_dev, const double* r_dev, int subdomain_iter, double subdomain_atol,
                              double subdomain_rtol);
/* The multigrid smoother built on it, d4est_solver_multigrid_smoother_schwarz (src/Solver/d4est_solver_multigrid_smoother_schwarz.c:98-196):
 * smoother_iterations times { r = rhs - A u; schwarz_iterate(u, r) }, then r = rhs - A u.  mesh_plan is the plan of the mesh itself (faces
 * set, homogeneous Dirichlet data, same stream as the subdomain plan).  On several ranks mesh_plan is the rank's own plan -- its
 * apply_lhs hooks do the trace exchange -- and the handle must carry an element exchange for the whole-element exchanges around the
 * subdomain solves (without one this entry is for one rank). */
void d4est_hip_schwarz_smooth(d4est_hip_schwarz_t* sz, d4est_hip_plan_t* mesh_plan, double* u_dev, const double* rhs_dev, double* r_dev,
                              int smoother_iterations, int subdomain_iter, double subdomain_atol, double subdomain_rtol);
/* schwarz->subdomain_solve_iterations / _residuals of the last iterate (d4est_solver_schwarz.c:259-260), host arrays of n_subdomains */
void d4est_hip_schwarz_get_info(d4est_hip_schwarz_t* sz, int* final_iter_host, double* final_res_host);
/* blocking host reads of device counters the handle has made so far: the look at the "still iterating" counter before the first and then
 * every 8th subdomain sweep, and the sweep count the public d4est_hip_schwarz_iterate returns.  The exchange ends add none. */
long long d4est_hip_schwarz_host_reads(const d4est_hip_schwarz_t* sz);

/* ---- the subdomain solver: batched CG (the default) or restarted GMRES (csrc/d4est_hip_schwarz_gmres.hip) -----------------------------
 * [d4est_solver_schwarz] subdomain_solver = cg | gmres with subdomain_inner_iter.  kind 0: the CG of
 * d4est_solver_schwarz_subdomain_solver_cg.c, subdomain_inner_iter is ignored and any GMRES workspace is freed.  kind 1:
 * d4est_solver_schwarz_subdomain_solver_gmres (src/Solver/d4est_solver_schwarz_subdomain_solver_gmres.c:165-443) with restart length
 * mr = subdomain_inner_iter.  A handle on which this was never called runs CG.  Returns
 *   0  ok
 *   1  unknown kind ("Not a supported subdomain solver", d4est_solver_schwarz_subdomain_solver.c:87; ksp has no device form)
 *   2  mr <= 0 (subdomain_inner_iter is a required input, subdomain_solver_gmres.c:88; the options check of :93-97 leaves it out and a
 *      restart length <= 0 reads g[k] / h[k][k] of an empty cycle at :399)
 *   3  mr is larger than the smallest restricted_nodal_size of a subdomain (the reference aborts with "nodes < mr", :203-205)
 *   4  mr > D4EST_HIP_SCHWARZ_GMRES_MAX_MR = 128.  The cap keeps what one subdomain carries between kernels -- the rotated upper triangle
 *      of h, c, s, g and y: 70 KB at the cap -- below half of a CU's 160 KB of LDS; the kernels themselves stage one column (Arnoldi)
 *      or one row (back-substitution) of it at a time, 2 KB at the cap.  It admits the full GMRES of the smallest corner subdomain
 *      at p = 2, overlap 2 (125 restricted nodes).
 * and leaves the handle as it was on a non-zero code.  Every entry that solves subdomain problems follows the choice without a change of
 * signature: d4est_hip_schwarz_iterate and _smooth, the V-cycle's Schwarz smoother, the reuse_smoother bottom solver, d4est_hip_pc_schwarz_*,
 * on one rank and on sharded handles.  Under GMRES subdomain_iter is the reference's itr_max (restart cycles), subdomain_atol / _rtol are
 * tol_abs / tol_rel and a subdomain stops when rho <= rho_tol && rho <= tol_abs (:391, :418 -- both must hold);
 * d4est_hip_schwarz_get_info returns final_iter = itr_used (inner steps made) and final_res = rho (:441-442);
 * d4est_hip_schwarz_iterate returns the number of batched operator applies it made (mr per restart cycle plus one at the start of every
 * cycle but the first, where x = 0), a count the host keeps itself; d4est_hip_schwarz_host_reads counts one look at the "still
 * iterating" counter per restart cycle after the first.
 * Deviation: the reference divides by rho = |rhs - A x| unguarded (:281), so a subdomain whose residual is exactly zero at a cycle start
 * becomes NaN there; here it is finished: x unchanged, final_res = 0, final_iter as reached.
 * The workspace ((mr + 1) basis vectors of nodal_size doubles and, per subdomain, (mr + 1) mr + 2 mr + (mr + 1) + 2 doubles and 2 ints)
 * is allocated here, never by an iterate, and freed by kind 0 and by destroy; _subdomain_solver reports kind, mr (0 under CG) and its
 * size in bytes (0 under CG); any of the three pointers may be NULL. */
#define D4EST_HIP_SCHWARZ_GMRES_MAX_MR 128
int d4est_hip_schwarz_set_subdomain_solver(d4est_hip_schwarz_t* sz, int kind, int subdomain_inner_iter);
void d4est_hip_schwarz_subdomain_solver(const d4est_hip_schwarz_t* sz, int* kind, int* subdomain_inner_iter, long long* workspace_bytes);

/* ---- the smoother on N ranks: the two whole-element exchanges of an iterate inside the handle --------------------------------------------
 * d4est_ghost_data_exchange of the residual before the subdomain solves (src/Solver/d4est_solver_schwarz.c:197-203; direction 0, owners
 * -> ghost copies) and d4est_solver_schwarz_transfer_ghost_data_and_add_corrections afterwards
 * (src/Solver/d4est_solver_schwarz_transfer_ghost_data.c:60-176; direction 1, ghost copies -> owners).
 *
 * sz was created on the rank's extended mesh: elements [0, n_own_elements) are the rank's own, the rest its ghost layer; subdomains exist
 * for the own elements only.  peer_rank is ascending.  send_elem[send_first[p] .. send_first[p+1]) are the own elements that lie in peer
 * p's ghost layer, recv_elem[recv_first[p] .. recv_first[p+1]) the ghost-layer elements that peer p owns, both in ascending global id on
 * both ends (parallel.ElementSchedule), so no metadata is exchanged; the block of an element is its (deg + 1)^3 doubles at its
 * mesh_nodal_stride, as create() copied them.  All arrays are HOST arrays, copied.  Aborts on an index on the wrong side of
 * n_own_elements, a ghost-layer element that no peer or more than one peer owns, an own element listed twice for one peer, and peers
 * that are not strictly ascending.
 *
 * Buffers: in direction 0 send_dev holds the send_elem blocks, peer after peer, and recv_dev the recv_elem blocks; in direction 1 the
 * roles swap (send_dev: the recv_elem blocks, recv_dev: the send_elem blocks).  d4est_hip_schwarz_exchange_first(sz, direction,
 * send_or_recv (0 send, 1 recv), p) is the first double of peer p's segment in that buffer, p = n_peers its total length.
 * Hook contract: on entry send_dev is complete as far as the subdomain plan's stream is concerned; on return recv_dev must be filled
 * as far as that stream is concerned (stream-ordered work or a blocking wait, the transport's choice; a collective must not wait on the
 * host without a time limit).  Every iterate calls the hook exactly once per direction on every rank, also on a rank without
 * subdomains and whatever the subdomain solves did.  fn == NULL removes the exchange (and frees its buffers).
 *
 * With an exchange set: d4est_hip_schwarz_iterate, _smooth, the V-cycle's Schwarz smoother, the reuse_smoother bottom solver and
 * d4est_hip_pc_schwarz_* take vectors of the OWN nodes (the prefix of the extended vector) and the rank's own plan as mesh_plan (ghost
 * sides, trace exchange hooks set); the codes of d4est_hip_multigrid_set_smoother_schwarz then read: 2 the plan's local_nodes is not the
 * handle's own node count, 4 the plan has no faces.  _restrict_field, _apply_over_subdomains and _add_correction stay extended-mesh
 * entries.  One iterate on the device: (1) one kernel sets the own part of the extended residual and writes the send blocks -- under
 * D4EST_HIP_SCHWARZ_FUSED_RESIDUAL=1 the smoother and pc loops form rhs - A u in this kernel, the same rounded operation -- (2) hook 0,
 * (3) one kernel unpacks the ghost-layer part, (4) the subdomain solves, the correction STORED to the extended vector, (5) one kernel
 * packs its ghost-layer part, hook 1, (6) one kernel adds, per own node, the own correction and then the received blocks in ascending
 * peer rank (a fixed order, no atomics) -- or stores that sum, for the preconditioner's zero start vector.  Nothing is allocated per
 * iterate and the exchange ends read nothing on the host. */
typedef void (*d4est_hip_element_exchange_fn)(void* ctx, int direction, const double* send_dev, double* recv_dev);
void d4est_hip_schwarz_set_element_exchange(d4est_hip_schwarz_t* sz, int n_own_elements, int n_peers, const int* peer_rank,
                                            const int* send_first, const int* send_elem, const int* recv_first, const int* recv_elem,
                                            d4est_hip_element_exchange_fn fn, void* ctx);
/* nodes of the own elements; the mesh's node count when no exchange is set */
long long d4est_hip_schwarz_own_nodes(const d4est_hip_schwarz_t* sz);
long long d4est_hip_schwarz_exchange_first(const d4est_hip_schwarz_t* sz, int direction, int send_or_recv, int peer);
/* the RCCL transport of the two exchanges, in C (no callback into the host language): per direction one grouped ncclSend / ncclRecv round
 * on the communicator's stream, with the communicator's event in from and event out to the subdomain plan's stream (as
 * d4est_hip_comm_sendrecv).  Same lists as above; installs the hook on sz.  Destroy the returned object before sz and comm. */
typedef struct d4est_hip_schwarz_rccl_exchange d4est_hip_schwarz_rccl_exchange_t;
d4est_hip_schwarz_rccl_exchange_t* d4est_hip_schwarz_set_rccl_exchange(d4est_hip_schwarz_t* sz, d4est_hip_comm_t* comm, int n_own_elements,
                                                                       int n_peers, const int* peer_rank, const int* send_first,
                                                                       const int* send_elem, const int* recv_first, const int* recv_elem);
void d4est_hip_schwarz_rccl_exchange_destroy(d4est_hip_schwarz_rccl_exchange_t* x);
long long d4est_hip_schwarz_rccl_exchange_count(const d4est_hip_schwarz_rccl_exchange_t* x);   /* rounds posted so far (two per iterate) */

/* ---- the Chebyshev and Schwarz Krylov preconditioners (csrc/d4est_hip_pc.hip) --------------------------------------------------------
 * d4est_krylov_pc_cheby_apply (src/Solver/d4est_krylov_pc_cheby.c:92-171) and d4est_krylov_pc_schwarz_apply
 * (src/Solver/d4est_krylov_pc_schwarz.c:59-116) as d4est_hip_pc_fn: pass _apply as pc and the object as pc_ctx to d4est_hip_fcg_solve or
 * d4est_hip_newton_solve; a d4est host binds d4est_krylov_pc_t.pc_apply to them.  Both run on the plan's stream; their scratch vectors
 * are allocated at create, nothing per apply.  The plan (and the Schwarz handle) stay the caller's and must outlive the object.
 *
 * Chebyshev, the [d4est_krylov_pc_cheby] keys: z = 0; when !cheby_reuse_eig or no bound is held (eig == -1), cg_eigs runs
 * cheby_eigs_cg_imax iterations from z, WHICH IT ADVANCES (with cheby_use_zero_guess_for_eigs from a zero scratch vector, z stays zero)
 * and eig = bound * cheby_eigs_max_multiplier; then cheby_imax iterations on [eig / cheby_eigs_lmax_lmin_ratio, eig] without a final
 * residual.  _eig returns the bound held (-1: none) and, optionally, how many cg_eigs runs the object has made; _reset_eig drops the
 * bound (after the operator changed: a new linearisation). */
typedef struct d4est_hip_pc_cheby d4est_hip_pc_cheby_t;
d4est_hip_pc_cheby_t* d4est_hip_pc_cheby_create(d4est_hip_plan_t* plan, int cheby_imax, int cheby_eigs_cg_imax, double cheby_eigs_lmax_lmin_ratio,
                                                double cheby_eigs_max_multiplier, int cheby_reuse_eig, int cheby_use_new_cg_eigs,
                                                int cheby_use_zero_guess_for_eigs);
void d4est_hip_pc_cheby_destroy(d4est_hip_pc_cheby_t* pc);
void d4est_hip_pc_cheby_apply(void* pc, const double* r_dev, double* z_dev);
double d4est_hip_pc_cheby_eig(const d4est_hip_pc_cheby_t* pc, int* cg_eigs_runs);
void d4est_hip_pc_cheby_reset_eig(d4est_hip_pc_cheby_t* pc);
/* Schwarz, [schwarz_pc] schwarz_pc_iterations and the three [d4est_solver_schwarz] CG options: z = 0, then schwarz_pc_iterations times
 * { residual = r - A z; schwarz_iterate(z, residual) }.  In the first pass z is zero, so on a plan with homogeneous boundary data the
 * residual is r itself and the correction is stored into z (no fill, no apply, no read of z; the same numbers).  mesh_plan is the
 * plan of the mesh itself, as for d4est_hip_schwarz_smooth: the subdomain plan's stream; on several ranks the rank's own plan and a
 * handle with an element exchange (z and r then are vectors of the own nodes).  create aborts on a mismatch. */
typedef struct d4est_hip_pc_schwarz d4est_hip_pc_schwarz_t;
d4est_hip_pc_schwarz_t* d4est_hip_pc_schwarz_create(d4est_hip_schwarz_t* schwarz, d4est_hip_plan_t* mesh_plan, int schwarz_pc_iterations,
                                                    int subdomain_iter, double subdomain_atol, double subdomain_rtol);
void d4est_hip_pc_schwarz_destroy(d4est_hip_pc_schwarz_t* pc);
void d4est_hip_pc_schwarz_apply(void* pc, const double* r_dev, double* z_dev);

/* ---- the hp-AMR step (csrc/d4est_hip_amr.hip) ----------------------------------------------------------------------------------------
 * What d4est_amr_step (src/hpAMR/d4est_amr.c:852-1035) does between two solves, minus p4est's own work: the estimator statistics, the
 * smooth_pred marking with its predictor, the p-balance update, and the interpolation of a field onto the refined and balanced grid.
 * p4est_refine_ext, p4est_balance_ext and the p-balance face walk (d4est_amr.c:923-958) stay on the host; they exchange the refinement
 * log, the balance log and the p_balance array -- one int per element -- with this object.  Everything runs on the object's stream
 * (default: the null stream); nothing allocates after create / set_balance; no floating-point atomics and fixed reduction orders, so
 * results are bit-identical from call to call.  One rank: reductions over ranks stay with the caller, as for the norms -- except through
 * the entries under "the hp-AMR step on several ranks" below, which take two communication hooks; of those, d4est_hip_par_amr_repartition may
 * allocate (it rebuilds the level), as create and set_balance do.
 *
 * create: the per-element degrees (1 .. 20, the limit of d4est_hip_transfer_create's kernels: two (deg + 1)^3 fields in the 160 KB LDS;
 * aborts above it), amr->max_degree, and the predictor filled with initial_pred as d4est_amr_smooth_pred_pre_refine_callback does
 * (src/hpAMR/d4est_amr_smooth_pred.c:23-71; the checkpoint branch is not covered).  Environment D4EST_HIP_AMR_TWO_STAGE=1, read here:
 * d4est_hip_amr_interpolate_field runs as two d4est_hip_transfer_prolong calls through an internal auxiliary vector (A/B measurement). */
d4est_hip_amr_t* d4est_hip_amr_create(int n_elements, const int* deg, int max_degree, double initial_pred);
void d4est_hip_amr_destroy(d4est_hip_amr_t* amr);
void d4est_hip_amr_set_stream(d4est_hip_amr_t* amr, void* hip_stream);
int d4est_hip_amr_n_elements(const d4est_hip_amr_t* amr);
long long d4est_hip_amr_local_nodes(const d4est_hip_amr_t* amr);
/* d4est_estimator_stats_compute_aux, the mpisize == 1 branch (src/Estimators/d4est_estimator_stats.c:219-251), results on the device:
 * stats_dev[0] estimator_total (a fixed-order sum of eta2), [1] estimator_mean = total / n, [2] estimator_max, [3] estimator_at_percentile
 * = entry (int)(((double)n)*(1.-((double)percentile/100.0))) of the ascending-sorted eta2 (:249; the index is evaluated on the host in that
 * arithmetic; the sort is a device radix sort, eta2_dev is left as it is).  percentile 1 .. 100; with percentile = 0 the reference reads
 * one past the end of the array: here stats_dev[3] = -1.  n = 0 writes 0, -1, -1, -1 (:234-238).  This entry keeps the ONE-RANK index of
 * :249 whatever d4est_hip_par_amr_set_comm says; the index of the reference's mpisize > 1 branch differs: d4est_hip_par_amr_stats_global. */
void d4est_hip_amr_stats(d4est_hip_amr_t* amr, const double* eta2_dev, int percentile, double* stats_dev);
/* d4est_amr_smooth_pred_mark_elements (src/hpAMR/d4est_amr_smooth_pred.c:215-268) for every element, with the marker
 * eta2 >= factor * (*threshold_dev): sigma * mean as in Problems/Stamm/stamm_multigrid_pc.c:35-50 (stats_dev + 1, sigma) and the
 * percentile markers (stats_dev + 3, 1.0).  Writes the refinement log and the new predictor (:253-267); the products are rounded
 * multiplications taken left to right, never fused: the predictor is bit-identical to a plain C evaluation. */
void d4est_hip_amr_mark_smooth_pred(d4est_hip_amr_t* amr, const double* eta2_dev, const double* threshold_dev, double factor,
                                    double gamma_h, double gamma_p, double gamma_n);
/* d4est_amr.c:973-981 and d4est_amr_smooth_pred_compute_post_p_balance_predictor (d4est_amr_smooth_pred.c:132-168): where
 * p_balance_host[e] >= p_balance_if_diff and deg < max_degree - 1 a non-negative log entry gains 1, a negative one loses 1, and the
 * predictor is multiplied by gamma_p (of the last mark call; 1 before any).  The face walk that fills p_balance is the host's. */
void d4est_hip_amr_p_balance(d4est_hip_amr_t* amr, const int* p_balance_host, int p_balance_if_diff);
/* The refinement log for p4est_refine_ext, already clipped at max_degree as d4est_amr_refine_callback does (d4est_amr.c:182-184);
 * synchronises the stream. */
void d4est_hip_amr_get_refinement_log(d4est_hip_amr_t* amr, int* log_host);
/* A log made elsewhere (the uniform and random schemes, another marker).  An entry whose magnitude is below the element's degree aborts
 * with the reference's message: coarsening is not supported in d4est_amr_interpolate_field_on_element either (d4est_amr.c:386-392). */
void d4est_hip_amr_set_refinement_log(d4est_hip_amr_t* amr, const int* log_host);
void d4est_hip_amr_get_predictor(d4est_hip_amr_t* amr, double* pred_host);
/* The balance log of d4est_amr_balance_elements (d4est_amr.c:219-283) over the auxiliary (refined, unbalanced) grid: 8 auxiliary elements
 * per negative entry of the refinement log, 1 otherwise; |balance_log[i]| is auxiliary element i's degree, a negative entry splits it into
 * 8 children of that degree.  n_aux or a degree that does not match aborts.  Builds the new grid's degree list and the transfer tables;
 * afterwards the three queries give what the host needs for the next plan (degrees in traversal order). */
void d4est_hip_amr_set_balance(d4est_hip_amr_t* amr, int n_aux, const int* balance_log_host);
int d4est_hip_amr_new_n_elements(const d4est_hip_amr_t* amr);
long long d4est_hip_amr_new_local_nodes(const d4est_hip_amr_t* amr);
void d4est_hip_amr_get_new_degrees(const d4est_hip_amr_t* amr, int* deg_host);
/* d4est_amr_interpolate_field (d4est_amr.c:397-482) in one kernel and without the auxiliary vector: every new element's 1-D operator per
 * direction is the product (formed in fp64 by set_balance) of stage 1 -- identity, p_prolong(deg -> deg') or hp_prolong(deg -> deg')[bit] --
 * and stage 2 -- identity or hp_prolong(deg' -> deg')[bit]; kept -> kept, kept / p-refined -> split, split -> kept and split -> split
 * (64 new elements from one) are all served.  field_old_dev has local_nodes entries, field_new_dev new_local_nodes. */
void d4est_hip_amr_interpolate_field(d4est_hip_amr_t* amr, const double* field_old_dev, double* field_new_dev);
/* Which kernels serve the transfer (read-only, after set_balance): one text line "NH dmax nout n" per work list of auxiliary elements.  NH:
 * source nodes per direction of the compile-time kernel (2 .. 8), 0 for the runtime-size kernel; dmax: the list's largest new-minus-old
 * size (instances exist for 0, 1 and 3: a list with 2 runs the 3); nout: the most new elements an auxiliary element of the list becomes
 * (1 or 8); n: entries.  In two-stage mode one line "-1 0 0 n_aux".  Same buffer convention as d4est_hip_transfer_describe. */
int d4est_hip_amr_describe(const d4est_hip_amr_t* amr, char* buf, int len);
/* d4est_amr_smooth_pred_compute_post_h_balance_predictor (d4est_amr_smooth_pred.c:73-129): children of a refined element inherit the
 * predictor, children of a balance split get 0.125 * gamma_h * 0.5^(2 |balance_log|) * aux (gamma_h of the last mark call); then the new
 * degrees become current and the object is ready for the next level (the balance state is dropped; synchronises the stream). */
void d4est_hip_amr_advance(d4est_hip_amr_t* amr);

/* ---- the hp-AMR step on several ranks (csrc/d4est_hip_amr.hip) ------------------------------------------------------------------------
 * The two places of d4est_amr_step that talk to other ranks: the estimator statistics over all ranks and the load balance after the
 * refinement.  The object reaches the other ranks through two hooks of the caller.  allreduce: the contract of d4est_hip_plan_set_comm --
 * an in-place SUM over ranks of n device doubles -- here ordered on the AMR object's stream.  sendrecv: ONE grouped point-to-point round on
 * contiguous device ranges, the shape of d4est_hip_comm_sendrecv: to peer_rank[p] go the doubles [send_first[p], send_first[p + 1]) of
 * send_dev, from it arrive [recv_first[p], recv_first[p + 1]) of recv_dev (peers ascending; the two first arrays are host arrays of
 * n_peers + 1 entries, valid during the call); ordered on the object's stream too.  Every rank of a repartition whose partitions differ
 * makes the round, also a rank without a peer (n_peers = 0), so a hook may be a collective of its transport.  Without set_comm the object
 * is rank 0 of world 1: the entries below work and call no hook.  These entries carry the prefix d4est_hip_par_amr_ ("parallel"): the
 * d4est_hip_amr_ names above are the one-rank interface, a closed list. */
typedef void (*d4est_hip_amr_sendrecv_fn)(void* ctx, int n_peers, const int* peer_rank, const double* send_dev, const long long* send_first,
                                          double* recv_dev, const long long* recv_first);
void d4est_hip_par_amr_set_comm(d4est_hip_amr_t* amr, int rank, int world, d4est_hip_allreduce_fn allreduce, d4est_hip_amr_sendrecv_fn sendrecv,
                            void* ctx);
/* d4est_estimator_stats_compute_aux, the mpisize > 1 branch (src/Estimators/d4est_estimator_stats.c:252-274), results on the device.  With
 * G the element count of all ranks: stats_dev[0] the SUM over ranks of each rank's fixed-order local sum (:265), [1] total / G (:266), [2] the
 * maximum over all ranks (:269), [3] what d4est_estimator_stats_get_global_percentile_parallel returns (:350-425): entry G - k of the
 * ascending order of ALL ranks' eta2 with k = (int)((double)(G * percentile) / 100.0) (:379, :391) -- not the index of the one-rank branch
 * (:249), which d4est_hip_amr_stats keeps.  k = 0 (the reference aborts, :396) writes -1 to [3]; G = 0 writes 0, -1, -1, -1; a rank without
 * elements is legal.  Instead of the reference's distributed sort and rank walk (:254, :383-418) a radix select over ranks: a double maps to
 * an order-preserving 64-bit key, eight passes of eight bits from the top; per pass a histogram of the local keys under the prefix chosen
 * so far (integer atomics), ONE allreduce call of the bins as doubles (exact below 2^53), and a one-wavefront kernel that picks the digit.
 * The percentile and the maximum share the passes; the first round also carries the local n and sum: eight hook calls whatever n is.  No
 * host read anywhere, the selection state stays on the device, eta2_dev is left as it is; the same bits on every call, and [2], [3] are
 * the bits a sort of the concatenated array gives, on any number of ranks.  d4est_hip_amr_mark_smooth_pred takes its threshold from
 * stats_dev + 1 or stats_dev + 3 as on one rank. */
void d4est_hip_par_amr_stats_global(d4est_hip_amr_t* amr, const double* eta2_dev, int percentile, double* stats_dev);
/* The transfer of d4est_amr_load_balance (src/hpAMR/d4est_amr.c:773-864) once p4est_partition_ext has run on the host: old_first_host and
 * new_first_host are p4est->global_first_quadrant before and after it (world + 1 entries).  Rank r sends rank p the intersection of its old
 * range with p's new range -- both partitions are Morton-contiguous, so every message is one contiguous slice and what arrives, in peer
 * order, is in global order; the part that stays is a device-to-device copy.  Called on the current level, after d4est_hip_amr_advance,
 * where the reference's drivers balance the load.  Moves every element's degree and predictor to the new owner (one pack kernel, one
 * sendrecv round, one unpack kernel; degrees travel as doubles), synchronises, reads the received degrees and rebuilds the level: n_elements,
 * local_nodes, the predictor and every later call see the new local list.  Returns the new local node count.  Allocates.  Equal arrays
 * call no hook.  A rank may end up without elements.  Aborts on arrays that are not monotone, that cover different totals, or whose old
 * range of this rank is not n_elements. */
long long d4est_hip_par_amr_repartition(d4est_hip_amr_t* amr, const long long* old_first_host, const long long* new_first_host);
/* p4est_transfer_custom's part (d4est_amr.c:803-863): one nodal field from the old partition (the node count before the repartition) to
 * the new one (the count it returned), node offsets from the old and the new degree lists; one call, one sendrecv round per field.  Valid
 * from d4est_hip_par_amr_repartition until the next d4est_hip_amr_mark_smooth_pred or d4est_hip_amr_advance. */
void d4est_hip_par_amr_repartition_field(d4est_hip_amr_t* amr, const double* field_old_dev, double* field_new_dev);

/* ---- point probes: field value and gradient at tree coordinates (csrc/d4est_hip_probe.hip) -----------------------------------------
 * d4est_mesh_interpolate_at_tree_coord (src/Mesh/d4est_mesh.c:3294-3362) with d4est_operators_interpolate
 * (src/dGMath/d4est_operators.c:2289-2340) for a batch of points, the field resident on the device: what the TwoPunctures drivers read
 * at the punctures after every AMR level (src/Problems/TwoPunctures/two_punctures_cactus_13tree_with_opt_puncture_finder.c:951-978),
 * and, in bulk, line-outs and resampling.  A probe object holds the located points of ONE plan; it is the caller's, keeps a pointer to
 * the plan and MUST NOT OUTLIVE IT (destroy the probe first).  All kernels run on the plan's stream; after create nothing allocates and
 * eval / eval_gradient do not synchronise with the host.  No atomics and fixed reduction orders: the same bits on every call.
 *
 * create (d4est_mesh.c:3308-3328): tree[n_points] and abc[3 n_points] (point p at abc[3 p + d], tree coordinates in [0, 1]^3), host arrays
 * or, with on_device != 0, device arrays -- then the three element arrays are device arrays too.  elem_tree / elem_q / elem_dq / root_len:
 * where every LOCAL element of the plan sits in the forest, the layout of d4est_hip_plan_set_geometry_analytic (on a brick elem_tree is
 * all zero).  One wavefront per point scans the elements for  q[d] / root_len <= abc[d] <= (q[d] + dq) / root_len,  d = 0, 1, 2, in the
 * point's tree -- inclusive on both ends, the bounds rounded as at :3322-3326 -- and takes the LOWEST matching local element id: the
 * first match of the reference's loop in quadrant order for a point on a face, edge or corner between elements.  err = 0 found, 1 not
 * found (data.err, :3360): the tree is out of range, abc is outside [0, 1]^3, or the quadrant is a ghost or another rank's; multi-rank
 * callers reduce the err == 0 values themselves.  rst[d] = 2 (abc[d] - amin) / (amax - amin) - 1 in that order of operations (:3339).
 * The points' deg and nodal_stride are taken from the plan.  n_points = 0 is valid: every call on such a probe is a no-op.  synchronises. */
typedef struct d4est_hip_probe d4est_hip_probe_t;
d4est_hip_probe_t* d4est_hip_probe_create(d4est_hip_plan_t* plan, int n_points, const int* tree, const double* abc, const int* elem_tree,
                                          const int* elem_q, const int* elem_dq, double root_len, int on_device);
void d4est_hip_probe_destroy(d4est_hip_probe_t* probe);
int d4est_hip_probe_n_points(const d4est_hip_probe_t* probe);
/* host outputs, any may be NULL: err_host[n_points]; elem_host[n_points] (data.id as a local element id, -1 where err = 1);
 * rst_host[3 n_points] (point p at 3 p + d; NaN where err = 1).  synchronises the stream. */
void d4est_hip_probe_info(const d4est_hip_probe_t* probe, int* err_host, int* elem_host, double* rst_host);
/* likewise the located elements' nodal_stride (data.nodal_stride) and deg, n_points each (0 where err = 1); either may be NULL */
void d4est_hip_probe_element_info(const d4est_hip_probe_t* probe, int* nodal_stride_host, int* deg_host);
/* d4est_operators_interpolate (d4est_operators.c:2289-2340) of n_fields fields, field f at u_dev + f * field_stride (doubles; each a
 * nodal vector of the plan):  out_dev[f * n_points + p] = sum_{k,j,i} l_k(t) l_j(s) l_i(r) u_f[nodal_stride + (k N + j) N + i],  i
 * fastest (d4est_kron_vec1_o_vec2_o_vec3_dot_x_sum as called at :2320-2330), l_i the product form of d4est_lgl_lagrange_1d
 * (src/dGMath/d4est_lgl.c:59-68) on the engine's Lobatto nodes (D4EST_HIP_TABLE_LOBATTO_NODES), factors taken in its order.  Degrees 1 ..
 * 19, mixed degrees in one launch: one wavefront per point forms the three basis vectors once for all fields, its lanes own (j, k)
 * columns and loop over i, a fixed-order wave reduction follows.  A point with err = 1 gets a quiet NaN (the reference leaves f_at_xyz
 * unset). */
void d4est_hip_probe_eval(d4est_hip_probe_t* probe, int n_fields, const double* u_dev, long long field_stride, double* out_dev);
/* The analytic map the plan's geometry was set with, for eval_gradient(physical = 1) and probe_xyz: geom_type D4EST_HIP_GEOM_BRICK with
 * params = extents {X0, X1, Y0, Y1, Z0, Z1} of d4est_hip_plan_set_geometry_brick (x_d = X0_d + (X1_d - X0_d) abc_d, one tree), or one
 * of the four sphere types with the params of d4est_hip_plan_set_geometry_analytic.  Aborts like that call on a bad type, radius or
 * flag, and when a found point's tree is not one of the map's. */
#define D4EST_HIP_GEOM_BRICK 0
void d4est_hip_probe_set_map(d4est_hip_probe_t* probe, int geom_type, const double* params);
/* grad_dev[d * n_points + p], d = 0, 1, 2.  physical = 0: the reference-space gradient (du/dr, du/ds, du/dt) from the derivative of the
 * same product-form basis at the point, d/dr through l'_i(r) l_j(s) l_k(t) and likewise in s and t.  physical = 1: (du/dx, du/dy, du/dz)
 * = sum_i (du/dr_i) dr_i/dx_d with dr/dx the inverse of the 3 x 3 Jacobian of the map of probe_set_map AT THE POINT, dx/d(abc) scaled by
 * the element's dq / root_len / 2 -- the plan stores no inverse Jacobian at the nodes that could be interpolated, only the combined metric
 * (csrc/d4est_hip_norms.hip:21-22).  physical = 1 without a map aborts.  err = 1: quiet NaN. */
void d4est_hip_probe_eval_gradient(d4est_hip_probe_t* probe, const double* u_dev, double* grad_dev, int physical);
/* data.xyz (d4est_mesh.c:3332): xyz_host[3 p + d] = the map of probe_set_map at (tree, abc) of point p (NaN where err = 1).  Needs a map;
 * synchronises the stream. */
void d4est_hip_probe_xyz(d4est_hip_probe_t* probe, double* xyz_host);

/* ---- problem data on the device: puncture and star source fields, Robin data by id (csrc/d4est_hip_problem.hip) ------------------------
 * The coefficient functions of the reference's shipped nonlinear drivers (TwoPunctures, multi-puncture, ConstantDensityStar) evaluated
 * where the coordinates already are, so that no array of quadrature size crosses the bus when the mesh changes.  All arithmetic of this
 * unit is compiled without floating-point contraction (no fused multiply-add): a field's value does not depend on the kernel that
 * evaluates it, and the term entries below give the bits of d4est_hip_field_eval on the coordinates of d4est_hip_plan_compute_xyz_*.
 *
 * Field ids (x, y, z -> one double):
 *   PUNCTURE_K2  confAij_sqr (src/Problems/TwoPunctures/two_punctures_fcns.h:180-248).  Not a transcription of the Levi-Civita loops:
 *                per puncture n = (x - C) / r, P.n and S x n are formed once, the six independent components of the symmetric
 *                A_ij = sum_n (1 / r^2) (n_i P_j + n_j P_i - (delta_ij - n_i n_j) P.n + (2 / r) ((S x n)_i n_j + (S x n)_j n_i))
 *                are accumulated over the punctures, and K2 = sum_ij (3/2 A_ij)^2 with the diagonal once and the off-diagonal twice.
 *   PUNCTURE_A   -K2 / 8, the `a` of two_punctures_neg_1o8_K2_psi_neg7 (:252-284), and exactly 0.0 where r > puncture_eps fails
 *   PUNCTURE_B   1 + sum_n m_n / (2 r_n) (:263-274), the `b` of the same callback (psi_0 = b + u)
 *   CDS_A        -2 pi rho(x), the `a` of neg_2pi_rho_up1_neg5 (src/Problems/ConstantDensityStar/constant_density_star_fcns.h:276-301,
 *                :347-357): -2 pi rho0 for r^2 <= R^2, else 0
 *   CDS_PSI      psi_fcn (:246-273): 1 + beta / r for r^2 > R^2, else C0 u_alpha (:88-111); the analytic solution and the Dirichlet
 *                boundary function (:303-330)
 *   INV_R        1 / sqrt(x^2 + y^2 + z^2): two_punctures_robin_coeff_sphere_fcn (two_punctures_fcns.h:640-655),
 *                constant_density_star_robin_coeff_sphere_fcn and _robin_bc_rhs_for_res_fcn (constant_density_star_fcns.h:9-24, :42-57)
 *   OKENDON_U    okendon_analytic_solution, DIM == 3 (src/Problems/Okendon/okendon_fcns.h:70-96): M r2^(1/(1-p)),
 *                M = 1 / pow((2/(1-p)) (1 + 2/(1-p)), 1/(1-p)); also its boundary function (:99-111)
 *   BY_PSI       boyen_york_model_analytic_solution (src/Problems/BoyenYorkModel/boyen_york_model_fcns.h:67-95):
 *                pow(1 + 2E/r + 6a^2/r^2 + 2a^2E/r^3 + a^4/r^4, .25), E = sqrt(P^2 + 4a^2); also its boundary function (:97-108)
 *   BY_A         boyen_york_model_helmholtz_fcn (:110-128): .75 (P^2/r^4) (1 - a^2/r^2)^2, the `a` of the residual callback (:131-149)
 *   LORENTZIAN_U      poisson_lorentzian_analytic_solution (src/Problems/Poisson/poisson_lorentzian_fcns.h:55-67): 1 / sqrt(1 + r^2)
 *   LORENTZIAN_RHS    poisson_lorentzian_rhs_fcn (:71-82): 3 / pow(1 + r^2, 2.5)
 *   LORENTZIAN_ROBIN  poisson_lorentzian_robin_coeff_fcn (:22-36): sqrt(r2) / (1 + r2)
 *   STAMM_U      stamm_analytic_solution, DIM == 3 (src/Problems/Stamm/stamm_fcns.h:78-114): x(1-x) y(1-y) z(1-z) |x - c2|^3
 *   STAMM_RHS    stamm_rhs_fcn, DIM == 3 (:149-208), its thirteen terms in the reference's order; exactly 0.0 at x = c2
 * Two behaviours of the reference are kept:
 *   (a) compute_confAij moves a point that lies exactly on a puncture to r = puncture_eps (:202-203): n = 0 there, the puncture
 *       contributes nothing and K2 is finite;
 *   (b) the test r > puncture_eps of the two power callbacks reads r after the loop, i.e. the distance to the LAST puncture only
 *       (:264-277).  On and within puncture_eps of the last puncture a = 0.0; exactly on an earlier puncture a is finite and b = +inf, so
 *       that the power kernels give a (1 / inf^7) = 0, not NaN.
 * params (host doubles): the puncture fields take {num_punctures, puncture_eps, then per puncture C[3], P[3], S[3], M}, n_params =
 * 2 + 10 num_punctures, 1 <= num_punctures <= 9 (the reference's num_punctures < MAX_PUNCTURES = 10); the star fields take {cx, cy, cz,
 * R, rho0, C0, alpha, beta}, n_params = 8 (alpha from the reference's bisection, constant_density_star_fcns.h:151-243, which stays on the
 * host); INV_R and the three Lorentzian fields take none (params may be NULL); OKENDON_U takes {p}, 0 < p < 1 (the range
 * okendon_params_init asserts); BY_PSI and BY_A take {a, P}; STAMM_U and STAMM_RHS take {c2x, c2y, c2z}.  A bad id or count aborts.
 *
 * d4est_hip_field_eval: out_dev[i] = field(xyz_dev[i], xyz_dev[n + i], xyz_dev[2 n + i]), the x | y | z layout of
 * d4est_hip_plan_compute_xyz_analytic; one thread per point on hip_stream (a hipStream_t, NULL = the default stream), no host
 * synchronisation, no allocation. */
#define D4EST_HIP_FIELD_PUNCTURE_K2 0
#define D4EST_HIP_FIELD_PUNCTURE_A 1
#define D4EST_HIP_FIELD_PUNCTURE_B 2
#define D4EST_HIP_FIELD_CDS_A 3
#define D4EST_HIP_FIELD_CDS_PSI 4
#define D4EST_HIP_FIELD_INV_R 5
#define D4EST_HIP_FIELD_OKENDON_U 6
#define D4EST_HIP_FIELD_BY_PSI 7
#define D4EST_HIP_FIELD_BY_A 8
#define D4EST_HIP_FIELD_LORENTZIAN_U 9
#define D4EST_HIP_FIELD_LORENTZIAN_RHS 10
#define D4EST_HIP_FIELD_LORENTZIAN_ROBIN 11
#define D4EST_HIP_FIELD_STAMM_U 12
#define D4EST_HIP_FIELD_STAMM_RHS 13
#define D4EST_HIP_MAX_PUNCTURES 10
void d4est_hip_field_eval(void* hip_stream, int field_id, const double* params, int n_params, const double* xyz_dev, long long n,
                          double* out_dev);
/* x | y | z of the single-tree brick at the plan's Lobatto and / or quadrature nodes (either output may be NULL), the layout and node
 * order of d4est_hip_plan_compute_xyz_analytic: x_d = X0_d + (X1_d - X0_d) (q_d + dq (r_d + 1) / 2) / root_len
 * (d4est_geometry_brick_X, src/Geometry/d4est_geometry_brick.c:119-149, on one tree).  elem_q[3 e + d] / elem_dq[e]: the elements'
 * corner and side length in p4est units, extents = {X0, X1, Y0, Y1, Z0, Z1} as in d4est_hip_plan_set_geometry_brick. */
void d4est_hip_plan_compute_xyz_brick(d4est_hip_plan_t* plan, const int* elem_q, const int* elem_dq, double root_len,
                                      const double* extents, double* xyz_lobatto_dev, double* xyz_quad_dev);
/* The puncture term a (b + u)^-7, a = PUNCTURE_A, b = PUNCTURE_B, and the star term a u^5, a = CDS_A, b = NULL, set on a plan by ONE
 * kernel: a workgroup per element, a thread per quadrature node takes the node's tree coordinate from the element's q / dq and the
 * plan's quadrature abscissae (Gauss or Lobatto by the plan's quad_type), evaluates the map, then a and b, and writes them into the
 * plan-owned arrays d4est_hip_plan_set_nonlinear_power would have filled by copy.  No xyz_quad temporary, no caller-side a / b, no
 * copy; mixed-degree plans in one launch.  Afterwards the plan is in the state set_nonlinear_power(a, b, k) leaves (k = -7 / k = 5):
 * d4est_hip_apply_nonlinear_term, _plan_linearise, _build_residual and _newton_solve work unchanged.  Replaces the caller-side loop over
 * xyz_quad with the callbacks cited above.  Coordinate sources:
 *   _brick     elem_q, elem_dq, root_len, extents as in d4est_hip_plan_compute_xyz_brick
 *   _analytic  geom_type, geom_params, elem_tree, elem_q, elem_dq, root_len as in d4est_hip_plan_set_geometry_analytic
 *   _xyz       the caller's xyz_quad_dev (x | y | z, 3 local_nodes_quad doubles), for numerical geometry
 * Stream-ordered after a staging copy of the element descriptions; the term's values equal d4est_hip_field_eval on the coordinates of
 * d4est_hip_plan_compute_xyz_brick / _analytic bit for bit. */
void d4est_hip_plan_set_puncture_term_brick(d4est_hip_plan_t* plan, const double* params, int n_params, const int* elem_q,
                                            const int* elem_dq, double root_len, const double* extents);
void d4est_hip_plan_set_puncture_term_analytic(d4est_hip_plan_t* plan, const double* params, int n_params, int geom_type,
                                               const double* geom_params, const int* elem_tree, const int* elem_q, const int* elem_dq,
                                               double root_len);
void d4est_hip_plan_set_puncture_term_xyz(d4est_hip_plan_t* plan, const double* params, int n_params, const double* xyz_quad_dev);
void d4est_hip_plan_set_cds_term_brick(d4est_hip_plan_t* plan, const double* params, int n_params, const int* elem_q, const int* elem_dq,
                                       double root_len, const double* extents);
void d4est_hip_plan_set_cds_term_analytic(d4est_hip_plan_t* plan, const double* params, int n_params, int geom_type,
                                          const double* geom_params, const int* elem_tree, const int* elem_q, const int* elem_dq,
                                          double root_len);
void d4est_hip_plan_set_cds_term_xyz(d4est_hip_plan_t* plan, const double* params, int n_params, const double* xyz_quad_dev);
/* The same for the two remaining nonlinear families, by the same kernel:
 *   Okendon     f = |u|^p as okendon_build_residual adds it to A u (okendon_fcns.h:328-406): a = +1, b = NULL, the REAL form with s = p
 *               (params = {p}); afterwards the plan is as d4est_hip_plan_set_nonlinear_abs_power(a, NULL, p) leaves it
 *   Boyen-York  f = BY_A u^-7 as boyen_york_model_build_residual adds it (boyen_york_model_fcns.h:239-332): a = BY_A, b = NULL, the
 *               integer form with k = -7 (params = {a, P}).  The reference's 1 / pow(u*u, 3.5) is u^-7 for the positive u it assumes
 *               (:142), the decision TwoPunctures' pow(psi^2, 3.5) got. */
void d4est_hip_plan_set_okendon_term_brick(d4est_hip_plan_t* plan, const double* params, int n_params, const int* elem_q,
                                           const int* elem_dq, double root_len, const double* extents);
void d4est_hip_plan_set_okendon_term_analytic(d4est_hip_plan_t* plan, const double* params, int n_params, int geom_type,
                                              const double* geom_params, const int* elem_tree, const int* elem_q, const int* elem_dq,
                                              double root_len);
void d4est_hip_plan_set_okendon_term_xyz(d4est_hip_plan_t* plan, const double* params, int n_params, const double* xyz_quad_dev);
void d4est_hip_plan_set_boyen_york_term_brick(d4est_hip_plan_t* plan, const double* params, int n_params, const int* elem_q,
                                              const int* elem_dq, double root_len, const double* extents);
void d4est_hip_plan_set_boyen_york_term_analytic(d4est_hip_plan_t* plan, const double* params, int n_params, int geom_type,
                                                 const double* geom_params, const int* elem_tree, const int* elem_q, const int* elem_dq,
                                                 double root_len);
void d4est_hip_plan_set_boyen_york_term_xyz(d4est_hip_plan_t* plan, const double* params, int n_params, const double* xyz_quad_dev);
/* The load vector of a linear problem from a field id: out = beta out + V^T W J f(x_quad) per element, beta = 0 or 1 -- what the
 * Poisson and Stamm drivers build with d4est_mesh_init_field on the quadrature nodes followed by
 * d4est_quadrature_apply_galerkin_integral (src/Quadrature/d4est_quadrature.c:142-213).  ONE kernel per degree bucket (map, field,
 * integrate; no coordinate or quadrature-sized temporary) when every element's (deg, deg_quad) is a pair
 * d4est_hip_apply_galerkin_integral serves with a one-kernel path; else d4est_hip_plan_compute_xyz_*, d4est_hip_field_eval and
 * d4est_hip_apply_galerkin_integral through plan-owned temporaries (allocated on first use, no synchronisation).  The one-kernel path
 * integrates with the even-odd contractions: its bits equal the three-call composition's while D4EST_HIP_TUNE_STIFFNESS_EO has its
 * default (on); with the key off the two agree to rounding.  Any field id, sources as for the term entries; needs plan_set_geometry (J). */
void d4est_hip_plan_build_load_by_id_brick(d4est_hip_plan_t* plan, int field_id, const double* params, int n_params, const int* elem_q,
                                           const int* elem_dq, double root_len, const double* extents, int beta, double* out_dev);
void d4est_hip_plan_build_load_by_id_analytic(d4est_hip_plan_t* plan, int field_id, const double* params, int n_params, int geom_type,
                                              const double* geom_params, const int* elem_tree, const int* elem_q, const int* elem_dq,
                                              double root_len, int beta, double* out_dev);
void d4est_hip_plan_build_load_by_id_xyz(d4est_hip_plan_t* plan, int field_id, const double* params, int n_params,
                                         const double* xyz_quad_dev, int beta, double* out_dev);
/* the plan-owned a and b (device, local_nodes_quad doubles; *b_dev NULL: b = 0) and k of the power term that is set (k = 0 while the
 * real form is set: d4est_hip_plan_nonlinear_exponent); returns 0 and writes nothing when the term is off.  Any output may be NULL.  The arrays live until the term is switched off or the plan destroyed. */
int d4est_hip_plan_nonlinear_coefficients(const d4est_hip_plan_t* plan, const double** a_dev, const double** b_dev, int* k);
/* xyz_m_mortar_quad of the boundary faces (src/Mesh/d4est_mesh.c:514-640, consumed at src/dGMath/d4est_laplacian_flux.c:47-112,
 * :200-204): x | y | z at the mortar quadrature nodes of every boundary side, indexed like sj -- side_mortar_stride[s] + k, the
 * components total_mortar_nodes apart (3 total_mortar_nodes doubles), k = a + NQ b over the face's two axes in increasing order, the
 * order in which the boundary flux kernels read sj and the Robin arrays.  The map is evaluated AT the face's quadrature points
 * (d4est_mesh.c:604-625), not interpolated from Lobatto nodes.  Entries of sides that are not boundary sides are left untouched.
 * Needs plan_set_faces; no ghost data is read (boundary sides are local).  Sources as for the term entries.  Unlike them, these two
 * entries and d4est_hip_plan_set_robin_by_id_* below are set-up calls that SYNCHRONISE: each builds the list of boundary sides on the
 * host, uploads it, and waits for its kernel before freeing the list. */
void d4est_hip_plan_compute_boundary_xyz_brick(d4est_hip_plan_t* plan, const int* elem_q, const int* elem_dq, double root_len,
                                               const double* extents, double* xyz_mortar_dev);
void d4est_hip_plan_compute_boundary_xyz_analytic(d4est_hip_plan_t* plan, int geom_type, const double* geom_params, const int* elem_tree,
                                                  const int* elem_q, const int* elem_dq, double root_len, double* xyz_mortar_dev);
/* Robin data from callback ids: one kernel over the boundary sides' mortar nodes evaluates the map, the coefficient and the right-hand
 * side and writes sj coeff and sj rhs into the plan's Robin arrays -- the state d4est_hip_plan_set_robin_values leaves, without a
 * coordinate array in between.  coeff_id: ROBIN_COEFF_INV_R (the sphere callbacks cited at INV_R), ROBIN_COEFF_LORENTZIAN
 * (LORENTZIAN_ROBIN above, with ROBIN_RHS_ZERO: poisson_lorentzian_robin_bc_rhs_fcn, poisson_lorentzian_fcns.h:38-52) or ROBIN_COEFF_BRICK
 * (two_punctures_robin_coeff_brick_fcn, two_punctures_fcns.h:612-638: n_axis x_axis / r^2; on a brick the normal of face f is
 * +-e_axis, so the coefficient is sign(f) x_axis / r^2 and no normal array is read); rhs_id: ROBIN_RHS_ZERO (two_punctures_robin_bc_rhs_fcn
 * :659-673, constant_density_star_robin_bc_rhs_for_jac_fcn :26-40) or ROBIN_RHS_INV_R (constant_density_star_robin_bc_rhs_for_res_fcn
 * :42-57).  ROBIN_COEFF_BRICK exists on the _brick source only.  Needs the mortar factors (sj);
 * d4est_hip_plan_set_robin_values(plan, NULL, ...) still switches back to Dirichlet.
 * Dirichlet data needs no entry of its own: d4est_hip_field_eval(CDS_PSI) on the three d4est_hip_plan_boundary_gather'ed Lobatto
 * coordinate vectors (stored x | y | z) gives the array d4est_hip_plan_set_dirichlet_values(on_device = 1) takes.
 * Not built: the Cactus-data variants and the alpha bisection. */
#define D4EST_HIP_ROBIN_COEFF_INV_R 0
#define D4EST_HIP_ROBIN_COEFF_BRICK 1
#define D4EST_HIP_ROBIN_COEFF_LORENTZIAN 2
#define D4EST_HIP_ROBIN_RHS_ZERO 0
#define D4EST_HIP_ROBIN_RHS_INV_R 1
void d4est_hip_plan_set_robin_by_id_brick(d4est_hip_plan_t* plan, int coeff_id, int rhs_id, const int* elem_q, const int* elem_dq,
                                          double root_len, const double* extents);
void d4est_hip_plan_set_robin_by_id_analytic(d4est_hip_plan_t* plan, int coeff_id, int rhs_id, int geom_type, const double* geom_params,
                                             const int* elem_tree, const int* elem_q, const int* elem_dq, double root_len);

#ifdef __cplusplus
}
#endif
#endif /* D4EST_HIP_H */
