/*
 * d4est_hip_compat.h -- the reference's OWN entry points for the hot path, exported by libd4est_hip_compat.so.
 *
 * "Functions a C-ABI replacement must export (same signatures, extern "C")".  Every prototype below is the
 * reference's, name and argument list unchanged (file:line beside each), so a d4est build can drop the object files that define
 * them (or link this library in front of them) and keep every caller untouched.  The struct arguments the reference passes by
 * pointer are forward-declared opaque here -- the shims never look inside them, with two exceptions stated below -- so this header
 * needs no p4est / d4est header.  A translation unit that already includes the reference's headers must NOT include this one
 * (the prototypes are identical; the opaque typedefs would collide): define D4EST_HIP_COMPAT_NO_TYPES to get only the binding API.
 *
 * Layout facts relied on (and nothing else):
 *   * d4est_quadrature_t starts with `d4est_quadrature_type_t quad_type` (an int-sized enum, 0 = Gauss-Legendre,
 *     1 = Gauss-Lobatto; src/Quadrature/d4est_quadrature.h:8-14, :117-119).  The compactified types abort, as unsupported.
 *   * d4est_elliptic_data_t is the struct of src/EllipticSystem/d4est_elliptic_data.h:6-37, mirrored below.
 *
 * Host pointers in, host pointers out, like the reference.  Element-level shims run on cached one-element plans with persistent
 * pinned staging and device buffers: no hipMalloc per call (one set per (deg, deg_quad) pair on first use).  They are the
 * compatibility path, PCIe- and launch-latency bound (tens of microseconds per element); the fast path is a whole-mesh plan
 * (include/d4est_hip.h) bound to the p4est with d4est_hip_compat_bind_mesh, which the operator-level shims use.
 * DIM = 3 only (the reference's d8est build); other `dim` values abort.  Volume objects run on the device; QUAD_OBJECT_MORTAR objects of
 * the quadrature entry points (interpolate, mass, galerkin, the two callback forms) are served on the host.  Errors abort (D4EST_ABORT).
 */
#ifndef D4EST_HIP_COMPAT_H
#define D4EST_HIP_COMPAT_H

#include "d4est_hip.h"

#ifdef __cplusplus
extern "C" {
#define D4EST_RESTRICT
#else
#define D4EST_RESTRICT restrict
#endif

#ifndef D4EST_HIP_COMPAT_NO_TYPES
/* opaque stand-ins for the reference's types (pointers only) */
typedef struct p8est p4est_t;                                   /* pXest.h: p4est_t == p8est_t when DIM = 3 */
typedef struct d4est_operators_opaque d4est_operators_t;        /* dGMath/d4est_operators.h:9-51 */
typedef struct d4est_geometry_opaque d4est_geometry_t;          /* Geometry/d4est_geometry.h */
typedef struct d4est_quadrature_opaque d4est_quadrature_t;      /* Quadrature/d4est_quadrature.h:117-130 */
typedef struct d4est_mesh_data_opaque d4est_mesh_data_t;        /* Mesh/d4est_mesh.h:123-169 */
typedef struct d4est_ghost_opaque d4est_ghost_t;                /* Mesh/d4est_ghost.h */
typedef struct d4est_ghost_data_opaque d4est_ghost_data_t;      /* Mesh/d4est_ghost_data.h */
typedef struct d4est_solver_schwarz_opaque d4est_solver_schwarz_t;   /* Solver/d4est_solver_schwarz.h:14-38 (not read by the shims) */
/* The CALLER-SET head of the two flux-data structs, mirrored member for member (dGMath/d4est_laplacian_flux.h:113-128,
 * dGMath/d4est_laplacian_with_opt_flux.h:125-139); the "internally set" tails are never touched here.  The operator-level shims read
 * flux_type, the SIPG prefactor (first member of d4est_laplacian_flux_sipg_params_t, dGMath/d4est_laplacian_flux_sipg.h:18-19) and
 * bc_type, and abort when they differ from what the bound plan was set up with (d4est_hip_compat_bind_flux). */
typedef struct d4est_laplacian_flux_data {
  int flux_type;                                   /* d4est_laplacian_flux_type_t: FLUX_SIPG 0, FLUX_NIPG 1, FLUX_IIPG 2, FLUX_NOT_SET 3 (d4est_laplacian_aux.h:6) */
  void (*interface_fcn)(void);                     /* d4est_laplacian_flux_interface_fcn_t */
  void (*boundary_fcn)(void);                      /* d4est_laplacian_flux_boundary_fcn_t */
  void* flux_data;                                 /* FLUX_SIPG: d4est_laplacian_flux_sipg_params_t* */
  int (*get_deg_mortar_quad)(void*, void*);
  void* get_deg_mortar_quad_ctx;
  int bc_type;                                     /* d4est_laplacian_bc_t: BC_ROBIN 0, BC_DIRICHLET 1, BC_NOT_SET 2 (d4est_laplacian_aux.h:7) */
  void* bc_data;
} d4est_laplacian_flux_data_t;
typedef struct d4est_laplacian_with_opt_flux_data {
  int flux_type;
  void (*interface_fcn)(void);
  void (*boundary_fcn)(void);
  void* flux_data;
  int (*get_deg_mortar_quad)(void*, void*);
  void* get_deg_mortar_quad_ctx;
  int skip_p_side;
  int last_mortar_side_id_m;
  int bc_type;
  void* bc_data;
} d4est_laplacian_with_opt_flux_data_t;
#define FLUX_SIPG 0
#define BC_ROBIN 0
#define BC_DIRICHLET 1
/* src/Mesh/d4est_xyz_functions.h:14-25 (DIM = 3): f(x, y, z, user); src/Mesh/d4est_mesh.h:19 */
typedef double (*d4est_xyz_fcn_t)(double, double, double, void*);
typedef int d4est_mesh_init_field_option_t;
#define INIT_FIELD_NOT_SET 0
#define INIT_FIELD_ON_LOBATTO 1
#define INIT_FIELD_ON_QUAD 2
/* the additive Schwarz metadata, mirrored member for member (src/Solver/d4est_solver_schwarz_metadata.h:19-90; p4est_qcoord_t = int32_t):
 * what d4est_hip_compat_flatten_schwarz_metadata walks */
typedef struct {
  int mpirank, tree, tree_quadid, id, deg;
  int faces[3];
  int core_faces[3];
  int is_core;
  int nodal_size, nodal_stride, restricted_nodal_size, restricted_nodal_stride;
} d4est_solver_schwarz_element_metadata_t;
typedef struct {
  int mpirank, subdomain_id, core_id;
  d4est_solver_schwarz_element_metadata_t* element_metadata;
  int core_deg, core_tree, num_elements, restricted_nodal_size, restricted_nodal_stride, nodal_size, nodal_stride, element_stride;
} d4est_solver_schwarz_subdomain_metadata_t;
typedef struct {
  int num_nodes_overlap;
  int restricted_nodal_size, nodal_size, num_subdomains, num_elements;
  d4est_solver_schwarz_subdomain_metadata_t* subdomain_metadata;
  d4est_solver_schwarz_element_metadata_t* element_metadata;
  void* subdomain_ghostdata;   /* d4est_ghost_data_ext_t* */
  void* element_ghostdata;
  d4est_ghost_t* d4est_ghost;
  const char* input_section;
} d4est_solver_schwarz_metadata_t;
typedef int d4est_quadrature_object_type_t;                     /* enum {QUAD_OBJECT_MORTAR, QUAD_OBJECT_VOLUME}, d4est_quadrature.h:16-17 */
typedef int d4est_quadrature_integrand_type_t;                  /* enum, d4est_quadrature.h:21-29 */
typedef int d4est_field_type_t;                                 /* enum, Mesh/d4est_field.h */
typedef int d4est_quadrature_apply_or_compute_matrix_t;         /* enum {QUAD_APPLY_MATRIX, QUAD_COMPUTE_MATRIX}, d4est_quadrature.h:19 */
#define QUAD_OBJECT_MORTAR 0
#define QUAD_OBJECT_VOLUME 1
#define QUAD_INTEGRAND_UNKNOWN 5
#define QUAD_APPLY_MATRIX 0
#define QUAD_COMPUTE_MATRIX 1
/* src/Mesh/d4est_xyz_functions.h:27-37 (DIM = 3): f(x, y, z, u, user) */
typedef double (*d4est_xyzu_fcn_t)(double, double, double, double, void*);

/* src/EllipticSystem/d4est_elliptic_data.h:6-37 (all four vectors are aliases the callee never owns) */
typedef struct {
  int mpirank;
  int local_nodes;
  int num_of_fields;
  d4est_field_type_t* field_types;
  double* Au;
  double* u;
  double* u0;
  double* rhs;
  void* user;
} d4est_elliptic_data_t;

/* src/EllipticSystem/d4est_elliptic_eqns.h:12-36 */
typedef void (*d4est_apply_operator_fcn_t)(p4est_t*, d4est_ghost_t*, d4est_ghost_data_t*, d4est_elliptic_data_t*, d4est_operators_t*,
                                           d4est_geometry_t*, d4est_quadrature_t*, d4est_mesh_data_t*, void*);
typedef struct {
  d4est_apply_operator_fcn_t apply_lhs;
  d4est_apply_operator_fcn_t build_residual;
  void* user;
} d4est_elliptic_eqns_t;

/* src/dGMath/d4est_laplacian_flux_sipg.h:8-16 and src/Estimators/d4est_estimator_bi.h:8-23, member for member (passed BY VALUE to
 * d4est_estimator_bi_compute, so the layout must be the reference's) */
typedef double (*penalty_calc_t)(int, double, int, double, double);
typedef struct d4est_mesh_size_parameters_opaque d4est_mesh_size_parameters_t;
typedef struct {
  double* estimator;
  int output_vtk;
  double* estimator_vtk;            /* residual term, je1 term, je2 term, je2 boundary term */
  double* estimator_vtk_per_face;
  penalty_calc_t u_penalty_fcn;
  penalty_calc_t u_dirichlet_penalty_fcn;
  penalty_calc_t gradu_penalty_fcn;
  d4est_mesh_size_parameters_t* size_params;
  double penalty_prefactor;
  void* user;
} d4est_estimator_bi_penalty_data_t;

/* src/dGMath/d4est_ip_energy_norm.h:9-19 and src/IO/d4est_norms.h:25-62, member for member: what d4est_norms_save's norm functions
 * are handed as their void* context.  d4est_element_data_t stays opaque: a skip_element_fcn cannot be evaluated here. */
typedef struct d4est_element_data_opaque d4est_element_data_t;
typedef struct {
  penalty_calc_t u_penalty_fcn;
  double penalty_prefactor;
  d4est_mesh_size_parameters_t* size_params;
  void* user;
  double ip_energy_norm_sqr_volume_term;
  double ip_energy_norm_sqr_boundary_term;
  double ip_energy_norm_sqr_interface_term;
} d4est_ip_energy_norm_data_t;
typedef struct {
  p4est_t* p4est;
  d4est_operators_t* d4est_ops;
  d4est_geometry_t* d4est_geom;
  d4est_quadrature_t* d4est_quad;
  d4est_mesh_data_t* d4est_factors;
} d4est_norms_fcn_L2_ctx_t;
typedef struct {
  p4est_t* p4est;
  d4est_ghost_t* ghost;
  d4est_ghost_data_t* ghost_data;
  d4est_operators_t* d4est_ops;
  d4est_geometry_t* d4est_geom;
  d4est_quadrature_t* d4est_quad;
  d4est_mesh_data_t* d4est_factors;
  int which_field;
  d4est_ip_energy_norm_data_t* energy_norm_data;
  double energy_estimator_sq_local;
  double* energy_estimator;
} d4est_norms_fcn_energy_ctx_t;
typedef double (*d4est_norm_fcn_t)(p4est_t*, double*, int, void*, int (*)(d4est_element_data_t*));

/* ---- element level: src/Quadrature/d4est_quadrature.h:132-141 ------------------------------------------------------------ */
void d4est_quadrature_apply_stiffness_matrix(d4est_operators_t *d4est_ops,d4est_quadrature_t *d4est_quadrature,d4est_geometry_t *d4est_geometry,void *object,d4est_quadrature_object_type_t object_type,d4est_quadrature_integrand_type_t integrand_type,double *in,int deg_lobatto,double *jac_quad,double *rst_xyz[3][3],int deg_quad,double *out);
void d4est_quadrature_apply_mass_matrix(d4est_operators_t *d4est_ops,d4est_geometry_t *d4est_geometry,d4est_quadrature_t *d4est_quadrature,void *object,d4est_quadrature_object_type_t object_type,d4est_quadrature_integrand_type_t integrand_type,double *in,int deg_lobatto,double *jac_quad,int deg_quad,double *out);
void d4est_quadrature_apply_galerkin_integral(d4est_operators_t *d4est_ops,d4est_geometry_t *d4est_geometry,d4est_quadrature_t *d4est_quadrature,void *object,d4est_quadrature_object_type_t object_type,d4est_quadrature_integrand_type_t integrand_type,double *in_quad,int deg_lobatto,double *jac_quad,int deg_quad,double *out);
void d4est_quadrature_interpolate(d4est_operators_t *d4est_ops,d4est_quadrature_t *d4est_quadrature,d4est_geometry_t *d4est_geometry,void *object,d4est_quadrature_object_type_t object_type,d4est_quadrature_integrand_type_t integrand_type,double *u_lobatto_in,int deg_lobatto,double *u_quad_out,int deg_quad);
void d4est_quadrature_apply_inverse_mass_matrix(d4est_operators_t *d4est_ops,double *in,int deg_Lobatto,double *jac_Gauss,int deg_Gauss,int dim,double *out);
/* the mass terms of the nonlinear problems with their user callbacks (d4est_quadrature.h:135, :138; d4est_quadrature.c:776-936, :593-774),
 * called directly by the Problem files (src/Problems/ConstantDensityStar/constant_density_star_fcns.h:407, :575): the callbacks are host
 * function pointers, evaluated on the host at the quadrature nodes (or, interpolate_f, at the Lobatto nodes), the integrals run through
 * the shims above.  QUAD_COMPUTE_MATRIX (the dense element matrix the multigrid matrix operator asks for,
 * src/Solver/d4est_solver_multigrid_matrix_operator.c:215-238) is d4est_quadrature_compute_mass_matrix (:1143-1186) with jac * f(u) f(v): all
 * columns in one device call.  interpolate / apply_mass_matrix / apply_galerkin_integral
 * and these two also serve QUAD_OBJECT_MORTAR objects (dim - 1, on the host), as the reference's estimators and mesh update need. */
void d4est_quadrature_apply_fofufofvlj(d4est_operators_t *d4est_ops,d4est_geometry_t *d4est_geom,d4est_quadrature_t *d4est_quad,void *object,d4est_quadrature_object_type_t object_type,d4est_quadrature_integrand_type_t integrand_type,double *u,double *v,int deg_lobatto,double *jac_quad,double *xyz_quad[3],int deg_quad,double *out,d4est_xyzu_fcn_t fofu_fcn,void *fofu_ctx,d4est_xyzu_fcn_t fofv_fcn,void *fofv_ctx,int interpolate_f,double *xyz_lobatto[3]);
void d4est_quadrature_compute_mass_matrix(d4est_operators_t *d4est_ops,d4est_geometry_t *d4est_geometry,d4est_quadrature_t *d4est_quadrature,void *object,d4est_quadrature_object_type_t object_type,d4est_quadrature_integrand_type_t integrand_type,int deg_lobatto,double *jac_quad,int deg_quad,double *out);
void d4est_quadrature_apply_fofufofvlilj(d4est_operators_t *d4est_ops,d4est_geometry_t *d4est_geom,d4est_quadrature_t *d4est_quad,void *object,d4est_quadrature_object_type_t object_type,d4est_quadrature_integrand_type_t integrand_type,double *vec,double *u,double *v,int deg_lobatto,double *xyz_quad[3],double *jac_quad,int deg_quad,double *out,d4est_xyzu_fcn_t fofu_fcn,void *fofu_ctx,d4est_xyzu_fcn_t fofv_fcn,void *fofv_ctx,d4est_quadrature_apply_or_compute_matrix_t apply_or_compute_matrix,int interpolate_f,double *xyz_lobatto[3]);

/* ---- element level: src/dGMath/d4est_operators.h:69-126 -------------------------------------------------------------------- */
void d4est_operators_apply_dij(d4est_operators_t *d4est_ops,double *D4EST_RESTRICT in,int dim,int deg,int dir,double *D4EST_RESTRICT out);
void d4est_operators_apply_dij_transpose(d4est_operators_t *d4est_ops,double *D4EST_RESTRICT in,int dim,int deg,int dir,double *D4EST_RESTRICT out);
void d4est_operators_apply_lift(d4est_operators_t *d4est_ops,double *D4EST_RESTRICT in,int dim,int deg,int face,double *D4EST_RESTRICT out);
void d4est_operators_apply_slicer(d4est_operators_t *d4est_ops,double *D4EST_RESTRICT in,int dim,int face,int deg,double *D4EST_RESTRICT out);
void d4est_operators_apply_mij(d4est_operators_t *d4est_ops,double *D4EST_RESTRICT in,int dim,int deg,double *D4EST_RESTRICT out);
void d4est_operators_apply_invmij(d4est_operators_t *d4est_ops,double *D4EST_RESTRICT in,int dim,int deg,double *D4EST_RESTRICT out);
void d4est_operators_apply_p_prolong(d4est_operators_t *d4est_ops,double *D4EST_RESTRICT in,int degH,int dim,int degh,double *D4EST_RESTRICT out);
void d4est_operators_apply_hp_prolong(d4est_operators_t *d4est_ops,double *D4EST_RESTRICT in,int degH,int dim,int *degh,double *D4EST_RESTRICT out);
void d4est_operators_apply_p_restrict(d4est_operators_t *d4est_ops,double *D4EST_RESTRICT in,int degh,int dim,int degH,double *D4EST_RESTRICT out);
void d4est_operators_apply_hp_restrict(d4est_operators_t *d4est_ops,double *D4EST_RESTRICT in,int *degh,int dim,int degH,double *D4EST_RESTRICT out);
/* src/dGMath/d4est_operators.h:104, :107: the dense prolongation and the Galerkin product of the multigrid matrix operator's restriction
 * callback (src/Solver/d4est_solver_multigrid_matrix_operator.c:29).  compute_PT_mat_P forms sum_i P_i^T mat_i P_i; with eight children
 * the reference's own code reads a window of the transposed STACKED prolongation as the left factor (d4est_operators.c:651), which is not
 * P_i^T -- D4EST_HIP_REFERENCE_PT_WINDOW=1 reproduces that arithmetic to the letter (see DESIGN.md "MG matrix operator") */
void d4est_operators_compute_prolong_matrix(d4est_operators_t *d4est_ops,int degH,int dim,int *degh,int children,double *D4EST_RESTRICT prolong_mat);
void d4est_operators_compute_PT_mat_P(d4est_operators_t *d4est_ops,double *D4EST_RESTRICT mat,int degH,int dim,int *degh,int children,double *D4EST_RESTRICT PT_mat_P);
void d4est_operators_apply_p_prolong_transpose(d4est_operators_t *d4est_ops,double *D4EST_RESTRICT in,int degh,int dim,int degH,double *D4EST_RESTRICT out);
void d4est_operators_apply_hp_prolong_transpose(d4est_operators_t *d4est_ops,double *D4EST_RESTRICT in,int *degh,int dim,int degH,double *D4EST_RESTRICT out);

/* ---- operator / smoother level ---------------------------------------------------------------------------------------------
 * These take the p4est and the mesh-data structs, which the shims cannot read.  The host glue builds a
 * whole-mesh plan from them once per d4est_mesh_update and binds it to the p4est pointer; the shims look the plan up, run the
 * host-pointer entries of d4est_hip.h on the caller's vectors and ignore the other arguments.  An unbound p4est aborts.
 *   d4est_laplacian_apply_stiffness_matrix     src/dGMath/d4est_laplacian.h:22   u, Au: &vec[which_field * local_nodes]
 *   d4est_laplacian_apply_aij                  src/dGMath/d4est_laplacian.h:24   vectors from d4est_elliptic_data; flux_fcn_data
 *                                              is not read: SIPG parameters and boundary data are the plan's
 *   ..._smoother_cheby_iterate_aux             src/Solver/d4est_solver_multigrid_smoother_cheby.h:33; `fcns` is NOT called: the
 *                                              operator is the bound plan's apply_lhs (Laplacian + the zeroth-order term of
 *                                              d4est_hip_plan_set_lhs_coefficient), the whole loop runs on the device.  So that a
 *                                              caller with a DIFFERENT apply_lhs is not served the wrong operator silently, register
 *                                              the callback the plan stands for with d4est_hip_compat_bind_operator: the two shims
 *                                              then abort when fcns->apply_lhs is another function
 *   cg_eigs                                    src/Solver/d4est_solver_cg_eigs.h:9 */
/* also with the reference's own names and argument lists (registrations below supply what the opaque mesh structs would):
 *   d4est_laplacian_build_rhs_with_strong_bc   src/dGMath/d4est_laplacian.h:25  the source callback is evaluated on the host at the
 *                                              coordinates of d4est_hip_compat_bind_coordinates; boundary data as set on the plan
 *   d4est_solver_schwarz_iterate               src/Solver/d4est_solver_schwarz.h:42  on the handle of d4est_hip_compat_bind_schwarz
 *   d4est_operators_apply_flip, _reorient_face_data   src/dGMath/d4est_operators.h (index work, host)
 *   d4est_mortars_project_side_onto_mortar_space, _mass_mortar_onto_side   src/Mesh/d4est_mortars.h (face transfers, dim - 1, host)
 * apply_p_prolong & co. accept dim = 2 (faces: host) besides dim = 3 (device). */
void d4est_laplacian_build_rhs_with_strong_bc(p4est_t *p4est,d4est_ghost_t *ghost,d4est_ghost_data_t *ghost_data,d4est_operators_t *d4est_ops,d4est_geometry_t *d4est_geom,d4est_quadrature_t *d4est_quad,d4est_mesh_data_t *d4est_factors,d4est_elliptic_data_t *prob_vecs,d4est_laplacian_flux_data_t *flux_fcn_data_for_build_rhs,double *D4EST_RESTRICT rhs,d4est_xyz_fcn_t problem_rhs_fcn,d4est_mesh_init_field_option_t init_option,void *ctx,int which_field);
void d4est_solver_schwarz_iterate(p4est_t *p4est,d4est_geometry_t *d4est_geom,d4est_quadrature_t *d4est_quad,d4est_mesh_data_t *d4est_factors,d4est_ghost_t *ghost,d4est_solver_schwarz_t *schwarz,d4est_elliptic_data_t *vecs,double *r);
void d4est_operators_apply_flip(d4est_operators_t *d4est_ops,double *D4EST_RESTRICT in,int dim,int deg,int dir,double *out);
void d4est_operators_reorient_face_data(d4est_operators_t *d4est_ops,double *D4EST_RESTRICT in,int face_dim,int deg,int o,int f_m,int f_p,double *D4EST_RESTRICT out);
void d4est_mortars_project_side_onto_mortar_space(d4est_operators_t *d4est_ops,double *in_side,int faces_side,int *deg_side,double *out_mortar,int faces_mortar,int *deg_mortar);
void d4est_mortars_project_mass_mortar_onto_side(d4est_operators_t *dgmath,double *in_mortar,int faces_mortar,int *deg_mortar,double *out_side,int faces_side,int *deg_side);
void d4est_laplacian_apply_stiffness_matrix(p4est_t *p4est,d4est_operators_t *d4est_ops,d4est_geometry_t *d4est_geom,d4est_quadrature_t *d4est_quad,d4est_mesh_data_t *d4est_factors,double *D4EST_RESTRICT u,double *D4EST_RESTRICT Au,int local_nodes,int which_field);
void d4est_laplacian_apply_aij(p4est_t *p4est,d4est_ghost_t *d4est_ghost,d4est_ghost_data_t *d4est_ghost_data,d4est_elliptic_data_t *d4est_elliptic_data,d4est_laplacian_flux_data_t *flux_fcn_data,d4est_operators_t *d4est_ops,d4est_geometry_t *d4est_geom,d4est_quadrature_t *d4est_quad,d4est_mesh_data_t *d4est_factors,int which_field);
/* the "_with_opt" twins (src/dGMath/d4est_laplacian_with_opt.h:22-23): the reference's second implementation of the SAME operator,
 * which visits every face once and accumulates into both sides (d4est_laplacian_with_opt_flux_sipg.c:1231-1245); here they are the
 * same plan-bound applies as the two functions above */
void d4est_laplacian_with_opt_apply_stiffness_matrix(p4est_t *p4est,d4est_operators_t *d4est_ops,d4est_geometry_t *d4est_geom,d4est_quadrature_t *d4est_quad,d4est_mesh_data_t *d4est_factors,double *D4EST_RESTRICT u,double *D4EST_RESTRICT Au,int local_nodes,int which_field);
void d4est_laplacian_with_opt_apply_aij(p4est_t *p4est,d4est_ghost_t *d4est_ghost,d4est_ghost_data_t *d4est_ghost_data,d4est_elliptic_data_t *d4est_elliptic_data,d4est_laplacian_with_opt_flux_data_t *flux_fcn_data,d4est_operators_t *d4est_ops,d4est_geometry_t *d4est_geom,d4est_quadrature_t *d4est_quad,d4est_mesh_data_t *d4est_factors,int which_field);
void d4est_solver_multigrid_smoother_cheby_iterate_aux(p4est_t *p4est,d4est_operators_t *d4est_ops,d4est_geometry_t *d4est_geom,d4est_quadrature_t *d4est_quad,d4est_mesh_data_t *d4est_factors,d4est_ghost_t *d4est_ghost,d4est_ghost_data_t *d4est_ghost_data,d4est_elliptic_data_t *vecs,d4est_elliptic_eqns_t *fcns,double *r,int iter,double lmin,double lmax,int print_residual_norm,int mg_level,int compute_residual_at_end);
void cg_eigs(p4est_t *p4est,d4est_elliptic_data_t *vecs,d4est_elliptic_eqns_t *fcns,d4est_ghost_t *ghost,d4est_ghost_data_t *ghost_data,d4est_operators_t *d4est_ops,d4est_geometry_t *d4est_geom,d4est_quadrature_t *d4est_quad,d4est_mesh_data_t *d4est_factors,int imax,int print_spectral_bound_iterations,int use_new,double *spectral_bound);
/* src/Estimators/d4est_estimator_bi.h:201 (d4est_estimator_bi.c:343-560) on the bound plan, which must carry the estimator
 * (d4est_hip_plan_set_estimator).  As the reference: fcns->build_residual(p4est, ghost, ghost_data, prob_vecs, d4est_ops,
 * d4est_geom_for_residual, d4est_quad, d4est_factors_for_residual, fcns->user) leaves the residual in prob_vecs->Au (with the bound mesh
 * its apply_lhs already runs on the device); then u (field which_field) and Au go up and d4est_hip_estimator_bi runs.
 * Penalty functions: the reference's are static inline, so their addresses identify nothing -- each of the three is EVALUATED at fixed
 * probe arguments and matched against the ten closed forms of D4EST_HIP_EST_* (ids 1 / 9 and 3 / 6 are the same formula); no match,
 * or ids / prefactor other than the plan's, aborts.  Dirichlet data: u_bndry_fcn(x, y, z, bndry_ctx) at the boundary Lobatto face
 * nodes, taken from the Lobatto coordinates of d4est_hip_compat_bind_coordinates (required) through d4est_hip_plan_boundary_gather;
 * element diameters from d4est_hip_compat_bind_element_diameters or, when none are bound, the plan's own diam_volume
 * (d4est_hip_plan_compute_size_parameters_* / d4est_hip_plan_compute_diameters); neither aborts.  estimator_vtk (4 n, or NULL) receives the four terms;
 * estimator_vtk_per_face must be NULL (not supported: aborts).  The returned array of n doubles is allocated with sc_malloc(p4est_package_id,
 * .) when the process has libsc (found with dlsym(RTLD_DEFAULT, .)), so that the caller's P4EST_FREE releases it, else with malloc (plain-C
 * hosts without libsc: free it with free). */
double* d4est_estimator_bi_compute(p4est_t *p4est,d4est_elliptic_data_t *d4est_elliptic_data,d4est_elliptic_eqns_t *fcns,d4est_estimator_bi_penalty_data_t penalty_data,d4est_xyz_fcn_t u_bndry_fcn,void *bndry_ctx,d4est_ghost_t *d4est_ghost,d4est_ghost_data_t *d4est_ghost_data,d4est_operators_t *d4est_ops,d4est_geometry_t *d4est_geom_for_residual,d4est_mesh_data_t *d4est_factors_for_residual,d4est_geometry_t *d4est_geom_for_integrals,d4est_mesh_data_t *d4est_factors_for_integrals,d4est_quadrature_t *d4est_quad,int which_field,double *estimator_vtk,double *estimator_vtk_per_face);
/* ---- the columns of d4est_norms_save on the bound plan (include/d4est_hip.h "error norms") ------------------------------------------
 * The norm functions a driver lists in norm_fcns (src/IO/d4est_norms.h:68-75) and what they call.  Host vectors in; the vector goes
 * up, the norm runs on the device, the scalars come back.  Each returns this rank's LOCAL value -- sqrt of the local sum, the local
 * maximum -- where the reference returns the one reduced with sc_reduce: a one-rank run is unchanged, a multi-rank caller reduces the
 * squares itself.  A non-NULL skip_element_fcn ABORTS: d4est_element_data_t is opaque here, so it cannot be evaluated; evaluate it
 * per element into the skip mask of d4est_hip_norm_l2_sqr / d4est_hip_norm_linfty / d4est_hip_masked_sum instead.
 *   d4est_mesh_compute_l2_norm_sqr   src/Mesh/d4est_mesh.h (d4est_mesh.c:2299-2374)  l2_array (n_elements, or NULL) is filled
 *   d4est_norms_fcn_L2               d4est_norms.c:16-56     ctx: d4est_norms_fcn_L2_ctx_t, of which ctx->p4est is used
 *   d4est_norms_fcn_Linfty           d4est_norms.c:64-117    max(0, max_i v_i): the maximum of the values from 0, as the reference
 *   d4est_ip_energy_norm_compute     d4est_ip_energy_norm.c:286-448  the bound plan must carry d4est_hip_plan_set_energy_norm;
 *                                    u_penalty_fcn is EVALUATED at probe arguments and matched against the four SIPG closed forms
 *                                    (csrc/d4est_hip_compat_penalty.h); no match, or an id / prefactor other than the plan's, aborts.
 *                                    The three terms are left in energy_norm_data, the return value is their sum, not its root (as the
 *                                    reference).  which_field must be 0: the reference reads u without the field offset (:357)
 *   d4est_norms_fcn_energy           d4est_norms.c:201-244   ctx: d4est_norms_fcn_energy_ctx_t
 *   d4est_norms_fcn_energy_estimator d4est_norms.c:249-297   sqrt(ctx->energy_estimator_sq_local), as the reference without a skip
 *                                    function: a host value the driver formed -- on the device with d4est_hip_masked_sum(eta2) */
double d4est_mesh_compute_l2_norm_sqr(p4est_t *p4est,d4est_operators_t *d4est_ops,d4est_geometry_t *d4est_geom,d4est_quadrature_t *d4est_quad,d4est_mesh_data_t *d4est_factors,double *nodal_vec,int local_nodes,int(*skip_element_fcn)(d4est_element_data_t *),double *l2_array);
double d4est_norms_fcn_L2(p4est_t *p4est,double *field_value_errors,int num_nodes_local,void *norm_fcn_ctx,int(*skip_element_fcn)(d4est_element_data_t *));
double d4est_norms_fcn_Linfty(p4est_t *p4est,double *field_value_errors,int num_nodes_local,void *norm_fcn_ctx,int(*skip_element_fcn)(d4est_element_data_t *));
double d4est_ip_energy_norm_compute(p4est_t *p4est,double *u,d4est_ip_energy_norm_data_t *energy_norm_data,d4est_ghost_t *d4est_ghost,d4est_ghost_data_t *d4est_ghost_data,d4est_operators_t *d4est_ops,d4est_geometry_t *d4est_geom,d4est_quadrature_t *d4est_quad,d4est_mesh_data_t *d4est_factors,int which_field);
double d4est_norms_fcn_energy(p4est_t *p4est,double *field_value_errors,int num_nodes_local,void *norm_fcn_ctx,int(*skip_element_fcn)(d4est_element_data_t *));
double d4est_norms_fcn_energy_estimator(p4est_t *p4est,double *field_value_errors,int num_nodes_local,void *norm_fcn_ctx,int(*skip_element_fcn)(d4est_element_data_t *));
/* src/Quadrature/d4est_quadrature.h (d4est_quadrature.c:1019-1101): sum_q w_q [jac_q] u_q [v_q] at the quadrature nodes, v and jac_quad
 * may be NULL; volume (dim 3) and mortar (dim 2) objects, on the host in the reference's order of operations */
double d4est_quadrature_innerproduct(d4est_operators_t *d4est_ops,d4est_geometry_t *d4est_geom,d4est_quadrature_t *d4est_quad,void *object,d4est_quadrature_object_type_t object_type,d4est_quadrature_integrand_type_t integrand_type,double *u,double *v,double *jac_quad,int deg_quad);
/* src/dGMath/d4est_laplacian.h:21 (d4est_laplacian.c:236-281) on the bound plan: dudr_local[i] = D_i u of the local elements, on the
 * device (d4est_hip_compute_dudr).  The ghost elements' part needs the ghost layer, which is opaque here: dudr_ghost is not written,
 * and a bound plan that has ghost sides aborts when dudr_ghost is asked for (the engine exchanges traces, not element data) */
void d4est_laplacian_compute_dudr(p4est_t *p4est,d4est_ghost_t *d4est_ghost,d4est_ghost_data_t *d4est_ghost_data,d4est_operators_t *d4est_ops,d4est_geometry_t *d4est_geom,d4est_quadrature_t *d4est_quad,d4est_mesh_data_t *d4est_factors,double *dudr_local[3],double *dudr_ghost[3],double *D4EST_RESTRICT u,int local_nodes,int which_field);
/* src/dGMath/d4est_hessian.h (d4est_hessian.c:270-368) on the bound plan: del2field[local_nodes_quad] = the Laplacian of the host
 * vector field_lobatto[local_nodes] at the quadrature nodes (d4est_hip_hessian_trace).  The opaque pointers are not read.  The plan must
 * carry the coefficients of the form compute_method names -- HESSIAN_ANALYTICAL: d4est_hip_plan_set_hessian_analytic or _brick (the
 * brick's D2X is analytic and zero), HESSIAN_NUMERICAL: _set_hessian_numerical -- and any other combination aborts */
typedef int d4est_hessian_compute_method_t;                     /* enum {HESSIAN_ANALYTICAL, HESSIAN_NUMERICAL}, d4est_hessian.h:14 */
#define HESSIAN_ANALYTICAL 0
#define HESSIAN_NUMERICAL 1
void d4est_hessian_compute_hessian_trace_of_field_on_quadrature_points(p4est_t *p4est,d4est_operators_t *d4est_ops,d4est_geometry_t *d4est_geom,d4est_quadrature_t *d4est_quad,d4est_mesh_data_t *d4est_factors,d4est_hessian_compute_method_t compute_method,double *field_lobatto,double *del2field);
/* src/Mesh/d4est_mesh.h:63-80 and :208 (d4est_mesh.c:3294-3362) on the bound plan: the value of the host nodal vector f at tree
 * coordinates abc of tree tree_id, through a one-point d4est_hip_probe (locate, rst, the product-form Lagrange value; include/d4est_hip.h
 * "point probes").  The struct is the reference's, member for member (p4est_qcoord_t = int32_t), returned by value.  Where the forest's
 * elements sit is opaque here: register it with d4est_hip_compat_bind_forest (required; aborts without).  err = 1 when no local element
 * of the bound plan contains the point; as in the reference only err is then set -- here the other members are zero, f_at_xyz a NaN.
 * xyz is filled when a map was registered with the forest, else zero.  print is ignored (the reference's printf is commented out). */
typedef struct {
  int err;
  double f_at_xyz;
  int nodal_stride;
  double xyz [3];
  double rst [3];
  double abc [3];
  int id;
  int q [3];
  int dq;
} d4est_mesh_interpolate_data_t;
d4est_mesh_interpolate_data_t d4est_mesh_interpolate_at_tree_coord(p4est_t *p4est,d4est_operators_t *d4est_ops,d4est_geometry_t *d4est_geom,double abc[3],int tree_id,double *f,int print);
#endif /* D4EST_HIP_COMPAT_NO_TYPES */

/* ---- binding (not in the reference) ------------------------------------------------------------------------------------------ */
/* associate a whole-mesh plan with a p4est pointer (call after every d4est_mesh_update; re-binding replaces; plan = NULL unbinds).
 * The plan stays owned by the caller. */
void d4est_hip_compat_bind_mesh(const void* p4est, d4est_hip_plan_t* plan);
d4est_hip_plan_t* d4est_hip_compat_bound_plan(const void* p4est);
#ifndef D4EST_HIP_COMPAT_NO_TYPES
/* the apply_lhs callback whose operator the bound plan applies (e.g. constant_density_star_apply_jac): cheby_iterate_aux / cg_eigs abort
 * on any other fcns->apply_lhs; NULL removes the registration (then fcns is not looked at) */
void d4est_hip_compat_bind_operator(const void* p4est, d4est_apply_operator_fcn_t apply_lhs);
/* what the bound plan was set up with: [flux] sipg_penalty_prefactor and the boundary-condition type (BC_ROBIN 0 / BC_DIRICHLET 1).  Once
 * registered, d4est_laplacian_apply_aij, its _with_opt twin and d4est_laplacian_build_rhs_with_strong_bc ABORT when the flux data the
 * caller passes says otherwise (other flux type, other prefactor, other bc_type) instead of silently applying the plan's operator */
void d4est_hip_compat_bind_flux(const void* p4est, double sipg_penalty_prefactor, int bc_type);
/* the node coordinates of the mesh (d4est_factors->xyz[d] at the Lobatto nodes, ->xyz_quad[d] at the quadrature nodes; host arrays that
 * stay the caller's; either may be NULL): where d4est_laplacian_build_rhs_with_strong_bc evaluates the source callback */
void d4est_hip_compat_bind_coordinates(const void* p4est, double* xyz_lobatto[3], double* xyz_quad[3]);
/* d4est_factors->diam_volume (host array of the local elements, stays the caller's): the h of the estimator's residual term; takes
 * precedence over the diam_volume the plan computed itself */
void d4est_hip_compat_bind_element_diameters(const void* p4est, const double* diam_volume);
/* where the local elements of the bound plan sit in the forest -- d4est_element_data_t::tree, ::q[3], ::dq of every local element in
 * traversal order, root_len = P4EST_ROOT_LEN (host arrays, COPIED; call after every d4est_hip_compat_bind_mesh) -- and, optionally, the
 * map for data.xyz: geom_type / params of d4est_hip_probe_set_map, or geom_type < 0 for none.  For d4est_mesh_interpolate_at_tree_coord;
 * elem_tree = NULL removes the registration */
void d4est_hip_compat_bind_forest(const void* p4est, const int* elem_tree, const int* elem_q, const int* elem_dq, double root_len,
                                  int geom_type, const double* params);
/* the Schwarz smoother of this mesh and its three [d4est_solver_schwarz] CG options, for d4est_solver_schwarz_iterate; NULL unbinds */
void d4est_hip_compat_bind_schwarz(const void* p4est, d4est_hip_schwarz_t* sz, int subdomain_iter, double subdomain_atol, double subdomain_rtol);
/* the reference's Schwarz metadata as the flat arrays d4est_hip_schwarz_create takes; outputs caller-allocated:
 * sub_first[num_subdomains + 1], sub_elem[num_elements], sub_faces / sub_core_faces[3 num_elements] */
void d4est_hip_compat_flatten_schwarz_metadata(const d4est_solver_schwarz_metadata_t* md, int* sub_first, int* sub_elem, int* sub_faces, int* sub_core_faces);
/* d4est_laplacian_build_rhs_with_strong_bc (src/dGMath/d4est_laplacian.c:16-140) on the bound plan, with the source values handed over: rhs[which_field] = M f - A(0).
 * The reference's function evaluates the source callback through d4est_mesh_init_field (it needs the p4est and the mesh data, which
 * the shims cannot read), so the caller does that step -- one call it already has -- and passes the values: f at the Lobatto nodes
 * (init_option 1 = INIT_FIELD_ON_LOBATTO) or at the quadrature nodes (2 = INIT_FIELD_ON_QUAD; the values of d4est_mesh_init_field_option_t).  Boundary data: set the inhomogeneous
 * values on the plan first (d4est_hip_plan_set_dirichlet_values), the homogeneous ones afterwards.  INTEGRATION.md section 3. */
void d4est_hip_compat_build_rhs_with_strong_bc(const void* p4est, d4est_elliptic_data_t* prob_vecs, double* rhs, const double* f, int init_option, int which_field);
#endif
/* free the cached one-element plans, transfer objects and staging buffers of the element-level shims */
void d4est_hip_compat_release(void);

#ifdef __cplusplus
}
#endif
#endif /* D4EST_HIP_COMPAT_H */
