/* Plain C99 host that calls the error estimator through the REFERENCE's OWN PROTOTYPE, d4est_estimator_bi_compute
 * (src/Estimators/d4est_estimator_bi.h:201, include/d4est_hip_compat.h), with penalty functions of its own written as the reference
 * writes houston_gradu_prefactor_maxp_minh / houston_u_prefactor_maxp_minh / houston_u_dirichlet_prefactor_maxp_minh
 * (d4est_estimator_bi.h:152-196: config 4's choice), and checks the result against the device entry point d4est_hip_estimator_bi fed
 * with the same residual, diameters and Dirichlet data formed here.  No Python, no C++.
 *
 * Build / run: tests/test_estimator_compat_gpu.py.  Prints one line per check; exit code 0 = all within tolerance.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "d4est_hip_compat.h"

static int n_fail = 0;

static double lcg(unsigned long long* s) {
  *s = *s * 6364136223846793005ULL + 1442695040888963407ULL;
  return (double)(*s >> 11) / 9007199254740992.0;
}

static void check(const char* what, int p, const double* got, const double* ref, int n, double tol) {
  double num = 0, den = 0;
  for (int i = 0; i < n; i++) {
    const double d = fabs(got[i] - ref[i]);
    if (!(d <= num)) num = d;      /* (NaN propagates) */
    if (fabs(ref[i]) > den) den = fabs(ref[i]);
  }
  const double rel = num / (den > 0 ? den : 1);
  if (!(rel <= tol)) n_fail++;
  printf("%-40s p=%2d  n=%6d  rel-inf %.2e %s\n", what, p, n, rel, (rel <= tol) ? "" : "FAIL");
}

static double* vec(int n) { return (double*)calloc((size_t)(n > 0 ? n : 1), sizeof(double)); }

/* the three penalty functions, copied as formulas (the reference's are static inline in its header) */
static double my_gradu(int deg_m, double h_m, int deg_p, double h_p, double c) {
  (void)c;
  const double max_p = deg_m > deg_p ? deg_m : deg_p, min_h = h_m < h_p ? h_m : h_p;
  return sqrt(.5 * min_h / max_p);
}
static double my_u(int deg_m, double h_m, int deg_p, double h_p, double c) {
  const double max_p = deg_m > deg_p ? deg_m : deg_p, min_h = h_m < h_p ? h_m : h_p;
  return sqrt(.5 * c * max_p * max_p / min_h);
}
static double my_u_dirichlet(int deg_m, double h_m, int deg_p, double h_p, double c) {
  const double max_p = deg_m > deg_p ? deg_m : deg_p, min_h = h_m < h_p ? h_m : h_p;
  return sqrt(c * max_p * max_p / min_h);
}
static double probe_bndry(double x, double y, double z, void* ctx) { return *(double*)ctx + x * y - 0.5 * z; }   /* d4est_xyz_fcn_t */

static double* g_rhs = NULL;
/* build_residual of a Poisson problem (e.g. poisson_sinx_fcns.h): Au = rhs - A u, A through the reference-named operator shim */
static void probe_build_residual(p4est_t* p4est, d4est_ghost_t* ghost, d4est_ghost_data_t* ghost_data, d4est_elliptic_data_t* v,
                                 d4est_operators_t* ops, d4est_geometry_t* geom, d4est_quadrature_t* quad, d4est_mesh_data_t* factors, void* user) {
  (void)user;
  d4est_laplacian_apply_aij(p4est, ghost, ghost_data, v, NULL, ops, geom, quad, factors, 0);
  for (int i = 0; i < v->local_nodes; i++) v->Au[i] = g_rhs[i] - v->Au[i];
}

static void run(int p) {
  const int ne = 8, N = p + 1, n3 = N * N * N, n2 = N * N, ln = ne * n3;
  const double h = 0.5;
  int deg[8], degq[8], ns[8], qs[8];
  for (int e = 0; e < ne; e++) { deg[e] = degq[e] = p; ns[e] = qs[e] = e * n3; }
  int side_nbr[48], side_nbr_face[48], side_reorder[48], side_mortar_stride[48], side_bndry_stride[48];
  int total_mortar = 0, total_bndry = 0;
  for (int e = 0; e < ne; e++)
    for (int f = 0; f < 6; f++) {
      const int s = 6 * e + f, d = f / 2, pos = f % 2, c = (e >> d) & 1;
      side_nbr_face[s] = f ^ 1; side_reorder[s] = 0;
      side_nbr[s] = (c == pos) ? -1 : (e ^ (1 << d));
      side_mortar_stride[s] = total_mortar; total_mortar += n2;
      side_bndry_stride[s] = total_bndry; if (side_nbr[s] == -1) total_bndry += n2;
    }
  double *J = vec(ln), *rst = vec(9 * ln);
  for (int i = 0; i < ln; i++) { J[i] = h * h * h / 8; for (int a = 0; a < 3; a++) rst[(size_t)(3 * a + a) * ln + i] = 2 / h; }
  double *sj = vec(total_mortar), *nrm = vec(3 * total_mortar), *dm = vec(9 * total_mortar), *hm = vec(total_mortar);
  for (int s = 0; s < 48; s++) {
    const int S = side_mortar_stride[s], f = s % 6, d = f / 2;
    for (int k = 0; k < n2; k++) {
      sj[S + k] = h * h / 4; hm[S + k] = h / 2;
      nrm[3 * S + d * n2 + k] = (f % 2) ? 1.0 : -1.0;
      for (int a = 0; a < 3; a++) dm[9 * S + (a + 3 * a) * n2 + k] = 2 / h;
    }
  }
  const double pref = 10.0;
  d4est_hip_plan_t* plan = d4est_hip_plan_create(ne, deg, degq, ns, qs, D4EST_HIP_QUAD_LEGENDRE);
  d4est_hip_plan_set_geometry(plan, J, rst, 0);
  d4est_hip_plan_set_estimator(plan, D4EST_HIP_EST_HOUSTON_GRADU_MAXP_MINH, D4EST_HIP_EST_HOUSTON_U_MAXP_MINH,
                               D4EST_HIP_EST_HOUSTON_U_DIRICHLET_MAXP_MINH, pref);
  d4est_hip_plan_set_faces(plan, side_nbr, side_nbr_face, side_reorder, side_mortar_stride, side_bndry_stride, total_mortar, total_bndry, 0, NULL, NULL);
  d4est_hip_plan_set_sipg(plan, pref, 0);
  d4est_hip_plan_set_mortar_geometry(plan, sj, nrm, dm, dm, hm, hm, 0);
  int fake_p4est_storage = 0;
  p4est_t* p4est = (p4est_t*)&fake_p4est_storage;       /* the shims use the pointer as a key only */
  d4est_hip_compat_bind_mesh(p4est, plan);
  /* Lobatto node coordinates (d4est_factors->xyz) and element diameters (->diam_volume) */
  double* x1 = vec(N);
  d4est_hip_table(D4EST_HIP_TABLE_LOBATTO_NODES, p, 0, x1);
  double* xl[3];
  for (int d = 0; d < 3; d++) xl[d] = vec(ln);
  for (int e = 0; e < ne; e++)
    for (int k = 0; k < N; k++)
      for (int j = 0; j < N; j++)
        for (int i = 0; i < N; i++) {
          const int id[3] = {i, j, k}, v = ns[e] + i + N * (j + N * k);
          for (int d = 0; d < 3; d++) xl[d][v] = h * (((e >> d) & 1) + 0.5 * (x1[id[d]] + 1.0));
        }
  double diam[8];
  for (int e = 0; e < ne; e++) diam[e] = sqrt(3.0) * h * (1.0 + 0.01 * e);
  d4est_hip_compat_bind_coordinates(p4est, xl, NULL);
  d4est_hip_compat_bind_element_diameters(p4est, diam);

  unsigned long long seed = 7 + p;
  double *u = vec(ln), *Au = vec(ln), *res = vec(ln);
  g_rhs = vec(ln);
  for (int i = 0; i < ln; i++) { u[i] = lcg(&seed) - 0.5; g_rhs[i] = lcg(&seed) - 0.5; }
  d4est_elliptic_data_t vecs;
  memset(&vecs, 0, sizeof vecs);
  vecs.local_nodes = ln; vecs.num_of_fields = 1; vecs.u = u; vecs.Au = Au; vecs.rhs = g_rhs;
  d4est_elliptic_eqns_t fcns;
  memset(&fcns, 0, sizeof fcns);
  fcns.build_residual = probe_build_residual;
  d4est_estimator_bi_penalty_data_t pd;
  memset(&pd, 0, sizeof pd);
  pd.gradu_penalty_fcn = my_gradu; pd.u_penalty_fcn = my_u; pd.u_dirichlet_penalty_fcn = my_u_dirichlet; pd.penalty_prefactor = pref;
  double ctx = 0.3, *vtk = vec(4 * ne);
  double* est = d4est_estimator_bi_compute(p4est, &vecs, &fcns, pd, probe_bndry, &ctx, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0,
                                           vtk, NULL);

  /* the same through the device entry point, inputs formed here: residual, Dirichlet data at the boundary face nodes (slicer order) */
  vecs.Au = res;
  probe_build_residual(p4est, NULL, NULL, &vecs, NULL, NULL, NULL, NULL, NULL);
  double* g = vec(total_bndry);
  for (int e = 0; e < ne; e++)
    for (int f = 0; f < 6; f++) {
      const int s = 6 * e + f, d = f / 2, fix = (f & 1) ? N - 1 : 0;
      if (side_nbr[s] != -1) continue;
      const int t0 = d == 0 ? 1 : 0, t1 = d == 2 ? 1 : 2;
      for (int b = 0; b < N; b++)
        for (int a = 0; a < N; a++) {
          int id[3];
          id[d] = fix; id[t0] = a; id[t1] = b;
          const int v = ns[e] + id[0] + N * (id[1] + N * id[2]);
          g[side_bndry_stride[s] + a + N * b] = probe_bndry(xl[0][v], xl[1][v], xl[2][v], &ctx);
        }
    }
  const size_t vb = sizeof(double) * ln;
  double *d_u = d4est_hip_malloc(vb), *d_r = d4est_hip_malloc(vb), *d_g = d4est_hip_malloc(sizeof(double) * total_bndry),
         *d_diam = d4est_hip_malloc(sizeof diam), *d_eta = d4est_hip_malloc(sizeof(double) * ne), *d_t = d4est_hip_malloc(sizeof(double) * 4 * ne);
  d4est_hip_memcpy_h2d(d_u, u, vb);
  d4est_hip_memcpy_h2d(d_r, res, vb);
  d4est_hip_memcpy_h2d(d_g, g, sizeof(double) * total_bndry);
  d4est_hip_memcpy_h2d(d_diam, diam, sizeof diam);
  d4est_hip_estimator_bi(plan, d_u, NULL, d_r, d_diam, d_g, d_eta, d_t);
  d4est_hip_plan_synchronize(plan);
  double ref[8], *ref_t = vec(4 * ne);
  d4est_hip_memcpy_d2h(ref, d_eta, sizeof ref);
  d4est_hip_memcpy_d2h(ref_t, d_t, sizeof(double) * 4 * ne);
  check("d4est_estimator_bi_compute: residual", p, Au, res, ln, 0.0);
  check("d4est_estimator_bi_compute: estimator", p, est, ref, ne, 1e-14);
  check("d4est_estimator_bi_compute: estimator_vtk", p, vtk, ref_t, 4 * ne, 1e-14);
  int all_terms = 1;
  for (int t = 0; t < 4; t++) {
    double mx = 0;
    for (int e = 0; e < ne; e++) mx = fabs(ref_t[t * ne + e]) > mx ? fabs(ref_t[t * ne + e]) : mx;
    all_terms = all_terms && mx > 0;
  }
  if (!all_terms) n_fail++;
  printf("%-40s p=%2d  every term non-zero %s\n", "d4est_estimator_bi_compute: terms", p, all_terms ? "" : "FAIL");
  free(est);   /* no libsc in this process: the shim allocated with malloc */
  d4est_hip_free(d_u); d4est_hip_free(d_r); d4est_hip_free(d_g); d4est_hip_free(d_diam); d4est_hip_free(d_eta); d4est_hip_free(d_t);
  d4est_hip_compat_bind_mesh(p4est, NULL);
  d4est_hip_plan_destroy(plan);
  for (int d = 0; d < 3; d++) free(xl[d]);
  free(x1); free(J); free(rst); free(sj); free(nrm); free(dm); free(hm); free(u); free(Au); free(res); free(g_rhs); free(g); free(vtk); free(ref_t);
}

int main(void) {
  if (d4est_hip_device_count() < 1) { fprintf(stderr, "no HIP device\n"); return 77; }
  run(3);
  run(7);
  printf(n_fail ? "MISMATCH (%d)\n" : "ok\n", n_fail);
  return n_fail ? 1 : 0;
}
