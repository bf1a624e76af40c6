/* Plain C99 host that calls the error norms through the REFERENCE's OWN PROTOTYPES (include/d4est_hip_compat.h): d4est_mesh_compute_l2_norm_sqr,
 * d4est_norms_fcn_L2, d4est_norms_fcn_Linfty, d4est_ip_energy_norm_compute, d4est_norms_fcn_energy, d4est_norms_fcn_energy_estimator,
 * d4est_quadrature_innerproduct and d4est_laplacian_compute_dudr, with penalty functions of its own written as the reference writes its four
 * (src/dGMath/d4est_laplacian_flux_sipg.c:945-1005).  Each is checked against the device entry point of include/d4est_hip.h fed with the
 * same vector, and against values known by hand on the unit cube of 2 x 2 x 2 elements: the L2 norm of 1 is the volume, u = x has a volume
 * term equal to the volume and no interface term.  No Python, no C++.
 *
 * `norms_probe skip` touches no device: it hands d4est_norms_fcn_energy a skip_element_fcn and must end in the abort message.
 *
 * Build / run: tests/test_norms_compat_gpu.py.  Prints one line per check; exit code 0 = all within tolerance.
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
  printf("%-46s p=%2d  n=%6d  rel-inf %.2e %s\n", what, p, n, rel, (rel <= tol) ? "" : "FAIL");
}

static double* vec(int n) { return (double*)calloc((size_t)(n > 0 ? n : 1), sizeof(double)); }

/* the four penalty functions, copied as formulas (the reference's are static in its .c file) */
static double my_maxp_sqr_over_minh(int deg_m, double h_m, int deg_p, double h_p, double c) {
  const double max_deg = (deg_m > deg_p) ? deg_m : deg_p, min_h = (h_m < h_p) ? h_m : h_p;
  return (c * max_deg * max_deg) / min_h;
}
static double my_meanp_sqr_over_meanh(int deg_m, double h_m, int deg_p, double h_p, double c) {
  const double mean_p = .5 * (deg_m + deg_p), mean_h = .5 * (h_m + h_p);
  return (c * mean_p * mean_p) / mean_h;
}
static double my_maxpp1_sqr_over_minh(int deg_m, double h_m, int deg_p, double h_p, double c) {
  const double max_deg = (deg_m > deg_p) ? deg_m : deg_p, min_h = (h_m < h_p) ? h_m : h_p;
  return (c * (max_deg + 1) * (max_deg + 1)) / min_h;
}
static double my_mean_p_sqr_over_h(int deg_m, double h_m, int deg_p, double h_p, double c) {
  return c * (.5 * (deg_m * deg_m / h_m + deg_p * deg_p / h_p));
}
static const penalty_calc_t my_penalty[4] = {my_maxp_sqr_over_minh, my_meanp_sqr_over_meanh, my_maxpp1_sqr_over_minh, my_mean_p_sqr_over_h};

static int skip_odd(d4est_element_data_t* ed) { (void)ed; return 1; }

static void run(int p, int fcn_id) {
  const int ne = 8, N = p + 1, n3 = N * N * N, n2 = N * N, ln = ne * n3;
  const double h = 0.5, pref = 10.0;
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
  d4est_hip_plan_t* plan = d4est_hip_plan_create(ne, deg, degq, ns, qs, D4EST_HIP_QUAD_LEGENDRE);
  d4est_hip_plan_set_geometry(plan, J, rst, 0);
  d4est_hip_plan_set_energy_norm(plan, fcn_id, pref);
  d4est_hip_plan_set_faces(plan, side_nbr, side_nbr_face, side_reorder, side_mortar_stride, side_bndry_stride, total_mortar, total_bndry, 0, NULL, NULL);
  d4est_hip_plan_set_sipg(plan, pref, 0);
  d4est_hip_plan_set_mortar_geometry(plan, sj, nrm, dm, dm, hm, hm, 0);
  int fake_p4est_storage = 0;
  p4est_t* p4est = (p4est_t*)&fake_p4est_storage;       /* the shims use the pointer as a key only */
  d4est_hip_compat_bind_mesh(p4est, plan);

  /* x at the Lobatto nodes, a random error field, the constant 1 */
  double* x1 = vec(N);
  d4est_hip_table(D4EST_HIP_TABLE_LOBATTO_NODES, p, 0, x1);
  double *x = vec(ln), *one = vec(ln), *v = vec(ln);
  unsigned long long seed = 11 + p;
  for (int e = 0; e < ne; e++)
    for (int k = 0; k < N; k++)
      for (int j = 0; j < N; j++)
        for (int i = 0; i < N; i++) {
          const int id = ns[e] + i + N * (j + N * k);
          x[id] = h * ((e & 1) + 0.5 * (x1[i] + 1.0));
          one[id] = 1.0;
          v[id] = lcg(&seed) - 0.25;
        }

  /* the device entry points on the same vector */
  const size_t vb = sizeof(double) * ln;
  double *d_v = d4est_hip_malloc(vb), *d_out = d4est_hip_malloc(sizeof(double) * (ne + 8));
  d4est_hip_memcpy_h2d(d_v, v, vb);
  d4est_hip_norm_l2_sqr(plan, d_v, NULL, d_out + 8, d_out);
  d4est_hip_norm_linfty(plan, d_v, NULL, d_out + 1);
  d4est_hip_ip_energy_norm_sqr(plan, d_v, NULL, NULL, d_out + 2);
  d4est_hip_plan_synchronize(plan);
  double ref[8], *ref_arr = vec(ne);
  d4est_hip_memcpy_d2h(ref, d_out, sizeof ref);
  d4est_hip_memcpy_d2h(ref_arr, d_out + 8, sizeof(double) * ne);

  /* L2 */
  double* l2_array = vec(ne);
  double got = d4est_mesh_compute_l2_norm_sqr(p4est, NULL, NULL, NULL, NULL, v, ln, NULL, l2_array);
  check("d4est_mesh_compute_l2_norm_sqr: sum", p, &got, &ref[0], 1, 0.0);
  check("d4est_mesh_compute_l2_norm_sqr: l2_array", p, l2_array, ref_arr, ne, 0.0);
  d4est_norms_fcn_L2_ctx_t l2_ctx;
  memset(&l2_ctx, 0, sizeof l2_ctx);
  l2_ctx.p4est = p4est;
  double want = sqrt(ref[0]);
  got = d4est_norms_fcn_L2(p4est, v, ln, &l2_ctx, NULL);
  check("d4est_norms_fcn_L2", p, &got, &want, 1, 0.0);
  want = 1.0;   /* the volume of the unit cube */
  got = d4est_mesh_compute_l2_norm_sqr(p4est, NULL, NULL, NULL, NULL, one, ln, NULL, NULL);
  check("d4est_mesh_compute_l2_norm_sqr: |1|^2 = volume", p, &got, &want, 1, 1e-13);

  /* L-infinity: exact, and 0 for an all-negative vector */
  want = 0.0;
  for (int i = 0; i < ln; i++) want = v[i] > want ? v[i] : want;
  got = d4est_norms_fcn_Linfty(p4est, v, ln, NULL, NULL);
  check("d4est_norms_fcn_Linfty", p, &got, &want, 1, 0.0);
  check("d4est_norms_fcn_Linfty: device", p, &got, &ref[1], 1, 0.0);
  double* neg = vec(ln);
  for (int i = 0; i < ln; i++) neg[i] = -1.0 - v[i] * v[i];
  want = 0.0;
  got = d4est_norms_fcn_Linfty(p4est, neg, ln, NULL, NULL);
  check("d4est_norms_fcn_Linfty: all negative -> 0", p, &got, &want, 1, 0.0);

  /* IP energy norm */
  d4est_ip_energy_norm_data_t nd;
  memset(&nd, 0, sizeof nd);
  nd.u_penalty_fcn = my_penalty[fcn_id];
  nd.penalty_prefactor = pref;
  got = d4est_ip_energy_norm_compute(p4est, v, &nd, NULL, NULL, NULL, NULL, NULL, NULL, 0);
  const double terms[3] = {nd.ip_energy_norm_sqr_volume_term, nd.ip_energy_norm_sqr_boundary_term, nd.ip_energy_norm_sqr_interface_term};
  check("d4est_ip_energy_norm_compute: three terms", p, terms, &ref[2], 3, 0.0);
  check("d4est_ip_energy_norm_compute: return value", p, &got, &ref[5], 1, 0.0);
  want = (terms[0] + terms[1]) + terms[2];
  check("d4est_ip_energy_norm_compute: v + b + i", p, &got, &want, 1, 0.0);
  const int all_terms = terms[0] > 0 && terms[1] > 0 && terms[2] > 0;
  if (!all_terms) n_fail++;
  printf("%-46s p=%2d  every term positive %s\n", "d4est_ip_energy_norm_compute: terms", p, all_terms ? "" : "FAIL");
  d4est_norms_fcn_energy_ctx_t e_ctx;
  memset(&e_ctx, 0, sizeof e_ctx);
  e_ctx.p4est = p4est; e_ctx.energy_norm_data = &nd; e_ctx.which_field = 0; e_ctx.energy_estimator_sq_local = 6.25;
  want = sqrt(ref[5]);
  got = d4est_norms_fcn_energy(p4est, v, ln, &e_ctx, NULL);
  check("d4est_norms_fcn_energy", p, &got, &want, 1, 0.0);
  want = 2.5;
  got = d4est_norms_fcn_energy_estimator(p4est, v, ln, &e_ctx, NULL);
  check("d4est_norms_fcn_energy_estimator", p, &got, &want, 1, 0.0);
  /* u = x: |grad u|^2 = 1 over the unit cube, no jump; the boundary term is pen * int x^2 over the faces, here only > 0 is asked */
  (void)d4est_ip_energy_norm_compute(p4est, x, &nd, NULL, NULL, NULL, NULL, NULL, NULL, 0);
  want = 1.0;
  check("d4est_ip_energy_norm_compute: u = x, volume", p, &nd.ip_energy_norm_sqr_volume_term, &want, 1, 1e-12);
  const int no_jump = fabs(nd.ip_energy_norm_sqr_interface_term) <= 1e-12 * nd.ip_energy_norm_sqr_boundary_term;
  if (!no_jump) n_fail++;
  printf("%-46s p=%2d  interface %.2e of boundary %.6e %s\n", "d4est_ip_energy_norm_compute: u = x, interface", p,
         nd.ip_energy_norm_sqr_interface_term, nd.ip_energy_norm_sqr_boundary_term, no_jump ? "" : "FAIL");
  /* boundary closed form: the faces x = 1 (int 1), and the four faces along x (int x^2 = 1/3 each); pen(p, h/2, p, h/2) is constant */
  want = my_penalty[fcn_id](p, h / 2, p, h / 2, pref) * (1.0 + 4.0 / 3.0);
  check("d4est_ip_energy_norm_compute: u = x, boundary", p, &nd.ip_energy_norm_sqr_boundary_term, &want, 1, 1e-12);

  /* d4est_quadrature_innerproduct: volume and mortar objects against the sum written out here */
  {
    double* w = vec(N);
    d4est_hip_table(D4EST_HIP_TABLE_GAUSS_WEIGHTS, p, 0, w);
    int quad_type = 0;   /* QUAD_TYPE_GAUSS_LEGENDRE: the first member of d4est_quadrature_t */
    d4est_quadrature_t* quad = (d4est_quadrature_t*)&quad_type;
    double s3 = 0, s2 = 0, s3nov = 0;
    for (int k = 0; k < N; k++)
      for (int j = 0; j < N; j++)
        for (int i = 0; i < N; i++) {
          const int id = i + N * (j + N * k);
          s3 += J[id] * (w[k] * w[j] * w[i] * v[id] * x[id]);
          s3nov += w[k] * w[j] * w[i] * v[id];
        }
    for (int j = 0; j < N; j++)
      for (int i = 0; i < N; i++) s2 += sj[i + N * j] * (w[j] * w[i] * v[i + N * j] * x[i + N * j]);
    got = d4est_quadrature_innerproduct(NULL, NULL, quad, NULL, QUAD_OBJECT_VOLUME, QUAD_INTEGRAND_UNKNOWN, v, x, J, p);
    check("d4est_quadrature_innerproduct: volume", p, &got, &s3, 1, 1e-15);
    got = d4est_quadrature_innerproduct(NULL, NULL, quad, NULL, QUAD_OBJECT_VOLUME, QUAD_INTEGRAND_UNKNOWN, v, NULL, NULL, p);
    check("d4est_quadrature_innerproduct: no v, no jac", p, &got, &s3nov, 1, 1e-15);
    got = d4est_quadrature_innerproduct(NULL, NULL, quad, NULL, QUAD_OBJECT_MORTAR, QUAD_INTEGRAND_UNKNOWN, v, x, sj, p);
    check("d4est_quadrature_innerproduct: mortar", p, &got, &s2, 1, 1e-15);
    free(w);
  }

  /* d4est_laplacian_compute_dudr against the element-level d4est_operators_apply_dij */
  {
    double *dl[3], *want_d = vec(ln);
    for (int i = 0; i < 3; i++) dl[i] = vec(ln);
    d4est_laplacian_compute_dudr(p4est, NULL, NULL, NULL, NULL, NULL, NULL, dl, NULL, v, ln, 0);
    for (int i = 0; i < 3; i++) {
      for (int e = 0; e < ne; e++) d4est_operators_apply_dij(NULL, v + ns[e], 3, p, i, want_d + ns[e]);
      check("d4est_laplacian_compute_dudr", p, dl[i], want_d, ln, 1e-14);
      free(dl[i]);
    }
    free(want_d);
  }

  d4est_hip_free(d_v); d4est_hip_free(d_out);
  d4est_hip_compat_bind_mesh(p4est, NULL);
  d4est_hip_plan_destroy(plan);
  free(x1); free(x); free(one); free(v); free(neg); free(l2_array); free(ref_arr);
  free(J); free(rst); free(sj); free(nrm); free(dm); free(hm);
}

int main(int argc, char** argv) {
  if (argc > 1 && strcmp(argv[1], "skip") == 0) {
    /* no device work before the check: the shim must abort on the skip function itself (d4est_norms.c:211-213) */
    d4est_norms_fcn_energy_ctx_t e_ctx;
    memset(&e_ctx, 0, sizeof e_ctx);
    double v1 = 0;
    (void)d4est_norms_fcn_energy(NULL, &v1, 1, &e_ctx, skip_odd);
    printf("returned\n");
    return 0;
  }
  if (argc > 1 && strcmp(argv[1], "skip-l2") == 0) {
    d4est_norms_fcn_L2_ctx_t l2_ctx;
    memset(&l2_ctx, 0, sizeof l2_ctx);
    double v1 = 0;
    (void)d4est_norms_fcn_L2(NULL, &v1, 1, &l2_ctx, skip_odd);
    printf("returned\n");
    return 0;
  }
  if (d4est_hip_device_count() < 1) { fprintf(stderr, "no HIP device\n"); return 77; }
  run(3, 0);
  run(2, 1);
  run(4, 2);
  run(7, 3);
  d4est_hip_compat_release();
  printf(n_fail ? "MISMATCH (%d)\n" : "ok\n", n_fail);
  return n_fail ? 1 : 0;
}
