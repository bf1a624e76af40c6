/* Plain C99 host for the element size parameters: d4est_hip_plan_set_h_types -> brick geometry (volume and mortars, the mortar form
 * computing the size parameters itself) -> d4est_hip_plan_size_parameter -> d4est_hip_estimator_bi with a NULL diameter array, on a
 * 2 x 2 x 2 brick with extents (0,1) x (0,2) x (0,0.5).  Checks the arrays against the closed form, the estimator against the call with
 * the explicit array, and the residual term under VOL_H_EQ_CUBE_APPROX against a third of its VOL_H_EQ_DIAM value.  No Python, no C++.
 *
 * Build / run: tests/test_sizes_probe_gpu.py.  Prints one line per check; exit code 0 = all within tolerance.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "d4est_hip.h"

static int n_fail = 0;

static void check(const char* what, const double* got, const double* ref, int n, double tol) {
  double num = 0, den = 0;
  for (int i = 0; i < n; i++) {
    const double d = fabs(got[i] - ref[i]);
    if (!(d <= num)) num = d;      /* (NaN propagates) */
    if (fabs(ref[i]) > den) den = fabs(ref[i]);
  }
  const double rel = num / (den > 0 ? den : 1);
  if (!(rel <= tol)) n_fail++;
  printf("%-44s n=%4d  rel-inf %.2e %s\n", what, n, rel, (rel <= tol) ? "" : "FAIL");
}

static double lcg(unsigned long long* s) {
  *s = *s * 6364136223846793005ULL + 1442695040888963407ULL;
  return (double)(*s >> 11) / 9007199254740992.0;
}

/* term 0 of every element into term0[8] */
static void run(int volume_h_type, double* term0) {
  enum { ne = 8, p = 3, N = p + 1, n3 = N * N * N, n2 = N * N, ln = ne * n3 };
  const double extents[6] = {0, 1, 0, 2, 0, 0.5}, w[3] = {0.5, 1.0, 0.25};   /* element widths */
  int deg[ne], ns[ne], dq[ne];
  for (int e = 0; e < ne; e++) { deg[e] = p; ns[e] = e * n3; dq[e] = 1; }
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
  d4est_hip_plan_t* plan = d4est_hip_plan_create(ne, deg, deg, ns, ns, D4EST_HIP_QUAD_LEGENDRE);
  d4est_hip_plan_set_geometry_brick(plan, dq, 2.0, extents);
  d4est_hip_plan_set_estimator(plan, D4EST_HIP_EST_HOUSTON_GRADU_MAXP_MINH, D4EST_HIP_EST_HOUSTON_U_MAXP_MINH,
                               D4EST_HIP_EST_HOUSTON_U_DIRICHLET_MAXP_MINH, 10.0);
  d4est_hip_plan_set_faces(plan, side_nbr, side_nbr_face, side_reorder, side_mortar_stride, side_bndry_stride, total_mortar, total_bndry, 0, NULL, NULL);
  d4est_hip_plan_set_sipg(plan, 10.0, 0);
  const double* dev = NULL;
  long long count = -1;
  if (d4est_hip_plan_size_parameter(plan, D4EST_HIP_SIZE_DIAM_VOLUME, &dev, &count) != 0 || dev != NULL) {
    n_fail++;
    printf("size_parameter before any computation: FAIL\n");
  }
  d4est_hip_plan_set_h_types(plan, D4EST_HIP_FACE_H_EQ_VOLUME_DIV_AREA, volume_h_type);
  d4est_hip_plan_set_mortar_geometry_brick(plan, dq, 2.0, extents);   /* computes the size parameters it needs */
  double got[48], ref[48];
  const double diam = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]) * (volume_h_type == D4EST_HIP_VOL_H_EQ_CUBE_APPROX ? 1. / sqrt(3.) : 1.);
  for (int which = 0; which <= D4EST_HIP_SIZE_J_DIV_SJ_MAX; which++) {
    const int per = (which == D4EST_HIP_SIZE_DIAM_VOLUME || which == D4EST_HIP_SIZE_VOLUME) ? 1 : 6;
    if (!d4est_hip_plan_size_parameter(plan, which, &dev, &count) || count != per * ne) {
      n_fail++;
      printf("size_parameter %d: not computed / count %lld FAIL\n", which, count);
      continue;
    }
    d4est_hip_plan_synchronize(plan);
    d4est_hip_memcpy_d2h(got, dev, sizeof(double) * (size_t)count);
    for (int i = 0; i < per * ne; i++) {
      const int d = (i % 6) / 2, o0 = d == 0 ? 1 : 0, o1 = d == 2 ? 1 : 2;
      ref[i] = which == D4EST_HIP_SIZE_DIAM_VOLUME ? diam
             : which == D4EST_HIP_SIZE_VOLUME      ? w[0] * w[1] * w[2]
             : which == D4EST_HIP_SIZE_AREA        ? w[o0] * w[o1]
             : which == D4EST_HIP_SIZE_DIAM_FACE   ? sqrt(w[o0] * w[o0] + w[o1] * w[o1])
                                                   : 0.5 * w[d];
    }
    char what[64];
    snprintf(what, sizeof what, "size parameter %d (volume_h_type %d)", which, volume_h_type);
    check(what, got, ref, per * ne, (which == D4EST_HIP_SIZE_DIAM_VOLUME || which == D4EST_HIP_SIZE_DIAM_FACE) ? 1e-14 : 1e-12);
  }
  /* the estimator with the plan's diameters against the explicit array */
  unsigned long long seed = 11;
  double *u = malloc(sizeof(double) * ln), *r = malloc(sizeof(double) * ln);
  for (int i = 0; i < ln; i++) { u[i] = lcg(&seed) - 0.5; r[i] = lcg(&seed) - 0.5; }
  const size_t vb = sizeof(double) * ln;
  double *d_u = d4est_hip_malloc(vb), *d_r = d4est_hip_malloc(vb), *d_out = d4est_hip_malloc(sizeof(double) * 10 * ne);
  d4est_hip_memcpy_h2d(d_u, u, vb);
  d4est_hip_memcpy_h2d(d_r, r, vb);
  d4est_hip_plan_size_parameter(plan, D4EST_HIP_SIZE_DIAM_VOLUME, &dev, &count);
  d4est_hip_estimator_bi(plan, d_u, NULL, d_r, NULL, NULL, d_out, d_out + ne);
  d4est_hip_estimator_bi(plan, d_u, NULL, d_r, dev, NULL, d_out + 5 * ne, d_out + 6 * ne);
  d4est_hip_plan_synchronize(plan);
  double out[10 * ne];
  d4est_hip_memcpy_d2h(out, d_out, sizeof out);
  check("estimator_bi(NULL diam) vs explicit array", out, out + 5 * ne, 5 * ne, 0.0);
  for (int e = 0; e < ne; e++) term0[e] = out[ne + e];
  d4est_hip_free(d_u); d4est_hip_free(d_r); d4est_hip_free(d_out);
  d4est_hip_plan_destroy(plan);
  free(u); free(r);
}

int main(void) {
  if (d4est_hip_device_count() < 1) { fprintf(stderr, "no HIP device\n"); return 77; }
  double t_diam[8], t_cube[8], third[8];
  run(D4EST_HIP_VOL_H_EQ_DIAM, t_diam);
  run(D4EST_HIP_VOL_H_EQ_CUBE_APPROX, t_cube);
  int positive = 1;
  for (int e = 0; e < 8; e++) { third[e] = t_diam[e] / 3.0; positive = positive && t_diam[e] > 0; }
  if (!positive) { n_fail++; printf("residual term not positive FAIL\n"); }
  check("term 0: CUBE_APPROX vs DIAM / 3", t_cube, third, 8, 1e-15);
  printf(n_fail ? "MISMATCH (%d)\n" : "ok\n", n_fail);
  return n_fail ? 1 : 0;
}
