/* Plain C99 host for the problem data of the remaining families (include/d4est_hip.h: the field ids OKENDON_U ... STAMM_RHS of
 * d4est_hip_field_eval, d4est_hip_plan_set_okendon_term_brick with _plan_nonlinear_exponent, _plan_set_boyen_york_term_xyz,
 * d4est_hip_plan_build_load_by_id_brick / _xyz, ROBIN_COEFF_LORENTZIAN) on a 2 x 2 x 2 brick of degree 2 on [1, 2]^3.  Prints one
 * checksum per result, the exclusive-or of (2 i + 1) * bits(v_i) as tests/c/problem_probe.c.  Build / run / compare with the same
 * calls through ctypes: tests/test_problem_more_probe_gpu.py. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "d4est_hip.h"

#define NE 8
#define P 2
#define N (P + 1)
#define N3 (N * N * N)
#define T (N * N)
#define NQT (NE * N3)
#define TM (6 * NE * T)

static void checksum(const char* name, const double* d_v, size_t n) {
  double* h = (double*)malloc(n * sizeof(double));
  unsigned long long acc = 0ull, bits;
  size_t i;
  d4est_hip_device_synchronize();
  d4est_hip_memcpy_d2h(h, d_v, n * sizeof(double));
  for (i = 0; i < n; ++i) {
    memcpy(&bits, &h[i], sizeof(bits));
    acc ^= bits * (2ull * (unsigned long long)i + 1ull);
  }
  printf("%s %016llx\n", name, acc);
  free(h);
}

int main(void) {
  int deg[NE], ns[NE], q[3 * NE], dq[NE];
  int side_nbr[6 * NE], side_nbr_face[6 * NE], side_reorder[6 * NE], mstride[6 * NE], bstride[6 * NE];
  const double extents[6] = {1., 2., 1., 2., 1., 2.};
  const double okendon[1] = {0.5}, by[2] = {0.7, 1.3}, stamm[3] = {0.25, 0.3, 0.35};
  static double ones[NQT];
  const double *a = NULL, *b = NULL;
  double *d_xyz, *d_out, *d_u, *d_Au, s = 0.;
  d4est_hip_plan_t* plan;
  int e, f, k = 99, nb = 0, id;

  if (d4est_hip_device_count() < 1) { printf("no device\n"); return 2; }
  for (e = 0; e < NE; ++e) {
    deg[e] = P; ns[e] = e * N3; dq[e] = 1;
    q[3 * e] = e & 1; q[3 * e + 1] = (e >> 1) & 1; q[3 * e + 2] = (e >> 2) & 1;
    for (f = 0; f < 6; ++f) {
      const int sd = 6 * e + f, dir = f >> 1, inner = ((e >> dir) & 1) != (f & 1);
      side_nbr[sd] = inner ? (e ^ (1 << dir)) : -1;
      side_nbr_face[sd] = f ^ 1;
      side_reorder[sd] = 0;
      mstride[sd] = sd * T;
      bstride[sd] = nb;
      if (!inner) nb += T;
    }
  }
  for (e = 0; e < NQT; ++e) ones[e] = 1.0 + 0.001 * (e % 17);
  plan = d4est_hip_plan_create(NE, deg, deg, ns, ns, D4EST_HIP_QUAD_LEGENDRE);
  d4est_hip_plan_set_geometry_brick(plan, dq, 2.0, extents);
  d4est_hip_plan_set_faces(plan, side_nbr, side_nbr_face, side_reorder, mstride, bstride, TM, nb, 0, NULL, NULL);
  d4est_hip_plan_set_sipg(plan, 10.0, 0);
  d4est_hip_plan_set_mortar_geometry_brick(plan, dq, 2.0, extents);

  d_xyz = (double*)d4est_hip_malloc(3 * NQT * sizeof(double));
  d_out = (double*)d4est_hip_malloc(NQT * sizeof(double));
  d_u = (double*)d4est_hip_malloc(NQT * sizeof(double));
  d_Au = (double*)d4est_hip_malloc(NQT * sizeof(double));
  d4est_hip_memcpy_h2d(d_u, ones, NQT * sizeof(double));

  d4est_hip_plan_compute_xyz_brick(plan, q, dq, 2.0, extents, NULL, d_xyz);
  d4est_hip_plan_synchronize(plan);
  for (id = D4EST_HIP_FIELD_OKENDON_U; id <= D4EST_HIP_FIELD_STAMM_RHS; ++id) {
    char name[32];
    const double* pr = id == D4EST_HIP_FIELD_OKENDON_U ? okendon : id <= D4EST_HIP_FIELD_BY_A ? by : id >= D4EST_HIP_FIELD_STAMM_U ? stamm : NULL;
    const int np = id == D4EST_HIP_FIELD_OKENDON_U ? 1 : id <= D4EST_HIP_FIELD_BY_A ? 2 : id >= D4EST_HIP_FIELD_STAMM_U ? 3 : 0;
    d4est_hip_field_eval(NULL, id, pr, np, d_xyz, NQT, d_out);
    sprintf(name, "field_%d", id);
    checksum(name, d_out, NQT);
  }

  d4est_hip_plan_set_okendon_term_brick(plan, okendon, 1, q, dq, 2.0, extents);
  if (!d4est_hip_plan_nonlinear_coefficients(plan, &a, &b, &k) || b || k != 0) return 3;
  if (!d4est_hip_plan_nonlinear_exponent(plan, &s) || s != 0.5) return 4;
  checksum("okendon_a", a, NQT);
  d4est_hip_apply_nonlinear_term(plan, d_u, 0, d_Au);
  checksum("okendon_term", d_Au, NQT);
  d4est_hip_plan_set_nonlinear_abs_power(plan, d_u, NULL, 0.3);
  d4est_hip_apply_nonlinear_term(plan, d_u, 0, d_Au);
  checksum("abs_power_term", d_Au, NQT);

  d4est_hip_plan_set_boyen_york_term_xyz(plan, by, 2, d_xyz);
  if (!d4est_hip_plan_nonlinear_coefficients(plan, &a, &b, &k) || b || k != -7) return 5;
  if (d4est_hip_plan_nonlinear_exponent(plan, &s)) return 6;
  checksum("boyen_york_a", a, NQT);

  d4est_hip_plan_build_load_by_id_brick(plan, D4EST_HIP_FIELD_STAMM_RHS, stamm, 3, q, dq, 2.0, extents, 0, d_Au);
  checksum("load_brick", d_Au, NQT);
  d4est_hip_plan_build_load_by_id_xyz(plan, D4EST_HIP_FIELD_LORENTZIAN_RHS, NULL, 0, d_xyz, 1, d_Au);
  checksum("load_xyz_accumulated", d_Au, NQT);

  d4est_hip_plan_set_robin_by_id_brick(plan, D4EST_HIP_ROBIN_COEFF_LORENTZIAN, D4EST_HIP_ROBIN_RHS_ZERO, q, dq, 2.0, extents);
  d4est_hip_apply_aij(plan, d_u, NULL, d_Au);
  checksum("robin_lorentzian", d_Au, NQT);
  d4est_hip_plan_set_robin_values(plan, NULL, NULL, 0);

  d4est_hip_free(d_xyz); d4est_hip_free(d_out); d4est_hip_free(d_u); d4est_hip_free(d_Au);
  d4est_hip_plan_destroy(plan);
  printf("ok\n");
  return 0;
}
