/* Plain C99 host that calls every entry of the problem unit (include/d4est_hip.h: d4est_hip_field_eval, _plan_compute_xyz_brick,
 * _plan_set_puncture_term_* / _plan_set_cds_term_*, _plan_nonlinear_coefficients, _plan_compute_boundary_xyz_*, _plan_set_robin_by_id_*)
 * once on a 2 x 2 x 2 brick of degree 2 on [-4, 4]^3 and prints one checksum per result: the exclusive-or of (2 i + 1) * bits(v_i) over
 * the array, exact and the same from any language.  The _analytic entries see the same eight cells as the centre cube (tree 6) of the
 * 7-tree cubed sphere.  Build / run / compare with the same calls through ctypes: tests/test_problem_probe_gpu.py. */
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
  int deg[NE], ns[NE], tree7[NE], q[3 * NE], dq[NE];
  int side_nbr[6 * NE], side_nbr_face[6 * NE], side_reorder[6 * NE], mstride[6 * NE], bstride[6 * NE];
  const double extents[6] = {-4., 4., -4., 4., -4., 4.};
  const double sphere[3] = {3., 6., 0.};
  const double punct[22] = {2., 1e-15, -3., 0., 0., 0., -.2, 0., 0.05, 0., 0.1, .5, 3., 0., 0., 0., .2, 0., 0., -0.1, 0.02, .5};
  const double star[8] = {0.25, -0.5, 0.125, 3.0, 0.01, 1.7, 5.0, -0.3};
  static double ones[NQT];
  const double *a = NULL, *b = NULL;
  double *d_xyz, *d_out, *d_bxyz, *d_u, *d_Au;
  d4est_hip_plan_t* plan;
  int e, f, k = 0, nb = 0, id;

  if (d4est_hip_device_count() < 1) { printf("no device\n"); return 2; }
  for (e = 0; e < NE; ++e) {
    deg[e] = P; ns[e] = e * N3; tree7[e] = 6; dq[e] = 1;
    q[3 * e] = e & 1; q[3 * e + 1] = (e >> 1) & 1; q[3 * e + 2] = (e >> 2) & 1;
    for (f = 0; f < 6; ++f) {
      const int s = 6 * e + f, dir = f >> 1, inner = ((e >> dir) & 1) != (f & 1);
      side_nbr[s] = inner ? (e ^ (1 << dir)) : -1;
      side_nbr_face[s] = f ^ 1;
      side_reorder[s] = 0;
      mstride[s] = s * T;
      bstride[s] = nb;
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
  d_bxyz = (double*)d4est_hip_malloc(3 * TM * sizeof(double));
  d_u = (double*)d4est_hip_malloc(NQT * sizeof(double));
  d_Au = (double*)d4est_hip_malloc(NQT * sizeof(double));
  d4est_hip_memcpy_h2d(d_u, ones, NQT * sizeof(double));

  d4est_hip_plan_compute_xyz_brick(plan, q, dq, 2.0, extents, NULL, d_xyz);
  checksum("xyz_brick", d_xyz, 3 * NQT);
  for (id = D4EST_HIP_FIELD_PUNCTURE_K2; id <= D4EST_HIP_FIELD_INV_R; ++id) {
    char name[32];
    const int is_p = id <= D4EST_HIP_FIELD_PUNCTURE_B, is_s = !is_p && id != D4EST_HIP_FIELD_INV_R;
    d4est_hip_plan_synchronize(plan);
    d4est_hip_field_eval(NULL, id, is_p ? punct : is_s ? star : NULL, is_p ? 22 : is_s ? 8 : 0, d_xyz, NQT, d_out);
    sprintf(name, "field_%d", id);
    checksum(name, d_out, NQT);
  }
#define TERM(label, call)                                                        \
  call;                                                                          \
  if (!d4est_hip_plan_nonlinear_coefficients(plan, &a, &b, &k)) return 3;        \
  checksum(label "_a", a, NQT);                                                  \
  if (b) checksum(label "_b", b, NQT);                                           \
  printf(label "_k %016llx\n", (unsigned long long)(long long)k);
  TERM("puncture_brick", d4est_hip_plan_set_puncture_term_brick(plan, punct, 22, q, dq, 2.0, extents))
  TERM("puncture_analytic", d4est_hip_plan_set_puncture_term_analytic(plan, punct, 22, D4EST_HIP_GEOM_CUBED_SPHERE_7TREE, sphere, tree7, q, dq, 2.0))
  TERM("puncture_xyz", d4est_hip_plan_set_puncture_term_xyz(plan, punct, 22, d_xyz))
  TERM("cds_brick", d4est_hip_plan_set_cds_term_brick(plan, star, 8, q, dq, 2.0, extents))
  TERM("cds_analytic", d4est_hip_plan_set_cds_term_analytic(plan, star, 8, D4EST_HIP_GEOM_CUBED_SPHERE_7TREE, sphere, tree7, q, dq, 2.0))
  TERM("cds_xyz", d4est_hip_plan_set_cds_term_xyz(plan, star, 8, d_xyz))

  d4est_hip_memset(d_bxyz, 0, 3 * TM * sizeof(double));
  d4est_hip_plan_compute_boundary_xyz_brick(plan, q, dq, 2.0, extents, d_bxyz);
  checksum("boundary_brick", d_bxyz, 3 * TM);
  d4est_hip_memset(d_bxyz, 0, 3 * TM * sizeof(double));
  d4est_hip_plan_compute_boundary_xyz_analytic(plan, D4EST_HIP_GEOM_CUBED_SPHERE_7TREE, sphere, tree7, q, dq, 2.0, d_bxyz);
  checksum("boundary_analytic", d_bxyz, 3 * TM);

  d4est_hip_plan_set_robin_by_id_brick(plan, D4EST_HIP_ROBIN_COEFF_BRICK, D4EST_HIP_ROBIN_RHS_INV_R, q, dq, 2.0, extents);
  d4est_hip_apply_aij(plan, d_u, NULL, d_Au);
  checksum("robin_brick", d_Au, NQT);
  d4est_hip_plan_set_robin_by_id_analytic(plan, D4EST_HIP_ROBIN_COEFF_INV_R, D4EST_HIP_ROBIN_RHS_ZERO, D4EST_HIP_GEOM_CUBED_SPHERE_7TREE, sphere,
                                          tree7, q, dq, 2.0);
  d4est_hip_apply_aij(plan, d_u, NULL, d_Au);
  checksum("robin_analytic", d_Au, NQT);
  d4est_hip_plan_set_robin_values(plan, NULL, NULL, 0);

  d4est_hip_free(d_xyz); d4est_hip_free(d_out); d4est_hip_free(d_bxyz); d4est_hip_free(d_u); d4est_hip_free(d_Au);
  d4est_hip_plan_destroy(plan);
  printf("ok\n");
  return 0;
}
