/* Plain C99 host that reads a field at tree coordinates through the C-ABI (include/d4est_hip.h: d4est_hip_probe_create / _info /
 * _element_info / _eval / _set_map / _xyz) and through the REFERENCE's OWN PROTOTYPE (include/d4est_hip_compat.h:
 * d4est_mesh_interpolate_at_tree_coord) on the bound plan with the forest registered by d4est_hip_compat_bind_forest.  Mesh: the brick
 * [0, 2] x [0, 1] x [-1, 3] as 8 elements of degree 3; u = x^2 + 2 y^3 - z + x y z, which degree 3 holds exactly.  Three points: inside an
 * element, on the corner shared by all eight (the first element takes it), and outside the tree (err = 1).
 * Build / run: tests/test_probe_compat_gpu.py.  Prints one line per check; exit code 0 = all within tolerance. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "d4est_hip.h"
#include "d4est_hip_compat.h"

#define NE 8
#define P 3
#define N (P + 1)
#define N3 (N * N * N)
#define NP 3

static int fails = 0;
static void check(const char* what, double err, double tol) {
  printf("%-72s %.3e (tol %.1e) %s\n", what, err, tol, err <= tol ? "pass" : "FAIL");
  if (!(err <= tol)) ++fails;
}

static double field(double x, double y, double z) { return x * x + 2. * y * y * y - z + x * y * z; }

int main(void) {
  int deg[NE], ns[NE], tree_e[NE], q[3 * NE], dq[NE];
  double xl[N];
  const double extents[6] = {0., 2., 0., 1., -1., 3.};
  static double u[NE * N3];
  int tree_p[NP] = {0, 0, 0};
  double abc[3 * NP] = {0.3, 0.6, 0.2, 0.5, 0.5, 0.5, 1.5, 0.5, 0.5};
  int err[NP], elem[NP], nstr[NP], degp[NP];
  double rst[3 * NP], xyz[3 * NP], val[NP];
  double *d_u, *d_out;
  d4est_hip_plan_t* plan;
  d4est_hip_probe_t* probe;
  int p4est_stand_in = 0;
  p4est_t* p4est = (p4est_t*)&p4est_stand_in;   /* the shims only use the pointer as a key */
  int e, i, j, k, p, d;

  if (d4est_hip_device_count() < 1) { printf("no device\n"); return 2; }
  if (d4est_hip_table(D4EST_HIP_TABLE_LOBATTO_NODES, P, 0, xl) != N) { printf("table size\n"); return 2; }
  for (e = 0; e < NE; ++e) {
    /* Morton order, x the fastest bit */
    deg[e] = P; ns[e] = e * N3; tree_e[e] = 0; dq[e] = 1;
    q[3 * e] = e & 1; q[3 * e + 1] = (e >> 1) & 1; q[3 * e + 2] = (e >> 2) & 1;
    for (k = 0; k < N; ++k)
      for (j = 0; j < N; ++j)
        for (i = 0; i < N; ++i) {
          const double a = 0.5 * q[3 * e] + 0.25 * (xl[i] + 1.), b = 0.5 * q[3 * e + 1] + 0.25 * (xl[j] + 1.),
                       c = 0.5 * q[3 * e + 2] + 0.25 * (xl[k] + 1.);
          u[e * N3 + i + N * (j + N * k)] = field(2. * a, b, -1. + 4. * c);
        }
  }
  plan = d4est_hip_plan_create(NE, deg, deg, ns, ns, D4EST_HIP_QUAD_LEGENDRE);
  probe = d4est_hip_probe_create(plan, NP, tree_p, abc, tree_e, q, dq, 2.0, 0);
  check("probe_n_points", fabs((double)d4est_hip_probe_n_points(probe) - NP), 0.);
  d4est_hip_probe_info(probe, err, elem, rst);
  d4est_hip_probe_element_info(probe, nstr, degp);
  check("err = 0, 0, 1", (double)(abs(err[0]) + abs(err[1]) + abs(err[2] - 1)), 0.);
  check("elements 2, 0, -1 (the corner goes to the first element)", (double)(abs(elem[0] - 2) + abs(elem[1]) + abs(elem[2] + 1)), 0.);
  check("nodal_stride and deg of the located elements", (double)(abs(nstr[0] - 2 * N3) + abs(nstr[1]) + abs(degp[0] - P) + abs(degp[1] - P)), 0.);
  check("rst of the corner point is (1, 1, 1)", fabs(rst[3] - 1.) + fabs(rst[4] - 1.) + fabs(rst[5] - 1.), 0.);
  check("rst of the point outside is NaN", (rst[6] != rst[6] && rst[7] != rst[7] && rst[8] != rst[8]) ? 0. : 1., 0.);

  d_u = (double*)d4est_hip_malloc(sizeof(u));
  d_out = (double*)d4est_hip_malloc(sizeof(val));
  d4est_hip_memcpy_h2d(d_u, u, sizeof(u));
  d4est_hip_memset(d_out, 0, sizeof(val));
  d4est_hip_probe_eval(probe, 1, d_u, 0, d_out);
  d4est_hip_device_synchronize();
  d4est_hip_memcpy_d2h(val, d_out, sizeof(val));
  d4est_hip_probe_set_map(probe, D4EST_HIP_GEOM_BRICK, extents);
  d4est_hip_probe_xyz(probe, xyz);
  for (p = 0; p < 2; ++p) {
    /* (N^3 + 6 N) eps S with S <= Lebesgue^3 |u|_inf < 2^3 * 13: 88 * 2.3e-16 * 104 */
    check("d4est_hip_probe_eval against the polynomial", fabs(val[p] - field(2. * abc[3 * p], abc[3 * p + 1], -1. + 4. * abc[3 * p + 2])), 2.1e-12);
    check("d4est_hip_probe_xyz against the brick map",
          fabs(xyz[3 * p] - 2. * abc[3 * p]) + fabs(xyz[3 * p + 1] - abc[3 * p + 1]) + fabs(xyz[3 * p + 2] - (-1. + 4. * abc[3 * p + 2])), 1e-15);
  }
  check("value and xyz of the point outside are NaN", (val[2] != val[2] && xyz[6] != xyz[6]) ? 0. : 1., 0.);

  d4est_hip_compat_bind_mesh(p4est, plan);
  d4est_hip_compat_bind_forest(p4est, tree_e, q, dq, 2.0, D4EST_HIP_GEOM_BRICK, extents);
  for (p = 0; p < NP; ++p) {
    const d4est_mesh_interpolate_data_t data = d4est_mesh_interpolate_at_tree_coord(p4est, NULL, NULL, &abc[3 * p], tree_p[p], u, 0);
    double diff = (double)abs(data.err - err[p]);
    if (err[p] == 0) {
      diff += memcmp(&data.f_at_xyz, &val[p], sizeof(double)) ? 1. : 0.;
      diff += memcmp(data.rst, &rst[3 * p], 3 * sizeof(double)) ? 1. : 0.;
      diff += memcmp(data.xyz, &xyz[3 * p], 3 * sizeof(double)) ? 1. : 0.;
      diff += memcmp(data.abc, &abc[3 * p], 3 * sizeof(double)) ? 1. : 0.;
      for (d = 0; d < 3; ++d) diff += (double)abs(data.q[d] - q[3 * elem[p] + d]);
      diff += (double)(abs(data.dq - dq[elem[p]]) + abs(data.id - elem[p]) + abs(data.nodal_stride - nstr[p]));
    } else {
      diff += (data.f_at_xyz != data.f_at_xyz) ? 0. : 1.;
    }
    check("the reference-named shim fills the struct with the C-ABI results", diff, 0.);
  }
  d4est_hip_compat_bind_mesh(p4est, NULL);

  d4est_hip_free(d_u);
  d4est_hip_free(d_out);
  d4est_hip_probe_destroy(probe);
  d4est_hip_plan_destroy(plan);
  d4est_hip_compat_release();
  printf(fails ? "FAILED\n" : "ok\n");
  return fails ? 1 : 0;
}
