/* Plain C99 host that evaluates the Laplacian of a field at the quadrature nodes through the C-ABI (include/d4est_hip.h:
 * d4est_hip_plan_set_hessian_brick, d4est_hip_plan_hessian_info / _supported, d4est_hip_hessian_trace) and through the REFERENCE's OWN
 * PROTOTYPE (include/d4est_hip_compat.h: d4est_hessian_compute_hessian_trace_of_field_on_quadrature_points) on the bound plan.  Mesh: the unit cube as 8 elements of degree 3 with
 * deg_quad = 4; u = x^2 + 2 y^2 + 3 z^2 + x y z, whose Laplacian is 12 at every node.
 * Build / run: tests/test_hessian_probe_gpu.py.  Prints one line per check; exit code 0 = all within tolerance. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "d4est_hip.h"
#include "d4est_hip_compat.h"

#define NE 8
#define P 3
#define PQ 4
#define N (P + 1)
#define NQ (PQ + 1)
#define N3 (N * N * N)
#define NQ3 (NQ * NQ * NQ)

static int fails = 0;
static void check(const char* what, double err, double tol) {
  printf("%-72s %.3e (tol %.1e) %s\n", what, err, tol, err <= tol ? "pass" : "FAIL");
  if (!(err <= tol)) ++fails;
}

int main(void) {
  int deg[NE], degq[NE], ns[NE], qs[NE], dq[NE];
  double xl[N];
  const double extents[6] = {0., 1., 0., 1., 0., 1.};
  static double u[NE * N3], lap_abi[NE * NQ3], lap_shim[NE * NQ3];
  double *d_u, *d_lap, err;
  d4est_hip_plan_t* plan;
  int p4est_stand_in = 0;
  p4est_t* p4est = (p4est_t*)&p4est_stand_in;   /* the shims only use the pointer as a key */
  int e, i, j, k;

  if (d4est_hip_device_count() < 1) { printf("no device\n"); return 2; }
  if (d4est_hip_table(D4EST_HIP_TABLE_LOBATTO_NODES, P, 0, xl) != N) { printf("table size\n"); return 2; }
  for (e = 0; e < NE; ++e) {
    /* Morton order, x the fastest bit */
    const double x0 = 0.5 * (e & 1), y0 = 0.5 * ((e >> 1) & 1), z0 = 0.5 * ((e >> 2) & 1);
    deg[e] = P; degq[e] = PQ; ns[e] = e * N3; qs[e] = e * NQ3; dq[e] = 1;
    for (k = 0; k < N; ++k)
      for (j = 0; j < N; ++j)
        for (i = 0; i < N; ++i) {
          const double x = x0 + 0.25 * (xl[i] + 1.), y = y0 + 0.25 * (xl[j] + 1.), z = z0 + 0.25 * (xl[k] + 1.);
          u[e * N3 + i + N * (j + N * k)] = x * x + 2. * y * y + 3. * z * z + x * y * z;
        }
  }
  plan = d4est_hip_plan_create(NE, deg, degq, ns, qs, D4EST_HIP_QUAD_LEGENDRE);
  check("hessian_info before the set-up is 0", (double)d4est_hip_plan_hessian_info(plan), 0.);
  check("hessian_supported is 1", fabs((double)d4est_hip_plan_hessian_supported(plan) - 1.), 0.);
  d4est_hip_plan_set_hessian_brick(plan, dq, 2.0, extents);
  check("hessian_info after set_hessian_brick is 1", fabs((double)d4est_hip_plan_hessian_info(plan) - 1.), 0.);

  d_u = (double*)d4est_hip_malloc(sizeof(u));
  d_lap = (double*)d4est_hip_malloc(sizeof(lap_abi));
  d4est_hip_memcpy_h2d(d_u, u, sizeof(u));
  d4est_hip_memset(d_lap, 0xff, sizeof(lap_abi));
  d4est_hip_hessian_trace(plan, d_u, d_lap);
  d4est_hip_device_synchronize();
  d4est_hip_memcpy_d2h(lap_abi, d_lap, sizeof(lap_abi));
  err = 0.;
  for (i = 0; i < NE * NQ3; ++i) err = fmax(err, fabs(lap_abi[i] - 12.));
  /* 1e-11 |u|_inf / h^2 with |u|_inf = 7 and h = 1/2 (the CPU pin's tolerance, tests/test_hessian_dense.py) */
  check("d4est_hip_hessian_trace: |Lap u - 12|_inf", err, 1e-11 * 7. * 4.);

  d4est_hip_compat_bind_mesh(p4est, plan);
  for (i = 0; i < NE * NQ3; ++i) lap_shim[i] = -1.;
  d4est_hessian_compute_hessian_trace_of_field_on_quadrature_points(p4est, NULL, NULL, NULL, NULL, HESSIAN_ANALYTICAL, u, lap_shim);
  check("the reference-named shim gives the same bits", memcmp(lap_abi, lap_shim, sizeof(lap_abi)) ? 1. : 0., 0.);
  d4est_hip_compat_bind_mesh(p4est, NULL);

  d4est_hip_free(d_u);
  d4est_hip_free(d_lap);
  d4est_hip_plan_destroy(plan);
  d4est_hip_compat_release();
  printf(fails ? "FAILED\n" : "ok\n");
  return fails ? 1 : 0;
}
