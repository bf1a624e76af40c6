/* Host-only check of the set-up code of the norm shims (no device, no library to link): the mirrored context structs of
 * include/d4est_hip_compat.h have the layout the reference's declarations give (src/dGMath/d4est_ip_energy_norm.h:9-19,
 * src/IO/d4est_norms.h:25-51), and the penalty probing of csrc/d4est_hip_compat_penalty.h names each of the four SIPG penalty functions,
 * written here as the reference writes them, and refuses anything else.  Plain C99 with its own main, so it can also be built with
 * -fsanitize=address,undefined.  Exit code 0 = all checks hold.
 */
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "d4est_hip_compat.h"
#include "d4est_hip_compat_penalty.h"

static int n_fail = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) { n_fail++; printf("FAIL %s\n", #cond); }        \
  } while (0)

/* the reference's declarations, restated with the types spelled out (pointers, int, double) */
struct ref_energy_norm_data { double (*f)(int, double, int, double, double); double c; void* size_params; void* user; double vol, bndry, iface; };
struct ref_l2_ctx { void *p4est, *ops, *geom, *quad, *factors; };
struct ref_energy_ctx { void *p4est, *ghost, *ghost_data, *ops, *geom, *quad, *factors; int which_field; void* energy_norm_data; double sq_local; double* estimator; };

static double f_maxp(int deg_m, double h_m, int deg_p, double h_p, double c) {
  double max_deg = (deg_m > deg_p) ? deg_m : deg_p;
  double min_h = (h_m < h_p) ? h_m : h_p;
  return (c * (max_deg) * (max_deg)) / min_h;
}
static double f_meanp(int deg_m, double h_m, int deg_p, double h_p, double c) {
  double mean_p = .5 * (deg_m + deg_p);
  double mean_p_sqr = mean_p * mean_p;
  double mean_h = .5 * (h_m + h_p);
  return (c * mean_p_sqr) / mean_h;
}
static double f_maxpp1(int deg_m, double h_m, int deg_p, double h_p, double c) {
  double max_deg = (deg_m > deg_p) ? deg_m : deg_p;
  double min_h = (h_m < h_p) ? h_m : h_p;
  return (c * (max_deg + 1) * (max_deg + 1)) / min_h;
}
static double f_mean_p_sqr_over_h(int deg_m, double h_m, int deg_p, double h_p, double c) {
  double mean_penalty = .5 * (deg_m * deg_m / h_m + deg_p * deg_p / h_p);
  return (c * mean_penalty);
}
static double f_squared(int deg_m, double h_m, int deg_p, double h_p, double c) {   /* an estimator-style prefactor: none of the four */
  const double v = f_maxp(deg_m, h_m, deg_p, h_p, c);
  return v * v;
}
static double f_no_prefactor(int deg_m, double h_m, int deg_p, double h_p, double c) { return f_maxp(deg_m, h_m, deg_p, h_p, 1.0) + 0 * c; }

int main(void) {
  EXPECT(sizeof(d4est_ip_energy_norm_data_t) == sizeof(struct ref_energy_norm_data));
  EXPECT(offsetof(d4est_ip_energy_norm_data_t, u_penalty_fcn) == offsetof(struct ref_energy_norm_data, f));
  EXPECT(offsetof(d4est_ip_energy_norm_data_t, penalty_prefactor) == offsetof(struct ref_energy_norm_data, c));
  EXPECT(offsetof(d4est_ip_energy_norm_data_t, size_params) == offsetof(struct ref_energy_norm_data, size_params));
  EXPECT(offsetof(d4est_ip_energy_norm_data_t, user) == offsetof(struct ref_energy_norm_data, user));
  EXPECT(offsetof(d4est_ip_energy_norm_data_t, ip_energy_norm_sqr_volume_term) == offsetof(struct ref_energy_norm_data, vol));
  EXPECT(offsetof(d4est_ip_energy_norm_data_t, ip_energy_norm_sqr_boundary_term) == offsetof(struct ref_energy_norm_data, bndry));
  EXPECT(offsetof(d4est_ip_energy_norm_data_t, ip_energy_norm_sqr_interface_term) == offsetof(struct ref_energy_norm_data, iface));
  EXPECT(sizeof(d4est_norms_fcn_L2_ctx_t) == sizeof(struct ref_l2_ctx));
  EXPECT(offsetof(d4est_norms_fcn_L2_ctx_t, d4est_factors) == offsetof(struct ref_l2_ctx, factors));
  EXPECT(sizeof(d4est_norms_fcn_energy_ctx_t) == sizeof(struct ref_energy_ctx));
  EXPECT(offsetof(d4est_norms_fcn_energy_ctx_t, ghost) == offsetof(struct ref_energy_ctx, ghost));
  EXPECT(offsetof(d4est_norms_fcn_energy_ctx_t, d4est_factors) == offsetof(struct ref_energy_ctx, factors));
  EXPECT(offsetof(d4est_norms_fcn_energy_ctx_t, which_field) == offsetof(struct ref_energy_ctx, which_field));
  EXPECT(offsetof(d4est_norms_fcn_energy_ctx_t, energy_norm_data) == offsetof(struct ref_energy_ctx, energy_norm_data));
  EXPECT(offsetof(d4est_norms_fcn_energy_ctx_t, energy_estimator_sq_local) == offsetof(struct ref_energy_ctx, sq_local));
  EXPECT(offsetof(d4est_norms_fcn_energy_ctx_t, energy_estimator) == offsetof(struct ref_energy_ctx, estimator));

  /* a context filled through the mirrored type reads back through the restated one */
  d4est_ip_energy_norm_data_t nd;
  memset(&nd, 0, sizeof nd);
  nd.u_penalty_fcn = f_meanp; nd.penalty_prefactor = 2.5; nd.ip_energy_norm_sqr_interface_term = 7.0;
  struct ref_energy_norm_data rd;
  memcpy(&rd, &nd, sizeof rd);
  EXPECT(rd.f == f_meanp && rd.c == 2.5 && rd.iface == 7.0 && rd.vol == 0.0);

  EXPECT(d4est_hip_compat_identify_sipg(f_maxp) == 0);
  EXPECT(d4est_hip_compat_identify_sipg(f_meanp) == 1);
  EXPECT(d4est_hip_compat_identify_sipg(f_maxpp1) == 2);
  EXPECT(d4est_hip_compat_identify_sipg(f_mean_p_sqr_over_h) == 3);
  EXPECT(d4est_hip_compat_identify_sipg(f_squared) == -1);
  EXPECT(d4est_hip_compat_identify_sipg(f_no_prefactor) == -1);
  EXPECT(d4est_hip_compat_identify_sipg(NULL) == -1);
  /* the closed forms at a point worked out by hand: deg 3 | 5, h 0.5 | 0.25, c = 2 */
  EXPECT(d4est_hip_compat_sipg_closed_form(0, 3, 0.5, 5, 0.25, 2.0) == 200.0);     /* 2 * 25 / 0.25 */
  EXPECT(d4est_hip_compat_sipg_closed_form(1, 3, 0.5, 5, 0.25, 2.0) == 32.0 / 0.375);   /* 2 * 16 / 0.375 */
  EXPECT(d4est_hip_compat_sipg_closed_form(2, 3, 0.5, 5, 0.25, 2.0) == 288.0);     /* 2 * 36 / 0.25 */
  EXPECT(d4est_hip_compat_sipg_closed_form(3, 3, 0.5, 5, 0.25, 2.0) == 118.0);     /* 2 * .5 * (18 + 100) */
  printf(n_fail ? "MISMATCH (%d)\n" : "ok\n", n_fail);
  return n_fail ? 1 : 0;
}
