/*
 * d4est_hip_compat_penalty.h -- which of the four SIPG penalty functions a caller's penalty_calc_t is.
 *
 * The reference's four (src/dGMath/d4est_laplacian_flux_sipg.c:945-1005) are static, so their addresses identify nothing: the
 * function is EVALUATED at fixed probe arguments, with a probe prefactor of our own, and matched against the four closed forms by the
 * ids of d4est_hip_plan_set_sipg.  Plain C99 and C++, host only, no other header of the project: the compat library includes it, and
 * so does the stand-alone host check tests/c/norms_compat_host.c.
 */
#ifndef D4EST_HIP_COMPAT_PENALTY_H
#define D4EST_HIP_COMPAT_PENALTY_H

#include <math.h>

/* ids of d4est_hip_plan_set_sipg: 0 maxp_sqr_over_minh, 1 meanp_sqr_over_meanh, 2 maxpp1_sqr_over_minh, 3 mean_p_sqr_over_h */
static inline double d4est_hip_compat_sipg_closed_form(int id, int deg_m, double h_m, int deg_p, double h_p, double c) {
  const double max_deg = (deg_m > deg_p) ? deg_m : deg_p, min_h = (h_m < h_p) ? h_m : h_p;
  switch (id) {
    case 0: return (c * max_deg * max_deg) / min_h;
    case 1: {
      const double mean_p = .5 * (deg_m + deg_p), mean_h = .5 * (h_m + h_p);
      return (c * (mean_p * mean_p)) / mean_h;
    }
    case 2: return (c * (max_deg + 1) * (max_deg + 1)) / min_h;
    default: return c * (.5 * (deg_m * deg_m / h_m + deg_p * deg_p / h_p));
  }
}

/* the id in 0..3 whose closed form agrees with fcn at every probe point, or -1 (NULL included): nothing is substituted silently.
 * The probe points have deg_m != deg_p and h_m != h_p in both orders, where the four forms all differ. */
static inline int d4est_hip_compat_identify_sipg(double (*fcn)(int, double, int, double, double)) {
  static const int dm[4] = {3, 7, 2, 9}, dp[4] = {5, 4, 2, 6};
  static const double hm[4] = {0.25, 0.031, 0.7, 0.12}, hp[4] = {0.4, 0.05, 0.7, 0.09}, c = 1.7;
  if (!fcn) return -1;
  for (int id = 0; id < 4; ++id) {
    int ok = 1;
    for (int k = 0; k < 4 && ok; ++k) {
      const double want = d4est_hip_compat_sipg_closed_form(id, dm[k], hm[k], dp[k], hp[k], c), got = fcn(dm[k], hm[k], dp[k], hp[k], c);
      ok = fabs(got - want) <= 1e-13 * fabs(want);
    }
    if (ok) return id;
  }
  return -1;
}

#endif /* D4EST_HIP_COMPAT_PENALTY_H */
