// The four SIPG penalty functions (penalty_calc_t) by the ids of d4est_hip_plan_set_sipg: shared by the operator's face factors
// (d4est_hip_faces_geometry.hip) and the IP energy norm (d4est_hip_norms.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace d4est_hip {

__device__ inline double sipg_penalty(int fcn, int deg_m, double h_m, int deg_p, double h_p, double prefactor) {
  // src/dGMath/d4est_laplacian_flux_sipg.c:945-1005
  if (fcn == 0) {
    const double max_deg = (deg_m > deg_p) ? deg_m : deg_p, min_h = (h_m < h_p) ? h_m : h_p;
    return (prefactor * max_deg * max_deg) / min_h;
  } else if (fcn == 1) {
    const double mean_p = .5 * (deg_m + deg_p), mean_h = .5 * (h_m + h_p);
    return (prefactor * mean_p * mean_p) / mean_h;
  } else if (fcn == 2) {
    const double max_deg = (deg_m > deg_p) ? deg_m : deg_p, min_h = (h_m < h_p) ? h_m : h_p;
    return (prefactor * (max_deg + 1) * (max_deg + 1)) / min_h;
  }
  return prefactor * .5 * (deg_m * deg_m / h_m + deg_p * deg_p / h_p);
}

}  // namespace d4est_hip
