// The two Krylov preconditioners that are not the multigrid: d4est_krylov_pc_cheby_apply (src/Solver/d4est_krylov_pc_cheby.c:92-171) and
// d4est_krylov_pc_schwarz_apply (src/Solver/d4est_krylov_pc_schwarz.c:59-116), each as a d4est_hip_pc_fn whose ctx is the object.  They
// tie together pieces that exist -- cg_eigs and cheby_iterate of d4est_hip_solver.hip, the Schwarz handle's loop of
// d4est_hip_schwarz.hip -- on the plan's stream.  The reference allocates Au, r, the zero vector and the residual inside every apply
// (pc_cheby :105, :120, :148; pc_schwarz :70-71); here they are allocated once, at create.
#include <algorithm>

#include "d4est_hip_internal.h"

struct d4est_hip_pc_cheby {
  d4est_hip_plan* plan = nullptr;
  // the [d4est_krylov_pc_cheby] keys (pc_cheby :21-61)
  int cheby_imax = 0, eigs_cg_imax = 0, reuse_eig = 0, use_new = 0, use_zero_guess = 0;
  double ratio = 1.0, multiplier = 1.0;
  double eig = -1.0;        // kpccheby->eig, -1 = none yet (:196)
  int eig_runs = 0;         // cg_eigs calls so far (a report; the reference keeps no count)
  double *Au = nullptr, *r = nullptr, *zero = nullptr;
};

struct d4est_hip_pc_schwarz {
  d4est_hip_schwarz* schwarz = nullptr;
  d4est_hip_plan* plan = nullptr;
  int iterations = 0, subdomain_iter = 0;      // [schwarz_pc] schwarz_pc_iterations (pc_schwarz :21-24); the handle's CG options
  double subdomain_atol = 0.0, subdomain_rtol = 0.0;
  double *Au = nullptr, *residual = nullptr;
};

extern "C" {

d4est_hip_pc_cheby_t* d4est_hip_pc_cheby_create(d4est_hip_plan_t* plan, int cheby_imax, int cheby_eigs_cg_imax, double cheby_eigs_lmax_lmin_ratio,
                                                double cheby_eigs_max_multiplier, int cheby_reuse_eig, int cheby_use_new_cg_eigs,
                                                int cheby_use_zero_guess_for_eigs) {
  if (!plan || !plan->has_faces) D4EST_HIP_ABORT("pc_cheby_create: the plan needs its faces (plan_set_faces)");
  if (cheby_imax < 0 || cheby_eigs_cg_imax < 1 || !(cheby_eigs_lmax_lmin_ratio > 0.0))
    D4EST_HIP_ABORT("pc_cheby_create: cheby_imax = %d, cheby_eigs_cg_imax = %d, ratio = %g", cheby_imax, cheby_eigs_cg_imax, cheby_eigs_lmax_lmin_ratio);
  d4est_hip_pc_cheby* pc = new d4est_hip_pc_cheby();
  pc->plan = plan;
  pc->cheby_imax = cheby_imax;
  pc->eigs_cg_imax = cheby_eigs_cg_imax;
  pc->ratio = cheby_eigs_lmax_lmin_ratio;
  pc->multiplier = cheby_eigs_max_multiplier;
  pc->reuse_eig = cheby_reuse_eig;
  pc->use_new = cheby_use_new_cg_eigs;
  pc->use_zero_guess = cheby_use_zero_guess_for_eigs;
  const size_t bytes = std::max<size_t>((size_t)plan->local_nodes, 1) * sizeof(double);
  HIP_CHECK(hipMalloc(&pc->Au, bytes));
  HIP_CHECK(hipMalloc(&pc->r, bytes));
  if (pc->use_zero_guess) HIP_CHECK(hipMalloc(&pc->zero, bytes));
  return pc;
}

void d4est_hip_pc_cheby_destroy(d4est_hip_pc_cheby_t* pc) {
  if (!pc) return;
  (void)hipFree(pc->Au); (void)hipFree(pc->r); (void)hipFree(pc->zero);
  delete pc;
}

void d4est_hip_pc_cheby_apply(void* ctx, const double* r_dev, double* z_dev) {
  d4est_hip_pc_cheby* pc = static_cast<d4est_hip_pc_cheby*>(ctx);
  if (!pc || !r_dev || !z_dev) D4EST_HIP_ABORT("pc_cheby_apply: NULL argument");
  d4est_hip_plan* plan = pc->plan;
  const size_t bytes = std::max<size_t>((size_t)plan->local_nodes, 1) * sizeof(double);
  HIP_CHECK(hipMemsetAsync(z_dev, 0, bytes, plan->stream));                        // :104
  // :107-112: u = yp, rhs = xp, an Au of the preconditioner's own
  if (!pc->reuse_eig || pc->eig == -1) {                                           // :114-115
    double* start = z_dev;                       // cg_eigs advances the iterate it is given: z leaves it as the Chebyshev start
    if (pc->use_zero_guess) {                                                      // :119-122
      start = pc->zero;
      HIP_CHECK(hipMemsetAsync(start, 0, bytes, plan->stream));
    }
    pc->eig = d4est_hip::cg_eigs(plan, start, r_dev, pc->Au, pc->eigs_cg_imax, pc->use_new, nullptr);   // :123-138
    pc->eig_runs++;
    // :140-143: u = yp again
    pc->eig *= pc->multiplier;                                                     // :145
  }
  // :149-167: iterate_aux(r, cheby_imax, eig / ratio, eig, print, mg_level = -1, compute_residual_at_end = 0)
  d4est_hip::cheby_iterate(plan, z_dev, r_dev, pc->Au, pc->r, pc->cheby_imax, pc->eig / pc->ratio, pc->eig, 0);
}

double d4est_hip_pc_cheby_eig(const d4est_hip_pc_cheby_t* pc, int* cg_eigs_runs) {
  if (!pc) D4EST_HIP_ABORT("pc_cheby_eig: NULL object");
  if (cg_eigs_runs) *cg_eigs_runs = pc->eig_runs;
  return pc->eig;
}

void d4est_hip_pc_cheby_reset_eig(d4est_hip_pc_cheby_t* pc) {
  if (!pc) D4EST_HIP_ABORT("pc_cheby_reset_eig: NULL object");
  pc->eig = -1.0;   // the value d4est_krylov_pc_cheby_create leaves (:196): the next apply computes a bound whatever cheby_reuse_eig says
}

d4est_hip_pc_schwarz_t* d4est_hip_pc_schwarz_create(d4est_hip_schwarz_t* schwarz, d4est_hip_plan_t* mesh_plan, int schwarz_pc_iterations,
                                                    int subdomain_iter, double subdomain_atol, double subdomain_rtol) {
  const int code = d4est_hip::schwarz_smoother_check(schwarz, mesh_plan);
  if (code != 0)
    D4EST_HIP_ABORT("pc_schwarz_create: code %d (1 NULL argument, 2 the handle's mesh node count is not the plan's, 3 the subdomain plan is "
                    "not on the plan's stream, 4 the plan has ghost sides or no faces)", code);
  // d4est_solver_schwarz_subdomain_solver_cg.c:86-92; schwarz_pc_iterations is a required key (pc_schwarz :142)
  if (schwarz_pc_iterations < 0 || subdomain_iter <= 0 || !(subdomain_atol > 0) || !(subdomain_rtol > 0))
    D4EST_HIP_ABORT("pc_schwarz_create: some options are <= 0");
  d4est_hip_pc_schwarz* pc = new d4est_hip_pc_schwarz();
  pc->schwarz = schwarz;                                                           // :145
  pc->plan = mesh_plan;
  pc->iterations = schwarz_pc_iterations;
  pc->subdomain_iter = subdomain_iter;
  pc->subdomain_atol = subdomain_atol;
  pc->subdomain_rtol = subdomain_rtol;
  const size_t bytes = std::max<size_t>((size_t)mesh_plan->local_nodes, 1) * sizeof(double);
  HIP_CHECK(hipMalloc(&pc->Au, bytes));                                            // :70
  HIP_CHECK(hipMalloc(&pc->residual, bytes));                                      // :71
  return pc;
}

void d4est_hip_pc_schwarz_destroy(d4est_hip_pc_schwarz_t* pc) {
  if (!pc) return;
  (void)hipFree(pc->Au); (void)hipFree(pc->residual);
  delete pc;
}

void d4est_hip_pc_schwarz_apply(void* ctx, const double* r_dev, double* z_dev) {
  d4est_hip_pc_schwarz* pc = static_cast<d4est_hip_pc_schwarz*>(ctx);
  if (!pc || !r_dev || !z_dev) D4EST_HIP_ABORT("pc_schwarz_apply: NULL argument");
  d4est_hip::schwarz_pc_run(pc->schwarz, pc->plan, r_dev, z_dev, pc->Au, pc->residual, pc->iterations, pc->subdomain_iter,
                            pc->subdomain_atol, pc->subdomain_rtol);
}

}  // extern "C"
