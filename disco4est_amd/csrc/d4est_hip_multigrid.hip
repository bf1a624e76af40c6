// The hp-multigrid V-cycle on the device: d4est_solver_multigrid_vcycle / d4est_solver_multigrid_solve
// (src/Solver/d4est_solver_multigrid.c:751-1348, :1420-1506), the Chebyshev smoother driver with its eigenvalue-reuse rules
// (src/Solver/d4est_solver_multigrid_smoother_cheby.c:222-376), the Schwarz smoother (d4est_solver_multigrid_smoother_schwarz.c:89-204),
// the CG, Chebyshev and reuse_smoother bottom solvers (d4est_solver_multigrid_bottom_solver_cg.c:48-198,
// d4est_solver_multigrid_bottom_solver_cheby.c:59-113, d4est_solver_multigrid_bottom_solver_reuse_smoother.c:20-39) and the
// preconditioner d4est_krylov_pc_multigrid_apply (src/Solver/d4est_krylov_pc_multigrid.c:40-77).
//
// The object ties together pieces that exist: every level's operator is a plan (apply_lhs with whatever zeroth-order term and
// communication hooks the caller set on it), the smoother is cheby_iterate / cg_eigs or the caller's Schwarz handles (one per level,
// d4est_hip_schwarz.hip: schwarz_smoother_run), the bottom CG is cg_solve, the grid transfers are transfer objects.  Levels are numbered as in the reference: 0 = bottom (coarsest) ... n_levels - 1 = top (finest); transfers[l]
// connects level l (coarse) and l + 1 (fine).  The workspace is one arena per vector kind, laid out like the reference's Ae_at0,
// err_at0, res_at0, rres_at0 (:797-800): the top level first (stride_to_fine_data = 0), then every coarser level; Ae, err and res exist
// only below the top (the top uses the caller's Au, u, rhs), rres on every level.  Allocated once, at create.
//
// What the cycle itself adds between the smoother calls, compared with the reference's statements:
//   - err = 0 of every level (:859, :1115) is ONE memset over the err arena at the start of the cycle (nothing writes err before its
//     level's own fill);
//   - the restriction writes res_{l-1} directly: the reference restricts into rres_{l-1} and copies to res_{l-1} (:1090-1095), and
//     nobody reads rres_{l-1} before that level's smoother overwrites it;
//   - the correction u_{l+1} += P err_l is one kernel (d4est_hip_transfer_prolong_add): the reference copies err_l to rres_l, prolongs
//     into rres_{l+1} and adds with axpy 1.0 (:1182-1250) -- P err_l is rounded to a double before it is added in both, so the numbers
//     are the same bit for bit; environment D4EST_HIP_MG_UNFUSED_CORRECTION=1 (read at create) runs prolong + add as two kernels;
//   - vcycle_r2 = rres_top . rres_top (:1330-1332) through the plan's fixed-order two-stage reduction (no atomics).
// The host reads r2 once per cycle (the stop rule of :1467-1494); that is the only synchronisation the object adds to those its parts
// make (cg_eigs reads its Lanczos coefficients, cg_solve its stop flag, a Schwarz iterate its "still iterating" counter before the
// first and then every 8th subdomain sweep).
//
// Not here: the Schwarz smoother on plans with ghost sides (the whole-element exchanges around an iterate are the host's), the PETSc
// bottom solver, the reference-named compat entry points (they need d4est_solver_multigrid_t's layout and a mutating p4est),
// hierarchies coarsened across ranks (every level's hooks are simply used).
// Coarse operators are whatever the caller set on plans[l]; homogeneous boundary data on every level is the caller's contract, as in the
// reference, where build_rhs_with_strong_bc moved g into rhs.  The object never switches D4EST_HIP_TUNE_GRAPH on: the plans are the
// caller's (a caller may set key 9 on launch-bound coarse plans).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "d4est_hip_internal.h"
#include "d4est_hip_transfer.h"

namespace d4est_hip {

namespace {

// the per-level smoother as the V-cycle sees it (d4est_solver_multigrid_smoother_t: smooth + update)
struct Smoother {
  virtual ~Smoother() {}
  virtual void pre_v(int vcycle_index) = 0;           // mg_state == PRE_V
  virtual void upv_pre_smooth(int vcycle_index) = 0;  // mg_state == UPV_PRE_SMOOTH
  // smooth A u = rhs on `level`; r = rhs - A u of the final iterate on exit
  virtual void smooth(int level, double* u, const double* rhs, double* Au, double* r) = 0;
  virtual double eig(int level) const = 0;            // the spectral bound last used on `level`, -1: none (or a smoother without one)
  virtual bool covers_level0() const = 0;             // the smoother can run on level 0 (the reuse_smoother bottom solver)
};

}  // namespace

}  // namespace d4est_hip

struct d4est_hip_multigrid {
  int n_levels = 0;
  std::vector<d4est_hip_plan*> plans;
  std::vector<d4est_hip_transfer*> transfers;
  std::vector<long long> nodes, off;   // off[l]: stride_to_fine_data of level l (off[top] = 0)
  long long total_nodes = 0, top_nodes = 0, max_nodes = 0;
  double *Ae = nullptr, *err = nullptr, *res = nullptr;   // levels below the top: level l at [off[l] - top_nodes]
  double* rres = nullptr;                                 // every level: level l at [off[l]]
  double* zero = nullptr;      // the zero start of cheby_use_zero_guess_for_eigs (max_nodes)
  double* pc_Au = nullptr;     // the preconditioner's Au (top_nodes), d4est_krylov_pc_multigrid.c:51
  double* r2_dev = nullptr;
  double* r2_host = nullptr;   // pinned
  bool fused_correction = true;
  d4est_hip::Smoother* smoother = nullptr;
  // bottom solver: 0 none, 1 CG, 2 Chebyshev, 3 reuse_smoother
  int bottom_kind = 0;
  int bottom_imax = 0;
  double bottom_atol = 0.0, bottom_rtol = 0.0;
  int bcheby_imax = 0, bcheby_eigs_cg_imax = 0, bcheby_use_new = 0;
  double bcheby_ratio = 1.0, bcheby_multiplier = 1.0, bcheby_eig = 0.0;
  // preconditioner parameters (d4est_hip_multigrid_set_pc)
  int pc_imax = 1;
  double pc_atol = 0.0, pc_rtol = 0.0;
  // reports
  int last_vcycles = 0, last_bottom_iterations = 0;

  hipStream_t stream() const { return plans[n_levels - 1]->stream; }
  double* lvl(double* arena, int l) const { return arena + (off[l] - top_nodes); }   // Ae / err / res of a level below the top
};

namespace d4est_hip {

namespace {

// d4est_solver_multigrid_smoother_cheby (d4est_solver_multigrid_smoother_cheby.c:222-376)
struct ChebySmoother : Smoother {
  d4est_hip_multigrid* mg;
  int cheby_imax, eigs_cg_imax, reuse_fromdown, reuse_fromlast, use_new, use_zero_guess;
  double ratio, multiplier;
  int eigs_compute = 1;
  std::vector<double> eigs;

  void pre_v(int vcycle) override {             // :234-244
    eigs_compute = (reuse_fromlast == 1 && vcycle != 0) ? 0 : 1;
  }
  void upv_pre_smooth(int vcycle) override {    // :246-257
    eigs_compute = (reuse_fromdown == 1 || (reuse_fromlast == 1 && vcycle != 0)) ? 0 : 1;
  }
  void smooth(int level, double* u, const double* rhs, double* Au, double* r) override {
    d4est_hip_plan* plan = mg->plans[level];
    if (eigs_compute) {                          // :280-311
      double* start = u;                         // cg_eigs advances the iterate it is given, as in the reference
      if (use_zero_guess) {                      // :282-286: a zero vector stands in for u, which stays as it is
        start = mg->zero;
        HIP_CHECK(hipMemsetAsync(start, 0, std::max<size_t>((size_t)plan->local_nodes, 1) * sizeof(double), plan->stream));
      }
      eigs[level] = cg_eigs(plan, start, rhs, Au, eigs_cg_imax, use_new, nullptr);
      eigs[level] *= multiplier;                 // :310
    }
    // :313-318 (use_zero_guess without reuse_fromdownvcycle) is refused by the setter.  :320-353 runs one more cg_eigs from a zero vector
    // whose bound goes to a dummy: it writes only that zero vector and Au, which the first apply of the iteration below overwrites,
    // so it has no effect on any vector the cycle reads and is skipped here.
    const double lmax = eigs[level], lmin = eigs[level] / ratio;   // :355-357
    cheby_iterate(plan, u, rhs, Au, r, cheby_imax, lmin, lmax, 1);  // :364-375
  }
  double eig(int level) const override { return eigs[level]; }
  // level 0 takes its bound like any other level: eigs_compute is what PRE_V left (the update callback knows no bottom state,
  // :234-257), so the first cycle always computes eigs[0] before a later one can reuse it
  bool covers_level0() const override { return true; }
};

// d4est_solver_multigrid_smoother_schwarz (src/Solver/d4est_solver_multigrid_smoother_schwarz.c:89-204)
struct SchwarzSmoother : Smoother {
  d4est_hip_multigrid* mg;
  std::vector<d4est_hip_schwarz*> schwarz_on_level;   // the caller's handles (:221, :240-242)
  int iterations, subdomain_iter;
  double subdomain_atol, subdomain_rtol;

  // d4est_solver_multigrid_smoother_schwarz_update (:296-365) keeps debug counters and builds the level's Schwarz data at
  // DOWNV_POST_BALANCE; the data are the caller's here, so nothing is left for PRE_V and UPV_PRE_SMOOTH: no eigenvalue state
  void pre_v(int) override {}
  void upv_pre_smooth(int) override {}
  void smooth(int level, double* u, const double* rhs, double* /*Au: the reference's smoother leaves vecs->Au alone, :112-113*/,
              double* r) override {
    // :110-152 iterations x { r = rhs - A u; schwarz_iterate(u, r) }, :154-196 r = rhs - A u
    schwarz_smoother_run(schwarz_on_level[level], mg->plans[level], u, rhs, r, iterations, subdomain_iter, subdomain_atol, subdomain_rtol);
  }
  double eig(int) const override { return -1.0; }
  bool covers_level0() const override { return schwarz_on_level[0] != nullptr; }
};

const char* check_message(int code) {
  switch (code) {
    case 0: return "ok";
    case 1: return "The code sees less than two multigrid levels, cannot run multigrid, try increasing min_level in initial_mesh";
    case 2: return "NULL plan or transfer entry";
    case 3: return "a transfer's node counts do not match the plans of its two levels";
    default: return "unknown";
  }
}

void require_ready(d4est_hip_multigrid* mg, const char* who) {
  if (!mg) D4EST_HIP_ABORT("%s: NULL multigrid object", who);
  if (!d4est_hip_multigrid_ready(mg)) D4EST_HIP_ABORT("%s: the object is not ready (set a smoother and a bottom solver first)", who);
}

// the bottom solver on (err_0, res_0, Ae_0); rres_0 is its residual vector
void bottom_solve(d4est_hip_multigrid* mg) {
  d4est_hip_plan* plan = mg->plans[0];
  double *u = mg->lvl(mg->err, 0), *rhs = mg->lvl(mg->res, 0), *Au = mg->lvl(mg->Ae, 0), *r = mg->rres + mg->off[0];
  if (mg->bottom_kind == 1) {
    // d4est_solver_multigrid_bottom_solver_cg.c:48-198 is the recurrence of d4est_solver_cg_solve, statement for statement
    mg->last_bottom_iterations = cg_solve(plan, u, rhs, Au, mg->bottom_imax, mg->bottom_atol, mg->bottom_rtol, nullptr);
  } else if (mg->bottom_kind == 3) {
    // d4est_solver_multigrid_bottom_solver_reuse_smoother.c:30-37: smoother->smooth(p4est, vecs, fcns, r, 0)
    mg->smoother->smooth(0, u, rhs, Au, r);
    mg->last_bottom_iterations = 0;   // (the smoother reports no count)
  } else {
    // d4est_solver_multigrid_bottom_solver_cheby.c:73-112: cg_eigs from the current iterate on every call, the multiplier, the iteration
    mg->bcheby_eig = cg_eigs(plan, u, rhs, Au, mg->bcheby_eigs_cg_imax, mg->bcheby_use_new, nullptr);
    mg->bcheby_eig *= mg->bcheby_multiplier;
    cheby_iterate(plan, u, rhs, Au, r, mg->bcheby_imax, mg->bcheby_eig / mg->bcheby_ratio, mg->bcheby_eig, 1);
    mg->last_bottom_iterations = mg->bcheby_imax;
  }
}

// d4est_solver_multigrid_vcycle (:751-1348); leaves vcycle_r2_local in mg->r2_dev
void vcycle(d4est_hip_multigrid* mg, double* u, const double* rhs, double* Au, int vcycle_index) {
  const int top = mg->n_levels - 1;
  hipStream_t st = mg->stream();
  // err = 0 on every level below the top (:859, :1115)
  HIP_CHECK(hipMemsetAsync(mg->err, 0, std::max<size_t>((size_t)(mg->total_nodes - mg->top_nodes), 1) * sizeof(double), st));
  mg->smoother->pre_v(vcycle_index);                                                             // :843
  for (int level = top; level > 0; --level) {                                                    // :847
    double* r = mg->rres + mg->off[level];
    if (level == top) mg->smoother->smooth(level, u, rhs, Au, r);                                // :861-866, :905-912
    else mg->smoother->smooth(level, mg->lvl(mg->err, level), mg->lvl(mg->res, level), mg->lvl(mg->Ae, level), r);   // :867-872
    // restriction of rres_level (:1054-1077); res_{level-1} = rres_{level-1} (:1090-1095) written directly
    d4est_hip_transfer_restrict(mg->transfers[level - 1], r, mg->lvl(mg->res, level - 1));
  }
  bottom_solve(mg);                                                                              // :1115-1148
  for (int level = 0; level < top; ++level) {                                                    // :1168
    double* fine_u = (level + 1 == top) ? u : mg->lvl(mg->err, level + 1);                       // :1231-1242
    if (mg->fused_correction) {
      // rres_level = err_level (:1182-1184), its prolongation into rres_{level+1} (:1199-1205), u_{level+1} += rres_{level+1} (:1250)
      d4est_hip_transfer_prolong_add(mg->transfers[level], mg->lvl(mg->err, level), fine_u);
    } else {
      double* rf = mg->rres + mg->off[level + 1];
      d4est_hip_transfer_prolong(mg->transfers[level], mg->lvl(mg->err, level), rf);
      // u_{level+1} += rres_{level+1}, on the top plan's stream like the rest of the cycle (a level's node count is its plan's: an int)
      launch_add(mg->plans[top], mg->plans[level + 1]->local_nodes, rf, fine_u);
    }
    mg->smoother->upv_pre_smooth(vcycle_index);                                                  // :1261
    double* r = mg->rres + mg->off[level + 1];
    if (level + 1 == top) mg->smoother->smooth(level + 1, u, rhs, Au, r);                        // :1263-1270
    else mg->smoother->smooth(level + 1, mg->lvl(mg->err, level + 1), mg->lvl(mg->res, level + 1), mg->lvl(mg->Ae, level + 1), r);
  }
  // vcycle_r2_local_current = rres_top . rres_top (:1330-1332)
  launch_dot(mg->plans[top], (int)mg->top_nodes, mg->rres, mg->rres, mg->r2_dev);
}

// r2 through the finest plan's allreduce hook (1 scalar, d4est_solver_multigrid_compute_residual :1392-1416), then to the host
double read_r2_global(d4est_hip_multigrid* mg) {
  d4est_hip_plan* plan = mg->plans[mg->n_levels - 1];
  if (plan->allreduce_fn) plan->allreduce_fn(plan->comm_ctx, mg->r2_dev, 1);
  HIP_CHECK(hipMemcpyAsync(mg->r2_host, mg->r2_dev, sizeof(double), hipMemcpyDeviceToHost, plan->stream));
  HIP_CHECK(hipStreamSynchronize(plan->stream));
  return *mg->r2_host;
}

// d4est_solver_multigrid_solve (:1420-1506)
int solve(d4est_hip_multigrid* mg, double* u, const double* rhs, double* Au, int imax, double atol, double rtol, double* hist) {
  d4est_hip_plan* plan = mg->plans[mg->n_levels - 1];
  // :1365-1402: r = -Au + rhs, r2_0 = r.r (rres_top is free until the first smoother call writes it)
  apply_operator(plan, u, Au);
  launch_residual(plan, plan->local_nodes, rhs, Au, mg->rres);
  launch_dot(plan, plan->local_nodes, mg->rres, mg->rres, mg->r2_dev);
  double r2 = read_r2_global(mg);
  double r2_last = r2;                                                // :1455
  const double stoptol = rtol * rtol * r2 + atol * atol;              // :1458-1459
  if (hist) hist[0] = r2;
  int n = 0;
  while (n < imax && r2 > stoptol) {                                  // :1467-1472
    vcycle(mg, u, rhs, Au, n);                                        // :1475 (vcycle_num_finished = n)
    r2 = read_r2_global(mg);                                          // :1477-1482
    n++;                                                              // :1484
    if (hist) hist[n] = r2;
    if (std::sqrt(r2 / r2_last) >= .99) break;                        // :1488-1491
    r2_last = r2;                                                     // :1493
  }
  mg->last_vcycles = n;
  return n;
}

}  // namespace

}  // namespace d4est_hip

extern "C" {

int d4est_hip_multigrid_check(int n_levels, d4est_hip_plan_t* const* plans, d4est_hip_transfer_t* const* transfers) {
  if (n_levels < 2) return 1;   // d4est_solver_multigrid.c:1435-1438
  if (!plans || !transfers) return 2;
  for (int l = 0; l < n_levels; ++l)
    if (!plans[l]) return 2;
  for (int l = 0; l + 1 < n_levels; ++l)
    if (!transfers[l]) return 2;
  for (int l = 0; l + 1 < n_levels; ++l)
    if (transfers[l]->coarse_nodes != plans[l]->local_nodes || transfers[l]->fine_nodes != plans[l + 1]->local_nodes) return 3;
  return 0;
}

d4est_hip_multigrid_t* d4est_hip_multigrid_create(int n_levels, d4est_hip_plan_t* const* plans, d4est_hip_transfer_t* const* transfers) {
  const int code = d4est_hip_multigrid_check(n_levels, plans, transfers);
  if (code != 0) D4EST_HIP_ABORT("multigrid_create: %s (code %d)", d4est_hip::check_message(code), code);
  d4est_hip_multigrid* mg = new d4est_hip_multigrid();
  mg->n_levels = n_levels;
  mg->plans.assign(plans, plans + n_levels);
  mg->transfers.assign(transfers, transfers + (n_levels - 1));
  mg->nodes.resize(n_levels);
  mg->off.resize(n_levels);
  long long o = 0;
  for (int l = n_levels - 1; l >= 0; --l) {   // the top level first, as stride_to_fine_data advances (:1097)
    mg->nodes[l] = plans[l]->local_nodes;
    mg->off[l] = o;
    o += mg->nodes[l];
    mg->max_nodes = std::max(mg->max_nodes, mg->nodes[l]);
  }
  mg->total_nodes = o;
  mg->top_nodes = mg->nodes[n_levels - 1];
  const size_t below = std::max<size_t>((size_t)(mg->total_nodes - mg->top_nodes), 1) * sizeof(double);
  HIP_CHECK(hipMalloc(&mg->Ae, below));
  HIP_CHECK(hipMalloc(&mg->err, below));
  HIP_CHECK(hipMalloc(&mg->res, below));
  HIP_CHECK(hipMalloc(&mg->rres, std::max<size_t>((size_t)mg->total_nodes, 1) * sizeof(double)));
  HIP_CHECK(hipMalloc(&mg->zero, std::max<size_t>((size_t)mg->max_nodes, 1) * sizeof(double)));
  HIP_CHECK(hipMalloc(&mg->pc_Au, std::max<size_t>((size_t)mg->top_nodes, 1) * sizeof(double)));
  HIP_CHECK(hipMalloc(&mg->r2_dev, sizeof(double)));
  HIP_CHECK(hipHostMalloc((void**)&mg->r2_host, sizeof(double), hipHostMallocDefault));
  mg->fused_correction = std::getenv("D4EST_HIP_MG_UNFUSED_CORRECTION") == nullptr;
  // one stream for the whole hierarchy: ordering between levels is stream order and nothing else
  d4est_hip_multigrid_set_stream(mg, plans[n_levels - 1]->stream);
  return mg;
}

void d4est_hip_multigrid_destroy(d4est_hip_multigrid_t* mg) {
  if (!mg) return;
  (void)hipFree(mg->Ae); (void)hipFree(mg->err); (void)hipFree(mg->res); (void)hipFree(mg->rres); (void)hipFree(mg->zero);
  (void)hipFree(mg->pc_Au); (void)hipFree(mg->r2_dev);
  if (mg->r2_host) (void)hipHostFree(mg->r2_host);
  delete mg->smoother;
  delete mg;
}

void d4est_hip_multigrid_set_stream(d4est_hip_multigrid_t* mg, void* hip_stream) {
  if (!mg) D4EST_HIP_ABORT("multigrid_set_stream: NULL multigrid object");
  for (d4est_hip_plan* p : mg->plans)
    if (p->stream != (hipStream_t)hip_stream) d4est_hip_plan_set_stream(p, hip_stream);
  for (d4est_hip_transfer* t : mg->transfers) d4est_hip_transfer_set_stream(t, hip_stream);
}

int d4est_hip_multigrid_set_smoother_cheby(d4est_hip_multigrid_t* mg, int cheby_imax, int cheby_eigs_cg_imax, double cheby_eigs_lmax_lmin_ratio,
                                           double cheby_eigs_max_multiplier, int cheby_eigs_reuse_fromdownvcycle,
                                           int cheby_eigs_reuse_fromlastvcycle, int cheby_use_new_cg_eigs, int cheby_use_zero_guess_for_eigs) {
  if (!mg) D4EST_HIP_ABORT("multigrid_set_smoother_cheby: NULL multigrid object");
  delete mg->smoother;
  mg->smoother = nullptr;
  // "If you set cheby_use_zero_guess_for_eigs == 1, please set cheby_eigs_reuse_fromdownvcycle = 1" (smoother_cheby.c:313-318)
  if (cheby_use_zero_guess_for_eigs == 1 && cheby_eigs_reuse_fromdownvcycle != 1) return 1;
  if (cheby_imax < 0 || cheby_eigs_cg_imax < 1 || !(cheby_eigs_lmax_lmin_ratio > 0.0)) return 2;
  d4est_hip::ChebySmoother* s = new d4est_hip::ChebySmoother();
  s->mg = mg;
  s->cheby_imax = cheby_imax;
  s->eigs_cg_imax = cheby_eigs_cg_imax;
  s->ratio = cheby_eigs_lmax_lmin_ratio;
  s->multiplier = cheby_eigs_max_multiplier;
  s->reuse_fromdown = cheby_eigs_reuse_fromdownvcycle;
  s->reuse_fromlast = cheby_eigs_reuse_fromlastvcycle;
  s->use_new = cheby_use_new_cg_eigs;
  s->use_zero_guess = cheby_use_zero_guess_for_eigs;
  s->eigs.assign(mg->n_levels, -1.0);   // (the reference allocates the array without a value, :391; -1 marks "none yet")
  mg->smoother = s;
  return 0;
}

int d4est_hip_multigrid_set_smoother_schwarz(d4est_hip_multigrid_t* mg, d4est_hip_schwarz_t* const* schwarz_on_level, int smoother_iterations,
                                             int subdomain_iter, double subdomain_atol, double subdomain_rtol) {
  if (!mg) D4EST_HIP_ABORT("multigrid_set_smoother_schwarz: NULL multigrid object");
  delete mg->smoother;
  mg->smoother = nullptr;
  if (!schwarz_on_level) return 1;
  for (int l = 1; l < mg->n_levels; ++l)
    if (!schwarz_on_level[l]) return 1;                 // (level 0 may be NULL: only the reuse_smoother bottom solver smooths there)
  for (int l = 0; l < mg->n_levels; ++l) {
    if (!schwarz_on_level[l]) continue;
    // 2: node counts, 3: streams, 4: ghost sides under a handle without an element exchange (or no faces)
    const int code = d4est_hip::schwarz_smoother_check(schwarz_on_level[l], mg->plans[l]);
    if (code != 0) return code;
  }
  // "some subdomain solver options are <= 0" (d4est_solver_schwarz_subdomain_solver_cg.c:86-92); a negative iteration count runs nothing
  if (subdomain_iter <= 0 || !(subdomain_atol > 0) || !(subdomain_rtol > 0) || smoother_iterations < 0) return 5;
  d4est_hip::SchwarzSmoother* s = new d4est_hip::SchwarzSmoother();
  s->mg = mg;
  s->schwarz_on_level.assign(schwarz_on_level, schwarz_on_level + mg->n_levels);
  s->iterations = smoother_iterations;
  s->subdomain_iter = subdomain_iter;
  s->subdomain_atol = subdomain_atol;
  s->subdomain_rtol = subdomain_rtol;
  mg->smoother = s;
  return 0;
}

void d4est_hip_multigrid_set_bottom_solver_reuse_smoother(d4est_hip_multigrid_t* mg) {
  if (!mg) D4EST_HIP_ABORT("multigrid_set_bottom_solver_reuse_smoother: NULL multigrid object");
  mg->bottom_kind = 3;   // d4est_solver_multigrid_bottom_solver_reuse_smoother_init (:5-18): no parameters of its own
}

void d4est_hip_multigrid_set_bottom_solver_cg(d4est_hip_multigrid_t* mg, int bottom_imax, double bottom_atol, double bottom_rtol) {
  if (!mg) D4EST_HIP_ABORT("multigrid_set_bottom_solver_cg: NULL multigrid object");
  if (bottom_imax < 0) D4EST_HIP_ABORT("multigrid_set_bottom_solver_cg: bottom_imax = %d", bottom_imax);
  mg->bottom_kind = 1;
  mg->bottom_imax = bottom_imax;
  mg->bottom_atol = bottom_atol;
  mg->bottom_rtol = bottom_rtol;
}

void d4est_hip_multigrid_set_bottom_solver_cheby(d4est_hip_multigrid_t* mg, int cheby_imax, int cheby_eigs_cg_imax, double lmax_lmin_ratio,
                                                 double max_multiplier, int use_new_cg_eigs) {
  if (!mg) D4EST_HIP_ABORT("multigrid_set_bottom_solver_cheby: NULL multigrid object");
  if (cheby_imax < 0 || cheby_eigs_cg_imax < 1 || !(lmax_lmin_ratio > 0.0))
    D4EST_HIP_ABORT("multigrid_set_bottom_solver_cheby: cheby_imax = %d, cheby_eigs_cg_imax = %d, ratio = %g", cheby_imax, cheby_eigs_cg_imax, lmax_lmin_ratio);
  mg->bottom_kind = 2;
  mg->bcheby_imax = cheby_imax;
  mg->bcheby_eigs_cg_imax = cheby_eigs_cg_imax;
  mg->bcheby_ratio = lmax_lmin_ratio;
  mg->bcheby_multiplier = max_multiplier;
  mg->bcheby_use_new = use_new_cg_eigs;
}

void d4est_hip_multigrid_set_pc(d4est_hip_multigrid_t* mg, int vcycle_imax, double vcycle_atol, double vcycle_rtol) {
  if (!mg) D4EST_HIP_ABORT("multigrid_set_pc: NULL multigrid object");
  if (vcycle_imax < 0) D4EST_HIP_ABORT("multigrid_set_pc: vcycle_imax = %d", vcycle_imax);
  mg->pc_imax = vcycle_imax;
  mg->pc_atol = vcycle_atol;
  mg->pc_rtol = vcycle_rtol;
}

int d4est_hip_multigrid_ready(const d4est_hip_multigrid_t* mg) {
  if (!mg || !mg->smoother || mg->bottom_kind == 0) return 0;
  if (mg->bottom_kind == 3 && !mg->smoother->covers_level0()) return 0;   // reuse_smoother needs the smoother on level 0
  return 1;
}

void d4est_hip_multigrid_smooth_level(d4est_hip_multigrid_t* mg, int level, double* u_dev, const double* rhs_dev, double* Au_dev,
                                      double* r_dev) {
  if (!mg || !mg->smoother) D4EST_HIP_ABORT("multigrid_smooth_level: no smoother is set");
  if (level < 0 || level >= mg->n_levels || (level == 0 && !mg->smoother->covers_level0()))
    D4EST_HIP_ABORT("multigrid_smooth_level: the smoother does not cover level %d", level);
  if (!u_dev || !rhs_dev || !Au_dev || !r_dev) D4EST_HIP_ABORT("multigrid_smooth_level: NULL vector");
  mg->smoother->smooth(level, u_dev, rhs_dev, Au_dev, r_dev);
}

void d4est_hip_multigrid_vcycle(d4est_hip_multigrid_t* mg, double* u_dev, const double* rhs_dev, double* Au_dev, int vcycle_index) {
  d4est_hip::require_ready(mg, "multigrid_vcycle");
  if (!u_dev || !rhs_dev || !Au_dev) D4EST_HIP_ABORT("multigrid_vcycle: NULL vector");
  d4est_hip::vcycle(mg, u_dev, rhs_dev, Au_dev, vcycle_index);
}

double d4est_hip_multigrid_vcycle_r2(d4est_hip_multigrid_t* mg) {
  if (!mg) D4EST_HIP_ABORT("multigrid_vcycle_r2: NULL multigrid object");
  HIP_CHECK(hipMemcpyAsync(mg->r2_host, mg->r2_dev, sizeof(double), hipMemcpyDeviceToHost, mg->stream()));
  HIP_CHECK(hipStreamSynchronize(mg->stream()));
  return *mg->r2_host;
}

int d4est_hip_multigrid_solve(d4est_hip_multigrid_t* mg, double* u_dev, const double* rhs_dev, double* Au_dev, int vcycle_imax,
                              double vcycle_atol, double vcycle_rtol, double* history_host) {
  d4est_hip::require_ready(mg, "multigrid_solve");
  if (!u_dev || !rhs_dev || !Au_dev) D4EST_HIP_ABORT("multigrid_solve: NULL vector");
  if (vcycle_imax < 0) D4EST_HIP_ABORT("multigrid_solve: vcycle_imax = %d", vcycle_imax);
  return d4est_hip::solve(mg, u_dev, rhs_dev, Au_dev, vcycle_imax, vcycle_atol, vcycle_rtol, history_host);
}

void d4est_hip_multigrid_pc_apply(void* ctx, const double* r_dev, double* z_dev) {
  d4est_hip_multigrid* mg = static_cast<d4est_hip_multigrid*>(ctx);
  d4est_hip::require_ready(mg, "multigrid_pc_apply");
  if (!r_dev || !z_dev) D4EST_HIP_ABORT("multigrid_pc_apply: NULL vector");
  // d4est_krylov_pc_multigrid.c:50-74: z = 0, a fresh Au, u = z, rhs = r, then d4est_solver_multigrid_solve
  HIP_CHECK(hipMemsetAsync(z_dev, 0, std::max<size_t>((size_t)mg->top_nodes, 1) * sizeof(double), mg->stream()));
  (void)d4est_hip::solve(mg, z_dev, r_dev, mg->pc_Au, mg->pc_imax, mg->pc_atol, mg->pc_rtol, nullptr);
}

void d4est_hip_multigrid_get_info(const d4est_hip_multigrid_t* mg, double* eigs_host, int* vcycles, int* bottom_iterations) {
  if (!mg) D4EST_HIP_ABORT("multigrid_get_info: NULL multigrid object");
  if (eigs_host) {
    for (int l = 0; l < mg->n_levels; ++l) eigs_host[l] = mg->smoother ? mg->smoother->eig(l) : -1.0;
    if (mg->bottom_kind == 2) eigs_host[0] = mg->bcheby_eig;   // level 0 is never smoothed: the bottom Chebyshev solver's bound
  }
  if (vcycles) *vcycles = mg->last_vcycles;
  if (bottom_iterations) *bottom_iterations = mg->last_bottom_iterations;
}

}  // extern "C"
