"""Timing of the fused nonlinear term and linearisation (csrc/d4est_hip_nonlinear.hip): tools/time_nonlinear.py [out.json]

On config 2's mesh (level-4 brick, p = 7, 2.1 MDoF) and on bench.py's mixed_p3_to_9_level4 (p = 3 ... 9 scattered over the level-4 brick),
with the TwoPunctures-shaped power k = -7 and a, b given at the quadrature nodes:
* residual term: d4est_hip_apply_nonlinear_term (one kernel) against the composition it replaces -- d4est_hip_interpolate, a torch
  pointwise expression, d4est_hip_apply_galerkin_integral;
* linearisation: d4est_hip_plan_linearise (one kernel: c and w J c) against interpolate, the pointwise expression,
  d4est_hip_plan_set_lhs_coefficient (a copy) and the w J c pass the first apply after it runs -- timed through that apply
  (d4est_hip_apply_weighted_mass_matrix on the separate path does not read w J c, so the composed row times the pass by the difference
  between the first apply_lhs after set_lhs_coefficient and a second one; both rows are printed).
Event-timed on the plan's stream after warm-up, 50 repetitions, median / min / max; the two forms alternate.  The composed rows use only
entry points the library had before the fused ones, so the script gives the baseline on an older checkout (fused rows are skipped).
Where the library has the real form a |b + u|^s (d4est_hip_plan_set_nonlinear_abs_power, s = 0.5) the same two comparisons are timed
for it: the rows term_abs_* and linearise_abs_*."""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from disco4est_amd import Plan, mesh as M  # noqa: E402

dev = torch.device("cuda:0")
REPS, WARM, K, S_ABS = 50, 5, -7, 0.5


def timed_pair(fns, stream):
    """event-timed repetitions of every callable in turn (alternating): {name: stats in us}"""
    ts = {k: [] for k in fns}
    with torch.cuda.stream(stream):
        for _ in range(WARM):
            for f in fns.values():
                f()
        stream.synchronize()
        for _ in range(REPS):
            for k, f in fns.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                f()
                b.record(stream)
                b.synchronize()
                ts[k].append(a.elapsed_time(b) * 1e3)
    return {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "reps": REPS} for k, v in ts.items()}


def case(name, degs, stream):
    m = M.BrickMesh(4, degs)
    J, rst = m.geometry(None)
    plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, 0, stream=stream)
    plan.set_geometry(J, rst)
    plan.set_faces(m.build_sides(None))
    nq = m.local_nodes_quad
    a = torch.from_numpy(-(0.5 + M.splitmix64_uniform(11, nq))).to(dev)
    b = torch.from_numpy(1.0 + 0.2 * M.splitmix64_uniform(12, nq)).to(dev)
    u = torch.from_numpy(0.1 * M.splitmix64_uniform(13, m.local_nodes)).to(dev)
    out, out2 = torch.empty_like(u), torch.empty_like(u)
    uq = torch.empty(nq, dtype=torch.float64, device=dev)
    Ka = K * a
    fused = hasattr(plan, "apply_nonlinear_term")
    r = float(nq) / m.local_nodes

    def term_composed():
        plan.interpolate(u, uq)
        plan.apply_galerkin_integral(a * torch.pow(b + uq, K), out)

    def lin_composed():
        plan.interpolate(u, uq)
        plan.set_lhs_coefficient(Ka * torch.pow(b + uq, K - 1))
        plan.apply_lhs(u, out)           # the first apply forms w J c (or reads c on the separate path)

    def lhs_only():
        plan.apply_lhs(u, out)

    fns = {"term_composed": term_composed}
    if fused:
        plan.set_nonlinear_power(a, b, K)
        fns["term_fused"] = lambda: plan.apply_nonlinear_term(u, out2, 0)
    res = timed_pair(fns, stream)
    lin = {"linearise_composed_plus_apply_lhs": lin_composed, "apply_lhs_alone": lhs_only}
    if fused:
        def lin_fused():
            plan.linearise(u)
            plan.apply_lhs(u, out2)
        lin["linearise_fused_plus_apply_lhs"] = lin_fused
    res.update(timed_pair(lin, stream))
    if hasattr(plan, "set_nonlinear_abs_power"):
        def term_abs_composed():
            plan.interpolate(u, uq)
            t = b + uq
            plan.apply_galerkin_integral(a * torch.pow(t * t, 0.5 * S_ABS), out)

        def lin_abs_composed():
            plan.interpolate(u, uq)
            t = b + uq
            plan.set_lhs_coefficient((S_ABS * a) / torch.pow(t * t, 0.5 * (1.0 - S_ABS)))
            plan.apply_lhs(u, out)

        def lin_abs_fused():
            plan.linearise(u)
            plan.apply_lhs(u, out2)
        plan.set_nonlinear_abs_power(a, b, S_ABS)
        res.update(timed_pair({"term_abs_composed": term_abs_composed,
                               "term_abs_fused": lambda: plan.apply_nonlinear_term(u, out2, 0)}, stream))
        res.update(timed_pair({"linearise_abs_composed_plus_apply_lhs": lin_abs_composed,
                               "linearise_abs_fused_plus_apply_lhs": lin_abs_fused}, stream))
        with torch.cuda.stream(stream):
            term_abs_composed()
            plan.apply_nonlinear_term(u, out2, 0)
        stream.synchronize()
        res["term_abs_rel_inf_difference"] = float((out - out2).abs().max() / out.abs().max())
        plan.set_nonlinear_power(a, b, K)
    if fused:
        with torch.cuda.stream(stream):   # (the torch expression must run on the plan's stream)
            term_composed()
            plan.apply_nonlinear_term(u, out2, 0)
        stream.synchronize()
        res["term_rel_inf_difference"] = float((out - out2).abs().max() / out.abs().max())
        res["fused_single_kernel"] = bool(plan.nonlinear_fused())
    res.update({"dofs": m.local_nodes, "elements": m.n_elements, "quad_nodes_per_dof": r, "face_path": plan.face_path(),
                "bytes_per_dof_fused_term": 16 + 24 * r, "bytes_per_dof_composed_term_min": 16 + 40 * r})
    for k, v in res.items():
        print("%-22s %-36s %s" % (name, k, ("%.1f us (min %.1f, max %.1f)" % (v["median_us"], v["min_us"], v["max_us"])) if isinstance(v, dict) else v))
    plan.destroy()
    return res


def main():
    stream = torch.cuda.Stream()
    out = {"config2_level4_p7": case("config2_level4_p7", 7, stream),
           "mixed_p3_to_9_level4": case("mixed_p3_to_9_level4", 3 + (np.arange(8 ** 4) * 5) % 7, stream)}
    line = json.dumps(out)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        open(sys.argv[1], "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
