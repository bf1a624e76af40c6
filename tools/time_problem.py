"""Times the one-kernel puncture-term set-up (Plan.set_puncture_term, csrc/d4est_hip_problem.hip) against the path it replaces:
compute_xyz_analytic, a download, the numpy evaluation of a and b (tests/dense_problem.py, the reference's loop order), an upload and
set_nonlinear_power.  Mesh: the 13-tree cubed sphere at level 3, p = 7, two punctures (init_two_punctures_data's values).
Also times the load vector by id (Plan.build_load, STAMM_RHS and LORENTZIAN_RHS) against the three calls it replaces -- compute_xyz_analytic,
field_eval, apply_galerkin_integral -- and the Boyen-York / Okendon term setters (rows load_* and set_*_term_s; the geometric factors are
set for them).  Writes profiles/time_problem.json (or --out).  Usage: python tools/time_problem.py [--level 3] [--deg 7] [--reps 20] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--level", type=int, default=3)
    ap.add_argument("--deg", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_problem.json"))
    args = ap.parse_args()
    import torch
    from disco4est_amd import Plan, capi, forest as F
    from tests import dense_problem as DP
    gpu = torch.device("cuda:0")
    mp = F.CubedSphere13Map(1.0, 2.0, 20.0, compactify_outer=True)
    m = F.ForestMesh(F.cubed_sphere_13tree_connectivity(), args.level, args.deg, mp)
    tree, q, dq = m.cells()
    plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, 0)
    params = capi.puncture_params([[-3., 0., 0.], [3., 0., 0.]], [[0., -.2, 0.], [0., .2, 0.]], np.zeros((2, 3)), [.5, .5])
    src = (2, mp.params, tree, q, dq, m.nf)
    nq = plan.local_nodes_quad

    def sync():
        torch.cuda.synchronize(gpu)

    # the one-kernel path (host staging of the cell descriptions included)
    plan.set_puncture_term(params, analytic=src)
    sync()
    t_new = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        plan.set_puncture_term(params, analytic=src)
        sync()
        t_new.append(time.perf_counter() - t0)
    a_new, b_new, _ = plan.nonlinear_coefficients()
    a_new, b_new = a_new.clone(), b_new.clone()

    # the replaced path with its stages, twice: the first pass carries the first launch of the coordinate kernel and the first large
    # host copies of the process (cold), the second is the steady state (warm); the numpy evaluation dominates both
    xyz = torch.empty(3 * nq, dtype=torch.float64, device=gpu)

    def replaced():
        stages = {}
        t0 = time.perf_counter()
        plan.compute_xyz_analytic(*src, xyz_quad=xyz)
        sync()
        stages["compute_xyz_analytic"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        X = xyz.cpu().numpy().reshape(3, nq)
        stages["download"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        a = DP.puncture_a(X[0], X[1], X[2], params)
        b = DP.puncture_b(X[0], X[1], X[2], params)
        stages["numpy_evaluation"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        da, db = torch.from_numpy(a).to(gpu), torch.from_numpy(b).to(gpu)
        sync()
        stages["upload"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        plan.set_nonlinear_power(da, db, -7)
        sync()
        stages["set_nonlinear_power"] = time.perf_counter() - t0
        stages["total"] = float(sum(stages.values()))
        stages["total_without_numpy_evaluation"] = stages["total"] - stages["numpy_evaluation"]
        return stages, da, db
    cold, da, db = replaced()
    warm, da, db = replaced()
    # the device evaluation alone, on resident coordinates
    o = torch.empty(nq, dtype=torch.float64, device=gpu)
    capi.field_eval("PUNCTURE_A", params, xyz, o)
    sync()
    t0 = time.perf_counter()
    for _ in range(args.reps):
        capi.field_eval("PUNCTURE_A", params, xyz, o)
    sync()
    t_field = (time.perf_counter() - t0) / args.reps
    # the load vector by id against its three-call composition, and the two new term setters
    more = {}
    plan.set_geometry_analytic(2, mp.params, tree, q, dq, m.nf)
    n = plan.local_nodes
    fq = torch.empty(nq, dtype=torch.float64, device=gpu)
    load, load3 = torch.empty(n, dtype=torch.float64, device=gpu), torch.empty(n, dtype=torch.float64, device=gpu)

    def timed(fn):
        fn()
        sync()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            sync()
            ts.append(time.perf_counter() - t0)
        return {"median": float(np.median(ts)), "min": float(np.min(ts)), "max": float(np.max(ts))}
    for fid, pr in (("STAMM_RHS", capi.stamm_params(0.25, 0.3, 0.35)), ("LORENTZIAN_RHS", None)):
        def three_calls():
            plan.compute_xyz_analytic(*src, xyz_quad=xyz)
            capi.field_eval(fid, pr, xyz, fq, getattr(plan, "_stream_handle", 0))
            plan.apply_galerkin_integral(fq, load3)
        more["load_%s_one_kernel_s" % fid] = timed(lambda: plan.build_load(fid, pr, load, analytic=src))
        more["load_%s_three_calls_s" % fid] = timed(three_calls)
        more["load_%s_bit_equal" % fid] = bool(torch.equal(load, load3))
    more["load_one_kernel_path"] = bool(plan.nonlinear_fused())
    more["set_boyen_york_term_s"] = timed(lambda: plan.set_boyen_york_term(capi.boyen_york_params(0.7, 1.3), analytic=src))
    more["set_okendon_term_s"] = timed(lambda: plan.set_okendon_term(capi.okendon_params(0.5), analytic=src))
    scale = float(a_new.abs().max())
    res = {
        "tool": "tools/time_problem.py", "device": torch.cuda.get_device_name(0), "mesh": "cubed_sphere 13 trees, level %d, p = %d" % (args.level, args.deg),
        "elements": int(m.n_elements), "quadrature_nodes": int(nq), "punctures": 2, "reps": args.reps,
        "one_kernel_set_term_s": {"median": float(np.median(t_new)), "min": float(np.min(t_new)), "max": float(np.max(t_new))},
        "replaced_path_cold_s": cold, "replaced_path_warm_s": warm,
        "field_eval_puncture_a_s": t_field,
        "field_eval_points_per_s": nq / t_field,
        "max_abs_a_difference_between_paths": float((a_new - da).abs().max()), "max_abs_a": scale,
        "max_abs_b_difference_between_paths": float((b_new - db)[torch.isfinite(db)].abs().max()),
    }
    res.update(more)
    plan.destroy()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
