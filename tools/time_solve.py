"""Timing of the device Krylov solves (d4est_hip_cg_solve / _fcg_solve): tools/time_solve.py [out.json]

* CG on config 2's mesh (level-4 brick, p = 7, 2.1 MDoF): ms per iteration against one apply_lhs;
* the bottom-level CG of a multigrid hierarchy (level-2 brick, p = 1, 512 DoF, launch-bound): us per iteration for several
  D4EST_HIP_TUNE_KRYLOV_CHECK batch sizes (1 = one host read of the stop flag per iteration);
* FCG without preconditioner on config 2's mesh: ms per iteration.
Each timed configuration is preceded by a parity check: the solve with the stop flag read after every iteration gives the same count
and the same u, bit for bit."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from disco4est_amd import Plan, mesh as M  # noqa: E402

KRYLOV_CHECK = 15
dev = torch.device("cuda:0")


def setup(level, deg):
    m = M.BrickMesh(level, deg)
    J, rst = m.geometry(None); sides = m.build_sides(None)
    plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, 0)
    plan.set_geometry(J, rst)
    plan.set_faces(sides, 10.0, 0)
    rhs = torch.from_numpy(M.splitmix64_uniform(5, m.local_nodes) - 0.5).to(dev)
    return m, plan, rhs


def wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def parity(plan, rhs, imax, rtol, check):
    runs = []
    for c in (1, check):
        plan.set_tuning(KRYLOV_CHECK, c)
        u = torch.zeros_like(rhs); Au = torch.empty_like(rhs)
        it, _ = plan.cg_solve(u, rhs, Au, imax, 0.0, rtol)
        runs.append((it, u.cpu().numpy()))
    assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1]), "batch %d changes the solve" % check
    return runs[0][0]


def cg_per_iter(plan, rhs, iters, reps):
    """(solve with `iters` iterations - solve with 0 iterations) / iters: the set-up apply and the final reads cancel"""
    u = torch.zeros_like(rhs); Au = torch.empty_like(rhs)
    t_n = wall(lambda: (u.zero_(), plan.cg_solve(u, rhs, Au, iters, 0.0, 0.0)), reps)
    t_0 = wall(lambda: (u.zero_(), plan.cg_solve(u, rhs, Au, 0, 0.0, 0.0)), reps)
    return (t_n - t_0) / iters


def main():
    out = {}
    # config 2: level-4 brick, p = 7
    m, plan, rhs = setup(4, 7)
    out["config2"] = {"local_nodes": m.local_nodes, "face_path": plan.face_path()}
    out["config2"]["parity_iterations"] = parity(plan, rhs, 40, 0.0, 8)
    x = torch.rand_like(rhs); Ax = torch.empty_like(rhs)
    out["config2"]["apply_lhs_us"] = wall(lambda: plan.apply_lhs(x, Ax), 50) * 1e6
    plan.set_tuning(KRYLOV_CHECK, -1)
    t = cg_per_iter(plan, rhs, 40, 5)
    out["config2"]["cg_us_per_iter"] = t * 1e6
    # 11 vector passes of 8 B x local_nodes: the BLAS-1 share at the issue's 5 TB/s target
    out["config2"]["blas1_floor_us"] = 11 * 8 * m.local_nodes / 5e12 * 1e6
    out["config2"]["cg_minus_apply_us"] = out["config2"]["cg_us_per_iter"] - out["config2"]["apply_lhs_us"]
    u = torch.zeros_like(rhs); Au = torch.empty_like(rhs)
    t_f = wall(lambda: (u.zero_(), plan.fcg_solve(u, rhs, Au, 40, 0.0, 0.0)), 5)
    t_f0 = wall(lambda: (u.zero_(), plan.fcg_solve(u, rhs, Au, 0, 0.0, 0.0)), 5)
    out["config2"]["fcg_identity_us_per_iter"] = (t_f - t_f0) / 40 * 1e6
    plan.destroy()
    # the bottom level of config 2's hierarchy: level-2 brick, p = 1 (the reference's bottom CG: up to 100 iterations, rtol 1e-10)
    m, plan, rhs = setup(2, 1)
    out["bottom"] = {"local_nodes": m.local_nodes, "face_path": plan.face_path(), "us_per_iter": {}}
    out["bottom"]["parity_iterations"] = parity(plan, rhs, 100, 1e-10, 8)
    x = torch.rand_like(rhs); Ax = torch.empty_like(rhs)
    out["bottom"]["apply_lhs_us"] = wall(lambda: plan.apply_lhs(x, Ax), 200) * 1e6
    for check in (1, 4, 8, 16, 32, 100):
        plan.set_tuning(KRYLOV_CHECK, check)
        out["bottom"]["us_per_iter"][str(check)] = cg_per_iter(plan, rhs, 100, 10) * 1e6
    plan.destroy()
    print(json.dumps(out, indent=1))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
