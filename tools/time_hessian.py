"""Times d4est_hip_hessian_trace on one GPU: the brick at level 4 (4096 elements) at p = 3, 7, 11, 15 and the 13-tree cubed sphere
(level 2, p = 7).  Prints microseconds per apply (median of the timed calls, events on the plan's stream), GDoF/s and the fraction of
the algorithmic traffic of 88 B/DoF (8 u + 72 coefficients + 8 out at deg_quad = deg) against 8 TB/s.

    python tools/time_hessian.py [--reps 20]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(plan, n_nodes, n_quad, reps, dev):
    import torch
    u = torch.rand(n_nodes, dtype=torch.float64, device=dev)
    out = torch.empty(n_quad, dtype=torch.float64, device=dev)
    for _ in range(3):
        plan.hessian_trace(u, out)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        plan.hessian_trace(u, out)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    assert bool(torch.isfinite(out).all())
    return float(np.median(ts))


def main():
    import torch
    from disco4est_amd import Plan, forest as F
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for p in (3, 7, 11, 15):
        ne, n3 = 4096, (p + 1) ** 3
        stride = np.arange(ne, dtype=np.int64) * n3
        plan = Plan(np.full(ne, p), np.full(ne, p), stride, stride, 0)
        plan.set_hessian_brick(np.ones(ne, dtype=np.int32), 16.0, (0., 1., 0., 1., 0., 1.))
        rows.append(("brick level 4 p=%d" % p, ne * n3, _time(plan, ne * n3, ne * n3, args.reps, dev)))
        plan.destroy()
    mp = F.CubedSphere13Map(1.0, 2.0, 6.0)
    fm = F.ForestMesh(F.cubed_sphere_13tree_connectivity(), 2, 7, mp)
    plan = Plan(fm.deg, fm.deg_quad, fm.nodal_stride, fm.quad_stride, 0)
    tree, q, dq = fm.cells()
    plan.set_hessian_analytic(2, mp.params, tree, q, dq, fm.nf)
    rows.append(("13-tree sphere level 2 p=7", fm.local_nodes, _time(plan, fm.local_nodes, fm.local_nodes_quad, args.reps, dev)))
    plan.destroy()
    for name, dofs, us in rows:
        gdofs = dofs / us * 1e-3
        print("%-28s %9d DoF  %9.1f us  %7.2f GDoF/s  %5.1f %% of 88 B/DoF at 8 TB/s" % (name, dofs, us, gdofs, 100.0 * gdofs * 88.0 / 8000.0))


if __name__ == "__main__":
    main()
