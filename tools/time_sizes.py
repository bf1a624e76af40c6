"""Wall time of the size-parameter pass (d4est_hip_plan_compute_size_parameters_analytic) on the 13-tree sphere at level 3
(13 * 512 elements), for p = 7 and p = 15: the figure recorded in DESIGN.md section 12.  Prints one JSON line per degree.

    python tools/time_sizes.py [--level 3] [--degrees 7 15] [--repeat 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--level", type=int, default=3)
    ap.add_argument("--degrees", type=int, nargs="+", default=[7, 15])
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    import torch
    from disco4est_amd import Plan, build as b, forest as F
    from disco4est_amd.mesh import morton_order
    if b.needs_build():
        b.build_library(verbose=False)
    assert torch.cuda.is_available(), "needs a GPU"
    mp = F.CubedSphere13Map(1.0, 2.0, 20.0, compactify_outer=True)
    base = morton_order(a.level)
    nb, nf = base.shape[0], 1 << a.level
    tree = np.repeat(np.arange(13), nb).astype(np.int32)
    q = np.tile(base, (13, 1)).astype(np.int32)
    dq = np.ones(13 * nb, dtype=np.int32)
    for p in a.degrees:
        n3 = (p + 1) ** 3
        stride = (np.arange(13 * nb, dtype=np.int64) * n3).astype(np.int32)
        deg = np.full(13 * nb, p, dtype=np.int32)
        plan = Plan(deg, deg, stride, stride, 0)
        form = (2, mp.params, tree, q, dq, float(nf))
        plan.compute_size_parameters(analytic=form)      # first call: allocations
        torch.cuda.synchronize()
        times = []
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            plan.compute_size_parameters(analytic=form)
            plan.lib.d4est_hip_plan_synchronize(plan.handle)
            times.append(time.perf_counter() - t0)
        dv = plan.size_parameter("diam_volume")
        print(json.dumps({"what": "size parameters, 13-tree sphere", "level": a.level, "elements": int(13 * nb), "deg": p,
                          "pairs_per_element": n3 * n3, "ms_median": 1e3 * float(np.median(times)), "ms_min": 1e3 * min(times),
                          "diam_volume_max": float(dv.max())}))
        plan.destroy()


if __name__ == "__main__":
    main()
