"""Time the device-generated geometry of the 13-tree cubed sphere against the upload of host-computed factors.

Mesh: [geometry] name = cubed_sphere at level 3, p = 7 (13 * 8^3 = 6656 elements), R = (1, 2, 6), Gauss quadrature, deg_quad = deg.

  candidate  Plan.set_geometry_analytic + set_mortar_geometry_analytic: the host passes tree, q, dq per element
  baseline   Plan.set_geometry + set_mortar_geometry fed host arrays that are ALREADY computed (96 B per quadrature node, 24 doubles
             per mortar node): upload plus pre-combination, without the Python map that produced them

Each is the wall clock around a plan synchronise, 3 warm-up and 10 timed repetitions, median reported.  Prints one JSON line.

    timeout 900 python tools/time_geometry.py [--level 3] [--deg 7] [--cache FILE.npz]

--cache keeps the host arrays of the baseline (minutes of numpy at level 3) in a file and re-uses them on the next run.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIDE_INT_KEYS = ("side_nbr", "side_nbr_face", "side_reorder", "side_mortar_stride", "side_bndry_stride", "ghost_deg", "ghost_deg_quad")
SIDE_REAL_KEYS = ("sj", "n", "drst_m", "drst_p", "hm", "hp")


def host_arrays(level, deg, cache):
    from disco4est_amd import forest as F
    if cache and os.path.exists(cache):
        z = np.load(cache)
        if int(z["level"]) == level and int(z["deg"]) == deg:
            return {k: z[k] for k in z.files}
    conn = F.cubed_sphere_13tree_connectivity()
    mp = F.CubedSphere13Map(1.0, 2.0, 6.0)
    m = F.ForestMesh(conn, level, deg, mp)
    J, rst = m.geometry()
    s = m.build_sides()
    tree, q, dq = m.cells()
    d = {"level": level, "deg": deg, "J": J, "rst": rst, "tree": tree, "q": q, "dq": dq, "nf": m.nf, "params": np.asarray(mp.params),
         "deg_e": m.deg, "deg_quad_e": m.deg_quad, "nodal_stride": m.nodal_stride, "quad_stride": m.quad_stride,
         "total_mortar_nodes": s["total_mortar_nodes"], "total_bndry_nodes": s["total_bndry_nodes"]}
    for k in SIDE_INT_KEYS + SIDE_REAL_KEYS:
        d[k] = np.asarray(s[k])
    if cache:
        np.savez(cache, **d)
    return d


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--level", type=int, default=3)
    ap.add_argument("--deg", type=int, default=7)
    ap.add_argument("--cache", default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-only", action="store_true", help="compute (and cache) the host arrays, then stop: needs no GPU")
    a = ap.parse_args()
    d = host_arrays(a.level, a.deg, a.cache)
    if a.host_only:
        return
    import torch
    from disco4est_amd import Plan
    if not torch.cuda.is_available():
        sys.exit("time_geometry: no GPU is visible")
    sides = {k: d[k] for k in SIDE_INT_KEYS + SIDE_REAL_KEYS}
    sides["total_mortar_nodes"], sides["total_bndry_nodes"] = int(d["total_mortar_nodes"]), int(d["total_bndry_nodes"])
    params, tree, q, dq, nf = d["params"], d["tree"], d["q"], d["dq"], float(d["nf"])
    plan = Plan(d["deg_e"], d["deg_quad_e"], d["nodal_stride"], d["quad_stride"], 0)
    plan.set_geometry(d["J"], d["rst"])
    plan.set_faces(sides, 10.0, 0)          # topology once; the timed calls replace the factors only
    arrs = [np.ascontiguousarray(sides[k], dtype=np.float64) for k in SIDE_REAL_KEYS]
    vp = [x.ctypes.data for x in arrs]

    def candidate():
        plan.set_geometry_analytic(2, params, tree, q, dq, nf)
        plan.set_geometry_analytic(2, params, tree, q, dq, nf, mortars=True)

    def baseline():
        plan.set_geometry(d["J"], d["rst"])
        plan.lib.d4est_hip_plan_set_mortar_geometry(plan.handle, *vp, 0)

    out = {"mesh": "cubed_sphere 13 trees", "level": a.level, "deg": a.deg, "elements": int(len(tree)),
           "host_bytes_baseline": int(d["J"].nbytes + d["rst"].nbytes + sum(x.nbytes for x in arrs)),
           "host_bytes_candidate": int(tree.nbytes + q.nbytes + dq.nbytes), "warmup": a.warmup, "reps": a.reps}
    for name, fn in (("baseline", baseline), ("candidate", candidate)):
        times = []
        for it in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if it >= a.warmup:
                times.append(time.perf_counter() - t0)
        out[name + "_median_ms"] = 1e3 * float(np.median(times))
        out[name + "_min_ms"] = 1e3 * float(np.min(times))
    plan.destroy()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
