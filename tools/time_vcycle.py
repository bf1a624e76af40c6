"""Timing of the device V-cycle (d4est_hip_multigrid_vcycle): tools/time_vcycle.py [out.json]

* two-level: the hierarchy of bench.py's sec_multigrid (level-4 brick, p = 7 fine; level-3 brick, p = 7 coarse), the same work as its
  two_grid(): 3 Chebyshev iterations on a fixed window before and after the correction, 3 on the coarse level;
* three-level: p = 7 -> 3 -> 1 on the level-4 brick (two p-coarsenings).
One d4est_hip_multigrid_vcycle is timed with events on the plans' stream (warm-up, 30 repetitions: median, min, max) with the fused
correction (d4est_hip_transfer_prolong_add) and with prolong + add as two kernels (D4EST_HIP_MG_UNFUSED_CORRECTION=1), against the same
cycle composed from Python calls exactly as sec_multigrid's two_grid() does.  The Python composition uses only entry points the
library had before the multigrid object, so the same script run on an older checkout (where `Multigrid` does not exist: those rows are
then skipped) gives the baseline.  To take the eigenvalue estimate out of the timed region the object runs with
reuse_fromlastvcycle = 1 and vcycle_index = 1 after one untimed cycle with index 0; the Python composition is given the bounds that cycle
found.  Then FCG on the two-level hierarchy to a relative residual of 1e-8 without and with the object as preconditioner:
iterations and wall time."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from disco4est_amd import Plan, Transfer, mesh as M  # noqa: E402

try:
    from disco4est_amd import Multigrid  # noqa: E402
except ImportError:      # an older checkout: the Python composition alone (the baseline)
    Multigrid = None

dev = torch.device("cuda:0")
CHEBY, EIGS, RATIO, MULT = 3, 10, 30.0, 1.1
REPS, WARM = 30, 5


def plan_of(level, deg, stream):
    m = M.BrickMesh(level, deg)
    J, rst = m.geometry(None); sides = m.build_sides(None)
    p = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, 0, stream=stream)
    p.set_geometry(J, rst)
    p.set_faces(sides, 10.0, 0)
    return m, p


def p_transfer(n_el, degH, degh, stream):
    dh = np.ascontiguousarray(np.stack([np.full(n_el, degh, np.int32)] + [np.zeros(n_el, np.int32)] * 7, axis=1).reshape(-1))
    return Transfer(np.zeros(n_el, np.int32), np.full(n_el, degH, np.int32), dh, stream=stream)


def timed(fn, stream):
    """event-timed repetitions on `stream`: (median, min, max) in us"""
    with torch.cuda.stream(stream):
        for _ in range(WARM):
            fn()
        stream.synchronize()
        ts = []
        for _ in range(REPS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
    return {"median_us": statistics.median(ts), "min_us": min(ts), "max_us": max(ts), "reps": REPS}


def hierarchy(kind, stream):
    """plans coarsest first and the transfers between them"""
    if kind == "two_level_h":
        mc, pc = plan_of(3, 7, stream)
        mf, pf = plan_of(4, 7, stream)
        T = Transfer(np.ones(mc.n_elements, np.int32), np.full(mc.n_elements, 7, np.int32), np.full(8 * mc.n_elements, 7, np.int32), stream=stream)
        return [mc, mf], [pc, pf], [T]
    m0, p0 = plan_of(4, 1, stream)
    m1, p1 = plan_of(4, 3, stream)
    m2, p2 = plan_of(4, 7, stream)
    n = m2.n_elements
    return [m0, m1, m2], [p0, p1, p2], [p_transfer(n, 1, 3, stream), p_transfer(n, 3, 7, stream)]


def python_cycle(plans, transfers, eigs, vec):
    """the cycle composed from Python calls as bench.py's two_grid() does (cheby_iterate on fixed windows, restrict, zero_, prolong, add_),
    generalised to any depth; the bottom level is 3 Chebyshev iterations (two_grid's coarse solve)"""
    top = len(plans) - 1

    def cycle():
        for l in range(top, 0, -1):
            u, rhs, Au, r = vec[l]
            if l != top:
                u.zero_()
            plans[l].cheby_iterate(u, rhs, Au, r, CHEBY, eigs[l] / RATIO, eigs[l], 1)
            transfers[l - 1].restrict(r, vec[l - 1][1])
        u, rhs, Au, r = vec[0]
        u.zero_()
        plans[0].cheby_iterate(u, rhs, Au, r, CHEBY, eigs[0] / RATIO, eigs[0], 0)
        for l in range(0, top):
            ef = vec[l + 1][3]
            transfers[l].prolong(vec[l][0], ef)
            vec[l + 1][0].add_(ef)
            u, rhs, Au, r = vec[l + 1]
            plans[l + 1].cheby_iterate(u, rhs, Au, r, CHEBY, eigs[l + 1] / RATIO, eigs[l + 1], 0 if l + 1 == top else 1)
    return cycle


def main():
    out = {"settings": {"cheby_imax": CHEBY, "cheby_eigs_cg_imax": EIGS, "ratio": RATIO, "multiplier": MULT},
           "has_multigrid_object": Multigrid is not None}
    stream = torch.cuda.Stream()
    for kind in ("two_level_h", "three_level_p"):
        with torch.cuda.stream(stream):
            meshes, plans, transfers = hierarchy(kind, stream)
            top = len(plans) - 1
            rhs = torch.from_numpy(M.splitmix64_uniform(5, meshes[top].local_nodes) - 0.5).to(dev)
            ent = {"nodes": [m.local_nodes for m in meshes], "face_paths": [p.face_path() for p in plans]}
            # bounds per level: cg_eigs from zero on a random right-hand side (what the object's first cycle does on the top level)
            eigs = []
            for m, p in zip(meshes, plans):
                b = torch.from_numpy(M.splitmix64_uniform(7, m.local_nodes) - 0.5).to(dev)
                x = torch.zeros_like(b); Ax = torch.empty_like(b)
                eigs.append(MULT * p.cg_eigs(x, b, Ax, EIGS, 1)[0])
            ent["eigs"] = eigs
            vec = [[torch.zeros(m.local_nodes, dtype=torch.float64, device=dev) for _ in range(4)] for m in meshes]
            vec[top][1].copy_(rhs)
            stream.synchronize()
        ent["python_composition"] = timed(python_cycle(plans, transfers, eigs, vec), stream)
        if Multigrid is not None:
            # bottom "cheby": the reference's Chebyshev bottom solver, which runs its cg_eigs (EIGS iterations, one host read) in EVERY
            # cycle -- more work than the Python composition's bottom level; bottom "cg3": 3 CG iterations (4 applies, two reads of the
            # stop flag), the closest the reference's bottom solvers come to two_grid()'s 3 fixed-window iterations
            for name, env, bottom in (("c_vcycle_fused", None, "cheby"), ("c_vcycle_unfused", "1", "cheby"),
                                      ("c_vcycle_fused_bottom_cg3", None, "cg3"), ("c_vcycle_unfused_bottom_cg3", "1", "cg3")):
                if env:
                    os.environ["D4EST_HIP_MG_UNFUSED_CORRECTION"] = env
                else:
                    os.environ.pop("D4EST_HIP_MG_UNFUSED_CORRECTION", None)
                with torch.cuda.stream(stream):
                    mg = Multigrid(plans, transfers)
                    assert mg.set_smoother_cheby(CHEBY, EIGS, RATIO, MULT, 1, 1, 1, 0) == 0
                    if bottom == "cheby":
                        mg.set_bottom_solver_cheby(CHEBY, EIGS, RATIO, MULT, 1)
                    else:
                        mg.set_bottom_solver_cg(3, 0.0, 0.0)
                    u = torch.zeros_like(rhs); Au = torch.empty_like(rhs)
                    r2_first = mg.vcycle(u, rhs, Au, 0)            # untimed: takes the bounds
                    ent[name] = timed(lambda: mg.lib.d4est_hip_multigrid_vcycle(mg.handle, u.data_ptr(), rhs.data_ptr(), Au.data_ptr(), 1), stream)
                    ent[name]["r2_after_first_cycle"] = r2_first
                    ent[name]["eigs"] = mg.info()[0].tolist()
                    mg.destroy()
            os.environ.pop("D4EST_HIP_MG_UNFUSED_CORRECTION", None)
            if kind == "two_level_h":
                with torch.cuda.stream(stream):
                    mg = Multigrid(plans, transfers)
                    assert mg.set_smoother_cheby(CHEBY, EIGS, RATIO, MULT, 0, 0, 1, 0) == 0
                    mg.set_bottom_solver_cg(100, 0.0, 1e-10)
                    mg.set_pc(1, 0.0, 0.0)
                    fcg = {}
                    for label, pc in (("pc_none", None), ("pc_multigrid", mg)):
                        u = torch.zeros_like(rhs); Au = torch.empty_like(rhs)
                        plans[top].fcg_solve(u, rhs, Au, 2, 0.0, 0.0, pc=pc)      # warm-up
                        u.zero_()
                        stream.synchronize()
                        t0 = time.perf_counter()
                        it, hist = plans[top].fcg_solve(u, rhs, Au, 3000, 0.0, 1e-8, pc=pc)
                        stream.synchronize()
                        fcg[label] = {"iterations": it, "wall_ms": (time.perf_counter() - t0) * 1e3, "r0": float(hist[0]), "r_last": float(hist[-1])}
                    ent["fcg_rtol_1e-8"] = fcg
                    mg.destroy()
        out[kind] = ent
        for t in transfers:
            t.destroy()
        for p in plans:
            p.destroy()
    print(json.dumps(out, indent=1))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
