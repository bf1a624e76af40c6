"""Timing of the device V-cycle with the Schwarz smoother: tools/time_vcycle_schwarz.py [out.json]

The two-level hierarchy of tools/time_vcycle.py (level-4 brick, p = 7 fine; level-3 brick, p = 7 coarse), one Schwarz iteration before
and after the correction (overlap 2, 12 subdomain CG iterations at rtol 1e-4, the smoother settings of
tests/test_multigrid_gpu.py::test_two_grid_cycle_with_schwarz_smoother), 3 CG iterations on the bottom level.  One
d4est_hip_multigrid_vcycle is timed with events on the plans' stream (warm-up, repetitions: median, min, max)
  * with the residual formed in the subdomain CG's start kernel (D4EST_HIP_SCHWARZ_FUSED_RESIDUAL=1, read when the Schwarz handle is
    created),
  * with the residual kernel followed by the start kernel (D4EST_HIP_SCHWARZ_UNFUSED_RESIDUAL=1),
and against the same cycle composed from Python calls around the public d4est_hip_schwarz_smooth, whose iterates each end with a
blocking read.  Host synchronisations per cycle are counted from the loop structure: an iterate looks at the "still iterating" counter
before sweep 0, 8, 16, ... (every look happens: the loop reaches it unless all subdomains started with a zero residual); the public
iterate adds one read at its end; a bottom CG of 3 iterations reads its stop flag as tools/time_vcycle.py notes."""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from disco4est_amd import Multigrid, Plan, Transfer, mesh as M  # noqa: E402
from disco4est_amd.schwarz import Schwarz  # noqa: E402

dev = torch.device("cuda:0")
OVERLAP, SUB_ITER, SUB_ATOL, SUB_RTOL = 2, 12, 1e-15, 1e-4
REPS, WARM = 10, 2


def level_of(level, deg, stream):
    m = M.BrickMesh(level, deg)
    J, rst = m.geometry(None); sides = m.build_sides(None)
    p = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, 0, stream=stream)
    p.set_geometry(J, rst)
    p.set_faces(sides, 10.0, 0)
    return m, p, (J, rst, sides)


def timed(fn, stream):
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


def main():
    fine_level = int(os.environ.get("TIME_VCYCLE_SCHWARZ_LEVEL", "4"))
    stream = torch.cuda.Stream()
    out = {"settings": {"fine_level": fine_level, "deg": 7, "overlap": OVERLAP, "subdomain_iter": SUB_ITER, "subdomain_atol": SUB_ATOL,
                        "subdomain_rtol": SUB_RTOL, "smoother_iterations": 1, "bottom": "cg, 3 iterations"}}
    with torch.cuda.stream(stream):
        mc, pc, _ = level_of(fine_level - 1, 7, stream)
        mf, pf, (J, rst, sides) = level_of(fine_level, 7, stream)
        T = Transfer(np.ones(mc.n_elements, np.int32), np.full(mc.n_elements, 7, np.int32), np.full(8 * mc.n_elements, 7, np.int32), stream=stream)
        rhs = torch.from_numpy(M.splitmix64_uniform(5, mf.local_nodes) - 0.5).to(dev)
        out["nodes"] = [mc.local_nodes, mf.local_nodes]
        looks = len(range(0, SUB_ITER, 8))
        for name, env in (("c_vcycle_fused_residual", "D4EST_HIP_SCHWARZ_FUSED_RESIDUAL"),
                          ("c_vcycle_unfused_residual", "D4EST_HIP_SCHWARZ_UNFUSED_RESIDUAL")):
            for k in ("D4EST_HIP_SCHWARZ_FUSED_RESIDUAL", "D4EST_HIP_SCHWARZ_UNFUSED_RESIDUAL"):
                os.environ.pop(k, None)
            os.environ[env] = "1"
            sz = Schwarz(mf, sides, J, rst, OVERLAP, SUB_ITER, SUB_ATOL, SUB_RTOL, 10.0, 0, stream=stream)
            os.environ.pop(env, None)
            out["subdomain_field_nodes"] = int(sz.nodal_size)
            out["condensed_copies"] = sz.condensed_copies()
            mg = Multigrid([pc, pf], [T])
            assert mg.set_smoother_schwarz([None, sz], 1) == 0
            mg.set_bottom_solver_cg(3, 0.0, 0.0)
            u = torch.zeros_like(rhs); Au = torch.empty_like(rhs)
            r2_first = mg.vcycle(u, rhs, Au, 0)
            ent = timed(lambda: mg.lib.d4est_hip_multigrid_vcycle(mg.handle, u.data_ptr(), rhs.data_ptr(), Au.data_ptr(), 1), stream)
            ent["r2_after_first_cycle"] = r2_first
            ent["schwarz_host_syncs_per_cycle"] = 2 * looks          # two iterates per cycle, no read at their end
            out[name] = ent
            if name == "c_vcycle_fused_residual":
                # the same cycle from Python around the public smoother entry: each of its iterates ends with a blocking read
                r, ec, rc, Ac, ef = (torch.zeros(n, dtype=torch.float64, device=dev) for n in
                                     (mf.local_nodes, mc.local_nodes, mc.local_nodes, mc.local_nodes, mf.local_nodes))
                v = torch.zeros_like(rhs)

                def python_cycle():
                    sz.smooth(pf, v, rhs, r, 1)
                    T.restrict(r, rc)
                    ec.zero_()
                    pc.cg_solve(ec, rc, Ac, 3, 0.0, 0.0)
                    T.prolong(ec, ef)
                    v.add_(ef)
                    sz.smooth(pf, v, rhs, r, 1)

                ent = timed(python_cycle, stream)
                ent["schwarz_host_syncs_per_cycle"] = 2 * (looks + 1)
                out["python_composition_public_smooth"] = ent
            mg.destroy()
            sz.destroy()
    for x in (T, pc, pf):
        x.destroy()
    print(json.dumps(out, indent=1))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
