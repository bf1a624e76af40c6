"""Time per inner step of the batched GMRES(mr) subdomain solver on the mesh and options of bench.py's Schwarz secondary (the affine
brick of --level / --deg, overlap 2, penalty prefactor 10), split into the operator apply and the new kernels, next to the existing CG
sweep on the same handle (reported whole: see the comment at its line).

What each number is.  "iterate" is one d4est_hip_schwarz_iterate between device events, tolerances off (1e-300), so GMRES makes
cycles x mr inner steps and CG `--cg-iter` sweeps.  "apply" is d4est_hip_schwarz_apply_over_subdomains alone, timed the same way on the
restricted residual.  "new kernels per step" is (iterate - applies x apply - correction) / inner steps: the start, Arnoldi and update
kernels together, the start and update kernels spread over their cycle's steps; "correction" is add_correction alone.  Every figure is
the median of --reps windows after --warm warm-up calls, with the smallest and largest window next to it.

    python tools/time_schwarz_gmres.py [--level 4] [--deg 7] [--mr 2 4 8] [--cycles 2] [--reps 7]
"""
import argparse
import json
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from disco4est_amd import mesh as M  # noqa: E402
from disco4est_amd.schwarz import Schwarz  # noqa: E402


def windows(fn, reps, warm, stream):
    """median, min, max (ms) of `reps` timed calls of fn after `warm` untimed ones"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out)), float(min(out)), float(max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--level", type=int, default=4)
    ap.add_argument("--deg", type=int, default=7)
    ap.add_argument("--overlap", type=int, default=2)
    ap.add_argument("--mr", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--cycles", type=int, default=2)
    ap.add_argument("--cg-iter", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_schwarz_gmres.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    try:
        commit = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL, text=True).strip()
    except Exception:
        commit = "unknown"
    m = M.BrickMesh(a.level, a.deg)
    J, rst = m.geometry(None)
    sides = m.build_sides(None)
    sz = Schwarz(m, sides, J, rst, a.overlap, a.cg_iter, 1e-300, 1e-300, 10.0, 0)
    md = sz.metadata
    res = {"commit": commit, "level": a.level, "deg": a.deg, "overlap": a.overlap, "subdomains": md.num_subdomains,
           "subdomain_elements": md.num_elements, "field_over_subdomains_MB": sz.nodal_size * 8 / 1e6,
           "restricted_MB": md.restricted_nodal_size * 8 / 1e6, "face_path": sz.plan.face_path(), "condensed_copies": sz.condensed_copies()}
    print(json.dumps(res))
    r = torch.from_numpy(M.splitmix64_uniform(1, m.local_nodes) - 0.5).to(dev)
    u = torch.zeros_like(r)
    x = torch.empty(sz.nodal_size, dtype=torch.float64, device=dev)
    y = torch.empty_like(x)
    sz.restrict_field(r, x)
    apply_ms = windows(lambda: sz.apply_over_subdomains(x, y), a.reps, a.warm, stream)
    corr_ms = windows(lambda: sz.add_correction(x, u), a.reps, a.warm, stream)
    res["apply_over_subdomains_ms"] = apply_ms
    res["add_correction_ms"] = corr_ms
    print("apply_over_subdomains: %.3f ms (min %.3f, max %.3f); add_correction: %.3f ms" % (apply_ms + corr_ms[:1]))
    del y
    sweeps = []
    cg_ms = windows(lambda: sweeps.append(sz.iterate(u, r)), a.reps, a.warm, stream)
    per = (cg_ms[0] - corr_ms[0]) / sweeps[-1]
    # (a CG sweep applies the operator WITHOUT the mask pass of apply_over_subdomains -- its vectors are only read on the restricted
    # nodes -- so its two parts cannot be told apart with the apply figure above; the sweep is reported whole)
    res["cg"] = {"iterate_ms": cg_ms, "sweeps": sweeps[-1], "ms_per_sweep": per}
    print("CG: %d sweeps, iterate %.3f ms (min %.3f, max %.3f) = %.3f ms per sweep (operator without the mask pass + the CG kernel)"
          % ((sweeps[-1],) + cg_ms + (per,)))
    res["gmres"] = {}
    for mr in a.mr:
        sz.set_subdomain_solver("gmres", mr)
        sz.subdomain_iter = a.cycles
        applies = []
        g_ms = windows(lambda: applies.append(sz.iterate(u, r)), a.reps, a.warm, stream)
        steps = mr * a.cycles
        it, _ = sz.info()
        assert int(it.min()) == steps == int(it.max()), (it.min(), it.max(), steps)
        new_ms = (g_ms[0] - applies[-1] * apply_ms[0] - corr_ms[0]) / steps
        res["gmres"][mr] = {"iterate_ms": g_ms, "inner_steps": steps, "applies": applies[-1], "ms_per_inner_step": (g_ms[0] - corr_ms[0]) / steps,
                            "apply_ms_per_step": applies[-1] * apply_ms[0] / steps, "new_kernels_ms_per_step": new_ms,
                            "workspace_MB": sz.subdomain_solver()[2] / 1e6}
        print("GMRES(%d) x %d cycles: iterate %.3f ms (min %.3f, max %.3f), %d applies; per inner step %.3f ms = apply %.3f + new kernels %.3f; "
              "workspace %.0f MB" % ((mr, a.cycles) + g_ms + (applies[-1], (g_ms[0] - corr_ms[0]) / steps, applies[-1] * apply_ms[0] / steps, new_ms,
                                     sz.subdomain_solver()[2] / 1e6)))
        sz.set_subdomain_solver("cg")
        sz.subdomain_iter = a.cg_iter
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    sz.destroy()


if __name__ == "__main__":
    main()
