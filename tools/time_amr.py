"""Times the device hp-AMR step on the GPU (HIP events, warmed up, variants alternating round by round):
  fused        Amr.interpolate_field, one kernel, no auxiliary vector
  two_stage    the same call with D4EST_HIP_AMR_TWO_STAGE=1 (two prolongations inside the object)
  two_prolong  two Transfer.prolong calls on the same logs (what a caller could do before)
  stats_mark   Amr.stats + Amr.mark_smooth_pred on the device
  host_sort    the device-to-host copy of eta2 plus numpy's sort and mean (what a host-side marker needs first)
on a level-L brick (8^L elements, degrees 3 .. 7 cycling, every 8th element h-refined, every 64th auxiliary element balance-split).
Prints one JSON line per level.  Usage: python tools/time_amr.py [--levels 4 5] [--reps 200] [--rounds 5] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def grids(level):
    n = 8 ** level
    e = np.arange(n)
    deg = (3 + e % 5).astype(np.int32)
    log = np.where(e % 8 == 7, -deg, deg).astype(np.int32)
    aux_deg = np.repeat(deg, np.where(log < 0, 8, 1))
    bal = np.where(np.arange(aux_deg.size) % 64 == 63, -aux_deg, aux_deg).astype(np.int32)
    # the same two loops as Transfer item lists
    h1 = (log < 0).astype(np.int32)
    dh1 = np.zeros((n, 8), np.int32)
    dh1[:, 0] = deg
    dh1[log < 0, :] = deg[log < 0, None]
    h2 = (bal < 0).astype(np.int32)
    dh2 = np.zeros((aux_deg.size, 8), np.int32)
    dh2[:, 0] = aux_deg
    dh2[bal < 0, :] = aux_deg[bal < 0, None]
    return deg, log, bal, (h1, deg, dh1.reshape(-1)), (h2, aux_deg.astype(np.int32), dh2.reshape(-1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", type=int, nargs="+", default=[4, 5])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from disco4est_amd import Amr, Transfer
    from disco4est_amd import mesh as M
    if not torch.cuda.is_available():
        sys.exit("time_amr: no GPU visible; timings are taken on the device only")
    gpu = torch.device("cuda:0")
    lines = []
    for level in a.levels:
        deg, log, bal, s1, s2 = grids(level)
        os.environ.pop("D4EST_HIP_AMR_TWO_STAGE", None)
        fused = Amr(deg, 8, 1.0)
        os.environ["D4EST_HIP_AMR_TWO_STAGE"] = "1"
        staged = Amr(deg, 8, 1.0)
        os.environ.pop("D4EST_HIP_AMR_TWO_STAGE", None)
        for o in (fused, staged):
            o.set_refinement_log(log)
            o.set_balance(bal)
        t1, t2 = Transfer(*s1), Transfer(*s2)
        assert (t1.coarse_nodes, t1.fine_nodes, t2.fine_nodes) == (fused.local_nodes, t2.coarse_nodes, fused.new_local_nodes)
        x = torch.from_numpy(M.splitmix64_uniform(5, fused.local_nodes) - 0.5).to(gpu)
        aux = torch.empty(t1.fine_nodes, dtype=torch.float64, device=gpu)
        outs = {k: torch.empty(fused.new_local_nodes, dtype=torch.float64, device=gpu) for k in ("fused", "two_stage", "two_prolong")}
        eta2 = torch.from_numpy(2.0 * M.splitmix64_uniform(9, deg.size)).to(gpu)
        stats = torch.empty(4, dtype=torch.float64, device=gpu)
        marker = Amr(deg, 8, 1.0)

        def two_prolong():
            t1.prolong(x, aux)
            t2.prolong(aux, outs["two_prolong"])

        def stats_mark():
            marker.stats(eta2, 5, stats)
            marker.mark_smooth_pred(eta2, stats[1:2], 0.5, 0.25, 0.1, 1.0)

        def host_sort():
            h = eta2.cpu().numpy()
            np.sort(h)
            h.mean()

        variants = {"fused": lambda: fused.interpolate_field(x, outs["fused"]),
                    "two_stage": lambda: staged.interpolate_field(x, outs["two_stage"]),
                    "two_prolong": two_prolong, "stats_mark": stats_mark, "host_sort": host_sort}
        for f in variants.values():
            for _ in range(20):
                f()
        torch.cuda.synchronize()
        scale = float(outs["two_prolong"].abs().max())
        diff = {k: float((outs[k] - outs["two_prolong"]).abs().max()) / scale for k in ("fused", "two_stage")}
        us = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, f in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    f()
                e1.record()
                e1.synchronize()
                us[k].append(1e3 * e0.elapsed_time(e1) / a.reps)
        nb_old, nb_aux, nb_new = 8 * fused.local_nodes, 8 * t1.fine_nodes, 8 * fused.new_local_nodes
        line = {"level": level, "n_old": int(deg.size), "n_aux": int(bal.size), "n_new": fused.new_n_elements,
                "bytes_fused": nb_old + nb_new, "bytes_two_stage": nb_old + 2 * nb_aux + nb_new,
                "us_median": {k: float(np.median(v)) for k, v in us.items()}, "us_min": {k: float(np.min(v)) for k, v in us.items()},
                "us_max": {k: float(np.max(v)) for k, v in us.items()}, "max_rel_diff_vs_two_prolong": diff,
                "describe": fused.describe(), "reps": a.reps, "rounds": a.rounds}
        line["GBps_fused"] = line["bytes_fused"] / line["us_median"]["fused"] * 1e-3
        print(json.dumps(line), flush=True)
        lines.append(line)
        for o in (fused, staged, marker, t1, t2):
            o.destroy()
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
