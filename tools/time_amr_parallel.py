"""Times the hp-AMR step on several ranks on ONE GPU: two (--world) virtual ranks, threads in lock-step on the null stream with the
in-process transport of tests/test_schwarz_sharded_gpu.py (a barrier per round, device-to-device copies for the messages), so the
numbers are the library's kernels, launches and hook calls plus that transport -- not a network.
  stats_global       Amr.stats_global (8 digit passes, 8 allreduce calls), per call
  stats_one_rank     Amr.stats on the whole list on one rank (device radix sort), per call, for scale
  repartition_field  Amr.repartition from the partition by elements to the one by nodes (and back on the next repetition) plus one
                     nodal field, per call pair
on --elements elements (default 32768) of degrees 1 .. 4 cycling.  Wall-clock around a synchronised device, median over --rounds.
Prints one JSON line.  Usage: python tools/time_amr_parallel.py [--elements 32768] [--world 2] [--reps 20] [--rounds 5] [--out FILE]"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=int, default=32768)
    ap.add_argument("--world", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from disco4est_amd import Amr, mesh as M, parallel as P
    from tests.test_schwarz_sharded_gpu import _LockstepTransport, _Mailbox, _run_lockstep
    if not torch.cuda.is_available():
        sys.exit("time_amr_parallel: no GPU visible; timings are taken on the device only")
    gpu = torch.device("cuda:0")
    n, world = a.elements, a.world
    # degrees 1 .. 4 in blocks, so that the partition by nodes differs from the one by elements
    deg = (1 + (np.arange(n) * 4) // n).astype(np.int32)
    off = np.concatenate([[0], np.cumsum((deg.astype(np.int64) + 1) ** 3)])
    by_el = np.asarray([(n * r) // world for r in range(world + 1)], dtype=np.int64)
    by_nodes = P.first_of(P.partition_by_dofs(deg, world))
    moved = int(np.abs(by_nodes - by_el).max())
    eta2 = 2.0 * M.splitmix64_uniform(9, n)
    field = M.splitmix64_uniform(10, int(off[-1])) - 0.5

    mb = _Mailbox()
    barrier = threading.Barrier(world, timeout=120)
    transports = [_LockstepTransport(r, world, mb, barrier) for r in range(world)]
    amrs = [Amr(deg[by_el[r]:by_el[r + 1]], 8, 1.0) for r in range(world)]
    for am, tr in zip(amrs, transports):
        P.attach_amr(am, tr, gpu)
    d_eta = [torch.from_numpy(eta2[by_el[r]:by_el[r + 1]]).to(gpu) for r in range(world)]
    stats = [torch.empty(4, dtype=torch.float64, device=gpu) for _ in range(world)]
    f_el = [torch.from_numpy(field[off[by_el[r]]:off[by_el[r + 1]]]).to(gpu) for r in range(world)]
    f_nd = [torch.empty(int(off[by_nodes[r + 1]] - off[by_nodes[r]]), dtype=torch.float64, device=gpu) for r in range(world)]
    whole = Amr(deg, 8, 1.0)
    d_eta_whole = torch.from_numpy(eta2).to(gpu)
    stats_whole = torch.empty(4, dtype=torch.float64, device=gpu)

    def timed(body, reps):
        """seconds per repetition of body(rank) run by every rank in lock-step"""
        def run(r):
            for _ in range(reps):
                body(r)
            torch.cuda.synchronize()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _run_lockstep(world, barrier, gpu, run)
        return (time.perf_counter() - t0) / reps

    def stats_body(r):
        amrs[r].stats_global(d_eta[r], 5, stats[r])

    def repart_body(r):          # there and back: the object is at the partition by elements again
        amrs[r].repartition(by_el, by_nodes)
        amrs[r].repartition_field(f_el[r], f_nd[r])
        amrs[r].repartition(by_nodes, by_el)
        amrs[r].repartition_field(f_nd[r], f_el[r])

    timed(stats_body, 3)
    timed(repart_body, 1)
    us = {"stats_global": [], "stats_one_rank": [], "repartition_field": []}
    for _ in range(a.rounds):
        us["stats_global"].append(1e6 * timed(stats_body, a.reps))
        mb.box.clear()
        us["repartition_field"].append(1e6 * timed(repart_body, max(a.reps // 4, 1)) / 2)
        mb.box.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            whole.stats(d_eta_whole, 5, stats_whole)
        torch.cuda.synchronize()
        us["stats_one_rank"].append(1e6 * (time.perf_counter() - t0) / a.reps)
    back = np.concatenate([t.cpu().numpy() for t in f_el])
    line = {"elements": n, "world": world, "nodes": int(off[-1]), "elements_moved": moved,
            "field_round_trip_is_exact": bool(np.array_equal(back, field)),
            "global_max_and_percentile": [float(v) for v in stats[0].cpu().numpy()[2:]],
            "one_rank_max": float(stats_whole.cpu().numpy()[2]),
            "us_median": {k: float(np.median(v)) for k, v in us.items()}, "us_min": {k: float(np.min(v)) for k, v in us.items()},
            "us_max": {k: float(np.max(v)) for k, v in us.items()}, "reps": a.reps, "rounds": a.rounds}
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    for o in amrs + [whole]:
        o.destroy()


if __name__ == "__main__":
    main()
