"""apply_lhs of ONE shard of config 4's mesh class (level-4 brick, every 64th octant refined, p = 3 ... 9 graded), split into 2 and 8
shards by DoF count, with the two-phase kernels (tuning key 14 = 0: what a sharded plan runs by default) against the hybrid operator's
ghost-aware form (key 14 = 2).  One JSON line per (shards, key 14) case.

    python tools/time_hybrid_sharded.py [--level 4] [--shards 2 8] [--reps 200] [--rounds 5]

The shard runs alone ("virtual rank"): its exchange hooks pack and unpack on the device as in a real run, and an in-process stand-in
takes the place of the wire -- `start` copies the packed blocks (the send), `finish` copies the peers' blocks, seeded numbers of the right
length, into the receive buffers.  What is timed is therefore the shard's kernels and hook calls, not a network.  Both forms see the same
ghost data, so their results are compared too (rel-inf; fp64 re-association only).  The two forms alternate, `rounds` times each, after
a warm-up that lets the clocks settle; the median and the extremes of the rounds are reported."""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from disco4est_amd import Plan, mesh as M, parallel as P   # noqa: E402

spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
bench = importlib.util.module_from_spec(spec)
spec.loader.exec_module(bench)


class StandInTransport:
    def __init__(self):
        self.sent, self.peer = {}, {}

    def start(self, send_buf, recv_buf):
        for p, t in send_buf.items():
            if p not in self.sent:
                self.sent[p] = torch.empty_like(t)
            self.sent[p].copy_(t)
        return recv_buf

    def finish(self, recv_buf):
        for p, t in recv_buf.items():
            if p not in self.peer:
                self.peer[p] = torch.from_numpy(M.splitmix64_uniform(1000 + p, t.numel()) - 0.5).to(t.device)
            t.copy_(self.peer[p])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--level", type=int, default=4)
    ap.add_argument("--shards", type=int, nargs="+", default=[2, 8])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_hybrid_sharded: no GPU -- a time is taken on the device or not at all")
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream()
    L = args.level
    refine = np.zeros(8 ** L, dtype=bool)
    refine[::64] = True
    gd = bench.graded_degrees(L)
    deg_global = np.concatenate([np.full(8 if refine[b] else 1, gd[b]) for b in range(8 ** L)]).astype(np.int32)
    for world in args.shards:
        parts = P.partition_by_dofs(deg_global, world)
        rank = world // 2
        first, count = parts[rank]
        m = M.HangingBrickMesh(L, refine, deg_global, first=first, count=count)
        J, rst = m.geometry(None)
        sides = m.build_sides(None)
        x = torch.from_numpy(m.field()).to(dev)
        plans, outs = {}, {}
        for key14 in (0, 2):
            p = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, 0, stream=st)
            p.set_tuning(14, key14)
            p.set_geometry(J, rst)
            p.set_faces(sides, 10.0, 0)
            ex = P.attach(p, m, sides, parts, StandInTransport(), dev)
            y = torch.empty_like(x)
            plans[key14] = (p, ex, y)
        times = {0: [], 2: []}
        for rnd in range(args.rounds):
            for key14 in (0, 2):
                p, _, y = plans[key14]
                times[key14].append(bench.time_region(lambda: p.apply_lhs(x, y), args.reps, st, torch, warm=20 if rnd == 0 else 5))
        for key14 in (0, 2):
            outs[key14] = plans[key14][2].clone()
        diff = float((outs[2] - outs[0]).abs().max() / outs[0].abs().max())
        for key14 in (0, 2):
            t = sorted(times[key14])
            print(json.dumps({"tool": "time_hybrid_sharded", "level": L, "shards": world, "rank": rank, "elements": m.n_elements,
                              "dofs": m.local_nodes, "ghost_trace_doubles": int(plans[key14][0].ghost_trace_size), "key14": key14,
                              "face_path": plans[key14][0].face_path(), "apply_lhs_us_median": round(1e3 * t[len(t) // 2], 2),
                              "apply_lhs_us_min": round(1e3 * t[0], 2), "apply_lhs_us_max": round(1e3 * t[-1], 2),
                              "reps": args.reps, "rounds": args.rounds, "rel_inf_key2_vs_key0": diff}), flush=True)
        for key14 in (0, 2):
            plans[key14][0].destroy()


if __name__ == "__main__":
    main()
