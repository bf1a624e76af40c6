"""One small plan per schedule of apply_operator and per face-kernel family; per case the plan's face_path and the SHA-256 of every
output vector of one apply_lhs, one apply_aij and one 3-iteration cheby_iterate (update fused, and with tuning key 10 = 0).

    python tools/launch_sequence.py [--only NAME ...] > listing.txt

Two builds with the same kernels and the same launches print the same listing, bit for bit: diff the listings of two libraries
(D4EST_HIP_LIBRARY=<other build>) after a change to the host-side scheduling.  Under `rocprofv3 --kernel-trace` (tools/profile_any.sh) the
same run gives the ordered kernel list per case (every case starts with one launch of a marker size, see `mark`); `--compare A.csv B.csv`
holds two such traces against each other: kernel name, grid, workgroup and LDS bytes of every launch in dispatch order, overall and per
queue.  With D4EST_HIP_HYBRID_SERIAL=1 the forked schedules run on one stream and the order is total.

Meshes: level-1 / level-2 bricks from disco4est_amd.mesh, at most a few hundred elements; fields and right-hand sides are seeded.  The
sharded cases run ONE shard alone through its exchange hooks with an in-process stand-in for the wire (as tools/time_hybrid_sharded.py:
seeded peer blocks, not a second live rank), once per rank of two, and without apply_aij (it takes no exchange hooks)."""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from disco4est_amd import Plan, mesh as M, parallel as P   # noqa: E402


class StandInTransport:
    """`finish` fills the receive buffers with seeded numbers of the right length (the peer's blocks)"""

    def start(self, send_buf, recv_buf):
        return recv_buf

    def finish(self, recv_buf):
        for p, t in recv_buf.items():
            t.copy_(torch.from_numpy(M.splitmix64_uniform(1000 + p, t.numel()) - 0.5).to(t.device))


def sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def hanging(level, deg, every=8, **kw):
    refine = np.zeros(8 ** level, dtype=bool)
    refine[::every] = True
    if not np.isscalar(deg):   # degrees per BASE cell -> per element
        deg = np.concatenate([np.full(8 if refine[b] else 1, deg[b]) for b in range(8 ** level)]).astype(np.int32)
    return M.HangingBrickMesh(level, refine, deg, **kw)


def slabs(level, lo, hi):
    """degree lo in the lower half of the brick (x), hi in the upper half"""
    ijk = M.morton_order(level)
    return np.where(ijk[:, 0] < (1 << level) // 2, lo, hi).astype(np.int32)


# name, mesh factory (first, count) -> mesh, tuning keys set before the geometry / faces, extras
CASES = [
    ("p7-direct-whole", lambda f, c: M.BrickMesh(2, 7), {11: 2}, {}),
    ("p7-direct-whole-coeff", lambda f, c: M.BrickMesh(2, 7), {11: 2}, {"coeff": True}),
    ("p3-direct-faces+volume", lambda f, c: M.BrickMesh(2, 3, 1), {11: 2}, {}),
    ("p9-multiwave-whole", lambda f, c: M.BrickMesh(1, 9), {11: 2}, {}),
    ("p17-two-phase-generic", lambda f, c: M.BrickMesh(1, 17), {}, {}),
    ("p7-two-phase", lambda f, c: M.BrickMesh(2, 7), {11: 0}, {}),
    ("p7-two-phase-coeff", lambda f, c: M.BrickMesh(2, 7), {11: 0}, {"coeff": True}),
    ("p7-two-phase-wave", lambda f, c: M.BrickMesh(2, 7), {11: 0, 3: 1}, {}),
    ("p7-two-phase-fork", lambda f, c: M.BrickMesh(2, 7), {11: 0, 5: 1}, {}),
    ("p9-two-phase-tiled", lambda f, c: M.BrickMesh(1, 9), {11: 0}, {}),
    ("p3-key3=0-generic", lambda f, c: M.BrickMesh(2, 3), {11: 0, 3: 0}, {}),
    ("mixed-p3-p4-hybrid", lambda f, c: M.BrickMesh(2, slabs(2, 3, 4)), {14: 1}, {}),
    ("mixed-p3-p9-family-split", lambda f, c: M.BrickMesh(2, slabs(2, 3, 9)), {14: 0}, {}),
    ("mixed-p3-p9-hybrid", lambda f, c: M.BrickMesh(2, slabs(2, 3, 9)), {14: 1}, {}),
    ("hanging-p3-hybrid", lambda f, c: hanging(2, 3), {14: 1}, {}),
    ("hanging-p3-two-phase-split", lambda f, c: hanging(2, 3), {14: 0}, {}),
    ("hanging-mixed-p3-p4-hybrid", lambda f, c: hanging(2, slabs(2, 3, 4)), {14: 1}, {}),
    ("hanging-p9-split-tiled", lambda f, c: hanging(1, 9, every=4), {14: 0}, {}),
    ("hanging-p9-hybrid", lambda f, c: hanging(1, 9, every=4), {14: 1}, {}),
    ("hanging-mixed-p3-p9", lambda f, c: hanging(2, slabs(2, 3, 9)), {}, {}),
    ("hanging-p3-key13=0-hp-tiled", lambda f, c: hanging(2, 3), {13: 0}, {}),
    ("hanging-p3-key3=0-hp-generic", lambda f, c: hanging(2, 3), {3: 0}, {}),
    ("shard-p7-direct-ghost-split", lambda f, c: M.BrickMesh(2, 7, first=f, count=c), {11: 2}, {"world": 2}),
    ("shard-p7-two-phase-ghosts", lambda f, c: M.BrickMesh(2, 7, first=f, count=c), {11: 0}, {"world": 2}),
    ("shard-hanging-p3-hybrid-key14=2", lambda f, c: hanging(2, 3, first=f, count=c), {14: 2}, {"world": 2}),
    ("shard-mixed-p3-p4-hybrid-key14=2", lambda f, c: M.BrickMesh(2, slabs(2, 3, 4), first=f, count=c), {14: 2}, {"world": 2}),
    ("p3-subdomain-plan-key8=1", lambda f, c: M.BrickMesh(2, 3), {11: 0, 8: 1}, {}),
]


def run_case(name, make, tune, extra, dev, mark):
    world = extra.get("world", 1)
    whole = make(0, None)
    parts = P.partition_by_dofs(whole.deg, world) if world > 1 else [(0, None)]
    for rank, (first, count) in enumerate(parts):
        m = make(first, count)
        J, rst = m.geometry(None)
        sides = m.build_sides(None)
        plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, 0)
        for k, v in tune.items():
            plan.set_tuning(k, v)
        plan.set_geometry(J, rst)
        plan.set_faces(sides, 10.0, 0)
        ex = P.attach(plan, m, sides, parts, StandInTransport(), dev) if world > 1 else None
        if extra.get("coeff"):
            plan.set_lhs_coefficient(torch.from_numpy(1.0 + M.splitmix64_uniform(5, m.local_nodes_quad)).to(dev))
        u = torch.from_numpy(m.field()).to(dev)
        rhs = torch.from_numpy(M.splitmix64_uniform(11, m.local_nodes) - 0.5).to(dev)
        tag = "%s%s" % (name, " rank %d/%d" % (rank, world) if world > 1 else "")
        mark.zero_()   # the marker launch of this case in a kernel trace
        print("%s: %d elements, face_path = %s" % (tag, m.n_elements, plan.face_path()), flush=True)
        out = torch.full_like(u, float("nan"))
        plan.apply_lhs(u, out)
        print("  apply_lhs   Au %s" % sha(out), flush=True)
        if world == 1:
            out.fill_(float("nan"))
            plan.apply_aij(u, out)
            print("  apply_aij   Au %s" % sha(out), flush=True)
        for key10 in (-1, 0):
            plan.set_tuning(10, key10)
            x, Au, r = u.clone(), torch.zeros_like(u), torch.zeros_like(u)
            plan.cheby_iterate(x, rhs, Au, r, 3, 2.0, 60.0, 1)
            print("  cheby(key 10 = %2d) u %s Au %s r %s  [%s]" % (key10, sha(x), sha(Au), sha(r), plan.last_kernel()), flush=True)
        plan.destroy()
        del ex


def launches(trace_csv):
    """the library's launches in the kernel trace of one run (rocprofv3 --kernel-trace --output-format csv), in dispatch order: (queue,
    name, grid, workgroup, LDS bytes); queues are numbered by first appearance, their ids differ from process to process.  torch's own
    kernels and the runtime's copy kernels are left out: whether a copy runs as a kernel or on a DMA engine varies from run to run"""
    import csv
    rows = sorted((r for r in csv.DictReader(open(trace_csv)) if "d4est_hip" in r["Kernel_Name"]), key=lambda r: int(r["Dispatch_Id"]))
    queue = {}
    return [(queue.setdefault(r["Queue_Id"], len(queue)), r["Kernel_Name"], tuple(int(r["Grid_Size_" + c]) for c in "XYZ"),
             tuple(int(r["Workgroup_Size_" + c]) for c in "XYZ"), int(r["LDS_Block_Size"])) for r in rows]


def compare(a_csv, b_csv):
    """exit status 0 when both traces hold the same launches in the same order, overall and on every queue"""
    a, b = launches(a_csv), launches(b_csv)
    print("%d / %d launches of %d / %d kernels on %d / %d queues" %
          (len(a), len(b), len({x[1] for x in a}), len({x[1] for x in b}), len({x[0] for x in a}), len({x[0] for x in b})))
    same_total = [x[1:] for x in a] == [x[1:] for x in b]
    same_queue = all([x for x in a if x[0] == q] == [x for x in b if x[0] == q] for q in {x[0] for x in a + b})
    print("dispatch order, all queues together: %s; per queue: %s" % ("identical" if same_total else "DIFFERENT", "identical" if same_queue else "DIFFERENT"))
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            print("first difference at launch %d:\n  %s\n  %s" % (i, x, y))
            break
    return 0 if same_total and same_queue and len(a) == len(b) else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--compare", nargs=2, metavar="TRACE_CSV", default=None, help="compare two kernel traces of this tool instead of running")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    if not torch.cuda.is_available():
        sys.exit("launch_sequence: no GPU")
    dev = torch.device("cuda:0")
    mark = torch.ones(12345, dtype=torch.float64, device=dev)
    for name, make, tune, extra in CASES:
        if args.only is None or name in args.only:
            run_case(name, make, tune, extra, dev, mark)


if __name__ == "__main__":
    main()
