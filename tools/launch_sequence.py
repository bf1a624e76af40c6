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


# ---- the volume unit (d4est_hip_volume.hip, the fused term of d4est_hip_nonlinear.hip): `--volume`
# One plan per (degrees, deg_quad - deg, level, straight / curved); on it apply_stiffness_matrix under every listed tuning (key: value),
# then the mass-like applies, du/dr and the fused nonlinear term with tuning key 6 at -1 and 0.  Per apply: last_kernel() and the SHA-256
# of every output.  D4EST_HIP_STIFFNESS_SPLIT_LAUNCH is read once per process: run `--volume mixed` again with it set.
def _grid(**keys):
    """every combination of the values listed per tuning key, as {key: value} dicts"""
    out = [{}]
    for k, vals in keys.items():
        out = [{**t, int(k[1:]): v} for t in out for v in vals]
    return out


WAVE_TUNINGS = [{0: a, 1: b, 7: 0, 16: e} for a, b in ((-1, -1), (0, 0), (1, 0), (0, 1), (1, 1), (0, 2), (0, 3), (0, 11), (0, 12)) for e in (1, 0)]
AFFINE_TOO = [{0: a, 1: b, 16: e} for a, b in ((-1, -1), (0, 0), (0, 11), (0, 12), (0, 3)) for e in (1, 0)]
BIG_TUNINGS = _grid(k4=(-1, 0, 1, 2), k6=(-1, 0), k12=(1, 0))
ALTERNATE = lambda a, b: np.where(np.arange(8) % 2 == 0, a, b).astype(np.int32)   # noqa: E731
VOLUME_CASES = (
    [("wave", deg, inc, 1, WAVE_TUNINGS + AFFINE_TOO) for deg in (1, 3, 5, 6, 7) for inc in (0, 1, 2)]
    + [("multiwave", deg, 0, 1, BIG_TUNINGS) for deg in (8, 9, 11, 12, 13, 14, 15)]
    + [("big", deg, 0, 1, _grid(k4=(-1, 0), k6=(-1, 0))) for deg in (16, 19)]
    + [("generic", 20, 0, 0, [{}])]
    + [("mixed", ALTERNATE(a, b), 0, 1, [{}, {7: 0}, {16: 1}, {1: 12}, {12: 1}, {4: 0}, {6: 0}]) for a, b in ((3, 4), (9, 11), (9, 12), (8, 10), (11, 12), (3, 9))]
    + [("threshold", deg, 0, 5, [{}, {7: 0}, {0: 0}]) for deg in (1, 3)]
)


def run_volume_case(kind, deg, inc, level, tunings, dev, mark):
    for curved in ((True,) if kind == "threshold" else (False, True)):
        m = M.BrickMesh(level, deg, inc)
        J, rst = m.geometry(M.SineMap(0.05) if curved else None)
        plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, m.quad_type)
        plan.set_geometry(J, rst)
        u = torch.from_numpy(m.field()).to(dev)
        fq = torch.from_numpy(1.0 + M.splitmix64_uniform(7, m.local_nodes_quad)).to(dev)
        name = "volume-%s p%s+%d level %d %s" % (kind, deg if np.isscalar(deg) else "%d/%d" % (deg[0], deg[1]), inc, level, "curved" if curved else "straight")
        mark.zero_()
        print("%s: %d elements" % (name, m.n_elements), flush=True)
        for tune in tunings:
            for k in (0, 1, 4, 6, 7, 12, 16):
                plan.set_tuning(k, tune.get(k, -1))
            out = torch.full_like(u, float("nan"))
            plan.apply_stiffness_matrix(u, out)
            print("  stiffness %-44s Au %s  [%s]" % (sorted(tune.items()), sha(out), plan.last_kernel()), flush=True)
        for k in (0, 1, 4, 7, 12, 16):
            plan.set_tuning(k, -1)
        for key6 in (-1, 0):
            plan.set_tuning(6, key6)
            n, q = torch.full_like(u, float("nan")), torch.full_like(fq, float("nan"))
            line = []
            for label, call, res in (("mass", lambda: plan.apply_mass_matrix(u, n), n), ("galerkin", lambda: plan.apply_galerkin_integral(fq, n), n),
                                     ("interpolate", lambda: plan.interpolate(u, q), q), ("weighted", lambda: plan.apply_weighted_mass_matrix(u, fq, n), n),
                                     ("mij", lambda: plan.apply_mij(u, n), n), ("invmij", lambda: plan.apply_invmij(u, n), n)):
                call()
                line.append("%s %s" % (label, sha(res)))
            if inc == 0:   # (the inverse mass needs deg_quad = deg)
                plan.apply_inverse_mass_matrix(u, n)
                line.append("invmass %s" % sha(n))
            d = [torch.full_like(u, float("nan")) for _ in range(3)]
            plan.compute_dudr(u, *d)
            line += ["dudr%d %s" % (i, sha(t)) for i, t in enumerate(d)]
            plan.set_nonlinear_power(fq, None, 3)
            plan.apply_nonlinear_term(u, n)
            line.append("nonlinear(fused %d) %s" % (plan.nonlinear_fused(), sha(n)))
            print("  key 6 = %2d: %s" % (key6, "  ".join(line)), flush=True)
        plan.destroy()


def digest(listing):
    """a listing of this tool, one line per case: the case's heading, how many result lines follow it and the SHA-256 of those lines
    (short enough to commit and to read; two listings agree exactly when their digests do); the distinct last_kernel strings after it"""
    cases, kernels = [], {}
    for line in open(listing):
        if not line.strip() or line.startswith("#"):
            continue
        if not line.startswith(" "):
            cases.append([line.strip(), 0, hashlib.sha256()])
            continue
        cases[-1][1] += 1
        cases[-1][2].update(line.encode())
        if line.rstrip().endswith("]") and "[d4est_hip::" in line:
            name = line[line.index("[d4est_hip::") + 1:line.rstrip().rindex("]")]
            kernels[name] = kernels.get(name, 0) + 1
    for head, n, h in cases:
        print("%s | %d lines | %s" % (head, n, h.hexdigest()))
    print("last_kernel strings:\n%s" % "\n".join("  %4d x %s" % (n, name) for name, n in sorted(kernels.items())))


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
    ap.add_argument("--volume", nargs="*", metavar="KIND", default=None,
                    help="the volume unit's cases instead of the operator's (all kinds, or of wave multiwave big generic mixed threshold)")
    ap.add_argument("--digest", metavar="LISTING", default=None, help="one line per case of a listing this tool printed, instead of running")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    if args.digest:
        return digest(args.digest)
    if not torch.cuda.is_available():
        sys.exit("launch_sequence: no GPU")
    dev = torch.device("cuda:0")
    mark = torch.ones(12345, dtype=torch.float64, device=dev)
    if args.volume is not None:
        for case in VOLUME_CASES:
            if not args.volume or case[0] in args.volume:
                run_volume_case(*case, dev, mark)
        return
    for name, make, tune, extra in CASES:
        if args.only is None or name in args.only:
            run_case(name, make, tune, extra, dev, mark)


if __name__ == "__main__":
    main()
