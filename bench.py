#!/usr/bin/env python
"""bench.py -- GDoF/s of the matrix-free 3-D DG stiffness apply (Au = K u), p = 7, fp64.

Contract (see the task statement):  python bench.py --gpus N --steps K --warmup W
For N > 1 the driver launches one rank per GPU with torch.distributed.run (RANK / LOCAL_RANK / WORLD_SIZE in the
environment); started by hand with --gpus N and no WORLD_SIZE, bench.py launches that command itself and relays its
output.  The volume stiffness apply is element-independent, so ranks own disjoint Morton shards and the HEADLINE data
path has NO collective (weak scaling: every rank owns one config-2 brick's worth of elements).  A step = one stiffness
apply over the rank's whole shard, inputs resident in HBM.  With --full on N > 1 ranks the line also carries, under "secondary",
the full operator and the Chebyshev iteration on config 2 SPLIT N ways (strong scaling) with the face-trace exchange
over RCCL in C (csrc/d4est_hip_comm.hip) -- the replacement of d4est_ghost_data_exchange.

A plain run does only what the headline needs: set-up, W warm-up steps, K timed steps, the result line.  --full adds the parity
gate against the CPU oracle, the "secondary" numbers and the CPU baseline.  --dump-outputs DIR writes the last timed step's A u
(float64 .npy; the inputs are seeded, so two builds can be compared output for output).

Rank 0 prints ONE JSON line on stdout.  Everything else goes to stderr.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak, /opt/skills/guides/MI355X_MICROARCH.md "Chip-level parameters"


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def algorithmic_bytes_per_dof(N, NQ):
    """read u (8) + write Au (8) + 6 symmetric metric entries per quadrature node."""
    return 16.0 + 48.0 * (NQ / N) ** 3


def cpu_baseline(mesh, J, rst, u, budget_s=12.0):
    """Times the CPU restatement of the reference algorithm (oracle, kind "port") on the host
    cores of this box, on a bounded sample of the same workload."""
    from tests import oracle_lib
    oracle = oracle_lib.load(native=True)
    cores = min(os.cpu_count() or 1, 16)  # a 1-GPU box's CPU share is 16 cores
    try:
        cores = min(cores, len(os.sched_getaffinity(0)))
    except Exception:
        pass
    # sample: leading elements of the same mesh (same p, same geometry layout); sized for ~budget_s
    from disco4est_amd import mesh as M
    probe = M.BrickMesh(mesh.level, int(mesh.deg[0]), quad_type=mesh.quad_type, first=0, count=min(mesh.n_elements, 8 * cores))
    Jp, rstp = probe.geometry(None)
    up = np.ascontiguousarray(u[:probe.local_nodes])
    t0 = time.perf_counter()
    oracle.apply_stiffness(probe, Jp, rstp, up, nthreads=cores)
    t_probe = max(time.perf_counter() - t0, 1e-6)
    per_elem = t_probe / probe.n_elements
    n_sample = int(max(cores, min(mesh.n_elements, budget_s / 3.0 / per_elem)))
    sample = M.BrickMesh(mesh.level, int(mesh.deg[0]), quad_type=mesh.quad_type, first=0, count=n_sample)
    Js, rsts = sample.geometry(None)
    us = np.ascontiguousarray(u[:sample.local_nodes])
    oracle.apply_stiffness(sample, Js, rsts, us, nthreads=cores)  # warm-up
    reps, t_acc = 0, 0.0
    while reps < 2 or (t_acc < budget_s * 0.6 and reps < 50):
        t0 = time.perf_counter()
        oracle.apply_stiffness(sample, Js, rsts, us, nthreads=cores)
        t_acc += time.perf_counter() - t0
        reps += 1
    gdofs = sample.local_nodes * reps / t_acc / 1e9
    # one core, on a smaller slice (compare with the survey-time 3.5 MDoF/s per core of the real reference)
    one = M.BrickMesh(mesh.level, int(mesh.deg[0]), quad_type=mesh.quad_type, first=0, count=max(1, min(n_sample, int(2.0 / per_elem / cores))))
    J1, rst1 = one.geometry(None)
    u1 = np.ascontiguousarray(u[:one.local_nodes])
    oracle.apply_stiffness(one, J1, rst1, u1, nthreads=1)
    t0 = time.perf_counter()
    oracle.apply_stiffness(one, J1, rst1, u1, nthreads=1)
    gdofs_1 = one.local_nodes / max(time.perf_counter() - t0, 1e-9) / 1e9
    return {
        "value": gdofs, "unit": "GDoF/s", "cores": cores, "kind": "port", "value_1_core": gdofs_1,
        "sample": "%d of %d elements (p=%d) of the same brick, %d reps, %d OpenMP threads over elements; "
                  "oracle/d4est_oracle.c (27-pass reference algorithm, naive row-major dgemm, gcc -O3 -march=native)"
                  % (sample.n_elements, mesh.n_elements, int(mesh.deg[0]), reps, cores),
    }


DUMP_BUDGET_BYTES = 64 << 20   # --dump-outputs: at most this much in all


def dump_output(path, name, y, budget):
    """--dump-outputs: the array the timed path hands its caller, as float64 DIR/<name>.npy.  Above the budget a fixed, seeded sample of
    it instead, with its sorted indices in DIR/<name>_sample_index.npy (values and indices take half the budget each)."""
    os.makedirs(path, exist_ok=True)
    a = y.detach().cpu().numpy().astype(np.float64, copy=False).reshape(-1)
    if a.nbytes > budget:
        idx = np.sort(np.random.default_rng(20240607).choice(a.size, budget // 16, replace=False))
        np.save(os.path.join(path, name + "_sample_index.npy"), idx.astype(np.float64))
        a = a[idx]
    np.save(os.path.join(path, name + ".npy"), a)
    log("dumped %s (%d values) to %s" % (name, a.size, path))


# bytes per DoF one iteration of the 5-iteration fused Chebyshev loop moves on top of full_operator_bytes_per_dof: + rhs 8 + p read 8 and
# written 8 + the new iterate 8, - 8 for A u, which is stored in the last iteration only, + (last iteration: A u 8 + r 8; the copy back
# of the iterate after an odd count 16; the memset of p 8) / 5 = 8  (d4est_hip_solver.hip: cheby_iterate_body)
CHEBY_VECTOR_BYTES_PER_DOF = 32.0


def time_region(fn, reps, stream, torch, warm=10, settle_s=0.06):
    """average milliseconds per call, HIP events on the launch stream.  warm: untimed calls first; then more untimed batches until
    settle_s seconds of back-to-back work have passed -- the chip's clocks take tens of milliseconds of sustained load to settle
    (p = 15, 8192 elements: 588 us on the first call after an idle gap, 470 us from the 35th on; level 4, p = 11 apply_aij: 212 us in the
    first 35 calls, 190 us afterwards), and a secondary should report the steady state a smoother loop runs in"""
    import time
    t0 = time.perf_counter()
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    for _ in range(50):
        if time.perf_counter() - t0 >= settle_s:
            break
        for _ in range(max(reps, 1)):
            fn()
        torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def brick_plan(level, deg, stream, torch, dev, count=None):
    """plan of a uniform brick with the geometric factors GENERATED ON THE DEVICE (no 80 B/node host arrays): the big secondaries"""
    from disco4est_amd import Plan, mesh as M
    m = M.BrickMesh(level, deg, count=count)
    plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, 0, stream=stream)
    plan.set_geometry_brick(np.ones(m.n_elements, dtype=np.int32), float(1 << level), [0.0, 1.0, 0.0, 1.0, 0.0, 1.0])
    plan.set_tuning(7, 0)     # general path: the per-node metric is streamed
    x = torch.rand(m.local_nodes, dtype=torch.float64, device=dev)
    return m, plan, x, torch.empty_like(x)


def full_operator_bytes_per_dof(N, NQ):
    """algorithmic bytes of one full operator apply per DoF: u 8 + A u 8 + metric 48 (NQ/N)^3 + the 7 pre-combined face factors per
    mortar node of 6 sides (= 64 + 336 / N at NQ = N); mortar-node traces and the neighbours' u are intermediates, not counted"""
    return algorithmic_bytes_per_dof(N, NQ) + 6.0 * 7.0 * 8.0 * NQ * NQ / N ** 3


def brick_operator_plan(level, deg, stream, torch, dev):
    """brick_plan + the SIPG faces, every geometric factor generated on the device (general path: per-node metric streamed)"""
    m, plan, x, y = brick_plan(level, deg, stream, torch, dev)
    sides = m.build_sides(None, geometry=False)
    plan.set_faces(sides, 10.0, 0, brick=(np.ones(m.n_elements, dtype=np.int32), float(1 << level), [0.0, 1.0, 0.0, 1.0, 0.0, 1.0]))
    return m, plan, x, y


def gate_operator(name, plan, level, deg, x, y, shards=3, factory=None, n_total=None, cnt=64):
    """parity gate of a timed full-operator secondary: A u of the plan's default kernel path against the oracle on 64-element shards cut
    from the mesh (whole-element ghost data gathered from the global vector); raises if the worst shard exceeds 1e-12.
    factory(first, count) -> the shard's mesh (default: the uniform brick of `level`, `deg`); n_total: elements of the whole mesh"""
    from disco4est_amd import mesh as M
    from tests import oracle_lib
    oracle = oracle_lib.load()
    plan.apply_aij(x, y)
    u, got = x.cpu().numpy(), y.cpu().numpy()
    n = 8 ** level if n_total is None else n_total
    cnt = min(cnt, n)
    firsts = sorted({0, ((n // 2 + n // 16) // cnt) * cnt, n - cnt})
    worst = 0.0
    for first in firsts[:shards]:
        sub = M.BrickMesh(level, deg, first=first, count=cnt) if factory is None else factory(first, cnt)
        Js, rsts = sub.geometry(None); ss = sub.build_sides(None)
        s0 = sub.global_nodal_offset
        ref = oracle.apply_aij(sub, Js, rsts, ss, np.ascontiguousarray(u[s0:s0 + sub.local_nodes]),
                               u_ghost=(sub.gather_ghost(ss, u) if ss["ghost_nodes"] > 0 else None), nthreads=min(os.cpu_count() or 1, 16))
        worst = max(worst, np.abs(got[s0:s0 + sub.local_nodes] - ref).max() / np.abs(ref).max())
    log("parity gate %s: A u against the oracle on %d shards of %d elements: rel-inf = %.3e  [%s]" % (name, len(firsts[:shards]), cnt, worst, plan.face_path()))
    if not worst <= 1e-12:
        raise RuntimeError("parity gate of %s failed: %.3e" % (name, worst))
    return worst


FP64_PEAK_TFLOPS = 78.6   # MI355X dense FP64 vector = matrix peak, /opt/skills/guides/MI355X_MICROARCH.md


def stiffness_flops_per_dof(N, NQ):
    """fused sum-factorisation, forward 2 (2 N^3 NQ + 3 N^2 NQ^2 + 3 N NQ^3), backward the same, metric 15 NQ^3
    (= 32 N + 15 per DoF at NQ = N)"""
    return (4.0 * (2 * N ** 3 * NQ + 3 * N * N * NQ * NQ + 3 * N * NQ ** 3) + 15.0 * NQ ** 3) / N ** 3


def mixed_operator_bytes(m, sides):
    """algorithmic bytes of one full operator apply on any mesh: u 8 + A u 8 per node, metric 48 per quadrature node, the 7 pre-combined
    face factors per mortar quadrature node (total_mortar_nodes counts every side's block once; the four small sides of a hanging face
    share theirs)"""
    return 16.0 * m.local_nodes + 48.0 * m.local_nodes_quad + 56.0 * float(sides["total_mortar_nodes"])


def graded_degrees(level):
    """config 4's degree field: p = 3 ... 9 over the level-`level` brick, SMOOTHLY graded (what smooth_pred hp-adaptation leaves behind:
    high degree where the solution is smooth, i.e. away from a corner here), neighbours differ by at most one"""
    from disco4est_amd import mesh as M
    ijk = M.morton_order(level).astype(np.float64)
    n = float(1 << level)
    r = np.sqrt(((ijk + 0.5) ** 2).sum(axis=1)) / (np.sqrt(3.0) * n)      # distance from the corner, 0 .. 1
    return np.clip(np.rint(3.0 + 6.0 * r), 3, 9).astype(np.int32)


def eig_window(plan, x, torch, its=12):
    """(lmin, lmax) for the Chebyshev secondaries: 1.1 x a power-iteration estimate of the largest eigenvalue, and 1/30 of it (the
    reference's smoother window, d4est_solver_multigrid_smoother_cheby.c:60-76) -- so that the timed iterations contract"""
    v = torch.rand_like(x); Av = torch.empty_like(x); lam = 1.0
    for _ in range(its):
        plan.apply_aij(v, Av)
        lam = float(torch.linalg.norm(Av) / torch.linalg.norm(v))
        v = Av / torch.linalg.norm(Av)
    return 1.1 * lam / 30.0, 1.1 * lam


def gate_cheby(name, plan, x, rhs, torch, iters=5, lmin=1.0, lmax=30.0):
    """parity gate of a timed Chebyshev secondary: the fused loop (update in the operator kernel's epilogue) against the recurrence of
    d4est_solver_multigrid_smoother_cheby.c:104-154 written out with separate vector operations around the (gated) operator"""
    uc = x.clone(); r = torch.empty_like(x); Au = torch.empty_like(x)
    plan.cheby_iterate(uc, rhs, Au, r, iters, lmin, lmax, 0)
    d, c = (lmax + lmin) / 2, (lmax - lmin) / 2
    ur = x.clone(); p = torch.zeros_like(x); Aur = torch.empty_like(x); alpha = 0.0
    for i in range(iters):
        alpha = 1 / d if i == 0 else (2 * d / (2 * d * d - c * c) if i == 1 else 1 / (d - alpha * c * c / 4))
        beta = alpha * d - 1
        plan.apply_aij(ur, Aur)
        p = alpha * (rhs - Aur) + beta * p
        ur = ur + p
    err = float((uc - ur).abs().max() / ur.abs().max())
    log("parity gate %s: %d fused Chebyshev iterations against the written-out recurrence: rel-inf = %.3e" % (name, iters, err))
    if not err <= 1e-12:
        raise RuntimeError("parity gate of %s failed: %.3e" % (name, err))
    return err


def gate_schwarz(torch, dev):
    """parity gate of the Schwarz secondary: one iterate (10 CG sweeps, tolerances off) on a 64-element p = 7 brick with overlap 2 --
    the kernels the timed config-2 iterate runs (whole-operator kernel on the subdomain plan, condensed corner copies, flat CG kernel)
    -- against the serial oracle (oracle/d4est_oracle_schwarz.c): same correction to 1e-9, same per-subdomain iteration counts"""
    from disco4est_amd import mesh as M
    from disco4est_amd.schwarz import Schwarz
    from tests import oracle_lib
    oracle = oracle_lib.load()
    m = M.BrickMesh(2, 7)
    J, rst = m.geometry(None); sides = m.build_sides(None)
    oracle.set_operator(m, J, rst, sides, 10.0, 0, threads=min(os.cpu_count() or 1, 16))
    sz = Schwarz(m, sides, J, rst, 2, 10, 1e-300, 1e-300, 10.0, 0)
    sz.plan.set_tuning(11, 2)    # the timed mesh is large enough for the one-kernel operator by default; this one is forced onto it
    r = M.splitmix64_uniform(42, m.local_nodes) - 0.5
    u0 = np.zeros(m.local_nodes)
    u_ref, it_ref, _ = oracle.schwarz_iterate(sz.metadata, u0, r, 10, 1e-300, 1e-300)
    u = torch.zeros(m.local_nodes, dtype=torch.float64, device=dev)
    sz.iterate(u, torch.from_numpy(r).to(dev))
    it, _ = sz.info()
    err = float(np.abs(u.cpu().numpy() - u_ref).max() / np.abs(u_ref).max())
    same = bool(np.array_equal(it, it_ref))
    log("parity gate schwarz_iterate_10_cg: against the serial oracle on 64 elements: rel-inf = %.3e, iteration counts equal: %s  [%s, %d condensed copies]"
        % (err, same, sz.plan.face_path(), sz.condensed_copies()))
    sz.destroy()
    if not (err <= 1e-9 and same):
        raise RuntimeError("parity gate of schwarz_iterate_10_cg failed: %.3e" % err)
    return err


def sharded_secondary(args, rank, world, dev, stream, dist, torch):
    """config 2 split over the ranks (strong scaling): apply_lhs and Chebyshev iterations with the face-trace exchange over RCCL
    in C; the sharded operator is checked against the same operator applied by ONE rank (rank-count invariance, d4est_test_mpi.sh)."""
    from disco4est_amd import Plan, mesh as M, parallel as P
    full = M.BrickMesh(args.level, args.deg)
    parts = P.partition_by_dofs(full.deg_global, world)
    first, count = parts[rank]
    m = M.BrickMesh(args.level, args.deg, first=first, count=count)
    J, rst = m.geometry(None)
    sides = m.build_sides(None)
    plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, 0, stream=stream)
    plan.set_geometry(J, rst)
    plan.set_tuning(7, 0)
    plan.set_faces(sides, 10.0, 0)
    sched = P.plan_schedule(plan, m, sides, parts)
    summ = [None] * world
    dist.all_gather_object(summ, P.schedule_summary(sched))
    ok, why = P.check_schedules_match(summ)
    if not ok:   # a mismatch would hang the grouped send / receive round: report instead
        return {"error": "exchange schedules of the ranks do not match: " + why}
    # transport: the library's RCCL exchange in C.  Rehearsals on ONE GPU (D4EST_BENCH_BACKEND=gloo; RCCL refuses two ranks on a device)
    # fall back to the host-side transport over torch.distributed, so that the schedules, the boundary / interior split of the
    # operator and the gather still run -- labelled in the result
    rehearsal = os.environ.get("D4EST_BENCH_BACKEND", "nccl") != "nccl"

    class _HostExchange:   # the handful of attributes the code below reads from the RCCL exchange wrapper
        def __init__(self, ex):
            self.ex, self.send_doubles = ex, int(sum(ex.s.send_len[p_] for p_ in ex.s.peers))
        def count(self):
            return -1
        def destroy(self):
            pass

    class _NoComm:
        def destroy(self):
            pass

    def wire(plan_, m_, sides_, parts_):
        if rehearsal:
            return _HostExchange(P.attach(plan_, m_, sides_, parts_, P.DistTransport(), dev))
        return P.attach_rccl(plan_, m_, sides_, parts_, comm)

    comm = _NoComm() if rehearsal else P.RcclComm(rank, world)
    x = wire(plan, m, sides, parts)
    u = torch.from_numpy(m.field(None)).to(dev)      # slice of ONE global field (offset by the shard's position)
    Au, rhs, r = torch.empty_like(u), torch.zeros_like(u), torch.empty_like(u)
    plan.apply_lhs(u, Au)
    torch.cuda.synchronize()
    # rank-count invariance: gather the sharded A u on rank 0 and compare with the one-rank operator on the whole mesh
    gathered = [None] * world if rank == 0 else None
    dist.gather_object(Au.cpu().numpy(), gathered, dst=0)
    invariance = None
    if rank == 0:
        Jf, rstf = full.geometry(None)
        pf = Plan(full.deg, full.deg_quad, full.nodal_stride, full.quad_stride, 0, stream=stream)
        pf.set_geometry(Jf, rstf)
        pf.set_tuning(7, 0)
        pf.set_faces(full.build_sides(None), 10.0, 0)
        uf = torch.from_numpy(full.field(None)).to(dev)
        ref = torch.empty_like(uf)
        pf.apply_aij(uf, ref)
        ref = ref.cpu().numpy()
        got = np.concatenate(gathered)
        invariance = float(np.abs(got - ref).max() / np.abs(ref).max())
        pf.destroy()
    res = {"transport": "host-side torch.distributed (one-GPU rehearsal)" if rehearsal else "RCCL in C (csrc/d4est_hip_comm.hip)",
           "ranks": world, "elements_per_rank": [int(c) for _, c in parts], "exchange_doubles_sent_by_rank0": int(x.send_doubles),
           "peers_of_rank0": [int(p_) for p_ in sched.peers], "rank_count_invariance_rel_inf": invariance}
    if not rehearsal:   # what RCCL itself says (ncclCommCount) -- absent on the host-transport rehearsal, where RCCL saw no ranks at all
        res["rccl_ranks"] = int(comm.lib.d4est_hip_comm_nccl_count(comm.handle))
        if res["rccl_ranks"] != world:
            return {"error": "ncclCommCount = %d but WORLD_SIZE = %d" % (res["rccl_ranks"], world)}

    def timed(fn, reps):
        for _ in range(3):
            fn()
        torch.cuda.synchronize(); dist.barrier(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize(); dist.barrier(); torch.cuda.synchronize()
        t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return t.item() / reps * 1e3

    ms = timed(lambda: plan.apply_lhs(u, Au), 50)
    res["apply_aij_config2_strong"] = {"ms": ms, "GDoF_per_s": full.local_nodes / (ms * 1e-3) / 1e9}
    ms = timed(lambda: plan.cheby_iterate(u, rhs, Au, r, 5, 1.0, 30.0, 0), 20)
    res["cheby_5_iterations_config2_strong"] = {"ms": ms, "GDoF_per_s": full.local_nodes * 5 / (ms * 1e-3) / 1e9}
    res["exchanges_posted"] = int(x.count())
    # roofline entry of the sharded full operator: algorithmic bytes of ONE rank's share per apply over the measured time
    N = args.deg + 1
    bpd_aij = full_operator_bytes_per_dof(N, N)
    res["apply_aij_config2_strong"]["roofline"] = {"bound": "hbm", "achieved": bpd_aij * full.local_nodes / world / (res["apply_aij_config2_strong"]["ms"] * 1e-3) / 1e9,
                                                   "peak": HBM_PEAK_GBS, "unit": "GB/s", "algorithmic_bytes_per_dof": bpd_aij}
    res["apply_aij_config2_strong"]["roofline"]["frac"] = res["apply_aij_config2_strong"]["roofline"]["achieved"] / HBM_PEAK_GBS
    x.destroy(); plan.destroy()
    # ---- config 4's shape: degrees p = 3 ... 9 graded smoothly across the level-4 brick, split N ways BY DoF COUNT (p4est_partition with
    # weights, SURVEY.md section 8e: the shards hold very different element counts); full operator, strong scaling
    try:
        degs = graded_degrees(args.level)
        fullm = M.BrickMesh(args.level, degs)
        mparts = P.partition_by_dofs(fullm.deg_global, world)
        mm = M.BrickMesh(args.level, degs, first=mparts[rank][0], count=mparts[rank][1])
        Jm, rstm = mm.geometry(None)
        sm = mm.build_sides(None)
        pm = Plan(mm.deg, mm.deg_quad, mm.nodal_stride, mm.quad_stride, 0, stream=stream)
        pm.set_geometry(Jm, rstm)
        pm.set_tuning(7, 0)
        pm.set_faces(sm, 10.0, 0)
        xm = wire(pm, mm, sm, mparts)
        um = torch.from_numpy(mm.field(None)).to(dev)
        Aum = torch.empty_like(um)
        ms = timed(lambda: pm.apply_lhs(um, Aum), 30)
        dofs_r = [int(sum((int(d) + 1) ** 3 for d in degs[f:f + c])) for f, c in mparts]
        res["apply_aij_mixed_p3_to_9_strong"] = {"ms": ms, "GDoF_per_s": fullm.local_nodes / (ms * 1e-3) / 1e9, "dofs": fullm.local_nodes,
                                                 "elements_per_rank": [int(c) for _, c in mparts], "dofs_per_rank": dofs_r,
                                                 "dof_imbalance": max(dofs_r) / (sum(dofs_r) / float(world)), "face_path": pm.face_path(),
                                                 "exchange_doubles_sent_by_rank0": int(xm.send_doubles)}
        xm.destroy(); pm.destroy()
    except Exception as exc:
        res["apply_aij_mixed_p3_to_9_strong"] = {"error": repr(exc)}
    # ---- WEAK scaling of the full operator: one config-2 brick's worth of elements per rank, WITH neighbours -- the domain is the box of
    # the first `world` level-`level` sub-cubes of the level + 1 Morton sequence (world = 8: the whole level + 1 cube), every rank
    # owns one sub-cube and exchanges face traces with up to three others
    try:
        lvl = args.level + 1
        per = 8 ** args.level
        wparts = [(r_ * per, per) for r_ in range(world)]
        mw_ = M.BrickMesh(lvl, args.deg, first=rank * per, count=per, domain=world * per)
        Jw, rstw = mw_.geometry(None)
        sw = mw_.build_sides(None)
        pw = Plan(mw_.deg, mw_.deg_quad, mw_.nodal_stride, mw_.quad_stride, 0, stream=stream)
        pw.set_geometry(Jw, rstw)
        pw.set_tuning(7, 0)
        pw.set_faces(sw, 10.0, 0)
        xw = wire(pw, mw_, sw, wparts)
        uw = torch.from_numpy(mw_.field(None)).to(dev)
        Auw = torch.empty_like(uw)
        ms = timed(lambda: pw.apply_lhs(uw, Auw), 50)
        tot = mw_.local_nodes * world
        res["apply_aij_config2_weak"] = {"ms": ms, "GDoF_per_s": tot / (ms * 1e-3) / 1e9, "elements_per_rank": per, "face_path": pw.face_path(),
                                         "exchange_doubles_sent_by_rank0": int(xw.send_doubles),
                                         "roofline": {"bound": "hbm", "achieved": bpd_aij * mw_.local_nodes / (ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS,
                                                      "unit": "GB/s", "frac": bpd_aij * mw_.local_nodes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                                      "algorithmic_bytes_per_dof": bpd_aij}}
        xw.destroy(); pw.destroy()
    except Exception as exc:
        res["apply_aij_config2_weak"] = {"error": repr(exc)}
    comm.destroy()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--level", type=int, default=4)
    ap.add_argument("--deg", type=int, default=7)
    ap.add_argument("--deg-quad-inc", type=int, default=0)
    ap.add_argument("--geometry", choices=["affine", "sine"], default="affine")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--no-secondary", action="store_true")
    ap.add_argument("--sharded-secondary", action="store_true",
                    help="N = 1 only: also run the N-rank secondary (RCCL transport, gather, rank-count invariance) on the single rank -- a rehearsal of its code path")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline: the parity gate against the CPU oracle, the secondary numbers (other operators, "
                         "degrees, sizes and mesh classes, each gated), the CPU baseline and, on N > 1 ranks, the sharded secondaries "
                         "(--no-check / --no-secondary / --no-cpu-baseline switch parts of it off)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last step computed (A u of the headline apply) to DIR/<name>.npy as float64")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    # `python bench.py --gpus N` by hand: become the launcher (before anything touches the GPU) and relay the ranks' output
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        import subprocess
        port = os.environ.get("MASTER_PORT", "29533")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
               "--master-port", port, os.path.abspath(__file__)] + sys.argv[1:]
        log("launching: " + " ".join(cmd))
        raise SystemExit(subprocess.run(cmd).returncode)
    if int(os.environ.get("WORLD_SIZE", "1")) != args.gpus:
        raise SystemExit("bench.py: WORLD_SIZE=%s but --gpus %d -- refusing to report a line for a different rank count"
                         % (os.environ.get("WORLD_SIZE", "1"), args.gpus))

    # stdout carries exactly ONE line, the JSON result: everything else a library may print there (RCCL's version banner at
    # communicator creation, for one) is sent to stderr by pointing fd 1 at fd 2 until the line is written
    sys.stdout.flush()
    result_fd = os.dup(1)
    os.dup2(2, 1)

    def emit(obj):
        sys.stdout.flush()
        os.write(result_fd, (json.dumps(obj) + "\n").encode())

    import torch
    from disco4est_amd import Plan, build, mesh as M

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (no CPU fallback)")
    dev_index = local_rank % max(torch.cuda.device_count(), 1)   # one rank per GPU; the modulo only matters for rehearsals on smaller boxes
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    dist = None
    if world > 1 or args.sharded_secondary:
        import torch.distributed as dist_mod
        dist = dist_mod
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29534")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        backend = os.environ.get("D4EST_BENCH_BACKEND", "nccl")   # nccl = RCCL over xGMI; "gloo" only to rehearse the N > 1 path on one GPU
        try:
            dist.init_process_group(backend=backend, device_id=dev) if backend == "nccl" else dist.init_process_group(backend=backend)
        except TypeError:  # older signature without device_id
            dist.init_process_group(backend=backend)
        dist.barrier()
    # the library normally travels pre-built; if the sources look newer, rank 0 rebuilds and everybody waits
    if build.needs_build() and rank == 0:
        build.build_library(verbose=False)
    if dist is not None:
        dist.barrier()

    # ---- workload: config 2 of BASELINE.json, one brick per rank (weak scaling)
    mesh = M.BrickMesh(args.level, args.deg, deg_quad_inc=args.deg_quad_inc)
    mp = M.SineMap(0.05) if args.geometry == "sine" else None
    J, rst = mesh.geometry(mp)
    u = mesh.field(mp, seed=102321 + rank)
    N, NQ = args.deg + 1, args.deg + args.deg_quad_inc + 1

    stream = torch.cuda.current_stream()
    plan = Plan(mesh.deg, mesh.deg_quad, mesh.nodal_stride, mesh.quad_stride, 0, stream=stream)
    plan.set_geometry(J, rst)
    # headline = the GENERAL path (per-node metric streamed from HBM, 64 B/DoF, like the reference): the affine shortcut the
    # engine would take by itself on this brick is switched off here and reported separately under "secondary"
    plan.set_tuning(7, 0)
    du = torch.from_numpy(u).to(dev)
    dAu = torch.empty_like(du)

    # ---- parity gate on a sample before any timing is reported (--full)
    if args.full and not args.no_check and rank == 0:
        from tests import oracle_lib
        oracle = oracle_lib.load()
        plan.apply_stiffness_matrix(du, dAu)
        got = dAu.cpu().numpy()
        worst = 0.0
        for e in range(0, mesh.n_elements, max(1, mesh.n_elements // 16)):
            sub = M.BrickMesh(args.level, args.deg, deg_quad_inc=args.deg_quad_inc, first=e, count=1)
            Je, rste = sub.geometry(mp)
            s, n3 = mesh.nodal_stride[e], N ** 3
            ref = oracle.apply_stiffness(sub, Je, rste, np.ascontiguousarray(u[s:s + n3]))
            worst = max(worst, np.abs(got[s:s + n3] - ref).max() / np.abs(ref).max())
        log("parity vs oracle on sampled elements: rel-inf = %.3e" % worst)
        if not worst <= 1e-12:
            raise SystemExit("parity gate failed: %.3e" % worst)

    # ---- warm-up, then time exactly K steps
    for _ in range(args.warmup):
        plan.apply_stiffness_matrix(du, dAu)
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    ev0.record(stream)
    for _ in range(args.steps):
        plan.apply_stiffness_matrix(du, dAu)
    ev1.record(stream)
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    kernel_ms = ev0.elapsed_time(ev1) / args.steps  # HIP events on the launch stream: average launch duration

    if dist is not None:
        t = torch.tensor([elapsed, kernel_ms], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed, kernel_ms = t[0].item(), t[1].item()
    if args.dump_outputs:
        dump_output(args.dump_outputs, "Au" if world == 1 else "Au_rank%d" % rank, dAu, DUMP_BUDGET_BYTES // world)

    dofs_per_rank = mesh.local_nodes
    total_dofs = dofs_per_rank * world
    value = total_dofs * args.steps / elapsed / 1e9
    bpd = algorithmic_bytes_per_dof(N, NQ)
    achieved = bpd * dofs_per_rank / (kernel_ms * 1e-3) / 1e9  # GB/s of the dominant kernel on one GPU

    traffic = None
    tf = os.path.join(ROOT, "profiles", "traffic.json")
    if os.path.exists(tf):
        try:
            rec = json.load(open(tf))
            key = "level%d_p%d_inc%d" % (args.level, args.deg, args.deg_quad_inc)
            traffic = rec.get(key, {}).get("hbm_bytes_per_launch")
        except Exception:
            traffic = None

    out = {
        "metric": "GDoF/s for matrix-free 3D DG stiffness apply (Ax), p=%d" % args.deg,
        "value": value,
        "unit": "GDoF/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f64",
        "data": "synthetic",
        "config": {
            "workload": "3D Poisson stiffness apply on a single-tree brick, uniform level=%d (%d elements/GPU), p=%d, "
                        "deg_quad=deg+%d, Gauss-Legendre; general path (per-node symmetric metric streamed, %s values)"
                        % (args.level, mesh.n_elements, args.deg, args.deg_quad_inc, args.geometry),
            "dofs_per_gpu": dofs_per_rank,
            "elements_per_gpu": mesh.n_elements,
            "sharding": "one Morton-contiguous brick per rank, no data-path collective",
        },
        "roofline": {
            "bound": "hbm",
            "achieved": achieved,
            "peak": HBM_PEAK_GBS,
            "unit": "GB/s",
            "frac": achieved / HBM_PEAK_GBS,
            "traffic": traffic,
            "kernel": plan.last_kernel(),
            "kernel_avg_ms": kernel_ms,
            "algorithmic_bytes_per_dof": bpd,
        },
    }
    # ---- secondary, single-GPU only (reported, not the headline; --full): the full operator A u (volume + SIPG faces,
    # d4est_laplacian_apply_aij) and one Chebyshev smoother iteration (apply + fused update), SURVEY.md section 8d
    if args.full and rank == 0 and world == 1 and not args.no_secondary:
        try:
            sides = mesh.build_sides(mp)
            plan.set_faces(sides, 10.0, 0)
            rhs = torch.zeros_like(du)
            r = torch.empty_like(du)
            sec = {}
            # parity gates BEFORE the numbers (none of them inside a timed region): the operator on the default kernel path of this mesh
            # against the oracle on 64-element shards, the fused Chebyshev loop against the written-out recurrence
            gates = {}
            lmin, lmax = eig_window(plan, du, torch)
            if not args.no_check:
                gates["apply_aij"] = gate_operator("apply_aij", plan, args.level, args.deg, du, dAu) if (args.geometry != "sine" and args.deg_quad_inc == 0) else None
                gates["cheby_5_iterations"] = gate_cheby("cheby_5_iterations", plan, du, rhs, torch, 5, lmin, lmax)
            for name, fn, applies in (("apply_aij", lambda: plan.apply_aij(du, dAu), 1),
                                      ("cheby_5_iterations", lambda: plan.cheby_iterate(du, rhs, dAu, r, 5, lmin, lmax, 0), 5)):
                ms = time_region(fn, 50, stream, torch, warm=10)
                sec[name] = {"ms": ms, "GDoF_per_s": dofs_per_rank * applies / (ms * 1e-3) / 1e9}
                # a Chebyshev iteration moves the operator's bytes (A u itself is not stored) plus the smoother's own vectors: rhs read,
                # p read and written, the new iterate written (u is the operator's input; r is written in the last iteration only)
                bpd_aij = full_operator_bytes_per_dof(N, NQ) + (CHEBY_VECTOR_BYTES_PER_DOF if applies > 1 else 0.0)
                sec[name]["algorithmic_bytes_per_dof"] = bpd_aij
                sec[name]["roofline_frac_hbm"] = bpd_aij * dofs_per_rank * applies / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS
                sec[name]["face_path"] = plan.face_path()   # "direct+volume": the whole operator in one kernel (u in, A u out)
                sec[name]["parity_gate_rel_inf"] = gates.get(name)
            # apply_lhs of a linearised nonlinear problem (BASELINE config 4's operator: Laplacian + V^T W J f'(u0) V u,
            # constant_density_star_fcns.h:528-603): the zeroth-order term rides in the operator kernel's volume stage (w J c pre-combined
            # at plan_set_lhs_coefficient: +8 B per node).  Gate: against apply_aij + the separate weighted-mass kernel (each held to the oracle).
            cq = 1.0 + torch.rand(mesh.local_nodes_quad, dtype=torch.float64, device=dev)
            plan.set_lhs_coefficient(cq)
            glhs = None
            if not args.no_check:
                ya, yb = torch.empty_like(du), torch.empty_like(du)
                plan.apply_lhs(du, ya)
                plan.apply_aij(du, yb)
                plan.apply_weighted_mass_matrix(du, cq, dAu)
                glhs = float((ya - (yb + dAu)).abs().max() / ya.abs().max())
                log("parity gate apply_lhs_with_coefficient: fused zeroth-order term against apply_aij + weighted mass: rel-inf = %.3e" % glhs)
                if not glhs <= 1e-12:
                    raise RuntimeError("parity gate of apply_lhs_with_coefficient failed: %.3e" % glhs)
                del ya, yb
            ms = time_region(lambda: plan.apply_lhs(du, dAu), 50, stream, torch, warm=10)
            bpd_lhs = full_operator_bytes_per_dof(N, NQ) + 8.0 * (NQ / N) ** 3
            sec["apply_lhs_with_coefficient"] = {"ms": ms, "GDoF_per_s": dofs_per_rank / (ms * 1e-3) / 1e9, "algorithmic_bytes_per_dof": bpd_lhs,
                                                 "roofline_frac_hbm": bpd_lhs * dofs_per_rank / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                                 "vs_apply_aij": ms / sec["apply_aij"]["ms"], "face_path": plan.face_path(),
                                                 "parity_gate_rel_inf": glhs}
            plan.set_lhs_coefficient(None)
            del cq
            # HBM traffic of one apply_aij from the PMC counters (2 FETCH_SIZE + WRITE_SIZE, profiles/): neighbours' u re-read past the L2
            try:
                rec = json.load(open(tf)) if os.path.exists(tf) else {}
                sec["apply_aij"]["traffic"] = rec.get("apply_aij_level%d_p%d" % (args.level, args.deg), {}).get("hbm_bytes_per_launch")
            except Exception:
                sec["apply_aij"]["traffic"] = None
            # the affine path: same brick, metric rebuilt from 6 numbers per element, 16 B/DoF
            if args.geometry != "sine":
                plan.set_tuning(7, -1)
                ms = time_region(lambda: plan.apply_stiffness_matrix(du, dAu), 100, stream, torch, warm=20)
                sec["stiffness_p%d_affine_path" % args.deg] = {"ms": ms, "GDoF_per_s": dofs_per_rank / (ms * 1e-3) / 1e9,
                                                                "algorithmic_bytes_per_dof": 16.0, "kernel": plan.last_kernel(),
                                                                "flops_per_dof": stiffness_flops_per_dof(N, NQ),
                                                                "roofline_frac_fp64": stiffness_flops_per_dof(N, NQ) * dofs_per_rank / (ms * 1e-3) / 1e12 / FP64_PEAK_TFLOPS}
                # ... and the full operator / the smoother iteration with the affine volume metric (the face factors are still streamed):
                # what a brick gets when tuning key 7 is left alone; labelled separately like the entry above
                for name, fn, applies in (("apply_aij_affine_path", lambda: plan.apply_aij(du, dAu), 1),
                                          ("cheby_5_iterations_affine_path", lambda: plan.cheby_iterate(du, rhs, dAu, r, 5, lmin, lmax, 0), 5)):
                    ms = time_region(fn, 50, stream, torch, warm=10)
                    bpd_af = 16.0 + 6.0 * 7.0 * 8.0 * NQ * NQ / N ** 3 + (CHEBY_VECTOR_BYTES_PER_DOF if applies > 1 else 0.0)
                    sec[name] = {"ms": ms, "GDoF_per_s": dofs_per_rank * applies / (ms * 1e-3) / 1e9, "face_path": plan.face_path(),
                                 "algorithmic_bytes_per_dof": bpd_af,
                                 "roofline_frac_hbm": bpd_af * dofs_per_rank * applies / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                 # the volume term's flops alone (the face terms add to them): a lower bound of the FP64 fraction
                                 "roofline_frac_fp64_volume_flops_only": stiffness_flops_per_dof(N, NQ) * dofs_per_rank * applies / (ms * 1e-3) / 1e12 / FP64_PEAK_TFLOPS}
                plan.set_tuning(7, 0)
            # stiffness apply at the other degrees SURVEY.md section 8d names (same general path, ~2-8 MDoF each)
            for deg, level, count in ((3, 5, None), (11, 4, None), (15, 4, 2048)):
                m2 = M.BrickMesh(level, deg, count=count)
                J2, rst2 = m2.geometry(None)
                p2 = Plan(m2.deg, m2.deg_quad, m2.nodal_stride, m2.quad_stride, 0, stream=stream)
                p2.set_geometry(J2, rst2)
                p2.set_tuning(7, 0)
                x2 = torch.from_numpy(m2.field()).to(dev)
                y2 = torch.empty_like(x2)
                ms = time_region(lambda: p2.apply_stiffness_matrix(x2, y2), 40, stream, torch, warm=20)
                sec["stiffness_p%d" % deg] = {"ms": ms, "GDoF_per_s": m2.local_nodes / (ms * 1e-3) / 1e9, "dofs": m2.local_nodes,
                                              "kernel": p2.last_kernel(), "stream_mode": p2.stream_mode()}
                if deg == 15:   # config 5's degree on the affine path (labelled separately: the brick's metric from 6 numbers per element)
                    p2.set_tuning(7, -1)
                    ms = time_region(lambda: p2.apply_stiffness_matrix(x2, y2), 40, stream, torch, warm=20)
                    sec["stiffness_p15_affine_path"] = {"ms": ms, "GDoF_per_s": m2.local_nodes / (ms * 1e-3) / 1e9, "dofs": m2.local_nodes,
                                                        "kernel": p2.last_kernel(), "algorithmic_bytes_per_dof": 16.0,
                                                        "flops_per_dof": stiffness_flops_per_dof(16, 16),
                                                        "roofline_frac_fp64": stiffness_flops_per_dof(16, 16) * m2.local_nodes / (ms * 1e-3) / 1e12 / FP64_PEAK_TFLOPS}
                p2.destroy()
                del x2, y2
            # off-cache points (the config-2 working set, 134 MB, sits in the 256 MB Infinity Cache): level 5 at p = 7 (1.07 GB per
            # apply) and BASELINE config 3 at full size (level 5, p = 11, 56.6 MDoF, 3.6 GB per apply); factors generated on the device
            # ... and config 5's degree at a size past the ramp (8192 elements, 33.6 MDoF, 2.1 GB per apply)
            # ... and the top of SURVEY.md section 8d's level sweep: level 6 at p = 7 (262 144 elements, 134 MDoF, 8.6 GB per apply)
            for name, level, deg, count in (("stiffness_p7_level5", 5, 7, None), ("stiffness_p7_level6", 6, 7, None),
                                            ("stiffness_p11_level5_config3", 5, 11, None),
                                            ("stiffness_p15_8192_elements", 5, 15, 8192)):
                m2, p2, x2, y2 = brick_plan(level, deg, stream, torch, dev, count=count)
                ms = time_region(lambda: p2.apply_stiffness_matrix(x2, y2), 10 if count is None else 30, stream, torch, warm=10 if count is None else 30)
                bytes_ = algorithmic_bytes_per_dof(deg + 1, deg + 1) * m2.local_nodes
                # stream_mode 1: the plan does not fit the Infinity Cache, so metric loads and A u stores carry the non-temporal hint (tuning key 12)
                sec[name] = {"ms": ms, "GDoF_per_s": m2.local_nodes / (ms * 1e-3) / 1e9, "dofs": m2.local_nodes, "kernel": p2.last_kernel(),
                             "roofline_frac_hbm": bytes_ / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "stream_mode": p2.stream_mode()}
                if deg == 11:
                    # the same config on the AFFINE path (labelled separately, SURVEY.md section 8d: the brick's metric is constant per
                    # element and is rebuilt from 6 numbers instead of being streamed: 16 B/DoF, arithmetic-bound)
                    p2.set_tuning(7, -1)
                    ms = time_region(lambda: p2.apply_stiffness_matrix(x2, y2), 10, stream, torch)
                    sec[name + "_affine_path"] = {"ms": ms, "GDoF_per_s": m2.local_nodes / (ms * 1e-3) / 1e9, "dofs": m2.local_nodes,
                                                  "kernel": p2.last_kernel(), "algorithmic_bytes_per_dof": 16.0,
                                                  "flops_per_dof": stiffness_flops_per_dof(deg + 1, deg + 1),
                                                  "roofline_frac_fp64": stiffness_flops_per_dof(deg + 1, deg + 1) * m2.local_nodes / (ms * 1e-3) / 1e12 / FP64_PEAK_TFLOPS}
                p2.destroy()
                del x2, y2
            # the FULL operator at the degrees of BASELINE configs 3 and 5: one kernel per apply
            # (operator_mw_kernel: volume term + trace-free SIPG faces per multi-wave workgroup); geometric factors generated on the
            # device, general path; each gated against the oracle on 64-element shards before it is timed
            for name, level, deg, reps in (("apply_aij_p11_level4", 4, 11, 30), ("apply_aij_p11_level5_config3", 5, 11, 8),
                                           ("apply_aij_p15_level4", 4, 15, 12)):
                m2, p2, x2, y2 = brick_operator_plan(level, deg, stream, torch, dev)
                g = None if args.no_check else gate_operator(name, p2, level, deg, x2, y2, shards=2 if level == 5 else 3)
                ms = time_region(lambda: p2.apply_aij(x2, y2), reps, stream, torch, warm=reps)
                bpd_aij = full_operator_bytes_per_dof(deg + 1, deg + 1)
                sec[name] = {"ms": ms, "GDoF_per_s": m2.local_nodes / (ms * 1e-3) / 1e9, "dofs": m2.local_nodes, "elements": m2.n_elements,
                             "algorithmic_bytes_per_dof": bpd_aij,
                             "roofline_frac_hbm": bpd_aij * m2.local_nodes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                             "face_path": p2.face_path(), "kernel": p2.last_kernel(), "parity_gate_rel_inf": g, "stream_mode": p2.stream_mode()}
                try:
                    sec[name]["traffic"] = (json.load(open(tf)) if os.path.exists(tf) else {}).get(name, {}).get("hbm_bytes_per_launch")
                except Exception:
                    sec[name]["traffic"] = None
                if name == "apply_aij_p11_level4":
                    rhs2 = torch.zeros_like(x2); r2 = torch.empty_like(x2)
                    l0, l1 = eig_window(p2, x2, torch)
                    gc = None if args.no_check else gate_cheby("cheby_5_iterations_p11_level4", p2, x2, rhs2, torch, 5, l0, l1)
                    ms = time_region(lambda: p2.cheby_iterate(x2, rhs2, y2, r2, 5, l0, l1, 0), 10, stream, torch, warm=5)
                    bpd_ch = bpd_aij + CHEBY_VECTOR_BYTES_PER_DOF
                    sec["cheby_5_iterations_p11_level4"] = {"ms": ms, "GDoF_per_s": 5 * m2.local_nodes / (ms * 1e-3) / 1e9,
                                                            "algorithmic_bytes_per_dof": bpd_ch, "parity_gate_rel_inf": gc,
                                                            "roofline_frac_hbm": 5 * bpd_ch * m2.local_nodes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS}
                    del rhs2, r2
                p2.destroy()
                del x2, y2
            # additive Schwarz smoother on the same mesh: one d4est_solver_schwarz_iterate with
            # 10 CG iterations per subdomain (tolerances off), all subdomains batched on the subdomain plan
            if args.geometry != "sine" and mesh.n_elements <= 4096:
                from disco4est_amd.schwarz import Schwarz
                gsz = None if args.no_check else gate_schwarz(torch, dev)
                sz = Schwarz(mesh, sides, J, rst, 2, 10, 1e-300, 1e-300, 10.0, 0, stream=stream)
                us = torch.zeros_like(du)
                sz.iterate(us, du)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(3):
                    sz.iterate(us, du)
                e1.record(stream)
                torch.cuda.synchronize()
                ms = e0.elapsed_time(e1) / 3
                sec["schwarz_iterate_10_cg"] = {"ms": ms, "subdomains": sz.metadata.num_subdomains,
                                                "subdomain_elements": sz.metadata.num_elements, "num_nodes_overlap": 2,
                                                "ms_per_cg_sweep": ms / 10, "face_path": sz.plan.face_path(),
                                                # corner copies whose operator rows are dense blocks probed from the operator
                                                "condensed_copies": sz.condensed_copies(), "parity_gate_rel_inf": gsz}
                sz.destroy()
                del us
            # BASELINE config 4's shape in miniature: degrees p = 3 ... 9 scattered over the level-4 brick (1.75 MDoF), general path --
            # the volume term (the buckets with deg_quad = deg <= 7 in one launch, p = 8, 9 in a second one) and the full operator
            # (two-phase tiled face kernels: the mesh holds degrees above 7)
            if args.geometry != "sine":
                degs = 3 + (np.arange(8 ** 4) * 5) % 7
                m4 = M.BrickMesh(4, degs)
                J4, rst4 = m4.geometry(None)
                p4 = Plan(m4.deg, m4.deg_quad, m4.nodal_stride, m4.quad_stride, 0, stream=stream)
                p4.set_geometry(J4, rst4)
                p4.set_tuning(7, 0)
                p4.set_faces(m4.build_sides(None))
                x4 = torch.from_numpy(m4.field()).to(dev)
                y4 = torch.empty_like(x4)
                s4 = m4.build_sides(None)
                try:
                    g4 = None if args.no_check else gate_operator("mixed_p3_to_9_level4", p4, 4, None, x4, y4, shards=3,
                                                                  factory=lambda first, cnt: M.BrickMesh(4, degs, first=first, count=cnt))
                except Exception as exc:   # recorded in the entry (and on stderr), the other secondaries still run
                    log("parity gate mixed_p3_to_9_level4 FAILED: %r" % (exc,))
                    g4 = "FAILED: " + repr(exc)
                ms_s = time_region(lambda: p4.apply_stiffness_matrix(x4, y4), 50, stream, torch, warm=10)
                ms_a = time_region(lambda: p4.apply_aij(x4, y4), 50, stream, torch, warm=10)
                by4 = mixed_operator_bytes(m4, s4)
                sec["mixed_p3_to_9_level4"] = {"dofs": m4.local_nodes, "elements": m4.n_elements, "stiffness_ms": ms_s,
                                               "stiffness_GDoF_per_s": m4.local_nodes / (ms_s * 1e-3) / 1e9, "apply_aij_ms": ms_a,
                                               "apply_aij_GDoF_per_s": m4.local_nodes / (ms_a * 1e-3) / 1e9,
                                               "algorithmic_bytes_per_dof": by4 / m4.local_nodes,
                                               "roofline_frac_hbm": by4 / (ms_a * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                               "stiffness_roofline_frac_hbm": 64.0 * m4.local_nodes / (ms_s * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                               "traffic": (json.load(open(tf)) if os.path.exists(tf) else {}).get("mixed_p3_to_9_level4", {}).get("hbm_bytes_per_launch"),
                                               "face_path": p4.face_path(), "parity_gate_rel_inf": g4}
                p4.destroy()
                del x4, y4
            # a locally refined (hanging-face) brick, the mesh class of BASELINE config 4: level 4 with every 64th octant refined
            # (4544 elements, 336 hanging faces, 19 % of the elements touch one), p = 7, general path.  Plans with hanging faces run
            # traces + volume + flux; with every degree <= 7 the conforming sides go through the fast conforming face kernels and only
            # the hanging sides through the mortar-record kernels (tuning key 13).  Gate: that split against the all-records path
            # (both are held to the oracle by tests/test_faces_gpu.py::test_hp_split_parity / test_apply_aij_hanging_parity)
            if args.geometry != "sine":
                refine = np.zeros(8 ** 4, dtype=bool)
                refine[::64] = True
                m5 = M.HangingBrickMesh(4, refine, 7)
                J5, rst5 = m5.geometry(None)
                s5 = m5.build_sides(None)
                x5 = torch.from_numpy(m5.field()).to(dev)
                res5 = {}
                # three forms of the same operator: every side through the mortar-record kernels (0) / conforming sides through the fast
                # conforming kernels, hanging sides through the record kernels ("split") / the default: the hybrid operator in its
                # hanging-aware form -- EVERY element gets the whole operator from the one-kernel path (small hanging sides read the big
                # element's sub-mortar block and export their own), only the big sides' terms come from the record kernels, before / after it
                for key, (k13, k14) in (("records", (0, 0)), ("split", (-1, 0)), (-1, (-1, -1))):
                    p5 = Plan(m5.deg, m5.deg_quad, m5.nodal_stride, m5.quad_stride, 0, stream=stream)
                    p5.set_tuning(13, k13)
                    p5.set_tuning(14, k14)
                    p5.set_geometry(J5, rst5)
                    p5.set_tuning(7, 0)
                    p5.set_faces(s5)
                    y5 = torch.empty_like(x5)
                    ms5 = time_region(lambda: p5.apply_aij(x5, y5), 50, stream, torch, warm=10)
                    res5[key] = (ms5, y5.clone(), p5.face_path())
                    p5.destroy()
                res5[0] = res5["records"]
                g5 = max(float((res5[k_][1] - res5[0][1]).abs().max() / res5[0][1].abs().max()) for k_ in (-1, "split"))
                print("parity gate hanging_level4_p7: hybrid and split forms against the mortar-record kernels: rel-inf = %.3e" % g5, file=sys.stderr)
                if not args.no_check and not g5 <= 1e-12:
                    raise RuntimeError("hanging_level4_p7: the split face path deviates from the record kernels by %.3e" % g5)
                g5o = None
                if not args.no_check:   # the default path against the ORACLE on shards of the hanging mesh (ghost elements gathered from the global vector)
                    p5 = Plan(m5.deg, m5.deg_quad, m5.nodal_stride, m5.quad_stride, 0, stream=stream)
                    p5.set_geometry(J5, rst5); p5.set_tuning(7, 0); p5.set_faces(s5)
                    y5 = torch.empty_like(x5)
                    try:
                        g5o = gate_operator("hanging_level4_p7", p5, 4, None, x5, y5, shards=3, n_total=m5.n_elements, cnt=71,
                                            factory=lambda first, cnt: M.HangingBrickMesh(4, refine, 7, first=first, count=cnt))
                    except Exception as exc:
                        log("parity gate hanging_level4_p7 FAILED: %r" % (exc,))
                        g5o = "FAILED: " + repr(exc)
                    p5.destroy()
                # the smoother on that mesh: 5 Chebyshev iterations on the default path (update in the operator kernel and the record flux
                # kernel), gated against the written-out recurrence, and with the update as a separate kernel (tuning key 10 = 0)
                cheb5 = {}
                try:
                    p5 = Plan(m5.deg, m5.deg_quad, m5.nodal_stride, m5.quad_stride, 0, stream=stream)
                    p5.set_geometry(J5, rst5); p5.set_tuning(7, 0); p5.set_faces(s5)
                    y5 = torch.empty_like(x5); rhs5 = torch.zeros_like(x5); r5 = torch.empty_like(x5)
                    l0, l1 = eig_window(p5, x5, torch)
                    gc5 = None if args.no_check else gate_cheby("hanging_level4_p7 cheby", p5, x5, rhs5, torch, 5, l0, l1)
                    xc5 = x5.clone()
                    ms_f = time_region(lambda: p5.cheby_iterate(xc5, rhs5, y5, r5, 5, l0, l1, 0), 20, stream, torch, warm=5)
                    p5.set_tuning(10, 0)
                    ms_s = time_region(lambda: p5.cheby_iterate(xc5, rhs5, y5, r5, 5, l0, l1, 0), 20, stream, torch, warm=5)
                    p5.destroy()
                    cheb5 = {"cheby_5_iterations_ms": ms_f, "cheby_GDoF_per_s": 5 * m5.local_nodes / (ms_f * 1e-3) / 1e9,
                             "cheby_5_iterations_ms_separate_update_kernel": ms_s, "parity_gate_cheby_rel_inf": gc5}
                except Exception as exc:
                    log("hanging_level4_p7 cheby FAILED: %r" % (exc,))
                    cheb5 = {"cheby": "FAILED: " + repr(exc)}
                by5 = mixed_operator_bytes(m5, s5)
                sec["hanging_level4_p7"] = {"dofs": m5.local_nodes, "elements": m5.n_elements,
                                            "hanging_faces": int((np.asarray(s5["side_hang"]) == 1).sum()),
                                            "apply_aij_ms": res5[-1][0], "apply_aij_GDoF_per_s": m5.local_nodes / (res5[-1][0] * 1e-3) / 1e9,
                                            "algorithmic_bytes_per_dof": by5 / m5.local_nodes,
                                            "roofline_frac_hbm": by5 / (res5[-1][0] * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                            "traffic": (json.load(open(tf)) if os.path.exists(tf) else {}).get("hanging_level4_p7", {}).get("hbm_bytes_per_launch"),
                                            "apply_aij_ms_record_kernels_only": res5[0][0], "apply_aij_ms_two_phase_split": res5["split"][0],
                                            "face_path": res5[-1][2],
                                            "parity_gate_rel_inf": g5o, "parity_gate_rel_inf_vs_record_kernels": g5}
                sec["hanging_level4_p7"].update(cheb5)
                if "cheby_5_iterations_ms" in cheb5:
                    sec["hanging_level4_p7"]["cheby_roofline_frac_hbm"] = 5 * (by5 + CHEBY_VECTOR_BYTES_PER_DOF * m5.local_nodes) / (cheb5["cheby_5_iterations_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS
                del x5, res5
            # BASELINE config 4's mesh class proper: hanging faces AND mixed degrees, smoothly graded -- the level-4 brick with every 64th octant
            # refined and p = 3 ... 9 rising with the distance from a corner (4544 elements); the full operator and a Chebyshev iteration on it,
            # algorithmic bytes, oracle shard gate.  Also the graded mesh without the refinement (the mesh of profiles/r04_mixed_p_graded_*).
            def sec_config4():
                refine = np.zeros(8 ** 4, dtype=bool)
                refine[::64] = True
                gd = graded_degrees(4)
                for name, mk in (("mixed_p3_to_9_graded_level4", lambda **kw: M.BrickMesh(4, gd, **kw)),
                                 ("config4_mesh_class_level4", lambda **kw: M.HangingBrickMesh(4, refine, np.concatenate([np.full(8 if refine[b] else 1, gd[b]) for b in range(8 ** 4)]).astype(np.int32), **kw))):
                    m7 = mk()
                    J7, rst7 = m7.geometry(None); s7 = m7.build_sides(None)
                    p7 = Plan(m7.deg, m7.deg_quad, m7.nodal_stride, m7.quad_stride, 0, stream=stream)
                    p7.set_geometry(J7, rst7); p7.set_tuning(7, 0); p7.set_faces(s7)
                    x7 = torch.from_numpy(m7.field()).to(dev); y7 = torch.empty_like(x7)
                    cnt7 = 64 if name.startswith("mixed") else 71
                    try:
                        g7 = None if args.no_check else gate_operator(name, p7, 4, None, x7, y7, shards=3, n_total=m7.n_elements, cnt=cnt7,
                                                                      factory=lambda first, cnt: mk(first=first, count=cnt))
                    except Exception as exc:
                        log("parity gate %s FAILED: %r" % (name, exc))
                        g7 = "FAILED: " + repr(exc)
                    ms_a = time_region(lambda: p7.apply_aij(x7, y7), 50, stream, torch, warm=10)
                    l0, l1 = eig_window(p7, x7, torch)
                    rhs7 = torch.zeros_like(x7); r7 = torch.empty_like(x7)
                    gc7 = None if args.no_check else gate_cheby(name + " cheby", p7, x7, rhs7, torch, 5, l0, l1)
                    ms_c = time_region(lambda: p7.cheby_iterate(x7, rhs7, y7, r7, 5, l0, l1, 0), 20, stream, torch, warm=5)
                    by7 = mixed_operator_bytes(m7, s7)
                    sec[name] = {"dofs": m7.local_nodes, "elements": m7.n_elements, "degrees": "p = 3 ... 9 graded (neighbours differ by at most one)",
                                 "hanging_faces": int((np.asarray(s7["side_hang"]) == 1).sum()) if "side_hang" in s7 else 0,
                                 "apply_aij_ms": ms_a, "apply_aij_GDoF_per_s": m7.local_nodes / (ms_a * 1e-3) / 1e9,
                                 "algorithmic_bytes_per_dof": by7 / m7.local_nodes, "roofline_frac_hbm": by7 / (ms_a * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                 "cheby_5_iterations_ms": ms_c, "cheby_GDoF_per_s": 5 * m7.local_nodes / (ms_c * 1e-3) / 1e9,
                                 "cheby_roofline_frac_hbm": 5 * (by7 + CHEBY_VECTOR_BYTES_PER_DOF * m7.local_nodes) / (ms_c * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                 "traffic": (json.load(open(tf)) if os.path.exists(tf) else {}).get(name, {}).get("hbm_bytes_per_launch"),
                                 "face_path": p7.face_path(), "parity_gate_rel_inf": g7, "parity_gate_cheby_rel_inf": gc7}
                    p7.destroy()
                    del x7, y7, rhs7, r7
            if args.geometry != "sine":
                try:
                    sec_config4()
                except Exception as exc:
                    log("secondary config4_mesh_class_level4 failed: %r" % (exc,))
                    sec["config4_mesh_class_level4"] = {"error": repr(exc)}
            # config 4's mesh class AT SIZE (level 5: the throughput regime; at level 4 every kernel of these paths sits on its latency floor):
            # the locally refined p = 7 brick (36 352 elements, 18.6 MDoF), the graded p = 3 ... 9 brick (32 768 elements, 13.6 MDoF) and both at once
            # (graded degrees AND every 64th octant refined: the class proper), default
            # paths (at this size the hybrid operator on both: thousands of clean elements per degree bucket); gate: the same operator through
            # the two-phase kernels (hybrid off) -- both forms are held to the oracle at level 4 above
            def sec_config4_level5():
                refine5 = np.zeros(8 ** 5, dtype=bool)
                refine5[::64] = True
                gd5 = graded_degrees(5)
                for name, mk, alt in (("hanging_level5_p7", lambda: M.HangingBrickMesh(5, refine5, 7), 0),
                                      ("mixed_p3_to_9_graded_level5", lambda: M.BrickMesh(5, gd5), 0),
                                      ("config4_mesh_class_level5", lambda: M.HangingBrickMesh(5, refine5, np.concatenate([np.full(8 if refine5[b] else 1, gd5[b]) for b in range(8 ** 5)]).astype(np.int32)), 0)):
                    m8 = mk()
                    J8, rst8 = m8.geometry(None); s8 = m8.build_sides(None)
                    x8 = torch.from_numpy(m8.field()).to(dev)
                    res8 = {}
                    for key, k14 in (("default", -1), ("other", alt)):
                        if key == "other" and args.no_check:
                            continue
                        p8 = Plan(m8.deg, m8.deg_quad, m8.nodal_stride, m8.quad_stride, 0, stream=stream)
                        p8.set_tuning(14, k14); p8.set_geometry(J8, rst8); p8.set_tuning(7, 0); p8.set_faces(s8)
                        y8 = torch.empty_like(x8)
                        ms8 = time_region(lambda: p8.apply_aij(x8, y8), 10, stream, torch, warm=3)
                        ch8 = None
                        if key == "default":   # the smoother at size: 5 Chebyshev iterations (update fused where the path carries it), gated
                            try:
                                rhs8 = torch.zeros_like(x8); r8 = torch.empty_like(x8); yc8 = torch.empty_like(x8)
                                gc8 = None if args.no_check else gate_cheby(name + " cheby", p8, x8, rhs8, torch, 5, 1.0, 40.0)
                                xc8 = x8.clone()
                                ms_c8 = time_region(lambda: p8.cheby_iterate(xc8, rhs8, yc8, r8, 5, 1.0, 40.0, 0), 4, stream, torch, warm=1)
                                ch8 = (ms_c8, gc8)
                                del rhs8, r8, yc8, xc8
                            except Exception as exc:
                                log("%s cheby FAILED: %r" % (name, exc))
                                ch8 = (None, "FAILED: " + repr(exc))
                        res8[key] = (ms8, y8, p8.face_path(), ch8)
                        p8.destroy()
                    g8 = None
                    if "other" in res8:
                        g8 = float((res8["default"][1] - res8["other"][1]).abs().max() / res8["other"][1].abs().max())
                        log("parity gate %s: default path [%s] against [%s]: rel-inf = %.3e" % (name, res8["default"][2][:40], res8["other"][2][:40], g8))
                        if not g8 <= 1e-12:
                            raise RuntimeError("%s: the two operator paths differ by %.3e" % (name, g8))
                    by8 = mixed_operator_bytes(m8, s8)
                    ms8 = res8["default"][0]
                    sec[name] = {"dofs": m8.local_nodes, "elements": m8.n_elements, "apply_aij_ms": ms8,
                                 "apply_aij_GDoF_per_s": m8.local_nodes / (ms8 * 1e-3) / 1e9, "algorithmic_bytes_per_dof": by8 / m8.local_nodes,
                                 "roofline_frac_hbm": by8 / (ms8 * 1e-3) / 1e9 / HBM_PEAK_GBS, "face_path": res8["default"][2],
                                 "traffic": (json.load(open(tf)) if os.path.exists(tf) else {}).get(name, {}).get("hbm_bytes_per_launch"),
                                 "parity_gate_rel_inf_vs_other_path": g8,
                                 "apply_aij_ms_other_path": res8["other"][0] if "other" in res8 else None}
                    ch8 = res8["default"][3]
                    if ch8 is not None:
                        sec[name]["parity_gate_cheby_rel_inf"] = ch8[1]
                        if ch8[0] is not None:
                            sec[name]["cheby_5_iterations_ms"] = ch8[0]
                            sec[name]["cheby_GDoF_per_s"] = 5 * m8.local_nodes / (ch8[0] * 1e-3) / 1e9
                            sec[name]["cheby_roofline_frac_hbm"] = 5 * (by8 + CHEBY_VECTOR_BYTES_PER_DOF * m8.local_nodes) / (ch8[0] * 1e-3) / 1e9 / HBM_PEAK_GBS
                    del x8, res8
            if args.geometry != "sine":
                try:
                    sec_config4_level5()
                except Exception as exc:
                    log("secondary config4 level 5 failed: %r" % (exc,))
                    sec["hanging_level5_p7"] = sec.get("hanging_level5_p7", {"error": repr(exc)})
            # BASELINE config 5's mesh class AT SIZE: the reference's 7-tree cubed sphere, level 3 (3584 curved elements, 14.7 MDoF), p = 15, every
            # geometric factor (volume metric and mortar factors through the oriented tree faces) generated on the device from the analytic
            # map; side list from d4est_hip_build_sides.  Gate: the oracle on shards of 4 elements with host-computed factors.
            def sec_cubed_sphere():
                from disco4est_amd import forest as F
                conn = F.cubed_sphere_7tree_connectivity()
                cmap = F.CubedSphere7Map(1.0, 2.0)
                m6 = F.ForestMesh(conn, 3, 15, cmap)
                tree6, q6, dq6 = m6.cells()
                par6 = (1.0, 2.0, 0.0)
                p6 = Plan(m6.deg, m6.deg_quad, m6.nodal_stride, m6.quad_stride, 0, stream=stream)
                p6.set_geometry_analytic(1, par6, tree6, q6, dq6, m6.nf)
                p6.set_tuning(7, 0)
                s6 = m6.build_sides_c()
                p6.set_faces(s6, 10.0, 0, analytic=(1, par6, tree6, q6, dq6, m6.nf, None))
                x6 = torch.rand(m6.local_nodes, dtype=torch.float64, device=dev); y6 = torch.empty_like(x6)
                u6 = x6.cpu().numpy()
                g6 = None
                if not args.no_check:
                    from tests import oracle_lib
                    orc = oracle_lib.load()
                    p6.apply_aij(x6, y6)
                    got6 = y6.cpu().numpy(); g6 = 0.0
                    for first in (6 * 512, 2 * 512 + 200):   # in the centre cube (faces towards the wedges: orientation != 0) and in a wedge
                        sub = F.ForestMesh(conn, 3, 15, cmap, first=first, count=4)
                        Js, rsts = sub.geometry(); ss = sub.build_sides()
                        s0 = sub.global_nodal_offset
                        ref = orc.apply_aij(sub, Js, rsts, ss, np.ascontiguousarray(u6[s0:s0 + sub.local_nodes]), u_ghost=sub.gather_ghost(ss, u6),
                                            nthreads=min(os.cpu_count() or 1, 16))
                        g6 = max(g6, float(np.abs(got6[s0:s0 + sub.local_nodes] - ref).max() / np.abs(ref).max()))
                    log("parity gate apply_aij_cubed_sphere_p15: A u against the oracle on 2 shards of 4 curved elements: rel-inf = %.3e  [%s]" % (g6, p6.face_path()))
                    if not g6 <= 1e-12:
                        raise RuntimeError("parity gate of apply_aij_cubed_sphere_p15 failed: %.3e" % g6)
                ms = time_region(lambda: p6.apply_aij(x6, y6), 10, stream, torch, warm=10)
                by6 = 16.0 * m6.local_nodes + 48.0 * m6.local_nodes_quad + 56.0 * float(s6["total_mortar_nodes"])
                sec["apply_aij_cubed_sphere_p15"] = {"ms": ms, "GDoF_per_s": m6.local_nodes / (ms * 1e-3) / 1e9, "dofs": m6.local_nodes,
                                                     "elements": m6.n_elements, "trees": 7, "algorithmic_bytes_per_dof": by6 / m6.local_nodes,
                                                     "roofline_frac_hbm": by6 / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "face_path": p6.face_path(),
                                                     "kernel": p6.last_kernel(), "parity_gate_rel_inf": g6, "stream_mode": p6.stream_mode(),
                                                     "geometry": "cubed_sphere_7tree R0 = 1, R1 = 2, factors generated on the device"}
                p6.destroy()
                del x6, y6
            if args.geometry != "sine":
                try:
                    sec_cubed_sphere()
                except Exception as exc:   # this block's failure (a parity gate included) is recorded in its own entry
                    log("secondary apply_aij_cubed_sphere_p15 failed: %r" % (exc,))
                    sec["apply_aij_cubed_sphere_p15"] = {"error": repr(exc)}
            # The multigrid MATRIX OPERATOR (verdict row a14): apply_lhs on a COARSE level, whose zeroth-order term the reference holds as
            # Galerkin-restricted dense element blocks (Solver/d4est_solver_multigrid_matrix_operator.c).  Coarse = level 3, p = 7 (512
            # elements), fine = level 4, p = 7 (config 2): blocks built on the device (QUAD_COMPUTE_MATRIX for every fine element, P^T M P),
            # then the term (a) as the dense-block stream (1.07 GB per apply: HBM-bound) and (b) as the matrix-free Galerkin chain
            # (prolong, fine weighted mass, prolong-transpose).  Gate: (a) against a torch bmm of the same blocks, (b) against (a).
            def sec_multigrid():
                from disco4est_amd import Transfer
                mcz, pcz, xz, yz = brick_operator_plan(3, 7, stream, torch, dev)
                mfz, pfz, _, _ = brick_plan(4, 7, stream, torch, dev)
                cz = 1.0 + torch.rand(mfz.local_nodes_quad, dtype=torch.float64, device=dev)
                pfz.set_lhs_coefficient(cz)
                Tz = Transfer(np.ones(mcz.n_elements, np.int32), np.full(mcz.n_elements, 7, np.int32), np.full(8 * mcz.n_elements, 7, np.int32), stream=stream)
                fb = torch.empty(pfz.matrix_nodes(), dtype=torch.float64, device=dev)
                cb = torch.empty(pcz.matrix_nodes(), dtype=torch.float64, device=dev)
                t0 = time.perf_counter()
                pfz.compute_weighted_mass_blocks(cz, fb); Tz.galerkin_blocks(fb, cb); torch.cuda.synchronize()
                setup_ms = (time.perf_counter() - t0) * 1e3
                del fb
                ms_lap = time_region(lambda: pcz.apply_aij(xz, yz), 30, stream, torch, warm=10)
                lapz = yz.clone()
                pcz.set_lhs_element_blocks(cb)
                pcz.apply_lhs(xz, yz)
                refz = lapz + torch.bmm(cb.view(mcz.n_elements, 512, 512), xz.view(mcz.n_elements, 512, 1)).view(-1)
                gb_ = float((yz - refz).abs().max() / refz.abs().max())
                ya_ = yz.clone()
                ms_blk = time_region(lambda: pcz.apply_lhs(xz, yz), 20, stream, torch, warm=5)
                pcz.set_lhs_galerkin_chain([Tz], pfz)
                pcz.apply_lhs(xz, yz)
                gc_ = float((yz - ya_).abs().max() / ya_.abs().max())
                log("parity gate mg_matrix_operator_level3_p7: block term against torch.bmm rel-inf = %.3e, Galerkin chain against the blocks %.3e" % (gb_, gc_))
                if not args.no_check and not (gb_ <= 1e-12 and gc_ <= 1e-12):
                    raise RuntimeError("parity gate of mg_matrix_operator_level3_p7 failed: %.3e %.3e" % (gb_, gc_))
                ms_chn = time_region(lambda: pcz.apply_lhs(xz, yz), 20, stream, torch, warm=5)
                blk_bytes = 8.0 * cb.numel()
                sec["mg_matrix_operator_level3_p7"] = {
                    "coarse_elements": mcz.n_elements, "coarse_dofs": mcz.local_nodes, "fine_dofs": mfz.local_nodes, "apply_aij_ms": ms_lap,
                    "apply_lhs_blocks_ms": ms_blk, "block_term_ms": ms_blk - ms_lap, "block_bytes": blk_bytes,
                    "block_term_GB_per_s": blk_bytes / ((ms_blk - ms_lap) * 1e-3) / 1e9,
                    "block_term_roofline_frac_hbm": blk_bytes / ((ms_blk - ms_lap) * 1e-3) / 1e9 / HBM_PEAK_GBS,
                    "apply_lhs_chain_ms": ms_chn, "chain_term_ms": ms_chn - ms_lap,
                    # the chain's algorithmic bytes: fine coefficient 8 per fine quadrature node + the coarse vector in and out
                    "chain_algorithmic_bytes": 8.0 * mfz.local_nodes_quad + 16.0 * mcz.local_nodes,
                    "setup_blocks_ms": setup_ms, "parity_gate_rel_inf_blocks_vs_bmm": gb_, "parity_gate_rel_inf_chain_vs_blocks": gc_}
                pcz.set_lhs_galerkin_chain([], None)
                # hp-multigrid transfers at config-2 size (verdict item 8): p-coarsening 7 -> 6 on the level-4 brick and h-coarsening level 4 ->
                # level 3 at p = 7; algorithmic bytes = one vector in + one out.  Then a two-grid cycle on config 2 (3 Chebyshev iterations,
                # residual, restriction, 3 iterations on the level-3 re-discretisation, prolongation + correction, 3 iterations).
                hp = {}
                for tname, Tt in (("p7_to_p6_level4", Transfer(np.zeros(4096, np.int32), np.full(4096, 6, np.int32),
                                                                np.ascontiguousarray(np.stack([np.full(4096, 7, np.int32)] + [np.zeros(4096, np.int32)] * 7, axis=1).reshape(-1)), stream=stream)),
                                  ("level4_to_level3_p7", Tz)):
                    xc_ = torch.rand(Tt.coarse_nodes, dtype=torch.float64, device=dev); xf_ = torch.rand(Tt.fine_nodes, dtype=torch.float64, device=dev)
                    oc_, of_ = torch.empty_like(xc_), torch.empty_like(xf_)
                    byt = 8.0 * (Tt.coarse_nodes + Tt.fine_nodes)
                    ent = {"coarse_dofs": Tt.coarse_nodes, "fine_dofs": Tt.fine_nodes, "algorithmic_bytes": byt}
                    for op, fn in (("prolong", lambda: Tt.prolong(xc_, of_)), ("restrict", lambda: Tt.restrict(xf_, oc_)), ("project", lambda: Tt.project(xf_, oc_))):
                        ms_ = time_region(fn, 50, stream, torch, warm=10)
                        ent[op + "_us"] = ms_ * 1e3
                        ent[op + "_roofline_frac_hbm"] = byt / (ms_ * 1e-3) / 1e9 / HBM_PEAK_GBS
                    # adjointness <P xc, xf> = <xc, P^T xf> as the gate of the pair (each is held to the oracle by tests/test_transfer_gpu.py)
                    Tt.prolong(xc_, of_); Tt.restrict(xf_, oc_)
                    a_, b_ = float(of_ @ xf_), float(xc_ @ oc_)
                    ent["adjointness_rel"] = abs(a_ - b_) / max(abs(a_), abs(b_))
                    hp[tname] = ent
                    if Tt is not Tz:
                        Tt.destroy()
                sec["hp_transfer_level4_p7"] = hp
                l0f, l1f = lmin, lmax
                l0c, l1c = eig_window(pcz, xz, torch)
                rf = torch.empty_like(du); ef = torch.empty_like(du)
                rc = torch.empty_like(xz); ec = torch.empty_like(xz); Ac = torch.empty_like(xz); rr = torch.empty_like(xz)
                uu = torch.zeros_like(du)

                def two_grid():
                    plan.cheby_iterate(uu, du, dAu, rf, 3, l0f, l1f, 1)      # pre-smoothing, rf = rhs - A u on exit (rhs = du)
                    Tz.restrict(rf, rc)
                    ec.zero_()
                    pcz.cheby_iterate(ec, rc, Ac, rr, 3, l0c, l1c, 0)
                    Tz.prolong(ec, ef)
                    uu.add_(ef)
                    plan.cheby_iterate(uu, du, dAu, rf, 3, l0f, l1f, 0)
                ms_tg = time_region(two_grid, 20, stream, torch, warm=5)
                ms_sm = time_region(lambda: plan.cheby_iterate(uu, du, dAu, rf, 3, l0f, l1f, 1), 20, stream, torch, warm=5)
                sec["two_grid_cycle_level4_p7"] = {"ms": ms_tg, "fine_smoother_3_iterations_with_residual_ms": ms_sm,
                                                   "transfer_us": hp["level4_to_level3_p7"]["restrict_us"] + hp["level4_to_level3_p7"]["prolong_us"],
                                                   "fine_dofs": mesh.local_nodes, "coarse_dofs": mcz.local_nodes}
                pcz.destroy(); pfz.destroy(); Tz.destroy()
                del cb, cz, xz, yz
            if args.geometry != "sine":
                try:
                    sec_multigrid()
                except Exception as exc:   # this block's failure (a parity gate included) is recorded in its own entry
                    log("secondary mg_matrix_operator_level3_p7 failed: %r" % (exc,))
                    sec["mg_matrix_operator_level3_p7"] = {"error": repr(exc)}
            out["secondary"] = sec
        except Exception as exc:  # secondary numbers must never break the headline line
            out["secondary"] = {"error": repr(exc)}
    import threading as _threading
    emitted, dog, emit_lock = [False], None, _threading.Lock()
    if world == 1 and args.sharded_secondary:
        out["sharded_rehearsal"] = sharded_secondary(args, rank, world, dev, stream, dist, torch)
    if args.full and world > 1 and not args.no_secondary:
        # strong-scaling secondaries with the RCCL exchange; a watchdog prints the headline alone if they do not finish
        import threading

        def give_up():
            log("rank %d: the sharded secondary (or the final barrier) did not finish in time; reporting the headline without it" % rank)
            with emit_lock:   # (never kill the process while the main thread is inside emit(): the line must be whole, and printed once)
                if rank == 0 and not emitted[0]:
                    out["secondary"] = {"error": "sharded secondary timed out"}
                    out["cpu_baseline"] = None
                    emitted[0] = True
                    emit(out)
                # rank 0 has a complete result line on stdout: exit 0; a rank that hung in a collective reports it with its exit status
                os._exit(0 if rank == 0 else 3)

        dog = threading.Timer(float(os.environ.get("D4EST_BENCH_SECONDARY_TIMEOUT", "240")), give_up)
        dog.daemon = True
        dog.start()
        try:
            sec = sharded_secondary(args, rank, world, dev, stream, dist, torch)
        except Exception as exc:
            sec = {"error": repr(exc)}
        # the watchdog stays armed through the final barrier: a rank that failed here must not leave its peers (stuck in a collective
        # of the secondary) and itself (stuck in the barrier) waiting for each other; the result line is written once either way
        if rank == 0:
            out["secondary"] = sec
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(mesh, J, rst, u)
    elif rank == 0:
        out["cpu_baseline"] = None
    with emit_lock:
        if rank == 0 and not emitted[0]:
            emitted[0] = True
            emit(out)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if dog is not None:
        dog.cancel()


if __name__ == "__main__":
    main()
