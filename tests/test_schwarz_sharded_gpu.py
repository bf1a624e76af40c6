"""The Schwarz smoother and preconditioner on SHARDED plans: both whole-element exchanges inside the library
(d4est_hip_schwarz_set_element_exchange, schwarz.SchwarzShardNative), through d4est_hip_schwarz_iterate / _smooth, the V-cycle object, the
reuse_smoother bottom solver and d4est_hip_pc_schwarz_apply.

Several virtual ranks in one process on one GPU.  The ranks run as threads in lock-step, as tests/test_hybrid_ghost_gpu.py::_lockstep
does: null stream, one barrier per exchange / reduction round (with a time limit), barrier.abort() when a rank raises, joins with a time
limit -- a stuck rank fails the test.  The lazily built state of every rank (workspaces, condensed blocks) is created rank after rank
before the threads start.

Bounds.  Against the Python composition SchwarzShard on the same shards: equality (np.array_equal) -- the subdomain solves are the same
code on the same extended residual and the accumulate kernel adds in SchwarzShard's order.  Against one rank: 1e-10 relative to the size of
the correction, the bound tests/test_parallel_gpu.py::test_schwarz_virtual_ranks_match_single_rank uses for the composition.  V-cycle and
FCG histories: 1e-9 relative (the 1e-10 of a smoother call compounds over three cycles / the iterations).
Observed on MI355X: iterate 1e-16 .. 8e-16, smoother u 5e-15 / r 4e-13; V-cycle and FCG in their docstrings."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from tests import schwarz_shard_cases as C

pytestmark = pytest.mark.gpu
SUB = (10, 1e-15, 1e-15)          # 10 subdomain iterations at 1e-15 / 1e-15: stopped by the count
JOIN = 180.0


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


class _Mailbox:
    def __init__(self):
        self.box = {}


class _LocalTransport:
    """SchwarzShard's phases run one rank after the other (tests/test_parallel_gpu.py)"""

    def __init__(self, rank, mailbox):
        self.rank, self.mb = rank, mailbox

    def start(self, send_buf, recv_buf):
        for p, t in send_buf.items():
            self.mb.box[(self.rank, p)] = t.clone()
        return recv_buf

    def finish(self, recv_buf):
        for p, t in recv_buf.items():
            t.copy_(self.mb.box[(p, self.rank)])


class _LockstepTransport:
    """tests/test_hybrid_ghost_gpu.py's lock-step transport plus round(): one complete whole-element exchange.  Every rank makes the same
    sequence of rounds, so a per-rank counter names the round; the barrier stands for the completion of the messages."""

    def __init__(self, rank, world, mailbox, barrier):
        self.rank, self.world, self.mb, self.barrier = rank, world, mailbox, barrier
        self.k_x = self.k_r = self.k_e = 0

    def start(self, send_buf, recv_buf):
        for p, t in send_buf.items():
            self.mb.box[("x", self.rank, p, self.k_x)] = t.clone()
        return recv_buf

    def finish(self, recv_buf):
        self.barrier.wait()
        for p, t in recv_buf.items():
            t.copy_(self.mb.box[("x", p, self.rank, self.k_x)])
        self.k_x += 1

    def round(self, send_buf, recv_buf):
        for p, t in send_buf.items():
            self.mb.box[("e", self.rank, p, self.k_e)] = t.clone()
        self.barrier.wait()
        for p, t in recv_buf.items():
            t.copy_(self.mb.box[("e", p, self.rank, self.k_e)])
        self.k_e += 1

    def allreduce_sum(self, t):
        self.mb.box[("r", self.rank, self.k_r)] = t.clone()
        self.barrier.wait()
        tot = self.mb.box[("r", 0, self.k_r)].clone()
        for r in range(1, self.world):
            tot += self.mb.box[("r", r, self.k_r)]
        t.copy_(tot)
        self.k_r += 1


def _run_lockstep(world, barrier, gpu, body):
    """body(rank) on one thread per rank; returns the list of results"""
    import torch
    out, errs = [None] * world, []

    def run(r):
        try:
            torch.cuda.set_device(gpu)
            out[r] = body(r)
        except BaseException as e:   # (a rank that fails must not leave the others waiting)
            errs.append(e)
            barrier.abort()

    threads = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(JOIN)
    assert not any(t.is_alive() for t in threads), "a rank is stuck"
    assert not errs, errs
    return out


class _World:
    """the native shards of one partition with their lock-step transports; make(rank) -> SchwarzShardNative"""

    def __init__(self, world, gpu, make):
        from disco4est_amd import parallel as P
        self.world, self.gpu = world, gpu
        self.mb = _Mailbox()
        self.barrier = threading.Barrier(world, timeout=120)
        self.transports = [_LockstepTransport(r, world, self.mb, self.barrier) for r in range(world)]
        self.shards = [make(r) for r in range(world)]
        for sh, tr in zip(self.shards, self.transports):
            P.attach_schwarz(sh, tr, gpu)
            sh.schwarz.condensed_copies()        # the lazily built state, rank after rank, before any thread starts

    def run(self, body):
        return _run_lockstep(self.world, self.barrier, self.gpu, body)

    def close(self):
        for sh in self.shards:
            sh.destroy()


def _own_plan(make_mesh, mp, parts, rank, transport, gpu, prefactor=10.0):
    """the rank's own plan: ghost sides, the trace exchange and allreduce hooks on the lock-step transport"""
    from disco4est_amd import Plan, parallel as P
    first, count = parts[rank]
    m = make_mesh(first, count)
    J, rst = m.geometry(mp)
    s = m.build_sides(mp)
    plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, 0)
    plan.set_geometry(J, rst)
    plan.set_faces(s, prefactor, 0)
    ex = P.attach(plan, m, s, parts, transport, gpu)
    assert plan.ghost_trace_size > 0
    return m, plan, ex


def _global_plan(mesh, mp, prefactor=10.0):
    from disco4est_amd import Plan
    J, rst = mesh.geometry(mp)
    s = mesh.build_sides(mp)
    plan = Plan(mesh.deg, mesh.deg_quad, mesh.nodal_stride, mesh.quad_stride, 0)
    plan.set_geometry(J, rst)
    plan.set_faces(s, prefactor, 0)
    return plan, (J, rst, s)


def _classic_iterate(make_classic, world, slices, u0, r, gpu):
    """SchwarzShard.iterate of every rank, phase by phase (the Python composition)"""
    mb, mb_back = _Mailbox(), _Mailbox()
    shards = [make_classic(rank, _LocalTransport(rank, mb), _LocalTransport(rank, mb_back)) for rank in range(world)]
    us = [_t(u0[lo:hi], gpu) for lo, hi in slices]
    rs = [_t(r[lo:hi], gpu) for lo, hi in slices]
    for sh, rr in zip(shards, rs):
        sh.begin_residual_exchange(rr)
    for sh in shards:
        sh.solve_and_begin_correction_exchange()
    for sh, u in zip(shards, us):
        sh.end_correction_exchange(u)
    out = [u.cpu().numpy() for u in us]
    for sh in shards:
        sh.schwarz.destroy()
    return out


def _iterate_case(gpu, mg, mp, world, parts, rs, make_native, make_classic, seeds, want_multi_peer):
    """the two assertions of the iterate tests: bit-equal to SchwarzShard on the same shards, the single-rank iterate to 1e-10"""
    import torch
    from disco4est_amd import mesh as M, parallel as P
    from disco4est_amd.schwarz import Schwarz
    Jg, rstg = mg.geometry(mp); sg = mg.build_sides(mp)
    single = Schwarz(mg, sg, Jg, rstg, rs, *SUB)
    u0 = M.splitmix64_uniform(seeds[0], mg.local_nodes) - 0.5
    r = M.splitmix64_uniform(seeds[1], mg.local_nodes) - 0.5
    u_ref = _t(u0, gpu)
    single.iterate(u_ref, _t(r, gpu))
    u_ref = u_ref.cpu().numpy()
    single.destroy()
    slices = []
    for first, count in parts:
        lo = int(mg.global_nodal_stride[first])
        slices.append((lo, lo + int(((mg.deg[first:first + count].astype(np.int64) + 1) ** 3).sum())))
    classic = _classic_iterate(make_classic, world, slices, u0, r, gpu)
    W = _World(world, gpu, make_native)
    try:
        multi = []
        for sh in W.shards:
            send_elem = P.element_exchange_lists(sh.schedule, sh.mesh.nodal_stride)[2]
            multi.append(int((np.bincount(send_elem, minlength=sh.n_own) >= 2).sum()))
        if want_multi_peer:
            assert max(multi) > 0, "some own element must receive corrections from at least two peers"
        for sh, (lo, hi) in zip(W.shards, slices):
            assert sh.own_nodes == hi - lo and sh.schwarz.local_nodes == hi - lo and sh.mesh.n_elements > sh.n_own
        us = [_t(u0[lo:hi], gpu) for lo, hi in slices]
        rr = [_t(r[lo:hi], gpu) for lo, hi in slices]
        sweeps = W.run(lambda k: W.shards[k].iterate(us[k], rr[k]))
        torch.cuda.synchronize()
        assert all(0 < s <= SUB[0] for s in sweeps)
        got = np.empty_like(u_ref)
        for k, (lo, hi) in enumerate(slices):
            mine = us[k].cpu().numpy()
            assert np.array_equal(mine, classic[k]), ("rank %d differs from SchwarzShard.iterate" % k, np.abs(mine - classic[k]).max())
            got[lo:hi] = mine
        err = np.abs(got - u_ref).max() / np.abs(u_ref - u0).max()
        print("sharded iterate, world %d: vs one rank %.3e (bit-equal to the composition), multi-peer elements per rank %s" % (world, err, multi))
        assert err <= 1e-10, err
        return multi
    finally:
        W.close()


# ---- 1: iterate, brick -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,level,deg_spec,rs,curved", C.BRICK)
def test_iterate_brick(gpu, hiplib, world, level, deg_spec, rs, curved):
    from disco4est_amd import mesh as M
    from disco4est_amd.schwarz import SchwarzShard, SchwarzShardNative
    deg_global, parts = C.brick_case(world, level, deg_spec)
    mp = M.SineMap(0.04) if curved else None
    mg = M.BrickMesh(level, deg_global)
    multi = _iterate_case(gpu, mg, mp, world, parts, rs,
                          lambda rank: SchwarzShardNative(level, deg_global, parts, rank, mp, rs, *SUB),
                          lambda rank, tr, trb: SchwarzShard(level, deg_global, parts, rank, mp, rs, *SUB, tr, gpu, transport_back=trb),
                          (81, 82), world > 2)
    assert multi == {2: [0, 0], 3: [6, 12, 7], 4: [4, 4, 4, 4]}[world]


# ---- 2: iterate, hanging mesh ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,pattern,deg_spec,rs", C.HANGING)
def test_iterate_hanging_mesh(gpu, hiplib, world, pattern, deg_spec, rs):
    from disco4est_amd import mesh as M
    from disco4est_amd.schwarz import SchwarzShard, SchwarzShardNative
    refine, deg_global, parts = C.hanging_case(world, pattern, deg_spec)
    mp = M.SineMap(0.04)
    mg = M.HangingBrickMesh(1, refine, deg_global)
    _iterate_case(gpu, mg, mp, world, parts, rs,
                  lambda rank: SchwarzShardNative(1, deg_global, parts, rank, mp, rs, *SUB, refine=refine),
                  lambda rank, tr, trb: SchwarzShard(1, deg_global, parts, rank, mp, rs, *SUB, tr, gpu, transport_back=trb, refine=refine),
                  (83, 84), False)


# ---- 3: the smoother ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_smoother_through_both_entries(gpu, hiplib, world):
    """d4est_hip_schwarz_smooth and d4est_hip_multigrid_smooth_level (a two-level object, p - 1 below) on the rank's own plan: the
    gathered u and r equal one rank's Schwarz.smooth to 1e-10 (of max|u_ref - u0|, max|r_ref|), the two entries agree bit for bit"""
    import torch
    from disco4est_amd import Multigrid, Transfer, mesh as M
    from disco4est_amd.schwarz import Schwarz, SchwarzShardNative
    level, deg_spec, rs, iterations = 2, [2, 3], 2, 2
    deg_global, parts = C.brick_case(world, level, deg_spec)
    mp = M.SineMap(0.04)
    mg = M.BrickMesh(level, deg_global)
    plan_g, (Jg, rstg, sg) = _global_plan(mg, mp)
    single = Schwarz(mg, sg, Jg, rstg, rs, *SUB)
    u0 = M.splitmix64_uniform(91, mg.local_nodes) - 0.5
    rhs = M.splitmix64_uniform(92, mg.local_nodes) - 0.5
    u_ref = _t(u0, gpu); r_ref = torch.full_like(u_ref, float("nan"))
    single.smooth(plan_g, u_ref, _t(rhs, gpu), r_ref, iterations)
    u_ref, r_ref = u_ref.cpu().numpy(), r_ref.cpu().numpy()
    single.destroy(); plan_g.destroy()

    W = _World(world, gpu, lambda rank: SchwarzShardNative(level, deg_global, parts, rank, mp, rs, *SUB))
    keep = []
    try:
        ranks = []
        for k in range(world):
            first, count = parts[k]
            m, plan, ex = _own_plan(lambda f, c: M.BrickMesh(level, deg_global, first=f, count=c), mp, parts, k, W.transports[k], gpu)
            mc, coarse, exc = _own_plan(lambda f, c: M.BrickMesh(level, deg_global - 1, first=f, count=c), mp, parts, k, W.transports[k], gpu)
            degh = np.zeros(8 * count, dtype=np.int32)
            degh[0::8] = m.deg
            T = Transfer(np.zeros(count, np.int32), mc.deg.astype(np.int32), degh)
            mgo = Multigrid([coarse, plan], [T])
            assert mgo.set_smoother_schwarz([None, W.shards[k].schwarz], iterations) == 0
            lo = m.global_nodal_offset
            ranks.append((m, plan, mgo, lo, lo + m.local_nodes))
            keep += [ex, exc, mgo, T, coarse, plan]
        res = {}
        for entry in ("smooth", "smooth_level"):
            us = [_t(u0[lo:hi], gpu) for _, _, _, lo, hi in ranks]
            rr = [torch.full_like(u, float("nan")) for u in us]
            bs = [_t(rhs[lo:hi], gpu) for _, _, _, lo, hi in ranks]

            def body(k):
                m, plan, mgo, lo, hi = ranks[k]
                if entry == "smooth":
                    W.shards[k].schwarz.smooth(plan, us[k], bs[k], rr[k], iterations)
                else:
                    mgo.smooth_level(1, us[k], bs[k], torch.full_like(us[k], float("nan")), rr[k])

            W.run(body)
            torch.cuda.synchronize()
            res[entry] = (np.concatenate([u.cpu().numpy() for u in us]), np.concatenate([x.cpu().numpy() for x in rr]))
        eu = np.abs(res["smooth"][0] - u_ref).max() / np.abs(u_ref - u0).max()
        er = np.abs(res["smooth"][1] - r_ref).max() / np.abs(r_ref).max()
        print("sharded smoother, world %d: u %.3e, r %.3e vs one rank" % (world, eu, er))
        assert np.array_equal(res["smooth"][0], res["smooth_level"][0]) and np.array_equal(res["smooth"][1], res["smooth_level"][1])
        assert eu <= 1e-10 and er <= 1e-10, (eu, er)
    finally:
        for o in keep:
            if hasattr(o, "destroy"):
                o.destroy()
        W.close()


# ---- 4 / 5 / 7: V-cycle, preconditioner, host reads on the family-aligned world-2 split of the level 2 -> 1, p = 2 hierarchy ----------------
def _hierarchy(gpu, world, shard_sub=SUB):
    """world 1: global plans and one-rank Schwarz handles; world 2: per rank the own plans (32 / 32 fine, 4 / 4 coarse elements), the
    h-coarsening transfer of its own families and a sharded handle per level.  Returns (ranks, closer, World or None)"""
    from disco4est_amd import Multigrid, Transfer, mesh as M
    from disco4est_amd.schwarz import Schwarz, SchwarzShardNative
    mp = M.SineMap(0.03)
    dF, dC = np.full(64, 2, np.int32), np.full(8, 2, np.int32)
    keep = []
    if world == 1:
        mF, mC = M.BrickMesh(2, dF), M.BrickMesh(1, dC)
        pF, gF = _global_plan(mF, mp)
        pC, gC = _global_plan(mC, mp)
        sF = Schwarz(mF, gF[2], gF[0], gF[1], 2, *shard_sub)
        sC = Schwarz(mC, gC[2], gC[0], gC[1], 2, *shard_sub)
        T = Transfer(np.ones(8, np.int32), dC, dF.copy())
        mgo = Multigrid([pC, pF], [T])
        keep += [mgo, T, sF, sC, pF, pC]
        return [dict(plan=pF, mg=mgo, sz=[sC, sF], lo=0, hi=mF.local_nodes)], keep, None
    partsF, partsC = [(0, 32), (32, 32)], [(0, 4), (4, 4)]
    WF = _World(2, gpu, lambda rank: SchwarzShardNative(2, dF, partsF, rank, mp, 2, *shard_sub))
    # the coarse handles share the ranks' transports: every rank makes the same sequence of rounds whatever the level
    shC = [SchwarzShardNative(1, dC, partsC, rank, mp, 2, *shard_sub) for rank in range(2)]
    from disco4est_amd import parallel as P
    for sh, tr in zip(shC, WF.transports):
        P.attach_schwarz(sh, tr, gpu)
        sh.schwarz.condensed_copies()
    ranks = []
    for k in range(2):
        mFk, pF, exF = _own_plan(lambda f, c: M.BrickMesh(2, dF, first=f, count=c), mp, partsF, k, WF.transports[k], gpu)
        mCk, pC, exC = _own_plan(lambda f, c: M.BrickMesh(1, dC, first=f, count=c), mp, partsC, k, WF.transports[k], gpu)
        T = Transfer(np.ones(4, np.int32), np.full(4, 2, np.int32), np.full(32, 2, np.int32))
        mgo = Multigrid([pC, pF], [T])
        keep += [exF, exC, mgo, T, pF, pC]
        ranks.append(dict(plan=pF, mg=mgo, sz=[shC[k].schwarz, WF.shards[k].schwarz], lo=mFk.global_nodal_offset,
                          hi=mFk.global_nodal_offset + mFk.local_nodes))
    keep += shC
    return ranks, keep, WF


def _close(keep, W):
    for o in keep:
        if hasattr(o, "destroy"):
            o.destroy()
    if W is not None:
        W.close()


def _problem(seed, n=64 * 27):
    from disco4est_amd import mesh as M
    return M.splitmix64_uniform(seed, n) - 0.5, M.splitmix64_uniform(seed + 1, n) - 0.5


@pytest.mark.parametrize("bottom", ["reuse", "cg"])
def test_vcycle_solve_world_2_against_world_1(gpu, hiplib, bottom):
    """d4est_hip_multigrid_solve, 3 cycles, Schwarz smoother (2 iterations) on both levels: both ranks return world 1's cycle count and
    the r2 history agrees to 1e-9 relative.  Observed on MI355X: 8.7e-15 (reuse_smoother), 1.6e-15 (CG bottom solver)."""
    import torch
    u0, rhs = _problem(51)
    hist = {}
    for world in (1, 2):
        ranks, keep, W = _hierarchy(gpu, world)
        try:
            for st in ranks:
                assert st["mg"].set_smoother_schwarz(st["sz"], 2) == 0
                if bottom == "cg":
                    st["mg"].set_bottom_solver_cg(12, 0.0, 0.0)
                else:
                    st["mg"].set_bottom_solver_reuse_smoother()
                assert st["mg"].ready() == 1
                st["u"], st["rhs"] = _t(u0[st["lo"]:st["hi"]], gpu), _t(rhs[st["lo"]:st["hi"]], gpu)
                st["Au"] = torch.full_like(st["u"], float("nan"))
            body = lambda k: ranks[k]["mg"].solve(ranks[k]["u"], ranks[k]["rhs"], ranks[k]["Au"], 3, 0.0, 0.0)
            hist[world] = W.run(body) if W is not None else [body(0)]
            torch.cuda.synchronize()
        finally:
            _close(keep, W)
    n1, h1 = hist[1][0]
    worst = 0.0
    for n, h in hist[2]:
        assert n == n1 == 3 and len(h) == len(h1)
        worst = max(worst, float(np.max(np.abs(h - h1) / h1)))
    print("sharded V-cycle solve (bottom %s): r2 history %s, worst relative difference to one rank %.3e" % (bottom, list(h1), worst))
    assert np.array_equal(hist[2][0][1], hist[2][1][1])          # one history on every rank
    assert h1[-1] < h1[0]
    assert worst <= 1e-9, worst


def test_fcg_with_the_schwarz_preconditioner_world_2_against_world_1(gpu, hiplib):
    """d4est_hip_fcg_solve with d4est_hip_pc_schwarz_apply, 2 pc iterations (the zero-start store pass, then a pass on r - A z): the
    iteration count of world 1 and its |r_k| history to 1e-9 relative.  Observed on MI355X: 4.4e-15 over 20 iterations."""
    import torch
    from disco4est_amd import PcSchwarz
    u0, rhs = _problem(71)
    res = {}
    for world in (1, 2):
        ranks, keep, W = _hierarchy(gpu, world)
        try:
            for st in ranks:
                st["pc"] = PcSchwarz(st["sz"][1], st["plan"], 2)
                keep.insert(0, st["pc"])
                st["u"], st["rhs"] = _t(u0[st["lo"]:st["hi"]], gpu), _t(rhs[st["lo"]:st["hi"]], gpu)
                st["Au"] = torch.full_like(st["u"], float("nan"))
            body = lambda k: ranks[k]["plan"].fcg_solve(ranks[k]["u"], ranks[k]["rhs"], ranks[k]["Au"], 60, 0.0, 1e-8, pc=ranks[k]["pc"])
            res[world] = W.run(body) if W is not None else [body(0)]
            torch.cuda.synchronize()
        finally:
            _close(keep, W)
    it1, h1 = res[1][0]
    worst = 0.0
    for it, h in res[2]:
        assert it == it1 and 2 <= it < 60
        worst = max(worst, float(np.max(np.abs(h - h1) / h1)))
    print("sharded FCG + Schwarz pc: %d iterations, worst relative difference of |r_k| to one rank %.3e" % (it1, worst))
    assert worst <= 1e-9, worst


def test_no_host_read_at_the_end_of_an_iterate(gpu, hiplib):
    """one smooth_level call (2 smoother iterations) on a sharded handle: the only host reads are the looks at the "still iterating"
    counter before sweep 0 and then every 8th sweep of each iterate -- with 10 count-stopped sweeps that is sweeps 0 and 8: 2 per
    iterate, 4 per call; the public iterate adds the one read of its return value"""
    import torch
    u0, rhs = _problem(61)
    ranks, keep, W = _hierarchy(gpu, 2)
    try:
        for st in ranks:
            assert st["mg"].set_smoother_schwarz(st["sz"], 2) == 0
            st["u"], st["rhs"] = _t(u0[st["lo"]:st["hi"]], gpu), _t(rhs[st["lo"]:st["hi"]], gpu)
            st["Au"], st["r"] = torch.empty_like(st["u"]), torch.empty_like(st["u"])
        before = [st["sz"][1].host_reads() for st in ranks]
        W.run(lambda k: ranks[k]["mg"].smooth_level(1, ranks[k]["u"], ranks[k]["rhs"], ranks[k]["Au"], ranks[k]["r"]))
        after = [st["sz"][1].host_reads() for st in ranks]
        assert [a - b for a, b in zip(after, before)] == [2 * 2, 2 * 2]
        W.run(lambda k: ranks[k]["sz"][1].iterate(ranks[k]["u"], ranks[k]["r"]))
        assert [st["sz"][1].host_reads() - a for st, a in zip(ranks, after)] == [3, 3]
    finally:
        _close(keep, W)


# ---- 6: return codes and defaults ----------------------------------------------------------------------------------------------------------
def test_return_codes(gpu, hiplib):
    import torch
    from disco4est_amd import mesh as M, parallel as P
    from disco4est_amd.schwarz import Schwarz, SchwarzShardNative
    ranks, keep, W = _hierarchy(gpu, 2)
    other = None
    try:
        st = ranks[0]
        mgo = st["mg"]
        mgo.set_bottom_solver_cg(12, 0.0, 0.0)
        # a handle without an exchange on a plan with ghost sides: 4, as before
        mp = M.SineMap(0.03)
        mF = M.BrickMesh(2, np.full(64, 2, np.int32))
        J, rst = mF.geometry(mp)
        plain = Schwarz(mF, mF.build_sides(mp), J, rst, 2, *SUB)
        keep.append(plain)
        assert mgo.set_smoother_schwarz([None, plain], 1) == 4 and mgo.ready() == 0
        # a sharded handle: 0
        assert mgo.set_smoother_schwarz(st["sz"], 1) == 0 and mgo.ready() == 1
        assert mgo.set_smoother_schwarz([None, st["sz"][1]], 1) == 0
        # ... 2 when its own node count is not the plan's (rank 0 of a three-way split owns fewer elements)
        parts3 = P.partition_by_dofs(np.full(64, 2), 3)
        other = SchwarzShardNative(2, np.full(64, 2, np.int32), parts3, 0, mp, 2, *SUB)
        P.attach_schwarz(other, W.transports[0], gpu)
        assert other.own_nodes != st["plan"].local_nodes
        assert mgo.set_smoother_schwarz([None, other.schwarz], 1) == 2 and mgo.ready() == 0
        # ... removing the exchange makes it an extended-mesh handle again: ghost sides are refused
        other.schwarz.set_element_exchange(0, None, None)
        assert other.schwarz.local_nodes == other.mesh.local_nodes
        assert mgo.set_smoother_schwarz([None, other.schwarz], 1) == 4
        # ... 3 when the hierarchy is on another stream than the subdomain plan
        stream = torch.cuda.Stream(device=gpu)
        mgo.set_stream(stream)
        assert mgo.set_smoother_schwarz([None, st["sz"][1]], 1) == 3 and mgo.ready() == 0
        mgo.set_stream(0)
        assert mgo.set_smoother_schwarz([None, st["sz"][1]], 1) == 0 and mgo.ready() == 1
    finally:
        if other is not None:
            other.destroy()
        _close(keep, W)


_ABORT_CHILD = """
import sys
import numpy as np
from disco4est_amd import mesh as M, parallel as P
from disco4est_amd.schwarz import SchwarzShardNative
case = sys.argv[1]
deg = np.full(8, 2, np.int32)
parts = P.partition_by_dofs(deg, 3)
sh = SchwarzShardNative(1, deg, parts, 1, None, 2, 4, 1e-15, 1e-15)
peers, sf, se, rf, re_ = [a.copy() for a in P.element_exchange_lists(sh.schedule, sh.mesh.nodal_stride)]
assert len(peers) == 2 and len(se) > 0 and rf[1] > 0 and rf[2] > rf[1]
if case == "send_wrong_side":
    se[0] = sh.n_own
elif case == "recv_wrong_side":
    re_[0] = 0
elif case == "ghost_unowned":
    rf[2] -= 1
elif case == "ghost_owned_twice":
    re_[rf[1]] = re_[0]
elif case == "peers_unsorted":
    peers = peers[::-1].copy()
sh.schwarz.set_element_exchange(sh.n_own, (peers, sf, se, rf, re_), lambda d, a, b: None)
print("NOT REACHED")
"""


@pytest.mark.parametrize("case,message", [("send_wrong_side", "is not an own element"), ("recv_wrong_side", "is not in the ghost layer"),
                                          ("ghost_unowned", "no peer owns ghost-layer element"), ("ghost_owned_twice", "is owned by ranks"),
                                          ("peers_unsorted", "peers must be ascending")])
def test_malformed_lists_abort(gpu, hiplib, case, message):
    """host-side argument checks ([D4EST_HIP_ABORT], before any launch), seen from a child process"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-c", _ABORT_CHILD, case], capture_output=True, text=True, timeout=120, cwd=root, env=env)
    assert p.returncode != 0 and "NOT REACHED" not in p.stdout, p.stdout
    assert "[D4EST_HIP_ABORT] schwarz_set_element_exchange" in p.stderr and message in p.stderr, p.stderr
