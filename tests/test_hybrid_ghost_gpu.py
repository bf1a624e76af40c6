"""The hybrid operator on SHARDED plans (tuning key 14 = 2, csrc/d4est_hip_direct.hip "ghost-aware"): a conforming side against a ghost
element of the same degree no longer makes an element dirty -- the one-kernel path reads the (+) block from the exchanged ghost trace
buffer -- and apply_lhs / cheby_iterate / cg_eigs order their launches around the exchange hooks (traces, begin, clean elements without a
ghost side, end, clean elements beside a ghost side, dirty flux).

Several virtual ranks in ONE process on one GPU, as in tests/test_parallel_gpu.py: every rank has its own plan, an in-process mailbox
moves the packed trace blocks through the plans' exchange hooks, the gathered result is held to the one-rank oracle
(d4est_laplacian_apply_aij is one path for every mesh and every rank count, src/dGMath/d4est_laplacian.c:318-417).
Tolerances: fp64 re-association only -- rel-inf 1e-12 against the oracle, 1e-13 between the two device paths on the same shards."""
import re
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
RTOL = 1e-12


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


class _Mailbox:
    def __init__(self):
        self.box = {}


class _LocalTransport:
    """one rank after the other: every rank posts first (begin), then each rank's apply re-posts the same blocks and reads its peers'"""

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
    """the ranks run in threads, one library call each (cheby_iterate, cg_eigs): a barrier per exchange / reduction round stands in for the
    message completion -- everybody has posted round k before anybody reads it.  All plans use the null stream, so the device work is
    ordered as the host calls are.  The reduction adds in rank order on every rank (what an allreduce guarantees: one result everywhere)."""

    def __init__(self, rank, world, mailbox, barrier):
        self.rank, self.world, self.mb, self.barrier = rank, world, mailbox, barrier
        self.k_x = self.k_r = 0

    def start(self, send_buf, recv_buf):
        for p, t in send_buf.items():
            self.mb.box[("x", self.rank, p, self.k_x)] = t.clone()
        return recv_buf

    def finish(self, recv_buf):
        self.barrier.wait()
        for p, t in recv_buf.items():
            t.copy_(self.mb.box[("x", p, self.rank, self.k_x)])
        self.k_x += 1

    def allreduce_sum(self, t):
        self.mb.box[("r", self.rank, self.k_r)] = t.clone()
        self.barrier.wait()
        tot = self.mb.box[("r", 0, self.k_r)].clone()
        for r in range(1, self.world):
            tot += self.mb.box[("r", r, self.k_r)]
        t.copy_(tot)
        self.k_r += 1


def _counts(path):
    """(C, G, D) of 'hybrid...: direct+volume on C clean elements (G beside ghost sides), two-phase on D'"""
    m = re.search(r"on (\d+) clean elements \((\d+) beside ghost sides\), two-phase on (\d+)$", path)
    assert path.startswith("hybrid") and m, path
    return tuple(int(x) for x in m.groups())


def _shards(make, parts, mp, key14, gpu, transport, tune=()):
    """one plan per rank, wired to its transport; make(first, count) -> the rank's mesh"""
    from disco4est_amd import Plan, parallel as P
    ranks = []
    for r, (first, count) in enumerate(parts):
        m = make(first, count)
        J, rst = m.geometry(mp) if mp is not None else m.geometry()
        s = m.build_sides(mp) if mp is not None else m.build_sides()
        plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, 0)
        plan.set_tuning(14, key14)
        for k, v in tune:
            plan.set_tuning(k, v)
        plan.set_geometry(J, rst)
        plan.set_faces(s, 10.0, 0)
        ex = P.attach(plan, m, s, parts, transport(r), gpu)
        ranks.append({"m": m, "s": s, "plan": plan, "ex": ex})
    return ranks


def _gathered_apply_lhs(ranks, fields, n_global, gpu):
    """apply_lhs of every rank through its exchange hooks; the peers' blocks wait in the mailbox (posted up front from the same u)"""
    import torch
    for st, u in zip(ranks, fields):
        st["u"] = _t(u, gpu)
        tr = torch.empty(max(st["plan"].trace_size, 1), dtype=torch.float64, device=gpu)
        st["plan"].compute_face_traces(st["u"], tr)
        st["ex"].begin(tr)
    got = np.zeros(n_global)
    for st in ranks:
        Au = torch.full_like(st["u"], float("nan"))
        st["plan"].apply_lhs(st["u"], Au)
        m = st["m"]
        got[m.global_nodal_offset:m.global_nodal_offset + m.local_nodes] = Au.cpu().numpy()
    assert np.isfinite(got).all()
    return got


def _parity(make, parts, mp, gpu, oracle, tune=(), check=None):
    """key 14 = 2 against the oracle (1e-12) and against key 14 = 0 on the same shards (1e-13); returns the ranks' (C, G, D)"""
    mg = make(0, None)
    Jg, rstg = mg.geometry(mp) if mp is not None else mg.geometry()
    sg = mg.build_sides(mp) if mp is not None else mg.build_sides()
    ug = mg.field(mp) if mp is not None else mg.field()
    ref = oracle.apply_aij(mg, Jg, rstg, sg, ug, nthreads=8)
    res, counts = {}, []
    for key14 in (2, 0):
        mb = _Mailbox()
        ranks = _shards(make, parts, mp, key14, gpu, lambda r: _LocalTransport(r, mb), tune)
        if key14 == 2:
            for st in ranks:
                counts.append(_counts(st["plan"].face_path()))
                if check:
                    check(st, counts[-1])
        else:
            for st in ranks:
                assert not st["plan"].face_path().startswith("hybrid")
        fields = [st["m"].field(mp) if mp is not None else st["m"].field() for st in ranks]
        res[key14] = _gathered_apply_lhs(ranks, fields, ref.size, gpu)
        for st in ranks:
            st["plan"].destroy()
    e2, e0, e20 = _rel(res[2], ref), _rel(res[0], ref), _rel(res[2], res[0])
    print("hybrid ghost parity: key14=2 vs oracle %.3e, key14=0 vs oracle %.3e, 2 vs 0 %.3e, (C, G, D) per rank %s" % (e2, e0, e20, counts))
    assert e2 <= RTOL and e20 <= 1e-13, (e2, e0, e20)
    return counts


def _brick(level, deg_global):
    from disco4est_amd import mesh as M
    return lambda first, count: M.BrickMesh(level, deg_global, first=first, count=count)


# ---- 1 / 2: one degree, conforming (N = 4 with lane guards, N = 8 the FULL instance), straight and curved ---------------------------------
@pytest.mark.parametrize("deg,world,curved", [(3, 2, False), (3, 3, False), (7, 2, False), (7, 3, False), (3, 2, True)])
def test_one_degree_shards(gpu, hiplib, oracle, deg, world, curved):
    from disco4est_amd import mesh as M, parallel as P
    deg_global = np.full(64, deg)
    parts = P.partition_by_dofs(deg_global, world)
    counts = _parity(_brick(2, deg_global), parts, M.SineMap(0.04) if curved else None, gpu, oracle)
    for (C, G, D), (first, count) in zip(counts, parts):
        assert G > 0 and C == count and D == 0, (C, G, D)     # every side is conforming against the same degree: nobody is dirty


# ---- 3: mixed degree across the cut ------------------------------------------------------------------------------------------------------
def _expected_mixed(m, s, mixed_aware):
    """(clean, ghost-adjacent clean, elements with a different-degree ghost neighbour) of a conforming brick shard, deg_quad = deg"""
    nbr, gdeg = s["side_nbr"], s["ghost_deg"]
    clean = gadj = ndiff = 0
    for e in range(m.n_elements):
        ok, g, diff = True, False, False
        for f in range(6):
            n = int(nbr[6 * e + f])
            if n == -1:
                continue
            if n <= -2:
                same = int(gdeg[-(n + 2)]) == int(m.deg[e])
                g = g or same
                diff = diff or not same
                ok = ok and same
            else:
                ok = ok and (m.deg[n] == m.deg[e] or (mixed_aware and m.deg[n] < m.deg[e]))
        clean += ok
        gadj += ok and g
        ndiff += diff
    return clean, gadj, ndiff


def _mixed_case():
    """p = 3 for x < 1/2, p = 5 beyond, cut at element 28 of the Morton order (inside a p = 5 octant)"""
    from disco4est_amd import mesh as M
    ijk = M.morton_order(2)
    return np.where(ijk[:, 0] < 2, 3, 5).astype(np.int32), [(0, 28), (28, 36)]


@pytest.mark.parametrize("mixed_aware,stream", [(True, 0), (False, 0), (True, 1), (False, 1)])
def test_mixed_degree_across_the_cut(gpu, hiplib, oracle, monkeypatch, mixed_aware, stream):
    """p = 3 for x < 1/2, p = 5 beyond; the cut at element 28 of the Morton order runs inside a p = 5 octant: it separates p = 5 from p = 5
    elements (ghost-aware sides) and p = 3 from p = 5 elements (dirty on both ranks).  With the mixed-aware form a p = 5 element may have
    a lower-degree LOCAL neighbour, read from the trace array, and a ghost side, read from the ghost buffer, at once (the VOL & 32
    instances; without it the plain ones).  stream = 1 (tuning key 12) runs the stream-mode twins of either."""
    from disco4est_amd import mesh as M
    if not mixed_aware:
        monkeypatch.setenv("D4EST_HIP_HYBRID_NO_MIXED", "1")
    deg_global, parts = _mixed_case()
    seen = {"diff": 0, "same": 0}

    def check(st, cgd):
        C, G, D = cgd
        clean, gadj, ndiff = _expected_mixed(st["m"], st["s"], mixed_aware)
        seen["diff"] += ndiff
        seen["same"] += gadj
        assert (C, G, D) == (clean, gadj, st["m"].n_elements - clean), (cgd, clean, gadj, ndiff)
        assert D >= ndiff
        if mixed_aware:
            assert "mixed-aware" in st["plan"].face_path()

        assert st["plan"].stream_mode() == stream

    _parity(_brick(2, deg_global), parts, M.SineMap(0.04), gpu, oracle, tune=((12, stream),), check=check)
    assert seen["diff"] > 0 and seen["same"] > 0


# ---- 4: a hanging face cut by the shard boundary -----------------------------------------------------------------------------------------
def test_hanging_face_cut_by_the_shard_boundary(gpu, hiplib, oracle):
    from disco4est_amd import mesh as M, parallel as P
    refine = np.zeros(8, dtype=bool)
    refine[2] = True
    ne = M.HangingBrickMesh(1, refine, 3).global_elements
    deg_global = np.full(ne, 3)
    parts = P.partition_by_dofs(deg_global, 2)
    crossing = [0]

    def check(st, cgd):
        # One degree, one refined octant, hp split on: on one rank EVERY element is clean (hanging-aware form, tests/test_hybrid_gpu.py
        # "hanging_p4").  So on a shard the dirty elements are exactly those with a hanging side that the cut runs through -- a small side
        # whose big neighbour is a ghost, or a big side with a ghost among its four small neighbours -- and the ghost-adjacent clean
        # elements are the others with a conforming ghost side (same degree everywhere).  (C, G, D) from the side tables:
        s, m = st["s"], st["m"]
        hang, nbr, n4 = s["side_hang"], s["side_nbr"], s["side_nbr4"]
        cut, conf_ghost = set(), set()
        for sd in range(6 * m.n_elements):
            if (hang[sd] == 2 and nbr[sd] <= -2) or (hang[sd] == 1 and (n4[4 * sd:4 * sd + 4] <= -2).any()):
                cut.add(sd // 6)
            elif hang[sd] == 0 and nbr[sd] <= -2:
                conf_ghost.add(sd // 6)
        crossing[0] += len(cut)
        want = (m.n_elements - len(cut), len(conf_ghost - cut), len(cut))
        assert cgd == want, (cgd, want, sorted(cut))   # D is exactly the cut elements: none of them is in C

    _parity(lambda first, count: M.HangingBrickMesh(1, refine, deg_global, first=first, count=count), parts, M.SineMap(0.04), gpu, oracle,
            tune=((13, 1),), check=check)
    assert crossing[0] > 0, "the partition must cut a hanging face"


# ---- 5: orientation ----------------------------------------------------------------------------------------------------------------------
def test_oriented_tree_face_between_the_ranks(gpu, hiplib, oracle):
    """two trees glued with a non-trivial face orientation, one tree per rank: every ghost side is an oriented tree face"""
    from disco4est_amd import forest as F, mesh as M
    from tests.test_forest import TRIPLES
    trip, rots = [(t, r) for t, r in sorted(TRIPLES.items()) if t[2] != 0 and F.reference_reorientation_is_consistent(*t)][0]
    conn = F.Connectivity.rotated_pair(*rots)
    mp = F.TrilinearMap(conn, M.SineMap(0.03))
    oriented = [0]

    def check(st, cgd):
        s = st["s"]
        oriented[0] += int(((s["side_nbr"] <= -2) & (s["side_reorder"] != 0)).sum())
        assert cgd[1] > 0

    _parity(lambda first, count: F.ForestMesh(conn, 1, 3, mp, first=first, count=count), [(0, 8), (8, 8)], None, gpu, oracle, check=check)
    assert oriented[0] > 0, trip


# ---- 6: the smoother, ranks in lockstep --------------------------------------------------------------------------------------------------
def _lockstep(world, parts, deg_global, key10, u0, rhs, lmin, lmax, gpu, what, check=None):
    """cheby_iterate (5 iterations) or cg_eigs of every rank at once, one thread per rank; returns the gathered iterate / the ranks' bounds"""
    import torch
    mb = _Mailbox()
    barrier = threading.Barrier(world, timeout=120)
    ranks = _shards(_brick(2, deg_global), parts, None, 2, gpu, lambda r: _LockstepTransport(r, world, mb, barrier), tune=((10, key10),))
    out, errs = [None] * world, []
    for st in ranks:
        assert world == 1 or _counts(st["plan"].face_path())[1] > 0
        if check:
            check(st)
        lo, n = st["m"].global_nodal_offset, st["m"].local_nodes
        st["u"], st["rhs"] = _t(u0[lo:lo + n], gpu), _t(rhs[lo:lo + n], gpu)
        st["Au"], st["r"] = torch.empty_like(st["u"]), torch.empty_like(st["u"])

    def run(r):
        st = ranks[r]
        try:
            torch.cuda.set_device(gpu)
            if what == "cheby":
                st["plan"].cheby_iterate(st["u"], st["rhs"], st["Au"], st["r"], 5, lmin, lmax, 1)
                out[r] = (st["u"].cpu().numpy(), st["r"].cpu().numpy())
            else:
                out[r] = st["plan"].cg_eigs(st["u"], st["rhs"], st["Au"], 5)[0]
        except BaseException as e:   # (a rank that fails must not leave the others waiting)
            errs.append(e)
            barrier.abort()

    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for st in ranks:
        st["plan"].destroy()
    assert not errs, errs
    if what == "cheby":
        return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])
    return out


def test_smoothers_in_lockstep(gpu, hiplib, oracle):
    """5 Chebyshev iterations and cg_eigs on the one-degree mesh: world 1, 2, 3 give the oracle's iterate; the update fused into the
    operator kernels (key 10 = -1) is bit-identical to the separate update kernel (key 10 = 0) on the same shards"""
    from disco4est_amd import mesh as M, parallel as P
    deg_global = np.full(64, 3)
    mg = M.BrickMesh(2, deg_global)
    Jg, rstg = mg.geometry(None); sg = mg.build_sides(None)
    u0 = M.splitmix64_uniform(31, mg.local_nodes)
    rhs = M.splitmix64_uniform(32, mg.local_nodes) - 0.5
    oracle.set_operator(mg, Jg, rstg, sg, 10.0, 0)
    lmax_ref, _ = oracle.cg_eigs(np.zeros(mg.local_nodes), rhs, 5)
    lmin, lmax = lmax_ref / 30.0, lmax_ref
    u_ref, r_ref = oracle.cheby_iterate(u0, rhs, 5, lmin, lmax, 1)
    got = {}
    for world in (1, 2, 3):
        parts = P.partition_by_dofs(deg_global, world)
        u_f, r_f = _lockstep(world, parts, deg_global, -1, u0, rhs, lmin, lmax, gpu, "cheby")
        u_s, r_s = _lockstep(world, parts, deg_global, 0, u0, rhs, lmin, lmax, gpu, "cheby")
        assert np.array_equal(u_f, u_s) and np.array_equal(r_f, r_s), (world, _rel(u_f, u_s))
        bounds = _lockstep(world, parts, deg_global, -1, np.zeros_like(u0), rhs, lmin, lmax, gpu, "eigs")
        eu, er, eb = _rel(u_f, u_ref), _rel(r_f, r_ref), max(abs(b - lmax_ref) for b in bounds) / lmax_ref
        print("world %d: cheby u %.3e, r %.3e, cg_eigs bound %.3e vs the oracle" % (world, eu, er, eb))
        assert len(set(bounds)) == 1                       # one bound on every rank
        assert eu <= RTOL and er <= RTOL and eb <= RTOL, (world, eu, er, eb)
        got[world] = u_f
    for world in (2, 3):
        assert _rel(got[world], got[1]) <= RTOL


@pytest.mark.parametrize("mixed_aware", [True, False])
def test_fused_update_on_mixed_degree_shards(gpu, hiplib, oracle, monkeypatch, mixed_aware):
    """5 Chebyshev iterations on the shards of the mixed-degree case: both ranks have ghost-adjacent clean elements AND dirty elements, so
    with key 10 = -1 the update rides in the interior clean launches, in the ghost-adjacent ones (mixed-aware: the FUSE instances with
    VOL & 32) and in the flux kernels of the dirty list.  Bit-identical to the separate update kernel (key 10 = 0) -- the contract of key 10 --
    and the oracle's iterate to 1e-12."""
    from disco4est_amd import mesh as M
    if not mixed_aware:
        monkeypatch.setenv("D4EST_HIP_HYBRID_NO_MIXED", "1")
    deg_global, parts = _mixed_case()
    mg = M.BrickMesh(2, deg_global)
    Jg, rstg = mg.geometry(None); sg = mg.build_sides(None)
    u0 = M.splitmix64_uniform(41, mg.local_nodes)
    rhs = M.splitmix64_uniform(42, mg.local_nodes) - 0.5
    oracle.set_operator(mg, Jg, rstg, sg, 10.0, 0)
    lmax, _ = oracle.cg_eigs(np.zeros(mg.local_nodes), rhs, 5)
    lmin = lmax / 30.0
    u_ref, r_ref = oracle.cheby_iterate(u0, rhs, 5, lmin, lmax, 1)

    def check(st):
        C, G, D = _counts(st["plan"].face_path())
        assert G > 0 and D > 0 and C > G, (C, G, D)            # interior clean, ghost-adjacent clean and dirty launches all run
        assert ("mixed-aware" in st["plan"].face_path()) == mixed_aware

    u_f, r_f = _lockstep(2, parts, deg_global, -1, u0, rhs, lmin, lmax, gpu, "cheby", check)
    u_s, r_s = _lockstep(2, parts, deg_global, 0, u0, rhs, lmin, lmax, gpu, "cheby", check)
    eu, er = _rel(u_f, u_ref), _rel(r_f, r_ref)
    print("mixed-degree shards: fused vs separate update %.3e, cheby u %.3e, r %.3e vs the oracle" % (_rel(u_f, u_s), eu, er))
    assert np.array_equal(u_f, u_s) and np.array_equal(r_f, r_s), _rel(u_f, u_s)
    assert eu <= RTOL and er <= RTOL, (eu, er)


# ---- 7: unchanged defaults ---------------------------------------------------------------------------------------------------------------
def test_defaults_are_unchanged(gpu, hiplib):
    from disco4est_amd import Plan, mesh as M, parallel as P
    deg_global = np.full(64, 3)
    parts = P.partition_by_dofs(deg_global, 2)
    for key14 in (-1, 1):
        mb = _Mailbox()
        for st in _shards(_brick(2, deg_global), parts, None, key14, gpu, lambda r: _LocalTransport(r, mb)):
            assert st["plan"].face_path() == "two-phase"
            st["plan"].destroy()
    # one rank: value 2 is value 1
    ijk = M.morton_order(2)
    m = M.BrickMesh(2, np.where(ijk[:, 0] < 2, 2, 5).astype(np.int32))
    J, rst = m.geometry(None); s = m.build_sides(None)
    paths = []
    for key14 in (1, 2):
        plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, 0)
        plan.set_tuning(14, key14)
        plan.set_geometry(J, rst); plan.set_faces(s, 10.0, 0)
        paths.append(plan.face_path())
        plan.destroy()
    assert paths[0] == paths[1] and paths[0].startswith("hybrid") and "ghost" not in paths[0], paths


# ---- 8: p >= 8 -- the multi-wave whole-operator kernel has no ghost-aware form: ghost-adjacent elements stay two-phase ---------------------
@pytest.mark.parametrize("level", [1, 2])
def test_p8_ghost_adjacent_elements_stay_dirty(gpu, hiplib, oracle, level):
    """level 1: every element of either shard has a ghost side, so nobody is clean and the plan must not report the hybrid form at all;
    level 2: the interior elements are clean (operator_mw_kernel), every ghost-adjacent one is in D"""
    import torch
    from disco4est_amd import mesh as M, parallel as P
    deg_global = np.full(8 ** level, 8)
    parts = P.partition_by_dofs(deg_global, 2)
    make = _brick(level, deg_global)
    mg = make(0, None)
    Jg, rstg = mg.geometry(None); sg = mg.build_sides(None)
    ref = oracle.apply_aij(mg, Jg, rstg, sg, mg.field(), nthreads=8)
    mb = _Mailbox()
    ranks = _shards(make, parts, None, 2, gpu, lambda r: _LocalTransport(r, mb))
    for st in ranks:
        nbr = st["s"]["side_nbr"].reshape(-1, 6)
        n_adj = int((nbr <= -2).any(axis=1).sum())
        path = st["plan"].face_path()
        if level == 1:
            assert n_adj == st["m"].n_elements and not path.startswith("hybrid"), path
        else:
            C, G, D = _counts(path)
            assert G == 0 and D == n_adj and C == st["m"].n_elements - n_adj and C > 0, path
    got = _gathered_apply_lhs(ranks, [st["m"].field() for st in ranks], ref.size, gpu)
    for st in ranks:
        st["plan"].destroy()
    assert _rel(got, ref) <= RTOL, _rel(got, ref)
