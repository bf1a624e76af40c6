"""GPU tests of the hp-AMR step on several ranks (d4est_hip_par_amr_set_comm / _stats_global / _repartition / _repartition_field,
parallel.attach_amr) against tests/ref_amr_parallel.py (pinned by tests/test_ref_amr_parallel.py).

Several virtual ranks in one process on one GPU, threads in lock-step on the null stream as in tests/test_schwarz_sharded_gpu.py: one
barrier per allreduce / sendrecv round (with a time limit), barrier.abort() when a rank raises, joins with a time limit -- a stuck rank
fails the test.  The transport counts allreduce calls, rounds and non-empty messages.

Bounds.  Maximum and percentile: the bits of the sorted concatenation (a selection, no arithmetic).  Total: |got - ref| <= G 2^-52 total --
the terms are non-negative, every partial sum is at most the total, so each of the two summation orders (G - 1 additions each) is within
(G - 1) 2^-53 total (1 + O(G 2^-53)) of the exact sum.  Mean: got[0] / G exactly (one IEEE division).  Degrees, predictor and fields after
a repartition: copies, bit-equal.  The field after mark -> set_balance -> interpolate_field on the new shards: tests/test_amr_gpu.py's
FIELD_RTOL per new element against the dense two-stage reference on the GLOBAL grid (the shards' work lists may pick other compile-time
instances than one rank's, so no bit-equality with a one-rank run is asked)."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from tests import dense_transfer as DT
from tests import ref_amr as R
from tests import ref_amr_parallel as RP
from tests.test_amr_gpu import FIELD_RTOL
from tests.test_schwarz_sharded_gpu import _LockstepTransport, _Mailbox, _run_lockstep

pytestmark = pytest.mark.gpu
PASSES = 8                         # digit passes of the radix select = allreduce calls per stats_global
PERCENTILES = (1, 5, 10, 50, 99, 100)
GAMMA_H, GAMMA_P, GAMMA_N = 0.25, 0.1, 0.9
MAXDEG = 4


def _dev(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(gpu)


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def _uniform(seed, n):
    from disco4est_amd import mesh as M
    return M.splitmix64_uniform(seed, n)


class _CountingTransport(_LockstepTransport):
    def __init__(self, rank, world, mailbox, barrier):
        super().__init__(rank, world, mailbox, barrier)
        self.n_allreduce = self.n_rounds = self.n_messages = 0

    def round(self, send_buf, recv_buf):
        self.n_rounds += 1
        self.n_messages += sum(1 for t in send_buf.values() if t.numel())
        super().round(send_buf, recv_buf)

    def allreduce_sum(self, t):
        self.n_allreduce += 1
        super().allreduce_sum(t)


class _Ranks:
    """one Amr per virtual rank on a lock-step transport"""

    def __init__(self, gpu, deg_per_rank, max_degree=MAXDEG, initial_pred=1.0):
        from disco4est_amd import Amr, parallel as P
        self.gpu, self.world = gpu, len(deg_per_rank)
        self.barrier = threading.Barrier(self.world, timeout=60)
        mb = _Mailbox()
        self.transports = [_CountingTransport(r, self.world, mb, self.barrier) for r in range(self.world)]
        self.amrs = [Amr(np.asarray(d, np.int32), max_degree, initial_pred) for d in deg_per_rank]
        self.hooks = [P.attach_amr(a, t, gpu) for a, t in zip(self.amrs, self.transports)]

    def run(self, body):
        import torch
        out = _run_lockstep(self.world, self.barrier, self.gpu, body)
        torch.cuda.synchronize()
        return out

    def close(self):
        for a in self.amrs:
            a.destroy()


# ---- 1: the statistics ------------------------------------------------------------------------------------------------------------------
def _eta2(G, seed):
    """non-negative, magnitudes 1e-300 .. 1e+10, with ties, exact zeros, and a block of duplicates of 1.0 and of its predecessor: equal
    keys next to keys that differ from them in EVERY digit (0x3ff0000000000000 / 0x3fefffffffffffff), placed where the upper percentiles
    land (about 3 % of the other values are above 1)"""
    v = 10.0 ** (-300.0 + 310.0 * _uniform(seed, G))
    if G >= 5:
        v[1] = 0.0
        v[3] = v[0]
    if G >= 257:
        v[10:40] = 1.0
        v[40:70] = np.nextafter(1.0, 0.0)
        v[70:80] = 0.0
        v[80:90] = v[5]
        v[90] = 1e-300
        v[91] = 1e+10
    return v


def _splits(world, G):
    """uneven local sizes, one split with an EMPTY rank in the middle or at an end"""
    if world == 2:
        return [[G // 3, G - G // 3], [G, 0]]
    a = G // 4
    return [[a, G - a - (G + 1) // 2, (G + 1) // 2], [G - G // 5, 0, G // 5]]


@pytest.mark.parametrize("G", [1, 2, 5, 257, 1003])
@pytest.mark.parametrize("world", [2, 3])
def test_stats_global(gpu, hiplib, world, G):
    import torch
    eta2 = _eta2(G, 1000 + G)
    saw_k0 = False
    for sizes in _splits(world, G):
        assert sum(sizes) == G and len(sizes) == world
        cuts = np.concatenate([[0], np.cumsum(sizes)])
        parts = [eta2[cuts[r]:cuts[r + 1]] for r in range(world)]
        W = _Ranks(gpu, [np.full(n, 2) for n in sizes])
        try:
            d_eta = [_dev(p, gpu) for p in parts]
            d_stats = [[torch.full((4,), float("nan"), dtype=torch.float64, device=gpu) for _ in range(2 * len(PERCENTILES))] for _ in range(world)]

            def body(r):
                for i, pct in enumerate(PERCENTILES):          # every call twice
                    W.amrs[r].stats_global(d_eta[r], pct, d_stats[r][2 * i])
                    W.amrs[r].stats_global(d_eta[r], pct, d_stats[r][2 * i + 1])

            W.run(body)
            # the hook is called once per digit pass, whatever n is; no sendrecv round
            assert [t.n_allreduce for t in W.transports] == [PASSES * 2 * len(PERCENTILES)] * world
            assert [t.n_rounds for t in W.transports] == [0] * world
            for i, pct in enumerate(PERCENTILES):
                ref = RP.stats_global(parts, pct)
                k = RP.global_id_from_end(G, pct)
                saw_k0 |= k == 0
                for r in range(world):
                    got = d_stats[r][2 * i].cpu().numpy()
                    again = d_stats[r][2 * i + 1].cpu().numpy()
                    print("world %d G %d sizes %s pct %d rank %d: total %.17g (ref %.17g) mean %.17g max %.17g at_pct %.17g (k = %d)"
                          % (world, G, sizes, pct, r, got[0], ref[0], got[1], got[2], got[3], k))
                    assert np.array_equal(_bits(got), _bits(again)), "two identical calls differ"
                    assert np.array_equal(got[2:], np.asarray(ref[2:])) and np.array_equal(_bits(got[2:]), _bits(ref[2:]))
                    assert abs(got[0] - ref[0]) <= G * 2.0 ** -52 * ref[0]
                    assert got[1] == got[0] / G
                    if k == 0:
                        assert got[3] == -1.0
            for r in range(world):
                assert np.array_equal(d_eta[r].cpu().numpy(), parts[r]), "eta2 was modified"
        finally:
            W.close()
    assert saw_k0 == (G < 100)


def test_stats_global_without_elements_anywhere(gpu, hiplib):
    import torch
    W = _Ranks(gpu, [np.zeros(0), np.zeros(0)])
    try:
        st = [torch.full((4,), float("nan"), dtype=torch.float64, device=gpu) for _ in range(2)]
        empty = torch.empty(0, dtype=torch.float64, device=gpu)
        W.run(lambda r: W.amrs[r].stats_global(empty, 5, st[r]))
        for s in st:
            assert s.cpu().numpy().tolist() == [0.0, -1.0, -1.0, -1.0]
    finally:
        W.close()


# ---- 2: the same numbers on any number of ranks -------------------------------------------------------------------------------------------
def test_rank_count_invariance(gpu, hiplib):
    import torch
    from disco4est_amd import Amr
    G = 257
    eta2 = _eta2(G, 77)
    res = {}
    for world in (1, 2, 3):
        sizes = [G] if world == 1 else _splits(world, G)[0]
        cuts = np.concatenate([[0], np.cumsum(sizes)])
        d_eta = [_dev(eta2[cuts[r]:cuts[r + 1]], gpu) for r in range(world)]
        st = [[torch.full((4,), float("nan"), dtype=torch.float64, device=gpu) for _ in PERCENTILES] for _ in range(world)]
        if world == 1:            # no set_comm: world 1, no hook
            amr = Amr(np.full(G, 2, np.int32), MAXDEG, 1.0)
            for i, pct in enumerate(PERCENTILES):
                amr.stats_global(d_eta[0], pct, st[0][i])
            torch.cuda.synchronize()
            amr.destroy()
        else:
            W = _Ranks(gpu, [np.full(n, 2) for n in sizes])
            try:
                W.run(lambda r: [W.amrs[r].stats_global(d_eta[r], pct, st[r][i]) for i, pct in enumerate(PERCENTILES)])
            finally:
                W.close()
        res[world] = [[s.cpu().numpy() for s in row] for row in st]
    for i, pct in enumerate(PERCENTILES):
        ref = RP.stats_global([eta2], pct)
        one = res[1][0][i]
        assert np.array_equal(_bits(one[2:]), _bits(ref[2:])), pct
        for world in (2, 3):
            for row in res[world]:
                assert np.array_equal(_bits(row[i][2:]), _bits(one[2:])), (world, pct)
                assert np.array_equal(_bits(row[i]), _bits(res[world][0][i])), "the ranks of one world disagree"


# ---- the grid of tests 3 - 5 -----------------------------------------------------------------------------------------------------------------
N_EL = 41


def _level0():
    """41 elements of degree 1 .. 4; eta2 around 1 with the elements of degree 4 below every threshold used here"""
    deg0 = (np.arange(N_EL) * 7 % 4 + 1).astype(np.int32)
    eta2 = 0.5 + _uniform(31, N_EL)
    eta2[deg0 == 4] *= 1e-3
    return deg0, eta2


def _level1():
    """the global state after one step without h-refinement: mark at the median (marked: p-branch, degree + 1, predictor gamma_p eta2;
    others gamma_n * initial), balance log = log, advance: degrees 1 .. 4, a predictor that differs from element to element"""
    deg0, eta2 = _level0()
    thr = float(np.median(eta2))
    log, pred, branch = R.mark(eta2, [1e30] * N_EL, deg0, MAXDEG, thr, 1.0, GAMMA_H, GAMMA_P, GAMMA_N)
    assert set(branch) == {"p", "n"} and min(log) >= 1 and set(log) == {1, 2, 3, 4}
    pred = R.advance_predictor(pred, log, list(log), GAMMA_H)
    return deg0, eta2, thr, np.asarray(log, np.int32), np.asarray(pred, np.float64)


def _ranks_at_level1(gpu, first):
    """the shards of `first` brought to level 1 through the device calls; returns (_Ranks, deg1, pred1)"""
    deg0, eta2, thr, deg1, pred1 = _level1()
    W = _Ranks(gpu, RP.shard_elements(deg0, first), initial_pred=1e30)
    d_thr = _dev([thr], gpu)
    for a, e in zip(W.amrs, RP.shard_elements(eta2, first)):
        a.mark_smooth_pred(_dev(e, gpu), d_thr, 1.0, GAMMA_H, GAMMA_P, GAMMA_N)
        a.set_balance(a.get_refinement_log())
        a.advance()
    assert np.array_equal(np.concatenate([a.get_predictor() for a in W.amrs]), pred1)
    return W, deg1, pred1


def _degrees(amr, gpu):
    """the current degrees: the log of a mark call that marks nothing, with gamma_n = 1 (the predictor keeps its bits)"""
    n = amr.n_elements
    amr.mark_smooth_pred(_dev(np.zeros(n), gpu), _dev([1.0], gpu), 1.0, GAMMA_H, GAMMA_P, 1.0)
    return amr.get_refinement_log()


# ---- 3: marking with the global threshold ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,factor", [(3, 1.0), (1, 0.75)])
def test_mark_with_the_global_threshold(gpu, hiplib, which, factor):
    """stats_dev + 3 (percentile marker) and stats_dev + 1 (sigma * mean) of the global call on every shard against ONE Amr over the whole
    list that is handed the same threshold value"""
    import torch
    from disco4est_amd import Amr
    deg0, eta2 = _level0()
    first = np.asarray([0, 9, 9, N_EL])
    W = _Ranks(gpu, RP.shard_elements(deg0, first))
    whole = Amr(deg0, MAXDEG, 1.0)
    try:
        d_eta = [_dev(e, gpu) for e in RP.shard_elements(eta2, first)]
        st = [torch.full((4,), float("nan"), dtype=torch.float64, device=gpu) for _ in range(3)]

        def body(r):
            W.amrs[r].stats_global(d_eta[r], 25, st[r])
            W.amrs[r].mark_smooth_pred(d_eta[r], st[r][which:which + 1], factor, GAMMA_H, GAMMA_P, GAMMA_N)

        W.run(body)
        thr = st[0].cpu().numpy()[which]
        assert thr == RP.stats_global([eta2], 25)[which] or which == 1
        whole.mark_smooth_pred(_dev(eta2, gpu), _dev([thr], gpu), factor, GAMMA_H, GAMMA_P, GAMMA_N)
        log = np.concatenate([a.get_refinement_log() for a in W.amrs])
        pred = np.concatenate([a.get_predictor() for a in W.amrs])
        assert np.array_equal(log, whole.get_refinement_log())
        assert np.array_equal(_bits(pred), _bits(whole.get_predictor()))
        marked = int((log != deg0).sum())
        assert 0 < marked < N_EL, marked
        if which == 3:            # the percentile marker marks exactly the k largest (no ties in this eta2)
            assert marked == RP.global_id_from_end(N_EL, 25)
    finally:
        whole.destroy()
        W.close()


# ---- 4: repartition ------------------------------------------------------------------------------------------------------------------------------
def _repartition_cases():
    from disco4est_amd import parallel as P
    deg1 = _level1()[3]
    by_el = RP.by_elements(N_EL, 3)
    by_dofs = P.first_of(P.partition_by_dofs(deg1, 3))
    return {
        "elements to dofs": (by_el, by_dofs),
        "a rank left empty": (by_el, np.asarray([0, 20, 20, N_EL])),
        "a rank receives from two peers": (np.asarray([0, 10, 31, N_EL]), np.asarray([0, 5, 36, N_EL])),
        "from an empty rank, sends to two peers": (np.asarray([0, 0, N_EL, N_EL]), by_el),
        "old == new": (by_dofs, by_dofs.copy()),
    }


@pytest.mark.parametrize("name", ["elements to dofs", "a rank left empty", "a rank receives from two peers",
                                  "from an empty rank, sends to two peers", "old == new"])
def test_repartition(gpu, hiplib, name):
    import torch
    old, new = _repartition_cases()[name]
    msgs = RP.messages(old, new)
    if name == "elements to dofs":
        assert not np.array_equal(old, new) and msgs
    if name == "a rank receives from two peers":
        assert sorted(s for s, r, _, _ in msgs if r == 1) == [0, 2]
    W, deg1, pred1 = _ranks_at_level1(gpu, old)
    try:
        off = RP.node_offsets(deg1)
        fields = [_uniform(41, off[-1]) - 0.5, _uniform(42, off[-1]) - 0.5]
        f_old = [[_dev(s, gpu) for s in RP.shard_nodes(f, deg1, old)] for f in fields]
        for r in range(3):
            assert W.amrs[r].local_nodes == f_old[0][r].numel()
        f_new = [[None] * 3, [None] * 3]
        nodes = [None] * 3

        def body(r):
            a = W.amrs[r]
            nodes[r] = a.repartition(old, new)
            for j in range(2):
                f_new[j][r] = torch.full((nodes[r],), float("nan"), dtype=torch.float64, device=gpu)
                a.repartition_field(f_old[j][r], f_new[j][r])

        W.run(body)
        # one round for the state and one per field where the partitions differ, none otherwise; the messages are the slices' count
        want_rounds = 0 if np.array_equal(old, new) else 3
        assert [t.n_rounds for t in W.transports] == [want_rounds] * 3
        assert [t.n_messages for t in W.transports] == [3 * sum(1 for s, _, _, _ in msgs if s == r) for r in range(3)]
        if name == "old == new":
            assert sum(t.n_messages for t in W.transports) == 0
        assert [t.n_allreduce for t in W.transports] == [0] * 3
        for r, (lo, hi) in enumerate(RP.element_slices(new)):
            a = W.amrs[r]
            assert a.n_elements == hi - lo and a.local_nodes == nodes[r] == off[hi] - off[lo]
        if name == "a rank left empty":
            assert W.amrs[1].n_elements == 0 and nodes[1] == 0
        assert np.array_equal(_bits(np.concatenate([a.get_predictor() for a in W.amrs])), _bits(pred1))
        for j in range(2):
            got = np.concatenate([t.cpu().numpy() for t in f_new[j]])
            assert np.array_equal(_bits(got), _bits(fields[j])), (name, j)
            for r in range(3):        # the old shards are the caller's and untouched
                assert np.array_equal(f_old[j][r].cpu().numpy(), RP.shard_nodes(fields[j], deg1, old)[r])
        assert np.array_equal(np.concatenate([_degrees(a, gpu) for a in W.amrs]), deg1)
        assert np.array_equal(_bits(np.concatenate([a.get_predictor() for a in W.amrs])), _bits(pred1))
    finally:
        W.close()


_ABORT_CHILD = """
import sys
import numpy as np
from disco4est_amd import Amr
case = sys.argv[1]
amr = Amr(np.full(5, 2, np.int32), 4, 1.0)
amr.set_comm(1, 3, lambda p, n: None, lambda *a: None)
old, new = [0, 4, 9, 12], [0, 2, 10, 12]
if case == "not_monotone":
    new = [0, 10, 2, 12]
elif case == "totals":
    new = [0, 2, 10, 13]
elif case == "n_elements":
    old = [0, 4, 8, 12]
elif case == "no_hook":
    amr.set_comm(1, 3, lambda p, n: None, None)
amr.repartition(old, new)
print("NOT REACHED")
"""


@pytest.mark.parametrize("case,message", [("not_monotone", "must be monotone"), ("totals", "cover different totals"),
                                          ("n_elements", "the object holds 5"), ("no_hook", "no sendrecv hook is set")])
def test_inconsistent_partitions_abort(gpu, hiplib, case, message):
    """host-side argument checks ([D4EST_HIP_ABORT], before any launch), seen from a child process"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-c", _ABORT_CHILD, case], capture_output=True, text=True, timeout=120, cwd=root, env=env)
    assert p.returncode != 0 and "NOT REACHED" not in p.stdout, p.stdout
    assert "[D4EST_HIP_ABORT] amr_repartition" in p.stderr and message in p.stderr, p.stderr


# ---- 5: the next step on the new shards --------------------------------------------------------------------------------------------------------
def test_continue_after_repartition(gpu, hiplib, monkeypatch):
    """mark -> set_balance -> interpolate_field on the shards of the new partition: logs and predictor bit-equal to the reference on the
    global list, the gathered field within FIELD_RTOL of the dense two-stage reference on the global grid"""
    import torch
    monkeypatch.delenv("D4EST_HIP_TRANSFER_GENERIC", raising=False)
    monkeypatch.delenv("D4EST_HIP_AMR_TWO_STAGE", raising=False)
    old, new = _repartition_cases()["elements to dofs"]
    W, deg1, pred1 = _ranks_at_level1(gpu, old)
    try:
        off = RP.node_offsets(deg1)
        x = _uniform(43, off[-1]) - 0.5
        x_old = [_dev(s, gpu) for s in RP.shard_nodes(x, deg1, old)]
        eta2 = 0.5 + _uniform(44, N_EL)
        thr = float(np.sort(eta2)[N_EL - 12])
        log, pred2, branch = R.mark(eta2, pred1, deg1, MAXDEG, thr, 1.0, GAMMA_H, GAMMA_P, GAMMA_N)
        log = R.clip_log(log, MAXDEG)
        assert {"h", "n"} <= set(branch) and any(l < 0 for l in log)
        aux = R.aux_grid(deg1, log)
        split = set(range(0, len(aux), 5))
        bal = [(-a[0] if i in split else a[0]) for i, a in enumerate(aux)]
        s1, s2 = R.transfer_items(deg1, log, bal)
        d1, d2 = DT.DenseTransfer(*s1), DT.DenseTransfer(*s2)
        ref = d2.prolong(d1.prolong(x))
        new_deg = [d for d, _, _ in R.new_grid(aux, bal)]
        aux_owner = np.asarray([a[1] for a in aux])
        slices = RP.element_slices(new)
        d_eta = [_dev(e, gpu) for e in RP.shard_elements(eta2, new)]
        d_thr = _dev([thr], gpu)
        out = [None] * 3

        def body(r):
            a = W.amrs[r]
            n = a.repartition(old, new)
            x_new = torch.full((n,), float("nan"), dtype=torch.float64, device=gpu)
            a.repartition_field(x_old[r], x_new)
            a.mark_smooth_pred(d_eta[r], d_thr, 1.0, GAMMA_H, GAMMA_P, GAMMA_N)
            lo, hi = slices[r]
            assert a.get_refinement_log().tolist() == list(log[lo:hi])
            mine = [b for b, o in zip(bal, aux_owner) if lo <= o < hi]
            a.set_balance(mine)
            y = torch.full((a.new_local_nodes,), float("nan"), dtype=torch.float64, device=gpu)
            a.interpolate_field(x_new, y)
            out[r] = (y, a.new_degrees(), a.get_predictor())

        W.run(body)
        assert np.array_equal(np.concatenate([o[1] for o in out]), np.asarray(new_deg))
        assert np.array_equal(_bits(np.concatenate([o[2] for o in out])), _bits(pred2))
        got = np.concatenate([o[0].cpu().numpy() for o in out])
        assert got.size == d2.fine_nodes
        err = DT.elementwise_rel_err(got, ref, d2.fine_bounds)
        print("field after repartition -> mark -> set_balance -> interpolate_field: %.3e (bound %.1e)" % (err, FIELD_RTOL))
        assert err <= FIELD_RTOL, err
    finally:
        W.close()
