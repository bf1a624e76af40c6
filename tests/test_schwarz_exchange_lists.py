"""The whole-element exchange lists of the sharded Schwarz smoother (d4est_hip_schwarz_set_element_exchange) without a device: the lists
of all ranks are mutually consistent, and the per-element list the accumulate kernel walks reproduces SchwarzShard.end_correction_exchange."""
import os
import subprocess

import numpy as np
import pytest

from tests import schwarz_shard_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _all_ranks(case, kind):
    if kind == "brick":
        world, level, deg_spec, _, _ = case
        deg_global, parts = C.brick_case(world, level, deg_spec)
        return [C.RankLists(level, deg_global, parts, r) for r in range(world)]
    world, pattern, deg_spec, _ = case
    refine, deg_global, parts = C.hanging_case(world, pattern, deg_spec)
    return [C.RankLists(1, deg_global, parts, r, refine=refine) for r in range(world)]


CASES = [("brick", c) for c in C.BRICK] + [("hanging", c) for c in C.HANGING]


@pytest.mark.parametrize("kind,case", CASES)
def test_lists_of_all_ranks_are_consistent(kind, case):
    ranks = _all_ranks(case, kind)
    for a, la in enumerate(ranks):
        assert list(la.peers) == sorted(set(int(p) for p in la.peers)) and a not in la.peers
        assert np.all(la.send_elem < la.n_own) and np.all(la.recv_elem >= la.n_own)
        # every ghost-layer element is owned by exactly one peer
        assert sorted(la.recv_elem.tolist()) == list(range(la.n_own, la.mesh.n_elements))
        for i, b in enumerate(la.peers):
            lb = ranks[int(b)]
            assert a in lb.peers
            j = list(lb.peers).index(a)
            sent, expected = la.segment("send", i), lb.segment("recv", j)
            gs, gr = la.mesh.elements[sent], lb.mesh.elements[expected]
            # ascending global ids, the same elements on both ends: no metadata is exchanged
            assert np.all(np.diff(gs) > 0) and np.array_equal(gs, gr)
            # direction 0: a's send count is b's receive count; direction 1 swaps the roles of the same two segments
            assert int(la.n3[sent].sum()) == int(lb.n3[expected].sum())
            back_sent, back_expected = lb.segment("recv", j), la.segment("send", i)
            assert int(lb.n3[back_sent].sum()) == int(la.n3[back_expected].sum())


def test_some_own_element_is_corrected_by_two_peers():
    """the order of the additions in the accumulate kernel is only exercised where an own element lies in two peers' ghost layers"""
    got = {}
    for case in C.BRICK:
        got[case[0]] = [int((C.corrected_by(l) >= 2).sum()) for l in _all_ranks(case, "brick")]
        if case[0] == 4:
            assert max(int(C.corrected_by(l).max()) for l in _all_ranks(case, "brick")) == 3
    assert got == {2: [0, 0], 3: [6, 12, 7], 4: [4, 4, 4, 4]}, got


@pytest.mark.parametrize("kind,case", CASES)
def test_csr_accumulate_reproduces_the_python_composition(kind, case):
    """SchwarzShard.end_correction_exchange itself (its code, on CPU tensors, with a block copy in numpy standing in for the device
    copy_blocks) against the numpy restatement of the accumulate kernel's per-element list: equal, entry for entry"""
    import torch
    from disco4est_amd import parallel as P
    from disco4est_amd.schwarz import SchwarzShard

    def copy_blocks(n, src, src_off, dst, dst_off, ln):
        for k in range(n):
            a, b, l = int(src_off[k]), int(dst_off[k]), int(ln[k])
            dst[b:b + l] = src[a:a + l]

    class _Done:
        def finish(self, pending):
            pass

    for rank, lists in enumerate(_all_ranks(case, kind)):
        rng = np.random.default_rng(100 + rank)
        m = lists.mesh
        u_own, u_ext = rng.standard_normal(lists.own_nodes), rng.standard_normal(m.local_nodes)
        recv = rng.standard_normal(int(lists.n3[lists.send_elem].sum()))
        shard = SchwarzShard.__new__(SchwarzShard)
        shard.own_nodes = lists.own_nodes
        shard.u_ext = torch.from_numpy(u_ext.copy())
        shard.back = torch.zeros(m.local_nodes, dtype=torch.float64)
        shard.backward = P.TraceExchange(lists.schedule.reversed(), _Done(), copy_blocks, "cpu")
        at = 0
        for p in shard.backward.s.peers:           # the received buffer, peer after peer: the layout of the native receive buffer
            n = shard.backward.recv_buf[p].numel()
            shard.backward.recv_buf[p].copy_(torch.from_numpy(recv[at:at + n].copy()))
            at += n
        assert at == recv.size
        u = torch.from_numpy(u_own.copy())
        shard.end_correction_exchange(u)
        assert np.array_equal(u.numpy(), C.accumulate_csr(lists, u_own, u_ext, recv))


def test_new_symbols_are_exported_and_bound(hiplib):
    from disco4est_amd import capi, parallel, schwarz
    for s in ("d4est_hip_schwarz_set_element_exchange", "d4est_hip_schwarz_own_nodes", "d4est_hip_schwarz_exchange_first",
              "d4est_hip_schwarz_host_reads", "d4est_hip_schwarz_set_rccl_exchange", "d4est_hip_schwarz_rccl_exchange_destroy",
              "d4est_hip_schwarz_rccl_exchange_count"):
        assert hasattr(hiplib, s), "libd4est_hip.so does not export %s" % s
        assert s in capi.SIGNATURES
    assert hasattr(schwarz.Schwarz, "set_element_exchange") and hasattr(schwarz, "SchwarzShardNative")
    for name in ("attach_schwarz", "attach_schwarz_rccl", "element_exchange_lists"):
        assert hasattr(parallel, name)
    assert hasattr(parallel.DistTransport, "round")


def test_header_compiles_as_c99_with_the_element_exchange(tmp_path):
    src = tmp_path / "schwarz_exchange_header.c"
    src.write_text('#include "d4est_hip.h"\n'
                   "static void hook(void* ctx, int direction, const double* send_dev, double* recv_dev) {\n"
                   "  (void)ctx; (void)direction; (void)send_dev; (void)recv_dev;\n"
                   "}\n"
                   "long long use(d4est_hip_schwarz_t* sz, d4est_hip_comm_t* comm, const int* l) {\n"
                   "  d4est_hip_element_exchange_fn fn = hook;\n"
                   "  d4est_hip_schwarz_rccl_exchange_t* x = d4est_hip_schwarz_set_rccl_exchange(sz, comm, 4, 1, l, l, l, l, l);\n"
                   "  d4est_hip_schwarz_rccl_exchange_destroy(x);\n"
                   "  d4est_hip_schwarz_set_element_exchange(sz, 4, 1, l, l, l, l, l, fn, 0);\n"
                   "  return d4est_hip_schwarz_own_nodes(sz) + d4est_hip_schwarz_exchange_first(sz, 1, 0, 1) + d4est_hip_schwarz_host_reads(sz)\n"
                   "         + d4est_hip_schwarz_rccl_exchange_count(x);\n"
                   "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "schwarz_exchange_header.o")])
