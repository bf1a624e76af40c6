"""GPU sweep over EVERY compile-time instance of the hp-multigrid transfer kernels (csrc/d4est_hip_transfer.hip): coarse sizes
NH = 2 .. 16, list size differences dmax = 0 .. 3 (kernel instances DMAX = 0, 1, 3; a list with 2 runs the 3), prolongation with and
without the fused addition, restriction fed with P and with the transposed projection, the fused Galerkin term, the child-group counts
8 / 4 / 2 / 1 and the list-size rule, and the grid-stride loops of the generic kernels.

The reference is tests/dense_transfer.py (long double, pinned to the oracle by tests/test_transfer_dense.py).  Comparisons are PER
ELEMENT, each element against its own largest entry, at the transfer tolerance of tests/test_transfer_gpu.py (1e-12).  Transfer.describe()
tells which instance ran, so an item that silently took the generic path fails.  Every device vector sits between two bands of 64
sentinel doubles which must survive every call.

The expected child-group count is derived HERE from the two limits the kernels state (150 KB of LDS, 1024 threads per workgroup) and the
LDS images they document, not read from the library."""
import numpy as np
import pytest

from tests import dense_transfer as DT

pytestmark = pytest.mark.gpu
RTOL = 1e-12
GUARD = 64
SENTINEL = -1.2345678e77
DMAX_CLASS = {0: 0, 1: 1, 2: 3, 3: 3}
NH_ALL = list(range(2, 17))


# ---- the expected child groups ---------------------------------------------------------------------------------------------------
def _threads(nm):
    """one thread per line of the largest (x, y) plane, in whole wavefronts"""
    return -(-(nm * nm) // 64) * 64


def _groups(lds_doubles, threads, nc, n):
    if nc != 8 or n >= 8192:          # one child: nothing to share out; thousands of coarse elements fill the chip on their own
        return 1
    cg = 8
    while cg > 1 and (cg * lds_doubles * 8 > 150 * 1024 or cg * threads > 1024):
        cg //= 2
    return cg


def restrict_cg(NH, DMAX, nc=8, n=1):
    nm = NH + DMAX                    # images per child group: B [Nh][Nh][NH | 1] and C [Nh][NH][NH] at the largest fine size
    return _groups(nm * nm * (NH | 1) + nm * NH * NH, _threads(nm), nc, n)


def galerkin_cg(NH, DMAX, nc=8, n=1):
    nq = NH + DMAX                    # B [NH][NH][NQ | 1] and C [NH][NQ][NQ] at the largest quadrature size
    return _groups(NH * NH * (nq | 1) + NH * nq * nq, _threads(nq), nc, n)


def test_expected_child_groups_take_every_value():
    """over the sweep (every NH, every DMAX instance) the lists of eight children run with 8, 4, 2 and 1 child groups; the per-NH tests
    below assert that describe() reports exactly these values"""
    assert {restrict_cg(NH, D) for NH in NH_ALL for D in (0, 1, 3)} == {8, 4, 2, 1}
    assert {galerkin_cg(NH, D) for NH in NH_ALL for D in (0, 1, 3)} == {8, 4, 2, 1}
    assert restrict_cg(2, 3, 8, 8192) == 1 and restrict_cg(2, 3, 8, 8191) == 8 and restrict_cg(9, 1, 1, 5) == 1


# ---- guarded device vectors ------------------------------------------------------------------------------------------------------
class Guarded:
    """n live doubles with GUARD sentinel doubles before and after; .v is the interior (its data pointer is what the library gets)"""

    def __init__(self, gpu, n, fill):
        import torch
        self.full = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float64, device=gpu)
        self.v = self.full[GUARD:GUARD + n]
        if isinstance(fill, np.ndarray):
            self.v.copy_(torch.from_numpy(fill))
        else:
            self.v.fill_(fill)

    def intact(self):
        return bool((self.full[:GUARD] == SENTINEL).all()) and bool((self.full[-GUARD:] == SENTINEL).all())

    def numpy(self):
        return self.v.cpu().numpy()


def _run_all(gpu, t, d, seed, ops=("prolong", "prolong_add", "restrict", "project"), twice=True):
    """run the operations of Transfer t between guard bands, NaN-prefilled, and return the per-element errors against DenseTransfer d"""
    import torch
    from disco4est_amd import mesh as M
    xc = M.splitmix64_uniform(seed, d.coarse_nodes) - 0.5
    xf = M.splitmix64_uniform(seed + 100, d.fine_nodes) - 0.5
    gxc, gxf = Guarded(gpu, d.coarse_nodes, xc), Guarded(gpu, d.fine_nodes, xf)
    nan = float("nan")
    err = {}

    def call(fn, src, n_out, fill=nan):
        outs = []
        for _ in range(2 if twice else 1):
            o = Guarded(gpu, n_out, fill)
            fn(src.v, o.v)
            torch.cuda.synchronize()
            assert o.intact() and gxc.intact() and gxf.intact(), "a sentinel next to a live range was overwritten"
            outs.append(o)
        if twice:
            assert torch.equal(outs[0].v, outs[1].v), "two runs differ"
        return outs[0]

    if "prolong" in ops:
        pf = call(t.prolong, gxc, d.fine_nodes)
        err["prolong"] = DT.elementwise_rel_err(pf.numpy(), d.prolong(xc), d.fine_bounds)
        if "prolong_add" in ops:            # onto a non-zero fine vector: bit-equal to prolong followed by +=
            pa = call(t.prolong_add, gxc, d.fine_nodes, fill=xf)
            assert torch.equal(pa.v, gxf.v + pf.v), "prolong_add is not prolong followed by +="
        if "project" in ops:                # the round trip: bound of tests/test_transfer_gpu.py for coarse degrees <= 17
            back = call(t.project, pf, d.coarse_nodes)
            err["round_trip"] = float((back.v - gxc.v).abs().max())
    if "restrict" in ops:
        rc = call(t.restrict, gxf, d.coarse_nodes)
        err["restrict"] = DT.elementwise_rel_err(rc.numpy(), d.restrict(xf), d.coarse_bounds)
    if "project" in ops:
        pc = call(t.project, gxf, d.coarse_nodes)
        err["project"] = DT.elementwise_rel_err(pc.numpy(), d.project(xf), d.coarse_bounds)
    assert torch.equal(gxc.v, torch.from_numpy(xc).to(gpu)) and torch.equal(gxf.v, torch.from_numpy(xf).to(gpu)), "an input was modified"
    return err


def _assert_errors(err, where):
    print(where, " ".join("%s=%.2e" % kv for kv in sorted(err.items())))
    for k in ("prolong", "restrict", "project"):
        if k in err:
            assert err[k] <= RTOL, (where, k, err[k])
    if "round_trip" in err:
        assert err["round_trip"] <= 1e-11, (where, err["round_trip"])


# ---- (a) the instance sweep ------------------------------------------------------------------------------------------------------
def sweep_items(NH, dmax):
    """3 p-items and 3 hp-items of coarse size NH, interleaved.  The hp-items' children take every fine size NH .. NH + dmax; the largest
    sits on ONE child, at a different position in each item, the others cycle through the smaller sizes with a different phase per item"""
    dH = NH - 1
    hrefine, degh = [], []
    for j in range(3):
        hrefine += [0, 1]
        degh += [dH + (dmax, 0, (dmax + 1) // 2)[j]] + [0] * 7
        top = (NH + 3 * j) % 8
        degh += [dH + (dmax if c == top else ((c + j) % dmax if dmax else 0)) for c in range(8)]
    return np.array(hrefine, np.int32), np.full(6, dH, np.int32), np.array(degh, np.int32)


def test_sweep_items_are_what_the_sweep_needs():
    tops = set()
    for NH in NH_ALL:
        for dmax in range(4):
            h, dH, dh = sweep_items(NH, dmax)
            assert h.tolist() == [0, 1, 0, 1, 0, 1] and (dH == NH - 1).all()
            assert max(dh[0], dh[16], dh[32]) - (NH - 1) == dmax
            pos = []
            for j in range(3):
                off = dh[16 * j + 8:16 * j + 16] - (NH - 1)
                assert set(off.tolist()) == set(range(dmax + 1))
                pos.append(int(np.argmax(off)))
                assert dmax == 0 or (off == dmax).sum() == 1
            assert dmax == 0 or len(set(pos)) == 3
            tops.update(pos)
    assert tops == set(range(8))


@pytest.mark.parametrize("NH", NH_ALL)
def test_instance_sweep(gpu, hiplib, NH, monkeypatch):
    from disco4est_amd import Transfer
    monkeypatch.delenv("D4EST_HIP_TRANSFER_GENERIC", raising=False)
    for dmax in range(4):
        hrefine, degH, degh = sweep_items(NH, dmax)
        t = Transfer(hrefine, degH, degh)
        d = DT.DenseTransfer(hrefine, degH, degh)
        assert (t.coarse_nodes, t.fine_nodes) == (d.coarse_nodes, d.fine_nodes)
        desc = t.describe()
        cg = restrict_cg(NH, DMAX_CLASS[dmax], 8, 3)
        assert desc["prolong"] == [(NH, dmax, 1, 27, 1)], desc
        assert desc["restrict"] == [(NH, dmax, 1, 3, 1), (NH, dmax, 8, 3, cg)], desc
        assert desc["galerkin"] == []
        _assert_errors(_run_all(gpu, t, d, 1000 * NH + dmax), "NH=%d dmax=%d nc=8 cg=%d:" % (NH, dmax, cg))
        t.destroy()


# ---- (b) list-size rules ---------------------------------------------------------------------------------------------------------
def _many_hp(n, dH):
    k, c = np.arange(n)[:, None], np.arange(8)[None, :]
    return np.ones(n, np.int32), np.full(n, dH, np.int32), (dH + (k + c) % 3).astype(np.int32).reshape(-1)


@pytest.mark.parametrize("NH", [2, 3])
def test_list_size_rule(gpu, hiplib, NH, monkeypatch):
    """8192 coarse elements and more run with one child group, 8191 with the instance's eight"""
    from disco4est_amd import Transfer
    monkeypatch.delenv("D4EST_HIP_TRANSFER_GENERIC", raising=False)
    assert restrict_cg(NH, 3, 8, 8191) == 8
    for n, cg in ((8192, 1), (8191, 8)):
        items = _many_hp(n, NH - 1)
        t = Transfer(*items)
        d = DT.DenseTransfer(*items)
        desc = t.describe()
        assert desc["restrict"] == [(NH, 2, 8, n, cg)] and desc["prolong"] == [(NH, 2, 1, 8 * n, 1)], desc
        _assert_errors(_run_all(gpu, t, d, 7 * n + NH, ops=("prolong", "restrict", "project"), twice=False), "NH=%d n=%d cg=%d:" % (NH, n, cg))
        t.destroy()


def test_generic_grid_stride_prolong(gpu, hiplib, monkeypatch):
    """the generic prolongation launches min(n, 65536) workgroups: 8193 hp-items are 65544 fine elements"""
    from disco4est_amd import Transfer
    monkeypatch.setenv("D4EST_HIP_TRANSFER_GENERIC", "1")
    items = _many_hp(8193, 1)
    t = Transfer(*items)
    d = DT.DenseTransfer(*items)
    desc = t.describe()
    assert desc["prolong"] == [(0, 0, 1, 65544, 1)] and desc["restrict"] == [(0, 0, 1, 8193, 1)], desc
    _assert_errors(_run_all(gpu, t, d, 31, ops=("prolong", "prolong_add"), twice=False), "generic prolong, 65544 children:")
    t.destroy()


def test_generic_grid_stride_restrict_project(gpu, hiplib, monkeypatch):
    """the generic restriction / projection launch min(n, 65536) workgroups: 65537 p-items, degree 1 -> 1 and 2 alternating"""
    from disco4est_amd import Transfer
    monkeypatch.setenv("D4EST_HIP_TRANSFER_GENERIC", "1")
    n = 65537
    degh = np.zeros((n, 8), np.int32)
    degh[:, 0] = 1 + np.arange(n) % 2
    items = (np.zeros(n, np.int32), np.ones(n, np.int32), degh.reshape(-1))
    t = Transfer(*items)
    d = DT.DenseTransfer(*items)
    desc = t.describe()
    assert desc["restrict"] == [(0, 0, 1, n, 1)] and desc["prolong"] == [(0, 0, 1, n, 1)], desc
    _assert_errors(_run_all(gpu, t, d, 37, ops=("restrict", "project"), twice=False), "generic restrict / project, 65537 items:")
    t.destroy()


# ---- (c) the fused Galerkin term -------------------------------------------------------------------------------------------------
# Limits read from galerkin_fused_setup: the fused kernel serves one transfer whose fine plan is exactly its fine level (degrees and
# strides), with 2 <= NH <= 16 and 0 <= (deg_quad + 1) - NH <= 3 for every child, no shared quadrature blocks; anything else returns
# false and the chain runs unfused (prolong, weighted mass, restrict) -- no abort.  Plans take deg and deg_quad up to 23; the w J c
# builder has no size limit of its own (one launch per (deg, deg_quad) bucket).  The sweep stays inside: deg_quad <= 18.
def galerkin_cases(NH):
    """(hp, fine degrees, deg_quad_inc, quad_type): quadrature offsets 0 .. 3 by deg_quad_inc at fine degree = degH, for one child and
    for eight; one mixed case with the fine degrees AND inc nonzero; both quadrature types at NH in {4, 9, 16}"""
    dH = NH - 1
    cases = []
    for qt in ((0, 1) if NH in (4, 9, 16) else (0,)):
        for hp in (False, True):
            for inc in range(4):
                cases.append((hp, [dH] * (8 if hp else 1), inc, qt))
        cases.append((True, [dH + (c + NH) % 2 for c in range(8)], 1 + NH % 2, qt))   # offsets inc .. inc + 1 <= 3, eight children
    cases.append((False, [dH + 2], 1, 0))                                            # one child, offset 3 from degree and inc together
    return cases


def _coarse_level(oracle, NH, cache={}):
    """the coarse plan (a level-0 brick: one element of degree NH - 1, Gauss quadrature at its own degree -- the term's quadrature is the
    FINE plan's), its field and the oracle's Laplacian, shared by the cases of one NH"""
    from disco4est_amd import mesh as M
    from tests.test_mgmatrix_gpu import _plan
    if NH not in cache:
        for entry in cache.values():          # one NH at a time: the plan of the previous one goes
            entry[1].destroy()
        cache.clear()
        mp = M.SineMap(0.04)
        mc = M.BrickMesh(0, NH - 1)
        plan, J, rst, sides = _plan(mc, mp)
        u = mc.field(mp)
        cache[NH] = (mc, plan, u, oracle.apply_aij(mc, J, rst, sides, u))
    return cache[NH]


def _galerkin_case(gpu, oracle, monkeypatch, NH, hp, degf, inc, qt, expect_fused=True):
    """apply_lhs of the coarse plan with the chain [one transfer] -> fine plan against oracle.apply_aij + the dense term, once with the
    chain as it is and once unfused; describe() must show the Galerkin list exactly when the fused kernel serves the chain"""
    import torch
    from disco4est_amd import Plan, Transfer, mesh as M
    mp = M.SineMap(0.04)
    dH = NH - 1
    mc, plan, u, lap = _coarse_level(oracle, NH)
    mf = M.BrickMesh(1 if hp else 0, np.array(degf, np.int32), deg_quad_inc=inc, quad_type=qt)
    Jf, rstf = mf.geometry(mp)
    pf = Plan(mf.deg, mf.deg_quad, mf.nodal_stride, mf.quad_stride, qt)
    pf.set_geometry(Jf, rstf)
    items = (np.array([1 if hp else 0], np.int32), np.array([dH], np.int32), np.array((list(degf) + [0] * 8)[:8], np.int32))
    # the coefficient: positive and varying, scaled so that the term (linear in it) is a fifth of the Laplacian's size
    c0 = 0.5 + 2.0 * M.splitmix64_uniform(17 + NH, mf.local_nodes_quad)
    dq = [int(q) for q in mf.deg_quad]
    jc = [(Jf * c0)[mf.quad_stride[e]:mf.quad_stride[e] + (dq[e] + 1) ** 3] for e in range(mf.n_elements)]
    term0 = DT.galerkin_term(qt, hp, dH, list(degf), dq, jc, u)
    scale = 0.2 * np.abs(lap).max() / np.abs(term0).max()
    coeff, term = scale * c0, scale * term0
    assert np.abs(term).max() >= 0.1 * np.abs(lap).max()
    ref = lap + term
    dcoeff = torch.from_numpy(coeff).to(gpu)
    pf.set_lhs_coefficient(dcoeff)
    offs = sorted(q + 1 - NH for q in dq)
    nc = len(degf)
    where = "NH=%d nc=%d offsets %d..%d quad %d" % (NH, nc, offs[0], offs[-1], qt)
    for unfused in (False, True):
        if unfused:
            monkeypatch.setenv("D4EST_HIP_CHAIN_UNFUSED", "1")
        else:
            monkeypatch.delenv("D4EST_HIP_CHAIN_UNFUSED", raising=False)
        t = Transfer(*items)
        plan.set_lhs_galerkin_chain([t], pf)
        gu, gAu = Guarded(gpu, mc.local_nodes, u), Guarded(gpu, mc.local_nodes, float("nan"))
        plan.apply_lhs(gu.v, gAu.v)
        torch.cuda.synchronize()
        desc = t.describe()["galerkin"]
        if unfused or not expect_fused:
            assert desc == [], (where, desc)
        else:
            assert desc == [(NH, offs[-1], nc, 1, galerkin_cg(NH, DMAX_CLASS[offs[-1]], nc, 1))], (where, desc)
        assert gu.intact() and gAu.intact(), where
        err = np.abs(gAu.numpy() - ref).max() / np.abs(ref).max()
        print(where, "unfused" if unfused else "fused", "%.2e" % err)
        assert err <= RTOL, (where, unfused, err)
        plan.set_lhs_galerkin_chain([], None)
        t.destroy()
    pf.destroy()


@pytest.mark.parametrize("NH", NH_ALL)
def test_galerkin_sweep(gpu, hiplib, oracle, NH, monkeypatch):
    monkeypatch.delenv("D4EST_HIP_TRANSFER_GENERIC", raising=False)
    for hp, degf, inc, qt in galerkin_cases(NH):
        _galerkin_case(gpu, oracle, monkeypatch, NH, hp, degf, inc, qt)


def test_galerkin_falls_back_beyond_the_compile_time_sizes(gpu, hiplib, oracle, monkeypatch):
    """a quadrature offset of 4 is outside the fused kernel's instances: no Galerkin list, the chain runs unfused, the result stands"""
    monkeypatch.delenv("D4EST_HIP_TRANSFER_GENERIC", raising=False)
    _galerkin_case(gpu, oracle, monkeypatch, 4, True, [3, 4, 3, 4, 4, 3, 4, 3], 3, 0, expect_fused=False)   # offsets 3 and 4
