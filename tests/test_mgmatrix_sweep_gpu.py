"""GPU: the five kernels of csrc/d4est_hip_mgmatrix.hip (block_matvec_add, mass_blocks, galerkin_rows, galerkin_cols,
galerkin_cols_window) against the dense long-double forms of tests/dense_mgmatrix.py at every launch shape the host code can choose
(tests/mgmatrix_cases.py; tests/test_mgmatrix_dense.py proves on the CPU that the lists reach the shapes), and the switches between the
forms of the zeroth-order term on one plan against fresh plans, bit for bit.  No oracle: the dense forms are pinned to it on the CPU.
Every output is filled with NaN first; tolerances are the 1e-12 of tests/test_mgmatrix_gpu.py, relative to the max norm of the reference
(the matvec: of apply_lhs, as test_block_term_at_size).  Worst errors and run times: profiles/mgmatrix_tests.md."""
import numpy as np
import pytest

from tests import dense_mgmatrix as D
from tests import mgmatrix_cases as C
from tests.mgmatrix_cases import RTOL, hierarchy as _hierarchy

pytestmark = pytest.mark.gpu


def _dev(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _nan(n, gpu):
    import torch
    return torch.full((int(n),), float("nan"), dtype=torch.float64, device=gpu)


def _rel(got, ref, scale=None):
    """max |got - ref| / scale (default max |ref|); an entry that was never written (NaN) counts as infinite"""
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    d = np.abs(got - ref)
    d[~np.isfinite(got)] = np.inf
    return float(d.max() / (np.abs(ref).max() if scale is None else scale))


# ---- (a) Au_e += M_e u_e --------------------------------------------------------------------------------------------------------
def _spd_blocks(deg, off, n):
    """symmetric, strictly diagonally dominant with a positive diagonal (SPD by Gershgorin), made on the host: entries U(-1/2, 1/2)
    symmetrised, diagonal + N3 / 2 + 1"""
    from disco4est_amd import mesh as M
    out = np.full(n, np.nan)
    offs = D.consecutive_offsets(deg) if off is None else off
    for d in sorted(set(deg.tolist())):
        o = np.unique(offs[deg == d])
        n3 = (d + 1) ** 3
        R = (M.splitmix64_uniform(1000 + d, o.size * n3 * n3) - 0.5).reshape(-1, n3, n3)
        R = 0.5 * (R + R.transpose(0, 2, 1))
        R[:, np.arange(n3), np.arange(n3)] += 0.5 * n3 + 1.0
        if o.size == 1 or (np.diff(o) == n3 * n3).all():
            out[o[0]:o[0] + R.size] = R.ravel()
        else:
            out[(o[:, None] + np.arange(n3 * n3)).ravel()] = R.ravel()
    assert np.isfinite(out).all()
    return out


@pytest.mark.parametrize("name,level,deg,layout", C.MATVEC_CASES, ids=[c[0] for c in C.MATVEC_CASES])
def test_block_matvec(gpu, hiplib, name, level, deg, layout):
    import torch
    from disco4est_amd import Plan, mesh as M
    m = M.BrickMesh(level, C.degrees(level, deg))
    mp = M.SineMap(0.03) if level <= 2 else None          # (the big bricks affine: the term does not see the geometry)
    J, rst = m.geometry(mp)
    sides = m.build_sides(mp)
    plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, 0)
    plan.set_geometry(J, rst)
    plan.set_faces(sides, 10.0, 0)
    off, n = C.block_layout(m.deg, layout)
    blocks = _spd_blocks(m.deg, off, n)
    u = m.field(mp)
    dblocks, du = _dev(blocks, gpu), _dev(u, gpu)
    lap, lhs = _nan(m.local_nodes, gpu), _nan(m.local_nodes, gpu)
    plan.apply_aij(du, lap)
    plan.set_lhs_element_blocks(dblocks, off)
    plan.apply_lhs(du, lhs)
    ref = D.block_term(m, blocks, u, off)
    scale = float(lhs.abs().max())
    assert np.isfinite(scale) and np.abs(ref).max() > 1e-3 * scale          # the term is not negligible beside the Laplacian
    err = _rel(lhs - lap, ref, scale)
    print("block_matvec %s: %.3e" % (name, err))
    assert err <= RTOL, (name, err)
    again = _nan(m.local_nodes, gpu)
    plan.apply_lhs(du, again)
    assert torch.equal(lhs, again)
    plan.destroy()


# ---- (b) V^T W J c V --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_coeff", [True, False], ids=["coeff", "nocoeff"])
@pytest.mark.parametrize("quad_type", [0, 1], ids=["gauss", "lobatto"])
@pytest.mark.parametrize("level,deg,inc", C.MASS_CASES, ids=["l%d-p%s-inc%d" % (lv, "".join(map(str, p)) if isinstance(p, tuple) else p, i)
                                                             for lv, p, i in C.MASS_CASES])
def test_weighted_mass_blocks(gpu, hiplib, level, deg, inc, quad_type, with_coeff):
    from disco4est_amd import Plan, mesh as M
    m = M.BrickMesh(level, C.degrees(level, deg), deg_quad_inc=inc, quad_type=quad_type)
    mp = M.SineMap(0.04)
    J, rst = m.geometry(mp)
    plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, quad_type)
    plan.set_geometry(J, rst)
    coeff = 0.5 + 2.0 * M.splitmix64_uniform(41, m.local_nodes_quad) if with_coeff else None
    out = _nan(plan.matrix_nodes(), gpu)
    plan.compute_weighted_mass_blocks(_dev(coeff, gpu) if with_coeff else None, out)
    got = out.cpu().numpy()
    ref = D.mass_blocks(m, J, coeff)
    err = _rel(got, ref)
    print("mass_blocks l%d p%s inc%d q%d c%d: %.3e" % (level, deg, inc, quad_type, with_coeff, err))
    assert err <= RTOL, err
    off = D.consecutive_offsets(m.deg)
    worst = 0.0
    for e in range(m.n_elements):
        n3 = (int(m.deg[e]) + 1) ** 3
        b = got[off[e]:off[e] + n3 * n3].reshape(n3, n3)
        worst = max(worst, float(np.abs(b - b.T).max() / np.abs(b).max()))
    assert worst <= 1e-13, worst
    plan.destroy()


# ---- (c) sum_c P_c^T M_c P_c ------------------------------------------------------------------------------------------------------
_GALERKIN_INPUT = {}


def _galerkin_input(name):
    """the fine blocks of a case and both dense forms, computed once and shared by the two tests of the case"""
    from disco4est_amd import mesh as M
    if name not in _GALERKIN_INPUT:
        h, dH, dh = C.GALERKIN_CASES[name]
        n = sum((int(dh[8 * k + c]) + 1) ** 6 for k in range(h.size) for c in range(8 if h[k] == 1 else 1))
        fine = M.splitmix64_uniform(53, n) - 0.5
        fine.setflags(write=False)
        _GALERKIN_INPUT[name] = (fine, {})
    return _GALERKIN_INPUT[name]


@pytest.mark.parametrize("literal", [False, True], ids=["exact", "literal"])
@pytest.mark.parametrize("name", list(C.GALERKIN_CASES))
def test_galerkin_blocks(gpu, hiplib, name, literal):
    from disco4est_amd import Transfer
    h, dH, dh = C.GALERKIN_CASES[name]
    fine, refs = _galerkin_input(name)
    t = Transfer(h, dH, dh)
    out = _nan(D.matrix_nodes(dH), gpu)
    t.galerkin_blocks(_dev(fine, gpu), out, literal_window=literal)
    if literal not in refs:
        refs[literal] = D.restrict_blocks(h, dH, dh, fine, literal_window=literal)
    ref = refs[literal]
    # every coarse block against its OWN scale (a wrong small block must not hide behind a large one), and all of them together
    bounds = np.concatenate([D.consecutive_offsets(dH), [ref.size]])
    got = out.cpu().numpy()
    err = max(_rel(got[a:b], ref[a:b]) for a, b in zip(bounds[:-1], bounds[1:]))
    print("galerkin_blocks %s %s: %.3e" % (name, "literal" if literal else "exact", err))
    assert err <= RTOL, (name, literal, err)
    t.destroy()


# ---- (d) switching between the forms on one plan -----------------------------------------------------------------------------------
class _Level:
    """host data of a two-level pair (coarse mesh under test, its fine mesh, the transfer between them), made once per configuration"""

    def __init__(self, mc, mf, items):
        from disco4est_amd import mesh as M
        mp = M.SineMap(0.04)
        self.mc, self.mf, self.items = mc, mf, items
        self.geo_c = mc.geometry(mp) + (mc.build_sides(mp),)
        self.geo_f = mf.geometry(mp) + (mf.build_sides(mp),)
        self.u = mc.field(mp)
        self.rhs = M.splitmix64_uniform(61, mc.local_nodes) - 0.5
        self.cA = 0.5 + 2.0 * M.splitmix64_uniform(62, mc.local_nodes_quad)
        self.cB = 3.0 - 2.0 * M.splitmix64_uniform(63, mc.local_nodes_quad)
        self.cF = 0.5 + 2.0 * M.splitmix64_uniform(64, mf.local_nodes_quad)


def _plan_of(m, geo, stream, key9):
    from disco4est_amd import Plan
    plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, 0, stream=stream)
    plan.set_geometry(geo[0], geo[1])
    if key9 is not None:
        plan.set_tuning(9, key9)
    plan.set_faces(geo[2], 10.0, 0)
    return plan


class _Side:
    """one coarse plan with everything it needs to enter any state: its own coefficient tensor (overwritten with NaN after every set),
    its own fine plan and transfer (the fine coefficient tensor overwritten with NaN after the set), its own vectors"""

    def __init__(self, L, gpu, stream, key9):
        import torch
        from disco4est_amd import Transfer
        self.L, self.gpu, self.stream, self.key9 = L, gpu, stream, key9
        self.plan = _plan_of(L.mc, L.geo_c, stream, key9)
        self.fine = self.transfer = None
        self.c = _nan(L.mc.local_nodes_quad, gpu)
        n = L.mc.local_nodes
        self.u, self.rhs = _dev(L.u, gpu), _dev(L.rhs, gpu)
        self.lhs, self.x, self.Au, self.r = (torch.empty(n, dtype=torch.float64, device=gpu) for _ in range(4))
        self._Transfer = Transfer

    def _chain_parts(self):
        if self.fine is None:
            self.fine = _plan_of(self.L.mf, self.L.geo_f, self.stream, None)
            cf = _dev(self.L.cF, self.gpu)
            self.fine.set_lhs_coefficient(cf)
            cf.fill_(float("nan"))                       # the values were captured: the caller's tensor is free
            self._cf = cf
            self.transfer = self._Transfer(*self.L.items, stream=self.stream)
        return self.transfer, self.fine

    def enter(self, state, blocks, monkeypatch):
        kind = state.split(":")[0]
        if kind == "off-from-coeff":
            self.plan.set_lhs_coefficient(None)
        elif kind == "coeff":
            self.c.copy_(_dev(self.L.cA if state.endswith("A") else self.L.cB, self.gpu))
            self.plan.set_lhs_coefficient(self.c)        # (the same tensor every time, new values)
            self.c.fill_(float("nan"))
        elif kind == "blocks":
            self.plan.set_lhs_element_blocks(blocks[state[-1]])
        elif kind == "chain":
            if state.endswith("unfused"):
                monkeypatch.setenv("D4EST_HIP_CHAIN_UNFUSED", "1")
            else:
                monkeypatch.delenv("D4EST_HIP_CHAIN_UNFUSED", raising=False)
            t, fine = self._chain_parts()
            self.plan.set_lhs_galerkin_chain([t], fine)
            monkeypatch.delenv("D4EST_HIP_CHAIN_UNFUSED", raising=False)
        elif kind != "off":
            raise ValueError(state)

    def probe(self, lmin, lmax):
        """apply_lhs, two cheby_iterate calls with the same arguments (the second one replays the graph under tuning key 9), cg_eigs"""
        out, kernels = [], []
        self.lhs.fill_(float("nan"))
        self.plan.apply_lhs(self.u, self.lhs)
        out.append(self.lhs.clone()); kernels.append(self.plan.last_kernel())
        for _ in range(2):
            self.x.zero_()
            self.Au.fill_(float("nan")); self.r.fill_(float("nan"))
            self.plan.cheby_iterate(self.x, self.rhs, self.Au, self.r, 3, lmin, lmax, 1)
            out += [self.x.clone(), self.r.clone()]; kernels.append(self.plan.last_kernel())
        self.x.zero_()
        bound, _ = self.plan.cg_eigs(self.x, self.rhs, self.Au, 4, 1)
        out.append(self.x.clone()); kernels.append(self.plan.last_kernel())
        return out, bound, kernels

    def destroy(self):
        self.plan.destroy()
        if self.fine is not None:
            self.transfer.destroy()
            self.fine.destroy()


_WALK = ["off", "coeff:A", "coeff:B", "blocks:A", "chain:fused", "chain:unfused", "blocks:B", "coeff:A", "off-from-coeff"]


@pytest.mark.parametrize("config", ["hp3-middle", "p3-key9-off", "p3-key9-on"])
def test_switching_forms_matches_fresh_plans(gpu, hiplib, config, monkeypatch):
    """one plan walks off -> coefficient A -> coefficient B -> blocks -> chain (fused, unfused) -> blocks B -> coefficient A -> off with the
    same vectors all the way; after every step its results and kernel names equal, bit for bit, those of a fresh plan put directly into
    that state.  Every coefficient tensor is overwritten with NaN right after its setter returns."""
    import contextlib
    import torch
    from disco4est_amd import mesh as M
    if config == "hp3-middle":
        meshes, items = _hierarchy("hp3")
        L, stream, key9 = _Level(meshes[1], meshes[0], items[0]), None, None
    else:
        mc, mf = M.BrickMesh(1, 3, deg_quad_inc=1), M.BrickMesh(2, 3, deg_quad_inc=1)
        L = _Level(mc, mf, (np.ones(8, np.int32), np.full(8, 3, np.int32), np.full(64, 3, np.int32)))
        stream, key9 = torch.cuda.Stream(), (1 if config.endswith("on") else 0)
    with (torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
        walker = _Side(L, gpu, stream, key9)
        # blocks A: 1.5 x the Galerkin restriction of the fine level's blocks (NOT the chain's operator: a replayed graph of the wrong
        # form must show); blocks B: another multiple
        t, fine = walker._chain_parts()
        fb = _nan(fine.matrix_nodes(), gpu)
        fine.compute_weighted_mass_blocks(_dev(L.cF, gpu), fb)
        cb = _nan(walker.plan.matrix_nodes(), gpu)
        t.galerkin_blocks(fb, cb)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(cb).all())
        blocks = {"A": 1.5 * cb, "B": 0.75 * cb}
        bound0, _ = walker.plan.cg_eigs(torch.zeros_like(walker.x), walker.rhs, walker.Au, 8, 1)
        lmax = 2.2 * bound0
        lmin = lmax / 30.0
        first = None                                     # the results of step 0 (off): the Laplacian alone
        for step, state in enumerate(_WALK):
            walker.enter(state, blocks, monkeypatch)
            got = walker.probe(lmin, lmax)
            fresh = _Side(L, gpu, stream, key9)
            fresh.enter("off" if state.startswith("off") else state, blocks, monkeypatch)
            want = fresh.probe(lmin, lmax)
            fresh.destroy()
            for k, (a, b) in enumerate(zip(got[0], want[0])):
                # BOTH sides overwrite their coefficient tensors (the fine plan's under a chain included) with NaN after the setter, so a
                # form that read the caller's tensor would give NaN on both sides and torch.equal alone would not see it: this is the
                # assertion that catches it
                assert bool(torch.isfinite(b).all()) and bool(torch.isfinite(a).all()), (config, step, state, k)
                assert torch.equal(a, b), (config, step, state, k, float((a - b).abs().max()))
            assert got[1] == want[1], (config, step, state, got[1], want[1])
            assert got[2] == want[2], (config, step, state, got[2], want[2])
            if step == 0:
                first = got
            elif state.startswith(("coeff", "blocks", "chain")):
                # ... and the term is there: the result differs from the Laplacian alone
                assert not torch.equal(got[0][0], first[0][0]), (config, step, state)
        assert torch.equal(got[0][0], first[0][0])       # off again: the Laplacian alone
        walker.destroy()
