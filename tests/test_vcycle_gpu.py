"""The device multigrid (d4est_hip_multigrid_*: V-cycle, solve, preconditioner) and d4est_hip_transfer_prolong_add against the numpy
restatement of the reference's multigrid (tests/ref_multigrid.py) driven by the oracle: the oracle's registered operator (re-registered
per level: it holds one operator), its cheby_iterate and cg_eigs, and the item loop over its prolongation functions.

Tolerances.  The device operator is admitted to differ from the oracle's by RTOL = 1e-12 relative-inf per apply
(tests/test_mgmatrix_gpu.py).  How far a whole cycle amplifies such a difference is measured on the reference alone: the restatement
runs twice on the CPU with numpy forms of the two smoother kernels, once on the oracle's apply and once with every apply perturbed by
seeded noise of relative-inf size RTOL; the relative-inf distance between the two runs, separately for u, r2 and eigs, is the
amplification of an admitted difference.  The device must be within 10 x that distance of the oracle-driven restatement (one noise draw
is not the worst case).  DESIGN.md records the distances and the device's differences."""
import ctypes

import numpy as np
import pytest

from tests import ref_multigrid as RM
from tests import ref_solvers as RS

pytestmark = pytest.mark.gpu
RTOL = 1e-12
FACTOR = 10.0


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _rel_each(a, b):
    """largest relative difference entry by entry (eigs per level, r2 per cycle)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))) if a.size else 0.0


def _meshes(kind):
    """meshes finest first and the transfer item lists between consecutive levels (the hierarchies of tests/test_mgmatrix_gpu.py)"""
    from disco4est_amd import mesh as M
    if kind == "hp3":
        # level-2 brick (64 elements, p = 2..4 scattered: the eight children of a parent differ) -> h-coarsened level-1 brick (degH = the
        # smallest child degree, d4est_solver_multigrid_callbacks.h:52-75) -> p-coarsened (deg - 1, :9-20)
        deg2 = (2 + (np.arange(64) * 7 + (np.arange(64) // 8)) % 3).astype(np.int32)
        deg1 = deg2.reshape(8, 8).min(axis=1).astype(np.int32)
        deg0 = np.maximum(deg1 - 1, 1).astype(np.int32)
        meshes = [M.BrickMesh(2, deg2, deg_quad_inc=1), M.BrickMesh(1, deg1, deg_quad_inc=1), M.BrickMesh(1, deg0, deg_quad_inc=1)]
        items = [(np.ones(8, np.int32), deg1, deg2.copy()),
                 (np.zeros(8, np.int32), deg0, np.ascontiguousarray(np.stack([deg1] + [np.zeros(8, np.int32)] * 7, axis=1).reshape(-1)))]
        return meshes, items, [False, False, False]
    if kind == "hanging2":
        # fine: level-1 brick with octants 1 and 6 refined (22 elements, hanging faces), p = 2 / 3; coarse: the level-1 brick -- the refined
        # octants coarsen (eight children -> parent), the others are copied (the reference's third case) or lose one degree
        refine = np.zeros(8, dtype=bool)
        refine[[1, 6]] = True
        n_el = 8 - 2 + 16
        degf = (2 + (np.arange(n_el) * 5) % 2).astype(np.int32)
        mf = M.HangingBrickMesh(1, refine, degf, deg_quad_inc=0)
        hrefine, degH, degh = [], [], []
        k = 0
        for b in range(8):
            dh = np.zeros(8, np.int32)
            if refine[b]:
                dh[:] = degf[k:k + 8]
                hrefine.append(1); degH.append(int(dh.min())); k += 8
            else:
                dh[0] = degf[k]
                hrefine.append(0); degH.append(int(degf[k]) - (1 if b % 2 == 0 else 0)); k += 1   # p-coarsened or copied
            degh.append(dh)
        degH = np.array(degH, np.int32)
        mc = M.BrickMesh(1, degH, deg_quad_inc=0)
        return [mf, mc], [(np.array(hrefine, np.int32), degH, np.concatenate(degh))], [True, False]
    raise ValueError(kind)


def _oracle_transfer(oracle, hrefine, degH, degh, x, prolong):
    """item loop of the reference's transfer callbacks with the oracle's element functions (as tests/test_transfer_gpu.py)"""
    dp = ctypes.POINTER(ctypes.c_double)
    ip = ctypes.POINTER(ctypes.c_int)
    lib = oracle.lib
    lib.oracle_apply_p_prolong.argtypes = [dp, ctypes.c_int, ctypes.c_int, ctypes.c_int, dp]
    lib.oracle_apply_hp_prolong.argtypes = [dp, ctypes.c_int, ctypes.c_int, ip, dp]
    lib.oracle_apply_p_prolong_transpose.argtypes = [dp, ctypes.c_int, ctypes.c_int, ctypes.c_int, dp]
    lib.oracle_apply_hp_prolong_transpose.argtypes = [dp, ip, ctypes.c_int, ctypes.c_int, dp]
    nc_nodes = int(sum((int(d) + 1) ** 3 for d in degH))
    nf_nodes = int(sum((int(degh[8 * k + c]) + 1) ** 3 for k in range(len(hrefine)) for c in range(8 if hrefine[k] else 1)))
    out = np.zeros(nf_nodes if prolong else nc_nodes)
    co = fo = 0
    for k in range(len(hrefine)):
        dH = int(degH[k])
        nH = (dH + 1) ** 3
        dh = np.ascontiguousarray(degh[8 * k:8 * k + 8], dtype=np.int32)
        nc = 8 if hrefine[k] else 1
        nf = int(sum((int(d) + 1) ** 3 for d in dh[:nc]))
        if prolong:
            src = np.ascontiguousarray(x[co:co + nH]); dst = np.zeros(nf)
            if nc == 1:
                lib.oracle_apply_p_prolong(src.ctypes.data_as(dp), dH, 3, int(dh[0]), dst.ctypes.data_as(dp))
            else:
                lib.oracle_apply_hp_prolong(src.ctypes.data_as(dp), dH, 3, dh.ctypes.data_as(ip), dst.ctypes.data_as(dp))
            out[fo:fo + nf] = dst
        else:
            src = np.ascontiguousarray(x[fo:fo + nf]); dst = np.zeros(nH)
            if nc == 1:
                lib.oracle_apply_p_prolong_transpose(src.ctypes.data_as(dp), int(dh[0]), 3, dH, dst.ctypes.data_as(dp))
            else:
                lib.oracle_apply_hp_prolong_transpose(src.ctypes.data_as(dp), dh.ctypes.data_as(ip), 3, dH, dst.ctypes.data_as(dp))
            out[co:co + nH] = dst
        co += nH
        fo += nf
    return out


class _OracleLevels:
    """the CPU side of a hierarchy: per-level geometry and the oracle registered with one level at a time.  Levels in the reference's
    numbering: 0 = coarsest."""

    def __init__(self, kind, oracle, term=False):
        from disco4est_amd import mesh as M
        self.oracle, self.kind, self.term = oracle, kind, term
        self.mp = M.SineMap(0.04)
        meshes, items, hanging = _meshes(kind)
        self.meshes = meshes[::-1]
        self.items = items[::-1]            # items[l]: level l (coarse) <-> l + 1 (fine)
        self.hanging = hanging[::-1]
        self.geo = []
        for m in self.meshes:
            J, rst = m.geometry(self.mp)
            self.geo.append((J, rst, m.build_sides(self.mp)))
        self.n_levels = len(self.meshes)
        self.nodes = [m.local_nodes for m in self.meshes]
        self.coeff = None
        self.blocks = [None] * self.n_levels
        if term:
            # config 4's operator in miniature: f'(u0) on the finest level, its Galerkin-restricted element blocks below
            top = self.n_levels - 1
            self.coeff = 0.5 + 2.0 * M.splitmix64_uniform(17, self.meshes[top].local_nodes_quad)
            b = oracle.mg_matrix_setup(self.meshes[top], self.geo[top][0], self.coeff)
            for l in range(top - 1, -1, -1):
                b = oracle.mg_matrix_restriction(*self.items[l], b)
                self.blocks[l] = b
        self.registered = None
        self.noise = None            # None: the oracle's apply; else a numpy Generator: apply + RTOL noise

    def register(self, l):
        if self.registered == l:
            return
        J, rst, sides = self.geo[l]
        o = self.oracle
        o.set_operator(self.meshes[l], J, rst, sides, 10.0, 0, threads=4)
        o.set_hanging(sides if self.hanging[l] else None)
        o.set_lhs_coefficient(self.coeff if (self.term and l == self.n_levels - 1) else None)
        o.set_lhs_element_blocks(self.blocks[l] if (self.term and l < self.n_levels - 1) else None)
        self.registered = l

    def close(self):
        self.oracle.set_hanging(None)
        self.oracle.set_lhs_coefficient(None)
        self.oracle.set_lhs_element_blocks(None)
        self.registered = None

    def apply(self, l, u):
        self.register(l)
        Au = self.oracle.apply_lhs(np.ascontiguousarray(u))
        if self.noise is not None:      # an admitted difference: relative-inf size RTOL
            Au = Au + RTOL * np.abs(Au).max() * (2.0 * self.noise.random(Au.size) - 1.0)
        return Au

    def hierarchy(self, kernels):
        """kernels = 'oracle': the oracle's cheby_iterate / cg_eigs; 'numpy': tests/ref_multigrid.py's around self.apply"""
        def cheby(l, u, rhs, it, lmin, lmax):
            if kernels == "oracle":
                self.register(l)
                return self.oracle.cheby_iterate(u, rhs, it, lmin, lmax, 1)
            return RM.np_cheby_iterate(lambda x: self.apply(l, x), u, rhs, it, lmin, lmax)

        def eigs(l, u, rhs, imax, use_new):
            if kernels == "oracle":
                self.register(l)
                return self.oracle.cg_eigs(u, rhs, imax, use_new)
            return RM.np_cg_eigs(lambda x: self.apply(l, x), u, rhs, imax, use_new)

        return RM.Hierarchy(self.nodes, self.apply, cheby, eigs,
                            prolong=lambda l, x: _oracle_transfer(self.oracle, *self.items[l], x, True),
                            restrict=lambda l, x: _oracle_transfer(self.oracle, *self.items[l], x, False))

    def problem(self, seed=51):
        from disco4est_amd import mesh as M
        n = self.nodes[-1]
        return M.splitmix64_uniform(seed, n) - 0.5, M.splitmix64_uniform(seed + 1, n) - 0.5


class _Device:
    """plans, transfers and the Multigrid object of an _OracleLevels hierarchy"""

    def __init__(self, L, gpu):
        import torch
        from disco4est_amd import Plan, Transfer, Multigrid
        self.L, self.gpu = L, gpu
        self.plans = []
        for m, (J, rst, sides) in zip(L.meshes, L.geo):
            p = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, 0)
            p.set_geometry(J, rst)
            p.set_faces(sides, 10.0, 0)
            self.plans.append(p)
        self.transfers = [Transfer(h, dH, dh) for (h, dH, dh) in L.items]
        self.keep = []
        if L.term:
            top = L.n_levels - 1
            dcoeff = _t(L.coeff, gpu)
            self.plans[top].set_lhs_coefficient(dcoeff)
            blocks = torch.empty(self.plans[top].matrix_nodes(), dtype=torch.float64, device=gpu)
            self.plans[top].compute_weighted_mass_blocks(dcoeff, blocks)
            self.keep += [dcoeff, blocks]
            for l in range(top - 1, -1, -1):
                out = torch.empty(self.plans[l].matrix_nodes(), dtype=torch.float64, device=gpu)
                self.transfers[l].galerkin_blocks(blocks, out)
                self.plans[l].set_lhs_element_blocks(out)
                self.keep.append(out)
                blocks = out
        self.mg = Multigrid(self.plans, self.transfers)

    def close(self):
        self.mg.destroy()
        for t in self.transfers:
            t.destroy()
        for p in self.plans:
            p.destroy()


SM = dict(cheby_imax=3, cheby_eigs_cg_imax=5, cheby_eigs_lmax_lmin_ratio=30.0, cheby_eigs_max_multiplier=1.1, cheby_use_new_cg_eigs=1)
# bottom CG stopped by its iteration count (atol = rtol = 0): a count that cannot depend on the last bit
BOTTOM = {"cg": ("cg", (12, 0.0, 0.0)), "cheby": ("cheby", (6, 5, 30.0, 1.1, 1))}


def _ref_parts(n_levels, reuse, zero, bottom):
    sm = RM.ChebySmoother(n_levels, SM["cheby_imax"], SM["cheby_eigs_cg_imax"], SM["cheby_eigs_lmax_lmin_ratio"], SM["cheby_eigs_max_multiplier"],
                          reuse[0], reuse[1], SM["cheby_use_new_cg_eigs"], zero)
    kind, args = BOTTOM[bottom]
    return sm, (RM.BottomCG(*args) if kind == "cg" else RM.BottomCheby(*args))


def _configure(mg, reuse, zero, bottom):
    code = mg.set_smoother_cheby(SM["cheby_imax"], SM["cheby_eigs_cg_imax"], SM["cheby_eigs_lmax_lmin_ratio"], SM["cheby_eigs_max_multiplier"],
                                 reuse[0], reuse[1], SM["cheby_use_new_cg_eigs"], zero)
    assert code == 0
    kind, args = BOTTOM[bottom]
    if kind == "cg":
        mg.set_bottom_solver_cg(*args)
    else:
        mg.set_bottom_solver_cheby(*args)
    assert mg.ready() == 1


def _eigs_of(sm, bottom):
    e = list(sm.eigs)
    if bottom.eig is not None:
        e[0] = bottom.eig
    return np.array(e)


def _cycles_ref(L, kernels, noise_seed, reuse, zero, bottom, u0, rhs, indices):
    """the restatement's V-cycles with the given indices, one after another; returns per cycle (u, r2, eigs, bottom iterations)"""
    L.noise = np.random.default_rng(noise_seed) if noise_seed is not None else None
    h = L.hierarchy(kernels)
    sm, bs = _ref_parts(L.n_levels, reuse, zero, bottom)
    out, u = [], u0
    for idx in indices:
        u, r2 = RM.vcycle(h, sm, bs, u, rhs, idx)
        out.append((u, r2, _eigs_of(sm, bs), bs.iterations))
    L.noise = None
    return out


HIERARCHIES = [("hp3", False), ("hanging2", False), ("hp3", True)]
CONFIGS = [((0, 0), 0, "cg"), ((1, 1), 0, "cheby"), ((1, 0), 1, "cg"), ((0, 0), 0, "cheby")]


@pytest.mark.parametrize("reuse,zero,bottom", CONFIGS)
@pytest.mark.parametrize("kind,term", HIERARCHIES)
def test_vcycle_against_the_restatement(gpu, hiplib, oracle, kind, term, reuse, zero, bottom):
    """case 1: V-cycles with vcycle_index 0 and then 1 from a random start: u, vcycle_r2 and eigs[] after each"""
    import torch
    L = _OracleLevels(kind, oracle, term)
    D = _Device(L, gpu)
    try:
        u0, rhs = L.problem()
        indices = [0, 1]
        ref = _cycles_ref(L, "oracle", None, reuse, zero, bottom, u0, rhs, indices)
        cpu_a = _cycles_ref(L, "numpy", None, reuse, zero, bottom, u0, rhs, indices)
        cpu_b = _cycles_ref(L, "numpy", 1234, reuse, zero, bottom, u0, rhs, indices)
        _configure(D.mg, reuse, zero, bottom)
        du, drhs = _t(u0, gpu), _t(rhs, gpu)
        dAu = torch.full_like(du, float("nan"))
        for k, idx in enumerate(indices):
            r2 = D.mg.vcycle(du, drhs, dAu, idx)
            eigs, _, bit = D.mg.info()
            u_ref, r2_ref, e_ref, bit_ref = ref[k]
            dist = (_rel(cpu_b[k][0], cpu_a[k][0]), abs(cpu_b[k][1] - cpu_a[k][1]) / cpu_a[k][1], _rel_each(cpu_b[k][2][e_ref > 0], cpu_a[k][2][e_ref > 0]))
            got = (_rel(du.cpu().numpy(), u_ref), abs(r2 - r2_ref) / r2_ref, _rel_each(eigs[e_ref > 0], e_ref[e_ref > 0]))
            print("vcycle %s term=%d reuse=%s zero=%d bottom=%s index=%d: CPU distance (u, r2, eigs) = %.3e %.3e %.3e, device = %.3e %.3e %.3e"
                  % ((kind, term, reuse, zero, bottom, idx) + dist + got))
            assert bit == bit_ref
            assert np.array_equal(eigs > 0, e_ref > 0)             # the same levels hold a bound
            assert got[0] <= FACTOR * dist[0], ("u", got[0], dist[0])
            assert got[1] <= FACTOR * dist[1], ("r2", got[1], dist[1])
            assert got[2] <= FACTOR * dist[2], ("eigs", got[2], dist[2])
            # vcycle_r2 is |rhs - A u|^2 of what the cycle left in u (checked with the oracle, loosely: it is the yardstick's claim)
            r = rhs - L.apply(L.n_levels - 1, du.cpu().numpy())
            assert abs(float(r @ r) - r2) <= 1e-8 * r2
    finally:
        D.close()
        L.close()


def _gap(hist, lo, hi):
    """the stop index j in [lo, hi) where the restated history leaves the widest gap below everything before it, and a threshold in the
    middle of that gap (in log scale): a last-bit difference cannot move the count (as tests/test_krylov_gpu.py::_gap)"""
    h = np.asarray(hist, dtype=np.float64)
    best, jb = -1.0, None
    for j in range(max(lo, 2), min(hi, len(h))):
        g = np.log(h[1:j].min()) - np.log(h[j])
        if g > best:
            best, jb = g, j
    assert best > 0.05, best
    return jb, float(np.sqrt(h[1:jb].min() * h[jb]))


def _solve_ref(L, kernels, noise_seed, reuse, zero, bottom, u0, rhs, imax, atol, rtol):
    L.noise = np.random.default_rng(noise_seed) if noise_seed is not None else None
    h = L.hierarchy(kernels)
    sm, bs = _ref_parts(L.n_levels, reuse, zero, bottom)
    u, n, hist = RM.solve(h, sm, bs, u0, rhs, imax, atol, rtol)
    L.noise = None
    return u, n, np.array(hist), _eigs_of(sm, bs)


@pytest.mark.parametrize("kind,term", HIERARCHIES)
def test_solve_against_the_restatement(gpu, hiplib, oracle, kind, term):
    """case 2: cycle count, r2 history, final u; the stop falls in a gap of the restated history"""
    import torch
    # no reuse: every smoother call takes its own bound.  (A 5-iteration bound kept from an earlier, rougher iterate is too low for a
    # convergent smoother on these meshes -- in the restatement as on the device; the reuse rules are held to the restatement cycle by
    # cycle in test_vcycle_against_the_restatement.)
    reuse, zero, bottom = (0, 0), 0, "cg"
    L = _OracleLevels(kind, oracle, term)
    D = _Device(L, gpu)
    try:
        u0, rhs = L.problem(61)
        _, _, h_all, _ = _solve_ref(L, "oracle", None, reuse, zero, bottom, u0, rhs, 8, 0.0, 0.0)
        j, thr = _gap(h_all, 3, 8)                   # r2_j <= thr: stop after cycle j
        atol, rtol, imax = 0.0, float(np.sqrt(thr / h_all[0])), 40
        u_ref, n_ref, h_ref, e_ref = _solve_ref(L, "oracle", None, reuse, zero, bottom, u0, rhs, imax, atol, rtol)
        assert n_ref == j
        ua, na, ha, ea = _solve_ref(L, "numpy", None, reuse, zero, bottom, u0, rhs, imax, atol, rtol)
        ub, nb, hb, eb = _solve_ref(L, "numpy", 4321, reuse, zero, bottom, u0, rhs, imax, atol, rtol)
        assert na == nb == j                         # (else the gap was chosen badly: fix the case, not the tolerance)
        _configure(D.mg, reuse, zero, bottom)
        du, drhs = _t(u0, gpu), _t(rhs, gpu)
        dAu = torch.full_like(du, float("nan"))
        n, hist = D.mg.solve(du, drhs, dAu, imax, atol, rtol)
        eigs, cycles, _ = D.mg.info()
        dist = (_rel(ub, ua), _rel_each(hb, ha), _rel_each(eb[e_ref > 0], ea[e_ref > 0]))
        got = (_rel(du.cpu().numpy(), u_ref), _rel_each(hist, h_ref) if n == n_ref else float("inf"), _rel_each(eigs[e_ref > 0], e_ref[e_ref > 0]))
        print("solve %s term=%d: cycles %d (restatement %d), CPU distance (u, r2 history, eigs) = %.3e %.3e %.3e, device = %.3e %.3e %.3e"
              % ((kind, term, n, n_ref) + dist + got))
        assert n == n_ref == cycles
        assert got[0] <= FACTOR * dist[0], ("u", got[0], dist[0])
        assert got[1] <= FACTOR * dist[1], ("r2", got[1], dist[1])
        assert got[2] <= FACTOR * dist[2], ("eigs", got[2], dist[2])
        assert hist[-1] <= rtol * rtol * hist[0] < hist[-2]
    finally:
        D.close()
        L.close()


def _fcg_ref(L, kernels, noise_seed, pc_on, u0, rhs, imax, atol, rtol):
    L.noise = np.random.default_rng(noise_seed) if noise_seed is not None else None
    h = L.hierarchy(kernels)
    top = L.n_levels - 1

    def pc(r):
        sm, bs = _ref_parts(L.n_levels, (0, 0), 0, "cg")     # (every pc call starts with vcycle_num_finished = 0: nothing to carry over)
        return RM.pc_apply(h, sm, bs, r, 1, 0.0, 0.0)

    out = RS.fcg_solve(lambda x: L.apply(top, x), u0, rhs, imax, atol, rtol, pc=pc if pc_on else None)
    L.noise = None
    return out


@pytest.mark.parametrize("kind,term", [("hp3", True), ("hanging2", False)])
def test_preconditioner_and_fcg(gpu, hiplib, oracle, kind, term):
    """case 3: pc_apply is the solve from zero; Plan.fcg_solve(pc=mg) -- the C pointer path -- against the restated FCG with the restated
    preconditioner; strictly fewer iterations than without a preconditioner"""
    import torch
    L = _OracleLevels(kind, oracle, term)
    D = _Device(L, gpu)
    try:
        u0, rhs = L.problem(71)
        top = D.plans[-1]
        _configure(D.mg, (0, 0), 0, "cg")
        D.mg.set_pc(1, 0.0, 0.0)
        dr = _t(rhs, gpu)
        z = torch.full_like(dr, float("nan")); z2 = torch.zeros_like(dr); Au = torch.empty_like(dr)
        D.mg.pc_apply(dr, z)
        n, _ = D.mg.solve(z2, dr, Au, 1, 0.0, 0.0)
        assert n == 1 and torch.equal(z, z2)
        assert isinstance(D.mg.pc_fn, int) and D.mg.pc_fn != 0 and D.mg.pc_ctx == D.mg.handle
        # the stop of the preconditioned solve in a gap of its restated history
        _, _, h_all, _ = _fcg_ref(L, "oracle", None, True, u0, rhs, 10, 0.0, 0.0)
        j, tol = _gap(h_all, 4, 10)                  # |r_j| <= tol: stop after update j (count j + 1)
        atol, rtol, imax = 0.0, tol / h_all[0], 300
        u_ref, it_ref, h_ref, _ = _fcg_ref(L, "oracle", None, True, u0, rhs, imax, atol, rtol)
        assert it_ref == j + 1
        ua, ita, ha, _ = _fcg_ref(L, "numpy", None, True, u0, rhs, imax, atol, rtol)
        ub, itb, hb, _ = _fcg_ref(L, "numpy", 777, True, u0, rhs, imax, atol, rtol)
        assert ita == itb == it_ref
        du = _t(u0, gpu); dAu = torch.empty_like(du)
        it, hist = top.fcg_solve(du, dr, dAu, imax, atol, rtol, pc=D.mg)
        dist = (_rel(ub, ua), _rel_each(hb, ha))
        got = (_rel(du.cpu().numpy(), u_ref), _rel_each(hist, h_ref) if it == it_ref else float("inf"))
        # without a preconditioner, to the same tolerance on the same problem
        dv = _t(u0, gpu)
        it_plain, _ = top.fcg_solve(dv, dr, dAu, 2000, atol, rtol, pc=None)
        print("fcg %s term=%d: iterations %d (restatement %d, no preconditioner %d), CPU distance (u, history) = %.3e %.3e, device = %.3e %.3e"
              % ((kind, term, it, it_ref, it_plain) + dist + got))
        assert it == it_ref
        assert got[0] <= FACTOR * dist[0], ("u", got[0], dist[0])
        assert got[1] <= FACTOR * dist[1], ("history", got[1], dist[1])
        assert it < it_plain
    finally:
        D.close()
        L.close()


def _items(seed, n_items, pmax):
    """item lists of tests/test_transfer_gpu.py: random mixes of copies, p- and hp-items; the edges of the compile-time kernels"""
    if pmax == "p19":
        hrefine = np.array([0, 1, 0], dtype=np.int32)
        degH = np.array([17, 17, 18], dtype=np.int32)
        degh = np.zeros(24, dtype=np.int32)
        degh[0] = 19
        degh[8:16] = [17, 18, 19, 19, 18, 17, 19, 18]
        degh[16] = 19
        return hrefine, degH, degh
    if pmax == "p15d3":
        hrefine = np.array([1, 0, 0, 1], dtype=np.int32)
        degH = np.array([15, 15, 16, 3], dtype=np.int32)
        degh = np.zeros(32, dtype=np.int32)
        degh[0:8] = [15, 16, 17, 18, 18, 17, 16, 15]
        degh[8] = 18
        degh[16] = 17
        degh[24:32] = [3, 4, 5, 6, 7, 3, 4, 7]     # + 4: beyond the fast kernels' range, the whole item takes the generic path
        return hrefine, degH, degh
    rng = np.random.RandomState(seed)
    hrefine = rng.randint(0, 2, size=n_items).astype(np.int32)
    degH = rng.randint(1, pmax, size=n_items).astype(np.int32)
    degh = np.zeros(8 * n_items, dtype=np.int32)
    for k in range(n_items):
        nc = 8 if hrefine[k] else 1
        degh[8 * k:8 * k + nc] = degH[k] + rng.randint(0, 3, size=nc)
    hrefine[0], degh[0] = 0, degH[0]   # a pure copy item
    return hrefine, degH, degh


@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("seed,n_items,pmax", [(1, 7, 4), (2, 40, 6), (3, 9, 9), (4, 3, 13), (7, 3, "p19"), (9, 4, "p15d3"), (11, 64, 8)])
def test_prolong_add_is_prolong_then_add(gpu, hiplib, seed, n_items, pmax, generic, monkeypatch):
    """case 4: bit-identical to prolong into a scratch vector followed by +=; copies, p-items and hp-items, the compile-time kernels and
    (generic = True: D4EST_HIP_TRANSFER_GENERIC) the runtime-size kernel"""
    import torch
    from disco4est_amd import Transfer, mesh as M
    if generic:
        monkeypatch.setenv("D4EST_HIP_TRANSFER_GENERIC", "1")
    else:
        monkeypatch.delenv("D4EST_HIP_TRANSFER_GENERIC", raising=False)
    hrefine, degH, degh = _items(seed, n_items, pmax)
    t = Transfer(hrefine, degH, degh)
    xc = _t(M.splitmix64_uniform(seed, t.coarse_nodes) - 0.5, gpu)
    u0 = _t(1e3 * (M.splitmix64_uniform(seed + 50, t.fine_nodes) - 0.5), gpu)     # (different magnitudes: the sum rounds)
    scratch = torch.full((t.fine_nodes,), float("nan"), dtype=torch.float64, device=gpu)
    t.prolong(xc, scratch)
    want = u0.clone()
    want += scratch
    got = u0.clone()
    t.prolong_add(xc, got)
    assert torch.equal(got, want)
    assert not torch.equal(got, u0)
    t.destroy()


def test_solve_is_reproducible_and_leaves_the_operators_alone(gpu, hiplib, oracle):
    """case 5: two solves bit-identical; the allreduce hook counts of every plan; every plan's apply_lhs unchanged after destroy"""
    import torch
    L = _OracleLevels("hp3", oracle, True)
    D = _Device(L, gpu)
    try:
        u0, rhs = L.problem(81)
        xs = [_t(np.linspace(-1.0, 1.0, n) ** 3, gpu) for n in L.nodes]
        before = []
        for p, x in zip(D.plans, xs):
            y = torch.empty_like(x); p.apply_lhs(x, y); before.append(y)
        reuse, imax_e, imax_be = (0, 0), SM["cheby_eigs_cg_imax"], BOTTOM["cheby"][1][1]
        runs = []
        for hooked in (False, True, True):
            calls = [[] for _ in D.plans]
            for p, c in zip(D.plans, calls):
                p.set_comm(allreduce=(lambda ptr, n, c=c: c.append(n)) if hooked else None)
            _configure(D.mg, reuse, 0, "cheby")
            du = _t(u0, gpu); dAu = torch.empty_like(du)
            n, hist = D.mg.solve(du, _t(rhs, gpu), dAu, 4, 0.0, 1e-30)
            runs.append((n, hist.copy(), du.cpu().numpy(), dAu.cpu().numpy(), D.mg.info()[0].copy(), calls))
        for p in D.plans:
            p.set_comm()
        n, hist, u, Au, eigs, _ = runs[0]
        assert n >= 2
        for other in runs[1:]:
            assert other[0] == n and np.array_equal(other[1], hist) and np.array_equal(other[2], u) and np.array_equal(other[3], Au)
            assert np.array_equal(other[4], eigs)
        # hook calls, derived from the settings: a cg_eigs of imax iterations reduces 1 + 2 imax times (one scalar each); the solve itself
        # reduces r2 once before the first cycle and once after each (finest plan only); cycle k runs expected_eigs_calls(...)[l]
        # cg_eigs on level l >= 1 and one (the bottom Chebyshev solver's) on level 0
        calls = runs[1][5]
        top = L.n_levels - 1
        for l in range(L.n_levels):
            if l == 0:
                want = n * (1 + 2 * imax_be)
            else:
                want = sum(RM.expected_eigs_calls(L.n_levels, reuse[0], reuse[1], k)[l] for k in range(n)) * (1 + 2 * imax_e)
            if l == top:
                want += 1 + n
            assert len(calls[l]) == want and set(calls[l]) == {1}, (l, len(calls[l]), want)
        D.mg.destroy()
        for p, x, y0 in zip(D.plans, xs, before):
            y = torch.empty_like(x); p.apply_lhs(x, y)
            assert torch.equal(y, y0)
    finally:
        D.close()
        L.close()


def test_invalid_input_is_reported_by_codes(gpu, hiplib, oracle):
    """case 6: d4est_hip_multigrid_check and _ready and the smoother setter's code; no process aborts"""
    from disco4est_amd import Multigrid, multigrid_check
    L = _OracleLevels("hanging2", oracle)
    D = _Device(L, gpu)
    try:
        lib = hiplib
        assert lib.d4est_hip_multigrid_check(1, None, None) == 1 and lib.d4est_hip_multigrid_check(0, None, None) == 1
        assert lib.d4est_hip_multigrid_check(2, None, None) == 2
        assert multigrid_check(D.plans, D.transfers) == 0
        assert multigrid_check(D.plans[:1], []) == 1
        assert multigrid_check([D.plans[0], None], D.transfers) == 2
        assert multigrid_check(D.plans, [None]) == 2
        assert multigrid_check(D.plans[::-1], D.transfers) == 3          # coarse and fine swapped: the node counts do not match
        assert multigrid_check([D.plans[1], D.plans[1]], D.transfers) == 3
        with pytest.raises(ValueError, match="returned 3"):
            Multigrid(D.plans[::-1], D.transfers)
        mg = Multigrid(D.plans, D.transfers)
        assert mg.ready() == 0
        assert mg.set_smoother_cheby(3, 5, 30.0, 1.1, 0, 0, 1, 0) == 0
        assert mg.ready() == 0                                            # no bottom solver yet
        mg.set_bottom_solver_cg(10, 0.0, 1e-10)
        assert mg.ready() == 1
        # the reference's abort at smoother_cheby.c:313-318: a code, and the object is left not ready
        assert mg.set_smoother_cheby(3, 5, 30.0, 1.1, 0, 0, 1, 1) == 1
        assert mg.ready() == 0
        with pytest.raises(RuntimeError, match="smoother"):
            mg.vcycle(None, None, None)
        assert mg.set_smoother_cheby(3, 0, 30.0, 1.1, 0, 0, 1, 0) == 2 and mg.ready() == 0
        assert mg.set_smoother_cheby(3, 5, 30.0, 1.1, 1, 0, 1, 1) == 0 and mg.ready() == 1
        mg.destroy()
    finally:
        D.close()
        L.close()
