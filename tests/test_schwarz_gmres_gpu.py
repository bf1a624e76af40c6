"""The batched GMRES subdomain solver of the device Schwarz smoother (csrc/d4est_hip_schwarz_gmres.hip,
d4est_hip_schwarz_set_subdomain_solver) against tests/ref_schwarz_gmres.py, the numpy restatement of
d4est_solver_schwarz_subdomain_solver_gmres.c:243-422 (pinned by tests/test_ref_schwarz_gmres.py).

Reference.  The restatement runs once per subdomain with the device's own d4est_hip_schwarz_apply_over_subdomains as its operator
(applied to a field that is zero outside that subdomain; the entry is held to the oracle by tests/test_schwarz_gpu.py), on the
subdomain's slice of the restricted residual; the solutions are weighted and added by the device's add_correction.  What is compared
is the correction u - u0 of the mesh vector, in the norm and at the bound tests/test_schwarz_gpu.py::test_iterate_parity uses for the
CG (1e-9 relative to the largest entry), and final_iter / final_res per subdomain.

Marginal subdomains.  A stop test that the restatement evaluates within 1e-6 (relative) of its threshold may fall the other way on the
device, whose dot products are summed in another order; such subdomains (at most 10 % of a mesh's: the condition
tests/test_ref_schwarz_gmres.py::test_marginal_subdomain_cap holds for the reference alone) are excused from the final_iter / final_res
checks, and the correction is then compared on the elements no excused subdomain touches.

Meshes: tests/schwarz_gmres_cases.py (the issue's "overlap 1" on the level-2 brick is overlap 2 there: a one-node overlap has a
zero-width weight ramp and cannot be built), plus "big" (level 1, p = 7, overlap 8: 4096 restricted nodes per subdomain, the Arnoldi
kernel that keeps its vector in memory instead of registers)."""
import numpy as np
import pytest

from tests import ref_schwarz_gmres as RG
from tests import schwarz_gmres_cases as C

pytestmark = pytest.mark.gpu
DU_TOL = 1e-9            # tests/test_schwarz_gpu.py: _rel(u - u0, u_ref - u0) <= 1e-9
RES_TOL = 1e-6           # final_res, as np.testing.assert_allclose(res, res_ref, rtol=1e-6) there
EARLY = dict(mr=6, cycles=4, atol=1e300, rtol=0.3)          # subdomains leave their loops at different steps, mid-cycle


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


class _Case:
    """one mesh with its Schwarz handle (CG until a test selects GMRES) and the references computed on it so far"""

    def __init__(self, name, gpu):
        from disco4est_amd import mesh as M
        from disco4est_amd.schwarz import Schwarz
        if name == "big":
            self.m = M.BrickMesh(1, 7)
            self.mp = M.SineMap(0.04)
            self.J, self.rst = self.m.geometry(self.mp)
            self.sides = self.m.build_sides(self.mp)
            self.rs = 8
        else:
            self.m, self.mp, self.J, self.rst, self.sides, self.rs = C.build(name)
        self.gpu = gpu
        self.sz = self.new_handle()
        md = self.md = self.sz.metadata
        off = np.concatenate([[0], np.cumsum(md.elem_nodal_size)])
        self.seg = [(int(off[md.sub_first[s]]), int(off[md.sub_first[s + 1]])) for s in range(md.num_subdomains)]
        self.r = C.residual(self.m)
        self.refs = {}

    def new_handle(self, iters=1, atol=1e-15, rtol=1e-15):
        from disco4est_amd.schwarz import Schwarz
        return Schwarz(self.m, self.sides, self.J, self.rst, self.rs, iters, atol, rtol, 10.0, 0)

    def apply_one(self, s):
        """x -> A_s x for one subdomain's slice of a field over the subdomains, by the device's apply_over_subdomains"""
        import torch
        a, b = self.seg[s]
        xin = torch.zeros(self.sz.nodal_size, dtype=torch.float64, device=self.gpu)
        out = torch.empty_like(xin)

        def apply(x):
            xin[a:b] = _t(x, self.gpu)
            self.sz.apply_over_subdomains(xin, out)
            return out[a:b].cpu().numpy()
        return apply

    def restatement(self, r_mesh, o):
        """per subdomain GmresResult on the restricted r_mesh; fields are at element size, zero outside the overlap"""
        import torch
        rr = torch.empty(self.sz.nodal_size, dtype=torch.float64, device=self.gpu)
        self.sz.restrict_field(_t(r_mesh, self.gpu), rr)
        rr = rr.cpu().numpy()
        out = []
        for s, (a, b) in enumerate(self.seg):
            if not np.any(rr[a:b]):
                out.append(None)                        # a zero residual: the device form's stated deviation, du = 0
                continue
            out.append(RG.gmres(self.apply_one(s), rr[a:b], o["mr"], o["cycles"], o["atol"], o["rtol"]))
        return out

    def corrected(self, u0, results):
        """u0 + the weighted sum of the restatement's subdomain solutions (the device's add_correction)"""
        du = np.zeros(self.sz.nodal_size)
        for (a, b), res in zip(self.seg, results):
            if res is not None:
                du[a:b] = res.x
        u = _t(u0, self.gpu)
        self.sz.add_correction(_t(du, self.gpu), u)
        return u.cpu().numpy()

    def reference(self, key, o):
        """the shared reference of a set of options on the case's own residual and u0 = 0: computed once, never modified"""
        if key not in self.refs:
            results = self.restatement(self.r, o)
            u_ref = self.corrected(np.zeros(self.m.local_nodes), results)
            u_ref.setflags(write=False)
            self.refs[key] = (results, u_ref)
        return self.refs[key]

    def gmres_iterate(self, sz, o, u0, r_mesh):
        import torch
        sz.set_subdomain_solver(1, o["mr"])
        sz.subdomain_iter, sz.subdomain_atol, sz.subdomain_rtol = o["cycles"], o["atol"], o["rtol"]
        u = _t(u0, self.gpu)
        applies = sz.iterate(u, _t(r_mesh, self.gpu))
        it, res = sz.info()
        return u.cpu().numpy(), it, res, applies


_CASES = {}


@pytest.fixture(scope="module", autouse=True)
def _close_cases():
    yield
    for c in _CASES.values():
        c.sz.destroy()
    _CASES.clear()


def _case(name, gpu):
    if name not in _CASES:
        _CASES[name] = _Case(name, gpu)
    return _CASES[name]


def _check_against(case, o, key):
    """the assertions of cases 1 and 2; returns the excused subdomains"""
    results, u_ref = case.reference(key, o)
    u, it, res, applies = case.gmres_iterate(case.sz, o, np.zeros(case.m.local_nodes), case.r)
    n_sub = case.md.num_subdomains
    excused = C.excused(results)
    assert len(excused) <= C.EXCUSED_SHARE * n_sub, excused
    keep = np.array([s not in excused for s in range(n_sub)])
    it_ref = np.array([x.itr_used for x in results])
    res_ref = np.array([x.rho for x in results])
    err_res = float(np.max(np.abs(res[keep] - res_ref[keep]) / res_ref[keep]))
    # elements no excused subdomain touches
    ok_elem = np.ones(case.m.n_elements, dtype=bool)
    for s in excused:
        ok_elem[case.md.subdomain(s)[0]] = False
    nodes = np.concatenate([np.arange(case.m.nodal_stride[e], case.m.nodal_stride[e] + (case.m.deg[e] + 1) ** 3) for e in np.nonzero(ok_elem)[0]])
    err_u = float(np.abs(u[nodes] - u_ref[nodes]).max() / np.abs(u_ref).max())
    print("%s %s: inner steps %d .. %d, excused %s, correction %.3e, final_res %.3e, %d batched applies"
          % (key, o, it_ref.min(), it_ref.max(), excused, err_u, err_res, applies))
    assert np.isfinite(u).all()
    np.testing.assert_array_equal(it[keep], it_ref[keep])
    assert err_u <= DU_TOL, err_u
    return excused, it, res, res_ref, keep, applies, err_res


# ---- 1: fixed work ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.NAMES + ("big",))
def test_fixed_work(gpu, hiplib, name):
    """atol = rtol = 1e-300, mr = 4, 2 cycles: 8 inner steps on every subdomain; correction and final_res at the CG test's bound for du"""
    case = _case(name, gpu)
    o = C.FIXED
    excused, it, res, res_ref, keep, applies, err_res = _check_against(case, o, "fixed")
    assert excused == []
    assert np.all(it == 8)
    assert err_res <= DU_TOL, err_res
    # 4 applies per cycle and one more for the residual at the start of the second cycle
    assert applies == 2 * o["mr"] + 1


# ---- 2: the issue's convergent options, and a set under which subdomains do stop early ----------------------------------------------------
@pytest.mark.parametrize("name", C.NAMES)
def test_convergent(gpu, hiplib, name):
    case = _case(name, gpu)
    excused, it, res, res_ref, keep, applies, err_res = _check_against(case, C.CONVERGENT, "convergent")
    assert err_res <= RES_TOL, err_res


@pytest.mark.parametrize("name", ["interior", "hanging"])
def test_early_stop(gpu, hiplib, name):
    """rtol = 0.3 (atol out of the way): subdomains meet the AND test at different steps, some in the middle of a cycle; they are frozen
    until their cycle's update and the host leaves the restart loop when none is left"""
    case = _case(name, gpu)
    reads = case.sz.host_reads()
    excused, it, res, res_ref, keep, applies, err_res = _check_against(case, EARLY, "early")
    assert err_res <= RES_TOL, err_res
    assert it[keep].min() < it[keep].max() and np.any(it[keep] % EARLY["mr"] != 0), it
    assert it.max() < EARLY["mr"] * EARLY["cycles"]
    cycles_run = -(-int(it.max()) // EARLY["mr"])
    assert applies == cycles_run * EARLY["mr"] + (cycles_run - 1)
    assert case.sz.host_reads() - reads == cycles_run                     # one look per restart cycle after the first, the last one ends the loop


# ---- 3: SPD cross-check ------------------------------------------------------------------------------------------------------------------
def test_gmres_and_cg_agree_on_the_spd_operator(gpu, hiplib):
    """uniform mesh: full GMRES (mr = the smallest restricted size) and CG, both driven to 1e-10, give the same correction to 1e-8"""
    case = _case("corner", gpu)
    n_min = int(min(np.sum(case.md.elem_restricted_nodal_size[case.md.sub_first[s]:case.md.sub_first[s + 1]]) for s in range(case.md.num_subdomains)))
    assert n_min == 125
    u0 = np.zeros(case.m.local_nodes)
    o = dict(mr=n_min, cycles=3, atol=1e-10, rtol=1e-10)
    u_g, it_g, res_g, _ = case.gmres_iterate(case.sz, o, u0, case.r)
    cg = case.new_handle(400, 1e-10, 1e-10)
    try:
        u_c = _t(u0, gpu)
        cg.iterate(u_c, _t(case.r, gpu))
        it_c, res_c = cg.info()
        u_c = u_c.cpu().numpy()
    finally:
        cg.destroy()
    print("GMRES(%d) inner steps %s, rho %.3e; CG iterations %s; difference %.3e" % (n_min, it_g, res_g.max(), it_c, _rel(u_g, u_c)))
    assert it_c.max() < 400 and it_g.max() < 3 * n_min
    assert res_g.max() <= 1e-10
    assert _rel(u_g, u_c) <= 1e-8


# ---- 4: d4est_hip_schwarz_smooth -----------------------------------------------------------------------------------------------------------
def test_smooth_with_gmres(gpu, hiplib):
    """2 x { r = rhs - A u; iterate } and the exit residual against tests/ref_schwarz_smoother.SchwarzSmoother fed the restatement;
    bounds of tests/test_schwarz_gpu.py::test_multigrid_schwarz_smoother_parity (1e-9 on u, 1e-8 on r)"""
    import torch
    from disco4est_amd import Plan, mesh as M
    from tests import ref_schwarz_smoother as RZ
    case = _case("corner", gpu)
    m, o = case.m, C.FIXED
    plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, 0)
    plan.set_geometry(case.J, case.rst)
    plan.set_faces(case.sides, 10.0, 0)
    try:
        class H:
            @staticmethod
            def apply(level, u):
                out = torch.empty(m.local_nodes, dtype=torch.float64, device=gpu)
                plan.apply_lhs(_t(u, gpu), out)
                return out.cpu().numpy()

        sm = RZ.SchwarzSmoother(2, lambda level, u, r: case.corrected(u, case.restatement(r, o)))
        u0 = M.splitmix64_uniform(91, m.local_nodes) - 0.5
        rhs = M.splitmix64_uniform(92, m.local_nodes) - 0.5
        u_ref, r_ref = sm.smooth(H, 0, u0, rhs)
        case.sz.set_subdomain_solver("gmres", o["mr"])
        case.sz.subdomain_iter, case.sz.subdomain_atol, case.sz.subdomain_rtol = o["cycles"], o["atol"], o["rtol"]
        u = _t(u0, gpu); r = torch.full_like(u, float("nan"))
        case.sz.smooth(plan, u, _t(rhs, gpu), r, 2)
        print("smooth with GMRES: u %.3e, r %.3e" % (_rel(u.cpu().numpy(), u_ref), _rel(r.cpu().numpy(), r_ref)))
        assert sm.iterate_calls == 2
        assert _rel(u.cpu().numpy(), u_ref) <= 1e-9
        assert _rel(r.cpu().numpy(), r_ref) <= 1e-8
        assert np.linalg.norm(r_ref) < np.linalg.norm(rhs - H.apply(0, u0))
    finally:
        plan.destroy()


# ---- 5: the V-cycle's smoother and the preconditioner on a GMRES handle -----------------------------------------------------------------------
def test_vcycle_smoother_and_pc_follow_the_choice(gpu, hiplib):
    """d4est_hip_multigrid_smooth_level and d4est_hip_pc_schwarz_apply on a GMRES handle equal the same sequence of public calls
    (apply_lhs, the residual, d4est_hip_schwarz_iterate) bit for bit -- and differ from what the CG handle gives"""
    import torch
    from disco4est_amd import PcSchwarz
    from tests import mg_schwarz_levels as L
    o = C.FIXED
    sub = (o["cycles"], o["atol"], o["rtol"])
    H = L.Levels("two", gpu, sub=sub, schwarz_levels=[1])
    pc = None
    try:
        top = H.n_levels - 1
        sz, plan = H.schwarz[top], H.plans[top]
        u0, rhs = H.problem(61)
        drhs = L.t(rhs, gpu)
        mg = H.multigrid()
        assert mg.set_smoother_schwarz([None, sz], 2) == 0

        def by_object():
            u = L.t(u0, gpu); r = torch.full_like(u, float("nan")); Au = torch.full_like(u, float("nan"))
            mg.smooth_level(top, u, drhs, Au, r)
            return u, r

        def by_hand():
            u = L.t(u0, gpu); Au = torch.empty_like(u)
            for _ in range(2):
                plan.apply_lhs(u, Au)
                sz.iterate(u, drhs + (-1.0) * Au)
            plan.apply_lhs(u, Au)
            return u, drhs + (-1.0) * Au

        u_cg, _ = by_object()
        sz.set_subdomain_solver(1, o["mr"])
        assert sz.subdomain_solver()[:2] == (1, o["mr"])
        u_obj, r_obj = by_object()
        it_obj, res_obj = sz.info()
        u_hand, r_hand = by_hand()
        assert torch.equal(u_obj, u_hand) and torch.equal(r_obj, r_hand)
        assert np.all(it_obj == o["mr"] * o["cycles"]) and np.all(np.isfinite(res_obj))
        assert not torch.equal(u_obj, u_cg) and bool(torch.isfinite(u_obj).all())
        # the preconditioner: z = 0; iterate(z, r); residual = r - A z; iterate(z, residual)
        pc = PcSchwarz(sz, plan, 2)
        z = torch.full_like(drhs, float("nan"))
        pc.apply(drhs, z)
        zh = torch.zeros_like(drhs); Au = torch.empty_like(zh)
        sz.iterate(zh, drhs)
        plan.apply_lhs(zh, Au)
        sz.iterate(zh, (-1.0) * Au + drhs)
        assert torch.equal(z, zh) and float(z.abs().max()) > 0
    finally:
        if pc is not None:
            pc.destroy()
        H.close()


# ---- 6: two virtual ranks ------------------------------------------------------------------------------------------------------------------
def test_two_virtual_ranks_against_one(gpu, hiplib):
    """sharded handles (element exchange set, Python hooks) on the level-2 brick, two ranks in lock-step: the gathered correction equals
    one rank's to 1e-10 of its size, the bound of tests/test_schwarz_sharded_gpu.py"""
    import torch
    from disco4est_amd import mesh as M
    from disco4est_amd.schwarz import Schwarz, SchwarzShardNative
    from tests import schwarz_shard_cases as SC
    from tests import test_schwarz_sharded_gpu as SH
    o = C.FIXED
    sub = (o["cycles"], o["atol"], o["rtol"])
    world, level, rs = 2, 2, 2
    deg_global, parts = SC.brick_case(world, level, [2])
    mp = M.SineMap(0.04)
    mg = M.BrickMesh(level, deg_global)
    Jg, rstg = mg.geometry(mp); sg = mg.build_sides(mp)
    u0 = M.splitmix64_uniform(81, mg.local_nodes) - 0.5
    r = M.splitmix64_uniform(82, mg.local_nodes) - 0.5
    single = Schwarz(mg, sg, Jg, rstg, rs, *sub)
    single.set_subdomain_solver(1, o["mr"])
    u_ref = _t(u0, gpu)
    single.iterate(u_ref, _t(r, gpu))
    u_ref = u_ref.cpu().numpy()
    single.destroy()

    def make(rank):
        sh = SchwarzShardNative(level, deg_global, parts, rank, mp, rs, *sub)
        sh.set_subdomain_solver(1, o["mr"])
        return sh

    W = SH._World(world, gpu, make)
    try:
        slices = []
        for first, count in parts:
            lo = int(mg.global_nodal_stride[first])
            slices.append((lo, lo + int(((mg.deg[first:first + count].astype(np.int64) + 1) ** 3).sum())))
        us = [_t(u0[lo:hi], gpu) for lo, hi in slices]
        rr = [_t(r[lo:hi], gpu) for lo, hi in slices]
        applies = W.run(lambda k: W.shards[k].iterate(us[k], rr[k]))
        torch.cuda.synchronize()
        assert applies == [2 * o["mr"] + 1] * world
        got = np.concatenate([u.cpu().numpy() for u in us])
        err = np.abs(got - u_ref).max() / np.abs(u_ref - u0).max()
        print("sharded GMRES iterate, world 2 vs one rank: %.3e" % err)
        assert all(sh.schwarz.subdomain_solver()[0] == 1 for sh in W.shards)
        assert err <= 1e-10, err
    finally:
        W.close()


# ---- 7: determinism, zero residuals --------------------------------------------------------------------------------------------------------
def test_runs_are_bit_identical_and_zero_residuals_stay_zero(gpu, hiplib):
    import torch
    case = _case("interior", gpu)
    o = EARLY
    r = case.r.copy()
    for e in case.md.subdomain(0)[0]:                    # subdomain 0 (a corner of the brick) sees an all-zero residual
        r[case.m.nodal_stride[e]:case.m.nodal_stride[e] + (case.m.deg[e] + 1) ** 3] = 0.0
    u0 = np.zeros(case.m.local_nodes)
    runs = []
    for _ in range(2):
        sz = case.new_handle()
        try:
            runs.append(case.gmres_iterate(sz, o, u0, r))
        finally:
            sz.destroy()
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b)
    u, it, res, _ = runs[0]
    assert np.isfinite(u).all() and np.isfinite(res).all()
    assert it[0] == 0 and res[0] == 0.0
    assert np.all(it[1:] >= 1) and np.all(res[1:] > 0)
    # du of subdomain 0 is zero: the correction is what the restatement gives with that subdomain left out
    u_ref = case.corrected(u0, case.restatement(r, o))
    assert _rel(u, u_ref) <= DU_TOL
    # every residual zero: nothing is solved, nothing is added, nothing is NaN
    ustart = np.linspace(-1.0, 1.0, case.m.local_nodes)
    u, it, res, applies = case.gmres_iterate(case.sz, o, ustart, np.zeros(case.m.local_nodes))
    assert np.array_equal(u, ustart) and np.all(it == 0) and np.all(res == 0.0)
    assert applies == o["mr"]                            # the first cycle runs (as no-ops); the look before the second ends the loop


# ---- 8: the setter ---------------------------------------------------------------------------------------------------------------------------
def test_setter_codes_query_and_the_way_back_to_cg(gpu, hiplib):
    import torch
    case = _case("corner", gpu)
    sz = case.new_handle(5, 1e-15, 1e-15)
    untouched = case.new_handle(5, 1e-15, 1e-15)
    try:
        assert sz.subdomain_solver() == (0, 0, 0)                        # a fresh handle: CG, no workspace
        assert case.md.num_subdomains == 8
        n_min, cap = 125, 128
        for args, code in (((2, 4), 1), ((-1, 4), 1), ((1, 0), 2), ((1, -3), 2), ((1, n_min + 1), 3), ((1, 1000), 3)):
            with pytest.raises(ValueError) as ei:
                sz.set_subdomain_solver(*args)
            assert ei.value.args[1] == code, (args, ei.value.args)
            assert sz.subdomain_solver() == (0, 0, 0)                    # a refused call leaves the handle as it was
        big = _case("big", gpu).new_handle()                             # 4096 restricted nodes per subdomain: only the cap refuses 129
        try:
            with pytest.raises(ValueError) as ei:
                big.set_subdomain_solver(1, cap + 1)
            assert ei.value.args[1] == 4
            big.set_subdomain_solver(1, cap)
            assert big.subdomain_solver()[:2] == (1, cap)
        finally:
            big.destroy()
        mr = 5
        sz.set_subdomain_solver(1, mr)
        ns = case.md.num_subdomains
        want = 8 * ((mr + 1) * sz.nodal_size + ns * ((mr + 1) * mr + 2 * mr + (mr + 1) + 2)) + 4 * 2 * ns
        assert sz.subdomain_solver() == (1, mr, want)
        u = torch.zeros(case.m.local_nodes, dtype=torch.float64, device=gpu)
        sz.iterate(u, _t(case.r, gpu))
        info = sz.info()
        assert (info.solver, info.inner_iter, info.workspace_bytes) == (1, mr, want) and len(info) == 2
        assert np.all(info[0] == 5 * mr)
        sz.set_subdomain_solver(1, 3)                                      # another restart length: the workspace is replaced
        assert sz.subdomain_solver()[2] < want
        sz.set_subdomain_solver("cg")
        assert sz.subdomain_solver() == (0, 0, 0)
        ua, ub = torch.zeros_like(u), torch.zeros_like(u)
        sa = sz.iterate(ua, _t(case.r, gpu))
        sb = untouched.iterate(ub, _t(case.r, gpu))
        assert sa == sb and torch.equal(ua, ub)
        (ia, ra), (ib, rb) = sz.info(), untouched.info()
        assert np.array_equal(ia, ib) and np.array_equal(ra, rb)
        assert not torch.equal(ua, u)
    finally:
        sz.destroy(); untouched.destroy()
