"""The Schwarz smoother behind the device V-cycle object (d4est_hip_multigrid_set_smoother_schwarz), the reuse_smoother bottom solver and
the device code of the smoother loop (the residual formed in the subdomain CG's start, the iterate without a final host read).

Tolerances.  Cycle parity follows tests/test_vcycle_gpu.py: the restatement (tests/ref_multigrid.py driven by
tests/ref_schwarz_smoother.py) runs twice, once on the device's apply and once with every apply perturbed by seeded noise of
relative-inf size RTOL = 1e-12 (the difference admitted per apply); the object must be within FACTOR = 10 x the distance between the
two runs.  The subdomain solves of the parity cases stop by their iteration count (atol = rtol = 1e-15, as
tests/test_schwarz_gpu.py::test_multigrid_schwarz_smoother_parity), so that a last-bit difference cannot move a count.  The smoother
against the oracle uses that test's tolerances (1e-9 on u, 1e-8 on r).  Fused / unfused / public forms are compared with torch.equal."""
import numpy as np
import pytest

from tests import mg_schwarz_levels as L
from tests import ref_multigrid as RM
from tests import ref_schwarz_smoother as RZ

pytestmark = pytest.mark.gpu
FACTOR = 10.0
ITER = 2                          # smoother_iterations of the parity cases
BOTTOM_CG = (12, 0.0, 0.0)        # stopped by its count, as tests/test_vcycle_gpu.py


def _configure(mg, H, bottom, iterations=ITER):
    assert mg.set_smoother_schwarz(H.schwarz, iterations) == 0
    if bottom == "cg":
        mg.set_bottom_solver_cg(*BOTTOM_CG)
    else:
        mg.set_bottom_solver_reuse_smoother()
    assert mg.ready() == 1


def _ref_parts(H, bottom, iterations=ITER):
    sm = RZ.SchwarzSmoother(iterations, H.schwarz_iterate)
    return sm, (RM.BottomCG(*BOTTOM_CG) if bottom == "cg" else RZ.BottomReuseSmoother(sm))


@pytest.mark.parametrize("bottom", ["cg", "reuse"])
@pytest.mark.parametrize("kind", ["two", "three"])
def test_cycle_solve_and_pc_against_the_restatement(gpu, hiplib, kind, bottom):
    """case 1: V-cycles with index 0 and 1, a solve of three cycles and pc_apply: u and r2 against the restatement on device primitives"""
    import torch
    H = L.Levels(kind, gpu)
    try:
        u0, rhs = H.problem(51)
        mg = H.multigrid()
        _configure(mg, H, bottom)

        def cycles(noise):
            h = H.hierarchy(noise)
            sm, bs = _ref_parts(H, bottom)
            out, u = [], u0
            for idx in (0, 1):
                u, r2 = RM.vcycle(h, sm, bs, u, rhs, idx)
                out.append((u, r2))
            return out

        ref, pert = cycles(None), cycles(np.random.default_rng(1234))
        du, drhs = L.t(u0, gpu), L.t(rhs, gpu)
        dAu = torch.full_like(du, float("nan"))
        for k, idx in enumerate((0, 1)):
            r2 = mg.vcycle(du, drhs, dAu, idx)
            dist = (L.rel(pert[k][0], ref[k][0]), abs(pert[k][1] - ref[k][1]) / ref[k][1])
            got = (L.rel(du.cpu().numpy(), ref[k][0]), abs(r2 - ref[k][1]) / ref[k][1])
            print("vcycle %s bottom=%s index=%d: noise distance (u, r2) = %.3e %.3e, device = %.3e %.3e" % ((kind, bottom, idx) + dist + got))
            assert got[0] <= FACTOR * dist[0], ("u", got[0], dist[0])
            assert got[1] <= FACTOR * dist[1], ("r2", got[1], dist[1])
            r = rhs - H.apply(H.n_levels - 1, du.cpu().numpy())
            assert abs(float(r @ r) - r2) <= 1e-8 * r2
        eigs, _, bit = mg.info()
        assert np.array_equal(eigs, -np.ones(H.n_levels))            # no eigenvalue state
        assert bit == (BOTTOM_CG[0] if bottom == "cg" else 0)

        def solve(noise):
            sm, bs = _ref_parts(H, bottom)
            return RM.solve(H.hierarchy(noise), sm, bs, u0, rhs, 3, 0.0, 0.0)

        (ua, na, ha), (ub, nb, hb) = solve(None), solve(np.random.default_rng(4321))
        du = L.t(u0, gpu)
        n, hist = mg.solve(du, drhs, dAu, 3, 0.0, 0.0)
        dist = (L.rel(ub, ua), float(np.max(np.abs(np.array(hb) - np.array(ha)) / np.array(ha))))
        got = (L.rel(du.cpu().numpy(), ua), float(np.max(np.abs(hist - np.array(ha)) / np.array(ha))) if n == na else float("inf"))
        print("solve %s bottom=%s: cycles %d (restatement %d), noise distance (u, r2 history) = %.3e %.3e, device = %.3e %.3e"
              % ((kind, bottom, n, na) + dist + got))
        assert n == na == nb == 3
        assert got[0] <= FACTOR * dist[0] and got[1] <= FACTOR * dist[1], (got, dist)
        assert hist[-1] < hist[0]

        def pc(noise):
            sm, bs = _ref_parts(H, bottom)
            return RM.pc_apply(H.hierarchy(noise), sm, bs, rhs, 1, 0.0, 0.0)

        za, zb = pc(None), pc(np.random.default_rng(99))
        mg.set_pc(1, 0.0, 0.0)
        z = torch.full_like(drhs, float("nan"))
        mg.pc_apply(drhs, z)
        print("pc_apply %s bottom=%s: noise distance %.3e, device %.3e" % (kind, bottom, L.rel(zb, za), L.rel(z.cpu().numpy(), za)))
        assert L.rel(z.cpu().numpy(), za) <= FACTOR * L.rel(zb, za)
    finally:
        H.close()


def test_smoother_through_the_object_against_the_oracle(gpu, hiplib, oracle):
    """case 2: one smoother call of the object on the top level against oracle.schwarz_smoother (u and the exit r); the mesh, options and
    tolerances of tests/test_schwarz_gpu.py::test_multigrid_schwarz_smoother_parity"""
    import torch
    from disco4est_amd import Plan, Transfer, Multigrid, mesh as M
    from disco4est_amd.schwarz import Schwarz
    mp = M.SineMap(0.04)
    mf, mc = M.BrickMesh(2, 2), M.BrickMesh(2, 1)
    plans = []
    for m in (mc, mf):
        J, rst = m.geometry(mp); sides = m.build_sides(mp)
        p = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, 0)
        p.set_geometry(J, rst)
        p.set_faces(sides, 10.0, 0)
        plans.append(p)
    oracle.set_operator(mf, J, rst, sides, 10.0, 0, threads=1)
    sz = Schwarz(mf, sides, J, rst, 2, 6, 1e-15, 1e-15, 10.0, 0)
    degh = np.zeros(8 * 64, dtype=np.int32)
    degh[0::8] = 2
    T = Transfer(np.zeros(64, np.int32), np.full(64, 1, np.int32), degh)
    mg = Multigrid(plans, [T])
    try:
        assert mg.set_smoother_schwarz([None, sz], 3) == 0
        u0 = M.splitmix64_uniform(91, mf.local_nodes) - 0.5
        rhs = M.splitmix64_uniform(92, mf.local_nodes) - 0.5
        u_ref, r_ref = oracle.schwarz_smoother(sz.metadata, u0, rhs, 3, 6, 1e-15, 1e-15)
        u = L.t(u0, gpu); r = torch.full_like(u, float("nan")); Au = torch.full_like(u, float("nan"))
        mg.smooth_level(1, u, L.t(rhs, gpu), Au, r)
        print("smoother vs oracle: u %.3e, r %.3e" % (L.rel(u.cpu().numpy(), u_ref), L.rel(r.cpu().numpy(), r_ref)))
        assert L.rel(u.cpu().numpy(), u_ref) <= 1e-9
        assert L.rel(r.cpu().numpy(), r_ref) <= 1e-8
    finally:
        mg.destroy(); sz.destroy(); T.destroy()
        for p in plans:
            p.destroy()


@pytest.mark.parametrize("kind", ["two", "mixed", "hanging"])
def test_fused_and_unfused_residual_are_bit_identical(gpu, hiplib, kind, monkeypatch):
    """case 3: a three-iteration smoother call with the residual formed in the CG start (D4EST_HIP_SCHWARZ_FUSED_RESIDUAL=1), with
    D4EST_HIP_SCHWARZ_UNFUSED_RESIDUAL=1 (both read when the handle is created) and through the public d4est_hip_schwarz_smooth:
    torch.equal u and r; a V-cycle is bit-identical from run to run"""
    import torch
    sub = (12, 1e-15, 1e-4)               # tolerance-stopped subdomain solves: identical inputs must give identical counts
    monkeypatch.delenv("D4EST_HIP_SCHWARZ_UNFUSED_RESIDUAL", raising=False)
    monkeypatch.setenv("D4EST_HIP_SCHWARZ_FUSED_RESIDUAL", "1")
    H = L.Levels(kind, gpu, sub=sub, schwarz_levels=[1])          # its top-level handle: fused
    try:
        top = H.n_levels - 1
        monkeypatch.setenv("D4EST_HIP_SCHWARZ_UNFUSED_RESIDUAL", "1")
        unfused = H.new_schwarz(top, sub)
        monkeypatch.delenv("D4EST_HIP_SCHWARZ_UNFUSED_RESIDUAL")
        monkeypatch.delenv("D4EST_HIP_SCHWARZ_FUSED_RESIDUAL")
        u0, rhs = H.problem(61)
        drhs = L.t(rhs, gpu)
        mg = H.multigrid()
        out = {}
        for name, handle in (("fused", H.schwarz[top]), ("unfused", unfused)):
            assert mg.set_smoother_schwarz([None, handle], 3) == 0
            u = L.t(u0, gpu); r = torch.full_like(u, float("nan")); Au = torch.full_like(u, float("nan"))
            mg.smooth_level(top, u, drhs, Au, r)
            out[name] = (u, r, handle.info())
        u = L.t(u0, gpu); r = torch.full_like(u, float("nan"))
        H.schwarz[top].smooth(H.plans[top], u, drhs, r, 3)
        out["public"] = (u, r, H.schwarz[top].info())
        for name in ("unfused", "public"):
            assert torch.equal(out[name][0], out["fused"][0]) and torch.equal(out[name][1], out["fused"][1]), name
            assert np.array_equal(out[name][2][0], out["fused"][2][0]) and np.array_equal(out[name][2][1], out["fused"][2][1])
        assert not torch.equal(out["fused"][0], L.t(u0, gpu)) and bool(torch.isfinite(out["fused"][1]).all())
        # r is rhs - A u of the iterate returned
        Au = torch.empty_like(u)
        H.plans[top].apply_lhs(out["fused"][0], Au)
        assert float((out["fused"][1] - (drhs - Au)).abs().max()) <= 1e-11 * float(drhs.abs().max())
        # run to run
        assert mg.set_smoother_schwarz([None, H.schwarz[top]], 1) == 0
        mg.set_bottom_solver_cg(*BOTTOM_CG)
        runs = []
        for _ in range(2):
            u = L.t(u0, gpu); Au = torch.full_like(u, float("nan"))
            runs.append((mg.vcycle(u, drhs, Au, 0), u))
        assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])
        unfused.destroy()
    finally:
        H.close()


def test_public_iterate_and_get_info_are_unchanged(gpu, hiplib):
    """case 4: after a V-cycle get_info works; the iterate the smoother makes without its final host read leaves the same u, iteration
    counts and residuals as the public d4est_hip_schwarz_iterate on the same u and r, whose return value is the sweep count"""
    import torch
    sub = (12, 1e-15, 1e-4)
    H = L.Levels("two", gpu, sub=sub, schwarz_levels=[1])
    try:
        sz, plan = H.schwarz[1], H.plans[1]
        mg = H.multigrid()
        assert mg.set_smoother_schwarz([None, sz], 1) == 0
        mg.set_bottom_solver_cg(*BOTTOM_CG)
        u0, rhs = H.problem(71)
        drhs = L.t(rhs, gpu)
        u = L.t(u0, gpu); Au = torch.empty_like(u)
        mg.vcycle(u, drhs, Au, 0)
        it_v, res_v = sz.info()
        assert it_v.shape == (64,) and np.all(it_v >= 0) and np.all(it_v <= sub[0]) and np.all(np.isfinite(res_v))
        # one smoother call = one iterate on r = rhs - A u0, then the exit residual
        u1 = L.t(u0, gpu); r1 = torch.empty_like(u1)
        mg.smooth_level(1, u1, drhs, Au, r1)
        it_s, res_s = sz.info()
        u2 = L.t(u0, gpu); A0 = torch.empty_like(u2)
        plan.apply_lhs(u2, A0)
        sweeps = sz.iterate(u2, drhs + (-1.0) * A0)
        it_p, res_p = sz.info()
        assert torch.equal(u1, u2)
        assert np.array_equal(it_s, it_p) and np.array_equal(res_s, res_p)
        # sweeps in which any subdomain still iterated: a subdomain that broke at iteration k did k + 1 sweeps, one that ran out did `iter`
        assert sweeps == int(np.max(np.where(it_p < sub[0], it_p + 1, sub[0])))
        assert 0 < sweeps <= sub[0]
    finally:
        H.close()


def test_setter_codes(gpu, hiplib):
    """case 6: the codes of set_smoother_schwarz, each leaving the object not ready"""
    from disco4est_amd import Plan, Transfer, Multigrid, mesh as M
    H = L.Levels("two", gpu)
    try:
        mg = H.multigrid()
        mg.set_bottom_solver_cg(*BOTTOM_CG)
        assert mg.ready() == 0
        assert mg.set_smoother_schwarz(H.schwarz, 1) == 0 and mg.ready() == 1
        assert mg.set_smoother_schwarz([H.schwarz[0], None], 1) == 1 and mg.ready() == 0          # a NULL entry on a level >= 1
        with pytest.raises(RuntimeError, match="smoother"):
            mg.vcycle(None, None, None)
        assert mg.set_smoother_schwarz([None, H.schwarz[1]], 1) == 0 and mg.ready() == 1           # level 0 may be NULL ...
        mg.set_bottom_solver_reuse_smoother()
        assert mg.ready() == 0                                                                     # ... but not under reuse_smoother
        assert mg.set_smoother_schwarz(H.schwarz, 1) == 0 and mg.ready() == 1
        assert mg.set_smoother_schwarz([H.schwarz[0], H.schwarz[0]], 1) == 2 and mg.ready() == 0   # node counts
        assert mg.set_smoother_schwarz(H.schwarz, 1, subdomain_iter=0) == 5 and mg.ready() == 0    # subdomain options <= 0
        assert mg.set_smoother_schwarz(H.schwarz, 1, subdomain_rtol=0.0) == 5 and mg.ready() == 0
        assert mg.set_smoother_schwarz(H.schwarz, 1, subdomain_atol=-1.0) == 5 and mg.ready() == 0
        # the Chebyshev smoother covers level 0 by itself
        assert mg.set_smoother_cheby(3, 5, 30.0, 1.1, 0, 0, 1, 0) == 0 and mg.ready() == 1
        # a plan with ghost sides: one shard of a two-shard brick
        plans = []
        for deg in (2, 4):
            m = M.BrickMesh(2, deg, first=0, count=32)
            J, rst = m.geometry(H.mp); sides = m.build_sides(H.mp)
            assert np.any(np.asarray(sides["side_nbr"]) <= -2)
            p = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, 0)
            p.set_geometry(J, rst)
            p.set_faces(sides, 10.0, 0)
            plans.append(p)
        degh = np.zeros(8 * 32, dtype=np.int32)
        degh[0::8] = 4
        T = Transfer(np.zeros(32, np.int32), np.full(32, 2, np.int32), degh)
        shard = Multigrid(plans, [T])
        shard.set_bottom_solver_cg(*BOTTOM_CG)
        assert shard.set_smoother_schwarz(H.schwarz, 1) == 4 and shard.ready() == 0
        shard.destroy(); T.destroy()
        for p in plans:
            p.destroy()
    finally:
        H.close()


def test_three_cycles_contract(gpu, hiplib):
    """case 7: the 64-element problem of tests/test_multigrid_gpu.py::test_two_grid_cycle_with_schwarz_smoother through the object: the
    error falls by more than 0.6 per cycle and three cycles beat the same number of Schwarz iterations alone"""
    import torch
    from disco4est_amd import mesh as M
    H = L.Levels("two", gpu, sub=(12, 1e-15, 1e-4), coarse_prefactor=10.0 * 4.0, schwarz_levels=[1])
    try:
        mf, pf = H.meshes[1], H.plans[1]
        x, y, z = mf.nodal_coords(H.mp)
        u_exact = L.t(np.sin(2.0 * x) * np.cos(1.5 * y) + z * z + 0.02 * (M.splitmix64_uniform(3, mf.local_nodes) - 0.5), gpu)
        rhs = torch.zeros_like(u_exact)
        pf.apply_aij(u_exact, rhs)
        mg = H.multigrid()
        assert mg.set_smoother_schwarz([None, H.schwarz[1]], 1) == 0
        mg.set_bottom_solver_cg(60, 0.0, 0.0)
        err = lambda v: (v - u_exact).norm().item() / u_exact.norm().item()
        u, Au = torch.zeros_like(rhs), torch.zeros_like(rhs)
        history = [err(u)]
        for cycle in range(3):
            mg.vcycle(u, rhs, Au, cycle)
            history.append(err(u))
        us, r = torch.zeros_like(rhs), torch.zeros_like(rhs)
        assert mg.set_smoother_schwarz([None, H.schwarz[1]], 6) == 0
        mg.smooth_level(1, us, rhs, Au, r)                              # smoothing alone, same number of Schwarz iterations
        print("contraction:", history, err(us))
        assert all(b < 0.6 * a for a, b in zip(history[:-1], history[1:])), history
        assert history[-1] < 0.5 * err(us), (history, err(us))
    finally:
        H.close()
