"""GPU sweep over EVERY compile-time instance of the fused nonlinear kernels (csrc/d4est_hip_nonlinear.hip): the 26 (N, NQ) pairs of
D4EST_HIP_FAST_PAIRS and D4EST_HIP_BIG_PAIRS (csrc/d4est_hip_wave.h) in the term form (d4est_hip_apply_nonlinear_term) and in the coefficient form (d4est_hip_plan_linearise, read
back through d4est_hip_plan_lhs_coefficient_arrays), the branches of the host dispatcher launch_fused (the multi launch next to
per-bucket launches, one equal-order bucket, no bucket for the multi kernel, a bucket without a pair, MAXB buckets), ragged last
workgroups, Lobatto quadrature, a hanging mesh, a partition, an empty plan, and the zeroth-order term of apply_lhs on its own scale.

The reference is the oracle's interpolate / galerkin integral / weighted mass around tests/dense_nonlinear.py.  Errors are taken
relative to the reference's infinity norm (RTOL = 1e-12, the fp64 parity bound of this test family) and PER ELEMENT against the element's
own largest reference entry (20 RTOL, as tests/test_faces_gpu.py::test_apply_aij_mixed_p), so one wrong element among several cannot
hide.  Every device vector handed to the library sits between two bands of 64 sentinel doubles which must survive every call; outputs
are pre-filled with NaN where the call overwrites.

tests/test_nonlinear_dense.py pins PAIRS to the macro in the source."""
import ctypes

import numpy as np
import pytest

from tests import dense_nonlinear as DN

pytestmark = pytest.mark.gpu

RTOL = 1e-12
ELEM_RTOL = 20 * RTOL
GUARD = 64
SENTINEL = -1.2345678e77

# D4EST_HIP_FAST_PAIRS then D4EST_HIP_BIG_PAIRS, in the macros' order: (deg + 1, deg_quad + 1)
PAIRS = [(2, 2), (3, 3), (4, 4), (5, 5), (6, 6), (7, 7), (8, 8), (9, 9), (10, 10), (11, 11), (12, 12), (13, 13), (14, 14), (15, 15),
         (16, 16), (2, 3), (3, 4), (4, 5), (8, 9), (3, 6), (4, 6), (8, 10), (17, 17), (18, 18), (19, 19), (20, 20)]
# (k, with b): the powers of the shipped problems (u^5; (b + u)^-7 and its derivative's -8) and the degenerate k = 1, 0
POWERS = [(5, False), (-7, True), (-8, True), (1, True), (0, True)]
COEFF_POWERS = [(-7, True), (5, False)]


def elements_per_workgroup(NQ):
    """WaveCfg::EPB: NQ^2 lanes own an element, a 64-lane workgroup holds as many elements as fit"""
    return max(1, 64 // (NQ * NQ))


def pair_count(NQ):
    """one full workgroup followed by a ragged one: EPB + r elements, 0 < r < EPB; EPB = 1: three workgroups"""
    epb = elements_per_workgroup(NQ)
    return 3 if epb == 1 else epb + {16: 3, 7: 1, 4: 2, 2: 1}[epb]


# ---- guarded device vectors ------------------------------------------------------------------------------------------------------
class Guarded:
    """n live doubles with GUARD sentinel doubles before and after; .v is the interior (its data pointer is what the library gets)"""

    def __init__(self, gpu, n, fill):
        import torch
        self.full = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float64, device=gpu)
        self.v = self.full[GUARD:GUARD + n]
        if isinstance(fill, np.ndarray):
            self.v.copy_(torch.from_numpy(np.ascontiguousarray(fill, dtype=np.float64)))
        else:
            self.v.fill_(fill)

    def intact(self):
        return bool((self.full[:GUARD] == SENTINEL).all()) and bool((self.full[-GUARD:] == SENTINEL).all())

    def ptr(self):
        """the interior's address, also where the interior is empty (torch reports a null pointer for an empty view)"""
        return ctypes.c_void_p(self.full.data_ptr() + 8 * GUARD)

    def numpy(self):
        return self.v.cpu().numpy()


def _errors(got, ref, stride, size):
    """(error relative to the reference's infinity norm, largest per-element error relative to the element's own largest entry)"""
    d = np.abs(got - ref)
    per = 0.0
    for s, n in zip(stride, size):
        e = d[s:s + n].max() / np.abs(ref[s:s + n]).max()
        per = e if not (e <= per) else per          # a NaN sticks
    return float(d.max() / np.abs(ref).max()), float(per)


def _weights3(quad_type, deg_quad):
    """(w_k (w_a w_b)) at the node a + NQ (b + NQ k) from the library's 1-D weight table, the one a plan uploads: with it w J c is
    held to BIT equality.  (The oracle's Gauss weights are up to 37 ulp away from it at deg_quad = 19 -- tests/test_capi.py holds the
    two tables together at 1e-13 -- so a product of three of them cannot serve a bound of a few ulp.)"""
    from disco4est_amd import table
    w = table("gauss_weights" if quad_type == 0 else "lobatto_weights", deg_quad)
    return (w[:, None, None] * (w[None, :, None] * w[None, None, :])).reshape(-1)


# worst observed error / bound per family and case, printed as the cases run
WORST = {}


def _note(family, label, form, ratio):
    WORST[(family, label, form)] = max(WORST.get((family, label, form), 0.0), ratio)
    print("nonlinear sweep %s %-28s %-5s worst error / bound = %.3f" % (family, label, form, ratio))


class Setup:
    """a mesh with the fields of tests/test_nonlinear_fused_gpu.py::_Case on a plan: SineMap(0.03), a = -(0.5 + uniform),
    b = 0.1 + 0.2 uniform, u = 1 + 0.25 sin(...); a, b, u on the device between sentinel bands"""

    def __init__(self, gpu, oracle, m, faces=False, direct=None):
        from disco4est_amd import Plan, mesh as M
        self.gpu, self.oracle, self.m = gpu, oracle, m
        self.mp = mp = M.SineMap(0.03)
        self.J, self.rst = m.geometry(mp)
        self.plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, m.quad_type)
        if direct is not None:
            self.plan.set_tuning(11, direct)
        self.plan.set_geometry(self.J, self.rst)
        self.sides = None
        if faces:
            self.sides = m.build_sides(mp)
            self.plan.set_faces(self.sides, 10.0, 0)
        nq = m.local_nodes_quad
        self.a = -(0.5 + M.splitmix64_uniform(11, nq))
        self.b = 0.1 + 0.2 * M.splitmix64_uniform(12, nq)
        self.x, self.y, self.z = m.nodal_coords(mp)
        self.ga, self.gb = Guarded(gpu, nq, self.a), Guarded(gpu, nq, self.b)
        self.n3 = (m.deg.astype(np.int64) + 1) ** 3
        self.q3 = (m.deg_quad.astype(np.int64) + 1) ** 3
        self.fields = {}

    def field(self, s):
        """(u, V u by the oracle, u on the device) for the phase s; computed once"""
        if s not in self.fields:
            u = 1.0 + 0.25 * np.sin(1.1 * self.x + 2.0 * self.y + 3.0 * self.z + s)
            self.fields[s] = (u, self.oracle.interpolate(self.m, u), Guarded(self.gpu, self.m.local_nodes, u))
        return self.fields[s]

    def base(self, uq, with_b):
        """b + V u, asserted to stay where (b + u)^-8 is well-conditioned"""
        base = self.b + uq if with_b else uq
        assert base.min() >= 0.5 and base.max() <= 2.0, (base.min(), base.max())
        return base

    def set_power(self, k, with_b):
        self.plan.set_nonlinear_power(self.ga.v, self.gb.v if with_b else None, k)

    def inputs_intact(self):
        import torch
        ok = self.ga.intact() and self.gb.intact() and all(f[2].intact() for f in self.fields.values())
        ok = ok and torch.equal(self.ga.v.cpu(), torch.from_numpy(self.a)) and torch.equal(self.gb.v.cpu(), torch.from_numpy(self.b))
        return ok and all(torch.equal(f[2].v.cpu(), torch.from_numpy(f[0])) for f in self.fields.values())

    def destroy(self):
        self.plan.destroy()


def check_term(S, family, label, fused):
    """the term form against V^T W J a (b + V u)^k for every power, beta = 0 onto NaN and beta = 1 onto a non-zero vector, twice"""
    import torch
    m, plan = S.m, S.plan
    assert plan.nonlinear_fused() == fused, label
    u, uq, gu = S.field(0.3)
    out0 = np.cos(3.0 * S.x - S.y) + 2.0
    worst = 0.0
    for k, with_b in POWERS:
        S.base(uq, with_b)
        ref = S.oracle.apply_galerkin(m, S.J, DN.term(S.a, S.b if with_b else None, uq, k))
        S.set_power(k, with_b)
        for beta in (0, 1):
            want = out0 + ref if beta else ref
            outs = []
            for _ in range(2):
                o = Guarded(S.gpu, m.local_nodes, out0 if beta else float("nan"))
                plan.apply_nonlinear_term(gu.v, o.v, beta)
                torch.cuda.synchronize()
                assert o.intact(), "a sentinel next to out was overwritten (%s k=%d beta=%d)" % (label, k, beta)
                outs.append(o)
            e, pe = _errors(outs[0].numpy(), want, m.nodal_stride, S.n3)
            print("  term %s k=%d b=%s beta=%d: rel-inf %.3e, per element %.3e" % (label, k, with_b, beta, e, pe))
            assert e <= RTOL and pe <= ELEM_RTOL, (label, k, beta, e, pe)
            assert torch.equal(outs[0].v, outs[1].v), "two runs differ (%s k=%d beta=%d)" % (label, k, beta)
            worst = max(worst, e / RTOL, pe / ELEM_RTOL)
    assert S.inputs_intact(), "an input or a sentinel next to it was modified (%s)" % label
    _note(family, label, "term", worst)


def check_coeff(S, family, label, fused):
    """the coefficient form: c against k a (b + V u0)^(k-1); w J c bit for bit against (w_k (w_a w_b)) (J c) formed in numpy from the c
    just read and the plan's weight table"""
    import torch
    m, plan = S.m, S.plan
    nq = m.local_nodes_quad
    assert plan.nonlinear_fused() == fused, label
    assert plan.lhs_coefficient_arrays() is None                 # nothing is set yet
    # the plan's c starts as NaN: an element that no launch covers shows
    plan.set_lhs_coefficient(Guarded(S.gpu, nq, float("nan")).v)
    torch.cuda.synchronize()
    c_nan, w_none = plan.lhs_coefficient_arrays()
    assert bool(torch.isnan(c_nan).all()) and w_none is None     # set_lhs_coefficient leaves w J c to the first apply
    W3 = np.concatenate([_weights3(m.quad_type, int(dq)) for dq in m.deg_quad])
    (u0, uq0, gu0), (u1, uq1, gu1) = S.field(0.0), S.field(1.7)
    worst = 0.0

    def read(gu):
        plan.linearise(gu.v)
        torch.cuda.synchronize()
        arrays = plan.lhs_coefficient_arrays()
        assert arrays is not None and arrays[0].numel() == nq
        if fused:
            assert arrays[1] is not None and arrays[1].numel() == nq
        else:
            assert arrays[1] is None                             # the composed path leaves w J c to the first apply
        return arrays[0].cpu().numpy(), (arrays[1].cpu().numpy() if fused else None)

    for k, with_b in COEFF_POWERS:
        S.set_power(k, with_b)
        bq = S.b if with_b else None
        firsts = []
        for uq, gu in ((uq0, gu0), (uq1, gu1)):
            S.base(uq, with_b)
            c_ref = DN.dterm(S.a, bq, uq, k)
            c, wjc = read(gu)
            e, pe = _errors(c, c_ref, m.quad_stride, S.q3)
            print("  coefficient %s k=%d: c rel-inf %.3e, per element %.3e" % (label, k, e, pe))
            assert e <= RTOL and pe <= ELEM_RTOL, (label, k, e, pe)
            worst = max(worst, e / RTOL, pe / ELEM_RTOL)
            if fused:
                w_ref = W3 * (S.J * c)
                ew = float((np.abs(wjc - w_ref) / np.abs(w_ref)).max())
                print("  coefficient %s k=%d: w J c entrywise %.3e (%.2f ulp; bit equality is required)" % (label, k, ew, ew * 2.0 ** 52))
                assert np.array_equal(wjc, w_ref), (label, k, ew, int((wjc != w_ref).sum()))
            firsts.append(c)
        # the second linearisation replaced the first (no stale array): the two fields differ by O(0.1) in u
        assert np.abs(firsts[1] - firsts[0]).max() > 1e-3 * np.abs(firsts[0]).max(), (label, k)
        plan.set_lhs_coefficient(None)
        assert plan.lhs_coefficient_arrays() is None
        c_again, _ = read(gu0)                                   # ... and linearise brings it back, to the same bits
        assert np.array_equal(c_again, firsts[0]), (label, k)
    # k = 0: both arrays are exactly zero
    S.set_power(0, True)
    c, wjc = read(gu1)
    assert np.array_equal(c, np.zeros(nq)), label
    if fused:
        assert np.array_equal(wjc, np.zeros(nq)), label
    assert S.inputs_intact(), "an input or a sentinel next to it was modified (%s)" % label
    _note(family, label, "coeff", worst)


# ---- (a), (b) every pair ---------------------------------------------------------------------------------------------------------
def _pair_mesh(N, NQ, quad_type=0):
    from disco4est_amd import mesh as M
    count = pair_count(NQ)
    return M.BrickMesh(2 if count > 8 else 1, N - 1, deg_quad_inc=NQ - N, quad_type=quad_type, first=0, count=count)


def test_pair_meshes_end_in_a_ragged_workgroup(hiplib):
    for N, NQ in PAIRS:
        epb, count = elements_per_workgroup(NQ), pair_count(NQ)
        assert (epb < count < 2 * epb) if epb > 1 else count == 3
        m = _pair_mesh(N, NQ)
        assert m.n_elements == count and (m.deg == N - 1).all() and (m.deg_quad == NQ - 1).all()
    assert pair_count(2) == 19 and {elements_per_workgroup(NQ) for _, NQ in PAIRS} == {16, 7, 4, 2, 1}


def _pair_setup(gpu, oracle, pair, cache={}):
    """the two forms of one pair run on the same plan and share the oracle's V u; one pair is kept at a time"""
    if pair not in cache:
        for S in cache.values():
            S.destroy()
        cache.clear()
        cache[pair] = Setup(gpu, oracle, _pair_mesh(*pair))
    return cache[pair]


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%d-%d" % p)
def test_every_pair_term_form(gpu, hiplib, oracle, pair):
    check_term(_pair_setup(gpu, oracle, pair), "a", "(%d,%d) x %d" % (pair + (pair_count(pair[1]),)), True)


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%d-%d" % p)
def test_every_pair_coefficient_form(gpu, hiplib, oracle, pair):
    check_coeff(_pair_setup(gpu, oracle, pair), "b", "(%d,%d) x %d" % (pair + (pair_count(pair[1]),)), True)


# ---- (c) the dispatcher ----------------------------------------------------------------------------------------------------------
# (name, level, degrees, deg_quad_inc, fused)
DISPATCH = [
    # N = 3, 6, 8 in the one multi launch; N = 9 and N = 10 in launches of their own
    ("multi-3-buckets+9+10", 1, [2, 9, 5, 8, 7, 2, 8, 5], 0, True),
    # one equal-order bucket N <= 8: no multi launch, the bucket must still get its own
    ("one-low-bucket+10", 1, [7, 9, 9, 7, 7, 9, 7, 7], 0, True),
    # (2,3), (3,4), (4,5): nothing qualifies for the multi kernel, three single launches
    ("over-integrated-mixed", 1, [1, 2, 3, 3, 2, 1, 2, 3], 1, True),
    # (5,6) has no pair: the whole plan composes
    ("one-bucket-without-pair", 1, [1, 2, 3, 4, 4, 3, 2, 1], 1, False),
    ("uniform-9-10-composed", 0, 8, 1, False),
    ("uniform-20-21-composed", 0, 19, 1, False),
    # N = 2 .. 8: NonlinMulti::MAXB buckets
    ("multi-7-buckets", 1, [1, 2, 3, 4, 5, 6, 7, 4], 0, True),
]


@pytest.mark.parametrize("name,level,deg,inc,fused", DISPATCH, ids=[d[0] for d in DISPATCH])
def test_dispatcher_branches(gpu, hiplib, oracle, name, level, deg, inc, fused):
    from disco4est_amd import mesh as M
    m = M.BrickMesh(level, np.array(deg, np.int32) if isinstance(deg, list) else deg, deg_quad_inc=inc)
    S = Setup(gpu, oracle, m)
    check_term(S, "c", name, fused)
    check_coeff(S, "c", name, fused)
    S.destroy()


# ---- (d) plan settings -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [(4, 4), (8, 8), (3, 4), (10, 10)], ids=lambda p: "%d-%d" % p)
def test_lobatto_quadrature(gpu, hiplib, oracle, pair):
    m = _pair_mesh(pair[0], pair[1], quad_type=1)
    assert m.quad_type == 1
    S = Setup(gpu, oracle, m)
    check_term(S, "d", "lobatto (%d,%d)" % pair, True)
    check_coeff(S, "d", "lobatto (%d,%d)" % pair, True)
    S.destroy()


def test_hanging_mesh(gpu, hiplib, oracle):
    """one refined octant: J differs by a factor of eight between neighbours, so a wrong quad offset shows in the size of the result"""
    from disco4est_amd import mesh as M
    refine = np.zeros(8, bool)
    refine[3] = True
    deg = 2 + (np.arange(15) * 2) % 3                            # p = 2 .. 4 on both element sizes
    m = M.HangingBrickMesh(1, refine, deg.astype(np.int32))
    S = Setup(gpu, oracle, m)
    Je = np.array([S.J[s:s + n].mean() for s, n in zip(m.quad_stride, S.q3)])
    big, small = Je[m.size == 2], Je[m.size == 1]
    assert big.size == 7 and small.size == 8 and big.min() > 4.0 * small.max() and 6.0 < big.mean() / small.mean() < 10.0
    assert set(m.deg[m.size == 2].tolist()) == {2, 3, 4} and set(m.deg[m.size == 1].tolist()) == {2, 3, 4}
    check_term(S, "d", "hanging p=2..4", True)
    check_coeff(S, "d", "hanging p=2..4", True)
    S.destroy()


def test_partition(gpu, hiplib, oracle):
    """the shard first = 2, count = 5 of a level-1 brick at p = 3: one full workgroup of four elements and one with a single element"""
    from disco4est_amd import mesh as M
    m = M.BrickMesh(1, 3, first=2, count=5)
    assert m.n_elements == 5 and m.ijk[0].tolist() == [0, 1, 0]
    S = Setup(gpu, oracle, m)
    check_term(S, "d", "partition 2+5 p=3", True)
    check_coeff(S, "d", "partition 2+5 p=3", True)
    S.destroy()


def test_empty_plan(gpu, hiplib):
    """no elements: both entries return without a launch and without touching anything.  The vectors are the (empty) interiors of
    guarded tensors, handed over by address"""
    import torch
    from disco4est_amd import Plan
    plan = Plan([], [], [], [], 0)
    assert plan.local_nodes == 0 and plan.local_nodes_quad == 0
    plan.set_geometry(np.zeros(0), np.zeros(0))
    ga, gb, gu, go = (Guarded(gpu, 0, 0.0) for _ in range(4))
    lib, h = plan.lib, plan.handle
    lib.d4est_hip_plan_set_nonlinear_power(h, ga.ptr(), gb.ptr(), -7)
    assert plan.nonlinear_fused()
    for beta in (0, 1):
        lib.d4est_hip_apply_nonlinear_term(h, gu.ptr(), beta, go.ptr())
    assert plan.lhs_coefficient_arrays() is None
    lib.d4est_hip_plan_linearise(h, gu.ptr())
    torch.cuda.synchronize()
    c, wjc = plan.lhs_coefficient_arrays()
    assert c.numel() == 0 and wjc is None
    assert all(g.intact() and g.full.numel() == 2 * GUARD for g in (ga, gb, gu, go))
    plan.set_lhs_coefficient(None)
    assert plan.lhs_coefficient_arrays() is None
    plan.destroy()


# ---- (e) the zeroth-order term of apply_lhs on its own scale -----------------------------------------------------------------------
@pytest.mark.parametrize("direct", [0, 2])
@pytest.mark.parametrize("deg", [3, 7])
def test_lhs_term_on_its_own_scale(gpu, hiplib, oracle, deg, direct):
    """apply_lhs(v) - apply_aij(v) after linearise(u0), both on the device, against the oracle's V^T W J c V v, relative to THAT term.
    The difference of two device results carries the Laplacian's rounding, RTOL |lap|, so the bound is RTOL max(1, |lap| / |wm|) with
    both norms from the oracle (tuning key 11: 0 = separate kernels reading c, 2 = the whole-operator kernel reading w J c)"""
    import torch
    from disco4est_amd import mesh as M
    m = M.BrickMesh(1, deg)
    S = Setup(gpu, oracle, m, faces=True, direct=direct)
    plan = S.plan
    k = -7
    S.set_power(k, True)
    v = m.field(S.mp)
    gv = Guarded(gpu, m.local_nodes, v)
    lap_ref = oracle.apply_aij(m, S.J, S.rst, S.sides, v)
    lap = Guarded(gpu, m.local_nodes, float("nan"))
    plan.apply_aij(gv.v, lap.v)
    worst = 0.0
    for s in (0.0, 1.7):
        u0, uq0, gu0 = S.field(s)
        S.base(uq0, True)
        wm_ref = oracle.apply_weighted_mass(m, S.J, DN.dterm(S.a, S.b, uq0, k), v)
        ratio = float(np.abs(lap_ref).max() / np.abs(wm_ref).max())
        bound = RTOL * max(1.0, ratio)
        plan.linearise(gu0.v)
        lhs = Guarded(gpu, m.local_nodes, float("nan"))
        plan.apply_lhs(gv.v, lhs.v)
        torch.cuda.synchronize()
        assert lhs.intact() and lap.intact() and gv.intact()
        got = (lhs.v - lap.v).cpu().numpy()
        e, pe = _errors(got, wm_ref, m.nodal_stride, S.n3)
        print("  lhs term p=%d key11=%d (%s) phase %.1f: |lap|/|wm| = %.3e, bound %.3e, rel-inf error of the term %.3e"
              % (deg, direct, plan.face_path(), s, ratio, bound, e))
        assert e <= bound, (deg, direct, s, e, bound)
        worst = max(worst, e / bound)
    plan.set_lhs_coefficient(None)                               # the term is off: apply_lhs is apply_aij again
    off = Guarded(gpu, m.local_nodes, float("nan"))
    plan.apply_lhs(gv.v, off.v)
    assert _errors(off.numpy(), lap_ref, m.nodal_stride, S.n3)[0] <= RTOL
    assert S.inputs_intact()
    _note("e", "p=%d key11=%d" % (deg, direct), "lhs", worst)
    S.destroy()
