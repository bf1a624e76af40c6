"""GPU sweep over EVERY compiled one-kernel instance of the real-power term a |b + u|^s (d4est_hip_plan_set_nonlinear_abs_power): the 26
(N, NQ) pairs of D4EST_HIP_FAST_PAIRS and D4EST_HIP_BIG_PAIRS in the term form and in the coefficient form, and every branch of the
host dispatcher (the mixed-degree launch, per-bucket launches, the three-call fallback), in the pattern of
tests/test_nonlinear_sweep_gpu.py, whose meshes (one full workgroup followed by a ragged one), sentinel-guarded vectors, per-element
error measure and bounds (RTOL = 1e-12 of the reference's infinity norm, 20 RTOL per element) it shares by import.  No instance that
plan_nonlinear_fused reports as fused is skipped: the pair list is the integer form's, pinned to the macro by
tests/test_nonlinear_dense.py.  The reference is the oracle's interpolate / galerkin integral around tests/dense_problem_more.py."""
import numpy as np
import pytest

from tests import dense_problem_more as DM
from tests.test_nonlinear_sweep_gpu import (DISPATCH, ELEM_RTOL, PAIRS, RTOL, Guarded, Setup, _errors, _pair_mesh, _weights3,
                                            pair_count)

pytestmark = pytest.mark.gpu

# (s, with b): both exponents of tests/test_abs_power_gpu.py, with and without b, each once per form
TERM_CASES = [(0.5, False), (0.3, True)]
COEFF_CASES = [(0.5, True), (0.3, False)]


def _set(S, s, with_b):
    S.plan.set_nonlinear_abs_power(S.ga.v, S.gb.v if with_b else None, s)
    assert S.plan.nonlinear_exponent() == s


def check_term(S, label, fused):
    import torch
    m, plan = S.m, S.plan
    assert plan.nonlinear_fused() == fused, label
    u, uq, gu = S.field(0.3)
    out0 = np.cos(3.0 * S.x - S.y) + 2.0
    for s, with_b in TERM_CASES:
        S.base(uq, with_b)                                       # |b + V u| in [0.5, 2]
        ref = S.oracle.apply_galerkin(m, S.J, DM.abs_term(S.a, S.b if with_b else None, uq, s))
        _set(S, s, with_b)
        for beta in (0, 1):
            want = out0 + ref if beta else ref
            o = Guarded(S.gpu, m.local_nodes, out0 if beta else float("nan"))
            plan.apply_nonlinear_term(gu.v, o.v, beta)
            torch.cuda.synchronize()
            assert o.intact(), "a sentinel next to out was overwritten (%s s=%g beta=%d)" % (label, s, beta)
            e, pe = _errors(o.numpy(), want, m.nodal_stride, S.n3)
            print("  abs term %s s=%g b=%s beta=%d: rel-inf %.3e, per element %.3e" % (label, s, with_b, beta, e, pe))
            assert e <= RTOL and pe <= ELEM_RTOL, (label, s, beta, e, pe)
    assert S.inputs_intact(), label


def check_coeff(S, label, fused):
    """c against s a / pow(t t, (1 - s) / 2); w J c bit for bit against (w_k (w_a w_b)) (J c) from the c just read"""
    import torch
    m, plan = S.m, S.plan
    nq = m.local_nodes_quad
    assert plan.nonlinear_fused() == fused, label
    plan.set_lhs_coefficient(Guarded(S.gpu, nq, float("nan")).v)    # an element that no launch covers shows as NaN
    W3 = np.concatenate([_weights3(m.quad_type, int(dq)) for dq in m.deg_quad])
    u0, uq0, gu0 = S.field(0.0)
    for s, with_b in COEFF_CASES:
        S.base(uq0, with_b)
        _set(S, s, with_b)
        plan.linearise(gu0.v)
        torch.cuda.synchronize()
        c, wjc = plan.lhs_coefficient_arrays()
        c = c.cpu().numpy()
        e, pe = _errors(c, DM.abs_dterm(S.a, S.b if with_b else None, uq0, s), m.quad_stride, S.q3)
        print("  abs coefficient %s s=%g b=%s: rel-inf %.3e, per element %.3e" % (label, s, with_b, e, pe))
        assert e <= RTOL and pe <= ELEM_RTOL, (label, s, e, pe)
        if fused:
            assert wjc is not None and np.array_equal(wjc.cpu().numpy(), W3 * (S.J * c)), (label, s)
        else:
            assert wjc is None                                   # the composed path leaves w J c to the first apply
    plan.set_lhs_coefficient(None)
    assert S.inputs_intact(), label


def _pair_setup(gpu, oracle, pair, cache={}):
    """the two forms of one pair share a plan and the oracle's V u; one pair is kept at a time"""
    if pair not in cache:
        for S in cache.values():
            S.destroy()
        cache.clear()
        cache[pair] = Setup(gpu, oracle, _pair_mesh(*pair))
    return cache[pair]


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%d-%d" % p)
def test_every_pair_term_form(gpu, hiplib, oracle, pair):
    S = _pair_setup(gpu, oracle, pair)
    assert S.m.n_elements == pair_count(pair[1]) >= 2
    check_term(S, "(%d,%d) x %d" % (pair + (S.m.n_elements,)), True)


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%d-%d" % p)
def test_every_pair_coefficient_form(gpu, hiplib, oracle, pair):
    S = _pair_setup(gpu, oracle, pair)
    check_coeff(S, "(%d,%d) x %d" % (pair + (S.m.n_elements,)), True)


@pytest.mark.parametrize("name,level,deg,inc,fused", DISPATCH, ids=[d[0] for d in DISPATCH])
def test_dispatcher_branches(gpu, hiplib, oracle, name, level, deg, inc, fused):
    """the mixed-degree launch next to per-bucket launches, one equal-order bucket, no bucket for the mixed launch, a bucket without a
    pair (the three-call fallback), MAXB buckets: the integer sweep's list"""
    from disco4est_amd import mesh as M
    m = M.BrickMesh(level, np.array(deg, np.int32) if isinstance(deg, list) else deg, deg_quad_inc=inc)
    S = Setup(gpu, oracle, m)
    check_term(S, name, fused)
    check_coeff(S, name, fused)
    S.destroy()
