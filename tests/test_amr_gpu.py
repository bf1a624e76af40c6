"""GPU tests of the device hp-AMR step (csrc/d4est_hip_amr.hip, disco4est_amd.Amr): estimator statistics, smooth_pred marking, p-balance,
the refinement / balance logs, the fused field transfer and the predictor propagation, against tests/ref_amr.py (pinned by
tests/test_ref_amr.py) and, for the field, two tests/dense_transfer.DenseTransfer.prolong calls in sequence (long double).

All grids are the eight elements of a 2 x 2 x 2 brick in z-order (one 64-element array for the sort).  p4est's part -- which auxiliary
elements the 2:1 balance splits -- is written down by hand in each case: the object only ever sees the logs.

Field tolerance 2e-12 per new element against its own largest entry: the project's 1e-12 transfer tolerance for two composed stages (the
fused kernel rounds once where the reference rounds twice)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import dense_transfer as DT
from tests import ref_amr as R
from tests.test_transfer_sweep_gpu import Guarded

pytestmark = pytest.mark.gpu
FIELD_RTOL = 2e-12
GAMMA_H, GAMMA_P, GAMMA_N = 0.25, 0.1, 0.9
DEG8 = [1, 2, 3, 4, 4, 3, 2, 1]
MAXDEG = 4
INITIAL_PRED = 1.0
MARK_SEED, MARK_FACTOR = 5, 0.5
E2E_SEED, E2E_SIGMA, E2E_PBAL, E2E_IF_DIFF = 6, 0.75, [0, 1, 2, 0, 1, 2, 0, 1], 1


def _uniform(seed, n):
    from disco4est_amd import mesh as M
    return M.splitmix64_uniform(seed, n)


def _dev(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(gpu)


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


# ---- statistics -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 8, 37, 64])
def test_stats(gpu, hiplib, n):
    import torch
    from disco4est_amd import Amr
    eta2 = 3.0 * _uniform(100 + n, n) ** 2
    amr = Amr(np.full(n, 2, np.int32), MAXDEG, INITIAL_PRED)
    d_eta, d_stats = _dev(eta2, gpu), torch.full((4,), float("nan"), dtype=torch.float64, device=gpu)
    for pct in (1, 5, 50, 100, 0):
        ref = R.stats(eta2, pct)
        amr.stats(d_eta, pct, d_stats)
        got = d_stats.cpu().numpy()
        amr.stats(d_eta, pct, d_stats)
        assert (_bits(d_stats.cpu().numpy()) == _bits(got)).all(), "two identical calls differ"
        print("n=%d pct=%d total %.17g (ref %.17g) mean %.17g max %.17g at_pct %.17g" % (n, pct, got[0], ref[0], got[1], got[2], got[3]))
        assert abs(got[0] - ref[0]) <= 1e-13 * abs(ref[0]) and abs(got[1] - ref[1]) <= 1e-13 * abs(ref[1])
        assert _bits(got[2]) == _bits(ref[2]) and _bits(got[3]) == _bits(ref[3])
        if pct == 0:
            assert got[3] == -1.0
    assert (d_eta.cpu().numpy() == eta2).all(), "eta2 was modified"
    amr.destroy()


# ---- marking --------------------------------------------------------------------------------------------------------------------------
def mark_inputs():
    eta2 = 2.0 * _uniform(MARK_SEED, 8)
    thr = R.stats(eta2, 5)[1]
    return eta2, thr, R.mark(eta2, [INITIAL_PRED] * 8, DEG8, MAXDEG, thr, MARK_FACTOR, GAMMA_H, GAMMA_P, GAMMA_N)


def test_mark_inputs_show_every_branch():
    """on the reference alone: the p-branch, the h-branch by eta2 > predictor, the h-branch by deg == max_degree, and unmarked elements"""
    eta2, thr, (log, pred, branch) = mark_inputs()
    kinds = set()
    for e in range(8):
        if branch[e] == "h":
            kinds.add("h-maxdeg" if (eta2[e] <= INITIAL_PRED and DEG8[e] == MAXDEG) else "h-eta" if eta2[e] > INITIAL_PRED else "h?")
        else:
            kinds.add(branch[e])
    assert kinds == {"p", "h-eta", "h-maxdeg", "n"}, (kinds, eta2, thr)
    assert max(log) == MAXDEG        # min(deg + 1, max_degree) at its bound


def test_mark(gpu, hiplib):
    from disco4est_amd import Amr
    eta2, thr, (log, pred, _) = mark_inputs()
    amr = Amr(DEG8, MAXDEG, INITIAL_PRED)
    assert (amr.get_predictor() == INITIAL_PRED).all()
    amr.mark_smooth_pred(_dev(eta2, gpu), _dev([thr], gpu), MARK_FACTOR, GAMMA_H, GAMMA_P, GAMMA_N)
    assert amr.get_refinement_log().tolist() == log
    assert (_bits(amr.get_predictor()) == _bits(pred)).all(), (amr.get_predictor(), pred)
    amr.destroy()


# ---- statistics -> marking -> p-balance -> log ------------------------------------------------------------------------------------------
def e2e_reference():
    eta2 = 2.0 * _uniform(E2E_SEED, 8)
    st = R.stats(eta2, 5)
    log, pred, branch = R.mark(eta2, [INITIAL_PRED] * 8, DEG8, MAXDEG, st[1], E2E_SIGMA, GAMMA_H, GAMMA_P, GAMMA_N)
    log, pred = R.p_balance(log, pred, DEG8, MAXDEG, E2E_PBAL, E2E_IF_DIFF, GAMMA_P)
    return eta2, st, R.clip_log(log, MAXDEG), pred, branch


def test_e2e_inputs_are_away_from_the_threshold():
    """the device mean may differ from the reference's by an ulp (another summation order): no eta2 within 1e-9 relative of sigma * mean"""
    eta2, st, log, _, branch = e2e_reference()
    t = E2E_SIGMA * st[1]
    assert (np.abs(eta2 - t) > 1e-9 * t).all()
    assert {"p", "h", "n"} <= set(branch) and any(l != d and l != -d and l != d + 1 for l, d in zip(log, DEG8)), "p-balance changes nothing"


def test_stats_mark_p_balance_log(gpu, hiplib):
    import torch
    from disco4est_amd import Amr
    eta2, st, log, pred, _ = e2e_reference()
    amr = Amr(DEG8, MAXDEG, INITIAL_PRED)
    d_eta, d_stats = _dev(eta2, gpu), torch.empty(4, dtype=torch.float64, device=gpu)
    amr.stats(d_eta, 5, d_stats)
    amr.mark_smooth_pred(d_eta, d_stats[1:2], E2E_SIGMA, GAMMA_H, GAMMA_P, GAMMA_N)
    amr.p_balance(E2E_PBAL, E2E_IF_DIFF)
    assert amr.get_refinement_log().tolist() == log
    assert (_bits(amr.get_predictor()) == _bits(pred)).all()
    amr.destroy()


# ---- the field transfer -----------------------------------------------------------------------------------------------------------------
def _balance(deg, log, split):
    """the balance log over the auxiliary grid with the auxiliary elements `split` split"""
    aux = R.aux_grid(deg, log)
    return [(-a[0] if i in split else a[0]) for i, a in enumerate(aux)]


def _run_transfer(gpu, deg, log, bal, seed, max_degree=12, x=None):
    """Amr.interpolate_field between guard bands into a NaN-filled vector, twice; returns (result, error against the dense reference,
    describe(), bounds of the new elements)"""
    import torch
    from disco4est_amd import Amr
    s1, s2 = R.transfer_items(deg, log, bal)
    d1, d2 = DT.DenseTransfer(*s1), DT.DenseTransfer(*s2)
    assert d1.fine_nodes == d2.coarse_nodes
    amr = Amr(deg, max_degree, INITIAL_PRED)
    amr.set_refinement_log(log)
    assert amr.get_refinement_log().tolist() == list(log)
    amr.set_balance(bal)
    new = R.new_grid(R.aux_grid(deg, log), bal)
    assert amr.new_n_elements == len(new) and amr.new_degrees().tolist() == [d for d, _, _ in new]
    assert (amr.local_nodes, amr.new_local_nodes) == (d1.coarse_nodes, d2.fine_nodes)
    if x is None:
        x = _uniform(seed, d1.coarse_nodes) - 0.5
    ref = d2.prolong(d1.prolong(x))
    gx = Guarded(gpu, d1.coarse_nodes, x)
    outs = []
    for _ in range(2):
        go = Guarded(gpu, d2.fine_nodes, float("nan"))
        amr.interpolate_field(gx.v, go.v)
        torch.cuda.synchronize()
        assert go.intact() and gx.intact(), "a sentinel next to a live range was overwritten"
        outs.append(go)
    assert torch.equal(outs[0].v, outs[1].v), "two runs differ"
    assert (gx.numpy() == x).all(), "the input was modified"
    desc = amr.describe()
    amr.destroy()
    got = outs[0].numpy()
    return got, DT.elementwise_rel_err(got, ref, d2.fine_bounds), desc, d2.fine_bounds


D7 = [1, 2, 3, 1, 2, 3, 1, 2]
FIELD_CASES = {
    # name: (deg, log, split auxiliary elements)
    "identity": (DEG8, DEG8, []),
    "p+1": (D7, [d + 1 for d in D7], []),
    "p+2": (D7, [d + 2 for d in D7], []),
    "h": (DEG8, [-d for d in DEG8], []),
    "p+1 then balance split": (D7, [d + 1 for d in D7], [0, 3, 6]),
    "h then one child split (64 outputs path)": (DEG8, [-1, 2, 3, 4, 4, 3, 2, 1], [3]),
    "mixed": (DEG8, [2, -2, 3, -4, 4, 4, -3, 3], [0, 4, 10, 11, 19, 20]),
}


@pytest.mark.parametrize("name", sorted(FIELD_CASES))
def test_field_transfer(gpu, hiplib, monkeypatch, name):
    monkeypatch.delenv("D4EST_HIP_TRANSFER_GENERIC", raising=False)
    monkeypatch.delenv("D4EST_HIP_AMR_TWO_STAGE", raising=False)
    deg, log, split = FIELD_CASES[name]
    bal = _balance(deg, log, split)
    assert len(bal) > max(split, default=0)
    got, err, desc, _ = _run_transfer(gpu, deg, log, bal, 500 + len(name))
    print(name, "fused err %.2e" % err, desc)
    assert err <= FIELD_RTOL, (name, err)
    assert desc and all(NH >= 2 for NH, _, _, _ in desc), desc            # degrees <= 7: compile-time instances only
    monkeypatch.setenv("D4EST_HIP_AMR_TWO_STAGE", "1")
    got2, err2, desc2, bounds = _run_transfer(gpu, deg, log, bal, 500 + len(name))
    print(name, "two-stage err %.2e" % err2, desc2)
    assert desc2 == [(-1, 0, 0, len(bal))]
    assert err2 <= FIELD_RTOL
    assert DT.elementwise_rel_err(got, got2, bounds) <= FIELD_RTOL


def test_field_transfer_both_sides_of_the_compile_time_boundary(gpu, hiplib, monkeypatch):
    """p = 7 -> 8 runs the NH = 8 instance, p = 8 -> 9 the runtime-size kernel, in one call; with D4EST_HIP_TRANSFER_GENERIC everything
    runs the runtime-size kernel"""
    monkeypatch.delenv("D4EST_HIP_TRANSFER_GENERIC", raising=False)
    monkeypatch.delenv("D4EST_HIP_AMR_TWO_STAGE", raising=False)
    deg = [7, 7, 8, 8, 7, 8, 7, 8]
    log = [8, -7, 9, -8, 7, 8, 8, 9]
    bal = _balance(deg, log, [0, 3, 10, 12])      # a p-refined 7 -> 8, a child of the split 7, the p-refined 8 -> 9, a child of the split 8
    assert len(bal) == 22
    got, err, desc, bounds = _run_transfer(gpu, deg, log, bal, 77)
    print("7->8 / 8->9 err %.2e" % err, desc)
    assert desc == [(8, 1, 8, 11), (0, 0, 0, 11)]
    assert err <= FIELD_RTOL
    monkeypatch.setenv("D4EST_HIP_TRANSFER_GENERIC", "1")
    got_g, err_g, desc_g, _ = _run_transfer(gpu, deg, log, bal, 77)
    assert desc_g == [(0, 0, 0, 22)] and err_g <= FIELD_RTOL
    assert DT.elementwise_rel_err(got, got_g, bounds) <= FIELD_RTOL


def sweep_case(NH, dmax):
    """eight elements of degree NH - 1 whose new sizes take every value NH .. NH + dmax, with kept -> split, split -> kept and
    split -> split among them: 22 auxiliary elements in one list"""
    dH = NH - 1
    deg = [dH] * 8
    log = [dH + dmax, -(dH + dmax), dH + (dmax + 1) // 2, -dH] + [dH + e % (dmax + 1) for e in range(4, 8)]
    return deg, log, _balance(deg, log, [0, 6, 9, 12, 21])


@pytest.mark.parametrize("NH", range(2, 9))
def test_instance_sweep(gpu, hiplib, monkeypatch, NH):
    """every compile-time instance of the fused kernel (NH = 2 .. 8; DMAX = 0, 1, 3 -- a list with 2 runs the 3) serves its list, as
    describe() shows; together with the runtime-size list of the boundary test these are all the instances the build contains"""
    monkeypatch.delenv("D4EST_HIP_TRANSFER_GENERIC", raising=False)
    monkeypatch.delenv("D4EST_HIP_AMR_TWO_STAGE", raising=False)
    for dmax in range(4):
        deg, log, bal = sweep_case(NH, dmax)
        _, err, desc, _ = _run_transfer(gpu, deg, log, bal, 100 * NH + dmax, max_degree=NH + 3)
        print("NH=%d dmax=%d err %.2e" % (NH, dmax, err))
        assert desc == [(NH, dmax, 8, 22)], desc
        assert err <= FIELD_RTOL, (NH, dmax, err)


def _boxes(log, bal):
    old = [((e & 1) * .5, ((e >> 1) & 1) * .5, ((e >> 2) & 1) * .5, .5) for e in range(8)]

    def kids(b):
        x, y, z, h = b
        return [(x + (c & 1) * h / 2, y + ((c >> 1) & 1) * h / 2, z + ((c >> 2) & 1) * h / 2, h / 2) for c in range(8)]
    aux = []
    for e in range(8):
        aux += kids(old[e]) if log[e] < 0 else [old[e]]
    new = []
    for i in range(len(aux)):
        new += kids(aux[i]) if bal[i] < 0 else [aux[i]]
    return old, new


def _sample(f, boxes, degs):
    out = []
    for (x0, y0, z0, h), d in zip(boxes, degs):
        r = (np.asarray(DT._rule("lobatto", d + 1)[0], dtype=np.float64) + 1.0) * 0.5 * h
        X, Y, Z = x0 + r[None, None, :], y0 + r[None, :, None], z0 + r[:, None, None]      # x fastest
        out.append(np.broadcast_to(f(X, Y, Z), (d + 1,) * 3).ravel())
    return np.concatenate(out)


def test_polynomial_is_reproduced(gpu, hiplib, monkeypatch):
    """a polynomial of degree 3 per variable on degree-3 elements is its own interpolant: the new field is the polynomial at the new nodes
    (kept, p-refined by 1 and 2, h-refined, p-refined then split, h-refined then split)"""
    monkeypatch.delenv("D4EST_HIP_TRANSFER_GENERIC", raising=False)
    monkeypatch.delenv("D4EST_HIP_AMR_TWO_STAGE", raising=False)

    def f(x, y, z):
        return (1 + x + 2 * x ** 2 - x ** 3) * (0.5 - y + y ** 3) * (2 + z ** 2 - 0.7 * z ** 3)
    deg = [3] * 8
    log = [3, 4, 5, -3, 4, -3, 3, -4]
    bal = _balance(deg, log, [1, 5, 14, 20])
    old, new = _boxes(log, bal)
    new_deg = [d for d, _, _ in R.new_grid(R.aux_grid(deg, log), bal)]
    got, err, _, _ = _run_transfer(gpu, deg, log, bal, 0, x=_sample(f, old, deg))
    want = _sample(f, new, new_deg)
    print("polynomial: max abs error %.2e (dense reference %.2e)" % (np.abs(got - want).max(), err))
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


# ---- two consecutive levels ---------------------------------------------------------------------------------------------------------
def test_two_levels(gpu, hiplib):
    from disco4est_amd import Amr
    eta2, thr, (log, pred, _) = mark_inputs()
    log, pred = R.p_balance(log, pred, DEG8, MAXDEG, E2E_PBAL, E2E_IF_DIFF, GAMMA_P)
    log = R.clip_log(log, MAXDEG)
    aux = R.aux_grid(DEG8, log)
    bal = [(-a[0] if i % 5 == 2 else a[0]) for i, a in enumerate(aux)]
    new_deg = [d for d, _, _ in R.new_grid(aux, bal)]
    pred1 = R.advance_predictor(pred, log, bal, GAMMA_H)
    assert any(l < 0 for l in log) and len(new_deg) > len(aux) > 8
    eta2b = 2.0 * _uniform(90, len(new_deg)) * np.array([0.25 ** d for d in new_deg])
    thr2 = R.stats(eta2b, 5)[1]
    log2, pred2, branch2 = R.mark(eta2b, pred1, new_deg, MAXDEG, thr2, 0.5, GAMMA_H, GAMMA_P, GAMMA_N)
    assert {"p", "h", "n"} <= set(branch2)

    amr = Amr(DEG8, MAXDEG, INITIAL_PRED)
    amr.mark_smooth_pred(_dev(eta2, gpu), _dev([thr], gpu), MARK_FACTOR, GAMMA_H, GAMMA_P, GAMMA_N)
    amr.p_balance(E2E_PBAL, E2E_IF_DIFF)
    assert amr.get_refinement_log().tolist() == log
    amr.set_balance(bal)
    assert amr.new_degrees().tolist() == new_deg
    amr.advance()
    assert amr.n_elements == len(new_deg) and amr.local_nodes == sum((d + 1) ** 3 for d in new_deg)
    assert (_bits(amr.get_predictor()) == _bits(pred1)).all()
    amr.mark_smooth_pred(_dev(eta2b, gpu), _dev([thr2], gpu), 0.5, GAMMA_H, GAMMA_P, GAMMA_N)
    assert amr.get_refinement_log().tolist() == log2
    assert (_bits(amr.get_predictor()) == _bits(pred2)).all()
    amr.destroy()


# ---- aborts ---------------------------------------------------------------------------------------------------------------------------
_ABORT_CHILD = r"""
import sys
from disco4est_amd import Amr
mode = sys.argv[1]
amr = Amr([2, 2, 3], 5, 1.0)
if mode == "coarsen":
    amr.set_refinement_log([2, 2, 2])
else:
    amr.set_refinement_log([3, -2, 3])
    amr.set_balance([3] + [2] * 8 if mode == "n_aux" else [3] + [2] * 7 + [-3, 3])
print("NOT REACHED")
"""


@pytest.mark.parametrize("mode, message", [
    ("n_aux", "amr_set_balance: n_aux = 9, but the refinement log makes 10 auxiliary elements"),
    ("degree", "amr_set_balance: balance_log[8] = -3, but auxiliary element 8 has degree 2"),
    ("coarsen", "hp amr code should be >= deg or -deg, coarsening is currently not supported in amr"),
])
def test_argument_errors_abort(gpu, hiplib, mode, message):
    """host-side argument checks ([D4EST_HIP_ABORT], before any launch), seen from a child process"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-c", _ABORT_CHILD, mode], capture_output=True, text=True, timeout=120, cwd=root, env=env)
    assert p.returncode != 0 and "NOT REACHED" not in p.stdout
    assert "[D4EST_HIP_ABORT]" in p.stderr and message in p.stderr, p.stderr
