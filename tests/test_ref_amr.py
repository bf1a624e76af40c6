"""Pins tests/ref_amr.py (the numpy / Python restatement of the reference's hp-AMR bookkeeping) with cases computed by hand.  CPU only."""
import numpy as np
import pytest

from tests import ref_amr as R


@pytest.mark.parametrize("n, expect", [(1, (0, 0, 0, 0)), (7, (6, 6, 3, 0)), (8, (7, 7, 4, 0)), (100, (99, 95, 50, 0))])
def test_percentile_index(n, expect):
    """(int)(n * (1 - percentile / 100)) for percentiles 1, 5, 50, 100: 7 * .99 = 6.93, 7 * .95 = 6.65, 7 * .5 = 3.5; 8 * .99 = 7.92,
    8 * .95 = 7.6; 100 * .99 and 100 * .95 round to 99 and 95 in double arithmetic"""
    assert tuple(R.percentile_index(n, p) for p in (1, 5, 50, 100)) == expect
    assert R.percentile_index(n, 0) == n          # one past the end: the reference's out-of-bounds read


def test_stats_by_hand():
    eta2 = [3.0, 1.0, 2.0, 5.0, 4.0, 0.5, 7.0]    # sorted: .5 1 2 3 4 5 7
    assert R.stats(eta2, 50) == (22.5, 22.5 / 7.0, 7.0, 3.0)
    assert R.stats(eta2, 100)[3] == 0.5 and R.stats(eta2, 1)[3] == 7.0 and R.stats(eta2, 5)[3] == 7.0
    assert R.stats(eta2, 0)[3] == -1.0
    assert R.stats([4.0], 1) == (4.0, 4.0, 4.0, 4.0)
    assert R.stats([], 5) == (0.0, -1.0, -1.0, -1.0)


def test_pow():
    assert [R.dbl_pow_int(.5, b) for b in (0, 1, 2, 5, 8)] == [1.0, 0.5, 0.25, 0.03125, 0.00390625]


def test_mark_branches_by_hand():
    """threshold .25, factor 1, gamma_h .25, gamma_p .125, gamma_n .5, max_degree 4, predictor 1 everywhere:
    e0 deg 2, eta .5: marked, eta <= pred, deg < max     -> log 3,  pred .125 * .5
    e1 deg 2, eta 2.: marked, eta > pred                 -> log -2, pred .25 * 2 * .5^4 * .125 = 2^-8
    e2 deg 4, eta .5: marked, eta <= pred, deg == max    -> log -4, pred .25 * .5 * .5^8 * .125 = 2^-14
    e3 deg 3, eta .125: not marked                       -> log 3,  pred .5 * 1
    e4 deg 3, eta .25: marked (>=), p-branch             -> log 4 = min(deg + 1, max)"""
    log, pred, branch = R.mark([.5, 2., .5, .125, .25], [1.] * 5, [2, 2, 4, 3, 3], 4, .25, 1.0, .25, .125, .5)
    assert log == [3, -2, -4, 3, 4]
    assert pred == [.0625, 2. ** -8, 2. ** -14, .5, .03125]
    assert branch == ["p", "h", "h", "n", "p"]
    # the factor scales the threshold: with factor 4 only eta >= 1 is marked
    assert R.mark([.5, 2.], [1., 1.], [2, 2], 4, .25, 4.0, .25, .125, .5)[0] == [2, -2]


def test_p_balance_by_hand():
    log, pred = R.p_balance([3, -2, 2], [1., 2., 4.], [2, 2, 2], 5, [1, 2, 0], 1, .5)
    assert log == [4, -3, 2] and pred == [.5, 1., 4.]
    # deg < max_degree - 1 fails at max_degree 3: nothing changes
    assert R.p_balance([3, -2, 2], [1., 2., 4.], [2, 2, 2], 3, [1, 2, 0], 1, .5) == ([3, -2, 2], [1., 2., 4.])
    assert R.clip_log([5, -7, 3], 4) == [4, -7, 3]


def test_grids_and_predictor_propagation_by_hand():
    """two elements: e0 (deg 1) h-refined, e1 (deg 2) kept; auxiliary child 2 of e0 and e1 itself are balance-split.
    gamma_h .5: split children of aux 2 get .125 * .5 * .5^2 * 1 = 2^-6, those of e1 .125 * .5 * .5^4 * 2 = 2^-7"""
    deg, log = [1, 2], [-1, 2]
    aux = R.aux_grid(deg, log)
    assert aux == [(1, 0, c) for c in range(8)] + [(2, 1, -1)]
    bal = [1, 1, -1, 1, 1, 1, 1, 1, -2]
    new = R.new_grid(aux, bal)
    assert len(new) == 7 + 8 + 8 and [d for d, _, _ in new] == [1] * 15 + [2] * 8
    assert new[2:10] == [(1, 2, c) for c in range(8)] and new[1] == (1, 1, -1)
    pred = R.advance_predictor([1., 2.], log, bal, .5)
    assert pred == [1., 1.] + [2. ** -6] * 8 + [1.] * 5 + [2. ** -7] * 8
    (h1, dH1, dh1), (h2, dH2, dh2) = R.transfer_items(deg, log, bal)
    assert h1.tolist() == [1, 0] and dH1.tolist() == [1, 2] and dh1.tolist() == [1] * 8 + [2] + [0] * 7
    assert h2.tolist() == [0, 0, 1, 0, 0, 0, 0, 0, 1] and dH2.tolist() == [1] * 8 + [2]
    assert dh2.reshape(-1, 8)[2].tolist() == [1] * 8 and dh2.reshape(-1, 8)[0].tolist() == [1] + [0] * 7
    assert dh2.reshape(-1, 8)[8].tolist() == [2] * 8
