"""Plain restatement of the reference's hp-AMR bookkeeping in Python floats (IEEE doubles, no fused multiply-add), one loop per loop of
the reference and in its order.  TEST INFRASTRUCTURE: shares no code with the library.  Pinned by tests/test_ref_amr.py.

  estimator statistics   src/Estimators/d4est_estimator_stats.c:219-251 (the mpisize == 1 branch)
  smooth_pred marking    src/hpAMR/d4est_amr_smooth_pred.c:215-268
  p-balance              src/hpAMR/d4est_amr.c:973-981, d4est_amr_smooth_pred.c:132-168
  refine / balance logs  src/hpAMR/d4est_amr.c:160-283
  predictor propagation  src/hpAMR/d4est_amr_smooth_pred.c:73-129
  field interpolation    src/hpAMR/d4est_amr.c:397-482, as two item lists for tests/dense_transfer.DenseTransfer"""
import numpy as np

ONE_OVER_CHILDREN = 0.125          # d4est_amr_smooth_pred.c:17-21, P4EST_DIM == 3
CHILDREN = 8


def percentile_index(n, percentile):
    """d4est_estimator_stats.c:249: (int)(((double)local_size)*(1.-((double)compute_percentile/100.0)))"""
    return int(float(n) * (1. - (float(percentile) / 100.0)))


def stats(eta2, percentile):
    """(total, mean, max, estimator_at_percentile); the total is the caller's running sum in element order (d4est_estimator_stats.c:39-58
    style loops), -1 where the reference's index leaves the array (percentile 0)"""
    eta2 = [float(v) for v in eta2]
    n = len(eta2)
    if n == 0:
        return 0.0, -1.0, -1.0, -1.0                       # :234-238
    total = 0.0
    for v in eta2:
        total += v
    s = sorted(eta2)                                       # :243
    idx = percentile_index(n, percentile)
    return total, total / float(n), s[n - 1], (s[idx] if idx < n else -1.0)   # :245-249


def dbl_pow_int(a, b):
    """d4est_util_dbl_pow_int (src/Utilities/d4est_util.c:157-185), b >= 0"""
    if b == 0:
        return 1.0
    r = dbl_pow_int(a, b // 2)
    r *= r
    if b % 2 != 0:
        r *= a
    return r


def mark(eta2, pred, deg, max_degree, threshold, factor, gamma_h, gamma_p, gamma_n):
    """d4est_amr_smooth_pred.c:240-267 with the marker eta2 >= factor * threshold.  Returns (log, pred, branch); branch per element:
    'p', 'h' or 'n'."""
    log, out, branch = [], [], []
    for e in range(len(deg)):
        eta, eta_pred, d = float(eta2[e]), float(pred[e]), int(deg[e])
        if eta >= factor * threshold:
            if eta <= eta_pred and d < max_degree:
                log.append(min(d + 1, max_degree))
                eta_pred = gamma_p * eta
                branch.append("p")
            else:
                log.append(-d)
                eta_pred = gamma_h * eta * dbl_pow_int(.5, 2 * d) * ONE_OVER_CHILDREN
                branch.append("h")
        else:
            eta_pred = gamma_n * eta_pred
            log.append(d)
            branch.append("n")
        out.append(eta_pred)
    return log, out, branch


def p_balance(log, pred, deg, max_degree, p_bal, p_balance_if_diff, gamma_p):
    """d4est_amr.c:973-981 and d4est_amr_smooth_pred.c:158-163"""
    log, pred = list(log), list(pred)
    for e in range(len(deg)):
        if p_bal[e] >= p_balance_if_diff and deg[e] < max_degree - 1:
            if log[e] < 0:
                log[e] -= 1
            else:
                log[e] += 1
            pred[e] = gamma_p * pred[e]
    return log, pred


def clip_log(log, max_degree):
    """d4est_amr_refine_callback, d4est_amr.c:182-184"""
    return [(max_degree if l > max_degree else l) for l in log]


def aux_grid(deg, log):
    """the refined, unbalanced grid (d4est_amr.c:176-213): per auxiliary element (degree, old element, child position or -1)"""
    out = []
    for e in range(len(deg)):
        if log[e] < 0:
            for c in range(CHILDREN):
                out.append((abs(log[e]), e, c))
        else:
            out.append((log[e], e, -1))
    return out


def new_grid(aux, balance_log):
    """the balanced grid (d4est_amr.c:236-240): per new element (degree, auxiliary element, child position or -1)"""
    assert len(aux) == len(balance_log)
    out = []
    for i, (d, _, _) in enumerate(aux):
        assert abs(balance_log[i]) == d
        if balance_log[i] < 0:
            for c in range(CHILDREN):
                out.append((d, i, c))
        else:
            out.append((d, i, -1))
    return out


def advance_predictor(pred, log, balance_log, gamma_h):
    """d4est_amr_smooth_pred_compute_post_h_balance_predictor, d4est_amr_smooth_pred.c:86-126"""
    aux = []
    for i in range(len(log)):
        for _ in range(CHILDREN if log[i] < 0 else 1):
            aux.append(pred[i])
    out = []
    for i in range(len(balance_log)):
        if balance_log[i] < 0:
            for _ in range(CHILDREN):
                h_pow = abs(balance_log[i])
                out.append(ONE_OVER_CHILDREN * gamma_h * dbl_pow_int(.5, 2 * h_pow) * aux[i])
        else:
            out.append(aux[i])
    return out


def transfer_items(deg, log, balance_log):
    """the two loops of d4est_amr_interpolate_field (d4est_amr.c:412-442, :449-479) as item lists (hrefine, degH, degh[8 k + c]) of
    tests/dense_transfer.DenseTransfer: old -> auxiliary grid, auxiliary -> new grid"""
    n = len(deg)
    h1 = np.array([1 if l < 0 else 0 for l in log], np.int32)
    dh1 = np.zeros((n, 8), np.int32)
    for e in range(n):
        dh1[e, :(8 if log[e] < 0 else 1)] = abs(log[e])     # :352-358
    aux = aux_grid(deg, log)
    m = len(aux)
    h2 = np.array([1 if b < 0 else 0 for b in balance_log], np.int32)
    dH2 = np.array([a[0] for a in aux], np.int32)
    dh2 = np.zeros((m, 8), np.int32)
    for i in range(m):
        dh2[i, :(8 if balance_log[i] < 0 else 1)] = dH2[i]
    return (h1, np.asarray(deg, np.int32), dh1.reshape(-1)), (h2, dH2, dh2.reshape(-1))
