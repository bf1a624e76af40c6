"""Pins tests/dense_nonlinear.py, the restatement the device power term, its linearisation and the device Newton loop are tested
against (tests/test_nonlinear_fused_gpu.py, tests/test_newton_gpu.py), and the presence of the new entry points."""
import os
import re

import numpy as np

from tests import dense_nonlinear as DN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_power_is_a_product():
    u = np.array([0.5, 1.0, 1.5, 2.0])
    a = np.array([-1.0, 2.0, 0.5, 3.0])
    b = np.array([0.25, 0.0, -0.5, 1.0])
    assert np.array_equal(DN.term(a, b, u, 1), a * (b + u))                     # k = 1 equals a (b + u)
    assert np.array_equal(DN.term(a, None, u, 1), a * u)
    assert np.array_equal(DN.term(a, b, u, 0), a)
    assert np.array_equal(DN.term(a, b, u, 3), a * (((b + u) * (b + u)) * (b + u)))
    assert np.array_equal(DN.term(a, b, u, -2), a * (1.0 / ((b + u) * (b + u))))
    assert np.array_equal(DN.dterm(a, b, u, 0), np.zeros(4))
    assert np.array_equal(DN.dterm(a, b, u, 1), a)
    assert np.allclose(DN.term(a, b, u, -7), a * (b + u) ** -7.0, rtol=1e-14, atol=0)


def test_derivative_agrees_with_a_central_difference():
    rng = np.random.default_rng(3)
    u = 0.5 + rng.random(50)
    a = rng.random(50) - 0.5
    b = 0.5 * rng.random(50)
    eps = 1e-5
    for k in (5, 4, -7, -8, 1, 0, 3):
        fd = (DN.term(a, b, u + eps, k) - DN.term(a, b, u - eps, k)) / (2 * eps)
        d = DN.dterm(a, b, u, k)
        # truncation eps^2 |f'''| / 6: largest for k = -8 at b + u = 0.5, 1e-10 / 6 * 720 * 2^11 / 2 = 1.3e-5 against |d| up to 2e3;
        # roundoff 1e-16 |f| / eps = 1e-11 |f|
        assert np.abs(fd - d).max() <= 1e-6 * max(np.abs(d).max(), 1.0), k


# A x + x^3 = rhs on a 3 x 3 SPD matrix with the solution x* = (1, -1/2, 1/4), Newton with exact linear solves from x = 0.
# |F| by iteration: 4.52, 2.18, 0.240, 4.08e-3, 1.26e-6, 1.2e-13 (quadratic from the third step on)
_A = np.array([[4.0, 1.0, 0.0], [1.0, 3.0, 1.0], [0.0, 1.0, 2.0]])
_XS = np.array([1.0, -0.5, 0.25])
_RHS = _A @ _XS + _XS ** 3
_ONE = np.ones(3)


def _residual(x):
    return _A @ x + DN.term(_ONE, None, x, 3) - _RHS


def _solve(x, minus_f):
    return np.linalg.solve(_A + np.diag(DN.dterm(_ONE, None, x, 3)), minus_f)


def test_newton_loop_counts():
    x0 = np.zeros(3)
    ierr, x, hist = DN.newton(_residual, _solve, x0, 1e-15, 1e-10, 0, 20)
    assert ierr == 0 and len(hist) == 6                        # 1.26e-6 > 1e-10 * 4.52 >= 1.2e-13: five iterations, converged
    assert np.abs(x - _XS).max() < 1e-13
    assert abs(hist[0] - np.linalg.norm(_RHS)) < 1e-15 and abs(hist[1] - 2.1806113940858967) < 1e-12
    # the first step by hand: J(0) = A, x1 = A^-1 rhs
    x1 = np.linalg.solve(_A, _RHS)
    assert abs(hist[1] - np.linalg.norm(_residual(x1))) < 1e-14
    ierr, _, hist = DN.newton(_residual, _solve, x0, 1e-15, 1e-2, 0, 20)
    assert ierr == 0 and len(hist) == 4                        # 0.240 > 1e-2 * 4.52 >= 4.08e-3: three iterations
    ierr, x, hist = DN.newton(_residual, _solve, x0, 1e-15, 1e-10, 0, 0)
    assert ierr == 1 and len(hist) == 1 and np.array_equal(x, x0)          # imax = 0: no iteration, not converged
    ierr, _, hist = DN.newton(_residual, _solve, x0, 1e-15, 1e-10, 0, 2)
    assert ierr == 1 and len(hist) == 3                        # stopped by imax
    # imin forces iterations on a converged guess; without it none runs
    ierr, _, hist = DN.newton(_residual, _solve, _XS, 1e-3, 0.0, 2, 20)
    assert ierr == 0 and len(hist) == 3
    ierr, _, hist = DN.newton(_residual, _solve, _XS, 1e-3, 0.0, 0, 20)
    assert ierr == 0 and len(hist) == 1
    # imax wins over imin
    ierr, _, hist = DN.newton(_residual, _solve, _XS, 1e-3, 0.0, 5, 1)
    assert len(hist) == 2


def _macro_pairs(source, macro):
    """the X(N, NQ) list of `#define macro(X) ...` (continuation lines included) in csrc/<source>"""
    txt = open(os.path.join(ROOT, "disco4est_amd", "csrc", source)).read()
    found = re.findall(r"^#define\s+%s\(X\)((?:[^\n]*\\\n)*[^\n]*)\n" % re.escape(macro), txt, flags=re.M)
    assert len(found) == 1, "%s: %d definitions of %s" % (source, len(found), macro)
    body = found[0].replace("\\\n", " ")
    pairs = [(int(a), int(b)) for a, b in re.findall(r"X\(\s*(\d+)\s*,\s*(\d+)\s*\)", body)]
    assert re.sub(r"X\(\s*\d+\s*,\s*\d+\s*\)", "", body).strip() == "", "%s holds more than X(N, NQ) entries: %r" % (macro, body)
    return pairs


def test_sweep_covers_the_compiled_pairs():
    """tests/test_nonlinear_sweep_gpu.py launches what the fused nonlinear kernels are compiled for, no more and no less: the two pair
    lists of d4est_hip_wave.h, which the nonlinear unit and the Galerkin integral's one-kernel path both walk through for_built_pair (the
    nonlinear unit keeps no list of its own); and every listed pair fits pair_built's LDS limit (WaveCfg::LDS_BYTES = 2 EPB NQ^2 (NQ | 1)
    doubles), so none of them silently composes"""
    from tests.test_nonlinear_sweep_gpu import PAIRS, elements_per_workgroup
    fast = _macro_pairs("d4est_hip_wave.h", "D4EST_HIP_FAST_PAIRS")
    big = _macro_pairs("d4est_hip_wave.h", "D4EST_HIP_BIG_PAIRS")
    assert not set(fast) & set(big) and len(fast + big) == len(set(fast + big))
    nonlin = fast + big
    assert len(nonlin) == len(set(nonlin)) == 26
    assert PAIRS == nonlin
    for unit in ("d4est_hip_nonlinear.hip", "d4est_hip_volume.hip"):
        txt = open(os.path.join(ROOT, "disco4est_amd", "csrc", unit)).read()
        assert "for_built_pair(" in txt and not re.search(r"^#define\s+D4EST_HIP_\w*PAIRS", txt, flags=re.M), unit
    for N, NQ in nonlin:
        assert 2 <= N <= NQ
        assert elements_per_workgroup(NQ) == max(1, 64 // (NQ * NQ))
        lds = 2 * max(1, 64 // (NQ * NQ)) * NQ * NQ * (NQ | 1) * 8
        assert lds <= 160 * 1024, (N, NQ, lds)
    assert 2 * 256 * 17 * 8 == 69632 and 2 * 400 * 21 * 8 == 134400      # (16,16) and (20,20): past 64 KB, the opt-in limit


_SYMBOLS = ["d4est_hip_plan_set_nonlinear_power", "d4est_hip_apply_nonlinear_term", "d4est_hip_plan_linearise", "d4est_hip_build_residual",
            "d4est_hip_newton_solve", "d4est_hip_plan_lhs_coefficient_arrays"]


def test_entry_points_are_declared_and_exported(hiplib):
    txt = open(os.path.join(ROOT, "include", "d4est_hip.h")).read()
    for s in _SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, txt), "include/d4est_hip.h does not declare %s" % s
        assert hasattr(hiplib, s), "libd4est_hip.so does not export %s" % s
