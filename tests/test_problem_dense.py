"""CPU pins of tests/dense_problem.py, the numpy restatement the GPU tests of csrc/d4est_hip_problem.hip compare against, and the host
side of the new entries: exported, declared, bound, and usable from plain C99 (tests/c/problem_probe.c)."""
import os
import re
import subprocess

import numpy as np

from tests import dense_problem as DP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "disco4est_amd")

SYMBOLS = ["d4est_hip_field_eval", "d4est_hip_plan_compute_xyz_brick", "d4est_hip_plan_set_puncture_term_brick",
           "d4est_hip_plan_set_puncture_term_analytic", "d4est_hip_plan_set_puncture_term_xyz", "d4est_hip_plan_set_cds_term_brick",
           "d4est_hip_plan_set_cds_term_analytic", "d4est_hip_plan_set_cds_term_xyz", "d4est_hip_plan_nonlinear_coefficients",
           "d4est_hip_plan_compute_boundary_xyz_brick", "d4est_hip_plan_compute_boundary_xyz_analytic",
           "d4est_hip_plan_set_robin_by_id_brick", "d4est_hip_plan_set_robin_by_id_analytic"]


def _params(C, P, S, M=1.0):
    return np.concatenate([[1.0, 1e-15], C, P, S, [M]])


def _pts():
    return np.random.default_rng(0).uniform(-3, 3, (3, 200))


def test_k2_of_one_puncture_without_spin_is_the_closed_form():
    """S = 0: K2 = (9/2) (P^2 + 2 (P.n)^2) / r^4, within the restatement's own bound"""
    C, P = np.array([0.5, 0.2, -0.1]), np.array([0.1, -0.2, 0.3])
    X = _pts()
    d = X - C[:, None]
    r = np.sqrt((d * d).sum(axis=0))
    n = d / r
    k2, bound = DP.k2_with_bound(X[0], X[1], X[2], _params(C, P, np.zeros(3)))
    closed = 4.5 * ((P * P).sum() + 2 * (P @ n) ** 2) / r ** 4
    assert np.all(np.abs(k2 - closed) <= bound) and np.all(bound <= 1e-12 * closed)


def test_k2_of_one_puncture_without_momentum_is_the_closed_form():
    """P = 0: K2 = 18 |S x n|^2 / r^6"""
    C, S = np.array([0.5, 0.2, -0.1]), np.array([0.1, 0.0, 0.2])
    X = _pts()
    d = X - C[:, None]
    r = np.sqrt((d * d).sum(axis=0))
    n = d / r
    k2, bound = DP.k2_with_bound(X[0], X[1], X[2], _params(C, np.zeros(3), S))
    closed = 18 * (np.cross(S, n.T) ** 2).sum(axis=1) / r ** 6
    assert np.all(np.abs(k2 - closed) <= bound)


def test_eps_rules_of_the_power_callbacks():
    """on a puncture compute_confAij moves r to eps (finite K2); the callbacks' test reads the LAST puncture's r only"""
    two = np.concatenate([[2.0, 1e-15], [-3, 0, 0], [0, -.2, 0], [0, 0, .1], [.5], [3, 0, 0], [0, .2, 0], [0, 0, 0], [.5]])
    X = np.array([[-3., 3., 1.], [0., 0., 2.], [0., 0., 0.5]])
    k2 = DP.conf_aij_sqr(X[0], X[1], X[2], two)
    a, b = DP.puncture_a(X[0], X[1], X[2], two), DP.puncture_b(X[0], X[1], X[2], two)
    assert np.all(np.isfinite(k2))
    assert np.isfinite(a[0]) and a[0] != 0 and b[0] == np.inf            # on puncture 0: the test passes on the last puncture's r
    assert a[1] == 0.0 and b[1] == np.inf                                # on the last puncture
    f = DP.neg_1o8_k2_psi_neg7(X[0], X[1], X[2], np.zeros(3), two)
    assert f[0] == 0.0 and f[1] == 0.0 and f[2] < 0                      # a / inf^7 = 0, not NaN
    # pow(psi0 psi0, 3.5) against the product of seven factors: the last bits only
    psi = b[2]
    assert abs(f[2] - a[2] / psi ** 7) <= 16 * 2.0 ** -53 * abs(f[2])


def test_cds_psi_is_continuous_at_the_surface():
    """parameters with C0 u_alpha(R) = 1 + beta / R, as constant_density_star_input sets them (:225-226)"""
    R, alpha, C0 = 3.0, 5.0, 1.7
    beta = R * (C0 * np.sqrt(alpha * R) / np.sqrt(R * R + alpha * R * alpha * R) - 1.)
    p = (0.25, -0.5, 0.125, R, 0.01, C0, alpha, beta)
    for s in (1 - 1e-12, 1 + 1e-12):
        x = np.array([p[0] + s * R]); y = np.array([p[1]]); z = np.array([p[2]])
        assert abs(DP.cds_psi(x, y, z, p)[0] - (1. + beta / R)) <= 1e-11
    x = np.array([p[0] + 0.5 * R, p[0] + 2 * R]); y = np.full(2, p[1]); z = np.full(2, p[2])
    assert DP.cds_a(x, y, z, p).tolist() == [-2 * np.pi * 0.01, 0.0]


def test_boundary_restatement_reproduces_the_outer_radius(hiplib):
    from disco4est_amd import forest as F
    mp = F.CubedSphere13Map(1.0, 2.0, 20.0, compactify_outer=True)
    m = F.ForestMesh(F.cubed_sphere_13tree_connectivity(), 0, 3, mp)
    s = m.build_sides_c()
    X = DP.boundary_xyz(m, s)
    bnd = np.isfinite(X[0])
    assert bnd.sum() == 6 * 16 and np.abs((X[:, bnd] ** 2).sum(axis=0) - 400.0).max() <= 400.0 * 1e-13


def test_problem_symbols_declared_exported_and_bound(hiplib):
    from disco4est_amd import capi, Plan
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "d4est_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(d4est_hip_[a-z0-9_]+)\s*\(", txt))
    for s in SYMBOLS:
        assert s in declared and hasattr(hiplib, s) and s in capi.SIGNATURES, s
    for name in ("compute_xyz_brick", "set_puncture_term", "set_cds_term", "nonlinear_coefficients", "compute_boundary_xyz",
                 "set_robin_by_id", "dirichlet_from_field"):
        assert callable(getattr(Plan, name))
    assert callable(capi.field_eval) and capi.FIELD["INV_R"] == 5 and capi.MAX_PUNCTURES == 10


def test_problem_source_is_in_the_build_list():
    from disco4est_amd import build
    assert "d4est_hip_problem.hip" in build.SOURCES


def test_header_and_problem_probe_compile_as_c99(hiplib, tmp_path):
    exe = str(tmp_path / "problem_probe")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "problem_probe.c"), "-L" + LIBDIR, "-ld4est_hip", "-lm",
                           "-Wl,-rpath," + LIBDIR, "-o", exe])
    assert os.path.exists(exe)
