"""The problem data of the remaining families driven from plain C99 (tests/c/problem_more_probe.c): the new field ids, a new term
setter, the real-power setter and its accessor, build_load and the Lorentzian Robin coefficient through include/d4est_hip.h compiled as
C, their checksums compared with the same calls through the ctypes binding -- exact, an exclusive-or of bit patterns."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "disco4est_amd")
EXT = (1., 2., 1., 2., 1., 2.)


def _checksum(t):
    v = np.ascontiguousarray(t.cpu().numpy()).view(np.uint64)
    with np.errstate(over="ignore"):
        return int(np.bitwise_xor.reduce(v * (2 * np.arange(v.size, dtype=np.uint64) + np.uint64(1))))


@pytest.mark.gpu
def test_new_problem_entries_from_c_match_the_binding(gpu, hiplib, tmp_path):
    import torch
    from disco4est_amd import Plan, capi, mesh as M
    exe = str(tmp_path / "problem_more_probe")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "problem_more_probe.c"), "-L" + LIBDIR, "-ld4est_hip", "-lm",
                           "-Wl,-rpath," + LIBDIR, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
    c = {ln.split()[0]: int(ln.split()[1], 16) for ln in out.stdout.splitlines() if len(ln.split()) == 2}

    m = M.BrickMesh(1, 2)
    tree, q, dq = m.cells()
    plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, 0)
    plan.set_geometry_brick(dq, m.root_len, EXT)
    sides = m.build_sides(geometry=False)
    plan.set_faces(sides, 10.0, 0, brick=(dq, m.root_len, EXT))
    brick = dict(brick=(q, dq, m.root_len, EXT))
    okendon, by, stamm = capi.okendon_params(0.5), capi.boyen_york_params(0.7, 1.3), capi.stamm_params(0.25, 0.3, 0.35)
    params = {6: okendon, 7: by, 8: by, 9: None, 10: None, 11: None, 12: stamm, 13: stamm}
    nq = plan.local_nodes_quad
    got = {}
    xyz = torch.empty(3 * nq, dtype=torch.float64, device=gpu)
    plan.compute_xyz_brick(q, dq, m.root_len, EXT, xyz_quad=xyz)
    o = torch.empty(nq, dtype=torch.float64, device=gpu)
    for fid in range(6, 14):
        capi.field_eval(fid, params[fid], xyz, o)
        got["field_%d" % fid] = _checksum(o)
    u = torch.from_numpy(1.0 + 0.001 * (np.arange(plan.local_nodes) % 17)).to(gpu)
    Au = torch.empty_like(u)
    plan.set_okendon_term(okendon, **brick)
    a, b, k = plan.nonlinear_coefficients()
    assert b is None and k == 0 and plan.nonlinear_exponent() == 0.5
    got["okendon_a"] = _checksum(a)
    plan.apply_nonlinear_term(u, Au)
    got["okendon_term"] = _checksum(Au)
    plan.set_nonlinear_abs_power(u, None, 0.3)                   # (deg_quad = deg: u has local_nodes_quad entries)
    plan.apply_nonlinear_term(u, Au)
    got["abs_power_term"] = _checksum(Au)
    plan.set_boyen_york_term(by, xyz=xyz)
    a, b, k = plan.nonlinear_coefficients()
    assert b is None and k == -7 and plan.nonlinear_exponent() is None
    got["boyen_york_a"] = _checksum(a)
    plan.build_load("STAMM_RHS", stamm, Au, **brick)
    got["load_brick"] = _checksum(Au)
    plan.build_load("LORENTZIAN_RHS", None, Au, beta=1, xyz=xyz)
    got["load_xyz_accumulated"] = _checksum(Au)
    plan.set_robin_by_id("LORENTZIAN", "ZERO", **brick)
    plan.apply_aij(u, Au)
    got["robin_lorentzian"] = _checksum(Au)
    plan.destroy()
    assert sorted(c) == sorted(got)
    bad = [k for k in got if got[k] != c[k]]
    assert not bad, bad
