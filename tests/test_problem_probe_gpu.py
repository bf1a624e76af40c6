"""The problem unit driven from plain C99 (tests/c/problem_probe.c): every new entry of include/d4est_hip.h called once on a 2 x 2 x 2
brick, its checksums compared with the same calls through the ctypes binding -- exact, the checksum is an exclusive-or of bit patterns."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "disco4est_amd")
EXT = (-4., 4., -4., 4., -4., 4.)
SPHERE7 = (1, (3., 6., 0.))


def _checksum(t):
    v = np.ascontiguousarray(t.cpu().numpy()).view(np.uint64)
    with np.errstate(over="ignore"):
        return int(np.bitwise_xor.reduce(v * (2 * np.arange(v.size, dtype=np.uint64) + np.uint64(1))))


@pytest.mark.gpu
def test_problem_entries_from_c_match_the_binding(gpu, hiplib, tmp_path):
    import torch
    from disco4est_amd import Plan, capi, mesh as M
    exe = str(tmp_path / "problem_probe")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "problem_probe.c"), "-L" + LIBDIR, "-ld4est_hip", "-lm",
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
    analytic = dict(analytic=(SPHERE7[0], SPHERE7[1], np.full(8, 6), q, dq, m.root_len))
    punct = capi.puncture_params([[-3., 0., 0.], [3., 0., 0.]], [[0., -.2, 0.], [0., .2, 0.]], [[0.05, 0., 0.1], [0., -0.1, 0.02]], [.5, .5])
    star = (0.25, -0.5, 0.125, 3.0, 0.01, 1.7, 5.0, -0.3)
    nq, tm = plan.local_nodes_quad, int(sides["total_mortar_nodes"])
    got = {}
    xyz = torch.empty(3 * nq, dtype=torch.float64, device=gpu)
    plan.compute_xyz_brick(q, dq, m.root_len, EXT, xyz_quad=xyz)
    got["xyz_brick"] = _checksum(xyz)
    o = torch.empty(nq, dtype=torch.float64, device=gpu)
    for fid in range(6):
        capi.field_eval(fid, punct if fid <= 2 else star, xyz, o)
        got["field_%d" % fid] = _checksum(o)
    for label, setter, params in (("puncture", plan.set_puncture_term, punct), ("cds", plan.set_cds_term, star)):
        for kind, src in (("brick", brick), ("analytic", analytic), ("xyz", dict(xyz=xyz))):
            setter(params, **src)
            a, b, k = plan.nonlinear_coefficients()
            got["%s_%s_a" % (label, kind)] = _checksum(a)
            if b is not None:
                got["%s_%s_b" % (label, kind)] = _checksum(b)
            got["%s_%s_k" % (label, kind)] = k & 0xFFFFFFFFFFFFFFFF
    for kind, src in (("brick", brick), ("analytic", analytic)):
        bx = torch.zeros(3 * tm, dtype=torch.float64, device=gpu)
        plan.compute_boundary_xyz(bx, **src)
        got["boundary_" + kind] = _checksum(bx)
    u = torch.from_numpy(1.0 + 0.001 * (np.arange(plan.local_nodes) % 17)).to(gpu)
    Au = torch.empty_like(u)
    plan.set_robin_by_id("BRICK", "INV_R", **brick)
    plan.apply_aij(u, Au)
    got["robin_brick"] = _checksum(Au)
    plan.set_robin_by_id("INV_R", "ZERO", **analytic)
    plan.apply_aij(u, Au)
    got["robin_analytic"] = _checksum(Au)
    plan.destroy()
    assert sorted(c) == sorted(got)
    bad = [k for k in got if got[k] != c[k]]
    assert not bad, bad
