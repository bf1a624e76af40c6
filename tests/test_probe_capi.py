"""CPU tests of the point probes' host side: the cross-compiled library exports every d4est_hip_probe_* symbol the header declares, the
binding covers them, the compat library exports the reference-named entry point, and the compat header (with the plain-C host that
uses it, tests/c/probe_probe.c) compiles as C99."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "disco4est_amd")

PROBE_SYMBOLS = ["d4est_hip_probe_create", "d4est_hip_probe_destroy", "d4est_hip_probe_n_points", "d4est_hip_probe_info",
                 "d4est_hip_probe_element_info", "d4est_hip_probe_eval", "d4est_hip_probe_set_map", "d4est_hip_probe_eval_gradient",
                 "d4est_hip_probe_xyz"]


def test_probe_symbols_declared_exported_and_bound(hiplib):
    from disco4est_amd import capi
    txt = open(os.path.join(ROOT, "include", "d4est_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = sorted(s for s in set(re.findall(r"\b(d4est_hip_[a-z0-9_]+)\s*\(", txt)) if s.startswith("d4est_hip_probe_"))
    assert declared == sorted(PROBE_SYMBOLS)
    for s in PROBE_SYMBOLS:
        assert hasattr(hiplib, s), "libd4est_hip.so does not export %s" % s
        assert s in capi.SIGNATURES


def test_probe_class_is_importable():
    import disco4est_amd
    from disco4est_amd import Probe
    assert "Probe" in disco4est_amd.__all__
    for name in ("info", "element_info", "eval", "set_map", "eval_gradient", "xyz", "destroy"):
        assert callable(getattr(Probe, name))


def test_probe_source_is_in_the_build_list():
    from disco4est_amd import build
    assert "d4est_hip_probe.hip" in build.SOURCES


def test_compat_library_exports_the_reference_named_entry(hiplib):
    from disco4est_amd import build
    lib = ctypes.CDLL(build.COMPAT_LIB)
    for s in ("d4est_mesh_interpolate_at_tree_coord", "d4est_hip_compat_bind_forest"):
        assert hasattr(lib, s), "libd4est_hip_compat.so does not export %s" % s


def test_compat_header_and_probe_compile_as_c99(hiplib, tmp_path):
    exe = str(tmp_path / "probe_probe")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "probe_probe.c"), "-L" + LIBDIR, "-ld4est_hip_compat", "-ld4est_hip",
                           "-lm", "-Wl,-rpath," + LIBDIR, "-o", exe])
    assert os.path.exists(exe)


def test_mesh_helpers_hand_over_the_element_cells():
    import numpy as np
    from disco4est_amd import mesh as M
    m = M.BrickMesh(1, 2)
    t, q, dq = m.cells()
    assert m.root_len == 2 and t.tolist() == [0] * 8 and dq.tolist() == [1] * 8 and q.tolist() == m.ijk.tolist()
    refine = np.zeros(8, dtype=bool)
    refine[0] = True
    h = M.HangingBrickMesh(1, refine, 1)
    t, q, dq = h.cells()
    assert h.root_len == 4 and len(t) == 15 and dq.tolist() == [1] * 8 + [2] * 7 and q[8].tolist() == [2, 0, 0]
