"""The point probes driven from plain C99 (tests/c/probe_probe.c): the C-ABI of include/d4est_hip.h and the reference-named entry point
d4est_mesh_interpolate_at_tree_coord of libd4est_hip_compat.so, whose struct must carry the C-ABI results for three points (one err = 1)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "disco4est_amd")


def _compile(tmp_path):
    exe = str(tmp_path / "probe_probe")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "probe_probe.c"), "-L" + LIBDIR, "-ld4est_hip_compat", "-ld4est_hip",
                           "-lm", "-Wl,-rpath," + LIBDIR, "-o", exe])
    return exe


@pytest.mark.gpu
def test_probe_through_the_c_abi_and_the_shim(gpu, hiplib, tmp_path):
    exe = _compile(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("ok")
