"""The Laplacian at the quadrature nodes driven from plain C99 (tests/c/hessian_probe.c): the C-ABI of include/d4est_hip.h and the
reference-named entry point d4est_hessian_compute_hessian_trace_of_field_on_quadrature_points of libd4est_hip_compat.so."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "disco4est_amd")


def _compile(tmp_path):
    exe = str(tmp_path / "hessian_probe")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "hessian_probe.c"), "-L" + LIBDIR, "-ld4est_hip_compat", "-ld4est_hip",
                           "-lm", "-Wl,-rpath," + LIBDIR, "-o", exe])
    return exe


def test_hessian_probe_compiles_as_c99(hiplib, tmp_path):
    assert os.path.exists(_compile(tmp_path))


@pytest.mark.gpu
def test_hessian_trace_through_the_c_abi_and_the_shim(gpu, hiplib, tmp_path):
    exe = _compile(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("ok")
