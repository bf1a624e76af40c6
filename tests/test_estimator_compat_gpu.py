"""The reference-named estimator entry point d4est_estimator_bi_compute (libd4est_hip_compat.so) driven from plain C99
(tests/c/estimator_probe.c) through the reference's prototype, against the device entry point d4est_hip_estimator_bi."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "disco4est_amd")


def _compile(tmp_path):
    exe = str(tmp_path / "estimator_probe")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "estimator_probe.c"), "-L" + LIBDIR, "-ld4est_hip_compat", "-ld4est_hip",
                           "-lm", "-Wl,-rpath," + LIBDIR, "-o", exe])
    return exe


def test_estimator_probe_compiles_as_c99(hiplib, tmp_path):
    assert os.path.exists(_compile(tmp_path))


@pytest.mark.gpu
def test_estimator_bi_compute_through_the_reference_prototype(gpu, hiplib, tmp_path):
    exe = _compile(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("ok")
