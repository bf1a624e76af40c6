"""The element size parameters driven from plain C99 (tests/c/sizes_probe.c): d4est_hip_plan_set_h_types, the brick mortar form,
d4est_hip_plan_size_parameter and d4est_hip_estimator_bi with a NULL diameter array, through the C-ABI alone."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "disco4est_amd")


def _compile(tmp_path):
    exe = str(tmp_path / "sizes_probe")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "sizes_probe.c"), "-L" + LIBDIR, "-ld4est_hip", "-lm",
                           "-Wl,-rpath," + LIBDIR, "-o", exe])
    return exe


def test_sizes_probe_compiles_as_c99(hiplib, tmp_path):
    assert os.path.exists(_compile(tmp_path))


@pytest.mark.gpu
def test_size_parameters_through_the_c_abi(gpu, hiplib, tmp_path):
    exe = _compile(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("ok")
