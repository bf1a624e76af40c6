"""The reference-named norm entry points of libd4est_hip_compat.so (d4est_mesh_compute_l2_norm_sqr, d4est_norms_fcn_L2 / _Linfty / _energy /
_energy_estimator, d4est_ip_energy_norm_compute, d4est_quadrature_innerproduct, d4est_laplacian_compute_dudr) driven from plain C99
(tests/c/norms_probe.c) through the reference's prototypes, against the device entry points of include/d4est_hip.h and hand values; and
the host-only check of their set-up code (tests/c/norms_compat_host.c: struct mirroring, penalty probing), which needs no device."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "disco4est_amd")


def _compile(tmp_path):
    exe = str(tmp_path / "norms_probe")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "norms_probe.c"), "-L" + LIBDIR, "-ld4est_hip_compat", "-ld4est_hip",
                           "-lm", "-Wl,-rpath," + LIBDIR, "-o", exe])
    return exe


def test_norms_probe_compiles_as_c99(hiplib, tmp_path):
    assert os.path.exists(_compile(tmp_path))


def test_norms_shim_setup_on_the_host(tmp_path):
    """struct layouts and penalty identification: a stand-alone C program, no library, no device"""
    exe = str(tmp_path / "norms_compat_host")
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(LIBDIR, "csrc"), os.path.join(ROOT, "tests", "c", "norms_compat_host.c"), "-lm", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("ok")


@pytest.mark.parametrize("mode, message", [("skip", "Do not use d4est_norms_fcn_energy when skip_element_fcn != NULL"),
                                           ("skip-l2", "d4est_norms_fcn_L2: skip_element_fcn != NULL")])
def test_skip_element_fcn_aborts_before_any_device_work(hiplib, tmp_path, mode, message):
    """d4est_element_data_t is opaque to the library: a skip function cannot be evaluated, and the shim says so (pointing to the mask
    argument of the C-ABI) instead of ignoring it.  The check comes before the bound plan is looked up, so no device is needed."""
    out = subprocess.run([_compile(tmp_path), mode], capture_output=True, text=True, timeout=60)
    assert out.returncode != 0
    assert "returned" not in out.stdout
    assert "[D4EST_HIP_ABORT]" in out.stderr and message in out.stderr, out.stderr


@pytest.mark.gpu
def test_norm_shims_through_the_reference_prototypes(gpu, hiplib, tmp_path):
    exe = _compile(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("ok")
