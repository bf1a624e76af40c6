"""The RCCL transport of the Schwarz smoother's whole-element exchanges (d4est_hip_schwarz_set_rccl_exchange), beside
tests/test_rccl_gpu.py::test_two_ranks: it needs two devices and is skipped on one."""
import pytest

pytestmark = pytest.mark.gpu


def test_two_ranks(hiplib):
    """two ranks on two GPUs (skipped on one-GPU boxes): tests/helpers/schwarz_rccl_two_rank_child.py, started as fresh child processes"""
    import os
    import subprocess
    import sys
    import torch
    if torch.cuda.device_count() < 2:          # (counting devices does not initialise the GPU)
        pytest.skip("needs two GPUs; this box has %d" % torch.cuda.device_count())
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29563", os.path.join(root, "tests", "helpers", "schwarz_rccl_two_rank_child.py")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=root)
    print(out.stdout[-4000:], out.stderr[-3000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "two-rank Schwarz RCCL check: ok" in out.stdout
