"""The hybrid operator's bucket rule (disco4est_amd/csrc/d4est_hip_hybrid_buckets.h, called by the face set-up in
d4est_hip_faces_setup.hip): which degree buckets keep their clean elements and whether the operator is set up at all.  The header is
plain C++, so the default rule -- 2048 clean elements per bucket, half of the mesh, reachable through a plan only with 4096 or more
elements on a GPU -- is checked here on the CPU: tests/c/hybrid_bucket_rule.cpp is compiled against it with g++ and run once per row."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# clean elements per bucket, elements, tuning key 14, D4EST_HIP_HYBRID_ONE_BUCKET_ONLY set -> set up?, all_buckets, the buckets kept
ROWS = [
    ((600,), 1000, -1, False, True, False, (0,)),
    ((499,), 1000, -1, False, False, False, ()),
    ((0,), 1000, 1, False, False, False, ()),
    ((300, 300), 1000, 1, False, True, False, (0, 1)),             # forced: nobody is demoted
    ((600, 300), 1000, -1, False, True, False, (0,)),              # the dominant bucket
    ((400, 400), 1000, -1, False, False, False, ()),               # no bucket holds half
    ((500, 500), 1000, -1, False, True, False, (0,)),              # a tie: the first largest
    ((2048, 2048, 100), 8000, -1, False, True, True, (0, 1)),      # at size: bucket 2 demoted
    ((2048, 2048, 100), 8400, -1, False, False, False, ()),        # kept sum below half, no dominant bucket
    ((5000, 2048, 100), 20000, -1, False, False, False, ()),
    ((6000, 2048), 10000, -1, True, False, False, ()),             # one_only blocks both demotion rules
    ((6000, 2048), 10000, -1, False, True, True, (0, 1)),
    # beside the rows above: the threshold itself, and the dominant rule where the at-size rule just misses
    ((2047, 2048), 4096, -1, False, True, False, (1,)),            # one bucket below 2048: not the at-size rule, but bucket 1 holds half
    ((2047, 2047), 4096, -1, False, False, False, ()),
    ((0, 700), 1000, -1, False, True, False, (0, 1)),              # one clean bucket: no demotion, an empty bucket is not touched
]


@pytest.fixture(scope="module")
def rule_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hybrid_bucket_rule") / "hybrid_bucket_rule")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "disco4est_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "hybrid_bucket_rule.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("cnt,ne,tuning,one_only,set_up,all_buckets,kept", ROWS)
def test_bucket_rule(rule_exe, cnt, ne, tuning, one_only, set_up, all_buckets, kept):
    args = [rule_exe, str(ne), str(tuning), str(int(one_only))] + [str(c) for c in cnt]
    out =subprocess.run(args, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    flags, _, buckets = out.stdout.strip().partition(":")
    assert flags.split() == [str(int(set_up)), str(int(all_buckets))]
    assert tuple(int(b) for b in buckets.split()) == kept


def test_header_has_no_hip():
    """the rule stays testable without a GPU toolchain: the header includes nothing of HIP and nothing of the plan"""
    text = open(os.path.join(ROOT, "disco4est_amd", "csrc", "d4est_hip_hybrid_buckets.h")).read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes == ["<cstddef>", "<vector>"]
