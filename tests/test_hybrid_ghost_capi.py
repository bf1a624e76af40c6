"""Public-interface side of the hybrid operator on sharded plans (tuning key 14 = 2): no new tuning key, the header still plain C99,
and the key's documentation states the opt-in.  No GPU needed."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "d4est_hip.h")

PROBE = r"""
#include "d4est_hip.h"
#include <stdio.h>
int main(void) {
  printf("%d %d\n", (int)D4EST_HIP_TUNE_HYBRID, (int)D4EST_HIP_TUNE_COUNT);
  return 0;
}
"""


def test_header_is_c99_and_the_tuning_keys_are_unchanged(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = str(tmp_path / "probe")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    key, count = (int(x) for x in subprocess.check_output([exe]).split())
    assert key == 14 and count == 17


def test_key_14_documents_the_opt_in():
    text = open(HEADER).read()
    line = [ln for ln in text.splitlines() if re.search(r"D4EST_HIP_TUNE_HYBRID\s*=\s*14", ln)]
    assert len(line) == 1
    doc = line[0]
    assert "(one rank)" not in doc
    assert re.search(r"\b2: as 1, and also on plans with ghost sides", doc), doc
    assert "D4EST_HIP_HYBRID_NO_GHOST" in doc
    # the face_path form of such plans
    assert "(G beside ghost sides), two-phase on D" in text
