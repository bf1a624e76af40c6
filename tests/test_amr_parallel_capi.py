"""CPU tests of the multi-rank hp-AMR entry points' host side: the header declares them, the cross-compiled library exports them, the
binding covers them, and the header is still plain C99 with the new hook type."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["d4est_hip_par_amr_set_comm", "d4est_hip_par_amr_stats_global", "d4est_hip_par_amr_repartition", "d4est_hip_par_amr_repartition_field"]

PROBE = r"""
#include "d4est_hip.h"
#include <stdio.h>
static void my_sendrecv(void* ctx, int n_peers, const int* peer_rank, const double* send_dev, const long long* send_first,
                        double* recv_dev, const long long* recv_first) {
  (void)ctx; (void)n_peers; (void)peer_rank; (void)send_dev; (void)send_first; (void)recv_dev; (void)recv_first;
}
static void my_allreduce(void* ctx, double* scalars_dev, int n) { (void)ctx; (void)scalars_dev; (void)n; }
int main(void) {
  d4est_hip_amr_sendrecv_fn s = my_sendrecv;
  d4est_hip_allreduce_fn a = my_allreduce;
  void (*set_comm)(d4est_hip_amr_t*, int, int, d4est_hip_allreduce_fn, d4est_hip_amr_sendrecv_fn, void*) = d4est_hip_par_amr_set_comm;
  void (*stats)(d4est_hip_amr_t*, const double*, int, double*) = d4est_hip_par_amr_stats_global;
  long long (*rep)(d4est_hip_amr_t*, const long long*, const long long*) = d4est_hip_par_amr_repartition;
  void (*field)(d4est_hip_amr_t*, const double*, double*) = d4est_hip_par_amr_repartition_field;
  printf("%d\n", (s != 0) + (a != 0) + (set_comm != 0) + (stats != 0) + (rep != 0) + (field != 0));
  return 0;
}
"""


def test_new_symbols_declared_exported_and_bound(hiplib):
    from disco4est_amd import capi
    txt = open(os.path.join(ROOT, "include", "d4est_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, code), "include/d4est_hip.h does not declare %s" % s
        assert hasattr(hiplib, s), "libd4est_hip.so does not export %s" % s
        assert s in capi.SIGNATURES
    assert "d4est_hip_amr_sendrecv_fn" in code
    # the header says which index each statistics entry uses and that repartition allocates
    assert "keeps the ONE-RANK index" in txt and "d4est_hip_par_amr_repartition may\n * allocate" in txt
    for cite in ("d4est_estimator_stats.c:252-274", ":350-425", ":379, :391", "d4est_amr.c:773-864"):
        assert cite in txt, cite


def test_header_is_c99_with_the_hook_types(tmp_path):
    """a C99 translation unit that takes the address of every new entry through a pointer of the documented type"""
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "probe.o")])


def test_binding_and_plumbing():
    from disco4est_amd import Amr, parallel as P
    for name in ("set_comm", "stats_global", "repartition", "repartition_field"):
        assert callable(getattr(Amr, name))
    assert callable(P.attach_amr)
    assert P.first_of([(0, 3), (3, 0), (3, 4)]).tolist() == [0, 3, 3, 7]
