"""CPU tests of the hp-AMR entry points' host side: the cross-compiled library exports every d4est_hip_amr_* symbol the header declares,
the binding covers them, and the Amr class is importable."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

AMR_SYMBOLS = ["d4est_hip_amr_create", "d4est_hip_amr_destroy", "d4est_hip_amr_set_stream", "d4est_hip_amr_n_elements",
               "d4est_hip_amr_local_nodes", "d4est_hip_amr_stats", "d4est_hip_amr_mark_smooth_pred", "d4est_hip_amr_p_balance",
               "d4est_hip_amr_get_refinement_log", "d4est_hip_amr_set_refinement_log", "d4est_hip_amr_get_predictor",
               "d4est_hip_amr_set_balance", "d4est_hip_amr_new_n_elements", "d4est_hip_amr_new_local_nodes",
               "d4est_hip_amr_get_new_degrees", "d4est_hip_amr_interpolate_field", "d4est_hip_amr_describe", "d4est_hip_amr_advance"]


def test_amr_symbols_declared_exported_and_bound(hiplib):
    from disco4est_amd import capi
    txt = open(os.path.join(ROOT, "include", "d4est_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = sorted(s for s in set(re.findall(r"\b(d4est_hip_[a-z0-9_]+)\s*\(", txt)) if s.startswith("d4est_hip_amr_"))
    assert declared == sorted(AMR_SYMBOLS)
    for s in AMR_SYMBOLS:
        assert hasattr(hiplib, s), "libd4est_hip.so does not export %s" % s
        assert s in capi.SIGNATURES


def test_amr_class_is_importable():
    import disco4est_amd
    from disco4est_amd import Amr
    assert "Amr" in disco4est_amd.__all__
    for name in ("stats", "mark_smooth_pred", "p_balance", "get_refinement_log", "set_refinement_log", "set_balance", "new_degrees",
                 "interpolate_field", "describe", "advance", "get_predictor", "destroy"):
        assert callable(getattr(Amr, name))


def test_amr_source_is_in_the_build_list():
    from disco4est_amd import build
    assert "d4est_hip_amr.hip" in build.SOURCES
