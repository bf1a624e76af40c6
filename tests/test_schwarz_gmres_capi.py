"""CPU tests of the subdomain-solver selection's host side: the cross-compiled library exports both entries with the signatures the
header documents, the binding covers them, the new source is in the build list, and the Python wrapper raises on a non-zero code."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {
    "d4est_hip_schwarz_set_subdomain_solver": ("int", ["d4est_hip_schwarz_t*", "int", "int"]),
    "d4est_hip_schwarz_subdomain_solver": ("void", ["const d4est_hip_schwarz_t*", "int*", "int*", "long long*"]),
}
CTYPES = {"int": ctypes.c_int, "void": None, "long long": ctypes.c_longlong}


def _header():
    txt = open(os.path.join(ROOT, "include", "d4est_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_symbols_declared_exported_and_bound(hiplib):
    from disco4est_amd import capi
    txt = _header()
    for name, (ret, args) in SYMBOLS.items():
        m = re.search(r"([a-z ]+?)\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
        assert m, "%s is not declared in include/d4est_hip.h" % name
        assert m.group(1).strip() == ret
        declared = [re.sub(r"\s*\b[a-z_]+$", "", a.strip()).replace(" *", "*") for a in m.group(2).split(",")]
        assert declared == args, (name, declared)
        assert hasattr(hiplib, name), "libd4est_hip.so does not export %s" % name
        restype, argtypes = capi.SIGNATURES[name]
        assert restype is CTYPES[ret]
        assert len(argtypes) == len(args)
        for a, c in zip(args, argtypes):
            assert c is (ctypes.c_void_p if a.endswith("*") else CTYPES[a]), (name, a, c)
    cap = re.search(r"#define\s+D4EST_HIP_SCHWARZ_GMRES_MAX_MR\s+(\d+)", txt)
    assert cap and int(cap.group(1)) >= 125          # the full GMRES of the smallest p = 2, overlap 2 subdomain must be selectable


def test_source_is_in_the_build_list():
    from disco4est_amd import build
    assert "d4est_hip_schwarz_gmres.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "d4est_hip_schwarz_gmres.hip"))


class _StubLib:
    """stands for the library: the setter answers with a fixed code, the query with what was set last"""

    def __init__(self, code):
        self.code, self.calls, self.state = code, [], (0, 0, 0)

    def d4est_hip_schwarz_set_subdomain_solver(self, handle, kind, inner):
        self.calls.append((handle, kind, inner))
        if self.code == 0:
            self.state = (kind, inner if kind == 1 else 0, 1000 * kind)
        return self.code

    def d4est_hip_schwarz_subdomain_solver(self, handle, kind, inner, ws):
        kind._obj.value, inner._obj.value, ws._obj.value = self.state


def _wrapper(code):
    from disco4est_amd.schwarz import Schwarz
    sz = Schwarz.__new__(Schwarz)                    # no device: only the two wrapper methods are exercised
    sz.lib, sz.handle, sz.plan = _StubLib(code), 1234, None
    return sz


@pytest.mark.parametrize("code", [1, 2, 3, 4])
def test_wrapper_raises_with_the_code(code):
    sz = _wrapper(code)
    with pytest.raises(ValueError) as ei:
        sz.set_subdomain_solver(1, 7)
    assert ei.value.args[1] == code and "code %d" % code in ei.value.args[0]
    assert sz.lib.calls == [(1234, 1, 7)]
    sz.handle = None


def test_wrapper_passes_the_choice_through():
    from disco4est_amd.schwarz import SchwarzShard, SchwarzShardNative
    sz = _wrapper(0)
    sz.set_subdomain_solver("gmres", 6)
    assert sz.lib.calls[-1] == (1234, 1, 6) and sz.subdomain_solver() == (1, 6, 1000)
    sz.set_subdomain_solver("cg")
    assert sz.lib.calls[-1] == (1234, 0, 0) and sz.subdomain_solver() == (0, 0, 0)
    for cls in (SchwarzShard, SchwarzShardNative):
        sh = cls.__new__(cls)
        sh.schwarz = sz
        sh.set_subdomain_solver(1, 3)
        assert sz.lib.calls[-1] == (1234, 1, 3)
    sz.handle = None
