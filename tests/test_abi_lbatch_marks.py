"""The marks of a sliced engine run (pm_lbatch_marks_*, pm_lbatch_run_sliced_marked in include/pymodem_amd.h): the entry points are exported by
the library, declared in the header as the ctypes mirror (pymodem_amd/_native.py) calls them, and the switch that turns the driver on is one of
the context's."""
import ctypes
import os
import re

from conftest import ROOT

NAMES = ("pm_lbatch_marks_create", "pm_lbatch_marks_destroy", "pm_lbatch_run_sliced_marked", "pm_lbatch_marks_ready", "pm_lbatch_marks_wait",
         "pm_lbatch_marks_wait_on", "pm_lbatch_marks_view")


def _declared(name):
    """the C types of the arguments of `name` as the header declares them, pointers as '*'"""
    with open(os.path.join(ROOT, "include", "pymodem_amd.h")) as f:
        text = f.read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, re.S)
    assert m, name + " is declared in the header"
    out = []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        out.append("*" if "*" in arg else arg.rsplit(" ", 1)[0].replace("const ", ""))
    return out


def test_the_entry_points_are_exported_and_typed_as_declared():
    from pymodem_amd import _native as N
    kinds = {"int64_t": ctypes.c_int64, "int": ctypes.c_int}
    for name in NAMES:
        assert name in N.EXPORTS and hasattr(N.lib(), name), name
        args, res = N._SIGS[name]
        assert res is ctypes.c_int
        declared = _declared(name)
        assert len(declared) == len(args), (name, declared)
        for want, got in zip(declared, args):
            if want == "*":
                assert got is ctypes.c_void_p or issubclass(got, ctypes._Pointer), (name, want, got)
            else:
                assert got is kinds[want], (name, want, got)
    # the marked run is the sliced run's argument list with the marks object and the chunk count behind it
    plain, marked = N._SIGS["pm_lbatch_run_sliced"][0], N._SIGS["pm_lbatch_run_sliced_marked"][0]
    assert marked[:len(plain)] == plain and len(marked) == len(plain) + 2
    assert _declared("pm_lbatch_run_sliced_marked")[:len(plain)] == _declared("pm_lbatch_run_sliced")


def test_the_readers_refuse_a_null_object_without_touching_a_device():
    from pymodem_amd import _native as N
    lib = N.lib()
    t = ctypes.c_int64(7)
    assert lib.pm_lbatch_marks_ready(None, ctypes.byref(t)) == -2
    assert lib.pm_lbatch_marks_wait(None, 0, 200) == -2
    assert lib.pm_lbatch_marks_wait_on(None, 0, None) == -2
    assert lib.pm_lbatch_marks_view(None, 0, None, None, None) == -2
    assert lib.pm_lbatch_marks_create(None, 4, None) == -2
    assert lib.pm_lbatch_marks_destroy(None) == 0


def test_the_switch_is_named_in_the_library_and_the_documents():
    for path in ("pymodem_amd/csrc/pm_common.h", "pymodem_amd/csrc/pm_runtime.hip", "README.md", "INTEGRATION.md", "DESIGN.md"):
        with open(os.path.join(ROOT, path)) as f:
            assert "PM_PIPE_BESIDE" in f.read(), path
