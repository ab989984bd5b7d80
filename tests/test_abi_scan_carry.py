"""The ctypes mirrors of pm_scan_carry, pm_scan_job and pm_host_job (pymodem_amd/_native.py) against include/pymodem_amd.h as a C compiler
lays them out: sizes and every field's offset, and the constants that go with the carry."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def test_carry_structs_and_constants_match_the_header(tmp_path):
    from pymodem_amd import _native as N
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    structs = {"pm_scan_carry": N.ScanCarry, "pm_scan_job": N.ScanJob, "pm_host_job": N.HostJob}
    src = ['#include "pymodem_amd.h"', "#include <stdio.h>", "#include <stddef.h>", "int main(void) {"]
    for name, cls in structs.items():
        src.append(f'    printf("sizeof {name} %zu\\n", sizeof({name}));')
        for field, _ in cls._fields_:
            src.append(f'    printf("offsetof {name} {field} %zu\\n", offsetof({name}, {field}));')
    src += ['    printf("const %d %d %d %d\\n", PM_SCAN_CARRY_START, PM_SCAN_CARRY_OK, PM_SCAN_CARRY_LOST, PM_SCAN_CARRY_BYTES);', "    return 0;", "}"]
    c = tmp_path / "abi.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    seen = 0
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        parts = line.split()
        if parts[0] == "sizeof":
            assert ctypes.sizeof(structs[parts[1]]) == int(parts[2]), line
        elif parts[0] == "offsetof":
            assert getattr(structs[parts[1]], parts[2]).offset == int(parts[3]), line
        else:
            assert [int(v) for v in parts[1:]] == [N.SCAN_CARRY_START, N.SCAN_CARRY_OK, N.SCAN_CARRY_LOST, N.SCAN_CARRY_BYTES]
        seen += 1
    assert seen == 3 + sum(len(cls._fields_) for cls in structs.values()) + 1
    assert N.ScanJob._fields_[-1][0] == "d_carry" and N.HostJob._fields_[-1][0] == "scan_carry", "appended: what lay in front stays where it was"
    assert N.scan_carry_dtype().itemsize == ctypes.sizeof(N.ScanCarry) and N.scan_carry_piece_dtype().itemsize == N.SCAN_CARRY_BYTES
    for name, (_, off) in N.scan_carry_dtype().fields.items():
        assert getattr(N.ScanCarry, name).offset == off
    assert np.dtype(N.scan_carry_dtype()).names == tuple(f for f, _ in N.ScanCarry._fields_)


def test_the_new_entry_points_are_exported_and_declared():
    from pymodem_amd import _native as N
    for name in ("pm_scan_carry_set", "pm_codec_decode_carried", "pm_codec_scan_state"):
        assert name in N.EXPORTS and hasattr(N.lib(), name)
