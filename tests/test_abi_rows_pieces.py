"""The ctypes mirror of pm_rows_carry (pymodem_amd/_native.py) against include/pymodem_amd.h as a C compiler lays it out: 64 bytes, the job
form's carry in front, `taken` and `last_addr` behind it; PM_ROWS_PIECE_TAIL_BYTES; and the two entry points of the rows' pieces."""
import ctypes
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_rows_carry_matches_the_header(tmp_path):
    from pymodem_amd import _native as N
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    fields = [f for f, _ in N.RowsCarry._fields_] + ["scan." + f for f, _ in N.ScanCarry._fields_]
    src = ['#include "pymodem_amd.h"', "#include <stdio.h>", "#include <stddef.h>", "int main(void) {",
           '    printf("sizeof %zu %zu\\n", sizeof(pm_rows_carry), _Alignof(pm_rows_carry));']
    for field in fields:
        src.append(f'    printf("offsetof {field} %zu\\n", offsetof(pm_rows_carry, {field}));')
    src += ['    printf("const %d\\n", PM_ROWS_PIECE_TAIL_BYTES);', "    return 0;", "}"]
    c = tmp_path / "abi.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    seen = 0
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        parts = line.split()
        if parts[0] == "sizeof":
            assert [int(v) for v in parts[1:]] == [ctypes.sizeof(N.RowsCarry), ctypes.alignment(N.RowsCarry)] == [64, 8], line
        elif parts[0] == "offsetof":
            names = parts[1].split(".")
            off = getattr(N.RowsCarry, names[0]).offset + (getattr(N.ScanCarry, names[1]).offset if len(names) > 1 else 0)
            assert off == int(parts[2]), line
        else:
            assert int(parts[1]) == N.ROWS_PIECE_TAIL_BYTES == N.SCAN_CARRY_BYTES + 8
        seen += 1
    assert seen == 1 + len(fields) + 1
    assert N.RowsCarry.scan.offset == 0 and N.RowsCarry.taken.offset == 48 and N.RowsCarry.last_addr.offset == 56
    dt = N.rows_carry_dtype()
    assert dt.itemsize == 64 and dt.fields["taken"][1] == 48 and dt.fields["last_addr"][1] == 56 and dt.fields["scan"][0] == N.scan_carry_dtype()


def test_the_new_entry_points_are_exported_and_declared():
    from pymodem_amd import _native as N
    for name in ("pm_rows_carry_start", "pm_rows_scan_pieces"):
        assert name in N.EXPORTS and hasattr(N.lib(), name)
    for kind, frames, packets, addrs in ((0, 1, 0, 1), (1, 0, 1, 0), (-1, 0, 0, 1)):
        for n in (0, 8, 2048, 2051):
            assert N.rows_piece_part_bytes(kind, frames, packets, n, addrs) == N.rows_scan_steps_bytes(n) + N.scan_part_bytes(kind, frames, packets, n, addrs) + 40
