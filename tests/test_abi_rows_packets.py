"""pm_rows_packets' part of the C ABI without a GPU: the head and the entry as a C compiler lays them out against the NumPy views of
pymodem_amd/_native.py, the status numbers against their names, the size formula, and the refusal that needs no device."""
import ctypes
import os
import shutil
import subprocess

import pytest

from conftest import ROOT
from pymodem_amd import _native as N


def test_layouts_and_status_numbers_are_the_header_s(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    views = {"pm_rows_packets_head": N.rows_packets_head_dtype(), "pm_rows_packets_entry": N.rows_packets_entry_dtype()}
    src = ['#include "pymodem_amd.h"', "#include <stdio.h>", "#include <stddef.h>", "int main(void) {"]
    for name, dt in views.items():
        src.append(f'    printf("sizeof {name} %zu\\n", sizeof({name}));')
        for field in dt.names:
            src.append(f'    printf("offsetof {name} {field} %zu %zu\\n", offsetof({name}, {field}), sizeof((({name} *)0)->{field}));')
    for name in N.ROWS_PACKETS_STATUS:
        src.append(f'    printf("status {name} %d\\n", PM_ROWS_PACKETS_{name});')
    src += ['    printf("packet %zu\\n", sizeof(pm_packet));', "    return 0;", "}"]
    c = tmp_path / "abi_rows_packets.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "abi_rows_packets"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    seen = 0
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        parts = line.split()
        if parts[0] == "sizeof":
            assert views[parts[1]].itemsize == int(parts[2]), line
        elif parts[0] == "offsetof":
            dt, offset = views[parts[1]].fields[parts[2]]
            assert (offset, dt.itemsize) == (int(parts[3]), int(parts[4])), line
        elif parts[0] == "status":
            assert N.ROWS_PACKETS_STATUS.index(parts[1]) == int(parts[2]), line
        elif parts[0] == "packet":
            assert int(parts[1]) == ctypes.sizeof(N.Packet) and int(parts[1]) % 8 == 0
        seen += 1
    assert seen == 2 + 3 + 6 + len(N.ROWS_PACKETS_STATUS) + 1
    assert (N.ROWS_PACKETS_HEAD_BYTES, N.ROWS_PACKETS_ENTRY_BYTES) == (views["pm_rows_packets_head"].itemsize, views["pm_rows_packets_entry"].itemsize)
    assert N.rows_packets_bytes(597) == 16 + 32 * 597 and N.rows_packets_bytes(3, 2) == 16 + 96 + 2 * 1320
    assert N.ROWS_PACKETS_STATUS[0] == "FINISHED", "status 0 is FINISHED"


def test_a_call_without_a_context_is_refused():
    lib = N.lib()
    used = ctypes.c_size_t(77)
    assert lib.pm_rows_packets(None, None, None, 0, 0, 1, None, 1, None, None, None, None, None, 0, ctypes.byref(used)) == -2      # PM_ERR_ARG
    buf = ctypes.create_string_buffer(256)
    lib.pm_last_error(buf, 256)
    assert b"bad argument" in buf.value and used.value == 77
