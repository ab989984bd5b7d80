"""pm_stream_packets' part of the C ABI without a GPU: the symbol exported by the library and declared in the header, the head and the
entry as a C compiler lays them out against the ctypes mirrors and the NumPy views of pymodem_amd/_native.py (32 and 32 bytes), the size
formulas, the record iterator on a hand-made dense form, and the refusal that needs no device."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from pymodem_amd import _native as N


def test_the_symbol_is_exported_and_declared():
    assert "pm_stream_packets" in N.EXPORTS
    assert hasattr(N.lib(), "pm_stream_packets")
    with open(os.path.join(ROOT, "include", "pymodem_amd.h")) as f:
        header = f.read()
    assert "int pm_stream_packets(pm_ctx *ctx, const pm_scan_job *h_jobs, int njobs, const int32_t *h_sources" in header
    assert "pm_packets_pack's wire form" in header, "the header says that the dense form is not the wire form"


def test_layouts_are_the_header_s(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    views = {"pm_stream_packets_head": (N.stream_packets_head_dtype(), N.StreamPacketsHead), "pm_stream_packets_entry": (N.stream_packets_entry_dtype(), N.StreamPacketsEntry)}
    src = ['#include "pymodem_amd.h"', "#include <stdio.h>", "#include <stddef.h>", "int main(void) {"]
    for name, (dt, _) in views.items():
        src.append(f'    printf("sizeof {name} %zu\\n", sizeof({name}));')
        for field in dt.names:
            src.append(f'    printf("offsetof {name} {field} %zu %zu\\n", offsetof({name}, {field}), sizeof((({name} *)0)->{field}));')
    src += ['    printf("head %zu\\n", sizeof(pm_packet_head));', "    return 0;", "}"]
    c = tmp_path / "abi_stream_packets.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "abi_stream_packets"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    seen = 0
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        parts = line.split()
        if parts[0] == "sizeof":
            dt, struct = views[parts[1]]
            assert dt.itemsize == ctypes.sizeof(struct) == int(parts[2]) == 32, line
        elif parts[0] == "offsetof":
            dt, struct = views[parts[1]]
            field, offset = dt.fields[parts[2]]
            mirror = getattr(struct, parts[2])
            assert (offset, field.itemsize) == (mirror.offset, mirror.size) == (int(parts[3]), int(parts[4])), line
        elif parts[0] == "head":
            assert int(parts[1]) == 40 == N.head_dtype().itemsize
        seen += 1
    assert seen == 2 + 5 + 6 + 1
    assert [name for name, _ in N.StreamPacketsHead._fields_] == list(N.stream_packets_head_dtype().names)
    assert [name for name, _ in N.StreamPacketsEntry._fields_] == list(N.stream_packets_entry_dtype().names)
    assert (N.STREAM_PACKETS_HEAD_BYTES, N.STREAM_PACKETS_ENTRY_BYTES) == (32, 32)
    assert N.stream_packets_bytes(64) == 32 + 32 * 64 and N.stream_packets_bytes(3, 96) == 32 + 96 + 96
    assert [N.stream_packets_record_bytes(n) for n in (0, 1, 8, 9, 18, 1280, 1281, 5000)] == [40, 48, 48, 56, 64, 1320, 1320, 1320]


def test_the_record_iterator():
    """two jobs by hand: records of 18 and 3 bytes for job 0, none for job 1 (NO_ROOM at the total)"""
    raw = np.zeros(N.stream_packets_bytes(2, 64 + 48), dtype=np.uint8)
    head = raw[:32].view(N.stream_packets_head_dtype())
    entries = raw[32:96].view(N.stream_packets_entry_dtype())
    head["jobs"], head["handed"], head["packets"], head["bytes"] = 2, 1, 2, 112
    entries[0] = (5, 0, 2, 0, 0, 0)
    entries[1] = (6, N.ROWS_PACKETS_STATUS.index("NO_ROOM"), 0, 112, 0, 0)
    for at, length, addr in ((96, 18, 1 << 40), (96 + 64, 3, -7)):
        h = raw[at:at + 40].view(N.head_dtype())
        h["streamaddress"], h["len"] = addr, length
        raw[at + 40:at + 40 + length] = np.arange(length) + 1
    got = [(j, int(h["streamaddress"]), bytes(d)) for j, h, d in N.stream_packets_records(raw, 2)]
    assert got == [(0, 1 << 40, bytes(range(1, 19))), (0, -7, bytes([1, 2, 3]))]


def test_a_call_without_a_context_is_refused():
    lib = N.lib()
    used = ctypes.c_size_t(77)
    assert lib.pm_stream_packets(None, None, 1, None, None, None, None, 0, ctypes.byref(used)) == -2      # PM_ERR_ARG
    buf = ctypes.create_string_buffer(256)
    lib.pm_last_error(buf, 256)
    assert b"bad argument" in buf.value and used.value == 77
