"""pm_rows_packets' three launches without a GPU: rows_packets_core_check.cpp steps them on the host with the rules of csrc/pm_rows_packets.h
-- the walk launch's workgroups, the room launch's trips and carry, the build launch's search and packet -- over the model's blocks, which
this test writes to a file; every entry and every packet row must be the model's (rows_packets_model.py).  The program then feeds every
finished row to the host decoder (pm_codec.cpp is compiled into it) and compares pm_codec_fetch's rows with its own.  Built with the
address and undefined-behaviour sanitizers, as a stand-alone program."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import il2p_packets_model as PM
import rows_packets_model as RP
from conftest import ROOT
from pymodem_amd import _native as N


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("rows_packets_core")
    exe = d / "rows_packets_core_check"
    csrc = os.path.join(ROOT, "pymodem_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                           os.path.join(ROOT, "tests", "rows_packets_core_check.cpp"), os.path.join(csrc, "pm_codec.cpp"), "-lpthread", "-o", str(exe)])
    return str(exe), d


def _write_call(f, row0, cap, capacity, chains, rows, want):
    """chains: [(kind, tol, crc, source, disable_rs, min_dist)]; rows: [(record count, n, part bytes)]; want: (head, entries, packet rows)"""
    f.write(struct.pack("<iiqqq", len(rows), len(chains), row0, capacity, cap))
    for c in chains:
        f.write(struct.pack("<6i", *c))
    for count, n, part in rows:
        f.write(struct.pack("<qqq", count, n, len(part)) + np.ascontiguousarray(part).tobytes())
    head, entries, packets = want
    f.write(head.tobytes() + entries.tobytes() + packets.tobytes())


def _stream_call(f):
    """il2p_packets_model's 49 streams as the rows of one call, a chain a row: every tolerance and option they come with"""
    streams = sorted(PM.all_streams().items())
    chains, rows, model = [], [], []
    for r, (name, (plain, tol, o)) in enumerate(streams):
        n = len(plain)
        steps = ((5 * r + 11 * np.arange(n, dtype=np.int64)) & 0xFFFF)
        addr = 1000 * r + np.cumsum(np.concatenate([[0], steps[1:]])) if n else np.zeros(0, np.int64)
        block, _ = PM.block_of(name)
        chains.append((1, tol, int(o["crc"]), 100 + r, int(o["disable_rs"]), int(o["min_dist"])))
        rows.append((n, n, RP.part_of_row(block, plain, addr, steps)))
        model.append(dict(kind=1, block=block, plain=plain, addr=addr, tol=tol, crc=o["crc"], source=100 + r))
    want = RP.model_call(model, 10 ** 6)
    assert int((want[1]["status"] == RP.FINISHED).sum()) == 40
    _write_call(f, 0, 1 << 16, 10 ** 6, chains, rows, want)


def _rows_call(f, row0, nrows, capacity, bump_last=False):
    import test_gpu_rows_scan as RS
    _, counts, models, plains = RS._rows()
    chains = [(0, 0, 1, 7, 0, 0), (1, RS.TOL, int(RS.OPTS["crc"]), 8, 0, 0), (-1, 0, 0, 9, 0, 0)]
    rows = []
    for row in range(row0, row0 + nrows):
        n = len(plains[row])
        steps = (7 * row + 3 * np.arange(n, dtype=np.int64)) & 0xFFFF
        part = RP.part_of_row(models[row][0], plains[row], RP.row_addresses(row, n), steps) if row % 3 != 2 else np.concatenate(
            [RP.part_of_row(models[row][0], plains[row], [], steps)])
        rows.append((counts[row] + (8 if bump_last and row == row0 + nrows - 1 else 0), n, part))
    left = (row0 + nrows - 1,) if bump_last else ()
    _write_call(f, row0, RS.CAP, capacity, chains, rows, RP.scan_rows_call(row0, nrows, capacity, (7, 8, 9), left))


def test_every_entry_and_packet_is_the_model_s_and_the_host_decoder_s(checker):
    exe, d = checker
    total = int(RP.scan_rows_call(3, 597, 10 ** 9, (7, 8, 9))[0]["packets"][0])
    with open(d / "calls.bin", "wb") as f:
        f.write(struct.pack("<i", 9))
        _stream_call(f)
        _rows_call(f, 3, 597, 10 ** 9)
        _rows_call(f, 3, 597, total - 1)                   # one packet short: the last row with packets and all behind it have no room
        _rows_call(f, 3, 597, 100)
        for nrows in (1, 255, 256, 257):
            _rows_call(f, 9, nrows, 10 ** 9)
        _rows_call(f, 3, 40, 10 ** 9, bump_last=True)      # a record that counts more than the host sized: the scan left the row out
    run = subprocess.run([exe, str(d / "calls.bin")], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    words = run.stdout.strip().split()
    assert words[0] == "9" and words[-2] == "0", run.stdout
    assert int(words[2]) >= 40 + 181 + 175 and int(words[5]) >= 221 + 433, run.stdout
