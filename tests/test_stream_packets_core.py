"""pm_stream_packets' three launches without a GPU: stream_packets_core_check.cpp steps them on the host with the rules of
csrc/pm_rows_packets.h -- the walk launch's wave with its trips of 64 events, ballot and prefix sum, the room launch's scan, the build
launch's search and record -- over the model's blocks, which this test writes to a file; every entry and every record must be the model's
(stream_packets_model.py), and the wave walk's accepted list pm_rpk::ax25_walk's.  The program then feeds every finished stream to the host
decoder (pm_codec.cpp is compiled into it) and compares pm_codec_fetch's packets with its own records.  Built with the address and
undefined-behaviour sanitizers, as a stand-alone program."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import frames_model as FM
import rows_packets_model as RP
import stream_packets_model as SP
from conftest import ROOT
from pymodem_amd import _native as N


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("stream_packets_core")
    exe = d / "stream_packets_core_check"
    csrc = os.path.join(ROOT, "pymodem_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                           os.path.join(ROOT, "tests", "stream_packets_core_check.cpp"), os.path.join(csrc, "pm_codec.cpp"), "-lpthread", "-o", str(exe)])
    return str(exe), d


def _write_call(f, jobs, room, want):
    f.write(struct.pack("<iq", len(jobs), room))
    for j in jobs:
        part = np.ascontiguousarray(j["block"]) if j["block"] is not None else np.zeros(N.scan_part_bytes(-1, 0, 0, len(j["plain"])), dtype=np.uint8)
        f.write(struct.pack("<6iqq", j["kind"], j["tol"], int(j["crc"]), j["source"], int(j.get("disable_rs", False)), int(j.get("min_dist", 0)), len(j["plain"]),
                            len(part)))
        f.write(part.tobytes() + np.ascontiguousarray(j["addr"], dtype="<i8").tobytes())
    head, entries, records = want
    f.write(head.tobytes() + entries.tobytes() + records.tobytes())


def _long_frame_call(f):
    """events65 with the table entry of its last event -- the second trip's only one -- saying more bytes than lie between its flags: the
    whole job is LONG_FRAME, whatever the first trip listed, and the job behind it is finished as ever"""
    jobs = [dict(SP.events_jobs()[4]), SP.ax25_jobs()[1]]
    assert jobs[0]["name"] == "events65"
    n = len(jobs[0]["plain"])
    block = jobs[0]["block"].copy()
    at = N.SCAN_HEAD + N.scan_list_bytes(0, n) + (n + 7) // 8 * 8 + 8 * 64
    assert 18 <= int(block[at:at + 4].view("<i4")[0]) <= 40
    block[at:at + 4] = np.array([41], dtype="<i4").view(np.uint8)
    jobs[0]["block"] = block
    head, entries, records = SP.model_call(jobs[1:], 10 ** 6)
    e = np.zeros(2, dtype=entries.dtype)
    e[0] = (0, RP.LONG_FRAME, 0, 0, 0, 0)
    e[1] = entries[0]
    head["jobs"], head["handed"] = 2, 1
    _write_call(f, jobs, 10 ** 6, (head, e, records))


def test_every_entry_and_record_is_the_model_s_and_the_host_decoder_s(checker):
    exe, d = checker
    il2p, il2p_walks = SP.il2p_jobs(), SP.il2p_walks()
    ax25, ax25_walks = SP.ax25_jobs() + SP.events_jobs(), SP.ax25_walks() + SP.events_walks()
    none = SP.job(-1, FM.all_streams()["shared_zero"], source=9)
    mix, mix_walks = [], []
    for k in range(64):                                     # 64 jobs of mixed kinds
        src, walks = ((il2p, il2p_walks), (ax25, ax25_walks))[k % 2]
        if k % 7 == 3:
            mix.append(none)
            mix_walks.append((RP.NO_CODEC, [], 0))
        else:
            mix.append(src[(5 * k) % len(src)])
            mix_walks.append(walks[(5 * k) % len(src)])
    total = int(SP.model_call(ax25, 10 ** 9, ax25_walks)[0]["bytes"][0])
    calls = [(il2p, 10 ** 9, il2p_walks), (ax25, 10 ** 9, ax25_walks), (ax25, total, ax25_walks), (ax25, total - 8, ax25_walks), (ax25, total - 1, ax25_walks),
             (ax25, 1000, ax25_walks), (ax25, 0, ax25_walks), (mix, 10 ** 9, mix_walks), (mix, 20000, mix_walks), (ax25[-1:], 10 ** 9, ax25_walks[-1:]),
             ([none], 64, [(RP.NO_CODEC, [], 0)])]
    with open(d / "calls.bin", "wb") as f:
        f.write(struct.pack("<i", len(calls) + 1))
        for jobs, room, walks in calls:
            _write_call(f, jobs, room, SP.model_call(jobs, room, walks))
        _long_frame_call(f)
    run = subprocess.run([exe, str(d / "calls.bin")], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    words = run.stdout.strip().split()
    assert words[0] == str(len(calls) + 1) and words[-2] == "0", run.stdout
    assert int(words[2]) >= 40 + 2 * 17 and int(words[5]) >= 60 + 2 * 300, run.stdout
