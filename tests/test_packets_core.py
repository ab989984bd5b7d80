"""The per-lane code of bitscan_headers_kernel and bitscan_blocks_kernel (csrc/pm_il2p_core.h) without a GPU: packets_core_check.cpp steps
the two launches' lanes one after the other on the host, and every stream's records and area must be the bit-serial model's
(il2p_packets_model.py); what the blocks launch restates for lanes is held to the shared rs_decode and descramble on random blocks."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import il2p_packets_model as PM
from conftest import ROOT


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("packets_core")
    exe = d / "packets_core_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "pymodem_amd", "csrc"), os.path.join(ROOT, "tests", "packets_core_check.cpp"), "-o", str(exe)])
    return str(exe), d


def test_every_stream_s_records_and_area_are_the_model_s(checker):
    exe, d = checker
    streams = PM.all_streams()
    with open(d / "streams.bin", "wb") as f:
        f.write(struct.pack("<i", len(streams)))
        for name in sorted(streams):
            plain, tol, o = streams[name]
            plain = np.ascontiguousarray(plain)
            n = len(plain)
            block, written = PM.block_of(name)
            _, _, recs, area = PM.split_packets(np.asarray(block), n)
            cands = np.array([k << 3 | S for k, S in PM.candidates(plain, tol)], dtype="<u4")
            f.write(struct.pack("<i", n) + plain.tobytes() + struct.pack("<iiii", o["crc"], o["disable_rs"], o["min_dist"], len(cands)) + cands.tobytes())
            f.write(struct.pack("<i", len(recs)) + recs.tobytes() + area.tobytes() + written[len(written) - len(area):].astype(np.uint8).tobytes())
    run = subprocess.run([exe, "streams", str(d / "streams.bin")], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert run.stdout.strip().endswith(f"{len(streams)} streams, 0 bad")


def test_the_lanes_syndromes_chien_search_and_descrambler_are_the_shared_decoder_s(checker):
    exe, _ = checker
    run = subprocess.run([exe, "random", "20000"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    blocks, corrected, failed, bad = (int(v) for v in run.stdout.strip().split()[0:7:2])
    assert (blocks, bad) == (20000, 0) and corrected > 5000 and failed > 5000, "both outcomes are well covered"
