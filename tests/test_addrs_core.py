"""The address checkpoints' arithmetic (csrc/pm_bitscan_addrs.h) without a GPU: addrs_core_check.cpp steps the row form on the host -- lane sums,
tile sums, the combine's carry, the in-tile scan, the stores -- for every tile size from 1 to 256 against a plain prefix sum, then the host's
look-up at every byte of every stream.  The program is built with the address and undefined-behaviour sanitizers, as a stand-alone program.
The sizes of the block's new piece are held to the header's in the same place."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import addrs_model as AM
from conftest import ROOT
from pymodem_amd import _native as N

SIZES = [0, 1, 63, 64, 65, 127, 128, 2047, 2048, 2049, 70000]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path_factory.mktemp("addrs_core") / "addrs_core_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "pymodem_amd", "csrc"), os.path.join(ROOT, "tests", "addrs_core_check.cpp"), "-o", str(exe)])
    return str(exe)


def test_the_row_form_and_the_look_up_match_the_prefix_sum(checker):
    run = subprocess.run([checker], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    places = 3 * 256 * sum((n + 63) // 64 for n in SIZES)
    lookups = 3 * sum(SIZES)
    assert run.stdout.strip().splitlines()[-1] == f"{3 * len(SIZES)} streams, {places} places, {lookups} look-ups, 0 mismatches", run.stdout[-3000:]


def test_the_model_is_the_same_prefix_sum():
    rng = np.random.default_rng(4)
    for n in SIZES:
        steps = rng.integers(0, 65536, n, dtype=np.uint16)
        first = (1 << 40) + 3
        A = AM.checkpoints(first, steps)
        assert len(A) == (n + 63) // 64 and A.nbytes == AM.addr_bytes(n) == N.scan_addr_bytes(n)
        a = first
        for k in range(n):
            a += int(steps[k]) if k else 0
            if k % 64 == 0:
                assert int(A[k // 64]) == a
    steps = np.full(70000, 65535, dtype=np.uint16)
    addr = AM.addresses(0, steps)
    # (65 537 steps of 65535 make 2^32 - 1: the step behind them is the first that 32 bits cannot hold, and 70 000 bytes have it)
    assert int(addr[65537]) == (1 << 32) - 1 and int(addr[65538]) >= 1 << 32 and len(addr) > 65538


def test_the_python_side_s_sizes_are_the_header_s():
    assert N.SCAN_ADDR_STRIDE == AM.STRIDE == 64
    for n in (0, 1, 63, 64, 65, 2048, 6144, 70000):
        for kind, frames, packets in ((0, 1, 0), (0, 0, 0), (1, 0, 1), (1, 0, 0), (-1, 0, 0)):
            assert N.scan_part_bytes(kind, frames, packets, n, 1) == N.scan_part_bytes(kind, frames, packets, n) + 8 * ((n + 63) // 64)
            assert N.scan_part_bytes(kind, frames, packets, n, 0) == N.scan_part_bytes(kind, frames, packets, n)
