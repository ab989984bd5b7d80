"""The three AX.25 launches of a stream scanned in pieces without a GPU: scan_carry_core_check.cpp steps them through
csrc/pm_bitscan_events.h lane by lane, for streams cut into two and three pieces, and every piece's record, list and carry must be those of
the bit-serial model (scan_carry_model.py) at the tile sizes 1, 2, 3, 17, 64, 125, 126, 255 and 256.  The program is built with the address
and undefined-behaviour sanitizers, as a stand-alone program."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import bitscan_model as M
import scan_carry_model as CM
import test_host_scan_carry as H
from conftest import ROOT
from pymodem_amd._native import SCAN_CARRY_LOST, scan_record_dtype

TILES = [1, 2, 3, 17, 64, 125, 126, 255, 256]


def streams():
    """(name, descrambled bytes, cuts): the windows of test_host_scan_carry.py cut at every byte around what the carry decides, in two pieces
    and -- with a second cut a few bytes, a word, a tile of 17 words behind -- in three; a piece inside a frame; runs of ones across cuts;
    the spans of 7999 .. 8001 bits cut in front of their bail; a stream of three default tiles"""
    out = []
    for name, (plain, at) in sorted(H.ax25_windows().items()):
        for cut in range(at - 5, at + 7):
            out.append((f"{name}@{cut}", plain, [cut]))
        for cut, more in ((at - 2, 1), (at, 8), (at - 7, 136), (at + 1, 23)):
            out.append((f"{name}@{cut}+{more}", plain, [cut, cut + more]))
    body = M.siggen.ax25_hdlc_bits(M._frame(120, 5), pre_flags=2, post_flags=2)
    plain = M._pack(M._rand_bits(np.random.default_rng(3), 400) + [0] + body + M._rand_bits(np.random.default_rng(4), 400))
    out.append(("inside_a_frame", plain, [72, 132]))
    plain = M._pack([0, 1, 0] + M.FLAG + [1] * 45 + [0] + M.FLAG + body + [1] * 5 + [0] * 3)
    for cuts in ([2, 3], [3, 5], [5, 6], [6, 7], [1, 8], [2]):
        out.append((f"run_of_ones{cuts}", plain, cuts))
    for name in ("span7999_flag_calm", "span8000_flag_calm", "span8001_start_calm", "span8000_flag_stuffed", "span7999_start_stuffed"):
        plain = M.edge_streams()[name]
        tail = M._pack(M.FLAG + M.siggen.ax25_hdlc_bits(M._frame(40, 9), pre_flags=1, post_flags=2) + M._rand_bits(np.random.default_rng(5), 800))
        out.append((name, np.concatenate([plain, tail]), [500, len(plain)]))
        out.append((name + "_late", np.concatenate([plain, tail]), [len(plain) - 40]))
    plain = M.edge_streams()["late_bail"]
    out.append(("late_bail", plain, [2048 + 3, 2 * 2048 - 1]))
    out.append(("late_bail_words", plain, [2048, 2 * 2048 + 8]))
    for n in (0, 1, 24):
        out.append((f"short{n}", M.ax25_streams()[f"short{n}"], [n // 2]))
    return out


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("scan_carry_core")
    exe = d / "scan_carry_core_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "pymodem_amd", "csrc"), os.path.join(ROOT, "tests", "scan_carry_core_check.cpp"), "-o", str(exe)])
    return str(exe), d


def _carry(c):
    return struct.pack("<iiqQ", c["state"], c["ones"], c["counted"], c["tail"])


def test_pieces_stepped_on_the_host_are_the_model_s(checker):
    exe, d = checker
    cases = streams()
    pieces_total, lost, two, three = 0, 0, 0, 0
    with open(d / "cases.bin", "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for name, plain, cuts in cases:
            pieces = CM.model_pieces(np.bitwise_not(np.asarray(plain, dtype=np.uint8)), cuts, 0x1, 1, 0)      # (the LFSR is not this program's)
            f.write(struct.pack("<i", len(pieces)))
            two, three = two + (len(pieces) == 2), three + (len(pieces) == 3)
            for part, _, cin, cout, p in pieces:
                rec = part[:32].view(scan_record_dtype())[0]
                ev = part[32:32 + 8 * int(rec["events"])]
                f.write(struct.pack("<i", len(p)) + p.tobytes() + _carry(cin))
                f.write(struct.pack("<qqi", int(rec["bail_bit"]), int(rec["last_flag"]), int(rec["events"])) + ev.tobytes() + _carry(cout))
                pieces_total += 1
                lost += cin["state"] == SCAN_CARRY_LOST
    assert two >= 100 and three >= 40 and lost >= 2
    run = subprocess.run([exe, str(d / "cases.bin")] + [str(t) for t in TILES], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert run.stdout.strip().splitlines()[-1] == f"{pieces_total * len(TILES)} runs, 0 mismatches, 0 lanes wanted a third event, 0 racing stores", run.stdout[-3000:]


def test_the_checker_fails_on_a_wrong_carry(checker):
    """the program compares: a model carry with one more counted bit is a mismatch"""
    exe, d = checker
    plain, at = H.ax25_windows()["straddle_flag_3"]
    pieces = CM.model_pieces(np.bitwise_not(plain), [at], 0x1, 1, 0)
    with open(d / "wrong.bin", "wb") as f:
        f.write(struct.pack("<ii", 1, len(pieces)))
        for k, (part, _, cin, cout, p) in enumerate(pieces):
            rec = part[:32].view(scan_record_dtype())[0]
            ev = part[32:32 + 8 * int(rec["events"])]
            f.write(struct.pack("<i", len(p)) + p.tobytes() + _carry(cin))
            f.write(struct.pack("<qqi", int(rec["bail_bit"]), int(rec["last_flag"]), int(rec["events"])) + ev.tobytes() + _carry(dict(cout, counted=cout["counted"] + (k == 1))))
    run = subprocess.run([exe, str(d / "wrong.bin"), "3"], capture_output=True, text=True)
    assert run.returncode == 1 and "2 runs, 1 mismatches" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
