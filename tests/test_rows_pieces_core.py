"""The piece arithmetic of pm_rows_scan_pieces (csrc/pm_bitscan_rows.h, pm_bitscan_addrs.h) without a GPU: rows_pieces_core_check.cpp steps
the prepare launch's trips on the host and every row's from, n, offsets and tiles must be those of the plain loop of rows_pieces_model.py --
the final rule, rows past their final piece, `upto` below `taken`, above the count and above the row's room, rows left out because the host's
length is wrong or the block is short -- and the step sums with the piece's step 0 must give the checkpoints and the total of a plain prefix
sum at every tile size from 1 to 256.  The program is built with the address and undefined-behaviour sanitizers, as a stand-alone program."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import rows_pieces_model as RM
from conftest import ROOT

CAP = 6144
CHAINS = [(0, 1, 0, 1), (1, 0, 1, 0), (-1, 0, 0, 1), (0, 0, 0, 0), (1, 0, 0, 1), (-1, 0, 0, 0)]


def test_the_rule():
    P = RM.piece_bytes
    assert P(100, CAP, 50, 0, False) == 48 and P(100, CAP, 50, 48, False) == 0 and P(100, CAP, 56, 48, False) == 8
    assert P(100, CAP, None, 48, False) == 48 and P(100, CAP, None, 96, False) == 0 and P(100, CAP, None, 96, True) == 4
    assert P(100, CAP, None, 100, True) == 0 and P(100, CAP, 1000, 100, True) == 0, "a row past its final piece gives empty pieces"
    assert P(100, CAP, 40, 48, False) == 0 and P(100, CAP, 40, 48, True) == 0 and P(100, CAP, -5, 0, True) == 0, "upto below taken"
    assert P(100, CAP, 10 ** 9, 0, True) == 100 and P(CAP + 100, CAP, CAP + 50, 0, True) == CAP and P(CAP + 100, CAP, None, 8, False) == CAP - 8
    assert P(-3, CAP, None, 0, True) == 0
    for m in range(1, 8):
        assert P(96 + m, CAP, None, 0, False) == 96 and P(96 + m, CAP, None, 96, True) == m and P(96 + m, CAP, None, 96 + m, True) == 0


def row_sets():
    """(rows (count, upto, taken, host_n), chains, tile_words, final, has_upto, short_by)"""
    rng = np.random.default_rng(20261)
    sets = []
    for nrows in (1, 255, 256, 257, 597, 4096):
        for tile_words in (1, 3, 256):
            for final, has_upto in ((0, 1), (1, 1), (1, 0), (0, 0)):
                if nrows == 4096 and (final, has_upto) != (0, 1):
                    continue
                counts = rng.integers(0, CAP + 200, nrows)
                taken = (rng.integers(0, CAP // 8 + 1, nrows) * 8) * (rng.random(nrows) < 0.7)
                taken = np.minimum(taken, np.minimum(counts, CAP) // 8 * 8)
                done = rng.random(nrows) < 0.1                # rows past their final piece: taken is the whole row, no multiple of 8
                taken = np.where(done & (np.minimum(counts, CAP) % 8 != 0), np.minimum(counts, CAP), taken)
                upto = taken + rng.integers(-40, 600, nrows)  # below taken, within 8 of it, beyond it
                upto[::7] = counts[::7] + 5                   # above the count
                upto[3::11] = CAP + 1000                      # above the row's room
                rows = []
                for r in range(nrows):
                    n = RM.piece_bytes(counts[r], CAP, upto[r] if has_upto else None, taken[r], final)
                    rows.append((int(counts[r]), int(upto[r]), int(taken[r]), n))
                sets.append((rows, CHAINS, tile_words, final, has_upto, 0))
                if nrows == 597:
                    # the host has a row's length wrong (too short: the row and those behind it pass the block), and a block 1 byte short
                    wrong = [list(r) for r in rows]
                    k = max(r for r in range(300) if rows[r][3] >= 8)
                    wrong[k][3] -= 8
                    sets.append(([tuple(r) for r in wrong], CHAINS, tile_words, final, has_upto, 0))
                    sets.append((rows, CHAINS, tile_words, final, has_upto, 1))
    return sets


def step_sums():
    """(tile_words, n, addr_before, steps padded to 8, checkpoints, total) at every tile size"""
    rng = np.random.default_rng(77)
    out = []
    for tw in range(1, 257):
        n = int(8 * tw * 2 + 8 * rng.integers(0, tw + 1) + rng.integers(0, 8)) if tw % 5 else int(rng.integers(0, 70))
        steps = rng.integers(0, 65536, (n + 7) // 8 * 8).astype(np.uint16)
        steps[:n][rng.random(n) < 0.05] = 65535
        if n:
            steps[0] = 65535 if tw % 2 else 1 + tw              # the piece's first step is not 0
        addr_before = int(rng.integers(0, 1 << 40))
        addr = addr_before + np.cumsum(steps[:n].astype(np.int64))
        out.append((tw, n, addr_before, steps, addr[::64].copy(), int(steps[:n].astype(np.int64).sum())))
    out.append((256, 2048 * 3, 5, np.full(2048 * 3, 65535, np.uint16), 5 + 65535 * (1 + 64 * np.arange(96, dtype=np.int64)), 65535 * 2048 * 3))
    return out


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("rows_pieces_core")
    exe = d / "rows_pieces_core_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "pymodem_amd", "csrc"), os.path.join(ROOT, "tests", "rows_pieces_core_check.cpp"), "-o", str(exe)])
    return str(exe), d


def test_prepare_trips_and_step_sums_match_the_plain_loops(checker):
    exe, d = checker
    sets, sums = row_sets(), step_sums()
    assert {len(s[0]) for s in sets} >= {1, 255, 256, 257, 597, 4096} and {s[2] for s in sets} == {1, 3, 256} and {s[0] for s in sums} == set(range(1, 257))
    left_out = checkpoints = 0
    with open(d / "cases.bin", "wb") as f:
        f.write(struct.pack("<i", len(sets)))
        for rows, chains, tile_words, final, has_upto, short_by in sets:
            table, (used, total) = RM.plain_table(rows, chains, tile_words, CAP, final, has_upto, short_by)
            left_out += sum(t[0] < 0 for t in table)
            f.write(struct.pack("<6i", len(rows), len(chains), tile_words, short_by, final, has_upto))
            for ch in chains:
                f.write(struct.pack("<4i", *ch))
            f.write(struct.pack("<q", CAP) + np.asarray(rows, "<i8").tobytes())
            for t in table:
                f.write(struct.pack("<4q2i", *t))
            f.write(struct.pack("<qi", used, total))
        f.write(struct.pack("<i", len(sums)))
        for tw, n, addr_before, steps, ckpt, total in sums:
            checkpoints += len(ckpt)
            f.write(struct.pack("<iqq", tw, n, addr_before) + steps.astype("<u2").tobytes() + ckpt.astype("<i8").tobytes() + struct.pack("<q", total))
    assert left_out > 0, "some rows are left out"
    run = subprocess.run([exe, str(d / "cases.bin")], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert run.stdout.strip().splitlines()[-1] == f"{len(sets)} cases, {len(sums)} step sums, {checkpoints} checkpoints, 0 mismatches", run.stdout[-3000:]


def test_a_wrong_length_leaves_the_row_out():
    rows = [(100, 100, 0, 96), (50, 50, 0, 48), (64, 64, 0, 64)]
    table, _ = RM.plain_table(rows, CHAINS, 256, CAP, 0, 1)
    assert [t[0] >= 0 for t in table] == [True, True, True] and [t[4] for t in table] == [96, 48, 64] and [t[3] for t in table] == [0, 0, 0]
    table, _ = RM.plain_table([(100, 100, 0, 96), (50, 50, 0, 40), (64, 64, 0, 64)], CHAINS, 256, CAP, 0, 1)
    assert [t[0] >= 0 for t in table] == [True, True, False], "the rows behind a row that the host has too short pass the block"
