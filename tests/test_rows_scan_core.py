"""Where things lie in a pm_rows_scan block (csrc/pm_bitscan_rows.h) without a GPU: rows_scan_core_check.cpp steps the prepare launch's
scan on the host -- trips of 256 rows, a carry from trip to trip -- and every row's block offset, first tile and first places must be those
of a plain prefix sum made here; for every tile index of every batch the binary search over the row table must return what the linear walk
of the job form's job_of_tile returns, rows of zero bytes included.  The program is built with the address and undefined-behaviour
sanitizers, as a stand-alone program."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from pymodem_amd import _native as N

CAP = 6144
EDGES = [0, 1, 7, 8, 2040, 2048, 2056]
# kinds cycling 0, 1, -1 with frames and packets on and off
CHAINS = [(0, 1, 0), (1, 0, 1), (-1, 0, 0), (0, 0, 0), (1, 0, 0), (-1, 0, 0)]


def table(counts, chains, tile_words, cap=CAP, short_by=0):
    """The plain prefix sum: per row (off, ev0, pk0, n, tile0), then (used, tiles)."""
    rows, off, tiles, events, places = [], 0, 0, 0, 0
    sizes = []
    for r, count in enumerate(counts):
        kind, frames, packets = chains[r % len(chains)]
        n = min(max(int(count), 0), cap)
        sizes.append((N.rows_scan_steps_bytes(n) + N.scan_part_bytes(kind, frames, packets, n), (-(-n // 8) + tile_words - 1) // tile_words,
                      n // 19 + 2 if frames else 0, n // 64 + 2 if packets else 0, n, frames, packets))
    limit = sum(s[0] for s in sizes) - short_by
    for size, t, e, p, n, frames, packets in sizes:
        fits = off + size <= limit
        rows.append((off if fits else -1, events if frames else -1, places if packets else -1, n, tiles))
        off, tiles, events, places = off + size, tiles + t, events + e, places + p
    return rows, (off, tiles)


def row_sets():
    rng = np.random.default_rng(20260)
    sets = []
    for nrows in (1, 255, 256, 257, 600, 4096):
        for tile_words in (1, 3, 256):
            counts = rng.integers(0, 6001, nrows)
            counts[::5] = [EDGES[k % len(EDGES)] for k in range(len(counts[::5]))]
            if nrows == 1:
                for c in EDGES + [int(counts[0])]:
                    sets.append(([c], CHAINS[:1], tile_words, 0))
                    sets.append(([c], CHAINS[1:2], tile_words, 0))
                continue
            sets.append((counts.tolist(), CHAINS, tile_words, 0))
    # runs of consecutive empty rows at the start, in the middle and at the end; every row empty; a count beyond the row's room
    for tile_words in (1, 3, 256):
        c = rng.integers(1, 3000, 600)
        c[:5] = 0
        c[254:259] = 0
        c[300:312] = 0
        c[-4:] = 0
        c[100] = CAP + 100
        sets.append((c.tolist(), CHAINS, tile_words, 0))
        sets.append(([0] * 300, CHAINS, tile_words, 0))
        sets.append(([0, 0, 0, 9, 0, 0], CHAINS[:2], tile_words, 0))
        # a block one byte short of the need: the last row with anything in it, and those behind, are left out
        sets.append((c.tolist(), CHAINS, tile_words, 1))
    return sets


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("rows_scan_core")
    exe = d / "rows_scan_core_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "pymodem_amd", "csrc"), os.path.join(ROOT, "tests", "rows_scan_core_check.cpp"), "-o", str(exe)])
    return str(exe), d


def test_prepare_scan_and_tile_search_match_the_prefix_sum(checker):
    exe, d = checker
    sets = row_sets()
    assert {len(s[0]) for s in sets} >= {1, 255, 256, 257, 600, 4096} and {s[2] for s in sets} == {1, 3, 256}
    tiles = 0
    with open(d / "cases.bin", "wb") as f:
        f.write(struct.pack("<i", len(sets)))
        for counts, chains, tile_words, short_by in sets:
            rows, (used, total) = table(counts, chains, tile_words, short_by=short_by)
            tiles += total
            f.write(struct.pack("<4i", len(counts), len(chains), tile_words, short_by))
            for ch in chains:
                f.write(struct.pack("<3i", *ch))
            f.write(np.asarray(counts, "<i8").tobytes() + struct.pack("<q", CAP))
            for row in rows:
                f.write(struct.pack("<3q2i", *row))
            f.write(struct.pack("<qi", used, total))
    run = subprocess.run([exe, str(d / "cases.bin")], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert run.stdout.strip().splitlines()[-1] == f"{len(sets)} cases, {tiles} tiles, 0 mismatches", run.stdout[-3000:]


def test_the_short_block_leaves_rows_out_and_the_full_one_none():
    c = [100, 0, 50, 0, 0]
    rows, _ = table(c, CHAINS, 256)
    assert all(r[0] >= 0 for r in rows)
    rows, _ = table(c, CHAINS, 256, short_by=1)
    # (every row ends at least a record -- 32 bytes -- in front of the next one's end: only the last row passes a block one byte short)
    assert [r[0] >= 0 for r in rows] == [True, True, True, True, False], "an empty row still has a record to write"
    rows, _ = table(c, CHAINS, 256, short_by=33)
    assert [r[0] >= 0 for r in rows] == [True, True, True, False, False]


def test_the_python_side_s_sizes_are_the_header_s():
    """_native.scan_part_bytes against the macros' own pieces, at the sizes where the divisions step"""
    for n in (0, 1, 7, 8, 18, 19, 63, 64, 65, 2048, 6144):
        assert N.scan_part_bytes(0, 1, 0, n) == N.SCAN_HEAD + N.scan_list_bytes(0, n) + (n + 7) // 8 * 8 + N.scan_frame_table_bytes(n) + N.scan_frame_area_bytes(n)
        assert N.scan_part_bytes(1, 0, 1, n) == N.SCAN_HEAD + N.scan_list_bytes(1, n) + (n + 7) // 8 * 8 + N.scan_packet_table_bytes(n) + N.scan_packet_area_bytes(n)
        assert N.scan_part_bytes(-1, 0, 0, n) == N.SCAN_HEAD + (n + 7) // 8 * 8
        assert N.rows_scan_steps_bytes(n) == (2 * n + 7) // 8 * 8
