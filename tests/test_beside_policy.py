"""process_recordings_device(beside=k) without a GPU: which mark the driver takes next (loop_batch.next_mark), and the size of a piece taken at
a mark (RowPieces.piece_bytes(mark=t)) against pm_rows_scan_pieces' rule written out in plain numpy -- from the mark's host copy alone, with
no look at the run's records."""
import types

import numpy as np
import pytest


def _drive(chunks, k, ready_at):
    """the driver's loop over next_mark with `ready_at(step)` for what pm_lbatch_marks_ready says at each ask -> the marks taken"""
    from pymodem_amd.loop_batch import next_mark
    taken, last, step = [], -1, 0
    while True:
        t = next_mark(last, ready_at(step), chunks, k)
        step += 1
        if t is None:
            return taken
        assert t > last and (t + 1) % k == 0 and 0 <= t < chunks
        taken.append(t)
        last = t


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("chunks", [1, 2, 3, 6, 7, 10, 110])
def test_every_due_mark_in_order_while_the_run_is_going(k, chunks):
    # nothing is ready when asked (the driver then waits for the mark it was given): every due mark, in order, the last chunk's too if it is due
    assert _drive(chunks, k, lambda step: -1) == [t for t in range(chunks) if (t + 1) % k == 0]
    # the mark before the last one is ready: the same -- only the LAST mark ends the taking
    assert _drive(chunks, k, lambda step: chunks - 2) == [t for t in range(chunks) if (t + 1) % k == 0]


@pytest.mark.parametrize("k", [1, 3])
def test_the_last_mark_ends_the_taking(k):
    from pymodem_amd.loop_batch import next_mark
    for chunks in (1, 3, 7, 9):
        assert next_mark(-1, chunks - 1, chunks, k) is None, "the run was over before the first ask: one final piece"
        assert _drive(chunks, k, lambda step: chunks - 1 if step >= 1 else -1) == [t for t in range(chunks) if (t + 1) % k == 0][:1]
    assert next_mark(2, 5, 7, 3) == 5 and next_mark(5, 5, 7, 3) is None      # chunks no multiple of k: mark 6 is not due
    assert next_mark(-1, -1, 1, 1) == 0 and next_mark(0, 0, 1, 1) is None    # a single chunk
    assert next_mark(-1, -1, 2, 3) is None                                   # no due mark at all
    assert next_mark(-1, 0, 0, 1) is None                                    # (no chunks)


def _plain_rule(avail, taken, final):
    """include/pymodem_amd.h: n = avail - from, rounded down to a multiple of 8 unless final, never below 0; a row whose taken is no multiple
    of 8 has had its final piece"""
    out = []
    for a, t in zip(avail, taken):
        if t % 8:
            out.append(0)
            continue
        n = int(a) - int(t)
        if not final:
            n -= n % 8
        out.append(max(n, 0))
    return out


def test_piece_bytes_at_a_mark_is_the_rule_over_the_marks_host_copy():
    from pymodem_amd.loop_batch import RowPieces
    rows, cap = 64, 40
    rng = np.random.default_rng(3)
    marks = [np.sort(rng.integers(0, 48, size=(5, rows)), axis=0)]          # counts only grow from mark to mark
    marks[0][:, :8] = [[0, 0, 0, 0, 0, 0, 0, 0], [1, 7, 8, 9, 15, 16, 17, 0], [1, 8, 8, 16, 16, 24, 31, 0], [8, 8, 9, 16, 23, 24, 32, 0], [8, 8, 9, 16, 23, 24, 40, 0]]

    class Marks:
        def h_upto(self, t):
            return np.minimum(marks[0][t], cap)

    def no_records(*a, **k):
        raise AssertionError("a piece at a mark does not look at the run's records")
    taker = RowPieces.__new__(RowPieces)
    taker.run = types.SimpleNamespace(marks=Marks(), cap=cap, records=no_records, fetch=no_records, ok=no_records)
    taker.taken = np.zeros(rows, dtype=np.int64)
    seen = set()
    for t in range(5):
        for row0, nrows in ((0, rows), (8, 24), (5, 1)):
            got = taker.piece_bytes(row0, nrows, mark=t)
            assert got.dtype == np.int64 and list(got) == _plain_rule(np.minimum(marks[0][t], cap)[row0:row0 + nrows], taker.taken[row0:row0 + nrows], False)
        n = taker.piece_bytes(0, rows, mark=t)
        assert (n % 8 == 0).all() and (taker.taken + n <= np.minimum(marks[0][t], cap)).all()
        seen |= set(int(v) for v in n)
        taker.taken += n
    assert {0, 8, 16} <= seen
    # a final cut at a mark takes what is left; nothing comes behind a final piece
    last = taker.piece_bytes(0, rows, final=True, mark=4)
    assert list(last) == _plain_rule(np.minimum(marks[0][4], cap), taker.taken, True) and (last % 8 != 0).any()
    taker.taken += last
    assert list(taker.piece_bytes(0, rows, mark=4)) == _plain_rule(np.minimum(marks[0][4], cap), taker.taken, False)
    with pytest.raises(AssertionError):
        taker.piece_bytes(0, rows, upto=np.zeros(rows, np.int64), mark=0)
