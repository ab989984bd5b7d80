"""The rules of pm_rows_packets as tests/rows_packets_model.py restates them, against the oracle's decoders, without a GPU: which streams
and rows the tables say everything about, and that every such row's packets are IL2PCodec.decode's / AX25Codec.decode's.  The counts are
conditions: a test of the kernels may leave out exactly the rows counted here as handed over, for the reason given here."""
import collections

import numpy as np

import il2p_packets_model as PM
import rows_packets_model as RP
from oracle import oracle as O

HANDED_STREAMS = {"cut_in_header": RP.INCOMPLETE, "cut_in_block1": RP.INCOMPLETE, "cut_in_block2": RP.INCOMPLETE, "cut_in_crc": RP.INCOMPLETE,
                  "first_candidate_lead9": RP.INCOMPLETE, "first_candidate_lead16": RP.INCOMPLETE, "late_hit": RP.LATE_HIT, "random_tol8": RP.TABLE_FULL,
                  "area_runs_out": RP.NOT_PLACED}


def test_the_49_streams():
    streams = PM.all_streams()
    assert len(streams) == 49
    handed, finished = {}, 0
    for name, (plain, tol, o) in sorted(streams.items()):
        status, packets, _ = RP.stream_walk(name)
        if status != RP.FINISHED:
            handed[name] = status
            assert not packets
            continue
        finished += 1
        want = PM.oracle_packets(plain, np.arange(len(plain)), tol, **o)
        assert [p[:3] for p in packets] == want, name
    assert handed == HANDED_STREAMS and finished == 40
    for name in [f"sync_{g}_behind_a_packet" for g in range(5)] + ["back_to_back", "block_errors", "block_errors_min_dist1", "resync_tol0", "resync_tol2"]:
        assert RP.stream_walk(name)[0] == RP.FINISHED and RP.stream_walk(name)[1], name


def _oracle_ax25(plain, addr):
    return [(int(p.streamaddress), bytes(bytearray(p.data)), 0) for p in O.AX25Codec(PM.IDENT).decode([int(b) for b in plain], [int(a) for a in addr])]


def test_the_597_rows():
    import test_gpu_rows_scan as RS
    _, _, _, plains = RS._rows()
    walks = RP.scan_rows_walks()
    count = {0: collections.Counter(), 1: collections.Counter(), 2: collections.Counter()}
    packets = collections.Counter()
    for row in range(RS.ROW0, RS.ROWS):
        kind = row % 3
        status, pkts, _ = walks[row]
        count[kind][RP.STATUS[status]] += 1
        if status != RP.FINISHED:
            continue
        packets[kind] += len(pkts)
        plain, addr = plains[row], RP.row_addresses(row, len(plains[row]))
        if kind == 1:
            assert [p[:3] for p in pkts] == PM.oracle_packets(plain, addr, RS.TOL, **RS.OPTS), row
        elif kind == 0:
            assert [p[:3] for p in pkts] == _oracle_ax25(plain, addr), row
    assert count[1] == {"FINISHED": 181, "NO_RECORD": 6, "INCOMPLETE": 11, "NOT_PLACED": 1} and packets[1] == 221
    assert count[0] == {"FINISHED": 175, "BAIL": 12, "SHORT": 12} and packets[0] == 433
    assert count[2] == {"NO_CODEC": 199}


def test_the_room():
    """one packet short of the total: the row that would pass it and every row behind it take none"""
    head, entries, rows = RP.scan_rows_call(3, 597, 10 ** 9)
    total = int(head["packets"][0])
    assert total == 221 + 433 and len(rows) == total and int(head["handed"][0]) == 597 - 181 - 175
    short, e2, rows2 = RP.scan_rows_call(3, 597, total - 1)
    last = int(np.flatnonzero(entries["packets"] > 0)[-1])
    assert (e2["status"][last:] == RP.NO_ROOM).all() and (e2["first"][last:] == int(short["packets"][0])).all() and (e2["packets"][last:] == 0).all()
    assert np.array_equal(e2[:last], entries[:last]) and np.array_equal(rows2, rows[:len(rows2)]) and len(rows2) == total - int(entries["packets"][last])
