"""The dense form of pm_stream_packets as tests/stream_packets_model.py restates it, against the oracle's decoders, without a GPU: which
of the model's streams the tables say everything about -- the same 40 of il2p_packets_model's 49 that the row form finishes, since the rule is
the same -- the status of every stream that is handed over, and that the records of every finished stream, read back through the package's
record iterator, are IL2PCodec.decode's / AX25Codec.decode's packets at the stream's own addresses, 16-bit steps or not.  The statuses are
conditions: a test of the kernels may leave out exactly the streams named here, for the reason given here."""
import numpy as np

import bitscan_model as M
import il2p_packets_model as PM
import rows_packets_model as RP
import stream_packets_model as SP
from oracle import oracle as O
from pymodem_amd import _native as N

HANDED_IL2P = {"cut_in_header": RP.INCOMPLETE, "cut_in_block1": RP.INCOMPLETE, "cut_in_block2": RP.INCOMPLETE, "cut_in_crc": RP.INCOMPLETE,
               "first_candidate_lead9": RP.INCOMPLETE, "first_candidate_lead16": RP.INCOMPLETE, "late_hit": RP.LATE_HIT, "random_tol8": RP.TABLE_FULL,
               "area_runs_out": RP.NOT_PLACED}
HANDED_AX25 = {"frame1100": RP.BAIL, "bail_at_once": RP.BAIL, "bail_after_a_flag": RP.BAIL, "short0": RP.SHORT, "short1": RP.SHORT, "short23": RP.SHORT}


def _oracle_ax25(plain, addr):
    return [(int(p.streamaddress), bytes(bytearray(p.data)), 0) for p in O.AX25Codec(PM.IDENT).decode([int(b) for b in plain], [int(a) for a in addr])]


def _dense(jobs, walks, room=10 ** 9):
    head, entries, records = SP.model_call(jobs, room, walks)
    raw = np.concatenate([head.view(np.uint8), entries.view(np.uint8), records])
    assert len(raw) == N.stream_packets_bytes(len(jobs), int(head["bytes"][0])) and len(records) % 8 == 0
    return head, entries, raw


def test_the_49_il2p_streams_finish_where_the_row_form_finishes_them():
    jobs, walks = SP.il2p_jobs(), SP.il2p_walks()
    assert len(jobs) == 49
    head, entries, raw = _dense(jobs, walks)
    assert {j["name"]: int(e["status"]) for j, e in zip(jobs, entries) if e["status"] != RP.FINISHED} == HANDED_IL2P
    assert int((entries["status"] == RP.FINISHED).sum()) == 40 and int(head["handed"][0]) == 9 and int(head["jobs"][0]) == 49
    # the same streams at addresses 0, 1, 2, ...: what test_rows_packets_model.py counts for the row form
    assert [RP.stream_walk(j["name"])[0] for j in jobs] == [int(s) for s in entries["status"]]
    got = SP.records_of(raw, len(jobs))
    some = 0
    for j, e, mine in zip(jobs, entries, got):
        if e["status"] != RP.FINISHED:
            assert not mine and e["packets"] == 0 and e["corrected_left"] == 0
            continue
        want = PM.oracle_packets(j["plain"], j["addr"], j["tol"], j["crc"], j["disable_rs"], j["min_dist"])
        assert mine == want, j["name"]
        some += len(want)
    assert some == int(head["packets"][0]) >= 60
    assert int(np.diff(jobs[0]["addr"]).max()) > 65535, "the addresses take steps that 16 bits do not hold"


def test_the_ax25_streams():
    jobs, walks = SP.ax25_jobs() + SP.events_jobs(), SP.ax25_walks() + SP.events_walks()
    head, entries, raw = _dense(jobs, walks)
    assert {j["name"]: int(e["status"]) for j, e in zip(jobs, entries) if e["status"] != RP.FINISHED} == HANDED_AX25
    got = SP.records_of(raw, len(jobs))
    for j, e, mine in zip(jobs, entries, got):
        if e["status"] != RP.FINISHED:
            continue
        want = _oracle_ax25(j["plain"], j["addr"])
        assert [(a, d[:N.PKT_MAX], c) for a, d, c in want] == mine, j["name"]
    by_name = {j["name"]: (j, e) for j, e in zip(jobs, entries)}
    for events in SP.EVENT_COUNTS:
        j, e = by_name[f"events{events}"]
        rec, _, _ = M.split_block(j["block"], 0, len(j["plain"]))
        assert int(rec["events"]) == events and int(e["packets"]) == max(0, events - 1), "a first flag that closes nothing, then a frame a flag"
    # a frame longer than a packet row is cut, and keeps the whole frame's CRCs
    j, e = by_name["long_no_bail"]
    at = N.stream_packets_bytes(len(jobs)) + int(e["first_byte"])
    h = raw[at:at + 40].view(N.head_dtype())[0]
    whole = _oracle_ax25(j["plain"], j["addr"])[0][1]
    assert len(whole) == 1830 and int(h["len"]) == N.PKT_MAX and N.stream_packets_record_bytes(1830) == 40 + N.PKT_MAX
    assert int(h["calculated_crc"]) == O.crc16(list(whole[:-2])) and int(h["carried_crc"]) == whole[-2] | whole[-1] << 8


def test_the_room_is_counted_in_bytes():
    """8 bytes short of the total: the last job with records and every job behind it take none, and lie at the total"""
    jobs, walks = SP.ax25_jobs(), SP.ax25_walks()
    head, entries, raw = _dense(jobs, walks)
    total = int(head["bytes"][0])
    assert _dense(jobs, walks, total)[2].tobytes() == raw.tobytes() and _dense(jobs, walks, total + 7)[2].tobytes() == raw.tobytes()
    short, e2, raw2 = _dense(jobs, walks, total - 8)
    last = int(np.flatnonzero(entries["packets"] > 0)[-1])
    assert (e2["status"][last:] == RP.NO_ROOM).all() and (e2["first_byte"][last:] == int(short["bytes"][0])).all() and (e2["packets"][last:] == 0).all()
    assert np.array_equal(e2[:last], entries[:last]) and int(short["bytes"][0]) == int(entries["first_byte"][last])
    assert int(short["handed"][0]) == int(head["handed"][0]) + int((entries["status"][last:] == RP.FINISHED).sum())
    assert raw2[N.stream_packets_bytes(len(jobs)):].tobytes() == raw[N.stream_packets_bytes(len(jobs)):][:int(short["bytes"][0])].tobytes()
    none, e3, _ = _dense(jobs, walks, 0)
    first = int(np.flatnonzero(entries["packets"] > 0)[0])
    assert int(none["bytes"][0]) == 0 and (e3["status"][first:] == RP.NO_ROOM).all() and np.array_equal(e3[:first], entries[:first])
