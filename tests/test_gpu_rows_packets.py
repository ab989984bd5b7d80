"""pm_rows_packets (csrc/pm_bitscan.hip with the rules of pm_rows_packets.h): finished pm_packet rows on the device, behind pm_rows_scan.
The 600 synthetic rows of test_gpu_rows_scan -- AX.25 with frames, IL2P with packets, descramble only -- scanned with checkpoints into a
device block: every entry's status, count, first place and register and every packet row must be what tests/rows_packets_model.py makes
from the model blocks and the oracle (test_rows_packets_model.py holds that to the oracle's decoders), in one call and in calls whose row
counts hit the lane, wave and scan-trip edges; with room for one packet less the model's NO_ROOM rows are marked and nothing is stored
behind the capacity; a block in host memory is refused; the tile size of the scan changes nothing.
Then the executor: process_recordings_device(..., rows_packets=True) against the call without -- rows and PacketMeta lists, deferred and
not, packets, LFSR registers and slicer states -- with every row accounted for and the codecs of finished recordings never fed; and a
planted bail through SlicedRun.fetch_packets, which goes the existing way."""
import ctypes
import functools

import numpy as np
import pytest

import rows_packets_model as RP
import test_gpu_rows_scan as RS
from conftest import tuned
from pymodem_amd import _native as N
from pymodem_amd._native import lib

pytestmark = pytest.mark.gpu

SOURCES = (7, 8, 9)
CANARY = 0xC7


def _chains():
    """test_gpu_rows_scan's three chains; those with a codec are scanned with the checkpoints"""
    desc = RS._desc(RS._chains())
    desc[0].addrs = desc[1].addrs = 1
    return desc


@functools.lru_cache(maxsize=None)
def _device():
    ctx = RS._ctx()
    return ctx, RS._device_rows(ctx)


def rows_packets(row0, nrows, room, tile=0, host_block=False):
    """pm_rows_scan into a device block and pm_rows_packets behind it -> (status of either, head, entries, packet rows, bytes behind the room)"""
    ctx, (d_data, d_steps, d_recs, _) = _device()
    _, counts, _, _ = RS._rows()
    desc = _chains()
    n = [min(c, RS.CAP) for c in counts[row0:row0 + nrows]]
    h_counts = (ctypes.c_int64 * nrows)(*n)
    need = sum(N.rows_scan_steps_bytes(c) + N.scan_part_bytes(desc[(row0 + k) % 3].codec_kind, desc[(row0 + k) % 3].frames, desc[(row0 + k) % 3].packets, c,
                                                              desc[(row0 + k) % 3].addrs) for k, c in enumerate(n))
    block = ctx.upload(np.full(need + 64, 0xA5, dtype=np.uint8))
    offs, used = (ctypes.c_int64 * nrows)(), ctypes.c_size_t()
    with tuned(ctx, bitscan_tile_words=tile):
        rc = lib().pm_rows_scan(ctx.handle, d_recs.ptr, d_data.ptr, d_steps.ptr, RS.CAP, row0, nrows, desc, 3, h_counts, block.ptr, need, offs, ctypes.byref(used))
        assert rc == 0 and used.value == need
        out_bytes = N.rows_packets_bytes(nrows, room)
        out = ctx.upload(np.full(out_bytes + 2 * N.packet_dtype().itemsize, CANARY, dtype=np.uint8))
        sources = (ctypes.c_int32 * 3)(*SOURCES)
        host = np.zeros(8, dtype=np.uint8)
        rc = lib().pm_rows_packets(ctx.handle, d_recs.ptr, d_steps.ptr, RS.CAP, row0, nrows, desc, 3, sources, h_counts, host.ctypes.data if host_block else block.ptr,
                                   offs, out.ptr, out_bytes, ctypes.byref(used))
    if rc != 0:
        ctx.sync()
        return rc, None, None, None, None
    assert used.value == N.rows_packets_bytes(nrows)
    ctx.sync()
    raw = out.download()
    head = raw[:16].view(N.rows_packets_head_dtype())
    entries = raw[16:16 + 32 * nrows].view(N.rows_packets_entry_dtype())
    total = int(head["packets"][0])
    assert 0 <= total <= room
    at = N.rows_packets_bytes(nrows)
    return rc, head, entries, raw[at:at + total * N.packet_dtype().itemsize].view(N.packet_dtype()), raw[at + total * N.packet_dtype().itemsize:]


@functools.lru_cache(maxsize=None)
def _registers():
    raws, _, _, _ = RS._rows()
    chains = RS._chains()
    return [RS.host_lfsr(raws[row], *chains[row % 3][:3])[1] for row in range(RS.ROWS)]


def _compare(row0, nrows, room, got):
    rc, head, entries, rows, behind = got
    want_head, want_entries, want_rows = RP.scan_rows_call(row0, nrows, room, SOURCES)
    assert rc == 0
    assert head.tobytes() == want_head.tobytes(), (head, want_head)
    for field in ("status", "packets", "first", "corrected_left", "reserved"):
        bad = np.flatnonzero(entries[field] != want_entries[field])
        assert len(bad) == 0, (field, row0 + int(bad[0]), entries[bad[0]], want_entries[bad[0]])
    assert [int(v) for v in entries["lfsr_state"]] == _registers()[row0:row0 + nrows], "the register behind every row"
    assert len(rows) == len(want_rows)
    for q in range(len(rows)):
        assert rows[q:q + 1].tobytes()[:40] == want_rows[q:q + 1].tobytes()[:40], (q, rows[q], want_rows[q])
        length = int(rows["len"][q])
        assert np.array_equal(rows["data"][q][:length], want_rows["data"][q][:length]), q
        assert not rows["data"][q][length:].any(), (q, "zeros behind the packet, as pm_codec_fetch leaves them")
    assert (behind == CANARY).all(), "nothing is stored behind the packets"
    return entries


def test_rows_3_to_599_in_one_call():
    nrows = RS.ROWS - RS.ROW0
    entries = _compare(RS.ROW0, nrows, 700, rows_packets(RS.ROW0, nrows, 700))
    kinds = (np.arange(RS.ROW0, RS.ROWS) % 3)
    finished = entries["status"] == RP.FINISHED
    assert int((finished & (kinds == 1)).sum()) >= 181 and int((finished & (kinds == 0)).sum()) >= 175
    assert int(entries["packets"][kinds == 1].sum()) == 221 and int(entries["packets"][kinds == 0].sum()) == 433


@pytest.mark.parametrize("nrows", [1, 63, 64, 65, 256, 257])
def test_calls_at_the_lane_wave_and_trip_edges(nrows):
    for row0 in (9, 128):
        _compare(row0, nrows, 700, rows_packets(row0, nrows, 700))


def test_one_packet_short_of_the_total():
    nrows = RS.ROWS - RS.ROW0
    total = int(RP.scan_rows_call(RS.ROW0, nrows, 10 ** 9, SOURCES)[0]["packets"][0])
    entries = _compare(RS.ROW0, nrows, total - 1, rows_packets(RS.ROW0, nrows, total - 1))
    assert (entries["status"] == RP.NO_ROOM).sum() >= 1
    _compare(RS.ROW0, nrows, 0, rows_packets(RS.ROW0, nrows, 0))
    _compare(RS.ROW0, nrows, total, rows_packets(RS.ROW0, nrows, total))


def test_a_block_in_host_memory_is_refused():
    assert rows_packets(RS.ROW0, 8, 10, host_block=True)[0] == -2      # PM_ERR_ARG


@pytest.mark.parametrize("tile", [1, 3, 0])
def test_the_scan_s_tile_size_changes_nothing(tile):
    _compare(RS.ROW0, 300, 700, rows_packets(RS.ROW0, 300, 700, tile=tile))


def test_arguments():
    ctx, (d_data, d_steps, d_recs, _) = _device()
    desc = RS._desc(RS._chains())                           # no checkpoints: not this way
    h_counts, offs, used = (ctypes.c_int64 * 8)(), (ctypes.c_int64 * 8)(), ctypes.c_size_t()
    out = ctx.upload(np.zeros(N.rows_packets_bytes(8, 4), dtype=np.uint8))
    args = (ctx.handle, d_recs.ptr, d_steps.ptr, RS.CAP, 0, 8)
    assert lib().pm_rows_packets(*args, desc, 3, None, h_counts, out.ptr, offs, out.ptr, N.rows_packets_bytes(8, 4), ctypes.byref(used)) == -2
    desc = _chains()
    desc[1].packets = 0                                     # an IL2P chain without its table
    assert lib().pm_rows_packets(*args, desc, 3, None, h_counts, out.ptr, offs, out.ptr, N.rows_packets_bytes(8, 4), ctypes.byref(used)) == -2
    desc = _chains()
    assert lib().pm_rows_packets(ctx.handle, d_recs.ptr, d_steps.ptr, RS.CAP, 0, 4097, desc, 3, None, h_counts, out.ptr, offs, out.ptr, 1 << 20, ctypes.byref(used)) == -2
    ctx.sync()


# ---- through the batch engine's executor ---------------------------------------------------------------------------------------------
def _walked(codec):
    w, j = ctypes.c_int64(), ctypes.c_int64()
    N.check(lib().pm_codec_walked(codec._handle(), ctypes.byref(w), ctypes.byref(j)))
    return w.value, j.value


def _executor_case(case):
    if case == "ax25":
        return "bpsk300_ax25", [dict(RS.lines_of("bpsk_300.json")[0], codec={"type": "ax25", "options": {}})]
    mode, cfg = {"qpsk": ("qpsk2400_il2p", "qpsk_2400.json"), "bpsk": ("bpsk300_il2p", "bpsk_300.json")}[case]
    return mode, RS.lines_of(cfg)


@functools.lru_cache(maxsize=None)
def _without(case, as_rows):
    """the same call with the scan switches on and rows_packets off: made once per case and result form"""
    from pymodem_amd.loop_batch import process_recordings_device
    mode, lines = _executor_case(case)
    recs = RS._recordings(mode)
    sets = RS._chain_sets(lines, len(recs))
    got = process_recordings_device(sets, recs, chunk=8192, rows=as_rows, scan=True, frames=True, packets=True, addrs=True)
    return RS._rows_of(got, as_rows), [[ch[3].shift_register for ch in cs] for cs in sets], [[bytes(ch[2]._state) for ch in cs] for cs in sets]


@pytest.mark.parametrize("defer", [False, True])
@pytest.mark.parametrize("as_rows", [True, False])
@pytest.mark.parametrize("case", ["qpsk", "bpsk", "ax25"])
def test_executor_with_finished_rows_equals_the_executor_without(case, as_rows, defer):
    from pymodem_amd.loop_batch import process_recordings_device
    mode, lines = _executor_case(case)
    recs = RS._recordings(mode)
    want = _without(case, as_rows)
    if case != "ax25":                                      # ... which is the call with every switch off
        plain = RS._plainly(mode, {"qpsk": "qpsk_2400.json", "bpsk": "bpsk_300.json"}[case], as_rows)
        assert want[0] == plain[0] and want[1] == plain[1]
    sets = RS._chain_sets(lines, len(recs))
    stages = {}
    got = process_recordings_device(sets, recs, chunk=8192, rows=as_rows, stages=stages, rows_packets=True, defer=defer)
    if defer:
        got = got()
    assert stages.get("scanned") is True and stages.get("fused_slicers")
    assert RS._rows_of(got, as_rows) == want[0]
    assert [[ch[3].shift_register for ch in cs] for cs in sets] == want[1], "the LFSR registers, from the entries"
    assert [[bytes(ch[2]._state) for ch in cs] for cs in sets] == want[2], "the slicer states"
    assert sum(len(chain) // (N.packet_dtype().itemsize if as_rows else 1) for rec in want[0] for chain in rec) >= 1, "at least one packet is decoded"
    tally = stages["rows_packets"]
    assert tally["rows"] == len(recs) * len(lines) and tally["finished"] + sum(tally["handed"].values()) == tally["rows"], "every row is accounted for"
    assert tally["copied_bytes"] > 0
    never_fed = [cs for cs in sets if all(ch[4]._h is None for ch in cs)]
    assert all(ch[4]._h is not None for cs in sets if cs not in never_fed for ch in cs), "a recording goes one way or the other, whole"
    if not tally["handed"]:
        assert len(never_fed) == len(sets)
    assert len(never_fed) >= 1, "at least one recording is finished on the device"
    for cs in never_fed:
        for ch in cs:
            assert _walked(ch[4]) == (0, 0), "a finished recording's codecs are never fed"


def test_the_switch_defaults_to_off_and_does_not_go_with_pieces_or_beside():
    from pymodem_amd.loop_batch import process_recordings_device
    ctx = RS._ctx()
    assert ctx.tuned("pipe_rows_packets") == 0
    mode, lines = _executor_case("bpsk")
    recs = RS._recordings(mode)
    for other in (dict(pieces=3), dict(beside=4)):
        with pytest.raises(ValueError):
            process_recordings_device(RS._chain_sets(lines, len(recs)), recs, chunk=8192, rows_packets=True, **other)
    with tuned(ctx, pipe_rows_packets=1):
        stages = {}
        got = process_recordings_device(RS._chain_sets(lines, len(recs)), recs, chunk=8192, rows=True, stages=stages)
        assert RS._rows_of(got, True) == _without("bpsk", True)[0] and stages["rows_packets"]["rows"] == len(recs) * len(lines)
    stages = {}
    process_recordings_device(RS._chain_sets(lines, len(recs)), recs, chunk=8192, rows=True, stages=stages)
    assert "rows_packets" not in stages and not stages.get("scanned")
    sets = RS._chain_sets(lines, len(recs))
    sets[1][0][4].decode_pending([])                        # a codec that has been used: the tables are made for a just-created decoder
    stages = {}
    got = process_recordings_device(sets, recs, chunk=8192, rows=True, stages=stages, rows_packets=True)
    assert RS._rows_of(got, True) == _without("bpsk", True)[0] and stages["rows_packets"] is False


def test_a_planted_bail_goes_the_existing_way():
    """Two recordings of one AX.25 chain as a synthetic run: the first row holds a span of 8000 bits without a reset and frames behind its
    bail (test_gpu_rows_pieces.planted_bail), the second two frames.  The first is named BAIL and its part of the scan block decodes, the
    existing way, to the host decoder's packets; the second is finished on the device."""
    import scan_carry_model as CM
    import test_gpu_rows_pieces as RP3
    import test_host_scan_carry as H
    from pymodem_amd import chain_builder as cb, chain_execute as ce
    from pymodem_amd.loop_batch import SlicedRun
    ctx = RS._ctx()
    line = _executor_case("ax25")[1][0]
    chains = [cb.build_chain(48000, line) for _ in range(2)]
    lfsr = chains[0][3]
    bail, cuts = RP3.planted_bail()
    plains = [bail, np.ascontiguousarray(bail[cuts[1]:])]
    cap = (len(bail) + 64) // 8 * 8
    data, steps = np.full(2 * cap, 0x3C, np.uint8), np.tile((30 + np.arange(cap) % 11).astype(np.uint16), 2)
    recs = np.zeros(2, dtype=N.rowslice_dtype())
    addrs, raws = [], []
    for r, plain in enumerate(plains):
        raw = CM.scramble(plain if lfsr.invert else np.bitwise_not(plain), lfsr.polynomial)
        assert np.array_equal(RS.host_lfsr(raw, lfsr.polynomial, 0, bool(lfsr.invert))[0], plain)
        data[r * cap:r * cap + len(raw)], steps[r * cap] = raw, 0
        recs["count"][r], recs["first_addr"][r] = len(plain), 12345 + 1000 * r
        addrs.append(12345 + 1000 * r + np.cumsum(steps[r * cap:r * cap + len(plain)].astype(np.int64)))
        recs["last_addr"][r] = addrs[r][-1]
        raws.append(raw)
    run = SlicedRun(ctx, ctx.upload(data), ctx.upload(steps), ctx.upload(recs.view(np.uint8)), cap, 2, 0)
    ctx.sync()
    entries, rows, handed = run.fetch_packets(0, 2, [chains[0]], sources=[5])
    assert [N.ROWS_PACKETS_STATUS[s] for s in entries["status"]] == ["BAIL", "FINISHED"] and list(handed) == [0]
    want = [H.Codec(0).decode(plain, addr) for plain, addr in zip(plains, addrs)]
    assert len(want[0]) >= 2 and len(want[1]) >= 2
    got0 = ce._host_rows_scanned([chains[0]], handed[0], [5], True, True, True)[0]
    assert H._rows(got0) == H._rows(want[0]) and int(chains[0][3].shift_register) == RS.host_lfsr(raws[0], lfsr.polynomial, 0, bool(lfsr.invert))[1]
    got1 = rows[int(entries["first"][1]):int(entries["first"][1]) + int(entries["packets"][1])]
    assert H._rows(got1) == H._rows(want[1]) and got1.tobytes() == want[1].tobytes()
    assert int(entries["lfsr_state"][1]) == RS.host_lfsr(raws[1], lfsr.polynomial, 0, bool(lfsr.invert))[1]
