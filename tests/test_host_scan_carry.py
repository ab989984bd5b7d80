"""pm_codec_decode_carried, pm_codec_scan_state and pm_host_job.scan_carry (pm_codec.cpp): parts written by scan_carry_model.py, piece after
piece, through the carried route for all four kinds of part -- event list, frame table, packet table, each with and without address
checkpoints.  The pm_packet rows must be those of pm_codec_decode fed the same pieces and the packets those of the oracle fed the whole
stream; pm_codec_walked must stay within what the model counts out per piece.  No GPU: the kernels are held to the same model in
test_gpu_scan_carry.py."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import bitscan_model as M
import frames_model as FM
import il2p_packets_model as PM
import scan_carry_model as CM
from conftest import GOLDEN
from oracle import oracle as O
from pymodem_amd._native import (SCAN_CARRY_LOST, SCAN_CARRY_OK, SCAN_CARRY_START, HostJob, NativeError, check, lib, packet_dtype, scan_carry_piece_dtype,
                                 scan_part_bytes)

POLY, INVERT = 0x21001, 1
FIRST = (1 << 40) + 3


class Codec:
    def __init__(self, kind, tol=0, crc=True, disable_rs=False, min_dist=0):
        self.h = ctypes.c_void_p()
        self.kind = kind
        check(lib().pm_codec_create(kind, int(crc), int(disable_rs), min_dist, tol, 5, ctypes.byref(self.h)))

    def __del__(self):
        lib().pm_codec_destroy(self.h)

    def fetch(self, pending):
        rows = np.zeros(max(1, pending), dtype=packet_dtype())
        got = ctypes.c_int64()
        check(lib().pm_codec_fetch(self.h, rows.ctypes.data, pending, ctypes.byref(got)))
        assert got.value == pending
        return rows[:pending].copy()

    def decode(self, data, addr):
        data, addr = np.ascontiguousarray(data), np.ascontiguousarray(addr)
        pending = ctypes.c_int64()
        check(lib().pm_codec_decode(self.h, data.ctypes.data, addr.ctypes.data, len(data), ctypes.byref(pending)))
        return self.fetch(pending.value)

    def carried(self, plain, addr, part, frames=0, packets=0, addrs=0):
        """addr: the piece's full addresses; with addrs they go as steps and first address, resolved from the part's checkpoints"""
        plain, addr, part = np.ascontiguousarray(plain), np.ascontiguousarray(addr, dtype=np.int64), np.ascontiguousarray(part)
        pending = ctypes.c_int64()
        if addrs:
            steps = np.diff(addr, prepend=addr[:1]).astype(np.uint16)
            check(lib().pm_codec_decode_carried(self.h, plain.ctypes.data, None, steps.ctypes.data, int(addr[0]) if len(addr) else 0, len(plain), part.ctypes.data,
                                                frames, packets, 1, ctypes.byref(pending)))
        else:
            check(lib().pm_codec_decode_carried(self.h, plain.ctypes.data, addr.ctypes.data, None, 0, len(plain), part.ctypes.data, frames, packets, 0,
                                                ctypes.byref(pending)))
        return self.fetch(pending.value)

    def walked(self):
        w, j = ctypes.c_int64(), ctypes.c_int64()
        check(lib().pm_codec_walked(self.h, ctypes.byref(w), ctypes.byref(j)))
        return w.value

    def fed(self):
        w, j = ctypes.c_int64(), ctypes.c_int64()
        check(lib().pm_codec_walked(self.h, ctypes.byref(w), ctypes.byref(j)))
        return w.value + j.value

    def scan_state(self):
        ones, counted = ctypes.c_int32(), ctypes.c_int64()
        check(lib().pm_codec_scan_state(self.h, ctypes.byref(ones), ctypes.byref(counted)))
        return ones.value, counted.value


def _addresses(n):
    return FIRST + 40 * np.arange(n, dtype=np.int64) + (np.arange(n, dtype=np.int64) // 100) * 7


def _oracle_rows(kind, plain, addr, opts):
    c = O.AX25Codec(ident="x") if kind == 0 else O.IL2PCodec("x", opts.get("crc", True), opts.get("disable_rs", False), opts.get("min_dist", 0), opts.get("tol", 0))
    return [(int(p.streamaddress), bytes(bytearray(p.data)), int(p.BytesCorrected)) for p in c.decode([int(b) for b in plain], [int(a) for a in addr])]


def _rows(rows):
    return [(int(r["streamaddress"]), bytes(r["data"][:r["len"]]), int(r["bytes_corrected"])) for r in rows]


def run_pieces(plain, cuts, kind, frames=0, packets=0, addrs=0, opts=None, expect_lost=()):
    """The stream in pieces through the model and the carried route.  The carry is reseeded from the codec -- as ScannedChain does -- in
    front of a piece whose carry says LOST.  Returns the model's pieces."""
    opts = dict(opts or {})
    tol = opts.get("tol", 0)
    plain = np.ascontiguousarray(plain, dtype=np.uint8)
    raw = CM.scramble(plain, POLY)
    addr = _addresses(len(plain))
    got, ref = Codec(kind, **opts), Codec(kind, **opts)
    pk = {k: v for k, v in opts.items() if k != "tol"} if packets else None
    edges = [0] + list(cuts) + [len(plain)]
    carry = CM.carry_start()
    rows_got, rows_ref, pieces = [], [], []
    for k, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        if carry["state"] == SCAN_CARRY_LOST and k not in expect_lost:
            carry = CM.carry_seeded(carry["lfsr_state"], *got.scan_state())
            if carry["state"] == SCAN_CARRY_START:           # (0, 0) from a codec that has been fed: this piece the ordinary way
                plain_piece, reg = CM.host_lfsr(raw[a:b], POLY, carry["lfsr_state"], INVERT)
                rows_got.append(got.decode(plain_piece, addr[a:b]))
                rows_ref.append(ref.decode(plain_piece, addr[a:b]))
                carry = dict(carry, lfsr_state=reg, state=SCAN_CARRY_LOST)
                continue
        cin = carry
        part, written, cout, plain_piece = CM.model_piece(raw[a:b], carry, POLY, INVERT, kind, tol, bool(frames), pk, addr[a:b] if addrs else None)
        assert len(part) == scan_part_bytes(kind, frames, packets, b - a, addrs) + 32
        assert np.array_equal(plain_piece, plain[a:b]), "the register crosses the cut"
        part = np.where(written, part, 0xA5).astype(np.uint8)       # what the device does not write is not read
        before = got.walked()
        rows_got.append(got.carried(plain_piece, addr[a:b], part, frames, packets, addrs))
        rows_ref.append(ref.decode(plain_piece, addr[a:b]))
        assert rows_got[-1].tobytes() == rows_ref[-1].tobytes(), (k, a, b)
        assert got.scan_state() == ref.scan_state()
        if kind == 0:
            assert got.walked() - before <= CM.walked_bound(part, b - a, frames), (k, a, b)
            if cout["state"] == SCAN_CARRY_OK and cout["counted"] < 8000:
                assert got.scan_state() == (cout["ones"], cout["counted"]), ("the model's carry-out is the decoder's registers", k, a, b)
        pieces.append((part, cin, cout))
        carry = cout
    flat = [r for rows in rows_got for r in _rows(rows)]
    assert flat == _oracle_rows(kind, plain, addr, opts), "the oracle fed the whole stream"
    return pieces


# ---- the model itself ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["random1", "dense", "len18_17_at3", "shared_zero", "abort_then_flag", "bail_at_once", "bail_after_a_flag", "short0", "short1", "short24",
                                  "span8000_start_calm", "span7999_flag_stuffed", "late_bail", "end3_six", "first_closes", "first_closes_after_run", "survive_at2",
                                  "two_flags_one_word", "long_no_bail"])
def test_a_single_start_piece_is_the_unpieced_model(name):
    plain = np.ascontiguousarray(FM.all_streams()[name])
    n = len(plain)
    raw = np.bitwise_not(plain)
    part, written, cout, p = CM.model_piece(raw, CM.carry_start(0), 0x1, 1, 0, 0, True)
    want, covered = FM.model_block_frames(plain, lfsr_state=0)
    front = len(M.model_block(plain, 0))
    assert np.array_equal(part[:front], want[:front])
    assert np.array_equal(part[:-32][written[:-32]], want[written[:-32]])
    assert np.array_equal(written[len(want) - len(covered):len(want)], covered)
    piece = part[-32:].view(scan_carry_piece_dtype())[0]
    assert (piece["state"], piece["ones"], piece["counted"], piece["pieces"], piece["bytes"]) == (SCAN_CARRY_START, 0, 0, 0, 0)
    assert cout["pieces"] == 1 and cout["bytes"] == n
    part, _, _, _ = CM.model_piece(raw, CM.carry_start(0), 0x1, 1, 0, 0, False)
    assert np.array_equal(part[:-32], M.model_block(plain, 0))


def test_the_oracle_s_codecs_fed_piece_by_piece_give_the_whole_stream_s_packets():
    plain = FM.all_streams()["abort_then_flag"]
    addr = _addresses(len(plain))
    want = _oracle_rows(0, plain, addr, {})
    assert len(want) >= 2
    for cut in range(1, len(plain), 7):
        c = O.AX25Codec(ident="x")
        got = c.decode([int(b) for b in plain[:cut]], [int(a) for a in addr[:cut]]) + c.decode([int(b) for b in plain[cut:]], [int(a) for a in addr[cut:]])
        assert [(int(p.streamaddress), bytes(bytearray(p.data)), int(p.BytesCorrected)) for p in got] == want
    plain, tol, o = PM.all_streams()["count64_crc" if "count64_crc" in PM.all_streams() else sorted(PM.all_streams())[0]]
    plain = plain[:700]
    addr = _addresses(len(plain))
    want = _oracle_rows(1, plain, addr, dict(o, tol=tol))
    for cut in range(1, len(plain), 37):
        c = O.IL2PCodec("x", o["crc"], o["disable_rs"], o["min_dist"], tol)
        got = c.decode([int(b) for b in plain[:cut]], [int(a) for a in addr[:cut]]) + c.decode([int(b) for b in plain[cut:]], [int(a) for a in addr[cut:]])
        assert [(int(p.streamaddress), bytes(bytearray(p.data)), int(p.BytesCorrected)) for p in got] == want


# ---- AX.25: cuts around what the carry decides ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ax25_windows():
    """name -> (plain bytes, the byte that holds the bit in question): 700 bytes of a straddle_* stream of bitscan_model.py around one of
    its marks -- a closing flag's zero, a frame's first stuffed zero, the zero behind seven ones, a closing flag's last one -- and a frame's
    inside"""
    out = {}
    streams = M.edge_streams()
    for name in ("straddle_flag", "straddle_stuffed", "straddle_run7", "straddle_bit151"):
        for which in (3, 11):                                 # two of the bit offsets
            mark = M.straddle_marks()[which]
            a = (mark >> 3) - 350
            out[f"{name}_{which}"] = (streams[name][a:a + 700].copy(), 350)
    out["inside_a_frame"] = (streams["straddle_flag"][(M.straddle_marks()[5] >> 3) - 330:(M.straddle_marks()[5] >> 3) + 370].copy(), 310)
    return out


MODES = [(0, 0), (1, 0), (0, 1), (1, 1)]


@pytest.mark.parametrize("frames,addrs", MODES)
@pytest.mark.parametrize("name", sorted(ax25_windows()))
def test_ax25_cut_at_every_byte_of_a_window(name, frames, addrs):
    plain, at = ax25_windows()[name]
    total = 0
    for cut in range(at - 5, at + 7):
        pieces = run_pieces(plain, [cut], 0, frames=frames, addrs=addrs)
        total += sum(int(p[0][:32].view(np.int32)[6]) for p in pieces)
        assert pieces[1][1]["state"] == SCAN_CARRY_OK
    assert total > 0, "events are listed"


@pytest.mark.parametrize("frames,addrs", MODES)
@pytest.mark.parametrize("size", [0, 1, 7, 8, 9, 23, 24])
def test_ax25_pieces_of_a_few_bytes(size, frames, addrs):
    plain, at = ax25_windows()["straddle_flag_3"]
    for start in (at - 30, at - 3, at):
        run_pieces(plain, [start, start + size], 0, frames=frames, addrs=addrs)
    cuts = list(range(100, 600, max(size, 1))) if size else [100, 100, 100, 300]
    run_pieces(plain, cuts, 0, frames=frames, addrs=addrs)


@pytest.mark.parametrize("frames,addrs", MODES)
def test_three_pieces_the_middle_one_without_a_reset(frames, addrs):
    body = M.siggen.ax25_hdlc_bits(M._frame(120, 5), pre_flags=2, post_flags=2)
    plain = M._pack(M._rand_bits(np.random.default_rng(3), 400) + [0] + body + M._rand_bits(np.random.default_rng(4), 400))
    start = (401 + 16) // 8 + 20
    pieces = run_pieces(plain, [start, start + 60], 0, frames=frames, addrs=addrs)
    assert int(pieces[1][0][:32].view(np.int32)[6]) == 0 and pieces[1][2]["counted"] == pieces[1][1]["counted"] + 480 - _dropped(plain[start:start + 60], pieces[1][1]["ones"])
    assert pieces[2][1]["counted"] > 480


def _dropped(piece, ones):
    d = 0
    for b in np.unpackbits(piece).tolist():
        if b:
            ones += 1
        else:
            d += ones == 5
            ones = 0
    return d


@pytest.mark.parametrize("frames,addrs", MODES)
@pytest.mark.parametrize("name", ["span8000_flag_calm", "span8000_flag_stuffed", "span8001_start_calm", "span7999_flag_calm"])
def test_a_span_cut_in_front_of_its_bail(name, frames, addrs):
    """span8000: piece 0 ends inside the span, piece 1 holds the flag that ends it -- its bail -- and hands on LOST, piece 2 starts LOST and
    goes wholly through the table, then the carry is seeded from the codec and piece 3 lists again.  span7999: no bail, nothing is lost."""
    assert name.startswith("span7999") or M.ax25_model(M.edge_streams()[name])[1] >= 0, "scanned whole, the stream bails"
    plain = M.edge_streams()[name]
    tail = M._pack(M.FLAG + M.siggen.ax25_hdlc_bits(M._frame(40, 9), pre_flags=1, post_flags=2) + M._rand_bits(np.random.default_rng(5), 800))
    plain = np.concatenate([plain, tail, tail])
    n0 = len(M.edge_streams()[name])
    cuts = [500, n0, n0 + len(tail)]
    pieces = run_pieces(plain, cuts, 0, frames=frames, addrs=addrs, expect_lost=(2,))
    states = [p[1]["state"] for p in pieces]
    if name.startswith("span7999") or name.endswith("stuffed"):
        # (stuffed: the span's 21 dropped zeros lie in piece 0, and piece 1 starts from what was COUNTED, as the decoder's registers do: 7979)
        assert states == [SCAN_CARRY_START, SCAN_CARRY_OK, SCAN_CARRY_OK, SCAN_CARRY_OK]
    else:
        assert states == [SCAN_CARRY_START, SCAN_CARRY_OK, SCAN_CARRY_LOST, SCAN_CARRY_OK]
        rec = pieces[2][0][:32]
        assert int(rec.view(np.int32)[6]) == 0 and int(rec.view(np.int64)[1]) >= 0, "a LOST piece lists nothing: its first reset is its bail"
        assert int(pieces[3][0][:32].view(np.int32)[6]) >= 2, "after the reseed the lists are back"


# ---- IL2P -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def il2p_stream():
    bits = PM._calm(91, 8 * 40 + 3) + PM._frame(20, 92) + PM._calm(93, 8 * 30 + 5) + PM._frame(33, 94, crc=True) + PM._calm(95, 8 * 50)
    return M._pack(bits)


@pytest.mark.parametrize("packets,addrs", MODES)
def test_il2p_cut_at_every_byte_of_a_packet(packets, addrs):
    """sync word, header, block and trailing CRC of the first packet, and the noise around it"""
    plain = il2p_stream()
    opts = dict(tol=0, crc=True, disable_rs=False, min_dist=0)
    first = 40 + PM.SYNC_AT // 8 - 2
    last = first + 2 + 3 + 15 + 20 + 16 + 4 + 3
    whole = _oracle_rows(1, plain, _addresses(len(plain)), opts)
    assert len(whole) == 2
    for cut in range(first, last):
        run_pieces(plain, [cut], 1, packets=packets, addrs=addrs, opts=opts)
    for size in (0, 1, 7, 8, 9, 23, 24):
        run_pieces(plain, [first + 4, first + 4 + size], 1, packets=packets, addrs=addrs, opts=opts)


@pytest.mark.parametrize("name", ["sync_flips2", "sync_in_first_bytes3", "pattern32"])
def test_il2p_streams_of_the_scan_in_uneven_pieces(name):
    plain, tol, _ = M.il2p_streams()[name]
    n = len(plain)
    cuts = sorted(set(int(c) for c in np.random.default_rng(n).integers(0, n, 9)))
    for packets in (0, 1):
        run_pieces(plain, cuts, 1, packets=packets, addrs=packets, opts=dict(tol=tol, crc=True, disable_rs=False, min_dist=0))


# ---- goldens ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["afsk_1200", "bpsk_300", "fsk_9600", "qpsk_2400"])
def test_golden_segments_piece_by_piece(golden, config_lines, tag):
    """the reference's slicer bytes of a recording fed in two segments -> the reference's packets per segment, every kind of part"""
    from pymodem_amd import chain_builder as cb
    g = golden("segments")
    for frames, addrs in MODES:
        chain = cb.build_chain(48000, config_lines(tag + ".json")[0])
        poly, invert, kind = chain[3].polynomial, int(bool(chain[3].invert)), chain[4]._kind
        if kind == 1 and frames:
            continue                                          # (IL2P chains: the list and the packet table, below)
        opts = dict(tol=int(chain[4].sync_tolerance), crc=bool(chain[4].collect_trailing_crc), disable_rs=bool(chain[4].disable_rs),
                    min_dist=int(chain[4].min_distance)) if kind == 1 else {}
        c = Codec(kind, **opts)
        carry = CM.carry_start(chain[3].shift_register)
        for k in range(2):
            data, addr = g[f"{tag}__seg{k}_slice_data"], g[f"{tag}__seg{k}_slice_addr"].astype(np.int64)
            use_addrs = addrs and len(addr) and int(np.diff(addr).max(initial=0)) < 65536 and int(np.diff(addr).min(initial=0)) >= 0
            packets = int(kind == 1 and addrs)               # (the two IL2P rounds: list without checkpoints, packet table with)
            pk = {k: v for k, v in opts.items() if k != "tol"} if packets else None
            part, written, carry, plain = CM.model_piece(data, carry, poly, invert, kind, opts.get("tol", 0), bool(frames), pk, addr if use_addrs else None)
            rows = c.carried(plain, addr, np.where(written, part, 0xA5).astype(np.uint8), frames, packets, int(bool(use_addrs)))
            assert len(rows) == int(g[f"{tag}__seg{k}_pkt_n"])
            assert np.array_equal(rows["streamaddress"], g[f"{tag}__seg{k}_pkt_addr"])
            assert np.array_equal(np.concatenate([r["data"][:r["len"]] for r in rows] + [np.zeros(0, np.uint8)]), g[f"{tag}__seg{k}_pkt_data"])


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_what_the_carried_route_refuses_leaves_the_codec_untouched():
    plain, at = ax25_windows()["straddle_flag_3"]
    raw = CM.scramble(plain, POLY)
    addr = _addresses(len(plain))
    pieces = CM.model_pieces(raw, [200, 400, 550], POLY, INVERT, 0, frames=True)
    parts = [np.where(w, p, 0xA5).astype(np.uint8) for p, w, _, _, _ in pieces]
    plains = [p[4] for p in pieces]
    edges = [0, 200, 400, 550, len(plain)]

    def feed(c, k, part=None):
        return c.carried(plains[k], addr[edges[k]:edges[k + 1]], parts[k] if part is None else part, 1, 0, 0)

    want = Codec(0)
    want_rows = [want.decode(plains[k], addr[edges[k]:edges[k + 1]]) for k in range(4)]
    c = Codec(0)
    assert feed(c, 0).tobytes() == want_rows[0].tobytes()
    state, fed = c.scan_state(), c.fed()
    with pytest.raises(NativeError, match="piece 2"):          # a skipped piece
        feed(c, 2)
    with pytest.raises(NativeError, match="START"):            # a repeated piece: piece 0 again, for a codec that has been fed
        feed(c, 0)
    assert (c.scan_state(), c.fed()) == (state, fed)
    assert feed(c, 1).tobytes() == want_rows[1].tobytes()
    with pytest.raises(NativeError, match="piece 1"):          # a repeated piece
        feed(c, 1)
    fresh = Codec(0)
    with pytest.raises(NativeError, match="never been fed"):   # a fresh codec with an OK carry piece
        feed(fresh, 1)
    assert fresh.fed() == 0
    assert feed(fresh, 0).tobytes() == want_rows[0].tobytes()
    no_piece = parts[2].copy()
    no_piece[-32:] = 0xA5                                       # a fed codec with no carry piece
    with pytest.raises(NativeError, match="carry piece"):
        feed(c, 2, no_piece)
    other = parts[2].copy()                                     # registers that are not the codec's
    other[-32:].view(scan_carry_piece_dtype())["counted"] += 8
    with pytest.raises(NativeError, match="counted"):
        feed(c, 2, other)
    assert feed(c, 2).tobytes() == want_rows[2].tobytes() and feed(c, 3).tobytes() == want_rows[3].tobytes()
    # the four existing entry points keep refusing a codec that has been fed, and a "not made" entry
    pending = ctypes.c_int64()
    with pytest.raises(NativeError, match="just-created"):
        check(lib().pm_codec_decode_framed(c.h, plains[1].ctypes.data, addr.ctypes.data, len(plains[1]), parts[1].ctypes.data, ctypes.byref(pending)))
    assert int(parts[1][32 + M.scan_list_bytes(0, 200) + 200:][:4].view("<i4")[0]) == -1, "piece 1 begins inside a frame's reach: its first entry is not made"
    fresh = Codec(0)
    with pytest.raises(NativeError, match="does not belong"):
        check(lib().pm_codec_decode_framed(fresh.h, plains[1].ctypes.data, addr.ctypes.data, len(plains[1]), parts[1].ctypes.data, ctypes.byref(pending)))


def test_the_batch_takes_a_carried_job():
    plain, at = ax25_windows()["straddle_bit151_11"]
    raw = CM.scramble(plain, POLY)
    addr = _addresses(len(plain))
    pieces = CM.model_pieces(raw, [at], POLY, INVERT, 0, frames=True, addr=addr)
    c, ref = Codec(0), Codec(0)
    reg = 0
    for k, (part, written, cin, cout, p) in enumerate(pieces):
        a, b = (0, at) if k == 0 else (at, len(plain))
        steps = np.diff(addr[a:b], prepend=addr[a:a + 1]).astype(np.uint16)
        seen = np.zeros(b - a, dtype=np.uint8)
        jobs = (HostJob * 1)()
        j = jobs[0]
        j.codec, j.h_data, j.h_addr, j.n = c.h, None, None, b - a
        j.h_addr_delta, j.addr_first, j.h_plain = steps.ctypes.data, int(addr[a]), seen.ctypes.data
        part = np.ascontiguousarray(part)
        j.h_scan, j.scan_frames, j.scan_addrs, j.scan_carry = part.ctypes.data, 1, 1, 1
        j.lfsr_poly, j.lfsr_state, j.lfsr_invert = POLY, reg, INVERT
        check(lib().pm_host_decode_batch(jobs, 1, 1))
        reg = j.lfsr_state
        assert reg == cout["lfsr_state"] and np.array_equal(seen, p)
        assert c.fetch(j.pending).tobytes() == ref.decode(p, addr[a:b]).tobytes()


def test_a_replayed_piece_0_is_refused_only_where_the_state_gives_it_away():
    """Piece 0 is taken at any time (a carry may be seeded at any time).  AX.25, a carry seeded OK from the codec: the replay meets registers
    that have moved on.  IL2P has no registers to hold against the piece: the replay is decoded again, as the header says."""
    plain, at = ax25_windows()["straddle_flag_3"]
    raw, addr = CM.scramble(plain, POLY), _addresses(len(plain))
    c = Codec(0)
    head, reg = CM.host_lfsr(raw[:200], POLY, 0, INVERT)
    c.decode(head, addr[:200])
    seeded = CM.carry_seeded(reg, *c.scan_state())
    assert seeded["state"] == SCAN_CARRY_OK and seeded["pieces"] == 0
    part, written, cout, p = CM.model_piece(raw[200:400], seeded, POLY, INVERT, 0, 0, True)
    c.carried(p, addr[200:400], part, 1, 0, 0)
    assert c.scan_state() != (seeded["ones"], seeded["counted"])
    with pytest.raises(NativeError, match="counted"):
        c.carried(p, addr[200:400], part, 1, 0, 0)
    iplain = il2p_stream()
    iraw, iaddr = CM.scramble(iplain, POLY), _addresses(len(iplain))
    opts = dict(crc=True, disable_rs=False, min_dist=0)
    part, written, cout, p = CM.model_piece(iraw, CM.carry_start(), POLY, INVERT, 1, 0, False, opts)
    c = Codec(1)
    first = c.carried(p, iaddr, part, 0, 1, 0)
    again = c.carried(p, iaddr, part, 0, 1, 0)
    assert len(first) == 2 and again.tobytes() == first.tobytes()
