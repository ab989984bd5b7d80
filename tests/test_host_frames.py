"""pm_codec_decode_framed (pm_codec.cpp) on blocks written by the bit-serial model of pm_stream_scan's frames (frames_model.py): packets,
pending count and the state the decoder is left in are pm_codec_decode's, the frames come from the frame area and their CRC from the table,
and pm_codec_walked shows that nothing but the stream's tail went through the decoder.  No GPU: the kernel is held to the same model in
test_gpu_frames.py."""
import ctypes

import numpy as np
import pytest

import bitscan_model as M
import frames_model as FM
from pymodem_amd._native import HostJob, NativeError, check, lib, packet_dtype


class Codec:
    def __init__(self, kind=0, tol=0):
        self.h = ctypes.c_void_p()
        check(lib().pm_codec_create(kind, 1, 0, 0, tol, 3, ctypes.byref(self.h)))

    def __del__(self):
        lib().pm_codec_destroy(self.h)

    def fetch(self, pending):
        rows = np.zeros(max(1, pending), dtype=packet_dtype())
        got = ctypes.c_int64()
        check(lib().pm_codec_fetch(self.h, rows.ctypes.data, pending, ctypes.byref(got)))
        assert got.value == pending
        return [(int(r["streamaddress"]), bytes(r["data"][:r["len"]]), int(r["len"]), int(r["calculated_crc"]), int(r["carried_crc"]), int(r["valid_crc"]),
                 int(r["valid_header"]), int(r["bytes_corrected"])) for r in rows[:pending]]

    def decode(self, data, addr):
        pending = ctypes.c_int64()
        check(lib().pm_codec_decode(self.h, data.ctypes.data, addr.ctypes.data, len(data), ctypes.byref(pending)))
        return pending.value, self.fetch(pending.value)

    def decode_framed(self, data, addr, block):
        pending = ctypes.c_int64()
        check(lib().pm_codec_decode_framed(self.h, data.ctypes.data, addr.ctypes.data, len(data), block.ctypes.data, ctypes.byref(pending)))
        return pending.value, self.fetch(pending.value)

    def walked(self):
        w, j = ctypes.c_int64(), ctypes.c_int64()
        check(lib().pm_codec_walked(self.h, ctypes.byref(w), ctypes.byref(j)))
        return w.value, j.value


def _more(n):
    """what the second call is fed: noise with a frame in it, so that the state the first call left decides what comes out"""
    more = np.random.default_rng(n + 5).integers(0, 256, 4096, dtype=np.uint8)
    frame = M._pack(M.FLAG * 3 + M.siggen.ax25_hdlc_bits(M._frame(30, 9), pre_flags=0))
    more[100:100 + len(frame)] = frame
    return more


def both_routes(plain):
    plain = np.ascontiguousarray(plain, dtype=np.uint8)
    n = len(plain)
    more = _more(n)
    addr = 1000 + 40 * np.arange(n + len(more), dtype=np.int64)
    block, _ = FM.model_block_frames(plain)
    rec, _, body = M.split_block(block, 0, n)
    a, b = Codec(), Codec()
    got = [a.decode_framed(np.ascontiguousarray(body), addr[:n], block)]
    walked, jumped = a.walked()
    assert walked + jumped == n and walked >= 0 and jumped >= 0
    got.append(a.decode(more, addr[n:]))
    want = [b.decode(plain, addr[:n]), b.decode(more, addr[n:])]
    return got, want, walked, rec


@pytest.mark.parametrize("name", sorted(FM.all_streams()))
def test_frames_come_from_the_area_and_the_tail_from_the_decoder(name):
    plain = FM.all_streams()[name]
    got, want, walked, rec = both_routes(plain)
    assert got == want
    n = len(plain)
    lens = [p[2] for p in want[0][1]]
    if name.startswith("random"):
        # what the frames are for: only the stretch behind the stream's last flag is walked.  A consumer that ignores the table and walks the
        # frames gives the same packets and fails here (the list route's own bound is n / 8).
        assert rec["bail_bit"] == -1 and len(lens) >= 40
        assert walked <= n // 64, (walked, n)
    if name.startswith("survive"):
        assert lens == [70], "the 40 bytes in front of the run's end stay in the frame"
    if name == "long_no_bail":
        (row,) = want[0][1]
        frame = [f for _, _, f in FM.frames_of(plain) if f is not None][0]
        assert rec["bail_bit"] == -1 and len(frame) == 1830
        assert row[2] == 1280 and row[1] == frame[:1280] and row[3] == FM.crc16(frame[:-2]) == FM.host_crc(frame[:-2]), "a row's worth of bytes, the whole frame's CRC"
    if name.startswith("first_closes"):
        assert lens == [30] and FM.frames_of(plain)[0][1] == -1
    if name.startswith("bail"):
        assert rec["bail_bit"] >= 8 * 1200 and 33 in lens, "the frame behind the bail comes out of the byte-wise tail"
    if name == "frame1100":
        assert lens == [1100, 25] and rec["bail_bit"] > 0
    if name.startswith("len18_17"):
        assert lens == [18, 40]


def test_the_table_s_crc_is_the_row_s():
    """The calculated CRC of a framed packet is the table's word, not a second pass over the bytes: a table with another CRC shows in the row."""
    plain = M._pack(M.siggen.ax25_hdlc_bits(M._frame(40, 4)))
    n = len(plain)
    block, _ = FM.model_block_frames(plain)
    table, _ = FM.split_frames(block, n)
    at = M.SCAN_HEAD + M.scan_list_bytes(0, n) + (n + 7) // 8 * 8
    e = int(np.flatnonzero(table["len"] > 0)[0])
    good = int(table["crc"][e])
    block[at + 8 * e + 4:at + 8 * e + 8] = np.array([good ^ 0x0101], dtype="<u4").view(np.uint8)
    addr = np.arange(n, dtype=np.int64)
    _, rows = Codec().decode_framed(np.ascontiguousarray(plain), addr, block)
    assert [(r[3], r[5]) for r in rows] == [(good ^ 0x0101, 0)]
    assert rows[0][4] == good, "the frame's own CRC bytes are the carried one"


@pytest.mark.parametrize("name", ["random1", "long_no_bail", "bail_after_a_flag", "first_closes", "survive_at5", "short25"])
def test_host_batch_with_scan_frames_equals_the_job_without(name):
    plain = np.ascontiguousarray(FM.all_streams()[name])
    raw = np.bitwise_not(plain)                               # the identity polynomial, inverted
    addr = 7 + 8 * np.arange(len(raw), dtype=np.int64)
    block, _ = FM.model_block_frames(plain, lfsr_state=0)
    results = []
    for route in ("framed", "scanned", "plain"):
        c = Codec()
        seen = np.zeros_like(raw)
        jobs = (HostJob * 1)()
        j = jobs[0]
        j.codec, j.h_data, j.h_addr, j.n = c.h, raw.ctypes.data, addr.ctypes.data, len(raw)
        j.lfsr_poly, j.lfsr_state, j.lfsr_invert, j.h_plain = 0x1, 0, 1, seen.ctypes.data
        j.h_scan = None if route == "plain" else block.ctypes.data
        j.scan_frames = int(route == "framed")
        check(lib().pm_host_decode_batch(jobs, 1, 1))
        results.append((j.lfsr_state, j.pending, seen.tobytes(), c.fetch(j.pending)))
    assert results[0] == results[2] and results[1] == results[2]


def _tamper(block, n, e, field, value):
    at = M.SCAN_HEAD + M.scan_list_bytes(0, n) + (n + 7) // 8 * 8 + 8 * e + (0 if field == "len" else 4)
    block[at:at + 4] = np.array([value], dtype="<i4").view(np.uint8)


def test_a_table_that_cannot_belong_to_the_stream_is_refused():
    plain = np.ascontiguousarray(FM.all_streams()["len18_17_at2"])
    n = len(plain)
    addr = np.arange(n, dtype=np.int64)
    good, _ = FM.model_block_frames(plain)
    events = FM.frames_of(plain)
    e = [k for k, (_, _, f) in enumerate(events) if f is not None][0]
    P, F, frame = events[e]
    room = (P - max(F, 0)) // 8
    assert len(frame) <= room
    Codec().decode_framed(plain, addr, good)                  # the model's own table passes
    for value in (room + 1, -1, n):
        block = good.copy()
        _tamper(block, n, e, "len", value)
        with pytest.raises(NativeError, match="does not belong"):
            Codec().decode_framed(plain, addr, block)
    block = good.copy()
    _tamper(block, n, e, "len", room)                          # as long as the span allows: taken (the bytes are the area's)
    assert Codec().decode_framed(plain, addr, block)[1][0][2] == room


def test_a_codec_that_has_been_fed_and_an_il2p_codec_are_refused():
    plain = np.ascontiguousarray(FM.all_streams()["len18_17_at0"])
    addr = np.arange(len(plain), dtype=np.int64)
    block, _ = FM.model_block_frames(plain)
    c = Codec()
    c.decode(plain[:10], addr[:10])
    with pytest.raises(NativeError, match="just-created"):
        c.decode_framed(plain, addr, block)
    with pytest.raises(NativeError, match="AX.25"):
        Codec(1, 2).decode_framed(plain, addr, block)
