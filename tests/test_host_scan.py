"""pm_codec_decode_scanned (pm_codec.cpp) on scan blocks written by the Python model of pm_stream_scan's layout (bitscan_model.py): the
packets, the pending count and the state the decoder is left in are pm_codec_decode's, and pm_codec_walked shows that the lists are
what the decoder went by.  No GPU: the blocks come from the model, the kernels are held to the same model in test_gpu_bitscan.py."""
import ctypes

import numpy as np
import pytest

import bitscan_model as M
from pymodem_amd._native import Packet, check, lib, packet_dtype


class Codec:
    def __init__(self, kind, tol=0):
        self.h = ctypes.c_void_p()
        check(lib().pm_codec_create(kind, 1, 0, 0, tol, 3, ctypes.byref(self.h)))

    def __del__(self):
        lib().pm_codec_destroy(self.h)

    def _fetch(self, pending):
        rows = np.zeros(max(1, pending), dtype=packet_dtype())
        got = ctypes.c_int64()
        check(lib().pm_codec_fetch(self.h, rows.ctypes.data, pending, ctypes.byref(got)))
        assert got.value == pending
        return [(int(r["streamaddress"]), bytes(r["data"][:r["len"]]), int(r["len"]), int(r["calculated_crc"]), int(r["carried_crc"]), int(r["valid_crc"]),
                 int(r["valid_header"]), int(r["bytes_corrected"])) for r in rows[:pending]]

    def decode(self, data, addr):
        pending = ctypes.c_int64()
        check(lib().pm_codec_decode(self.h, data.ctypes.data, addr.ctypes.data, len(data), ctypes.byref(pending)))
        return pending.value, self._fetch(pending.value)

    def decode_scanned(self, data, addr, block):
        pending = ctypes.c_int64()
        check(lib().pm_codec_decode_scanned(self.h, data.ctypes.data, addr.ctypes.data, len(data), block.ctypes.data, ctypes.byref(pending)))
        return pending.value, self._fetch(pending.value)

    def walked(self):
        w, j = ctypes.c_int64(), ctypes.c_int64()
        check(lib().pm_codec_walked(self.h, ctypes.byref(w), ctypes.byref(j)))
        return w.value, j.value


def both_routes(kind, tol, plain):
    """-> (packets of both calls by the scanned route, the same by the plain route, bytes walked in the scanned first call, record)"""
    plain = np.ascontiguousarray(plain, dtype=np.uint8)
    n = len(plain)
    more = np.random.default_rng(n + 5).integers(0, 256, 4096, dtype=np.uint8)
    if kind == 0:                                              # the second call finds something: a frame across the seam's far side
        frame = M._pack(M.FLAG * 3 + M.siggen.ax25_hdlc_bits(M._frame(30, 9), pre_flags=0))
        more[100:100 + len(frame)] = frame
    addr = 1000 + 40 * np.arange(n + len(more), dtype=np.int64)
    block = M.model_block(plain, kind, tol)
    rec, _, body = M.split_block(block, kind, n)
    a, b = Codec(kind, tol), Codec(kind, tol)
    got = [a.decode_scanned(np.ascontiguousarray(body), addr[:n], block)]
    walked, jumped = a.walked()
    assert walked + jumped == n and walked >= 0 and jumped >= 0
    got.append(a.decode(more, addr[n:]))
    want = [b.decode(plain, addr[:n]), b.decode(more, addr[n:])]
    return got, want, walked, rec


@pytest.mark.parametrize("name", sorted(M.ax25_streams()))
def test_ax25_decodes_from_the_event_list(name):
    plain = M.ax25_streams()[name]
    got, want, walked, rec = both_routes(0, 0, plain)
    assert got == want
    n = len(plain)
    if name.startswith("random"):
        # what the list is for: between closing flags (one in fourteen flags of random bits) nothing is walked.  A consumer that ignores
        # the list and walks every byte gives the same packets and fails here.
        assert rec["bail_bit"] == -1 and 40 <= rec["events"] <= 100
        assert walked <= n // 8, (walked, n)
    if name.startswith("len18_17"):
        assert [p[2] for p in want[0][1]] == [18, 40], "the 18-byte frame is a packet, the 17-byte frame is not"
    if name.startswith("bail"):
        assert rec["bail_bit"] >= 8 * 1200
        assert 33 in [p[2] for p in want[0][1]], "the frame behind the bail comes out of the byte-wise decoder"
    if name == "frame1100":
        assert [p[2] for p in want[0][1]] == [1100, 25] and rec["bail_bit"] > 0
    if name in ("shared_zero", "abort_then_flag"):
        assert len(want[0][1]) >= 2 and rec["bail_bit"] == -1
    if name == "dense":
        assert rec["bail_bit"] == -1


@pytest.mark.parametrize("name", sorted(M.il2p_streams()))
def test_il2p_jumps_from_candidate_to_candidate(name):
    plain, tol, planted = M.il2p_streams()[name]
    got, want, walked, rec = both_routes(1, tol, plain)
    assert got == want
    hit = M.il2p_model(plain, tol)
    for end, flips in planted.items():                        # the byte that holds the sync word's last bit
        k = (end - 1) >> 3
        if k >= 4:
            assert bool(hit[k]) == (flips <= tol), (name, end, flips)
    if name.startswith("sync_flips"):
        flips = int(name[-1])
        assert len(want[0][1]) == (8 if flips <= tol else 0)
    if name == "pattern32":
        assert len(want[0][1]) == 8
    if name.startswith("resync"):
        assert len(want[0][1]) >= 60
    if name == "random":
        # (1 + 24 + 276) / 2^24 per bit offset for the sync word: about nine candidates in 64 KiB, each a header attempt of 15 bytes and
        # four bytes until the register is the input again; n / 8 would hold seven false packets of full length besides
        assert rec["candidates"] < 64 and walked <= len(plain) // 8, (rec["candidates"], walked)


def test_a_codec_that_has_been_fed_is_refused():
    from pymodem_amd._native import NativeError
    plain = M.ax25_streams()["len18_17_at0"]
    addr = np.arange(len(plain), dtype=np.int64)
    for kind in (0, 1):
        c = Codec(kind, 2)
        c.decode(plain[:10], addr[:10])
        with pytest.raises(NativeError, match="just-created"):
            c.decode_scanned(plain, addr, M.model_block(plain, kind, 2))


def test_host_batch_takes_the_scanned_route():
    """pm_host_job.h_scan: bytes and register come from the block, h_plain receives a copy, the rows are the unscanned job's."""
    from pymodem_amd._native import HostJob
    rng = np.random.default_rng(5)
    raw = rng.integers(0, 256, 20000, dtype=np.uint8)
    addr = 7 + 8 * np.arange(len(raw), dtype=np.int64)
    for kind, poly, inv in ((0, 0x21001, 1), (1, 0x3, 0)):
        plain = np.zeros_like(raw)
        sr = ctypes.c_uint64(0)
        check(lib().pm_lfsr_unscramble(raw.ctypes.data, len(raw), poly, inv, ctypes.byref(sr), plain.ctypes.data))
        block = M.model_block(plain, kind, 2, lfsr_state=sr.value)
        results = []
        for scanned in (True, False):
            c = Codec(kind, 2)
            seen = np.zeros_like(raw)
            jobs = (HostJob * 1)()
            j = jobs[0]
            j.codec, j.h_data, j.h_addr, j.n = c.h, raw.ctypes.data, addr.ctypes.data, len(raw)
            j.lfsr_poly, j.lfsr_state, j.lfsr_invert, j.h_plain = poly, 0, inv, seen.ctypes.data
            j.h_scan = block.ctypes.data if scanned else None
            check(lib().pm_host_decode_batch(jobs, 1, 1))
            results.append((j.lfsr_state, j.pending, seen.tobytes(), c._fetch(j.pending)))
        assert results[0] == results[1]
        assert ctypes.sizeof(Packet) == packet_dtype().itemsize
