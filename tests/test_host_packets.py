"""pm_codec_decode_packets (pm_codec.cpp) on blocks written by the bit-serial model of pm_stream_scan's packets (il2p_packets_model.py):
packets, pending count, BytesCorrected and the state the decoder is left in are pm_codec_decode's, and pm_codec_walked shows that the attempts
with a record did not go through the decoder.  The model itself is held to the oracle's IL2PCodec.decode first.  No GPU: the kernels are held
to the same model in test_gpu_packets.py."""
import ctypes
import os

import numpy as np
import pytest

import bitscan_model as M
import il2p_packets_model as PM
from pymodem_amd._native import HostJob, NativeError, check, lib, packet_dtype

NAMES = sorted(PM.all_streams())


def _addr(n):
    return 1000 + 40 * np.arange(n, dtype=np.int64)


class Codec:
    def __init__(self, kind=1, tol=0, crc=True, disable_rs=False, min_dist=0):
        self.h = ctypes.c_void_p()
        check(lib().pm_codec_create(kind, int(crc), int(disable_rs), min_dist, tol, PM.IDENT, ctypes.byref(self.h)))

    def __del__(self):
        lib().pm_codec_destroy(self.h)

    def fetch(self, pending):
        rows = np.zeros(max(1, pending), dtype=packet_dtype())
        got = ctypes.c_int64()
        check(lib().pm_codec_fetch(self.h, rows.ctypes.data, pending, ctypes.byref(got)))
        assert got.value == pending
        return [(int(r["streamaddress"]), bytes(r["data"][:r["len"]]), int(r["bytes_corrected"]), int(r["calculated_crc"]), int(r["carried_crc"]), int(r["valid_crc"]),
                 int(r["valid_header"]), int(r["source_decoder"])) for r in rows[:pending]]

    def _call(self, fn, data, addr, *more):
        data = np.ascontiguousarray(data, dtype=np.uint8)
        pending = ctypes.c_int64()
        check(fn(self.h, data.ctypes.data, addr.ctypes.data, len(data), *more, ctypes.byref(pending)))
        return pending.value, self.fetch(pending.value)

    def decode(self, data, addr):
        return self._call(lib().pm_codec_decode, data, addr)

    def decode_packets(self, data, addr, block):
        return self._call(lib().pm_codec_decode_packets, data, addr, block.ctypes.data)

    def decode_scanned(self, data, addr, block):
        return self._call(lib().pm_codec_decode_scanned, data, addr, block.ctypes.data)

    def walked(self):
        w, j = ctypes.c_int64(), ctypes.c_int64()
        check(lib().pm_codec_walked(self.h, ctypes.byref(w), ctypes.byref(j)))
        return w.value, j.value


def _more(plain, seed):
    """what the second call is fed: the front of a packet closes the first call's stream (so that it begins there), the second call brings its
    rest and 4 KB of noise with another packet in it"""
    f = M._pack(PM._calm(seed, 24) + PM._frame(60, 900 + seed))
    first = np.concatenate([np.asarray(plain, dtype=np.uint8), f[:30]])
    more = np.random.default_rng(seed + 5).integers(0, 256, 4096, dtype=np.uint8)
    more[:len(f) - 30] = f[30:]
    g = M._pack(PM._frame(33, 901 + seed))
    more[700:700 + len(g)] = g
    return first, more


@pytest.mark.parametrize("name", NAMES)
def test_the_model_s_records_chain_to_the_oracle_s_packets(name):
    """The model is checked before anything is held to it: a consumer that uses its records by the rules gives IL2PCodec.decode's packets."""
    plain, tol, o = PM.all_streams()[name]
    block, _ = PM.block_of(name)
    addr = _addr(len(plain))
    got, info = PM.consume(plain, addr, tol, block=block, **o)
    assert got == PM.oracle_packets(plain, addr, tol, **o)
    records, placed, recs, _ = PM.split_packets(np.asarray(block), len(plain))
    assert records == len(recs) <= len(plain) // 64 + 2 and placed == int(np.isin(recs["status"], (PM.DONE, PM.BLOCK_FAIL)).sum())
    if name.startswith("count"):
        assert sorted(int(a) & 7 for a in recs["at"]) == list(range(8)) and len(got) == 8 and len(info["used"]) == 8
    if name == "late_hit":
        assert info["late_hits"] == 1 and len(got) == 1
    if name == "area_runs_out":
        assert recs["status"].tolist() == [PM.BLOCK_FAIL] * 12 + [PM.NOT_PLACED] * 28
    if name == "random_tol8":
        assert records == len(plain) // 64 + 2 and int(M.il2p_model(plain, tol).sum()) > records
        assert np.any(np.diff(recs["at"] >> 3) == 1), "candidates in neighbouring bytes"
    if name == "back_to_back":
        assert records == 130 and len(got) == 130
    if name.startswith("cut_in_") and name != "cut_in_whole":
        assert recs["status"].tolist() == [PM.INCOMPLETE]
    if name.startswith("first_candidate"):
        assert int(recs["at"][0]) >> 3 == 4 and int(recs["at"][-1]) >> 3 == len(plain) - 1 and recs["status"].tolist() == [PM.DONE, PM.INCOMPLETE]


def test_the_golden_resync_streams_chain_to_their_packets():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "il2p_resync.npz"))
    for tol in (0, 2):
        plain, addr = g[f"tol{tol}_data"], g[f"tol{tol}_addr"]
        got, info = PM.consume(plain, addr, tol)
        assert [p[0] for p in got] == g[f"tol{tol}_pkt_addr"].tolist() and [p[2] for p in got] == g[f"tol{tol}_pkt_corrected"].tolist()
        assert b"".join(p[1] for p in got) == g[f"tol{tol}_pkt_data"].tobytes() and len(info["used"]) > 300


def both_routes(name):
    plain, tol, o = PM.all_streams()[name]
    first, more = _more(plain, len(plain))
    addr = _addr(len(first) + len(more))
    block, _ = PM.model_block_packets(first, tol, **o)
    a, b = Codec(tol=tol, **o), Codec(tol=tol, **o)
    got = [a.decode_packets(first, addr[:len(first)], block)]
    walked, jumped = a.walked()
    assert walked + jumped == len(first) and walked >= 0 and jumped >= 0
    got.append(a.decode(more, addr[len(first):]))
    want = [b.decode(first, addr[:len(first)]), b.decode(more, addr[len(first):])]
    return got, want, walked, (first, addr, tol, o, block)


# the planted-packet streams without the adversarial spacing: what the cap on the machine's share is stated for
PLANTED = [n for n in NAMES if n.startswith(("count", "sync_flips", "header_errors", "block_errors", "errors876", "back_to_back", "cut_in_whole"))]


def _cap(used, n):
    """8 bytes per used record -- four for the sync_run guard, the hit byte, slack for the partial byte (which also pays for the four bytes
    that a fresh decoder walks at the stream's start) -- plus the bytes behind the last used record's end"""
    return 8 * len(used) + (n - (max(E for _, E in used) >> 3) if used else n)


@pytest.mark.parametrize("name", NAMES)
def test_rows_pending_corrections_and_the_state_left_behind_are_the_decoder_s(name):
    got, want, walked, (first, addr, tol, o, block) = both_routes(name)
    assert got == want
    assert len(want[1][1]) >= 1 or tol > 2, "the packet that begins in the first call comes out of the second (where chance hits leave it alone)"
    if name in PLANTED:
        _, info = PM.consume(first, addr, tol, block=block, **o)
        cap = _cap(info["used"], len(first))
        assert info["walked"] <= cap, "the model's chain stays within the cap"
        assert walked <= cap, (walked, cap)
        assert walked == info["walked"]


def test_the_records_are_what_spares_the_machine():
    """a consumer that ignores the table gives the same packets and walks every packet's bytes"""
    name = "count1023_crc"
    plain, tol, o = PM.all_streams()[name]
    block, _ = PM.block_of(name)
    addr = _addr(len(plain))
    a, b = Codec(tol=tol, **o), Codec(tol=tol, **o)
    assert a.decode_packets(plain, addr, np.asarray(block)) == b.decode_scanned(plain, addr, np.asarray(block))
    assert a.walked()[0] <= 8 * 8 + 6 and b.walked()[0] >= 8 * 1100


@pytest.mark.parametrize("name", ["count240_crc", "count0_nocrc", "block_errors", "block_errors_min_dist1", "block_errors_disable_rs", "late_hit", "area_runs_out", "short4",
                                  "sync_2_behind_a_packet"])
def test_host_batch_with_scan_packets_equals_the_job_without(name):
    plain, tol, o = PM.all_streams()[name]
    plain = np.ascontiguousarray(plain)
    raw = np.bitwise_not(plain)                               # the identity polynomial, inverted
    addr = 7 + 8 * np.arange(len(raw), dtype=np.int64)
    block, _ = PM.model_block_packets(plain, tol, lfsr_state=0, **o)
    results = []
    for route in ("packets", "scanned", "plain"):
        c = Codec(tol=tol, **o)
        seen = np.zeros_like(raw)
        jobs = (HostJob * 1)()
        j = jobs[0]
        j.codec, j.h_data, j.h_addr, j.n = c.h, raw.ctypes.data, addr.ctypes.data, len(raw)
        j.lfsr_poly, j.lfsr_state, j.lfsr_invert, j.h_plain = 0x1, 0, 1, seen.ctypes.data
        j.h_scan = None if route == "plain" else block.ctypes.data
        j.scan_packets = int(route == "packets")
        check(lib().pm_host_decode_batch(jobs, 1, 1))
        results.append((j.lfsr_state, j.pending, seen.tobytes(), c.fetch(j.pending)))
    assert results[0] == results[2] and results[1] == results[2]


def _tampered(block, n, e, **fields):
    out = np.array(block)
    at = M.SCAN_HEAD + M.scan_list_bytes(1, n) + (n + 7) // 8 * 8
    if e is None:
        head = out[at:at + 8].view("<i4")
        for k, v in fields.items():
            head[("records", "placed").index(k)] = v
    else:
        rec = out[at + 16 + 16 * e:at + 32 + 16 * e].view(PM.scan_packet_dtype())
        for k, v in fields.items():
            rec[k] = v
    return out


def test_a_table_that_cannot_belong_to_the_stream_is_refused():
    name = "block_errors"
    plain, tol, o = PM.all_streams()[name]
    plain = np.ascontiguousarray(plain)
    n = len(plain)
    addr = _addr(n)
    good = np.array(PM.block_of(name)[0])
    records, placed, recs, _ = PM.split_packets(good, n)
    done = int(np.flatnonzero(recs["status"] == PM.DONE)[1])
    failed = int(np.flatnonzero(recs["status"] == PM.BLOCK_FAIL)[0])
    want = Codec(tol=tol, **o).decode(plain, addr)
    assert Codec(tol=tol, **o).decode_packets(plain, addr, good) == want      # the model's own table passes
    H = 8 * (int(recs["at"][done]) >> 3) + (int(recs["at"][done]) & 7) + 1
    bad = [(None, dict(records=n // 64 + 3)), (None, dict(records=-1)), (None, dict(placed=records + 1)), (None, dict(placed=-1)),
           (done, dict(at=int(recs["at"][done - 1]))), (done, dict(at=int(recs["at"][done - 1]) - 8)), (0, dict(at=3 << 3 | 7)), (records - 1, dict(at=n << 3)),
           (done, dict(count=1024)), (done, dict(count=int(recs["count"][done]) + 1)), (done, dict(status=5)),
           (done, dict(off=(n + 7) // 8 * 8 - 8)), (done, dict(off=int(recs["off"][done]) + 4)), (failed, dict(off=(n + 7) // 8 * 8)),
           (done, dict(end=8 * n - H - 32 + 1)), (done, dict(end=int(recs["end"][done]) + 8)), (failed, dict(end=8 * n)), (failed, dict(end=119))]
    for e, fields in bad:
        c = Codec(tol=tol, **o)
        with pytest.raises(NativeError, match="does not belong"):
            c.decode_packets(plain, addr, _tampered(good, n, e, **fields))
        assert c.decode_packets(plain, addr, good) == want, "a refused table leaves the codec as it was"
    # what the rules let pass is harmless: a record at another offset is not used, a status that sends the hit to the machine neither
    for e, fields in ((done, dict(at=int(recs["at"][done]) ^ 1)), (done, dict(status=PM.INCOMPLETE)), (failed, dict(status=PM.NOT_PLACED))):
        assert Codec(tol=tol, **o).decode_packets(plain, addr, _tampered(good, n, e, **fields)) == want


def test_a_codec_that_has_been_fed_and_an_ax25_codec_are_refused():
    name = "count1_crc"
    plain, tol, o = PM.all_streams()[name]
    addr = _addr(len(plain))
    block = np.asarray(PM.block_of(name)[0])
    c = Codec(tol=tol, **o)
    c.decode(plain[:10], addr[:10])
    with pytest.raises(NativeError, match="just-created"):
        c.decode_packets(plain, addr, block)
    with pytest.raises(NativeError, match="IL2P"):
        Codec(kind=0).decode_packets(plain, addr, block)
