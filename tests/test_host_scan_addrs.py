"""pm_host_job.scan_addrs and pm_codec_decode_addrs (pm_codec.cpp): the three scanned routes -- event list, frame table, packet table -- with
the addresses behind checkpoints instead of expanded.  The blocks come from the models of the scan (bitscan_model, frames_model,
il2p_packets_model) with the checkpoints of addrs_model behind them; the pm_packet rows must be the job's with full addresses, byte for byte,
and pm_codec_addr_work must show that an address cost 63 steps at the most and was asked for only where a packet was queued or a byte walked.
No GPU: the kernels are held to the same model in test_gpu_scan_addrs.py and test_gpu_rows_addrs.py."""
import ctypes

import numpy as np
import pytest

import addrs_model as AM
import bitscan_model as M
import frames_model as FM
import il2p_packets_model as PM
from pymodem_amd._native import HostJob, NativeError, check, lib, packet_dtype, scan_part_bytes

FIRST = (1 << 40) + 3


def _steps(n, seed):
    """eight symbol periods mostly, with stretches of large and of zero steps: the sum passes 2^32 in a long stream"""
    rng = np.random.default_rng(seed)
    s = np.full(n, 40, dtype=np.uint16)
    big = rng.random(n) < 0.05
    s[big] = rng.integers(0, 65536, int(big.sum()), dtype=np.uint16)
    s[n // 3:n // 3 + 70] = 65535
    s[n // 2:n // 2 + 70] = 0
    if n:
        s[0] = 0
    return s


class Codec:
    def __init__(self, kind, tol=0, crc=True, disable_rs=False, min_dist=0):
        self.h = ctypes.c_void_p()
        check(lib().pm_codec_create(kind, int(crc), int(disable_rs), min_dist, tol, 5, ctypes.byref(self.h)))

    def __del__(self):
        lib().pm_codec_destroy(self.h)

    def fetch(self, pending):
        rows = np.zeros(max(1, pending), dtype=packet_dtype())
        got = ctypes.c_int64()
        check(lib().pm_codec_fetch(self.h, rows.ctypes.data, pending, ctypes.byref(got)))
        assert got.value == pending
        return rows[:pending].tobytes()                      # every field of every row

    def pair(self, fn):
        a, b = ctypes.c_int64(), ctypes.c_int64()
        check(fn(self.h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def walked(self):
        return self.pair(lib().pm_codec_walked)[0]

    def addr_work(self):
        return self.pair(lib().pm_codec_addr_work)


def cases():
    """(id, kind, frames, packets, codec options, plain bytes, the job's part without checkpoints)"""
    out = []
    for name in ("random1", "bail_after_a_flag", "len18_17_at0", "dense"):
        plain = np.ascontiguousarray(M.ax25_streams()[name], dtype=np.uint8)
        out.append(("list-ax25-" + name, 0, 0, 0, dict(tol=0), plain, lambda p=plain: M.model_block(p, 0, 0, lfsr_state=0)))
    for name in ("random", "resync_tol2" if "resync_tol2" in M.il2p_streams() else sorted(M.il2p_streams())[0], "pattern32"):
        plain, tol, _ = M.il2p_streams()[name]
        plain = np.ascontiguousarray(plain, dtype=np.uint8)
        out.append(("list-il2p-" + name, 1, 0, 0, dict(tol=tol), plain, lambda p=plain, t=tol: M.model_block(p, 1, t, lfsr_state=0)))
    for name in ("random1", "long_no_bail", "bail_after_a_flag", "first_closes", "survive_at5", "short25"):
        plain = np.ascontiguousarray(FM.all_streams()[name], dtype=np.uint8)
        out.append(("framed-" + name, 0, 1, 0, dict(tol=0), plain, lambda p=plain: FM.model_block_frames(p, lfsr_state=0)[0]))
    for name in ("count240_crc", "count0_nocrc", "block_errors", "late_hit", "area_runs_out", "short4", "sync_2_behind_a_packet", "back_to_back"):
        plain, tol, o = PM.all_streams()[name]
        plain = np.ascontiguousarray(plain, dtype=np.uint8)
        out.append(("packets-" + name, 1, 0, 1, dict(tol=tol, **o), plain, lambda p=plain, t=tol, o=o: PM.model_block_packets(p, t, lfsr_state=0, **o)[0]))
    return out


CASES = cases()


def _job(codec, raw, plain_out, block, frames, packets):
    jobs = (HostJob * 1)()
    j = jobs[0]
    j.codec, j.h_data, j.n = codec.h, raw.ctypes.data, len(raw)
    j.lfsr_poly, j.lfsr_state, j.lfsr_invert, j.h_plain = 0x1, 0, 1, plain_out.ctypes.data
    j.h_scan, j.scan_frames, j.scan_packets = block.ctypes.data, frames, packets
    return jobs, j


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_rows_with_checkpoints_are_the_rows_with_full_addresses(case):
    _, kind, frames, packets, opts, plain, make = case
    n = len(plain)
    raw = np.bitwise_not(plain)                               # the identity polynomial, inverted
    steps = _steps(n, n)
    addr = AM.addresses(FIRST, steps)
    part = np.ascontiguousarray(make(), dtype=np.uint8)
    assert len(part) == scan_part_bytes(kind, frames, packets, n)
    block = AM.with_checkpoints(part, FIRST, steps)
    assert len(block) == scan_part_bytes(kind, frames, packets, n, 1) == len(part) + AM.addr_bytes(n)
    results = []
    for route in ("full", "expanded", "checkpoints"):
        c = Codec(kind, **opts)
        seen = np.zeros_like(raw)
        jobs, j = _job(c, raw, seen, block, frames, packets)
        if route == "full":
            j.h_addr = addr.ctypes.data
        else:
            j.h_addr, j.h_addr_delta, j.addr_first = None, steps.ctypes.data, FIRST
            j.scan_addrs = int(route == "checkpoints")
        check(lib().pm_host_decode_batch(jobs, 1, 1))
        results.append((j.lfsr_state, j.pending, seen.tobytes(), c.fetch(j.pending)))
        lookups, added = c.addr_work()
        if route == "checkpoints":
            assert added <= 63 * lookups
            assert lookups <= j.pending + c.walked(), (lookups, j.pending, c.walked())
            assert lookups >= j.pending > 0 or j.pending == 0, "every queued packet has asked for its address"
        else:
            assert (lookups, added) == (0, 0), "the pointer form resolves nothing"
    assert results[1] == results[0], "the expansion that the job did until now"
    assert results[2] == results[0]
    if case[0] in ("list-ax25-random1", "framed-random1", "packets-back_to_back", "packets-count240_crc", "list-il2p-pattern32"):
        assert results[0][1] > 0, "packets whose addresses are compared"


def test_the_single_codec_entry_point_and_what_it_refuses():
    plain = np.ascontiguousarray(FM.all_streams()["random1"], dtype=np.uint8)
    n = len(plain)
    steps = _steps(n, 3)
    addr = AM.addresses(FIRST, steps)
    part = FM.model_block_frames(plain, lfsr_state=0)[0]
    block = AM.with_checkpoints(part, FIRST, steps)
    table_at = len(part)
    assert n > 3 * 64

    def decode(blk, first=FIRST, frames=1):
        c = Codec(0)
        pending = ctypes.c_int64()
        check(lib().pm_codec_decode_addrs(c.h, plain.ctypes.data, steps.ctypes.data, first, n, blk.ctypes.data, frames, 0, ctypes.byref(pending)))
        return c, c.fetch(pending.value)

    want = Codec(0)
    pending = ctypes.c_int64()
    check(lib().pm_codec_decode_framed(want.h, plain.ctypes.data, addr.ctypes.data, n, part.ctypes.data, ctypes.byref(pending)))
    want_rows = want.fetch(pending.value)
    assert pending.value >= 40
    c, rows = decode(block)
    assert rows == want_rows
    lookups, added = c.addr_work()
    assert pending.value <= lookups <= pending.value + c.walked() and added <= 63 * lookups

    def tampered(w, value):
        out = block.copy()
        out[table_at + 8 * w:table_at + 8 * w + 8] = np.array([value], dtype="<i8").view(np.uint8)
        return out
    A = AM.checkpoints(FIRST, steps)
    bad = [tampered(0, FIRST + 1), tampered(0, FIRST - 1),                       # A[0] is not the first address
           tampered(2, int(A[1]) - 1),                                           # one descending pair
           tampered(2, int(A[1]) + AM.MAX_GAP + 1)]                              # one gap that 64 steps cannot make
    for blk in bad:
        with pytest.raises(NativeError, match="checkpoint table"):
            decode(blk)
    with pytest.raises(NativeError, match="checkpoint table"):
        decode(block, first=FIRST + 1)
    # and through the batch: the job fails with PM_ERR_ARG
    c = Codec(0)
    seen = np.zeros_like(plain)
    jobs, j = _job(c, np.bitwise_not(plain), seen, bad[2], 1, 0)
    j.h_addr, j.h_addr_delta, j.addr_first, j.scan_addrs = None, steps.ctypes.data, FIRST, 1
    with pytest.raises(NativeError, match="checkpoint table"):
        check(lib().pm_host_decode_batch(jobs, 1, 1))
    # what the rules let pass: a gap of exactly 64 x 65535, and equal neighbours
    edge = steps.copy()
    edge[65:129], edge[129:193] = 65535, 0
    E = AM.checkpoints(FIRST, edge)
    assert int(E[2] - E[1]) == AM.MAX_GAP and E[3] == E[2]
    c = Codec(0)
    check(lib().pm_codec_decode_addrs(c.h, plain.ctypes.data, edge.ctypes.data, FIRST, n, AM.with_checkpoints(part, FIRST, edge).ctypes.data, 1, 0, ctypes.byref(pending)))
    # a refused table leaves the codec as it was: the same codec takes the good block afterwards
    c = Codec(0)
    pending = ctypes.c_int64()
    with pytest.raises(NativeError):
        check(lib().pm_codec_decode_addrs(c.h, plain.ctypes.data, steps.ctypes.data, FIRST, n, bad[0].ctypes.data, 1, 0, ctypes.byref(pending)))
    check(lib().pm_codec_decode_addrs(c.h, plain.ctypes.data, steps.ctypes.data, FIRST, n, block.ctypes.data, 1, 0, ctypes.byref(pending)))
    assert c.fetch(pending.value) == want_rows


def test_the_model_s_look_up_is_the_prefix_sum():
    steps = _steps(70_000, 1)
    steps[:] = 65535
    addr = AM.addresses(FIRST, steps)
    A = AM.checkpoints(FIRST, steps)
    assert len(A) == (70_000 + 63) // 64 and int(A[-1]) - FIRST > 1 << 32
    for k in (0, 1, 63, 64, 65, 65537, 69_999):
        a, added = AM.lookup(A, steps, k)
        assert a == int(addr[k]) and added == k % 64
