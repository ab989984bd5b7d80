"""pm_stream_scan with pm_scan_job.addrs (csrc/pm_bitscan.hip: the tile launch's gather): the address checkpoints behind everything else of a
job's part against addrs_model -- every kind, frames and packets on and off, the sizes at which the table gains a place and the tiles end,
at tiles of 1 to 256 words, a stream with a bail, addresses with a jump that no 16-bit step could make -- with every piece in front byte
for byte what the same call writes without addrs; and the pipelined executor with addrs on against the executor with it off."""
import ctypes
import functools
import os

import numpy as np
import pytest

import addrs_model as AM
import bitscan_model as M
from conftest import GOLDEN, read_wav_pcm16, tuned
from pymodem_amd._native import ScanJob, check, lib, scan_addr_bytes, scan_part_bytes

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 127, 128, 2047, 2048, 2049, 4096, 70000]
FORMS = [(-1, 0, 0), (0, 0, 0), (0, 1, 0), (1, 0, 0), (1, 0, 1)]          # (kind, frames, packets)
FIRST = (1 << 40) + 3


def _ctx():
    import pymodem_amd
    return pymodem_amd.Context.default()


@functools.lru_cache(maxsize=None)
def _jobs():
    """64 mixed jobs: (slicer bytes, kind, frames, packets, addresses): every size in every form, a stream with a bail, addresses with a jump
    of 2^20 between neighbouring bytes, and two more of odd sizes.  Made once, never changed."""
    rng = np.random.default_rng(64)
    jobs = []

    def addr_of(n, k):
        steps = rng.integers(0, 65536, n).astype(np.int64)
        return FIRST + 1000 * k + np.cumsum(steps) - (steps[0] if n else 0)
    for n in SIZES:
        for kind, frames, packets in FORMS:
            jobs.append((rng.integers(0, 256, n, dtype=np.uint8), kind, frames, packets, addr_of(n, len(jobs))))
    bail = np.bitwise_not(np.ascontiguousarray(M.ax25_streams()["bail_after_a_flag"], dtype=np.uint8))     # (the identity polynomial, inverted)
    jobs.append((bail, 0, 1, 0, addr_of(len(bail), 60)))
    jump = addr_of(3000, 61)
    jump[1500:] += 1 << 20
    jobs.append((rng.integers(0, 256, 3000, dtype=np.uint8), 1, 0, 1, jump))
    jobs.append((rng.integers(0, 256, 2055, dtype=np.uint8), 0, 0, 0, addr_of(2055, 62)))
    jobs.append((rng.integers(0, 256, 193, dtype=np.uint8), -1, 0, 0, addr_of(193, 63)))
    assert len(jobs) == 64
    return jobs


def run_scan(ctx, jobs, addrs, tile=0):
    """-> each job's part of the block, which starts out as 0xA5 bytes"""
    bufs = [ctx.upload(j[0] if len(j[0]) else np.zeros(8, np.uint8)) for j in jobs]
    abufs = [ctx.upload(j[4] if len(j[4]) else np.zeros(1, np.int64)) for j in jobs] if addrs else []
    arr = (ScanJob * len(jobs))()
    for k, (q, b, j) in enumerate(zip(arr, bufs, jobs)):
        q.d_data, q.n, q.lfsr_poly, q.lfsr_state, q.lfsr_invert, q.codec_kind, q.sync_tol = b.ptr.value, len(j[0]), 0x1, 0, 1, j[1], 1
        q.frames, q.packets, q.il2p_crc = j[2], j[3], 1
        if addrs:
            q.d_addr, q.addrs = abufs[k].ptr.value, 1
    need = sum(scan_part_bytes(j[1], j[2], j[3], len(j[0]), addrs) for j in jobs)
    block = ctx.upload(np.full(need + 64, 0xA5, dtype=np.uint8))
    offs, used = (ctypes.c_int64 * len(jobs))(), ctypes.c_size_t()
    with tuned(ctx, bitscan_tile_words=tile):
        check(lib().pm_stream_scan(ctx.handle, arr, len(jobs), block.ptr, need, offs, ctypes.byref(used)))
    ctx.sync()
    host = block.download()
    assert used.value == need
    assert (host[need:] == 0xA5).all(), "nothing is written behind the batch's part of the block"
    ends = list(offs)[1:] + [need]
    del bufs, abufs
    return [host[a:b].copy() for a, b in zip(offs, ends)], need


@functools.lru_cache(maxsize=None)
def _without(tile):
    return run_scan(_ctx(), _jobs(), 0, tile)


@pytest.mark.parametrize("tile", [1, 3, 17, 64, 255, 256])
def test_checkpoints_equal_the_model_and_the_rest_is_untouched(tile):
    ctx = _ctx()
    jobs = _jobs()
    with_addrs, need1 = run_scan(ctx, jobs, 1, tile)
    without, need0 = _without(tile)
    assert need1 - need0 == sum(scan_addr_bytes(len(j[0])) for j in jobs), "*h_used grows by the tables and nothing else"
    bailed = 0
    for k, (j, a, b) in enumerate(zip(jobs, with_addrs, without)):
        n = len(j[0])
        assert len(a) == len(b) + scan_addr_bytes(n) and len(b) == scan_part_bytes(j[1], j[2], j[3], n), k
        assert np.array_equal(a[:len(b)], b), (k, "every piece in front is what it is without addrs")
        table = a[len(b):].view("<i8")
        assert np.array_equal(table, AM.checkpoints_of_addresses(j[4])), (k, n, j[1:4])
        if k == 60:
            bail_bit = int(a[8:16].view("<i8")[0])
            assert 0 < bail_bit < 8 * n - 64 * 8 * 2, "checkpoints behind the bail are owed too"
            bailed += int((table[(bail_bit >> 3) // 64 + 1:] == AM.checkpoints_of_addresses(j[4])[(bail_bit >> 3) // 64 + 1:]).sum())
        if k == 61:
            assert int(table[24] - table[23]) > 1 << 20, "the job form reads full addresses: a jump is in the table as it is"
    assert bailed >= 1


def test_addrs_without_addresses_is_refused():
    ctx = _ctx()
    data = ctx.upload(np.zeros(64, np.uint8))
    arr = (ScanJob * 1)()
    arr[0].d_data, arr[0].n, arr[0].lfsr_poly, arr[0].codec_kind, arr[0].addrs = data.ptr.value, 64, 1, -1, 1
    offs, used = (ctypes.c_int64 * 1)(), ctypes.c_size_t()
    block = ctx.empty(4096, np.uint8)
    assert lib().pm_stream_scan(ctx.handle, arr, 1, block.ptr, 4096, offs, ctypes.byref(used)) == -2     # PM_ERR_ARG
    arr[0].addrs = 2
    arr[0].d_addr = data.ptr.value
    assert lib().pm_stream_scan(ctx.handle, arr, 1, block.ptr, 4096, offs, ctypes.byref(used)) == -2
    ctx.sync()


# ---- through the pipelined executor ---------------------------------------------------------------------------------------------------
def _through_the_pipe(chains_of, recs, nmax, rate, **switches):
    from pymodem_amd import chain_execute as ce
    ctx = _ctx()
    dev = [ctx.upload(r) for r in recs]
    ctx.sync()
    seen = {}
    for addrs in (True, False):
        pipe = ce.NativePipeline(chains_of(), nmax, rate / 40, ctx=ctx, scan=False, addrs=addrs, **switches)
        out = []
        for t in [pipe.submit(d) for d in dev]:
            table = pipe.table(t)
            out.append((table.rows.tobytes(), [int(c) for c in table.counts], [int(u) for u in table.unique_idx], int(table.CountGood())))
            del table
        pipe.close()
        seen[addrs] = out
    assert seen[True] == seen[False], "packet rows with addrs on are the rows with it off, in every field"
    return sum(sum(o[1]) for o in seen[True])


def test_pipeline_with_frames_and_addrs_on_the_bundled_recording_and_a_synthetic_one(golden, config_lines):
    from pymodem_amd import chain_builder as cb, siggen
    rate, audio = read_wav_pcm16(os.path.join(GOLDEN, "afsk_300_il2pc_noise.wav"))
    lines = config_lines("afsk_300_ax25.json")
    picked = (0, 1, 3, 4)
    recorded = sum(len(golden("wav_chains")[f"afsk_300_ax25__c{c}_pkt_addr"]) for c in picked)      # what the reference found in it
    assert recorded >= 4
    assert _through_the_pipe(lambda: [cb.build_chain(rate, lines[c]) for c in picked], [audio], len(audio), rate, frames=True) == recorded
    lines = config_lines("afsk_1200_ax25_super_opt.json")
    sig = siggen.recording("afsk1200_ax25", 48000, packets=3, seed=41, noise_sigma=700.0, payload_len=(20, 50))[0]
    noise = np.clip(np.random.default_rng(44).standard_normal(len(sig)) * 40000, -32768, 32767).astype(np.int16)
    assert _through_the_pipe(lambda: [cb.build_chain(48000, l) for l in lines], [sig, noise, sig], len(sig), 48000, frames=True) >= 6
    # and with addrs alone: the list route
    assert _through_the_pipe(lambda: [cb.build_chain(48000, l) for l in lines], [sig], len(sig), 48000) >= 3


def test_pipeline_with_packets_and_addrs_on_an_il2p_chain(config_lines):
    from pymodem_amd import chain_builder as cb, siggen
    lines = config_lines("afsk_1200_il2p.json")
    recs = [siggen.recording("afsk1200_il2p", 48000, packets=3, seed=40 + k, noise_sigma=700.0, payload_len=(20, 50))[0] for k in range(2)]
    n = max(len(r) for r in recs)
    assert _through_the_pipe(lambda: [cb.build_chain(48000, l) for l in lines], recs, n, 48000, packets=True) >= 2


def test_the_switch_is_off_unless_asked_for():
    assert _ctx().tuned("pipe_addrs") == 0 or os.environ.get("PM_PIPE_ADDRS") not in (None, "0")
