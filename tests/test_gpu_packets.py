"""pm_stream_scan with pm_scan_job.packets (csrc/pm_bitscan.hip: the candidate list of the emit launch, bitscan_headers_kernel,
bitscan_blocks_kernel): the packet table and the packet area against the bit-serial model of il2p_packets_model.py -- at tiles of 1, 3, 64 and
256 words, which decide the candidate list's ranks, with one wave per job in the blocks launch and with the default, behind a register that is
not zero -- and the executor with packets on against the executor without the scan stage and against the oracle."""
import ctypes
import functools

import numpy as np
import pytest

import bitscan_model as M
import frames_model as FM
import il2p_packets_model as PM
from conftest import tuned
from oracle import oracle as O
from pymodem_amd._native import (SCAN_HEAD, ScanJob, check, lib, scan_frame_area_bytes, scan_frame_table_bytes, scan_list_bytes, scan_packet_area_bytes,
                                 scan_packet_table_bytes)

pytestmark = pytest.mark.gpu
TILE_BYTES = 256 * 8
STD = dict(crc=True, disable_rs=False, min_dist=0)


def _ctx():
    import pymodem_amd
    return pymodem_amd.Context.default()


def _need(job):
    n = len(job[0])
    return (SCAN_HEAD + scan_list_bytes(job[4], n) + (n + 7) // 8 * 8 + (scan_frame_table_bytes(n) + scan_frame_area_bytes(n) if job[6] else 0)
            + (scan_packet_table_bytes(n) + scan_packet_area_bytes(n) if job[7] else 0))


def run_scan(ctx, jobs, tile=0, waves=0, short_by=0):
    """jobs: [(slicer bytes, poly, register, invert, kind, tol, frames, packets, codec options)] -> each job's part of the block (or (status,
    used, need) with short_by).  The block starts out as 0xA5 bytes: what the launches do not write shows."""
    assert len(jobs) <= 64
    bufs = [ctx.upload(j[0] if len(j[0]) else np.zeros(8, np.uint8)) for j in jobs]
    arr = (ScanJob * len(jobs))()
    for q, b, j in zip(arr, bufs, jobs):
        q.d_data, q.n, q.lfsr_poly, q.lfsr_state, q.lfsr_invert, q.codec_kind, q.sync_tol, q.frames = b.ptr.value, len(j[0]), j[1], j[2], int(j[3]), j[4], j[5], int(j[6])
        q.packets, q.il2p_crc, q.il2p_disable_rs, q.il2p_min_dist = int(j[7]), int(j[8]["crc"]), int(j[8]["disable_rs"]), int(j[8]["min_dist"])
    need = sum(_need(j) for j in jobs)
    block = ctx.upload(np.full(need + 8, 0xA5, dtype=np.uint8))
    offs, used = (ctypes.c_int64 * len(jobs))(), ctypes.c_size_t()
    with tuned(ctx, bitscan_tile_words=tile, bitscan_packet_waves=waves):
        rc = lib().pm_stream_scan(ctx.handle, arr, len(jobs), block.ptr, need - short_by, offs, ctypes.byref(used))
    if short_by:
        return rc, used.value, need
    check(rc)
    assert used.value == need, "*h_used is what the batch needs, packets included"
    ctx.sync()
    host = block.download()
    assert (host[need:] == 0xA5).all(), "nothing is written behind the batch's part of the block"
    ends = list(offs)[1:] + [need]
    del bufs
    return [host[a:b].copy() for a, b in zip(offs, ends)]


def host_lfsr(raw, poly, reg, invert):
    out, sr = np.zeros_like(raw), ctypes.c_uint64(reg)
    check(lib().pm_lfsr_unscramble(raw.ctypes.data, len(raw), poly, int(invert), ctypes.byref(sr), out.ctypes.data))
    return out, sr.value


@functools.lru_cache(maxsize=None)
def _jobs():
    """every stream as a job with packets: the long ones through the identity polynomial inverted; the short ones through G3RUH's behind a
    few bytes of noise that the job does not see, so that the register it starts from is not zero"""
    streams = PM.all_streams()
    out = []
    for k, name in enumerate(sorted(streams)):
        plain, tol, o = streams[name]
        if len(plain) > 1500:
            out.append((np.bitwise_not(plain), 0x1, 0, 1, 1, tol, 0, 1, o))
            continue
        a = (1, 7, 8, 9)[k % 4]
        both = np.concatenate([np.random.default_rng(1000 + k).integers(0, 256, a, dtype=np.uint8), plain])
        raw = np.packbits(np.array(M.siggen.lfsr_scramble(np.unpackbits(both).tolist(), 0x21001, True), dtype=np.uint8))
        reg = host_lfsr(raw[:a].copy(), 0x21001, 0, True)[1]
        assert reg != 0
        out.append((raw[a:].copy(), 0x21001, reg, 1, 1, tol, 0, 1, o))
    return out


def _compare_packets(name, part, plain, tol, model):
    n = len(plain)
    want_block, written = model
    want_block = np.asarray(want_block)
    want, got = M.split_block(want_block, 1, n), M.split_block(part, 1, n)
    for field in ("bail_bit", "last_flag", "events", "candidates"):
        assert got[0][field] == want[0][field], (name, field, int(got[0][field]), int(want[0][field]))
    assert np.array_equal(got[1], want[1]), (name, "bitmap")
    assert np.array_equal(got[2], want[2]), (name, "bytes")
    g, w = PM.split_packets(part, n), PM.split_packets(want_block, n)
    assert g[:2] == w[:2], (name, "records, placed", g[:2], w[:2])
    assert g[2].tolist() == w[2].tolist(), (name, "packet table")
    assert len(part) == len(want_block)
    front = SCAN_HEAD + scan_list_bytes(1, n) + (n + 7) // 8 * 8        # (the record's register aside, which the model does not make)
    assert np.array_equal(part[front:][written[front:]], want_block[front:][written[front:]]), (name, "table head, places, covered area")
    assert (part[~written] == 0xA5).all(), (name, "places past `records` and bytes that no DONE record covers are not written")


# tiles of 1, 3, 64 and 256 words decide the candidate list's ranks; the blocks launch's waves share the placed records
@pytest.mark.parametrize("tile,waves", [(1, 0), (3, 1), (64, 0), (0, 1), (0, 0)])
def test_packets_equal_the_model(tile, waves):
    ctx = _ctx()
    streams = PM.all_streams()
    names = sorted(streams)
    jobs = _jobs()
    with_packets = run_scan(ctx, jobs, tile, waves)
    without = run_scan(ctx, [j[:7] + (0, STD) for j in jobs], tile, waves)
    done = 0
    for name, part, bare in zip(names, with_packets, without):
        plain, tol, _ = streams[name]
        _compare_packets(name, part, plain, tol, PM.block_of(name))
        assert np.array_equal(part[:len(bare)], bare), (name, "what exists without packets is the same with them")
        done += int((PM.split_packets(part, len(plain))[2]["status"] == PM.DONE).sum())
    assert done >= 400


def test_a_mixed_batch_of_forty_streams_and_a_block_too_small():
    ctx = _ctx()
    rng = np.random.default_rng(35)
    lengths = [int(x) for x in rng.integers(1, 6000, 40)]
    lengths[7] = lengths[36] = lengths[9] = 0
    lengths[8], lengths[12], lengths[16], lengths[5], lengths[13], lengths[17] = TILE_BYTES - 8, TILE_BYTES, TILE_BYTES + 8, TILE_BYTES - 8, TILE_BYTES, TILE_BYTES + 8
    kinds = [(0, 1, -1, 1)[k % 4] for k in range(40)]
    plains = []
    for k, n in enumerate(lengths):
        bits = M._rand_bits(rng, 8 * n, (0.5, 0.8, 0.6)[k % 3])
        if kinds[k] == 0 and n >= 600:                           # frames and packets among the noise, so that the areas hold something
            for at in range(200, 8 * n - 3000, 2900):
                frame = M.siggen.ax25_hdlc_bits(M._frame(20 + (at + k) % 90, at + k), pre_flags=2)
                bits[at:at + len(frame)] = frame
        if kinds[k] == 1 and n >= 600:
            for at in range(203, 8 * n - 3000, 2901):
                frame = PM._frame(20 + (at + k) % 250, at + k)
                bits[at:at + len(frame)] = frame
        plains.append(M._pack(bits))
    opts = [dict(crc=bool(k & 4), disable_rs=False, min_dist=k % 3) for k in range(40)]
    jobs = [(np.bitwise_not(p), 0x1, 0, 1, kind, 1, kind == 0, kind == 1, o) for p, kind, o in zip(plains, kinds, opts)]
    frames = done = 0
    for k, part in enumerate(run_scan(ctx, jobs)):
        if kinds[k] == 0:
            model = FM.model_block_frames(plains[k])
            got_table, got_area = FM.split_frames(part, len(plains[k]))
            want_table, want_area = FM.split_frames(model[0], len(plains[k]))
            assert got_table.tolist() == want_table.tolist() and np.array_equal(got_area[model[1]], want_area[model[1]]), k
            frames += int((got_table["len"] > 0).sum())
        elif kinds[k] == 1:
            _compare_packets(k, part, plains[k], 1, PM.model_block_packets(plains[k], 1, **opts[k]))
            done += int((PM.split_packets(part, len(plains[k]))[2]["status"] == PM.DONE).sum())
        else:
            want = M.split_block(M.model_block(plains[k], -1, 1), -1, len(plains[k]))
            got = M.split_block(part, -1, len(plains[k]))
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), k
    assert frames >= 10 and done >= 20
    rc, used, need = run_scan(ctx, jobs, short_by=1)
    assert rc == -4 and used == need                          # PM_ERR_CAPACITY, and what the batch needs
    arr = (ScanJob * 1)()
    arr[0].codec_kind, arr[0].packets = 0, 1                  # packets are IL2P's
    offs, used = (ctypes.c_int64 * 1)(), ctypes.c_size_t()
    block = ctx.empty(4096, np.uint8)
    assert lib().pm_stream_scan(ctx.handle, arr, 1, block.ptr, 4096, offs, ctypes.byref(used)) == -2     # PM_ERR_ARG
    arr[0].codec_kind, arr[0].packets, arr[0].frames = 1, 0, 1                                             # and frames stay AX.25's
    assert lib().pm_stream_scan(ctx.handle, arr, 1, block.ptr, 4096, offs, ctypes.byref(used)) == -2
    ctx.sync()


# ---- through the executor -------------------------------------------------------------------------------------------------------
def _recordings(cfg):
    from pymodem_amd import siggen
    modes = {"afsk_1200_il2p.json": ["afsk1200_il2p"] * 3, "fsk_9600.json": ["fsk9600_ax25", "fsk9600_il2p", "fsk9600_ax25"]}[cfg]
    fast = cfg.startswith("fsk")
    recs = [siggen.recording(m, 48000, packets=7 if fast else 3, seed=40 + k, noise_sigma=700.0, payload_len=(20, 50))[0] for k, m in enumerate(modes)]
    recs.append(siggen.recording(modes[1], 48000, packets=4 if fast else 2, seed=47, noise_sigma=700.0, payload_len=(240, 300))[0])     # two-block packets
    n = max(len(r) for r in recs)
    recs.append(np.zeros(n, dtype=np.int16))                                                        # silence
    recs.append(np.clip(np.random.default_rng(44).standard_normal(n) * 40000, -32768, 32767).astype(np.int16))     # clipped noise
    return recs


@pytest.mark.parametrize("cfg", ["afsk_1200_il2p.json", "fsk_9600.json"])
def test_executor_with_packets_equals_the_executor_without_the_scan_stage(config_lines, cfg):
    """fsk_9600.json is mixed: its IL2P chains go the packets route, its AX.25 chain the scanned one."""
    from pymodem_amd import chain_builder as cb, chain_execute as ce
    lines = config_lines(cfg)
    recs = _recordings(cfg)
    ctx = _ctx()
    dev = [ctx.upload(r) for r in recs]
    ctx.sync()
    seen = {}
    for packets in (True, False):
        pipe = ce.NativePipeline([cb.build_chain(48000, l) for l in lines], max(len(r) for r in recs), 48000 / 40, ctx=ctx, keep_slices=True, scan=False, packets=packets)
        tickets = [pipe.submit(d) for d in dev]
        out = []
        for t in tickets:
            kept = [pipe.slices(t, c) for c in range(len(lines))]
            table = pipe.table(t)
            out.append({"rows": table.rows.tobytes(), "counts": [int(c) for c in table.counts], "unique": [int(u) for u in table.unique_idx],
                        "good": int(table.CountGood()), "table": table.rows.copy(),
                        "slices": [(s.data.tobytes(), s.address.tobytes(), p.tobytes()) for s, p in kept]})
            del table
        pipe.close()
        seen[packets] = out
    packets = 0
    for k, (a, b) in enumerate(zip(seen[True], seen[False])):
        for field in ("counts", "unique", "good", "slices", "rows"):
            assert a[field] == b[field], (cfg, k, field)
    for k, rec in enumerate(recs):
        at = 0
        for c, line in enumerate(lines):
            want = O.run_chain(O.build_chain(48000, line), rec, canon=True)["packets"]
            got = seen[True][k]["table"][at:at + seen[True][k]["counts"][c]]
            at += seen[True][k]["counts"][c]
            assert [int(x) for x in got["streamaddress"]] == [int(p.streamaddress) for p in want], (cfg, k, c)
            assert [bytes(r["data"][:r["len"]]) for r in got] == [bytes(bytearray(p.data)) for p in want], (cfg, k, c)
            assert [int(x) for x in got["bytes_corrected"]] == [int(p.BytesCorrected) for p in want], (cfg, k, c)
            packets += len(want) if k < 4 else 0
    assert packets > 0, "the planted packets are found"
