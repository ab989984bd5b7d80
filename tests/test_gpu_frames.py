"""pm_stream_scan with pm_scan_job.frames (csrc/pm_bitscan.hip: bitscan_frames_kernel): the frame table and the frame area against the
bit-serial model of frames_model.py -- with one word of a frame's span per trip, where every byte boundary, stuffed zero, run end and flag
straddles a trip, with three, and with the default, from lists made at the tile sizes of test_gpu_bitscan.py -- and the executor with
frames on against the executor without the scan stage and against the oracle."""
import functools

import ctypes

import numpy as np
import pytest

import bitscan_model as M
import frames_model as FM
from conftest import tuned
from oracle import oracle as O
from pymodem_amd._native import SCAN_HEAD, ScanJob, check, lib, scan_frame_area_bytes, scan_frame_table_bytes, scan_list_bytes

pytestmark = pytest.mark.gpu
TILE_BYTES = 256 * 8


def _ctx():
    import pymodem_amd
    return pymodem_amd.Context.default()


def _need(job):
    n = len(job[0])
    return SCAN_HEAD + scan_list_bytes(job[4], n) + (n + 7) // 8 * 8 + (scan_frame_table_bytes(n) + scan_frame_area_bytes(n) if job[6] else 0)


def run_scan(ctx, jobs, tile=0, words=0, short_by=0):
    """jobs: [(slicer bytes, poly, register, invert, kind, tol, frames)] -> each job's part of the block (or (status, used, need) with
    short_by).  The block starts out as 0xA5 bytes: what the launches do not write shows."""
    if len(jobs) > 64:                                        # a batch holds 64 jobs
        assert not short_by
        return run_scan(ctx, jobs[:64], tile, words) + run_scan(ctx, jobs[64:], tile, words)
    bufs = [ctx.upload(j[0] if len(j[0]) else np.zeros(8, np.uint8)) for j in jobs]
    arr = (ScanJob * len(jobs))()
    for q, b, j in zip(arr, bufs, jobs):
        q.d_data, q.n, q.lfsr_poly, q.lfsr_state, q.lfsr_invert, q.codec_kind, q.sync_tol, q.frames = b.ptr.value, len(j[0]), j[1], j[2], int(j[3]), j[4], j[5], int(j[6])
    need = sum(_need(j) for j in jobs)
    block = ctx.upload(np.full(need + 8, 0xA5, dtype=np.uint8))
    offs, used = (ctypes.c_int64 * len(jobs))(), ctypes.c_size_t()
    with tuned(ctx, bitscan_tile_words=tile, bitscan_frame_words=words):
        rc = lib().pm_stream_scan(ctx.handle, arr, len(jobs), block.ptr, need - short_by, offs, ctypes.byref(used))
    if short_by:
        return rc, used.value, need
    check(rc)
    assert used.value == need, "*h_used is what the batch needs, frames included"
    ctx.sync()
    host = block.download()
    assert (host[need:] == 0xA5).all(), "nothing is written behind the batch's part of the block"
    ends = list(offs)[1:] + [need]
    del bufs
    return [host[a:b].copy() for a, b in zip(offs, ends)]


def _scrambled(plain):
    """(slicer bytes, poly, register, invert) whose LFSR output is `plain`: the long streams through the identity polynomial inverted, the
    short ones through G3RUH's with its seventeen bits of history"""
    if len(plain) > 4096:
        return np.bitwise_not(plain), 0x1, 0, 1
    bits = M.siggen.lfsr_scramble(np.unpackbits(plain).tolist(), 0x21001, True)
    return np.packbits(np.array(bits, dtype=np.uint8)) if len(bits) else np.zeros(0, np.uint8), 0x21001, 0, 1


@pytest.fixture(scope="module")
def models():
    """name -> (block, covered) of the model, made once"""
    return {name: FM.model_block_frames(plain) for name, plain in FM.all_streams().items()}


def _compare_frames(name, part, plain, model):
    n = len(plain)
    want_block, covered = model
    want = M.split_block(want_block, 0, n)
    got = M.split_block(part, 0, n)
    for field in ("bail_bit", "last_flag", "events", "candidates"):
        assert got[0][field] == want[0][field], (name, field, int(got[0][field]), int(want[0][field]))
    assert np.array_equal(got[1], want[1]), (name, "list")
    assert np.array_equal(got[2], want[2]), (name, "bytes")
    got_table, got_area = FM.split_frames(part, n)
    want_table, want_area = FM.split_frames(want_block, n)
    assert got_table.tolist() == want_table.tolist(), (name, "frame table")
    assert np.array_equal(got_area[covered], want_area[covered]), (name, "frame area")
    assert (got_area[~covered] == 0xA5).all(), (name, "bytes that no frame covers are not written")
    at = SCAN_HEAD + scan_list_bytes(0, n) + (n + 7) // 8 * 8
    assert (part[at + 8 * len(got_table):at + scan_frame_table_bytes(n)] == 0xA5).all(), (name, "places past `events` are not written")


@functools.lru_cache(maxsize=None)
def _jobs():
    """every stream as a job with frames, scrambled once"""
    streams = FM.all_streams()
    return [_scrambled(streams[k]) + (0, 0, 1) for k in sorted(streams)]


# the frames launch does not read tiles, only the list it is given depends on them: every trip length at the smallest tile and at the
# default, the default trip at the tile sizes in between
@pytest.mark.parametrize("tile,words", [(t, w) for t in (1, 0) for w in (1, 3, 0)] + [(t, 0) for t in (2, 3, 17, 64, 125, 126, 255)])
def test_frames_equal_the_model(models, tile, words):
    ctx = _ctx()
    streams = FM.all_streams()
    names = sorted(streams)
    jobs = _jobs()
    with_frames = run_scan(ctx, jobs, tile, words)
    without = run_scan(ctx, [j[:6] + (0,) for j in jobs], tile, words)
    frames = 0
    for name, part, bare in zip(names, with_frames, without):
        _compare_frames(name, part, streams[name], models[name])
        assert np.array_equal(part[:len(bare)], bare), (name, "what exists without frames is the same with them")
        frames += int((FM.split_frames(part, len(streams[name]))[0]["len"] > 0).sum())
    assert frames >= 1193


def test_a_mixed_batch_of_forty_streams_and_a_block_too_small():
    ctx = _ctx()
    rng = np.random.default_rng(34)
    lengths = [int(x) for x in rng.integers(1, 6000, 40)]
    lengths[7] = lengths[36] = 0
    lengths[8], lengths[12], lengths[16] = TILE_BYTES - 8, TILE_BYTES, TILE_BYTES + 8
    kinds = [(0, 1, -1, 0)[k % 4] for k in range(40)]
    plains = []
    for k, n in enumerate(lengths):
        if kinds[k] == 0 and n >= 600:                           # frames among the noise, so that the areas hold something
            bits = M._rand_bits(rng, 8 * n, (0.5, 0.8, 0.6)[k % 3])
            for at in range(200, 8 * n - 3000, 2900):
                frame = M.siggen.ax25_hdlc_bits(M._frame(20 + (at + k) % 90, at + k), pre_flags=2)
                bits[at:at + len(frame)] = frame
            plains.append(M._pack(bits))
        else:
            plains.append(M._pack(M._rand_bits(rng, 8 * n, (0.5, 0.8, 0.6)[k % 3])))
    jobs = [(np.bitwise_not(p), 0x1, 0, 1, kind, 1, kind == 0) for p, kind in zip(plains, kinds)]
    frames = 0
    for k, part in enumerate(run_scan(ctx, jobs)):
        if kinds[k] == 0:
            _compare_frames(k, part, plains[k], FM.model_block_frames(plains[k]))
            frames += int((FM.split_frames(part, len(plains[k]))[0]["len"] > 0).sum())
        else:
            want = M.split_block(M.model_block(plains[k], kinds[k], 1), kinds[k], len(plains[k]))
            got = M.split_block(part, kinds[k], len(plains[k]))
            assert [int(got[0][f]) for f in ("bail_bit", "last_flag", "events", "candidates")] == [int(want[0][f]) for f in ("bail_bit", "last_flag", "events", "candidates")], k
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), k
    assert frames >= 20
    rc, used, need = run_scan(ctx, jobs, short_by=1)
    assert rc == -4 and used == need                          # PM_ERR_CAPACITY, and what the batch needs
    arr = (ScanJob * 1)()
    arr[0].codec_kind, arr[0].frames = 1, 1                   # frames are AX.25's
    offs, used = (ctypes.c_int64 * 1)(), ctypes.c_size_t()
    block = ctx.empty(4096, np.uint8)
    assert lib().pm_stream_scan(ctx.handle, arr, 1, block.ptr, 4096, offs, ctypes.byref(used)) == -2     # PM_ERR_ARG
    ctx.sync()


# ---- through the executor -------------------------------------------------------------------------------------------------------
def _recordings(cfg):
    from pymodem_amd import siggen
    modes = {"afsk_1200_ax25_super_opt.json": ["afsk1200_ax25"] * 3, "fsk_9600.json": ["fsk9600_ax25", "fsk9600_il2p", "fsk9600_ax25"]}[cfg]
    fast = cfg.startswith("fsk")
    recs = [siggen.recording(m, 48000, packets=7 if fast else 3, seed=40 + k, noise_sigma=700.0, payload_len=(20, 50))[0] for k, m in enumerate(modes)]
    n = max(len(r) for r in recs)
    recs.append(np.zeros(n, dtype=np.int16))                                                        # silence
    recs.append(np.clip(np.random.default_rng(44).standard_normal(n) * 40000, -32768, 32767).astype(np.int16))     # clipped noise
    return recs


@pytest.mark.parametrize("cfg", ["afsk_1200_ax25_super_opt.json", "fsk_9600.json"])
def test_executor_with_frames_equals_the_executor_without_the_scan_stage(config_lines, cfg):
    """fsk_9600.json is mixed: its IL2P chains go the scanned route, its AX.25 chain the framed one."""
    from pymodem_amd import chain_builder as cb, chain_execute as ce
    lines = config_lines(cfg)
    recs = _recordings(cfg)
    ctx = _ctx()
    dev = [ctx.upload(r) for r in recs]
    ctx.sync()
    seen = {}
    for frames in (True, False):
        pipe = ce.NativePipeline([cb.build_chain(48000, l) for l in lines], max(len(r) for r in recs), 48000 / 40, ctx=ctx, keep_slices=True, scan=False, frames=frames)
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
        seen[frames] = out
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
            packets += len(want) if k < 3 else 0
    assert packets > 0, "the planted frames are found"
