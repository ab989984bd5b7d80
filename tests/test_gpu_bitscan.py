"""pm_stream_scan (csrc/pm_bitscan.hip): the LFSR's bytes and register against pm_lfsr_unscramble, the AX.25 event lists and IL2P
candidate bitmaps against the bit-serial model of bitscan_model.py -- at the smallest tile, where every flag, run of ones, stuffed zero
and sync word straddles a tile boundary at some bit offset and only the combine's carry decides, at the default, where the scan over the
lanes decides, and at the sizes in between, where both do (125 and 126 words: the largest tile that cannot bail inside itself and the
smallest that can) -- and the executor with the stage on against the executor with it off and against the oracle."""
import ctypes
import functools

import numpy as np
import pytest

import bitscan_model as M
from conftest import tuned
from oracle import oracle as O
from pymodem_amd._native import SCAN_HEAD, ScanJob, check, lib, scan_list_bytes

pytestmark = pytest.mark.gpu
TILE_BYTES = 256 * 8            # the default tile: 256 words


def _ctx():
    import pymodem_amd
    return pymodem_amd.Context.default()


def _need(jobs):
    return sum(SCAN_HEAD + scan_list_bytes(j[4], len(j[0])) + (len(j[0]) + 7) // 8 * 8 for j in jobs)


def run_scan(ctx, jobs, tile=0, short_by=0):
    """jobs: [(slicer bytes, poly, register, invert, kind, tol)] -> each job's part of the block (or (status, used) with short_by)."""
    out = []
    for j0 in range(0, len(jobs), 64):
        part = jobs[j0:j0 + 64]
        bufs = [ctx.upload(j[0] if len(j[0]) else np.zeros(8, np.uint8)) for j in part]
        arr = (ScanJob * len(part))()
        for q, b, j in zip(arr, bufs, part):
            q.d_data, q.n, q.lfsr_poly, q.lfsr_state, q.lfsr_invert, q.codec_kind, q.sync_tol = b.ptr.value, len(j[0]), j[1], j[2], int(j[3]), j[4], j[5]
        need = _need(part)
        block = ctx.empty(need + 8, np.uint8)
        offs, used = (ctypes.c_int64 * len(part))(), ctypes.c_size_t()
        with tuned(ctx, bitscan_tile_words=tile):
            rc = lib().pm_stream_scan(ctx.handle, arr, len(part), block.ptr, need - short_by, offs, ctypes.byref(used))
        if short_by:
            return rc, used.value, need
        check(rc)
        assert used.value == need
        ctx.sync()
        host = block.download()
        ends = list(offs)[1:] + [need]
        out += [host[a:b].copy() for a, b in zip(offs, ends)]
        del bufs
    return out


def host_lfsr(raw, poly, reg, invert):
    plain = np.zeros(max(len(raw), 1), dtype=np.uint8)
    sr = ctypes.c_uint64(reg)
    raw = np.ascontiguousarray(raw)
    check(lib().pm_lfsr_unscramble(raw.ctypes.data, len(raw), poly, int(invert), ctypes.byref(sr), plain.ctypes.data))
    return plain[:len(raw)], sr.value


def test_lfsr_bytes_and_register_equal_the_host_s():
    ctx = _ctx()
    rng = np.random.default_rng(31)
    seeded = int(rng.integers(1, 1 << 62)) | (1 << 63)
    jobs = []
    for poly in (0x1, 0x3, 0x21001, 0x8000000000021001):
        for invert in (0, 1):
            for reg in (0, seeded):
                for n in (0, 1, 7, 8, 9, 63, 64, 65, 4096, 65536, TILE_BYTES - 1, TILE_BYTES, TILE_BYTES + 1):
                    jobs.append((rng.integers(0, 256, n, dtype=np.uint8), poly, reg, invert, -1, 0))
    for job, part in zip(jobs, run_scan(ctx, jobs)):
        raw, poly, reg, invert = job[:4]
        rec, _, plain = M.split_block(part, -1, len(raw))
        want, want_reg = host_lfsr(raw, poly, reg, invert)
        assert np.array_equal(plain, want), (hex(poly), invert, hex(reg), len(raw))
        assert int(rec["lfsr_state"]) == want_reg, (hex(poly), invert, hex(reg), len(raw))
        assert not part[SCAN_HEAD + len(raw):].any(), "the padding is zero"


@pytest.mark.parametrize("tile", [1, 3, 0])
def test_lfsr_register_carries_from_call_to_call(tile):
    ctx = _ctx()
    raw = np.random.default_rng(32).integers(0, 256, 65541, dtype=np.uint8)
    for poly, invert, cut in ((0x21001, 1, 1237), (0x8000000000000003, 0, 5), (0x3, 1, 65536)):
        whole, = run_scan(ctx, [(raw, poly, 0x1234567, invert, -1, 0)], tile)
        first, = run_scan(ctx, [(raw[:cut], poly, 0x1234567, invert, -1, 0)], tile)
        reg = int(M.split_block(first, -1, cut)[0]["lfsr_state"])
        second, = run_scan(ctx, [(raw[cut:].copy(), poly, reg, invert, -1, 0)], tile)
        rec, _, plain = M.split_block(whole, -1, len(raw))
        assert np.array_equal(np.concatenate([M.split_block(first, -1, cut)[2], M.split_block(second, -1, len(raw) - cut)[2]]), plain)
        assert M.split_block(second, -1, len(raw) - cut)[0]["lfsr_state"] == rec["lfsr_state"]
        want, want_reg = host_lfsr(raw, poly, 0x1234567, invert)
        assert np.array_equal(plain, want) and int(rec["lfsr_state"]) == want_reg


def _scrambled(plain, small_poly=0x21001):
    """(slicer bytes, poly, register, invert) whose LFSR output is `plain`: the long streams through the identity polynomial inverted, the
    short ones through G3RUH's with its seventeen bits of history."""
    if len(plain) > 4096:
        return np.bitwise_not(plain), 0x1, 0, 1
    bits = M.siggen.lfsr_scramble(np.unpackbits(plain).tolist(), small_poly, True)
    return np.packbits(np.array(bits, dtype=np.uint8)) if len(bits) else np.zeros(0, np.uint8), small_poly, 0, 1


def _compare(name, part, kind, tol, plain, want_block=None):
    want = M.split_block(M.model_block(plain, kind, tol) if want_block is None else want_block, kind, len(plain))
    got = M.split_block(part, kind, len(plain))
    for field in ("bail_bit", "last_flag", "events", "candidates"):
        assert got[0][field] == want[0][field], (name, field, int(got[0][field]), int(want[0][field]))
    assert np.array_equal(got[1], want[1]), (name, "list")
    assert np.array_equal(got[2], want[2]), (name, "bytes")


@functools.lru_cache(maxsize=None)
def _ax25_jobs():
    """every AX.25 stream as a job, scrambled once"""
    streams = M.ax25_streams()
    return [_scrambled(streams[k]) + (0, 0) for k in sorted(streams)]


@pytest.mark.parametrize("tile", [1, 2, 3, 17, 64, 125, 126, 255, 0])
def test_ax25_events_equal_the_model(tile):
    ctx = _ctx()
    streams = M.ax25_streams()
    names = sorted(streams)
    for name, part in zip(names, run_scan(ctx, _ax25_jobs(), tile)):
        _compare(name, part, 0, 0, streams[name], M.ax25_block(name))


NOISE = (1, 7, 8, 9)            # bytes in front of a stream that leave their mark in the register: less than a word, a word, more


@functools.lru_cache(maxsize=None)
def _seeded():
    """[(name, plain B, B's slicer bytes, register behind A)]: every structured stream B behind 1, 7, 8 and 9 bytes of noise A, A + B
    scrambled through G3RUH's polynomial, the register behind A from the host's descrambler"""
    out = []
    streams = M.ax25_streams()
    for k, name in enumerate(sorted(streams)):
        if name.startswith("random") or name == "dense":
            continue
        for a in NOISE:
            noise = np.random.default_rng(1000 * a + k).integers(0, 256, a, dtype=np.uint8)
            both = np.concatenate([noise, streams[name]])
            raw = np.packbits(np.array(M.siggen.lfsr_scramble(np.unpackbits(both).tolist(), 0x21001, True), dtype=np.uint8))
            plain_a, reg = host_lfsr(raw[:a], 0x21001, 0, True)
            assert np.array_equal(plain_a, noise) and reg != 0
            out.append((f"{name} behind {a}", streams[name], raw[a:].copy(), reg))
    return out


@functools.lru_cache(maxsize=None)
def _seeded_block(k, kind):
    """the model's block for _seeded()[k], made once for both tile sizes: read-only"""
    block = M.model_block(_seeded()[k][1], kind, 2)
    block.flags.writeable = False
    return block


@pytest.mark.parametrize("tile", [1, 0])
@pytest.mark.parametrize("kind", [0, 1])
def test_a_register_that_is_not_zero_reaches_the_marks(kind, tile):
    """The incoming register meets word 0 as the lane's own word and as the word in front of lane 1's."""
    ctx = _ctx()
    cases = _seeded()
    jobs = [(raw, 0x21001, reg, 1, kind, 2) for _, _, raw, reg in cases]
    for k, ((name, plain, raw, reg), part) in enumerate(zip(cases, run_scan(ctx, jobs, tile))):
        _compare(name, part, kind, 2, plain, _seeded_block(k, kind))
        assert int(M.split_block(part, kind, len(plain))[0]["lfsr_state"]) == host_lfsr(raw, 0x21001, reg, True)[1], name


@pytest.mark.parametrize("tile", [1, 0])
def test_il2p_candidates_equal_the_model(tile):
    ctx = _ctx()
    streams = M.il2p_streams()
    names = sorted(streams)
    jobs = [_scrambled(streams[k][0], 0x3) + (1, streams[k][1]) for k in names]
    for name, part in zip(names, run_scan(ctx, jobs, tile)):
        _compare(name, part, 1, streams[name][1], streams[name][0])


@pytest.mark.parametrize("tol", [-1, 24, 33, 100])
def test_il2p_sync_tol_at_its_clamps(tol):
    """pm_stream_scan takes sync_tol into [-1, 33]: below 0 nothing is a candidate, from 24 on every byte behind the fourth is (24 bits
    differ from the sync word in 24 places at most)."""
    ctx = _ctx()
    clamped = max(-1, min(33, tol))
    streams = M.il2p_streams()
    names = ["random", "short5"]
    jobs = [_scrambled(streams[k][0], 0x3) + (1, tol) for k in names]
    for name, part in zip(names, run_scan(ctx, jobs)):
        plain = streams[name][0]
        _compare(name, part, 1, clamped, plain)
        assert int(M.split_block(part, 1, len(plain))[0]["candidates"]) == (0 if tol < 0 else max(0, len(plain) - 4)), name


def test_a_batch_of_forty_streams_and_a_block_too_small():
    ctx = _ctx()
    rng = np.random.default_rng(33)
    lengths = [int(x) for x in rng.integers(1, 6000, 40)]
    lengths[7] = lengths[39] = 0
    lengths[11], lengths[12] = TILE_BYTES, TILE_BYTES + 8
    plains = [M._pack(M._rand_bits(rng, 8 * n, (0.5, 0.8, 0.6)[k % 3])) for k, n in enumerate(lengths)]
    kinds = [(0, 1, -1, 0)[k % 4] for k in range(40)]
    jobs = [(np.bitwise_not(p), 0x1, 0, 1, kind, 1) for p, kind in zip(plains, kinds)]
    for k, part in enumerate(run_scan(ctx, jobs)):
        _compare(k, part, kinds[k], 1, plains[k])
    rc, used, need = run_scan(ctx, jobs, short_by=1)
    assert rc == -4 and used == need                          # PM_ERR_CAPACITY, and what the batch needs
    ctx.sync()


# ---- through the executor -------------------------------------------------------------------------------------------------------
def _recordings(cfg):
    from pymodem_amd import siggen
    modes = {"afsk_1200_ax25_super_opt.json": ["afsk1200_ax25"] * 3, "fsk_9600.json": ["fsk9600_ax25", "fsk9600_il2p", "fsk9600_ax25"],
             "afsk_1200_il2p.json": ["afsk1200_il2p"] * 3}[cfg]
    fast = cfg.startswith("fsk")
    recs = [siggen.recording(m, 48000, packets=7 if fast else 3, seed=40 + k, noise_sigma=700.0, payload_len=(20, 50))[0] for k, m in enumerate(modes)]
    n = max(len(r) for r in recs)
    recs.append(np.zeros(n, dtype=np.int16))                                                        # silence
    recs.append(np.clip(np.random.default_rng(44).standard_normal(n) * 40000, -32768, 32767).astype(np.int16))     # clipped noise
    return recs


@pytest.mark.parametrize("cfg", ["afsk_1200_ax25_super_opt.json", "fsk_9600.json", "afsk_1200_il2p.json"])
def test_executor_with_the_scan_stage_equals_the_executor_without(config_lines, cfg):
    from pymodem_amd import chain_builder as cb, chain_execute as ce
    lines = config_lines(cfg)
    recs = _recordings(cfg)
    ctx = _ctx()
    dev = [ctx.upload(r) for r in recs]
    ctx.sync()
    seen = {}
    for scan in (True, False):
        pipe = ce.NativePipeline([cb.build_chain(48000, l) for l in lines], max(len(r) for r in recs), 48000 / 40, ctx=ctx, keep_slices=True, scan=scan)
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
        seen[scan] = out
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
