"""pm_rows_scan (csrc/pm_bitscan.hip behind the row table of pm_bitscan_rows.h): the bitstream scan for rows of a sliced engine run.
1. Synthetic rows -- 600 of them, cap 6144, three chains (AX.25 with frames, IL2P with packets, descramble only with another polynomial and
   a register that is not zero), rows 3 .. 599 in one call: every row's scan part is the bit-serial models' block for its bytes
   (bitscan_model, frames_model, il2p_packets_model; the 0xA5 fill still where nothing is to be written) and, byte for byte, what
   pm_stream_scan writes for the same bytes as jobs; the steps in front are the row's; nothing lies behind *h_used.
2. A block one byte short, and the argument checks.
3. process_recordings_device with the scan on the device equals the call with it off: packets, LFSR registers, and with packets on the
   IL2P codecs' walked bytes within the host route's bound.
The models' streams that do not fit a row's 6144 bytes are cut to it (their models are made for the cut): without many_frames' first 6144
bytes the AX.25 rows would hold 66 frames, not the hundred asked for."""
import ctypes
import functools

import numpy as np
import pytest

import bitscan_model as M
import frames_model as FM
import il2p_packets_model as PM
from conftest import tuned
from pymodem_amd import _native as N
from pymodem_amd._native import check, lib

pytestmark = pytest.mark.gpu

CAP, ROWS, ROW0 = 6144, 600, 3
TOL, OPTS = 1, dict(crc=True, disable_rs=False, min_dist=0)
EMPTY = (0, 1, 255, 256, 257, 599)
G3RUH, PREFIX = 0x21001, np.array([0x5A, 0xC3, 0x0F], dtype=np.uint8)     # chain 1: G3RUH's polynomial behind three bytes the rows do not see
POLY2, REG2 = 0x63003, 0x1234567                                           # chain 2: descramble only


def _ctx():
    import pymodem_amd
    return pymodem_amd.Context.default()


def host_lfsr(raw, poly, reg, invert):
    out, sr = np.zeros_like(raw), ctypes.c_uint64(reg)
    check(lib().pm_lfsr_unscramble(raw.ctypes.data, len(raw), poly, int(invert), ctypes.byref(sr), out.ctypes.data))
    return out, sr.value


@functools.lru_cache(maxsize=None)
def _chains():
    """[(poly, register, invert, kind, tol, frames, packets)]"""
    both = np.packbits(np.array(M.siggen.lfsr_scramble(np.unpackbits(PREFIX).tolist(), G3RUH, True), dtype=np.uint8))
    reg1 = host_lfsr(both, G3RUH, 0, True)[1]
    assert reg1 != 0
    return [(0x1, 0, 1, 0, 0, 1, 0), (G3RUH, reg1, 1, 1, TOL, 0, 1), (POLY2, REG2, 0, -1, 0, 0, 0)]


def _raw(kind, plain):
    """the slicer bytes whose descrambled stream is `plain` on the row's chain (kind -1: the bytes are the slicer's, whatever they give)"""
    plain = np.ascontiguousarray(plain, dtype=np.uint8)
    if kind == 0:
        return np.bitwise_not(plain)
    if kind == 1:
        both = np.concatenate([PREFIX, plain])
        return np.packbits(np.array(M.siggen.lfsr_scramble(np.unpackbits(both).tolist(), G3RUH, True), dtype=np.uint8))[len(PREFIX):].copy()
    return plain


@functools.lru_cache(maxsize=None)
def _rows():
    """-> (raw bytes per row, record counts, model per row (block, written mask or None), plain per row): made once, never changed"""
    rng = np.random.default_rng(600)
    named = {0: [np.asarray(p)[:CAP] for _, p in sorted(FM.all_streams().items())],
             1: [np.asarray(v[0])[:CAP] for _, v in sorted(PM.all_streams().items())] + [np.asarray(v[0])[:CAP] for _, v in sorted(M.il2p_streams().items())],
             2: []}
    for kind in (0, 1, 2):                                    # the tile's edges in every kind, and a row that outgrew its room
        for n in (2040, 2048, 2056, CAP):
            named[kind].append(M._pack(M._rand_bits(rng, 8 * n, (0.5, 0.8, 0.6)[kind])))
    plains, counts = [], []
    for row in range(ROWS):
        kind = row % 3
        if row in EMPTY:
            plain = np.zeros(0, np.uint8)
        elif row >= 9 and named[kind]:
            plain = named[kind].pop()
        else:
            plain = rng.integers(0, 256, int(rng.integers(0, 301)), dtype=np.uint8)
        plains.append(np.ascontiguousarray(plain, dtype=np.uint8))
        counts.append(len(plain))
    assert not any(named.values()), "every model stream has its row"
    full = [r for r in range(ROW0, ROWS) if counts[r] == CAP and r % 3 == 1]
    counts[full[0]] = CAP + 100                               # the record counts what the row had no room for: n = cap
    raws, models = [], []
    chains = _chains()
    for row, plain in enumerate(plains):
        kind = row % 3
        raw = _raw(kind, plain)
        if kind == 0:
            model = FM.model_block_frames(plain)
        elif kind == 1:
            model = PM.model_block_packets(plain, TOL, **OPTS)
        else:
            plain = host_lfsr(raw, POLY2, REG2, False)[0]
            plains[row] = plain
            model = (M.model_block(plain, -1), None)
        raws.append(raw)
        models.append(model)
    del chains
    return raws, counts, models, plains


def test_the_rows_hold_what_the_checks_are_worth():
    """no GPU work: at least 100 DONE records in the packets rows and 100 frames in the frames rows, between rows 3 and 599"""
    raws, counts, models, plains = _rows()
    done = frames = 0
    for row in range(ROW0, ROWS):
        n = len(plains[row])
        if row % 3 == 1:
            done += int((PM.split_packets(np.asarray(models[row][0]), n)[2]["status"] == PM.DONE).sum())
        elif row % 3 == 0:
            frames += int((FM.split_frames(np.asarray(models[row][0]), n)[0]["len"] > 0).sum())
    assert done >= 100 and frames >= 100, (done, frames)
    assert all(counts[r] == 0 for r in EMPTY) and {2040, 2048, 2056, CAP} <= {len(p) for p in plains[ROW0:]} and CAP + 100 in counts


def _device_rows(ctx):
    raws, counts, _, _ = _rows()
    data = np.full(ROWS * CAP, 0x3C, dtype=np.uint8)
    for row, raw in enumerate(raws):
        data[row * CAP:row * CAP + len(raw)] = raw
    steps = ((7 * np.arange(ROWS, dtype=np.int64)[:, None] + 3 * np.arange(CAP, dtype=np.int64)[None, :]) & 0xFFFF).astype(np.uint16).ravel()
    recs = np.zeros(ROWS, dtype=N.rowslice_dtype())
    recs["count"] = counts
    return ctx.upload(data), ctx.upload(steps), ctx.upload(recs.view(np.uint8)), steps


def _desc(chains):
    desc = (N.RowsScanChain * len(chains))()
    for d, (poly, reg, invert, kind, tol, frames, packets) in zip(desc, chains):
        d.lfsr_poly, d.lfsr_state, d.lfsr_invert, d.codec_kind, d.sync_tol, d.frames, d.packets = poly, reg, invert, kind, tol, frames, packets
        d.il2p_crc, d.il2p_disable_rs, d.il2p_min_dist = int(OPTS["crc"]), int(OPTS["disable_rs"]), int(OPTS["min_dist"])
    return desc


def _sizes(counts, chains, row0):
    n = [min(c, CAP) for c in counts]
    return [N.rows_scan_steps_bytes(c) + N.scan_part_bytes(chains[(row0 + k) % len(chains)][3], chains[(row0 + k) % len(chains)][5],
                                                          chains[(row0 + k) % len(chains)][6], c) for k, c in enumerate(n)]


def rows_scan(ctx, dev, row0, nrows, chains, counts, tile=0, waves=0, short_by=0, nchains=None):
    """-> (status, used, need, host copy of the block (with 64 bytes of fill behind the need), offsets)"""
    d_data, d_steps, d_recs, _ = dev
    h_counts = (ctypes.c_int64 * nrows)(*[min(c, CAP) for c in counts[:nrows]])
    need = sum(_sizes(counts[:nrows], chains, row0))
    block = ctx.upload(np.full(need + 64, 0xA5, dtype=np.uint8))
    offs, used = (ctypes.c_int64 * nrows)(), ctypes.c_size_t()
    with tuned(ctx, bitscan_tile_words=tile, bitscan_packet_waves=waves):
        rc = lib().pm_rows_scan(ctx.handle, d_recs.ptr, d_data.ptr, d_steps.ptr, CAP, row0, nrows, _desc(chains), len(chains) if nchains is None else nchains,
                                h_counts, block.ptr, need - short_by, offs, ctypes.byref(used))
    if rc != 0:
        return rc, used.value, need, None, None
    ctx.sync()
    return rc, used.value, need, block.download(), list(offs)


@functools.lru_cache(maxsize=None)
def _as_jobs():
    """what pm_stream_scan writes for the rows' bytes as jobs, 64 at a time, into blocks of 0xA5: made once, at the default tunes"""
    import test_gpu_packets as TP
    raws, counts, _, _ = _rows()
    chains = _chains()
    jobs = []
    for row in range(ROW0, ROWS):
        poly, reg, invert, kind, tol, frames, packets = chains[row % 3]
        jobs.append((raws[row], poly, reg, invert, kind, tol, frames, packets, OPTS))
    ctx = _ctx()
    return [part for lo in range(0, len(jobs), 64) for part in TP.run_scan(ctx, jobs[lo:lo + 64])]


# tiles of 1 and 3 words decide every rank of the lists and put thousands of tiles behind the search; one wave or eight share a row's records
@pytest.mark.parametrize("tile,waves", [(1, 1), (1, 0), (3, 1), (3, 0), (0, 1), (0, 0)])
def test_rows_equal_the_models_and_the_job_form(tile, waves):
    import test_gpu_frames as TF
    import test_gpu_packets as TP
    ctx = _ctx()
    raws, counts, models, plains = _rows()
    chains = _chains()
    dev = _device_rows(ctx)
    nrows = ROWS - ROW0
    rc, used, need, host, offs = rows_scan(ctx, dev, ROW0, nrows, chains, counts[ROW0:], tile, waves)
    assert rc == 0 and used == need
    assert (host[need:] == 0xA5).all(), "nothing is written behind *h_used"
    sizes = _sizes(counts[ROW0:], chains, ROW0)
    assert offs == [int(x) for x in np.concatenate(([0], np.cumsum(sizes)))[:-1]]
    as_jobs = _as_jobs()
    for k in range(nrows):
        row, kind = ROW0 + k, (ROW0 + k) % 3
        plain = plains[row]
        n = len(plain)
        assert n == min(counts[row], CAP)
        sw = N.rows_scan_steps_bytes(n)
        assert np.array_equal(host[offs[k]:offs[k] + 2 * n].view(np.uint16), dev[3][row * CAP:row * CAP + n]), (row, "the steps in front are the row's")
        part = host[offs[k] + sw:offs[k] + sizes[k]]
        register = int(part[:8].view("<u8")[0])
        assert register == host_lfsr(raws[row], *chains[kind][:3])[1], (row, "the register behind the stream")
        if kind == 0:
            TF._compare_frames(row, part, plain, models[row])
        elif kind == 1:
            TP._compare_packets(row, part, plain, TOL, models[row])
        else:
            want, got = M.split_block(models[row][0], -1, n), M.split_block(part, -1, n)
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and len(part) == len(models[row][0]), row
            for field in ("bail_bit", "last_flag", "events", "candidates"):
                assert got[0][field] == want[0][field], (row, field)
        assert np.array_equal(part, as_jobs[k]), (row, "byte for byte what pm_stream_scan writes for the same bytes as a job")


def test_capacity_and_arguments():
    ctx = _ctx()
    _, counts, _, _ = _rows()
    chains = _chains()
    dev = _device_rows(ctx)
    rc, used, need, _, _ = rows_scan(ctx, dev, ROW0, ROWS - ROW0, chains, counts[ROW0:], short_by=1)
    assert rc == -4 and used == need                          # PM_ERR_CAPACITY, and what the rows need
    small = [0] * 4097
    assert rows_scan(ctx, dev, 0, 4097, chains, small)[0] == -2                                          # PM_ERR_ARG: more rows than pm_rows_gather takes
    assert rows_scan(ctx, dev, 0, 4096, chains, small[:4096], short_by=1)[0] == -4, "4096 rows are within the limit"
    assert rows_scan(ctx, dev, 0, 8, chains * 22, counts[:8], nchains=65)[0] == -2
    assert rows_scan(ctx, dev, 0, 8, [chains[0], (G3RUH, 0, 1, 1, TOL, 1, 0)], counts[:8])[0] == -2      # frames are AX.25's
    assert rows_scan(ctx, dev, 0, 8, [(0x1, 0, 1, 0, 0, 0, 1), chains[1]], counts[:8])[0] == -2          # packets are IL2P's
    assert rows_scan(ctx, dev, 0, 8, [(0x1, 0, 1, 2, 0, 0, 0)], counts[:8])[0] == -2                     # kinds are -1 .. 1
    ctx.sync()


# ---- through the batch engine's executor ---------------------------------------------------------------------------------------------
def lines_of(cfg):
    import json
    import os
    from conftest import GOLDEN
    with open(os.path.join(GOLDEN, "configs", cfg)) as f:
        return [l for l in (json.loads(s) for s in f if s.strip()) if l.get("object_type") == "demod_chain"]


@functools.lru_cache(maxsize=None)
def _recordings(mode):
    from pymodem_amd import siggen
    recs = [siggen.recording(mode, 48000, packets=2, seed=50 + k, noise_sigma=900.0 + 300.0 * k, payload_len=(20, 40))[0] for k in range(4)]
    n = min(len(r) for r in recs)
    return [r[:n] for r in recs]


def _chain_sets(lines, count):
    from pymodem_amd import chain_builder as cb
    return [[cb.build_chain(48000, line) for line in lines] for _ in range(count)]


def _rows_of(result, as_rows):
    """comparable form of process_recordings_device's result"""
    if as_rows:
        return [[v.tobytes() for v in rec] for rec in result]
    return [[[(int(p.streamaddress), bytes(bytearray(p.data)), int(p.BytesCorrected)) for p in chain] for chain in rec] for rec in result]


@functools.lru_cache(maxsize=None)
def _plainly(mode, cfg, as_rows):
    """the same call with all three switches off: made once per config and result form"""
    from pymodem_amd.loop_batch import process_recordings_device
    recs = _recordings(mode)
    sets = _chain_sets(lines_of(cfg), len(recs))
    stages = {}
    got = process_recordings_device(sets, recs, chunk=8192, rows=as_rows, stages=stages, scan=False, frames=False, packets=False)
    assert stages.get("fused_slicers") and not stages.get("scanned")
    return _rows_of(got, as_rows), [[ch[3].shift_register for ch in cs] for cs in sets], stages["sliced"]


def _walk_bound(stream, chain):
    """the bound tests/test_host_packets.py holds the host route to: 8 walked bytes per used record plus the bytes behind the last one's end"""
    lfsr, codec = chain[3], chain[4]
    plain = host_lfsr(np.ascontiguousarray(stream.data), lfsr.polynomial, 0, bool(lfsr.invert))[0]
    o = dict(crc=bool(codec.collect_trailing_crc), disable_rs=bool(codec.disable_rs), min_dist=int(codec.min_distance))
    block, _ = PM.model_block_packets(plain, int(codec.sync_tolerance), **o)
    _, info = PM.consume(plain, np.asarray(stream.address), int(codec.sync_tolerance), block=block, **o)
    used, n = info["used"], len(plain)
    return 8 * len(used) + (n - (max(E for _, E in used) >> 3) if used else n)


@pytest.mark.parametrize("as_rows", [True, False])
@pytest.mark.parametrize("packets", [False, True])
@pytest.mark.parametrize("mode,cfg", [("qpsk2400_il2p", "qpsk_2400.json"), ("bpsk300_il2p", "bpsk_300.json")])
def test_executor_with_the_scan_on_the_device_equals_the_executor_without(mode, cfg, packets, as_rows):
    from pymodem_amd.loop_batch import process_recordings_device
    recs = _recordings(mode)
    want, registers, sliced = _plainly(mode, cfg, as_rows)
    sets = _chain_sets(lines_of(cfg), len(recs))
    stages = {}
    got = process_recordings_device(sets, recs, chunk=8192, rows=as_rows, stages=stages, scan=True, frames=False, packets=packets)
    assert stages.get("scanned") is True and stages.get("fused_slicers")
    assert _rows_of(got, as_rows) == want
    assert [[ch[3].shift_register for ch in cs] for cs in sets] == registers
    assert sum(len(chain) // (N.packet_dtype().itemsize if as_rows else 1) for rec in want for chain in rec) >= 1, "at least one packet is decoded"
    for k, cs in enumerate(sets):
        for c, ch in enumerate(cs):
            assert np.array_equal(stages["sliced"][k][c].data, sliced[k][c].data), "the diagnosis still shows the slicers' bytes"
            if packets:
                walked = ctypes.c_int64()
                check(lib().pm_codec_walked(ch[4]._handle(), ctypes.byref(walked), None))
                bound = _walk_bound(sliced[k][c], ch)
                assert walked.value <= bound, (cfg, k, c, walked.value, bound)


def test_executor_deferred_on_two_slots():
    from pymodem_amd.loop_batch import process_recordings_device
    mode, cfg = "bpsk300_il2p", "bpsk_300.json"
    recs = _recordings(mode)
    want, registers, _ = _plainly(mode, cfg, True)
    lines = lines_of(cfg)
    sets = [_chain_sets(lines, 2), _chain_sets(lines, 2)]
    rest = [process_recordings_device(sets[b], recs[2 * b:2 * b + 2], chunk=8192, rows=True, slot=b, defer=True, scan=True, packets=True) for b in range(2)]
    got = [x for f in rest for x in f()]
    assert _rows_of(got, True) == want
    assert [[ch[3].shift_register for ch in cs] for b in range(2) for cs in sets[b]] == registers


@pytest.mark.parametrize("as_rows", [True, False])
def test_executor_with_frames_on_ax25_over_a_carrier_loop_modem(as_rows):
    """siggen's bpsk300 modulator takes AX.25 frames as well (mode 'bpsk300_ax25'): the bpsk_300 chain line with its codec swapped for ax25"""
    from pymodem_amd.loop_batch import process_recordings_device
    line = dict(lines_of("bpsk_300.json")[0], codec={"type": "ax25", "options": {}})
    recs = _recordings("bpsk300_ax25")
    seen = []
    for scan, frames in ((False, False), (True, False), (True, True)):
        sets = _chain_sets([line], len(recs))
        stages = {}
        got = process_recordings_device(sets, recs, chunk=8192, rows=as_rows, stages=stages, scan=scan, frames=frames, packets=False)
        assert bool(stages.get("scanned")) == scan
        seen.append((_rows_of(got, as_rows), [[ch[3].shift_register for ch in cs] for cs in sets]))
    assert seen[1] == seen[0] and seen[2] == seen[0]
    assert sum(len(chain) for rec in seen[0][0] for chain in rec) >= 1, "the planted frames are found"


def test_the_switches_default_to_the_context_s_and_used_codecs_go_the_old_way():
    from pymodem_amd.loop_batch import process_recordings_device
    ctx = _ctx()
    assert ctx.tuned("pipe_scan") == 0 and ctx.tuned("pipe_packets") == 0 and ctx.tuned("pipe_frames") == 0, "off unless the environment says otherwise"
    mode, cfg = "bpsk300_il2p", "bpsk_300.json"
    recs = _recordings(mode)
    want, _, _ = _plainly(mode, cfg, True)
    lines = lines_of(cfg)
    stages = {}
    assert _rows_of(process_recordings_device(_chain_sets(lines, len(recs)), recs, chunk=8192, rows=True, stages=stages), True) == want
    assert not stages.get("scanned")
    with tuned(ctx, pipe_packets=1):
        stages = {}
        assert _rows_of(process_recordings_device(_chain_sets(lines, len(recs)), recs, chunk=8192, rows=True, stages=stages), True) == want
        assert stages.get("scanned") is True
    sets = _chain_sets(lines, len(recs))
    sets[1][0][4].decode_pending([])                          # a codec that has been used: the lists are made for a just-created decoder
    stages = {}
    assert _rows_of(process_recordings_device(sets, recs, chunk=8192, rows=True, stages=stages, scan=True), True) == want and not stages.get("scanned")
