"""pm_stream_scan with pm_scan_job.d_carry (csrc/pm_bitscan.hip) and pymodem_amd.scanned.ScannedChain: a stream scanned in pieces.  The
kernels are held to the bit-serial model of scan_carry_model.py on the cuts of test_host_scan_carry.py -- whole parts, carry piece included,
and the carry as the device holds it afterwards -- at the tile sizes where the combine's carry alone decides (1, 3), where the scan over the
lanes does (256) and in between (64; 125 and 126, the largest tile that cannot bail inside itself and the smallest that can).  ScannedChain
is held to the reference's two-segment goldens and to process_chain_device on the same pieces of the bundled recording."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import bitscan_model as M
import scan_carry_model as CM
import test_host_scan_carry as H
from conftest import GOLDEN, read_wav_pcm16, tuned
from pymodem_amd._native import (SCAN_CARRY_BYTES, SCAN_CARRY_LOST, SCAN_CARRY_OK, SCAN_CARRY_START, ScanCarry, ScanJob, check, lib, scan_carry_dtype,
                                 scan_part_bytes)

pytestmark = pytest.mark.gpu
POLY, INVERT = H.POLY, H.INVERT
TILES = [1, 3, 64, 125, 126, 0]                             # 0: the default, 256 words
IL2P_OPTS = dict(crc=True, disable_rs=False, min_dist=0)


def _ctx():
    import pymodem_amd
    return pymodem_amd.Context.default()


def new_carry(ctx, reg=0, ones=0, counted=0):
    buf = ctx.upload(np.full(ctypes.sizeof(ScanCarry), 0xA5, dtype=np.uint8))
    check(lib().pm_scan_carry_set(ctx.handle, buf.ptr, reg, ones, counted))
    return buf


def read_carry(buf):
    c = buf.download().view(scan_carry_dtype())[0]
    return {k: int(c[k]) for k in c.dtype.names}


def enqueue(ctx, jobs, tile=0, expect=0):
    """jobs: dicts of raw, kind, tol, frames, packets (None or the codec's options), addr (None or the n addresses), carry (None or a device
    buffer), reg.  One pm_stream_scan call into a block of 0xA5 bytes; -> (block, offsets, need) without waiting."""
    bufs, need = [], 0
    arr = (ScanJob * len(jobs))()
    for q, j in zip(arr, jobs):
        raw = np.ascontiguousarray(j["raw"], dtype=np.uint8)
        n = len(raw)
        d = ctx.upload(raw if n else np.zeros(8, np.uint8))
        bufs.append(d)
        q.d_data, q.n, q.lfsr_poly, q.lfsr_state, q.lfsr_invert = d.ptr.value, n, j.get("poly", POLY), j.get("reg", 0), j.get("invert", INVERT)
        q.codec_kind, q.sync_tol, q.frames, q.packets = j["kind"], j.get("tol", 0), int(bool(j.get("frames"))), int(j.get("packets") is not None)
        if j.get("packets") is not None:
            q.il2p_crc, q.il2p_disable_rs, q.il2p_min_dist = int(j["packets"]["crc"]), int(j["packets"]["disable_rs"]), j["packets"]["min_dist"]
        if j.get("addr") is not None:
            a = ctx.upload(np.ascontiguousarray(j["addr"], dtype=np.int64) if n else np.zeros(1, np.int64))
            bufs.append(a)
            q.d_addr, q.addrs = a.ptr.value, 1
        if j.get("carry") is not None:
            q.d_carry = j["carry"].ptr.value
        need += scan_part_bytes(j["kind"], q.frames, q.packets, n, q.addrs) + (SCAN_CARRY_BYTES if j.get("carry") is not None else 0)
    block = ctx.upload(np.full(need + 8, 0xA5, dtype=np.uint8))
    offs, used = (ctypes.c_int64 * len(jobs))(), ctypes.c_size_t()
    with tuned(ctx, bitscan_tile_words=tile):
        rc = lib().pm_stream_scan(ctx.handle, arr, len(jobs), block.ptr, need, offs, ctypes.byref(used))
    if expect:
        assert rc == expect
        return None
    check(rc)
    assert used.value == need
    return block, list(offs), need, bufs


def collect(got):
    block, offs, need, bufs = got
    host = block.download()
    assert (host[need:] == 0xA5).all(), "nothing is written behind the batch's part of the block"
    return [host[a:b].copy() for a, b in zip(offs, offs[1:] + [need])]


def run_scan(ctx, jobs, tile=0):
    got = enqueue(ctx, jobs, tile)
    ctx.sync()
    return collect(got)


def same(part, want, written, what):
    assert len(part) == len(want), what
    bad = np.flatnonzero((part != want) & written)
    assert len(bad) == 0, (what, "first difference at byte", int(bad[0]), int(part[bad[0]]), int(want[bad[0]]))
    assert (part[~written] == 0xA5).all(), (what, "what the model does not write is not written")


# ---- the streams and cuts of the host test, as (job options, raw bytes, cuts) ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for name, (plain, at) in sorted(H.ax25_windows().items()):
        raw = CM.scramble(plain, POLY)
        addr = H._addresses(len(plain))
        for cut in range(at - 5, at + 7):
            out.append((f"{name}@{cut}", dict(kind=0, frames=True), raw, addr, [cut]))
    plain, at = H.ax25_windows()["straddle_flag_3"]
    raw, addr = CM.scramble(plain, POLY), H._addresses(len(plain))
    for size in (0, 1, 7, 8, 9, 23, 24):
        out.append((f"size{size}", dict(kind=0, frames=True), raw, addr, [at - 3, at - 3 + size]))
        out.append((f"size{size}_list", dict(kind=0), raw, None, [at - 3, at - 3 + size]))
    plain = H.il2p_stream()
    raw, addr = CM.scramble(plain, POLY), H._addresses(len(plain))
    first = 40 + H.PM.SYNC_AT // 8 - 2
    for cut in range(first, first + 2 + 3 + 15 + 20 + 16 + 4 + 3):
        out.append((f"il2p@{cut}", dict(kind=1, packets=IL2P_OPTS), raw, addr, [cut]))
    for size in (0, 1, 7, 8, 9, 23, 24):
        out.append((f"il2p_size{size}", dict(kind=1, packets=IL2P_OPTS), raw, addr, [first + 4, first + 4 + size]))
        out.append((f"il2p_size{size}_list", dict(kind=1), raw, None, [first + 4, first + 4 + size]))
    plain = np.random.default_rng(77).integers(0, 256, 300, dtype=np.uint8)
    out.append(("descramble_only", dict(kind=-1), CM.scramble(plain, POLY), None, [1, 150]))
    # three pieces, the middle one inside a frame; a run of ones across two cuts; and a late cut in a long stream (several default tiles)
    body = M.siggen.ax25_hdlc_bits(M._frame(120, 5), pre_flags=2, post_flags=2)
    plain = M._pack(M._rand_bits(np.random.default_rng(3), 400) + [0] + body + M._rand_bits(np.random.default_rng(4), 400))
    out.append(("inside_a_frame", dict(kind=0, frames=True), CM.scramble(plain, POLY), H._addresses(len(plain)), [72, 132]))
    plain = M._pack([0, 1, 0] + M.FLAG + [1] * 45 + [0] + M.FLAG + body + [1] * 5 + [0] * 3)
    out.append(("run_of_ones", dict(kind=0, frames=True), CM.scramble(plain, POLY), H._addresses(len(plain)), [2, 3, 5, 6, 7]))
    plain = M.edge_streams()["late_bail"][:2 * 2048 + 900]
    out.append(("three_tiles", dict(kind=0, frames=True), CM.scramble(plain, POLY), H._addresses(len(plain)), [2048 + 3, 2 * 2048 - 1]))
    return out


@functools.lru_cache(maxsize=None)
def models():
    """per case the model's pieces, made once: [(part, written, carry in, carry out, plain)]"""
    out = []
    for name, opts, raw, addr, cuts in cases():
        out.append(CM.model_pieces(raw, cuts, POLY, INVERT, opts["kind"], 0, bool(opts.get("frames")), opts.get("packets"), addr))
    return out


@pytest.mark.parametrize("tile", TILES)
def test_pieces_are_the_model_s_at_every_tile_size(tile):
    ctx = _ctx()
    todo = list(zip(cases(), models()))
    for base in range(0, len(todo), 40):                      # forty streams a call, each with its own carry
        chunk = todo[base:base + 40]
        carries = [new_carry(ctx) for _ in chunk]
        for k in range(max(len(c[0][4]) for c in chunk) + 1):
            jobs, who = [], []
            for (case, pieces), carry in zip(chunk, carries):
                name, opts, raw, addr, cuts = case
                edges = [0] + cuts + [len(raw)]
                if k + 1 >= len(edges):
                    continue
                a, b = edges[k], edges[k + 1]
                jobs.append(dict(opts, raw=raw[a:b], addr=None if addr is None else addr[a:b], carry=carry, reg=0xDEAD))       # (reg: ignored with a carry)
                who.append((name, pieces[k], carry))
            for part, (name, (want, written, cin, cout, _), carry) in zip(run_scan(ctx, jobs, tile), who):
                same(part, want, written, (name, k, tile))
                assert read_carry(carry) == cout, (name, k, tile)


def _host_codec_state(plain_pieces):
    c = H.Codec(0)
    for p in plain_pieces:
        c.decode(p, np.arange(len(p), dtype=np.int64))
    return c.scan_state()


@pytest.mark.parametrize("tile", [3, 126, 0])
@pytest.mark.parametrize("name", ["span8000_flag_calm", "span8001_start_calm", "span7999_flag_calm", "span8000_flag_stuffed"])
def test_a_span_cut_in_front_of_its_bail_then_lost_then_seeded(name, tile):
    ctx = _ctx()
    plain = M.edge_streams()[name]
    tail = M._pack(M.FLAG + M.siggen.ax25_hdlc_bits(M._frame(40, 9), pre_flags=1, post_flags=2) + M._rand_bits(np.random.default_rng(5), 800))
    n0 = len(plain)
    plain = np.concatenate([plain, tail, tail])
    raw = CM.scramble(plain, POLY)
    edges = [0, 500, n0, n0 + len(tail), len(plain)]
    carry = new_carry(ctx)
    model = CM.carry_start()
    states = []
    for k in range(4):
        a, b = edges[k], edges[k + 1]
        if k == 3 and model["state"] == SCAN_CARRY_LOST:       # what ScannedChain does: the carry from the codec's registers
            ones, counted = _host_codec_state([CM.host_lfsr(raw[:a], POLY, 0, INVERT)[0]])
            check(lib().pm_scan_carry_set(ctx.handle, carry.ptr, model["lfsr_state"], ones, counted))
            model = CM.carry_seeded(model["lfsr_state"], ones, counted)
            assert read_carry(carry) == model
        want, written, after, _ = CM.model_piece(raw[a:b], model, POLY, INVERT, 0, 0, True)
        part, = run_scan(ctx, [dict(kind=0, frames=True, raw=raw[a:b], carry=carry)], tile)
        same(part, want, written, (name, k))
        assert read_carry(carry) == after
        states.append(model["state"])
        model = after
    lost = name in ("span8000_flag_calm", "span8001_start_calm")
    assert states == [SCAN_CARRY_START, SCAN_CARRY_OK, SCAN_CARRY_LOST if lost else SCAN_CARRY_OK, SCAN_CARRY_OK]


def test_seeds():
    ctx = _ctx()
    for args in ((0x1234, 0, 0), (0x1FFFF, 3, 17), (7, 7, 0), (7, 9, 0), (1, 0, 5), (0, 2, 7999), (0, 6, 9000), (5, 1, -1)):
        assert read_carry(new_carry(ctx, *args)) == CM.carry_seeded(*args), args


def test_a_start_carry_changes_nothing_but_the_carry_piece_and_uncarried_jobs_stay_what_they_are():
    ctx = _ctx()
    plain, at = H.ax25_windows()["straddle_run7_11"]
    raw, addr = CM.scramble(plain, POLY), H._addresses(len(plain))
    iplain = H.il2p_stream()
    iraw = CM.scramble(iplain, POLY)
    for tile in (3, 0):
        c1, c2 = new_carry(ctx), new_carry(ctx)
        jobs = [dict(kind=0, frames=True, raw=raw, addr=addr, carry=c1), dict(kind=0, frames=True, raw=raw, addr=addr),
                dict(kind=1, packets=IL2P_OPTS, raw=iraw, carry=c2), dict(kind=1, packets=IL2P_OPTS, raw=iraw), dict(kind=0, raw=raw)]
        with_c, without, iwith, iwithout, plain_list = run_scan(ctx, jobs, tile)
        assert np.array_equal(with_c[:-SCAN_CARRY_BYTES], without) and np.array_equal(iwith[:-SCAN_CARRY_BYTES], iwithout)
        assert np.array_equal(with_c[-SCAN_CARRY_BYTES:], CM.carry_piece(CM.carry_start()))
        got = M.split_block(plain_list, 0, len(plain))
        want = M.split_block(M.model_block(plain, 0, 0, int(got[0]["lfsr_state"])), 0, len(plain))
        assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), "model_block, beside carried jobs in one call"
        alone, = run_scan(ctx, [dict(kind=0, raw=raw)], tile)
        assert np.array_equal(alone, plain_list)


def test_two_jobs_of_a_call_may_not_share_a_carry():
    ctx = _ctx()
    raw = np.zeros(64, np.uint8)
    c = new_carry(ctx)
    ctx.sync()
    before = read_carry(c)
    enqueue(ctx, [dict(kind=0, raw=raw, carry=c), dict(kind=1, raw=raw), dict(kind=0, raw=raw, carry=c)], expect=-2)      # PM_ERR_ARG
    buf = ctypes.create_string_buffer(512)
    lib().pm_last_error(buf, 512)
    assert b"bad argument" in buf.value
    ctx.sync()
    assert read_carry(c) == before, "nothing was enqueued"


@pytest.mark.parametrize("tile", [1, 0])
def test_three_pieces_enqueued_back_to_back_equal_three_calls_with_a_wait_after_each(tile):
    ctx = _ctx()
    plain, at = H.ax25_windows()["straddle_bit151_3"]
    raw, addr = CM.scramble(plain, POLY), H._addresses(len(plain))
    edges = [0, at - 100, at + 1, len(plain)]
    pieces = [dict(kind=0, frames=True, raw=raw[a:b], addr=addr[a:b]) for a, b in zip(edges[:-1], edges[1:])]
    waited, c1 = [], new_carry(ctx)
    for p in pieces:
        waited += run_scan(ctx, [dict(p, carry=c1)], tile)
    c2 = new_carry(ctx)
    queued = [enqueue(ctx, [dict(p, carry=c2)], tile) for p in pieces]         # no host wait between the calls
    ctx.sync()
    for k, (got, want) in enumerate(zip(queued, waited)):
        assert np.array_equal(collect(got)[0], want), k
    assert read_carry(c1) == read_carry(c2) and read_carry(c2)["pieces"] == 3 and read_carry(c2)["bytes"] == len(plain)
    model = CM.model_pieces(raw, edges[1:-1], POLY, INVERT, 0, 0, True, None, addr)
    for part, (want, written, _, _, _) in zip(waited, model):
        same(part, want, written, "the model")


# ---- ScannedChain ------------------------------------------------------------------------------------------------------------------
def _pk(pkts):
    return [(int(p.streamaddress), bytes(bytearray(p.data)), int(p.BytesCorrected)) for p in pkts]


@pytest.mark.parametrize("tag", ["afsk_1200", "bpsk_300", "fsk_9600", "qpsk_2400"])
def test_scanned_chain_continues_like_the_reference(golden, config_lines, tag):
    from pymodem_amd import chain_builder as cb
    from pymodem_amd.scanned import ScannedChain
    from test_segments import check_segment
    g = golden("segments")
    cut = json.load(open(os.path.join(GOLDEN, "segments_summary.json")))[tag]["cut"]
    audio = g[tag + "__audio"]
    for switches in (dict(), dict(frames=True, packets=True, addrs=True)):
        chain = cb.build_chain(48000, config_lines(tag + ".json")[0])
        sc = ScannedChain(chain, **switches)
        for k, seg in enumerate((audio[:cut], audio[cut:])):
            st = {}
            pkts = sc.feed(seg, st)
            check_segment(g, f"{tag}__seg{k}", st["sliced"].data, st["sliced"].address, pkts)
        assert sc.pieces == 2 and sc.ordinary == 0 and sc.seeds >= 1


WAV_CUTS = [0, 1001, 4001, 150000, 151207, 610000, 900123, 1254569]    # seven uneven pieces, each longer than the chains' filters


@functools.lru_cache(maxsize=None)
def _wav():
    return read_wav_pcm16(os.path.join(GOLDEN, "afsk_300_il2pc_noise.wav"))


@functools.lru_cache(maxsize=None)
def _wav_reference():
    """process_chain_device on the seven pieces, chain by chain: per piece (slicer bytes, addresses, descrambled bytes, packets)"""
    from pymodem_amd import chain_builder as cb, chain_execute as ce
    rate, audio = _wav()
    assert WAV_CUTS[-1] == len(audio)
    lines = [l for l in (json.loads(s) for s in open(os.path.join(GOLDEN, "configs", "afsk_300.json")) if s.strip()) if l.get("object_type") == "demod_chain"]
    out = []
    for line in lines:
        chain = cb.build_chain(rate, line)
        rows = []
        for a, b in zip(WAV_CUTS[:-1], WAV_CUTS[1:]):
            st = {}
            pkts = ce.process_chain_device(chain, audio[a:b], st)
            rows.append((np.array(st["sliced"].data), np.array(st["sliced"].address), np.array(st["descrambled"].data), _pk(pkts)))
        out.append((line, rows, int(chain[3].shift_register)))
    return out


@pytest.mark.parametrize("frames,packets,addrs", [(0, 0, 0), (1, 1, 0), (0, 0, 1), (1, 1, 1), (1, 0, 1), (0, 1, 0)])
def test_scanned_chain_on_the_bundled_recording_in_seven_pieces(frames, packets, addrs):
    from pymodem_amd import chain_builder as cb
    from pymodem_amd.scanned import ScannedChain
    rate, audio = _wav()
    total = 0
    for line, rows, reg in _wav_reference():
        chain = cb.build_chain(rate, line)
        sc = ScannedChain(chain, frames=frames, packets=packets, addrs=addrs)
        for (a, b), (data, addr, plain, pkts) in zip(zip(WAV_CUTS[:-1], WAV_CUTS[1:]), rows):
            st = {}
            got = sc.feed(audio[a:b], st)
            assert np.array_equal(st["sliced"].data, data) and np.array_equal(st["sliced"].address, addr), (line["object_name"], a)
            assert np.array_equal(st["descrambled"].data, plain), (line["object_name"], a)
            assert _pk(got) == pkts, (line["object_name"], a)
            total += len(pkts)
        assert int(chain[3].shift_register) == reg
    assert total >= 50


def test_a_chain_fed_the_ordinary_way_continues_scanned_and_back():
    from pymodem_amd import chain_builder as cb, chain_execute as ce
    from pymodem_amd.scanned import ScannedChain
    rate, audio = _wav()
    for line, rows, reg in _wav_reference():
        chain = cb.build_chain(rate, line)
        sc = ScannedChain(chain, frames=True, packets=True, addrs=True)
        for k, ((a, b), (data, addr, plain, pkts)) in enumerate(zip(zip(WAV_CUTS[:-1], WAV_CUTS[1:]), rows)):
            got = ce.process_chain_device(chain, audio[a:b]) if k in (0, 1, 4) else sc.feed(audio[a:b])
            assert _pk(got) == pkts, (line["object_name"], k)
        assert int(chain[3].shift_register) == reg
        assert sc.seeds >= 2, "seeded at its first piece and again behind the piece that went the other way"


def test_a_piece_that_the_host_route_refuses_goes_the_ordinary_way_and_the_next_is_seeded_again():
    """The carry is moved under the chain's feet -- eight counted bits more than the decoder has -- so that pm_codec_decode_carried refuses
    the next part with the codec untouched: the piece's slicer bytes, already on the host, go through the host's LFSR and the codec's own
    search, nothing is lost, and the piece after is scanned again from a fresh seed."""
    from pymodem_amd import chain_builder as cb
    from pymodem_amd.scanned import ScannedChain
    rate, audio = _wav()
    line, rows, reg = _wav_reference()[0]
    chain = cb.build_chain(rate, line)
    assert chain[4]._kind == 0
    sc = ScannedChain(chain, frames=True, addrs=True)
    for k, ((a, b), (data, addr, plain, pkts)) in enumerate(zip(zip(WAV_CUTS[:-1], WAV_CUTS[1:]), rows)):
        if k == 4:
            ones, counted = ctypes.c_int32(), ctypes.c_int64()
            check(lib().pm_codec_scan_state(chain[4]._handle(), ctypes.byref(ones), ctypes.byref(counted)))
            assert counted.value < 7000
            check(lib().pm_scan_carry_set(sc.ctx.handle, sc._carry.ptr, int(chain[3].shift_register), ones.value, counted.value + 8))
        before = sc.ordinary
        st = {}
        got = sc.feed(audio[a:b], st)
        assert sc.ordinary - before == (k == 4), k
        assert np.array_equal(st["sliced"].data, data) and np.array_equal(st["descrambled"].data, plain) and _pk(got) == pkts, k
    assert int(chain[3].shift_register) == reg and sc.seeds == 2
