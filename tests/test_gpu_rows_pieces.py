"""pm_rows_scan_pieces (csrc/pm_bitscan.hip behind the piece table of pm_bitscan_rows.h): the rows of a sliced engine run scanned piece by
piece, a device carry per row.  The synthetic rows are those of test_gpu_rows_scan.py -- 600 rows, cap 6144, three chains, rows 3 .. 599 in
one call, so the prepare launch takes three trips.
1. Every row is taken in six calls whose `upto` arrays make, across the rows, pieces of 0 bytes (upto - taken < 8, upto below taken), of 8
   bytes, of exactly one tile, of one tile plus 8, an empty piece between two full ones, a final piece with n % 8 = 1 .. 7, and empty pieces
   behind the final one.  After each call every row's part is, byte for byte, what pm_stream_scan writes for the same n bytes as a job with
   d_carry that starts from the same carry-in (the job form, which test_gpu_scan_carry.py holds to its model); the 48 bytes of `scan` are
   that job's carry-out; taken and last_addr are the plain sums; the steps in front are the row's, addr_before is the address in front of
   the piece.  The rows of up to 300 bytes and three long ones are also held to rows_pieces_model.py.
2. The same at tiles of 1, 3, 64, 126 and 256 words, frame trips of 1 and 64 words, with addrs on all three chains and off.
3. Nothing lies behind *h_used; a block one byte short; the argument checks; a row whose h_counts entry is wrong keeps part and carry.
4. One call with START carries, d_upto NULL and final = 1 writes, in front of the 40-byte tail, what pm_rows_scan writes for those rows.
Then the executor: process_recordings_device(..., pieces=3) against the call without, and a planted bail through RowPieces."""
import ctypes
import functools

import numpy as np
import pytest

import rows_pieces_model as RM
import scan_carry_model as CM
import test_gpu_rows_scan as R
from conftest import tuned
from pymodem_amd import _native as N
from pymodem_amd._native import check, lib

pytestmark = pytest.mark.gpu

CAP, ROWS, ROW0 = R.CAP, R.ROWS, R.ROW0
NROWS = ROWS - ROW0
BIG = 10 ** 12


def chains_with(addrs):
    """[(poly, register, invert, kind, tol, frames, packets, addrs)]"""
    return [c + (int(addrs),) for c in R._chains()]


def desc_of(chains):
    desc = R._desc([c[:7] for c in chains])
    for d, c in zip(desc, chains):
        d.addrs = c[7]
    return desc


@functools.lru_cache(maxsize=None)
def _host_rows():
    """the rows' steps (the first of a row 0, some 65535), first addresses, and every byte's address: made once"""
    raws, counts, _, _ = R._rows()
    steps = ((7 * np.arange(ROWS, dtype=np.int64)[:, None] + 3 * np.arange(CAP, dtype=np.int64)[None, :]) & 0xFFFF).astype(np.uint16)
    steps[:, 0] = 0
    steps[:, 17] = 65535
    steps[::3, 64] = 65535
    steps[::5, 8] = 65535
    first = 1000 * np.arange(ROWS, dtype=np.int64) + 7
    addr = first[:, None] + np.cumsum(steps.astype(np.int64), axis=1)
    data = np.full((ROWS, CAP), 0x3C, dtype=np.uint8)
    for row, raw in enumerate(raws):
        data[row, :len(raw)] = raw
    return data, steps, first, addr


def _device(ctx):
    data, steps, first, addr = _host_rows()
    recs = np.zeros(ROWS, dtype=N.rowslice_dtype())
    recs["count"] = R._rows()[1]
    recs["first_addr"] = first
    return dict(data=ctx.upload(data.ravel()), steps=ctx.upload(steps.ravel()), recs=ctx.upload(recs.view(np.uint8)), addr=ctx.upload(addr.ravel()))


def schedule(counts, T):
    """Six calls for rows ROW0 ..: [(upto per row or None, final, n per row, taken per row in front of the call)], by the rule of the model."""
    patterns = [[0, 8, T, T + 8], [T, 0, T + 8, 8], [8, T + 8, 0, T], [16, -8, None, None]]
    taken = [0] * NROWS
    calls = []
    for k in range(6):
        final = k >= 4
        upto = None if k == 4 else np.zeros(NROWS, dtype=np.int64)
        ns = []
        for r in range(NROWS):
            if k < 4:
                want = patterns[r % 4][k]
                upto[r] = BIG if want is None else taken[r] + (r % 8 if want == 0 else want if want < 0 else want + r % 8)
            elif k == 5:
                upto[r] = BIG
            ns.append(RM.piece_bytes(counts[ROW0 + r], CAP, None if upto is None else upto[r], taken[r], final))
        calls.append((upto, final, ns, list(taken)))
        taken = [t + n for t, n in zip(taken, ns)]
    assert taken == [min(c, CAP) for c in counts[ROW0:]], "every row has gone whole"
    return calls


def sizes_of(ns, chains):
    return [N.rows_piece_part_bytes(chains[(ROW0 + r) % 3][3], chains[(ROW0 + r) % 3][5], chains[(ROW0 + r) % 3][6], n, chains[(ROW0 + r) % 3][7]) for r, n in enumerate(ns)]


def start_carries(ctx, chains, rows=ROWS):
    d = ctx.upload(np.full(rows * 64, 0xA5, dtype=np.uint8))
    check(lib().pm_rows_carry_start(ctx.handle, d.ptr, 0, rows, desc_of(chains), len(chains)))
    return d


def scan_pieces(ctx, dev, chains, carries, upto, final, ns, row0=ROW0, short_by=0, carries_ptr=None, upto_ptr=None, nrows=None, need=None):
    """One pm_rows_scan_pieces call into a block of 0xA5 -> (status, used, need, host block with 64 bytes of fill behind the need, offsets)"""
    nrows = len(ns) if nrows is None else nrows
    h_counts = (ctypes.c_int64 * nrows)(*ns[:nrows])
    need = sum(sizes_of(ns, chains)) if need is None else need
    block = ctx.upload(np.full(need + 64, 0xA5, dtype=np.uint8))
    d_upto = None if upto is None else ctx.upload(np.ascontiguousarray(upto, dtype=np.int64))
    offs, used = (ctypes.c_int64 * nrows)(), ctypes.c_size_t()
    rc = lib().pm_rows_scan_pieces(ctx.handle, dev["recs"].ptr, dev["data"].ptr, dev["steps"].ptr, CAP, row0, nrows, desc_of(chains), len(chains),
                                   carries.ptr if carries_ptr is None else carries_ptr, (None if d_upto is None else d_upto.ptr) if upto_ptr is None else upto_ptr,
                                   int(final), h_counts, block.ptr, need - short_by, offs, ctypes.byref(used))
    if rc != 0:
        return rc, used.value, need, None, None
    ctx.sync()
    return rc, used.value, need, block.download(), list(offs)


def as_jobs(ctx, dev, chains, job_carries, ns, taken):
    """The same pieces as jobs of pm_stream_scan with d_carry, 64 a call, on the rows' own bytes (a piece with bytes begins at a multiple of 8):
    -> the jobs' parts.  job_carries: the device's pm_scan_carry per row of the call, which the jobs move on."""
    parts, pending = [], []
    for lo in range(0, NROWS, 64):
        rows = range(lo, min(lo + 64, NROWS))
        arr = (N.ScanJob * len(rows))()
        need = []
        for q, r in zip(arr, rows):
            poly, reg, invert, kind, tol, frames, packets, addrs = chains[(ROW0 + r) % 3]
            n, at = ns[r], (ROW0 + r) * CAP + taken[r]
            assert n == 0 or at % 8 == 0
            q.d_data, q.n, q.lfsr_poly, q.lfsr_state, q.lfsr_invert = (dev["data"].ptr.value + at if n else None), n, poly, 0xDEAD, invert
            q.codec_kind, q.sync_tol, q.frames, q.packets = kind, tol, frames, packets
            q.il2p_crc, q.il2p_disable_rs, q.il2p_min_dist = int(R.OPTS["crc"]), int(R.OPTS["disable_rs"]), int(R.OPTS["min_dist"])
            if addrs:
                q.d_addr, q.addrs = dev["addr"].ptr.value + 8 * (at - at % 8), 1      # (n == 0: any aligned pointer)
            q.d_carry = job_carries.ptr.value + 48 * r
            need.append(N.scan_part_bytes(kind, frames, packets, n, addrs) + N.SCAN_CARRY_BYTES)
        block = ctx.upload(np.full(sum(need), 0xA5, dtype=np.uint8))
        offs, used = (ctypes.c_int64 * len(rows))(), ctypes.c_size_t()
        check(lib().pm_stream_scan(ctx.handle, arr, len(rows), block.ptr, sum(need), offs, ctypes.byref(used)))
        assert used.value == sum(need)
        pending.append((block, list(offs), need))
    ctx.sync()
    for block, offs, need in pending:
        host = block.download()
        parts += [host[a:a + b] for a, b in zip(offs, need)]
    return parts


@functools.lru_cache(maxsize=None)
def _model_rows():
    """the rows that are also held to the model: every row of up to 300 bytes, and the longest row of each kind"""
    counts = R._rows()[1]
    rows = [r for r in range(NROWS) if counts[ROW0 + r] <= 300]
    for kind in range(3):
        rows.append(max((r for r in range(NROWS) if (ROW0 + r) % 3 == kind), key=lambda r: min(counts[ROW0 + r], CAP)))
    return sorted(set(rows))


def model_check(r, chain, carry, n, part, what):
    """rows_pieces_model's part for the piece, from the model's own carry -> the carry behind it"""
    data, steps, first, _ = _host_rows()
    poly, reg, invert, kind, tol, frames, packets, addrs = chain
    want, written, after, _, _ = RM.model_row_piece(data[ROW0 + r], steps[ROW0 + r], first[ROW0 + r], carry, n, poly, invert, kind, tol, bool(frames),
                                                    R.OPTS if packets else None, bool(addrs))
    assert len(part) == len(want), what
    bad = np.flatnonzero((part != want) & written)
    assert len(bad) == 0, (what, "first difference from the model at byte", int(bad[0]), int(part[bad[0]]), int(want[bad[0]]))
    assert (part[~written] == 0xA5).all(), (what, "what the model does not write is not written")
    return after


# tile words, frame words, addrs, and whether the model rows are held to the model as well (once with addrs, once without)
CASES = [(1, 64, 1, False), (3, 1, 1, True), (64, 64, 0, False), (126, 1, 1, False), (256, 64, 1, False), (256, 1, 0, True)]


@pytest.mark.parametrize("tile,fw,addrs,model", CASES)
def test_pieces_equal_the_job_form_with_a_carry(tile, fw, addrs, model):
    ctx = R._ctx()
    counts = R._rows()[1]
    data, steps, first, addr = _host_rows()
    chains = chains_with(addrs)
    dev = _device(ctx)
    carries = start_carries(ctx, chains)
    ctx.sync()
    start = carries.download().view(N.rows_carry_dtype())
    for r in range(ROWS):
        assert {k: int(start[r]["scan"][k]) for k in start["scan"].dtype.names} == CM.carry_start(chains[r % 3][1]) and start[r]["taken"] == 0
    job_carries = ctx.upload(np.ascontiguousarray(start["scan"][ROW0:]).view(np.uint8))
    models = {r: RM.rows_carry_start(chains[(ROW0 + r) % 3][1]) for r in _model_rows()} if model else {}
    seen = dict(pieces=0, sizes=set(), final_mod=set(), between=0, behind_final=0)
    history = [[] for _ in range(NROWS)]
    T = 8 * tile
    with tuned(ctx, bitscan_tile_words=tile, bitscan_frame_words=fw):
        for k, (upto, final, ns, taken) in enumerate(schedule(counts, T)):
            rc, used, need, host, offs = scan_pieces(ctx, dev, chains, carries, upto, final, ns)
            assert rc == 0 and used == need
            assert (host[need:] == 0xA5).all(), "nothing is written behind *h_used"
            sizes = sizes_of(ns, chains)
            assert offs == [int(x) for x in np.concatenate(([0], np.cumsum(sizes)))[:-1]]
            jobs = as_jobs(ctx, dev, chains, job_carries, ns, taken)
            after = carries.download().view(N.rows_carry_dtype())
            job_after = job_carries.download().view(N.scan_carry_dtype())
            for r in range(NROWS):
                row, chain, n, a = ROW0 + r, chains[(ROW0 + r) % 3], ns[r], taken[r]
                part = host[offs[r]:offs[r] + sizes[r]]
                got_steps, scan, addr_before = RM.split_piece(part, chain[3], chain[5], chain[6], n, chain[7])
                assert np.array_equal(got_steps, steps[row, a:a + n]), (row, k, "the steps in front are the piece's")
                assert np.array_equal(scan, jobs[r]), (row, k, "byte for byte what pm_stream_scan writes for the same bytes as a job with d_carry")
                assert addr_before == (addr[row, a - 1] if a else first[row]), (row, k)
                assert after[row]["scan"].tobytes() == job_after[r].tobytes(), (row, k, "the carry-out is the job's")
                assert after[row]["taken"] == a + n and (a + n == 0 or after[row]["last_addr"] == addr[row, a + n - 1]), (row, k)
                if r in models:
                    models[r] = model_check(r, chain, models[r], n, part, (row, k))
                    assert {f: int(after[row]["scan"][f]) for f in after["scan"].dtype.names} == models[r]["scan"], (row, k)
                seen["pieces"] += 1
                seen["sizes"].add(n)
                if final and n:
                    seen["final_mod"].add(n % 8)
                history[r].append(n)
            assert (after[:ROW0].tobytes(), after[ROWS:].tobytes()) == (start[:ROW0].tobytes(), start[ROWS:].tobytes()), "rows outside the call keep their carries"
    for h in history:
        seen["between"] += any(h[i] == 0 and h[i - 1] > 0 and h[i + 1] > 0 for i in range(1, 4))
        seen["behind_final"] += h[4] % 8 != 0 and h[5] == 0
    assert seen["pieces"] == 6 * NROWS == 3582, "no row and no piece is left out of the comparison"
    assert {0, 8, T, T + 8} <= seen["sizes"] and seen["final_mod"] >= set(range(1, 8)) and seen["between"] >= 20 and seen["behind_final"] >= 100, seen
    assert not model or len(models) >= 500


def test_capacity_arguments_and_a_wrong_count():
    ctx = R._ctx()
    counts = R._rows()[1]
    chains = chains_with(1)
    dev = _device(ctx)
    calls = schedule(counts, 8 * 256)
    upto, final, ns, taken = calls[0]
    carries = start_carries(ctx, chains)
    ctx.sync()
    before = carries.download()
    rc, used, need, _, _ = scan_pieces(ctx, dev, chains, carries, upto, final, ns, short_by=1)
    assert rc == -4 and used == need                          # PM_ERR_CAPACITY, and what the pieces need
    assert scan_pieces(ctx, dev, chains, carries, upto, final, ns, carries_ptr=ctypes.c_void_p(None))[0] == -2
    assert scan_pieces(ctx, dev, chains, carries, upto, final, ns, carries_ptr=ctypes.c_void_p(carries.ptr.value + 4))[0] == -2
    assert scan_pieces(ctx, dev, chains, carries, upto, final, ns, upto_ptr=ctypes.c_void_p(dev["addr"].ptr.value + 4))[0] == -2
    assert scan_pieces(ctx, dev, chains, carries, None, final, [0] * 4097, row0=0)[0] == -2
    assert scan_pieces(ctx, dev, chains * 22, carries, None, final, [0] * 8, row0=0)[0] == -2     # 66 chains
    assert scan_pieces(ctx, dev, chains, carries, upto, final, [CAP + 8] + ns[1:])[0] == -2
    assert lib().pm_rows_carry_start(ctx.handle, None, 0, 8, desc_of(chains), 3) == -2
    assert lib().pm_rows_carry_start(ctx.handle, ctypes.c_void_p(carries.ptr.value + 4), 0, 8, desc_of(chains), 3) == -2
    ctx.sync()
    assert np.array_equal(carries.download(), before), "a refused call enqueues nothing"
    # the host has a row eight bytes short -- the last row of the call, so that its own part passes what was sized: it is left out
    last = max(r for r in range(NROWS) if ns[r] >= 8)
    assert last >= 512, "three trips of the prepare launch"
    wrong = list(ns[:last + 1])
    wrong[last] -= 8
    table, _ = RM.plain_table([(counts[ROW0 + r], int(upto[r]), 0, wrong[r]) for r in range(last + 1)], [(c[3], c[5], c[6], c[7]) for c in chains], 256, CAP, 0, 1)
    assert [r for r in range(last + 1) if table[r][0] < 0] == [last]      # (the plain loop's chains cycle from row 0; row 3 begins with chain 0 as well)
    rc, used, need, host, offs = scan_pieces(ctx, dev, chains, carries, upto[:last + 1], final, wrong)
    assert rc == 0 and used == need
    after = carries.download().view(N.rows_carry_dtype())
    was = before.view(N.rows_carry_dtype())
    assert (host[offs[last]:] == 0xA5).all(), "no part of a row that is left out is written"
    assert after[ROW0 + last:].tobytes() == was[ROW0 + last:].tobytes(), "a row that is left out keeps its carry"
    for r in range(last):
        assert after[ROW0 + r]["taken"] == ns[r] and after[ROW0 + r]["scan"]["pieces"] == 1, r


@pytest.mark.parametrize("tile,addrs", [(3, 1), (0, 1), (0, 0)])
def test_one_final_piece_from_start_is_pm_rows_scan(tile, addrs):
    ctx = R._ctx()
    counts = R._rows()[1]
    chains = chains_with(addrs)
    dev = _device(ctx)
    carries = start_carries(ctx, chains)
    ns = [min(c, CAP) for c in counts[ROW0:]]
    with tuned(ctx, bitscan_tile_words=tile):
        rc, used, need, host, offs = scan_pieces(ctx, dev, chains, carries, None, 1, ns)
        assert rc == 0 and used == need and (host[need:] == 0xA5).all()
        whole = [s - N.ROWS_PIECE_TAIL_BYTES for s in sizes_of(ns, chains)]
        block = ctx.upload(np.full(sum(whole), 0xA5, dtype=np.uint8))
        woffs, wused = (ctypes.c_int64 * NROWS)(), ctypes.c_size_t()
        check(lib().pm_rows_scan(ctx.handle, dev["recs"].ptr, dev["data"].ptr, dev["steps"].ptr, CAP, ROW0, NROWS, desc_of(chains), 3, (ctypes.c_int64 * NROWS)(*ns),
                                 block.ptr, sum(whole), woffs, ctypes.byref(wused)))
        ctx.sync()
    want = block.download()
    first = _host_rows()[2]
    start = CM.carry_piece(CM.carry_start())
    for r in range(NROWS):
        part = host[offs[r]:offs[r] + whole[r] + N.ROWS_PIECE_TAIL_BYTES]
        assert np.array_equal(part[:whole[r]], want[woffs[r]:woffs[r] + whole[r]]), (ROW0 + r, "what pm_rows_scan writes")
        assert np.array_equal(part[whole[r]:whole[r] + 32], start) and int(part[whole[r] + 32:].view("<i8")[0]) == first[ROW0 + r]
    after = carries.download().view(N.rows_carry_dtype())
    assert [int(t) for t in after["taken"][ROW0:ROWS]] == ns and (after["scan"]["pieces"][ROW0:ROWS] == 1).all()


# ---- through the batch engine's executor ---------------------------------------------------------------------------------------------
def _lines(which):
    lines = R.lines_of("bpsk_300.json")
    return lines if which == "il2p" else [dict(lines[0], codec={"type": "ax25", "options": {}})]


def _no_span_without_a_reset(sliced, sets):
    """the model's walk over every AX.25 chain's descrambled stream: no 8000 bits without a reset, so no piece bails and no carry is LOST"""
    for streams, cs in zip(sliced, sets):
        for stream, ch in zip(streams, cs):
            if ch[4]._kind == 0:
                plain = R.host_lfsr(np.ascontiguousarray(stream.data), ch[3].polynomial, 0, bool(ch[3].invert))[0]
                assert CM.ax25_walk(np.unpackbits(plain).tolist(), CM.carry_start())[1] < 0


@pytest.mark.parametrize("which,mode,as_rows", [("il2p", "bpsk300_il2p", True), ("ax25", "bpsk300_ax25", False), ("ax25", "bpsk300_ax25", True)])
def test_executor_in_three_pieces_equals_the_executor_without(which, mode, as_rows):
    from pymodem_amd.loop_batch import process_recordings_device
    recs = R._recordings(mode)
    lines = _lines(which)
    seen = []
    for pieces in (None, 3):
        sets = R._chain_sets(lines, len(recs))
        stages = {}
        got = process_recordings_device(sets, recs, chunk=8192, rows=as_rows, stages=stages, scan=True, frames=True, packets=True, addrs=True, pieces=pieces)
        assert stages.get("scanned") is True and stages.get("fused_slicers")
        seen.append((R._rows_of(got, as_rows), [[ch[3].shift_register for ch in cs] for cs in sets], [[bytes(ch[2]._state) for ch in cs] for cs in sets]))
        if pieces is None:
            assert "pieces" not in stages
            _no_span_without_a_reset(stages["sliced"], sets)
        else:
            assert stages["pieces"] == {"pieces": 3, "seeds": 0, "ordinary": 0}
    assert seen[1] == seen[0], "packets, LFSR registers and slicer states"
    assert sum(len(chain) // (N.packet_dtype().itemsize if as_rows else 1) for rec in seen[0][0] for chain in rec) >= 1, "at least one packet is decoded"


def test_pieces_are_ignored_where_the_scan_is_off_and_say_so():
    from pymodem_amd.loop_batch import process_recordings_device
    recs = R._recordings("bpsk300_il2p")
    want, registers, _ = R._plainly("bpsk300_il2p", "bpsk_300.json", True)
    sets = R._chain_sets(_lines("il2p"), len(recs))
    stages = {}
    got = process_recordings_device(sets, recs, chunk=8192, rows=True, stages=stages, scan=False, frames=False, packets=False, addrs=False, pieces=4)
    assert R._rows_of(got, True) == want and stages["pieces"] is False and not stages.get("scanned")
    with pytest.raises(ValueError):
        process_recordings_device(sets, recs, chunk=8192, pieces=1)


def planted_bail():
    """-> (descrambled stream, cuts): a span of 8000 bits without a reset whose closing flag -- the bail -- lies in the second piece, then two
    frames; every cut a multiple of 8"""
    import bitscan_model as M
    span = M.edge_streams()["span8000_flag_calm"]
    tail = M._pack(M.FLAG + M.siggen.ax25_hdlc_bits(M._frame(40, 9), pre_flags=1, post_flags=2) + M._rand_bits(np.random.default_rng(5), 800))
    plain = np.concatenate([span, tail, tail])
    return plain, [496, (len(span) + 7) // 8 * 8, (len(span) + len(tail) + 7) // 8 * 8]


def test_a_planted_bail_is_seeded_once_and_the_packets_are_right():
    """A synthetic row through RowPieces directly: the piece that holds the bail hands on LOST, the host decodes it, the row's carry is seeded
    from the codec's registers (taken and last_addr stay), and the pieces behind list again."""
    import test_host_scan_carry as H
    from pymodem_amd import chain_builder as cb, chain_execute as ce
    from pymodem_amd.loop_batch import SlicedRun
    ctx = R._ctx()
    chain = cb.build_chain(48000, _lines("ax25")[0])
    lfsr = chain[3]
    assert lfsr.shift_register == 0
    plain, cuts = planted_bail()
    n = len(plain)
    cap = (n + 64) // 8 * 8
    raw = CM.scramble(plain if lfsr.invert else np.bitwise_not(plain), lfsr.polynomial)
    assert np.array_equal(R.host_lfsr(raw, lfsr.polynomial, 0, bool(lfsr.invert))[0], plain)
    data, steps = np.full(cap, 0x3C, np.uint8), (30 + np.arange(cap) % 11).astype(np.uint16)
    data[:n], steps[0] = raw, 0
    recs = np.zeros(1, dtype=N.rowslice_dtype())
    recs["count"], recs["first_addr"] = n, 12345
    addr = 12345 + np.cumsum(steps[:n].astype(np.int64))
    recs["last_addr"] = addr[-1]
    run = SlicedRun(ctx, ctx.upload(data), ctx.upload(steps), ctx.upload(recs.view(np.uint8)), cap, 1, 0)
    ctx.sync()
    taker = run.pieces([chain], frames=True, addrs=True)
    rows, states = [], []
    for upto in cuts + [None]:
        got = taker.fetch(0, 1, None if upto is None else np.array([upto + 3]), upto is None)
        states.append(int(got[0][3][-32:].view(N.scan_carry_piece_dtype())[0]["state"]))
        views, again, ordinary = ce._host_rows_pieces([chain], got, None, True, False, True, raw=lambda j: taker.raw(j))
        taker.went_ordinary(ordinary)
        for j, reg, ones, counted in again:
            taker.seed(j, reg, ones, counted)
        rows.append(views[0])
    ctx.sync()
    assert (taker.seeds, taker.ordinary) == (1, 0) and states == [N.SCAN_CARRY_START, N.SCAN_CARRY_OK, N.SCAN_CARRY_OK, N.SCAN_CARRY_OK]
    carry = taker.carries.download().view(N.rows_carry_dtype())[0]
    assert carry["taken"] == n and carry["last_addr"] == addr[-1] and carry["scan"]["pieces"] == 2, "two pieces since the seed"
    ref = H.Codec(0)
    want = ref.decode(plain, addr)
    flat = np.concatenate(rows)
    assert len(want) >= 2 and H._rows(flat) == H._rows(want)
    assert int(lfsr.shift_register) == R.host_lfsr(raw, lfsr.polynomial, 0, bool(lfsr.invert))[1]
