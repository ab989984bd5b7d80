"""The marks of a sliced engine run (pm_lbatch_run_sliced_marked, rows_mark_kernel in csrc/pm_slicer.hip, the readers in csrc/pm_loopbatch.hip):
bpsk_300 (one output) and qpsk_2400 with two chains (two outputs, the quadrature slicer), 3 recordings in an engine made for 4, chunks of 2048
outputs, recordings whose nout is below one chunk, an exact multiple of the chunk, and no multiple.
1. The marked run leaves the bytes, steps and records of the unmarked run, byte for byte.
2. Mark t of a row is the number of the row's bytes whose address is <= min(nout, (t + 1) chunk) -- the row slicers' address formula, from the
   finished run's own addresses; marks never decrease; the last one is min(count, cap); host and device copies agree; every flag word is the
   OR of the records' flags.
3. The readers refuse t < 0 and t >= chunks, and everything behind a marked call that failed.
4. With the run complete: a piece at every mark in order and then the final one, through RowPieces.fetch(mark=t) and the carried host route,
   gives the rows that one fetch_scanned of the same run gives -- AX.25 and IL2P chains, frames, packets and addrs on."""
import ctypes

import numpy as np
import pytest

import test_gpu_loopbatch as L
import test_gpu_rows_scan as R
from conftest import noise_i16
from pymodem_amd import _native as N
from pymodem_amd._native import lib

pytestmark = pytest.mark.gpu

CHUNK = 2048
CONFIGS = {"bpsk_300": ("bpsk_300.json", None), "qpsk_2400": ("qpsk_2400.json", [1500.0, 1510.0])}


def _group(which):
    cfg, carriers = CONFIGS[which]
    return L.group_modems(cfg, 48000, carriers, take=1 if carriers is None else None)


def _slicers(group):
    from pymodem_amd import chain_builder as cb
    return [cb.build_chain(48000, line)[2] for line, _ in group]


def _device_copy(ctx, marks, t):
    from pymodem_amd.device import DeviceBuffer
    return DeviceBuffer.borrow(ctx, marks.d_upto(t), marks.rows, np.int64).download()


def _rows_bytes(run):
    """the run's records and, per row, its bytes and steps up to min(count, cap)"""
    recs = run.recs.download(run.rows * ctypes.sizeof(N.RowSliceRec)).view(N.rowslice_dtype()).copy()
    data, steps = run.data.download(run.rows * run.cap), run.steps.download(run.rows * run.cap)
    counts = np.minimum(recs["count"], run.cap)
    return recs, [(data[r * run.cap:r * run.cap + c].copy(), steps[r * run.cap:r * run.cap + c].copy()) for r, c in enumerate(counts)]


@pytest.mark.parametrize("nout", [1500, 3 * CHUNK, 4 * CHUNK + 777])
@pytest.mark.parametrize("which", ["bpsk_300", "qpsk_2400"])
def test_marks_of_a_run_and_the_run_itself(which, nout):
    import pymodem_amd
    from pymodem_amd.loop_batch import LoopBatch
    ctx = pymodem_amd.Context.default()
    group = _group(which)
    eng = LoopBatch([m for _, m in group], recordings=4, ctx=ctx, chunk=CHUNK)
    try:
        n = nout - eng.geometry(0)[0]
        assert eng.geometry(n) == (nout, CHUNK, -(-nout // CHUNK))
        dev = [ctx.upload(noise_i16(n, seed=700 + k, sigma=3000.0 + 1500.0 * k)) for k in range(3)]
        plain = eng.run_sliced(dev, _slicers(group))
        ctx.sync()
        assert plain.ok() and plain.marks is None
        want_recs, want_rows = _rows_bytes(plain)
        addresses = [a.address for a in plain.fetch(0, plain.rows)]
        ctx.sync()
        run = eng.run_sliced(dev, _slicers(group), marks=True)
        marks, chunks = run.marks, run.chunks
        assert chunks == -(-nout // CHUNK) and marks.rows == run.rows == 3 * len(group)
        ctx.sync()
        # 1. the run is the same run
        recs, rows = _rows_bytes(run)
        assert recs.tobytes() == want_recs.tobytes()
        for (d, s), (wd, ws) in zip(rows, want_rows):
            assert np.array_equal(d, wd) and np.array_equal(s, ws)
        # 2. the marks
        assert marks.ready() == chunks - 1
        before = np.zeros(run.rows, dtype=np.int64)
        for t in range(chunks):
            marks.wait(t)
            host = marks.h_upto(t).copy()
            upto = min(nout, (t + 1) * CHUNK)
            assert list(host) == [int(np.count_nonzero(a <= upto)) for a in addresses], (which, nout, t)
            assert (host >= before).all()
            assert np.array_equal(_device_copy(ctx, marks, t), host)
            assert marks.flags(t) == int(np.bitwise_or.reduce(recs["flags"])) == 0
            before = host
        assert np.array_equal(before, np.minimum(recs["count"], run.cap)), "the last mark is the records' min(count, cap)"
        assert before.sum() > 0
        # 3. the readers refuse what no call has recorded
        h, t64, p = marks._h, ctypes.c_int64(), ctypes.c_void_p()
        for t in (-1, chunks, chunks + 5, 1 << 40):
            assert lib().pm_lbatch_marks_wait(h, t, 200) == -2
            assert lib().pm_lbatch_marks_wait_on(h, t, ctx.handle) == -2
            assert lib().pm_lbatch_marks_view(h, t, ctypes.byref(p), None, None) == -2
        with pytest.raises(N.NativeError):
            marks.wait(chunks)
    finally:
        eng.close()


def _raw_marked(eng, handle, dev, group, recordings, cap, run):
    params = (N.SlicerParams * len(group))(*[sl._params() for sl in _slicers(group)])
    ptrs = (ctypes.c_void_p * len(dev))(*[a.ptr.value for a in dev])
    got, chunks = ctypes.c_int64(), ctypes.c_int64(77)
    rc = lib().pm_lbatch_run_sliced_marked(eng._h, ptrs, recordings, dev[0].n, params, len(group), run.data.ptr, run.steps.ptr, cap, run.recs.ptr,
                                           ctypes.byref(got), handle, ctypes.byref(chunks))
    return rc, chunks.value


def test_the_readers_refuse_everything_behind_a_failed_call():
    import pymodem_amd
    from pymodem_amd.loop_batch import LoopBatch
    ctx = pymodem_amd.Context.default()
    group = _group("bpsk_300")
    eng = LoopBatch([m for _, m in group], recordings=4, ctx=ctx, chunk=CHUNK)
    try:
        n = 3 * CHUNK + 5 - eng.geometry(0)[0]
        dev = [ctx.upload(noise_i16(n, seed=40 + k, sigma=4000.0)) for k in range(3)]
        run = eng.run_sliced(dev, _slicers(group), marks=True)
        ctx.sync()
        marks, handle = run.marks, run.marks._h
        assert run.chunks == 4 and marks.ready() == 3
        latest = ctypes.c_int64()

        def refused_everywhere():
            assert lib().pm_lbatch_marks_ready(handle, ctypes.byref(latest)) == 0 and latest.value == -1
            for t in range(-1, 5):
                assert lib().pm_lbatch_marks_wait(handle, t, 200) == -2
                assert lib().pm_lbatch_marks_wait_on(handle, t, ctx.handle) == -2
                assert lib().pm_lbatch_marks_view(handle, t, None, None, None) == -2
        # five recordings for an engine made for four; a room that is no multiple of 8: PM_ERR_ARG, nothing recorded, nothing to wait for
        assert _raw_marked(eng, handle, dev + dev[:2], group, 5, run.cap, run) == (-2, 0)
        refused_everywhere()
        assert _raw_marked(eng, handle, dev, group, 3, run.cap + 4, run) == (-2, 0)
        refused_everywhere()
        # a good call makes them answer again
        assert _raw_marked(eng, handle, dev, group, 3, run.cap, run) == (0, 4)
        ctx.sync()
        assert lib().pm_lbatch_marks_ready(handle, ctypes.byref(latest)) == 0 and latest.value == 3
        assert lib().pm_lbatch_marks_wait(handle, 3, 200) == 0 and lib().pm_lbatch_marks_wait(handle, 4, 200) == -2
        # marks made for fewer chunks than the run has: PM_ERR_CAPACITY, and that object has nothing to read either
        small = ctypes.c_void_p()
        assert lib().pm_lbatch_marks_create(eng._h, 3, ctypes.byref(small)) == 0
        try:
            assert _raw_marked(eng, small, dev, group, 3, run.cap, run) == (-4, 0)
            assert lib().pm_lbatch_marks_wait(small, 0, 200) == -2
            assert lib().pm_lbatch_marks_ready(small, ctypes.byref(latest)) == 0 and latest.value == -1
        finally:
            assert lib().pm_lbatch_marks_destroy(small) == 0
        assert lib().pm_lbatch_marks_create(eng._h, 0, ctypes.byref(small)) == -2
        ctx.sync()
    finally:
        eng.close()


def _lines(which):
    if which == "qpsk_il2p":
        return R.lines_of("qpsk_2400.json")[:2], "qpsk2400_il2p"
    lines = R.lines_of("bpsk_300.json")[:1]
    return (lines, "bpsk300_il2p") if which == "bpsk_il2p" else ([dict(lines[0], codec={"type": "ax25", "options": {}})], "bpsk300_ax25")


@pytest.mark.parametrize("which,chunk", [("bpsk_ax25", CHUNK), ("bpsk_il2p", CHUNK), ("qpsk_il2p", CHUNK), ("bpsk_il2p", 8192)])
def test_pieces_at_every_mark_then_the_final_one_equal_one_fetch_scanned(which, chunk):
    import pymodem_amd
    from pymodem_amd import chain_execute as ce
    from pymodem_amd.loop_batch import LoopBatch
    ctx = pymodem_amd.Context.default()
    lines, mode = _lines(which)
    recs = R._recordings(mode)[:3]
    nchains = len(lines)
    eng = LoopBatch([ch[1] for ch in R._chain_sets(lines, 1)[0]], recordings=4, ctx=ctx, chunk=chunk)
    try:
        dev = [ctx.upload(a) for a in recs]
        seen = []
        for in_pieces in (False, True):
            sets = R._chain_sets(lines, len(recs))
            run = eng.run_sliced(dev, [ch[2] for ch in sets[0]], marks=True)
            ctx.sync()
            assert run.ok() and run.chunks >= 6
            blocks = [[[] for _ in range(nchains)] for _ in recs]
            if not in_pieces:
                got = run.fetch_scanned(0, run.rows, sets[0], True, True, addrs=True)
                for rec, cs in enumerate(sets):
                    for c, v in enumerate(ce._host_rows_scanned(cs, got[rec * nchains:(rec + 1) * nchains], None, True, True, True)):
                        blocks[rec][c].append(v)
            else:
                taker = run.pieces(sets[0], frames=True, packets=True, addrs=True)
                sizes = set()
                for t in list(range(run.chunks)) + [None]:
                    got = taker.fetch(0, run.rows, None, t is None, mark=t)
                    sizes |= {g[2] for g in got}
                    if t is not None:
                        assert np.array_equal(taker.taken, run.marks.h_upto(t) // 8 * 8), "every piece goes up to its mark, cut at a multiple of 8"
                    for rec, cs in enumerate(sets):
                        views, again, ordinary = ce._host_rows_pieces(cs, got[rec * nchains:(rec + 1) * nchains], None, True, True, True,
                                                                      raw=lambda j, rec=rec: taker.raw(rec * nchains + j))
                        taker.went_ordinary(ordinary)
                        for j, reg, ones, counted in again:
                            taker.seed(rec * nchains + j, reg, ones, counted)
                        for c, v in enumerate(views):
                            blocks[rec][c].append(v)
                assert np.array_equal(taker.taken, np.minimum(run.records()["count"], run.cap))
                assert 8 in sizes and (0 in sizes or not which.startswith("bpsk")), "empty pieces and single cuts: where the cutting rule decides"
            seen.append(([[np.concatenate(v).tobytes() for v in rec] for rec in blocks], [[ch[3].shift_register for ch in cs] for cs in sets]))
        assert seen[1] == seen[0], "packet rows and LFSR registers"
        assert sum(len(chain) for rec in seen[0][0] for chain in rec) >= N.packet_dtype().itemsize, "at least one packet is decoded"
    finally:
        eng.close()
