"""process_recordings_device(..., beside=k): the host decodes beside the engine's run, taking the rows in pieces at the run's marks
(pymodem_amd/loop_batch.py: _beside, next_mark, RowPieces.fetch(mark=t)).  Against the same call without `beside`: packets or rows, the
slicers' end states, the LFSR registers, and what every chain's codec, LFSR and slicer make of a second recording afterwards.  How many marks
are taken before a run ends is a matter of timing; what is asserted about them is what holds whenever they are taken."""
import functools

import numpy as np
import pytest

import test_gpu_rows_scan as R
from conftest import tuned
from pymodem_amd import _native as N

pytestmark = pytest.mark.gpu

CHUNK = 2048
CASES = {"bpsk_il2p": ("bpsk300_il2p", "bpsk_300.json", None), "bpsk_ax25": ("bpsk300_ax25", "bpsk_300.json", "ax25"),
         "qpsk_il2p": ("qpsk2400_il2p", "qpsk_2400.json", None)}


def _lines(which):
    mode, cfg, codec = CASES[which]
    lines = R.lines_of(cfg)[:2]
    if codec:
        lines = [dict(lines[0], codec={"type": codec, "options": {}})]
    return mode, lines


@functools.lru_cache(maxsize=None)
def _second(mode):
    """a second, short recording for the chains to continue with"""
    from pymodem_amd import siggen
    return siggen.recording(mode, 48000, packets=1, seed=99, noise_sigma=700.0, payload_len=(20, 24))[0]


def _state_of(sets, mode):
    """registers and slicer states, and what every chain makes of a second recording from there (process_chain): its codec, LFSR and slicer
    continue"""
    from pymodem_amd.chain_execute import process_chain
    here = [[(int(ch[3].shift_register), bytes(ch[2]._state)) for ch in cs] for cs in sets]
    after = [[[(int(p.streamaddress), bytes(bytearray(p.data)), int(p.BytesCorrected)) for p in process_chain(ch, _second(mode))] for ch in cs] for cs in sets]
    return here, after


def _call(which, chunk, as_rows, defer, **how):
    from pymodem_amd.loop_batch import process_recordings_device
    mode, lines = _lines(which)
    recs = R._recordings(mode)
    sets = R._chain_sets(lines, len(recs))
    stages = {}
    got = process_recordings_device(sets, recs, chunk=chunk, rows=as_rows, stages=stages, defer=defer, **how)
    if defer:
        got = got()
    return R._rows_of(got, as_rows), _state_of(sets, mode), stages


@functools.lru_cache(maxsize=None)
def _without(which, chunk, as_rows):
    """the same call without `beside`, the scan on: made once per case"""
    got, state, stages = _call(which, chunk, as_rows, False, scan=True, frames=True, packets=True, addrs=True)
    assert stages.get("scanned") is True and stages.get("fused_slicers") and "beside" not in stages
    return got, state, stages["sliced"]


def _check_report(report, k, total_bytes):
    assert set(report) == {"every", "chunks", "marks", "seeds", "ordinary", "bytes_before_end"} and report["every"] == k
    marks, chunks = report["marks"], report["chunks"]
    assert marks == sorted(set(marks)) and all((t + 1) % k == 0 and 0 <= t < chunks for t in marks), "ascending, and due"
    assert 0 <= report["bytes_before_end"] <= total_bytes and report["bytes_before_end"] % 8 == 0
    assert (report["bytes_before_end"] > 0) <= (len(marks) > 0)
    return marks, chunks


@pytest.mark.parametrize("defer", [False, True])
@pytest.mark.parametrize("as_rows", [True, False])
@pytest.mark.parametrize("k", [1, 3])
def test_beside_equals_the_call_without(k, as_rows, defer):
    want, state, sliced = _without("bpsk_il2p", CHUNK, as_rows)
    got, after, stages = _call("bpsk_il2p", CHUNK, as_rows, defer, frames=True, packets=True, addrs=True, beside=k)
    assert stages.get("scanned") is True and stages.get("fused_slicers")
    marks, chunks = _check_report(stages["beside"], k, sum(len(s.data) for rec in sliced for s in rec))
    assert got == want, "packets"
    assert after == state, "LFSR registers, slicer end states, and how every chain continues"
    assert sum(len(chain) // (N.packet_dtype().itemsize if as_rows else 1) for rec in want for chain in rec) >= 1, "at least one packet is decoded"
    for rec, streams in enumerate(sliced):
        for c, s in enumerate(streams):
            assert np.array_equal(stages["sliced"][rec][c].data, s.data), "the diagnosis still shows the slicers' bytes"
    assert chunks >= 6
    if k == 1:
        assert 1 <= len(marks) <= chunks


@pytest.mark.parametrize("which,chunk,k", [("bpsk_ax25", 8192, 3), ("qpsk_il2p", CHUNK, 1), ("bpsk_ax25", CHUNK, 1)])
def test_beside_on_the_other_chains(which, chunk, k):
    want, state, sliced = _without(which, chunk, True)
    got, after, stages = _call(which, chunk, True, False, frames=True, packets=True, addrs=True, beside=k)
    _check_report(stages["beside"], k, sum(len(s.data) for rec in sliced for s in rec))
    assert got == want and after == state


def test_two_slots_as_a_service_runs_them():
    """defer=True on two slots, as a service has it: the remainder of the first batch (its final pieces) runs on a thread of its own while
    this thread drives the marks of the second batch's run.  Neither gets in the other's way: no part is refused, no carry seeded again."""
    import threading
    from pymodem_amd.loop_batch import process_recordings_device
    mode, lines = _lines("bpsk_il2p")
    recs = R._recordings(mode)
    want, _, _ = _without("bpsk_il2p", CHUNK, True)
    sets, stages, got = [R._chain_sets(lines, len(recs)) for _ in range(4)], [{} for _ in range(4)], [None] * 4
    threads = []
    for b in range(4):
        rest = process_recordings_device(sets[b], recs, chunk=CHUNK, rows=True, stages=stages[b], slot=b & 1, defer=True, frames=True, packets=True,
                                         addrs=True, beside=1)
        if threads:
            threads[-1].join()                               # (a slot is used again when its batch is through)
        threads.append(threading.Thread(target=lambda b=b, rest=rest: got.__setitem__(b, rest())))
        threads[-1].start()
    threads[-1].join()
    for b in range(4):
        assert R._rows_of(got[b], True) == want, b
        assert (stages[b]["beside"]["seeds"], stages[b]["beside"]["ordinary"]) == (0, 0), (b, stages[b]["beside"])


def test_the_switch_is_read_by_a_fresh_context_and_tune_is_honoured(monkeypatch):
    import pymodem_amd
    ctx = R._ctx()
    assert ctx.tuned("pipe_beside") == 0, "off unless the environment says otherwise"
    monkeypatch.setenv("PM_PIPE_BESIDE", "4")
    fresh = pymodem_amd.Context(ctx.device)
    try:
        assert fresh.tuned("pipe_beside") == 4
    finally:
        fresh.close()
    monkeypatch.delenv("PM_PIPE_BESIDE")
    want, state, _ = _without("bpsk_il2p", CHUNK, True)
    with tuned(ctx, pipe_beside=3):
        got, after, stages = _call("bpsk_il2p", CHUNK, True, False)          # nothing said: the context's switch, which implies the scan
        assert stages["beside"]["every"] == 3 and stages.get("scanned") is True
        assert got == want and after == state
        got, after, stages = _call("bpsk_il2p", CHUNK, True, False, beside=0)     # said: off
        assert "beside" not in stages and not stages.get("scanned") and got == want
        ctx.tune(pipe_beside=-2)
        with pytest.raises(ValueError):
            _call("bpsk_il2p", CHUNK, True, False)
    assert ctx.tuned("pipe_beside") == 0


def test_beside_is_ignored_where_the_scan_cannot_be_and_says_so():
    from pymodem_amd.loop_batch import process_recordings_device
    mode, lines = _lines("bpsk_il2p")
    recs = R._recordings(mode)
    want, _, _ = _without("bpsk_il2p", CHUNK, True)
    sets = R._chain_sets(lines, len(recs))
    sets[1][0][4].decode_pending([])                          # a codec that has been used: the lists are made for a just-created decoder
    stages = {}
    got = process_recordings_device(sets, recs, chunk=CHUNK, rows=True, stages=stages, beside=2)
    assert R._rows_of(got, True) == want and stages["beside"] is False and not stages.get("scanned")
    sets = R._chain_sets(lines, len(recs))
    for bad in (dict(beside=2, pieces=3), dict(beside=-1), dict(beside=1.5), dict(beside=True), dict(beside="2")):
        with pytest.raises(ValueError):
            process_recordings_device(sets, recs, chunk=CHUNK, rows=True, **bad)
    assert all(ch[4]._h is None and ch[3].shift_register == 0 for cs in sets for ch in cs), "a refused call has touched nothing"


@pytest.mark.parametrize("k", [1, 3])
def test_giving_up_at_a_flagged_mark(k, monkeypatch):
    """Room for 8 bytes a row: a row outgrows it after a few chunks and says so in its flags.  Without `beside` the run is sliced again from
    sign bitmaps; with it the driver has decoded pieces by then -- it puts registers and codecs back and goes the same way."""
    from pymodem_amd import loop_batch as lbm
    want, state, sliced = _without("bpsk_il2p", CHUNK, True)
    real = lbm.LoopBatch.run_sliced
    cap = 8
    monkeypatch.setattr(lbm.LoopBatch, "run_sliced", lambda self, *a, **kw: real(self, *a, **dict(kw, _cap=cap)))
    plain, plain_state, stages = _call("bpsk_il2p", CHUNK, True, False, scan=True, frames=True, packets=True, addrs=True)
    assert not stages.get("fused_slicers") and plain == want and plain_state == state, "the call without beside falls back too"
    got, after, stages = _call("bpsk_il2p", CHUNK, True, False, frames=True, packets=True, addrs=True, beside=k)
    # byte cap + 1 of a row (index cap) is the first that finds no room: its chunk's mark is the first with a flag
    first_flag = min((int(s.address[cap]) - 1) // CHUNK for rec in sliced for s in rec if len(s.data) > cap)
    due = next(t for t in range(first_flag, first_flag + k) if (t + 1) % k == 0)
    assert first_flag >= 3, "pieces have been decoded by then"
    assert stages["beside"] == {"gave_up": due} and not stages.get("fused_slicers")
    assert got == want and after == state, "the result, and the chains continue as if nothing had been fed"
