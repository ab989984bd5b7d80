"""The native executor with finished chains (pm_pipe with the switch pipe_done, NativePipeline(done=True): pm_stream_packets behind
pm_stream_scan, the host stage copies records instead of decoding) against the same executor without it (the second with frames=True), both
with keep_slices: every pm_packet row field for field, correlated_count included, the counts, the unique indices, the correlation table,
and the slices -- bytes, addresses, descrambled bytes.
A condition, so that the test cannot pass by handing everything over: the status of every chain of every recording is computed here by the
host model (tests/stream_packets_model.py: the model's scan part of the chain's descrambled bytes, the rule of its kind, the room) from the
slices of the run WITHOUT the switch, and done_stats() must equal the sums.  The recordings are chosen so that in one of them every AX.25
chain is FINISHED and that a very short one hands its chains over as SHORT; both are asserted.  One case gives a group so little room that
NO_ROOM sets in in the middle of a recording's chains, one goes through the device block and a copy (PM_PIPE_HOST_COPY=1)."""
import collections
import functools

import numpy as np
import pytest

import rows_packets_model as RP
import stream_packets_model as SP
from conftest import noise_i16, tuned

pytestmark = pytest.mark.gpu

CFG = "afsk_1200_ax25_super_opt.json"
RATE = 48000


def _ctx():
    import pymodem_amd
    return pymodem_amd.Context.default()


@functools.lru_cache(maxsize=None)
def _recordings():
    from pymodem_amd import siggen
    a = siggen.recording("afsk1200_ax25", RATE, packets=4, seed=51, noise_sigma=800.0, payload_len=(20, 60))[0]
    b = siggen.recording("afsk1200_ax25", RATE, packets=2, seed=52, noise_sigma=2500.0, payload_len=(10, 40))[0]
    f = siggen.recording("fsk9600_il2p", RATE, packets=4, seed=53, noise_sigma=900.0, payload_len=(20, 80))[0]
    return {"a": a, "b": b, "f": f, "short": noise_i16(3000), "silence": np.zeros(60000, np.int16)}


def _lines(config_lines, mixed):
    return (config_lines("fsk_9600.json") if mixed else []) + config_lines(CFG)


def _run(lines, order, one_by_one=False, **switches):
    """the recordings of `order` through a NativePipeline with keep_slices -> ([per recording: rows, counts, unique_idx, corr, slices], done_stats)"""
    from pymodem_amd import chain_builder as cb, chain_execute as ce
    ctx = _ctx()
    recs = _recordings()
    dev = {k: ctx.upload(recs[k]) for k in set(order)}
    ctx.sync()
    pipe = ce.NativePipeline([cb.build_chain(RATE, l) for l in lines], max(len(recs[k]) for k in order), RATE / 40, ctx=ctx, keep_slices=True, **switches)
    out = []

    def collect(t):
        slices = [pipe.slices(t, c) for c in range(len(lines))]      # (before the table: a recording without rows is released with it)
        table = pipe.table(t)
        out.append((table.rows.copy(), list(table.counts), table.unique_idx.copy(), table._corr.copy(),
                    [(s.data.copy(), np.asarray(s.address).copy(), plain) for s, plain in slices]))
        del table
    if one_by_one:
        for k in order:
            collect(pipe.submit(dev[k]))
    else:
        for t in [pipe.submit(dev[k]) for k in order]:
            collect(t)
    stats = pipe.done_stats()
    pipe.close()
    return out, stats


def _same(got, want, what):
    assert len(got) == len(want)
    for r, (g, w) in enumerate(zip(got, want)):
        assert g[1] == w[1], (what, r, "counts")
        assert g[0].dtype == w[0].dtype and g[0].tobytes() == w[0].tobytes(), (what, r, "rows, every field")
        assert np.array_equal(g[2], w[2]), (what, r, "unique indices")
        assert np.array_equal(g[3][:len(g[0])], w[3][:len(w[0])]), (what, r, "the correlation table")
        for c, (gs, ws) in enumerate(zip(g[4], w[4])):
            assert all(np.array_equal(x, y) for x, y in zip(gs, ws)), (what, r, c, "slices: data, addresses, plain")


def _jobs(lines, reference):
    """per recording its chains as the model's jobs, from the slices of the run without the switch"""
    from pymodem_amd import chain_builder as cb
    chains = [cb.build_chain(RATE, l) for l in lines]
    out = []
    for rec in reference:
        jobs = []
        for ch, (_, addr, plain) in zip(chains, rec[4]):
            codec = ch[4]
            jobs.append(SP.job(int(codec._kind), plain, None, addr, int(codec.sync_tolerance), bool(codec.collect_trailing_crc)))
        out.append(jobs)
    return out


def _expected(lines, reference, room=None):
    """per recording the statuses of its chains by the host model; room: the bytes of records a recording's group gets (None: the rule,
    under which NO_ROOM does not occur)"""
    return [[int(s) for s in SP.model_call(jobs, 10 ** 9 if room is None else room)[1]["status"]] for jobs in _jobs(lines, reference)]


def _stats_of(expected):
    count = collections.Counter(RP.STATUS[s] for rec in expected for s in rec)
    finished = count.pop("FINISHED", 0)
    return {"finished": finished, "handed": sum(count.values()), "status": dict(count)}


@functools.lru_cache(maxsize=None)
def _reference(mixed, order, frames):
    lines = _lines(_config_lines(), mixed)
    return _run(lines, order, frames=frames)[0]


def _config_lines():
    import json
    import os
    from conftest import GOLDEN

    def read(name):
        with open(os.path.join(GOLDEN, "configs", name)) as f:
            return [l for l in (json.loads(s) for s in f if s.strip()) if l.get("object_type") == "demod_chain"]
    return read


ORDER = ("a", "short", "b", "silence", "a", "b", "a", "short", "a", "b")


def test_done_equals_not_done_and_the_finished_chains_went_the_new_way():
    lines = _lines(_config_lines(), False)
    want = _reference(False, ORDER, True)
    got, stats = _run(lines, ORDER, done=True)
    _same(got, want, "afsk")
    _same(_reference(False, ORDER, False), want, "the executor with frames is the executor without")
    expected = _expected(lines, want)
    assert stats == _stats_of(expected), (stats, expected)
    assert all(s == RP.FINISHED for s in expected[0]) and sum(want[0][1]) >= 8, "recording a: every AX.25 chain is finished on the device, with packets"
    assert all(s == RP.SHORT for s in expected[1]), "a very short recording: handed over as SHORT"
    assert stats["finished"] >= 8 * 7 and stats["handed"] >= 16


def test_a_mixed_config_with_il2p_chains():
    lines = _lines(_config_lines(), True)
    order = ("f", "a", "short", "f", "b")
    want = _reference(True, order, True)
    got, stats = _run(lines, order, done=True)
    _same(got, want, "mixed")
    expected = _expected(lines, want)
    assert stats == _stats_of(expected), (stats, expected)
    assert sum(want[0][1][:3]) >= 3, "the IL2P chains decode packets"
    assert stats["finished"] >= 11


def test_room_that_runs_out_in_the_middle_of_a_recording_s_chains():
    lines = _lines(_config_lines(), False)
    order = ("a", "b", "short", "a")
    want = _reference(False, order, True)
    # the room of a group: what the first four chains of recording a come to, so that the fifth is the first without
    room = int(SP.model_call(_jobs(lines, want[:1])[0], 10 ** 9)[1]["first_byte"][4])
    assert room > 0 and room % 8 == 0
    with tuned(_ctx(), pipe_done_room=room):
        got, stats = _run(lines, order, one_by_one=True, done=True)      # (one recording a batch: a group is a recording's eight chains)
    _same(got, want, "little room")
    expected = _expected(lines, want, room)
    assert stats == _stats_of(expected), (stats, expected)
    assert expected[0] == [RP.FINISHED] * 4 + [RP.NO_ROOM] * 4, "NO_ROOM sets in behind chains that had room"
    assert stats["status"].get("NO_ROOM", 0) >= 2


def test_through_the_device_block_and_a_copy(monkeypatch):
    lines = _lines(_config_lines(), False)
    order = ("a", "short", "b")
    want = _reference(False, order, True)
    monkeypatch.setenv("PM_PIPE_HOST_COPY", "1")
    got, stats = _run(lines, order, done=True)
    _same(got, want, "host copy")
    assert stats == _stats_of(_expected(lines, want))


def test_the_switch_is_off_by_default():
    import os
    ctx = _ctx()
    assert ctx.tuned("pipe_done") == 0 or os.environ.get("PM_PIPE_DONE") not in (None, "0")
    assert ctx.tuned("pipe_done_room") == 0 or os.environ.get("PM_PIPE_DONE_ROOM") not in (None, "0")
    lines = _lines(_config_lines(), False)
    _, stats = _run(lines, ("short",), frames=True)
    assert stats == {"finished": 0, "handed": 0, "status": {}}
