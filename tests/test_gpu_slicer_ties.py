"""The slicer walkers (pm_slice_batch, pymodem_amd/csrc/pm_slicer.hip) where the clock lands ON the threshold, where the step forms differ
and where a carried state decides -- against the oracle's C port of the reference slicers (oracle/pm_oracle.c pmo_slice_binary and
pmo_slice_quadrature), bit for bit: data bytes, addresses and every field of the end state.  No tolerance anywhere.

The symbol decision fl(clk + 1.0) >= sps/2 - 0.5 is taken in four ways: the reference's compare (step32), the hand-scheduled clk >= tp
(step32a, four assembly bodies by LM0 / NS0), the event step's clk >= tp behind a run bound, and the scalar loop of a stream's partial last
word, which compares with thr again.  tests/slicer_ties.py makes the inputs: odd integer samples per symbol (an integer threshold: a stream
without crossings ties at every symbol), lock_rate 0.5 (ties between crossings), streams cut so that a tie is the last sample of a call's
partial last word, and start clocks at tp, its neighbours and the limits of pm_event_ok.  pm_slice_batch is driven directly, so that
samples_per_symbol, lock_rate and h_state are the test's own; the form and LM0 / NS0 of every call are read from the [slicer] trace.

Two fields of the reference's state hold more than the slicer objects carry, and are compared through the part that can ever reach an
output: working_byte through its working_bits low bits (the reference keeps shifted-out bits of the byte before), state_register through
its low two bits, the last symbol (the reference keeps the one before it too, which the next symbol shifts out before the demap reads it).
"""
import ctypes
import re

import numpy as np
import pytest

import slicer_ties as T
from conftest import tuned
from oracle import oracle as O

pytestmark = pytest.mark.gpu

QPSK = [3, 1, 2, 0, 2, 3, 0, 1, 1, 0, 3, 2, 0, 2, 1, 3]
_TRACE = re.compile(r"^\[slicer\] (\w+) step \(LM0 (\d), NS0 (\d)\)")


@pytest.fixture(scope="module")
def ctx():
    import pymodem_amd
    if pymodem_amd.lib().pm_device_count() < 1:
        pytest.fail("no GPU visible: -m gpu tests need an MI355X")
    return pymodem_amd.Context.default()


class Case:
    """One slicer over the consecutive pieces of a stream: the state the GPU leaves after a piece is the h_state of the next, the oracle
    object carries its own.  state: (clock, last_i_negative, last_q_negative, working_byte, working_bits, state_register, streamaddress)."""

    def __init__(self, name, sps, lock, xi, xq=None, bps=1, cuts=(), state=None):
        from pymodem_amd._native import SlicerState
        self.name, self.sps, self.lock, self.bps, self.quad = name, sps, lock, bps, xq is not None
        edges = [0] + [int(c) for c in cuts] + [len(xi)]
        self.pieces = [(xi[a:b], xq[a:b] if xq is not None else None) for a, b in zip(edges[:-1], edges[1:])]
        clk, li, lq, wbyte, wbits, sreg, addr = state or (0.0, 0, 0, 0, 0, 0, 0)
        assert wbits % bps == 0 and 0 <= wbits < 8 and 0 <= wbyte < (1 << wbits)
        self.state = SlicerState()
        self.state.phase_clock, self.state.last_i_negative, self.state.last_q_negative = clk, li, lq if self.quad else 0
        self.state.working_byte, self.state.working_bits, self.state.state_register, self.state.streamaddress = wbyte, wbits, sreg, addr
        self.oracle = O.QuadratureSlicer(48000, "qpsk_2400" if bps == 2 else "bpsk_300") if self.quad else O.BinarySlicer(48000, "1200")
        self.oracle.sps, self.oracle.lock_rate = sps, lock
        # (the oracle's state holds the last samples themselves: +1.0 / -1.0 stand for their signs)
        self.oracle.state = np.array([clk, -1.0 if li else 1.0, -1.0 if lq else 1.0, wbyte, wbits, addr, sreg, 0.0])
        self.sreg0 = sreg

    def want(self, r):
        """The oracle over piece r -> (data, addresses, the end state as the slicer object's fields)."""
        xi, xq = self.pieces[r]
        d, a = self.oracle.slice((xi, xq)) if self.quad else self.oracle.slice(xi)
        s = self.oracle.state
        bits = int(s[4])
        fields = {"phase_clock": T.bits_of(s[0]), "last_i_negative": int(s[1] < 0), "last_q_negative": int(s[2] < 0) if self.quad else 0,
                  "working_byte": int(s[3]) & ((1 << bits) - 1), "working_bits": bits,
                  "state_register": (int(s[6]) if self.quad else self.sreg0) & 3, "streamaddress": int(s[5])}
        return d, a, fields

    def got_fields(self):
        s = self.state
        return {"phase_clock": T.bits_of(s.phase_clock), "last_i_negative": s.last_i_negative, "last_q_negative": s.last_q_negative,
                "working_byte": s.working_byte, "working_bits": s.working_bits, "state_register": s.state_register & 3,
                "streamaddress": s.streamaddress}


def slice_on_gpu(ctx, cases, r, capfd, **switches):
    """Piece r of every case as ONE pm_slice_batch call (at most 64 jobs) -> [(data, addresses)] and the (form, LM0, NS0) of the call's
    [slicer] trace lines.  The cases' states are updated in place, as a slicer object's is."""
    from pymodem_amd._native import SliceJob, check as chk, lib as L
    assert 1 <= len(cases) <= 64
    # every distinct sample array once: one upload, one sign bitmap (streams start on 512-byte boundaries of the block)
    arrays, where, at = [], {}, 0
    for c in cases:
        for x in c.pieces[r]:
            if x is not None and id(x) not in where:
                where[id(x)] = (at, len(x))
                arrays.append((at, x))
                at += (len(x) + 63) // 64 * 64
    host = np.zeros(max(at, 64))
    for o, x in arrays:
        host[o:o + len(x)] = x
    dx = ctx.upload(host)
    words = at // 64 + 2 * len(arrays) + 2
    bits = ctx.empty(words, np.uint64)
    bit_at, w = {}, 0
    for o, x in arrays:
        chk(L().pm_signs_f64(ctx.handle, dx.view(o, len(x)).ptr, len(x), bits.view(w, (len(x) + 63) // 64 + 1).ptr))
        bit_at[o] = w
        w += (len(x) + 63) // 64 + 2
    caps, a_off, d_off, room = [], [], [], 0
    for c in cases:
        n = len(c.pieces[r][0])
        caps.append((n * c.bps + 7) // 8 + 8)              # one symbol per sample at the most, and the bits carried in
        a_off.append(room)
        room += caps[-1] * 8
    for cap in caps:
        d_off.append(room)
        room += (cap + 4 + 7) // 8 * 8
    block = ctx.empty(room, np.uint8)
    jobs = (SliceJob * len(cases))()
    for j, c in enumerate(cases):
        xi, xq = c.pieces[r]
        jobs[j].d_bits_i = bits.view(bit_at[where[id(xi)][0]], 1).ptr
        jobs[j].d_bits_q = bits.view(bit_at[where[id(xq)][0]], 1).ptr if xq is not None else None
        jobs[j].n = len(xi)
        p = jobs[j].params
        p.samples_per_symbol, p.lock_rate, p.bits_per_symbol, p.state_mask = c.sps, c.lock, c.bps, 0xF if c.bps == 2 else 0x3
        for k, v in enumerate(QPSK if c.bps == 2 else [0, 0, 1, 1]):
            p.demap[k] = v
        jobs[j].d_data, jobs[j].d_addr, jobs[j].cap = block.ptr.value + d_off[j], block.ptr.value + a_off[j], caps[j]
        jobs[j].h_state = ctypes.pointer(c.state)
    capfd.readouterr()
    with tuned(ctx, slicer_trace=1, **switches):
        chk(L().pm_slice_batch(ctx.handle, jobs, len(cases)))
    forms = {(m.group(1), int(m.group(2)), int(m.group(3))) for m in map(_TRACE.match, capfd.readouterr().err.splitlines()) if m}
    out = block.download(room)
    res = []
    for j in range(len(cases)):
        k = jobs[j].count
        assert 0 <= k <= caps[j]
        res.append((out[d_off[j]:d_off[j] + k].copy(), out[a_off[j]:a_off[j] + 8 * k].view(np.int64).copy()))
    return res, forms


def run_cases(ctx, capfd, cases, no_event=0, **switches):
    """Every piece of every case on the GPU, 64 jobs a call, against the oracle: first the results, then the form the call took -- the one
    pm_slicer_choose picks for the batch's parameters and start clocks.  -> the forms seen."""
    seen = set()
    for r in range(max(len(c.pieces) for c in cases)):
        todo = [c for c in cases if len(c.pieces) > r and len(c.pieces[r][0]) > 0]
        for g in range(0, len(todo), 64):
            group = todo[g:g + 64]
            expect = T.choose([(c.sps, c.lock, c.state.phase_clock) for c in group], event=not no_event)
            got, forms = slice_on_gpu(ctx, group, r, capfd, slicer_no_event_step=no_event, **switches)
            for c, (gd, ga) in zip(group, got):
                wd, wa, wf = c.want(r)
                what = (c.name, c.sps, c.lock, "piece", r, "of", [len(p[0]) for p in c.pieces], "as", sorted(forms))
                assert np.array_equal(gd, wd), (what, "data", gd[:8], wd[:8])
                assert np.array_equal(ga, wa), (what, "addresses", ga[:8], wa[:8])
                assert c.got_fields() == wf, (what, "end state")
            assert forms == {expect}, (forms, expect)
            seen |= forms
    return seen


def natural_cases(sps, lock):
    """The natural-tie streams at every length, each once whole and once cut behind a tie (the tie is then the last sample of the first
    call and lies in its partial last word: thr in the scalar loop and tp in the full words meet the same kind of sample)."""
    cases = []
    streams = {n: T.natural_streams(sps, n) for n in T.NATURAL_N}
    for name, n, cut in T.natural_plan(sps, lock):
        x = streams[n][name]
        cases.append(Case((name, n), sps, lock, x))
        if cut is not None:
            cases.append(Case((name, n, "cut", cut), sps, lock, x, cuts=[cut]))
    return cases


def toggles(sps, lock):
    """slicer_no_event_step 0, and 1 where it takes the batch to another kernel."""
    return [0, 1] if T.choose([(sps, lock, 0.0)])[0] == T.EVENT else [0]


@pytest.mark.parametrize("walkers", [None, (16, 4), (16, 16)], ids=["default", "chunk16-q4", "chunk16-q16"])
@pytest.mark.parametrize("sps,lock", T.NATURAL_PAIRS)
def test_natural_ties(ctx, capfd, sps, lock, walkers):
    """Silence, frames and lone crossings on and behind a tie, 1 to 25 600 samples, whole and cut at a tie.  walkers: chunks of 16 words
    and 4 or 16 words per launch -- cold walkers that start mid-stream and merge, or run to the end on silence."""
    T.check_natural_preconditions(sps, lock)
    switches = {} if walkers is None else {"slicer_chunk_words": walkers[0], "slicer_quantum_words": walkers[1]}
    for no_event in toggles(sps, lock):
        cases = natural_cases(sps, lock)
        assert len(cases) <= 64
        run_cases(ctx, capfd, cases, no_event, **switches)


def carried(j, bps, quad):
    """A non-trivial carried state for job j: an open byte of every length, both last signs, a previous symbol, an address count."""
    wbits = ([0, 2, 6, 4] if bps == 2 else [0, 3, 7, 4, 1])[j % (4 if bps == 2 else 5)]
    return (j & 1, (j >> 1) & 1 if quad else 0, (0xA5 + 37 * j) & ((1 << wbits) - 1), wbits, (j * 7) % 16 if quad else 0, 1000 + 977 * j)


def injected_cases(sps, lock, n, bps, quad, clocks):
    cases = []
    for k, clk in enumerate(clocks):
        li, lq, wbyte, wbits, sreg, addr = carried(k, bps, quad)
        si = T.injected_streams(n, sps, li)
        sq = T.injected_streams(n, sps, lq, seed=6)
        for name in si:
            xq = None
            if quad:                                         # the lone crossing in one arm, in the other, or in both
                xq = sq[name] if name != "cross-at-0" or k % 3 else sq["silence"]
            xi = si[name] if not (quad and name == "cross-at-0" and k % 3 == 1) else si["silence"]
            cases.append(Case((name, n, clk.hex()), sps, lock, xi, xq, bps, state=(clk, li, lq, wbyte, wbits, sreg, addr)))
    return cases


@pytest.mark.parametrize("kind", ["binary", "bpsk", "qpsk"])
@pytest.mark.parametrize("sps,lock,no_event", T.INJECTED_CONFIGS)
def test_injected_clocks(ctx, capfd, sps, lock, no_event, kind):
    """Every form from start clocks at tp, its neighbours, a sample below, thr, the zeros, -sps, sps - 1 and +-2048, with an open byte, last
    signs, a previous symbol and an address count carried in; the clock variants are the jobs of one batch.  Then the clock just beyond
    pm_event_ok's range: alone, and as ONE job of an otherwise eligible batch -- the whole batch moves to step32a, and still equals the
    oracle."""
    bps, quad = (2 if kind == "qpsk" else 1), kind != "binary"
    plain = T.choose([(sps, lock, 0.0)], event=not no_event)
    for n in T.INJECTED_N:
        cases = injected_cases(sps, lock, n, bps, quad, T.injected_clocks(sps))
        assert len(cases) <= 64
        assert run_cases(ctx, capfd, cases, no_event) == {plain}
    beyond = [c for n in T.INJECTED_N for c in injected_cases(sps, lock, n, bps, quad, [T.OUT_OF_RANGE])]
    fallback = (T.HAND,) + plain[1:] if plain[0] == T.EVENT else plain
    assert run_cases(ctx, capfd, beyond, no_event) == {fallback}
    mixed = injected_cases(sps, lock, 65, bps, quad, T.injected_clocks(sps)) + injected_cases(sps, lock, 65, bps, quad, [T.OUT_OF_RANGE])[:1]
    assert len(mixed) <= 64
    assert run_cases(ctx, capfd, mixed, no_event) == {fallback}


def test_all_nine_walker_kernels_are_reached(ctx, capfd):
    """Compare, and Hand and Event with each of LM0 x NS0: one batch each -- quadrature and binary jobs from a clock at tp, on silence
    and on frames, a full word and a partial one -- and the trace names nine different kernels."""
    seen = []
    for (sps, lock, no_event), form in zip(T.NINE, T.NINE_FORMS):
        tp = T.symbol_clock_threshold(sps / 2.0 - 0.5)
        cases = injected_cases(sps, lock, 1025, 1, False, [tp, 0.0]) + injected_cases(sps, lock, 1025, 2, True, [tp, 0.0])
        got = run_cases(ctx, capfd, cases, no_event)
        assert got == {form}, (sps, lock, no_event, got)
        seen.append(form)
    assert len(set(seen)) == 9
