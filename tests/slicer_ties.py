"""Inputs on which the symbol-timing slicers decide at a tie (tests/test_gpu_slicer_ties.py, tests/test_gpu_rowslice_ties.py and, for the
preconditions that need no GPU, tests/test_slicer_event_model.py): the reference recurrence in plain Python with a count of the samples at
which fl(clk + 1.0) == thr exactly, the streams that make such samples, the clocks to carry in, and the launchers' choice of step form.

A tie is a sample at which the sum clk + 1.0 equals the threshold sps/2 - 0.5: the reference's `>=` takes a symbol there, and the forms of
the step that read the decision off the clock (clk >= tp, tp = symbol_clock_threshold(thr)) must take it at the same sample.  With an odd
integer sps the threshold is an integer and a stream without crossings ties at every symbol; with lock_rate 0.5 a crossing leaves binary
fractions that tie now and then."""
import functools
import math

import numpy as np

COMPARE, HAND, EVENT = "compare", "step32a", "event"          # the [slicer] trace's names of the forms (pm_slicer.hip kFormNames)
NS0_OFF = 48000 / 1800                                        # samples per symbol whose low word is not zero (NS0 = 0)


def symbol_clock_threshold(thr):
    """pm_slicer_event.h symbol_clock_threshold: the smallest double x with fl(x + 1.0) >= thr; NaN where the header gives up (64 steps:
    thr = 1.0, where the answer lies 2^-54 below zero and the walk down from 0.0 goes through the subnormals -- such a batch keeps the
    compare on the sum)."""
    if not math.isfinite(thr):
        return math.nan
    x = thr - 1.0
    for k in range(64):
        p = math.nextafter(x, -math.inf)
        if not (p + 1.0 >= thr):
            break
        x = p
        if k == 63:
            return math.nan
    for k in range(64):
        if x + 1.0 >= thr:
            return x
        x = math.nextafter(x, math.inf)
    return math.nan


def bits_of(v):
    return int(np.float64(v).view(np.uint64))


def low_word_zero(v):
    return bits_of(v) & 0xFFFFFFFF == 0


def choose(jobs, event=True):
    """pm_slicer_choose (pm_slicer_event.h) over jobs of (sps, lock, clk0) -> (form, LM0, NS0) as the [slicer] trace prints them.
    tests/test_slicer_event_model.py holds it against the header's own."""
    hand, lm0, ns0 = True, True, True
    for sps, lock, clk0 in jobs:
        tp = symbol_clock_threshold(sps / 2.0 - 0.5)
        lm1 = lock - 1.0
        hand = hand and lm1 + 1.0 == lock and lock > 0.0 and math.isfinite(sps) and math.isfinite(clk0) and math.isfinite(tp)
        lm0 = lm0 and low_word_zero(lm1)
        ns0 = ns0 and low_word_zero(sps)
        event = (event and 1.0 <= sps <= 1024.0 and 0.5 <= lock <= 1.0 and -1024.0 <= tp <= 1024.0 and -2048.0 <= clk0 <= 2048.0
                 and sps >= 16.0)
    if not hand:
        return COMPARE, 0, 0
    return (EVENT if event else HAND), int(lm0), int(ns0)


def reference(neg, sps, lock, clk0=0.0, last_neg=False, neg_q=None, last_q_neg=False):
    """The reference recurrence (slicer.py:59-107, :193-242) on sign flags (True: sample < 0), sample by sample in Python floats.
    -> (tie samples, symbol samples, end clock): the samples at which clk + 1.0 == thr, and those at which a symbol was taken."""
    thr = sps / 2.0 - 0.5
    clk, ties, syms = clk0, [], []
    li, lq = bool(last_neg), bool(last_q_neg)
    neg = [bool(v) for v in neg]
    negq = [bool(v) for v in neg_q] if neg_q is not None else None
    for k, s in enumerate(neg):
        clk += 1.0
        if clk == thr:
            ties.append(k)
        if clk >= thr:
            clk -= sps
            syms.append(k)
        cross = s != li
        li = s
        if negq is not None:
            cross = cross or negq[k] != lq
            lq = negq[k]
        if cross:
            clk = clk * lock
    return ties, syms, clk


# ---- streams (+1.0 / -1.0 / 0.0 samples; a sample >= 0 is "not negative", as the slicers and pm_signs_f64 take it) ----------------------
def silence(n):
    return np.zeros(n)


def frames(n, sps, seed):
    """NRZI-like symbols of sps samples with jitter and a little noise (the `frames` stream of tests/test_gpu_slicer_event_step.py, scaled
    to sps): the first symbol is not negative, so nothing crosses before the first flip."""
    rng = np.random.default_rng(seed)
    full = max(n, 25600)                                     # (a shorter stream is the head of the 25 600-sample one)
    lengths = np.maximum(1, np.round(sps + rng.normal(0.0, 0.7, int(full / max(sps - 2.0, 1.0)) + 8)).astype(np.int64))
    flips = rng.random(lengths.size) < 0.5
    flips[0] = False
    levels = np.repeat(np.where(np.cumsum(flips) % 2 == 0, 1.0, -1.0), lengths)[:full]
    x = levels + 0.3 * rng.standard_normal(full)
    x[:int(sps)] = 1.0
    return np.where(x >= 0, 1.0, -1.0)[:n]


def lone_crossing(n, at):
    """Not negative up to sample `at`, negative from it on: one crossing, at sample `at` (none if at >= n)."""
    x = np.ones(n)
    x[at:] = -1.0
    return x


def first_tie(sps):
    """The first tie of a stream without crossings from clock 0.0 with an integer threshold: the sample at which clk + 1.0 reaches thr."""
    thr = sps / 2.0 - 0.5
    assert thr == int(thr) and thr >= 1
    return int(thr) - 1


# lock_rate 0.5 on frames: the seed was picked on the CPU so that, at every sps used here, the first 1025 samples already hold a tie
# between crossings (tests/test_slicer_event_model.py asserts it)
FRAME_SEED = 3


NATURAL_N = [1, 63, 64, 65, 1025, 25600]
LOCKS = [0.45, 0.5, 0.75, 0.77, 1.0, 0.0, -0.5]
# (sps, lock) of the natural-tie cases: odd integer sps with every lock; even sps with lock 0.5; the small sps of the Hand form; and a
# fractional sps (no natural ties: it is there for the NS0 = 0 kernels, which the injected clocks take to their ties)
NATURAL_PAIRS = ([(float(s), l) for s in (17, 25, 33) for l in LOCKS] + [(16.0, 0.5), (40.0, 0.5)]
                 + [(3.0, 0.5), (3.0, 0.75), (5.0, 0.5), (5.0, 0.88)] + [(NS0_OFF, 0.75), (NS0_OFF, 0.77)])


def natural_streams(sps, n):
    """{name: samples} of the natural-tie streams of n samples at sps."""
    out = {"silence": silence(n), "frames": frames(n, sps, FRAME_SEED)}
    thr = sps / 2.0 - 0.5
    if thr == int(thr) and thr >= 1:
        t = first_tie(sps)
        t2 = t + int(sps)                      # the second symbol's tie: a crossing there meets a clock that a symbol has already wrapped
        out["cross-on-tie"] = lone_crossing(n, t2)
        out["cross-after-tie"] = lone_crossing(n, t2 + 1)
    else:
        out["cross-early"] = lone_crossing(n, int(sps))
    return out


def cut_at_tie(x, sps, lock):
    """Where to cut the stream so that a tie sample is the last sample of a call and lies in that call's partial last word: the first tie
    that is not the last sample of a 64-sample word, plus one.  None if the stream has no such tie."""
    ties, _, _ = reference(x < 0, sps, lock)
    for t in ties:
        if t % 64 != 63 and t + 1 < len(x):
            return t + 1
    return None


@functools.lru_cache(maxsize=None)
def natural_plan(sps, lock):
    """[(stream name, n, cut or None)] of the natural-tie cases at (sps, lock): every stream at every length, and where to cut it."""
    return [(name, n, cut_at_tie(x, sps, lock)) for n in NATURAL_N for name, x in natural_streams(sps, n).items()]


@functools.lru_cache(maxsize=None)
def check_natural_preconditions(sps, lock):
    """What the natural-tie cases promise about their INPUTS, counted on the CPU by the reference recurrence: on silence with an integer
    threshold every symbol is taken at a tie and there are at least n/sps - 1 of them; with lock_rate 0.5 the frames of 1025 and of 25 600
    samples hold a tie BEHIND their first crossing; and where ties exist, streams are cut at one."""
    thr = sps / 2.0 - 0.5
    n = NATURAL_N[-1]
    if thr == int(thr):
        ties, syms, _ = reference(silence(n) < 0, sps, lock)
        assert ties == syms and len(ties) >= n / sps - 1, (sps, len(ties), len(syms))
    if lock == 0.5 and sps >= 16:
        for m in NATURAL_N[-2:]:
            x = frames(m, sps, FRAME_SEED)
            first = int(np.argmax(x < 0))
            assert (x < 0).any() and any(t > first for t in reference(x < 0, sps, lock)[0]), (sps, m)
    if thr == int(thr) or (lock == 0.5 and sps >= 16):
        cuts = [(name, m, cut) for name, m, cut in natural_plan(sps, lock) if cut is not None]
        assert len(cuts) >= 4 and any(m == n for _, m, _ in cuts), (sps, lock, cuts)
        assert all(cut % 64 != 0 for _, _, cut in cuts)
    return True


# ---- clocks to carry in ------------------------------------------------------------------------------------------------------------
def injected_clocks(sps):
    """Start clocks at and around the decision: tp and its neighbours, a sample before them, thr itself, the zeros, a whole symbol below, the
    clock whose symbol leaves an exact zero (sps - 1), and the limits of pm_event_ok's clock range (the last one lies beyond it: see OUT_OF_RANGE)."""
    thr = sps / 2.0 - 0.5
    tp = symbol_clock_threshold(thr)
    return [tp, math.nextafter(tp, -math.inf), math.nextafter(tp, math.inf), tp - 1.0, math.nextafter(tp - 1.0, -math.inf), thr,
            0.0, -0.0, -sps, sps - 1.0, 2048.0, -2048.0]


OUT_OF_RANGE = math.nextafter(2048.0, math.inf)               # beyond pm_event_ok: the batch falls back to step32a
INJECTED_N = [1, 64, 65, 4097]
# (sps, lock, slicer_no_event_step) that reach the nine walker kernels -- Compare; Hand and Event with LM0 x NS0 -- then Hand at a small sps
# and with lock rates whose lock - 1 is exact outside [0.5, 1]
NINE = [(25.0, 0.45, 0),
        (NS0_OFF, 0.77, 1), (NS0_OFF, 0.75, 1), (25.0, 0.77, 1), (25.0, 0.75, 1),
        (NS0_OFF, 0.77, 0), (NS0_OFF, 0.75, 0), (25.0, 0.77, 0), (17.0, 0.5, 0)]
NINE_FORMS = [(COMPARE, 0, 0), (HAND, 0, 0), (HAND, 1, 0), (HAND, 0, 1), (HAND, 1, 1), (EVENT, 0, 0), (EVENT, 1, 0), (EVENT, 0, 1), (EVENT, 1, 1)]
INJECTED_CONFIGS = NINE + [(5.0, 0.88, 0), (33.0, 1.0, 0), (40.0, 1.5, 0), (25.0, 0.0, 0), (25.0, -0.5, 0), (NS0_OFF, 0.0, 0)]


def injected_streams(n, sps, last_neg, seed=5):
    """{name: samples}: silence (of the sign the state carries: no crossing), one crossing at sample 0, one at the LAST sample (of a full
    word when n is a multiple of 64: the crossing's product is then the end state itself, zero's sign included), frames."""
    same = np.full(n, -1.0 if last_neg else 1.0)
    end = same.copy()
    end[-1] = -end[-1]
    return {"silence": same, "cross-at-0": -same, "cross-at-end": end, "frames": frames(n, sps, seed)}


# ---- the batch engine's row slicers (tests/test_gpu_rowslice_ties.py) --------------------------------------------------------------------
# (symbol rate at 48 kHz, lock): sps 25 and 48000/1800 with lock 0.75 / 0.77, and the compare at 0.45 -- the five rowslice_kernel forms
ROW_CASES = [(1920.0, 0.75), (1920.0, 0.77), (1800.0, 0.75), (1800.0, 0.77), (1920.0, 0.45)]
ROW_FORMS = [(HAND, 1, 1), (HAND, 0, 1), (HAND, 1, 0), (HAND, 0, 0), (COMPARE, 0, 0)]
