"""The slicer walkers' event step (pymodem_amd/csrc/pm_slicer_event.h) on the CPU: the kernel's own header compiled for the host
(tests/slicer_event_model.cpp), word by word against the reference recurrence (slicer.py:59-107) -- checkpoints, symbol flags and
end state bit for bit -- and its run-length bound checked against exact rational arithmetic.  No GPU needed."""
import ctypes
import math
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import slicer_ties as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_d, _i, _i64, _vp = ctypes.c_double, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    so = str(tmp_path_factory.mktemp("event") / "libslicer_event_model.so")
    subprocess.check_call([gxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "slicer_event_model.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.model_ok.argtypes, lib.model_ok.restype = [_d, _d, _d, _d], _i
    lib.model_run.argtypes, lib.model_run.restype = [_d, _d], _i
    lib.model_plain.argtypes, lib.model_plain.restype = [_d, _vp, _i64, _d, _d, _d, _vp, _vp], _d
    lib.model_event.argtypes, lib.model_event.restype = [_d, _vp, _i64, _d, _d, _d, _i, _vp, _vp, _vp], _d
    lib.model_threshold.argtypes, lib.model_threshold.restype = [_d], _d
    lib.model_choose.argtypes, lib.model_choose.restype = [_vp, _vp, _vp, _i, _i], _i
    return lib


def symbol_clock_threshold(thr):
    """pm_slicer_event.h symbol_clock_threshold: the smallest double x with fl(x + 1.0) >= thr."""
    x = thr - 1.0
    while math.nextafter(x, -math.inf) + 1.0 >= thr:
        x = math.nextafter(x, -math.inf)
    while not (x + 1.0 >= thr):
        x = math.nextafter(x, math.inf)
    return x


def crossings(signs, last=1):
    """Sign stream (+1 / -1, a multiple of 64 long) -> crossing flags per 64-sample word, bit b = sample b (slicer.py:99)."""
    neg = np.asarray(signs) < 0
    prev = np.concatenate([[last < 0], neg[:-1]])
    flags = (neg != prev).astype(np.uint64).reshape(-1, 64)
    return (flags << np.arange(64, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)


def compare(model, zc, sps, lock, clk0=0.0, evt=64):
    thr = sps / 2.0 - 0.5
    tp = symbol_clock_threshold(thr)
    assert model.model_ok(sps, lock, tp, clk0)
    zc = np.ascontiguousarray(zc, np.uint64)
    n = len(zc)
    s_ref, s_ev = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    c_ref, c_ev = np.zeros(n), np.zeros(n)
    ev = ctypes.c_int64(0)
    e_ref = model.model_plain(clk0, zc.ctypes.data, n, thr, sps, lock, s_ref.ctypes.data, c_ref.ctypes.data)
    e_ev = model.model_event(clk0, zc.ctypes.data, n, tp, sps, lock, evt, s_ev.ctypes.data, c_ev.ctypes.data, ctypes.byref(ev))
    bad = np.flatnonzero((c_ref.view(np.uint64) != c_ev.view(np.uint64)) | (s_ref != s_ev))
    assert bad.size == 0, f"sps {sps} lock {lock} clk0 {clk0!r}: first differing word {bad[0]}"
    assert np.float64(e_ref).view(np.uint64) == np.float64(e_ev).view(np.uint64)
    return ev.value / n


# every (samples per symbol, lock rate) the presets make: binary 300 / 1200 / 4800 / 9600 baud, quadrature 300 ... 2400 baud, at the
# sample rates the modems run at (including the AFSK demodulator's oversampled output rate)
RATES = [8000, 11025, 22050, 44100, 48000, 96000]
PAIRS = sorted({(r / b, l) for r in RATES for b, l in [(300, 0.75), (1200, 0.75), (9600, 0.88), (4800, 0.88), (300, 0.815),
                                                        (1200, 0.9), (2400, 0.99), (1800, 0.99)] if 1.0 <= r / b <= 1024.0}
               | {(40.0, 0.77), (8000 / 1200, 0.77), (44100 / 1200, 0.77), (11025 / 300, 0.77)})


def nrzi_like(rng, n, sps, jitter=0.7):
    out, bit = [], 1
    while len(out) < n:
        if rng.random() < 0.5:
            bit = -bit
        out += [bit] * max(1, int(round(sps + rng.normal(0.0, jitter))))
    return np.array(out[:n])


def noise(rng, n, mean):
    runs = np.maximum(1, rng.exponential(mean, n + 64).astype(np.int64))          # at least n samples
    signs = np.repeat(np.where(np.arange(runs.size) % 2 == 0, 1, -1), runs)
    return signs[:n]


@pytest.mark.parametrize("sps,lock", PAIRS)
def test_event_step_equals_reference_for_every_preset(model, sps, lock):
    rng = np.random.default_rng(int(sps * 1000) ^ int(lock * 1000))
    n = 64 * 512
    for signs in (nrzi_like(rng, n, sps), noise(rng, n, max(2.0, sps / 3)), rng.choice([-1, 1], n)):
        compare(model, crossings(signs), sps, lock)
        compare(model, crossings(signs), sps, lock, clk0=float(rng.uniform(-sps, sps)))


@pytest.mark.parametrize("sps,lock", [(40.0, 0.77), (8000 / 1200, 0.75), (44100 / 1200, 0.9), (320.0, 0.815)])
def test_clocks_at_and_below_every_power_of_two(model, sps, lock):
    # a run that starts just below a binade boundary with fine bits is where an addition first rounds
    tp = symbol_clock_threshold(sps / 2.0 - 0.5)
    zc = crossings(nrzi_like(np.random.default_rng(3), 64 * 8, sps))
    for e in range(-30, int(math.log2(sps)) + 2):
        p = 2.0 ** e
        for c in (p, math.nextafter(p, 0.0), math.nextafter(p, 0.0) - 2.0 ** (e - 40), -p, -math.nextafter(p, 0.0), p * lock,
                  p - 1.0, math.nextafter(p - 1.0, -math.inf), p * (1 + 2.0 ** -52)):
            if abs(c) <= 2048.0:
                compare(model, zc, sps, lock, clk0=c)
                compare(model, np.zeros(4, np.uint64), sps, lock, clk0=c)
    for c in (tp, math.nextafter(tp, -math.inf), math.nextafter(tp, math.inf), tp - 1.0, tp - 2.0 ** -20, tp - 2.0 ** -21, 0.0, -0.0):
        compare(model, zc, sps, lock, clk0=c)
        compare(model, np.zeros(4, np.uint64), sps, lock, clk0=c)


def test_digital_silence_and_dense_crossings(model):
    for sps, lock in [(40.0, 0.77), (8000 / 1200, 0.75), (11025 / 300, 0.815)]:
        compare(model, np.zeros(2000, np.uint64), sps, lock)                         # no crossing at all
        compare(model, np.full(200, 0xFFFFFFFFFFFFFFFF, np.uint64), sps, lock)        # one at every sample
        compare(model, np.full(200, 0x5555555555555555, np.uint64), sps, lock)
        rng = np.random.default_rng(5)
        for mean in (1.5, 3.0, 6.0, 12.0, 25.0):
            compare(model, crossings(noise(rng, 64 * 256, mean)), sps, lock)


def test_fallback_threshold_mixes_forms_bit_for_bit(model):
    rng = np.random.default_rng(9)
    zc = crossings(noise(rng, 64 * 1024, 4.0))
    for evt in (0, 1, 8, 16, 24, 64):
        compare(model, zc, 40.0, 0.77, evt=evt)


def test_events_per_word_on_nrzi_like_frames(model):
    # the event form pays per real step: on frame-like sign streams a word of 64 samples needs a handful
    rng = np.random.default_rng(11)
    per_word = compare(model, crossings(nrzi_like(rng, 64 * 4096, 40.0)), 40.0, 0.77)
    assert per_word < 8.0, per_word


def exact_run_ok(clk, k, tp):
    """clk + j exact for 0 <= j <= k and clk + j < tp for 0 <= j < k."""
    c = Fraction(clk)
    for j in range(k + 1):
        if Fraction(float(c + j)) != c + j:
            return False
        if j < k and c + j >= Fraction(tp):
            return False
    return True


def test_run_bound_is_a_lower_bound_in_exact_arithmetic(model):
    rng = np.random.default_rng(13)
    for sps, lock in [(40.0, 0.77), (8000 / 1200, 0.75), (44100 / 1200, 0.9), (320.0, 0.815), (1024.0, 0.99)]:
        tp = symbol_clock_threshold(sps / 2.0 - 0.5)
        tpe = tp - 2.0 ** -20
        clocks = [float(x) for x in rng.uniform(-sps, tp + 1.0, 300)]
        clocks += [float(x) * lock for x in rng.integers(-int(sps), int(tp) + 2, 100)]
        clocks += [2.0 ** e * s for e in range(-40, 11) for s in (1.0, -1.0, 1.0 - 2.0 ** -52, 1.0 + 2.0 ** -30)]
        clocks += [tp, math.nextafter(tp, -math.inf), tp - 1.0, math.nextafter(tp - 1.0, math.inf), 0.0, -0.0, 5e-324]
        for c in clocks:
            if abs(c) > 2048.0:
                continue
            k = model.model_run(c, tpe)
            assert 0 <= k and exact_run_ok(c, min(k, 200), tp), (sps, c, k)


def test_host_precondition_rejects_what_the_bound_does_not_cover(model):
    tp = symbol_clock_threshold(19.5)
    assert model.model_ok(40.0, 0.77, tp, 0.0)
    assert model.model_ok(1024.0, 0.5, symbol_clock_threshold(511.5), -2048.0)
    for sps, lock, t, clk0 in [(40.0, 1.01, tp, 0.0),             # the crossing's product may grow the clock
                               (40.0, 0.49, tp, 0.0),             # lock - 1 not exact (fma form)
                               (40.0, -0.77, tp, 0.0),
                               (0.5, 0.77, tp, 0.0),              # sps below one sample
                               (1025.0, 0.77, 511.0, 0.0),        # beyond the clock range the margins were sized for
                               (40.0, 0.77, 1500.0, 0.0),
                               (40.0, 0.77, -1500.0, 0.0),
                               (40.0, 0.77, tp, 2049.0),
                               (40.0, 0.77, tp, -1e300),
                               (math.nan, 0.77, tp, 0.0), (40.0, math.nan, tp, 0.0), (40.0, 0.77, math.nan, 0.0),
                               (40.0, 0.77, tp, math.nan), (40.0, 0.77, tp, math.inf), (math.inf, 0.77, tp, 0.0)]:
        assert not model.model_ok(sps, lock, t, clk0), (sps, lock, t, clk0)



COMPARE, HAND, EVENT = 0, 1, 2          # SlicerForm


def choose(model, jobs, event=True):
    """pm_slicer_choose over jobs of (sps, lock, clk0): (form, lm0, ns0)."""
    sps, lock, clk0 = (np.ascontiguousarray([j[k] for j in jobs], np.float64) for k in range(3))
    r = model.model_choose(sps.ctypes.data, lock.ctypes.data, clk0.ctypes.data, len(jobs), int(event))
    assert r >= 0
    return r >> 2, bool(r & 1), bool(r & 2)


def low_word_zero(x):
    return int(np.float64(x).view(np.uint64)) & 0xFFFFFFFF == 0


def test_symbol_clock_threshold_of_the_header(model):
    for sps, _ in PAIRS:
        thr = sps / 2.0 - 0.5
        assert np.float64(model.model_threshold(thr)).view(np.uint64) == np.float64(symbol_clock_threshold(thr)).view(np.uint64), sps
    for thr in (math.inf, -math.inf, math.nan):
        assert math.isnan(model.model_threshold(thr))


@pytest.mark.parametrize("sps,lock", PAIRS)
def test_step_form_of_every_preset(model, sps, lock):
    # the event step exactly where its preconditions hold and a word has few enough symbols for it to pay, the hand-scheduled step
    # elsewhere (fsk_9600 at 5 samples per symbol among them); LM0 / NS0 from the low words of lock_rate - 1 and sps
    tp = symbol_clock_threshold(sps / 2.0 - 0.5)
    want = EVENT if model.model_ok(sps, lock, tp, 0.0) and sps >= 16.0 else HAND
    lm0, ns0 = low_word_zero(lock - 1.0), low_word_zero(sps)
    assert choose(model, [(sps, lock, 0.0)]) == (want, lm0, ns0)
    assert choose(model, [(sps, lock, 0.0)], event=False) == (HAND, lm0, ns0)
    if sps == 5.0:
        assert want == HAND


def test_step_form_of_a_batch(model):
    assert choose(model, [(40.0, 0.77, 0.0), (40.0, 0.75, -3.5)]) == (EVENT, False, True)
    assert choose(model, [(40.0, 0.75, 0.0), (48000 / 1800, 0.75, 0.0)]) == (EVENT, True, False)
    assert choose(model, [(40.0, 0.75, 0.0), (5.0, 0.88, 0.0)]) == (HAND, False, True)       # one job below 16 samples per symbol
    assert choose(model, [(40.0, 0.75, 0.0), (40.0, 0.75, 3000.0)]) == (HAND, True, True)    # one clock beyond pm_event_ok's range
    assert choose(model, [(40.0, 0.77, 0.0), (40.0, 0.45, 0.0)])[0] == COMPARE


@pytest.mark.parametrize("sps,lock,clk0", [(40.0, 0.45, 0.0), (40.0, 0.3, 0.0), (5.0, 0.45, 0.0), (40.0, 0.77, math.nan),
                                           (40.0, 0.77, math.inf), (math.inf, 0.77, 0.0), (math.nan, 0.77, 0.0),
                                           (40.0, 0.0, 0.0), (25.0, -0.0, 0.0), (40.0, -0.5, 0.0), (5.0, -1.0, 0.0), (25.0, -2.0, 3.5)])
def test_step_form_falls_back_to_the_compare(model, sps, lock, clk0):
    # lock_rate - 1 not exact (the fma form needs it), a clock or samples per symbol that are not finite: the reference's compare.
    # lock_rate <= 0, although lock_rate - 1 is exact for 0.0, -0.5, -1.0: fma(c, lock - 1, c) and the reference's c * lock agree in value
    # but not in the sign of a zero (lock 0: c * 0.0 is -0.0 for c < 0, the fma's exact zero sum is +0.0; lock < 0: the other way round at
    # c = +0.0), and a stream that ends on such a sample carries that sign out in phase_clock
    if lock in (0.45, 0.3):
        assert (lock - 1.0) + 1.0 != lock
    if lock <= 0.0:
        assert (lock - 1.0) + 1.0 == lock
    assert choose(model, [(sps, lock, clk0)]) == (COMPARE, False, False)
    assert choose(model, [(40.0, 0.75, 0.0), (sps, lock, clk0)]) == (COMPARE, False, False)
    assert choose(model, [(sps, lock, clk0)], event=False) == (COMPARE, False, False)


# ---- the inputs of the tie tests (tests/slicer_ties.py; the GPU tests that use them: test_gpu_slicer_ties.py, test_gpu_rowslice_ties.py) -----
_FORM_NAMES = {COMPARE: T.COMPARE, HAND: T.HAND, EVENT: T.EVENT}


def header_choice(model, jobs, event=True):
    form, lm0, ns0 = choose(model, jobs, event)
    return _FORM_NAMES[form], int(lm0), int(ns0)


def test_python_copy_of_the_form_choice_equals_the_header(model):
    for thr in [12.0, 1.0, 2.0, 7.5, math.inf, math.nan] + [sps / 2.0 - 0.5 for sps, _ in PAIRS + T.NATURAL_PAIRS]:
        assert bits_equal(T.symbol_clock_threshold(thr), model.model_threshold(thr)) or (math.isnan(T.symbol_clock_threshold(thr))
                                                                                         and math.isnan(model.model_threshold(thr))), thr
    assert math.isnan(T.symbol_clock_threshold(1.0))          # 3 samples per symbol: the header cannot pin tp down, the batch compares
    singles = [(sps, lock, 0.0) for sps, lock in T.NATURAL_PAIRS] + [(sps, lock, 0.0) for sps, lock, _ in T.INJECTED_CONFIGS]
    singles += [(sps, lock, clk) for sps, lock, _ in T.INJECTED_CONFIGS for clk in T.injected_clocks(sps) + [T.OUT_OF_RANGE]]
    singles += [(sps, lock, clk0) for sps, lock in PAIRS for clk0 in (0.0, 3000.0)] + [(40.0, math.nan, 0.0), (40.0, 0.77, math.inf)]
    for job in singles:
        for event in (True, False):
            assert T.choose([job], event) == header_choice(model, [job], event), (job, event)
    for sps, lock, _ in T.INJECTED_CONFIGS:
        batch = [(sps, lock, clk) for clk in T.injected_clocks(sps)]
        for jobs in (batch, batch + [(sps, lock, T.OUT_OF_RANGE)]):
            for event in (True, False):
                assert T.choose(jobs, event) == header_choice(model, jobs, event), (sps, lock, event)


def bits_equal(a, b):
    return T.bits_of(a) == T.bits_of(b)


def test_tie_test_parameters_reach_every_kernel(model):
    # the nine walker kernels: Compare, and Hand and Event with LM0 x NS0 each
    got = [header_choice(model, [(sps, lock, 0.0)], event=not no_event) for sps, lock, no_event in T.NINE]
    assert got == T.NINE_FORMS and len(set(got)) == 9
    # ... each still the same kernel from every injected clock in pm_event_ok's range, and step32a from the one beyond it
    for (sps, lock, no_event), form in zip(T.NINE, T.NINE_FORMS):
        jobs = [(sps, lock, clk) for clk in T.injected_clocks(sps)]
        assert header_choice(model, jobs, event=not no_event) == form
        beyond = header_choice(model, jobs + [(sps, lock, T.OUT_OF_RANGE)], event=not no_event)
        assert beyond == ((T.HAND,) + form[1:] if form[0] == T.EVENT else form)
    # the five row kernels (the row slicers are chosen without the event step, from a clock of 0.0)
    rows = [header_choice(model, [(48000.0 / rate, lock, 0.0)] * 2, event=False) for rate, lock in T.ROW_CASES]
    assert rows == T.ROW_FORMS and len(set(rows)) == 5
    assert 48000.0 / 1920.0 == 25.0 and 48000.0 / 1800.0 == T.NS0_OFF


@pytest.mark.parametrize("sps,lock", T.NATURAL_PAIRS)
def test_natural_tie_inputs_hold_their_ties(sps, lock):
    assert T.check_natural_preconditions(sps, lock)
    for name, n, cut in T.natural_plan(sps, lock):
        if cut is not None:                                  # the cut leaves the tie as the last sample of a partial last word
            x = T.natural_streams(sps, n)[name]
            ties = T.reference(x[:cut] < 0, sps, lock)[0]
            assert ties and ties[-1] == cut - 1 and cut % 64 != 0 and cut < n, (name, n, cut)


def test_injected_clocks_decide_at_the_first_sample():
    # tp takes a symbol at sample 0 and ties there when thr is an integer; its predecessor does not; tp - 1 ties a sample later
    for sps, lock, _ in T.INJECTED_CONFIGS:
        thr = sps / 2.0 - 0.5
        tp = T.symbol_clock_threshold(thr)
        quiet = np.zeros(3) < 0
        assert T.reference(quiet, sps, lock, clk0=tp)[1][:1] == [0]
        assert 0 not in T.reference(quiet, sps, lock, clk0=math.nextafter(tp, -math.inf))[1]
        assert T.reference(quiet, sps, lock, clk0=math.nextafter(tp, math.inf))[1][:1] == [0]
        if thr == int(thr):
            assert T.reference(quiet, sps, lock, clk0=tp)[0][:1] == [0] and T.reference(quiet, sps, lock, clk0=tp - 1.0)[0][:1] == [1]
        assert (len(T.injected_clocks(sps)) + 1) * len(T.injected_streams(64, sps, 0)) <= 64


TIE_SPS, TIE_LOCKS = [17.0, 25.0, 33.0], [0.5, 0.75, 0.875, 1.0]


@pytest.mark.parametrize("lock", TIE_LOCKS)
@pytest.mark.parametrize("sps", TIE_SPS)
def test_event_step_equals_reference_on_tie_streams(model, sps, lock):
    """Odd integer samples per symbol (an integer threshold): silence ties at every symbol, and with lock_rate 0.5 frames tie between
    crossings.  The event header against the reference recurrence on silence, frames and a lone crossing on and behind a tie, from the
    clocks at and around tp as well."""
    n = 25600
    ties, syms, _ = T.reference(T.silence(n) < 0, sps, lock)
    assert ties == syms and len(ties) >= n / sps - 1
    streams = T.natural_streams(sps, n)
    assert set(streams) == {"silence", "frames", "cross-on-tie", "cross-after-tie"}
    if lock == 0.5:
        x = streams["frames"]
        assert any(t > int(np.argmax(x < 0)) for t in T.reference(x < 0, sps, lock)[0])
    on, after = (int(np.argmax(streams[k] < 0)) for k in ("cross-on-tie", "cross-after-tie"))
    assert on in ties and after - 1 in ties
    for name, x in streams.items():
        zc = crossings(np.where(x < 0, -1, 1))
        compare(model, zc, sps, lock)
        for clk0 in T.injected_clocks(sps):
            compare(model, zc[:8], sps, lock, clk0=clk0)
        compare(model, zc, sps, lock, evt=0)                  # every word through step32a's operations
