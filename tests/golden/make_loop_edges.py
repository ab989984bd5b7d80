#!/usr/bin/env python3
"""Fixtures for the carrier loops at the edges of their quantisers and branches, made by IMPORTING the reference
(ninocarrillo/pymodem) in the build container, as make_goldens.py does.  Only DATA is written:

    tests/golden/loop_edges.npz            per case: parameters, initial state, input rows, the reference's outputs, the end state
    tests/golden/loop_edges_recordings.npz seven degenerate recordings and the reference's modem outputs on them, every sample (a file
                                           of its own: no committed file may exceed 1 MiB)
    tests/golden/loop_edges_summary.json   per case: loop, length, piece boundaries, how many samples hit each edge

Run (build container only):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_loop_edges.py

The loop bodies below are compositions of the reference's own objects (NCO, IIR_1, PI_control, PhaseDetector, ComplexNumber) in the
order of psk.py:173-189 (BPSK Costas), :434-467 (QPSK Costas), :734-747 (MPSK) and afsk_pll.py:153-165 (AFSK PLL); an object's
coefficients or state may be overwritten after construction.  Nothing is computed here that the reference does not compute: the
counters only LOOK at the objects' state before and after each update.

Edges (counted per sample):
    slow    phase + step outside [0, 4 pi): a negative phase, or a turn or more in one sample (nco.py:36-39 make more than one trip
            or the second loop runs)
    idx256  int(phase * index_scaling) == 256: the reference's swallowed IndexError (nco.py:41-45), the old sine is kept
    rail    the integral is +-i_limit after the update (pi_control.py:28-31)
    tie     MPSK: the PI output is exactly k + 0.5, round() goes to the even neighbour (psk.py:740)
    clip    MPSK: floor(x * 32) >= 64 or <= -64 on either detector input (phase_detector.py:127-134)
"""
import contextlib
import io
import json
import math
import os
import sys

sys.dont_write_bytecode = True
REF = os.environ.get("PYMODEM_REFERENCE", "/root/reference")
sys.path.insert(0, REF)

import numpy as np  # noqa: E402

from modems_codecs.nco import NCO  # noqa: E402
from modems_codecs.iir import IIR_1  # noqa: E402
from modems_codecs.pi_control import PI_control  # noqa: E402
from modems_codecs.phase_detector import PhaseDetector  # noqa: E402
from modems_codecs.complexmath import ComplexNumber  # noqa: E402
import modems_codecs.psk as ref_psk  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
TWO_PI = 2.0 * math.pi
MAX_TRIPS = 256                 # the kernels' guard is 4096 trips and the oracle's C loops have none: stay far below
LOOPS = ("bpsk", "qpsk", "pll", "mpsk")
EDGES = ("slow", "idx256", "rail", "tie", "clip")
APPLIES = {"slow": LOOPS, "idx256": LOOPS, "rail": LOOPS, "tie": ("mpsk",), "clip": ("mpsk",)}


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


class RefLoop:
    """One carrier loop made of the reference's objects."""

    def __init__(self, kind, rate, carrier, cutoff, p, i, limit, gain, branch_cutoff=1200.0):
        self.kind = kind
        self.nco = NCO(sample_rate=rate, amplitude=1.0, set_frequency=carrier, wavetable_size=256)
        self.nco.sine_output = 0.0            # (the reference creates both on the first update; the first sample of a case that
        self.nco.cosine_output = 0.0          # starts on index 256 needs a sine to keep)
        self.lpf = IIR_1(sample_rate=rate, filter_type="lpf", cutoff=cutoff, gain=1.0)
        self.pi = PI_control(p=p, i=i, i_limit=limit, gain=gain)
        self.cos_lpf = IIR_1(sample_rate=rate, filter_type="lpf", cutoff=branch_cutoff, gain=1.0)
        self.sin_lpf = IIR_1(sample_rate=rate, filter_type="lpf", cutoff=branch_cutoff, gain=1.0)
        self.pd = PhaseDetector("qpsk", 64, 32)

    def params(self):
        n, f, c = self.nco, self.lpf, self.pi
        return np.array([n.phase_scaling_factor, n.index_scaling_factor, n.set_frequency, f.b_coefs[0], f.b_coefs[1], f.a_coefs[1],
                         c.p_rate, c.i_rate, c.i_limit, c.gain], dtype=np.float64)

    def state(self):
        n, f, c = self.nco, self.lpf, self.pi
        return np.array([n.phase_accumulator, n.control, n.sine_output, n.cosine_output, f.X[0], f.X[1], f.Y[0], c.integral, c.proportional],
                        dtype=np.float64)

    def branch(self):
        a, b = self.cos_lpf, self.sin_lpf
        return np.array([a.b_coefs[0], a.b_coefs[1], a.a_coefs[1], a.X[0], a.X[1], a.Y[0], b.X[0], b.X[1], b.Y[0]], dtype=np.float64)

    def step(self, s0, s1, count):
        """One sample in the reference's order; returns the outputs.  `count` gets the edges this sample hit."""
        nco, lpf, pi = self.nco, self.lpf, self.pi
        ph0 = nco.phase_accumulator + (nco.phase_scaling_factor * (nco.set_frequency + nco.control))      # what nco.py:35 will make
        assert math.isfinite(ph0)
        trips_down = trips_up = 0
        p = ph0
        while p >= TWO_PI:
            p = p - TWO_PI
            trips_down += 1
        while p < 0:
            p = p + TWO_PI
            trips_up += 1
        assert trips_down <= MAX_TRIPS and trips_up <= MAX_TRIPS, (trips_down, trips_up)
        with quiet():                                                   # (the IndexError path prints)
            nco.update()
        assert nco.phase_accumulator == p
        count["slow"] += not (0.0 <= ph0 < 2.0 * TWO_PI)
        count["idx256"] += int(nco.phase_accumulator * nco.index_scaling_factor) == 256
        if self.kind == "bpsk":                                         # psk.py:173-189
            in_phase = s0 * nco.ComplexOutput.real
            quadrature = s0 * nco.ComplexOutput.imag
            lpf.update(in_phase * quadrature)
            nco.control = pi.update_saturate(lpf.output)
            out = (in_phase, 0.0)
        elif self.kind == "pll":                                        # afsk_pll.py:153-165
            lpf.update(s0 * nco.sine_output)
            nco.control = pi.update_saturate(lpf.output)
            out = (pi.proportional, 0.0)
        elif self.kind == "qpsk":                                       # psk.py:434-467
            self.cos_lpf.update(s0 * nco.cosine_output)
            sign_c = 1 if self.cos_lpf.output >= 0 else -1
            self.sin_lpf.update(s0 * nco.sine_output)
            arm_c, arm_s = self.cos_lpf.output, self.sin_lpf.output
            out = (arm_s, arm_c)
            sign_s = 1 if arm_s >= 0 else -1
            lpf.update((arm_c * sign_s) - (arm_s * sign_c))
            nco.control = pi.update_saturate(lpf.output)
        else:                                                           # psk.py:734-747
            sample = ComplexNumber(s0, s1)
            sample.multiply(nco.ComplexOutput)
            lpf.update(self.pd.get_qpsk_angle_error(sample.real, sample.imag))
            nco.control = round(pi.update_saturate(lpf.output))
            out = (sample.real, sample.imag)
            count["tie"] += pi.output - math.floor(pi.output) == 0.5
            fr, fi = math.floor(sample.real * 32.0), math.floor(sample.imag * 32.0)
            count["clip"] += fr >= 64 or fr <= -64 or fi >= 64 or fi <= -64
        count["rail"] += abs(pi.integral) == pi.i_limit
        return out


CASES = {}          # name -> arrays
SUMMARY = {}        # name -> {"loop", "n", "splits", "counts", "kind"}


def run_case(name, kind, loop, x0, x1=None, splits=None, check=None):
    """Run `loop` over the input rows, record everything.  splits: piece boundaries the tests carry the state across (beside the
    halves and thirds every case is cut into).  check(loop, k): called after sample k (for the cases that promise a state)."""
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    x1 = np.zeros(len(x0)) if x1 is None else np.ascontiguousarray(x1, dtype=np.float64)
    assert np.all(np.isfinite(x0)) and np.all(np.isfinite(x1))
    d = {"params": loop.params(), "state0": loop.state(), "x0": x0}
    assert np.all(np.isfinite(d["params"])) and np.all(np.isfinite(d["state0"]))
    if loop.kind == "mpsk":
        d["x1"] = x1
    if loop.kind == "qpsk":
        d["branch0"] = loop.branch()
    count = dict.fromkeys(EDGES, 0)
    o0, o1 = np.empty(len(x0)), np.empty(len(x0))
    for k in range(len(x0)):
        o0[k], o1[k] = loop.step(float(x0[k]), float(x1[k]), count)
        if check is not None:
            check(loop, k)
    d["out0"] = o0
    if loop.kind in ("mpsk", "qpsk"):
        d["out1"] = o1
    d["state1"] = loop.state()
    if loop.kind == "qpsk":
        d["branch1"] = loop.branch()
    assert np.all(np.isfinite(o0)) and np.all(np.isfinite(o1)) and np.all(np.isfinite(d["state1"]))
    full = f"{loop.kind}__{name}"
    CASES[full] = d
    SUMMARY[full] = {"loop": loop.kind, "kind": kind, "n": len(x0), "splits": splits or [],
                     "counts": {e: int(count[e]) for e in EDGES if loop.kind in APPLIES[e]}}


def noise(n, seed, sigma):
    return np.random.default_rng(seed).standard_normal(n) * sigma


def near_locked(n, seed, rate, carrier):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    return np.sin(2 * np.pi * (carrier + 3.7) * t / rate + 0.4) * (0.6 + 0.3 * np.sin(t / 500.0)) + 0.2 * rng.standard_normal(n)


# the presets' loops (psk.py:38-55 BPSK 300, :311-338 QPSK 2400, :546-569 MPSK qpsk_2400, afsk_pll.py:34-52): rate, carrier, cutoff,
# p, i, limit, gain
PRESET = {
    "bpsk": (48000.0, 1500.0, 250.0, 0.06, 0.06 / 1000, 25 * 1.25, 7200),
    "qpsk": (48000.0, 1800.0, 200.0, 0.1, 0.1 / 500, 87.5, 450.0),
    "pll": (8000.0, 1700.0, 150.0, 0.6, 0.6 / 6000, 50, 900),
    "mpsk": (48000.0, 1500.0, 250.0, 0.3, 0.3 / 2000, 25 * 1.25, 14400 / 65536),
}
# parameters that throw each loop's phase about: a low carrier, an open loop filter, a proportional term of thousands of hertz per
# unit of error (each loop's error has its own scale: a product of two mixers, one mixer, two filtered arms, a table of degrees x 32)
SLOW = {
    "bpsk": (48000.0, 100.0, 20000.0, 500.0, 0.5, 5000.0, 400.0, 1.5),
    "qpsk": (48000.0, 100.0, 20000.0, 500.0, 0.5, 5000.0, 400.0, 1.5),
    "pll": (48000.0, 100.0, 20000.0, 500.0, 0.5, 5000.0, 400.0, 1.5),
    "mpsk": (48000.0, 100.0, 20000.0, 50.0, 0.5, 5000.0, 40.0, 1.5),
}


def inputs(kind, n, seed, sigma=None, rate=48000.0, carrier=1500.0):
    if sigma is None:
        a, b = near_locked(n, seed, rate, carrier), near_locked(n, seed + 1000, rate, carrier)
    else:
        a, b = noise(n, seed, sigma), noise(n, seed + 1000, sigma)
    return (a, b) if kind == "mpsk" else (a, None)


def zero_step(kind, frequency):
    """Carrier `frequency`, p = i = 0: the control stays 0 and the phase moves by phase_scaling * frequency alone."""
    return RefLoop(kind, 48000.0, frequency, 250.0, 0.0, 0.0, 31.25, 1.0)


def phase_is(edge_at):
    def check(loop, k):
        if k in edge_at:
            assert loop.nco.phase_accumulator == TWO_PI, (k, loop.nco.phase_accumulator)
    return check


def loop_cases():
    below = math.nextafter(TWO_PI, 0.0)
    half_ulp = (TWO_PI - below) / 2
    for kind in LOOPS:
        seed = 10 * LOOPS.index(kind)
        # -- the issue's table --------------------------------------------------------------------------------------------------
        lp = zero_step(kind, -1e-12)                                    # phase alternates 2 pi (exactly) / 0.0
        lp.nco.sine_output = 0.123
        run_case("idx256", "idx256", lp, *inputs(kind, 64, seed + 1, 0.7))
        rate, carrier, cutoff, p, i, limit, gain, sigma = SLOW[kind]
        run_case("slow", "slow", RefLoop(kind, rate, carrier, cutoff, p, i, limit, gain, branch_cutoff=20000.0), *inputs(kind, 2000, seed + 2, sigma))
        lp = RefLoop(kind, *PRESET[kind])                               # the presets' loops on noise far above the AGC's level
        if kind == "mpsk":
            lp.pi.integral = -lp.pi.i_limit                             # psk.py:703: this modem starts its integral on the rail
        run_case("rails", "rails", lp, *inputs(kind, 2000, seed + 3, 200.0 if kind == "qpsk" else 40.0))
        # -- the phase next to 2 pi ---------------------------------------------------------------------------------------------
        lp = zero_step(kind, 0.0)
        lp.nco.phase_accumulator = below                                # phase * index_scaling may round to 256.0 on the fast path
        lp.nco.sine_output = -0.321
        run_case("below_2pi", "near_2pi", lp, *inputs(kind, 33, seed + 4, 0.7))
        lp = zero_step(kind, -1e-12)                                    # 2 pi after samples 0, 2, 4, ..: pieces that END on the edge
        lp.nco.sine_output = 0.5
        run_case("carry_2pi", "carry_2pi", lp, *inputs(kind, 9, seed + 5, 0.7), splits=[[1], [3], [1, 5]], check=phase_is({0, 2, 4, 8}))
        lp = zero_step(kind, -1e-12)                                    # started ON 2 pi: 2 pi again after samples 1, 3, 5, ..: the pieces
        lp.nco.phase_accumulator = TWO_PI                               # after an EVEN cut (16-byte aligned rows: the transposing
        lp.nco.sine_output = -0.5                                       # tiles of the direct shape) start from the edge
        run_case("carry_2pi_even", "carry_2pi", lp, *inputs(kind, 10, seed + 8, 0.7), splits=[[2], [4], [2, 6]], check=phase_is({1, 3, 5, 9}))
        for tag, step in (("step_lt_half_ulp", -0.9 * half_ulp), ("step_gt_half_ulp", -1.1 * half_ulp)):
            lp = zero_step(kind, 0.0)
            lp.nco.set_frequency = step / lp.nco.phase_scaling_factor
            got = lp.nco.phase_scaling_factor * lp.nco.set_frequency
            assert (-half_ulp < got < 0) if "lt" in tag else (-2 * half_ulp < got < -half_ulp), got
            lp.nco.sine_output = 0.25
            run_case(tag, "tiny_step", lp, *inputs(kind, 64, seed + 6, 0.7))
        # -- the integral started on and next to its rails (the presets' loops on a near-locked signal) -------------------------
        limit = float(PRESET[kind][5])
        for tag, start in (("int_on_hi", limit), ("int_on_lo", -limit), ("int_in_hi", math.nextafter(limit, 0.0)), ("int_in_lo", math.nextafter(-limit, 0.0))):
            lp = RefLoop(kind, *PRESET[kind])
            lp.pi.integral = start
            x0, x1 = inputs(kind, 300, seed + 7, None, PRESET[kind][0], PRESET[kind][1])
            if kind == "pll" and start < 0:
                x0 = -x0                                                # (the PLL's error is linear in its input: this one pushes down)
            run_case(tag, "integral", lp, x0, x1)
    # -- MPSK only: round()'s ties and the detector's grid ------------------------------------------------------------------------
    lp = RefLoop("mpsk", 48000.0, 1500.0, 250.0, 0.5, 0.0, 31.25, 1.0)
    lp.lpf.b_coefs = [1.0, 0.0]                                         # the loop filter passes the detector's integer through:
    lp.lpf.a_coefs = [0.0, 0.0]                                         # control = round(0.5 * e), a tie for every odd e
    run_case("ties", "ties", lp, *inputs("mpsk", 1500, 71, 0.6))
    vals = [k / 32 for k in range(-66, 67)] + [0.0, -0.0, 5e-324, -5e-324, 2.0, -2.0, 63 / 32, -63 / 32, 1e300, -1e300]
    re, im = np.meshgrid(np.array(vals), np.array(vals), indexing="ij")
    lp = zero_step("mpsk", 0.0)                                         # carrier 0, phase 0: the NCO gives (1, -0.0), re = sr and im = si
    run_case("grid", "grid", lp, re.reshape(-1), im.reshape(-1))
    g = CASES["mpsk__grid"]
    assert np.array_equal(g["out0"], g["x0"]) and np.array_equal(g["out1"], g["x1"])
    pd = PhaseDetector("qpsk", 64, 32)
    g["pd"] = np.array([pd.get_qpsk_angle_error(float(a), float(b)) for a, b in zip(g["x0"], g["x1"])], dtype=np.int32)


# ---- degenerate recordings through the reference's modems ---------------------------------------------------------------------------
def recordings(n=8000):
    rng = np.random.default_rng(77)
    sq = np.where((np.arange(n) // 16) % 2 == 0, 32767, -32768)
    imp = np.zeros(n)
    imp[n // 2] = 32767
    burst = np.zeros(n)
    burst[2500:5500] = np.clip(np.rint(rng.standard_normal(3000) * 8000), -32768, 32767)
    neg = -np.abs(np.clip(np.rint(rng.standard_normal(n) * 8000), -32768, 32767))
    recs = {"zeros": np.zeros(n), "rail_hi": np.full(n, 32767), "rail_lo": np.full(n, -32768), "square": sq, "impulse": imp,
            "burst": burst, "neg_noise": neg}
    return {k: v.astype(np.int16) for k, v in recs.items()}


def recording_cases():
    out, summ = {}, {}
    for name, audio in recordings().items():
        out[f"rec__{name}"] = audio
        with quiet():
            b = np.asarray(ref_psk.BPSKModem(sample_rate=48000.0, config="300").demod(audio), dtype=np.float64)
            m = ref_psk.MPSKModem(sample_rate=48000.0, config="qpsk_2400").demod(audio)
        mi, mq = np.asarray(m.i_data, dtype=np.float64), np.asarray(m.q_data, dtype=np.float64)
        assert np.all(np.isfinite(b)) and np.all(np.isfinite(mi)) and np.all(np.isfinite(mq))
        out[f"rec__{name}__bpsk"] = b
        out[f"rec__{name}__mpsk_i"] = mi
        out[f"rec__{name}__mpsk_q"] = mq
        summ[name] = {"n": len(audio), "n_bpsk": len(b), "n_mpsk": len(mi), "max_bpsk": float(np.abs(b).max()), "max_mpsk": float(max(np.abs(mi).max(), np.abs(mq).max()))}
    return out, summ


def check_floors(summary):
    """Each edge is hit in at least one case of each loop it applies to; the slow cases are on the slow branch for a quarter of their
    samples at least; the tie case has 100 ties at least."""
    for edge in EDGES:
        for kind in APPLIES[edge]:
            assert any(c["loop"] == kind and c["counts"].get(edge, 0) > 0 for c in summary.values()), (edge, kind)
    for name, c in summary.items():
        if c["kind"] == "slow":
            assert 4 * c["counts"]["slow"] >= c["n"], (name, c["counts"])
        if c["kind"] == "ties":
            assert c["counts"]["tie"] >= 100, (name, c["counts"])


def main():
    loop_cases()
    check_floors(SUMMARY)
    flat = {f"{case}__{k}": v for case, d in CASES.items() for k, v in d.items()}
    recs, rec_summary = recording_cases()
    for name, arrays in (("loop_edges.npz", flat), ("loop_edges_recordings.npz", recs)):
        path = os.path.join(OUT, name)
        np.savez_compressed(path, **arrays)
        assert os.path.getsize(path) < 1 << 20, (name, os.path.getsize(path))
        print(name, os.path.getsize(path), "bytes")
    with open(os.path.join(OUT, "loop_edges_summary.json"), "w") as f:
        json.dump({"edges": list(EDGES), "applies": {e: list(APPLIES[e]) for e in EDGES}, "cases": SUMMARY,
                   "recordings": rec_summary}, f, indent=1, sort_keys=True)
        f.write("\n")
    for name, c in SUMMARY.items():
        print(f"{name:28s} n={c['n']:6d} {c['counts']}")


if __name__ == "__main__":
    main()
