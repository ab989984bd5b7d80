"""The oracle's carrier loops against the reference where their quantisers and branches decide (tests/golden/loop_edges.npz, made by
tests/golden/make_loop_edges.py from the reference's own NCO, IIR_1, PI_control and PhaseDetector): table index 256, a negative phase
and more than a turn per sample, round()'s ties, the integral on and next to its rails, the detector's clip and quadrant fold on its
grid.  The loops contain no FIR, so the contract is equality: `==` on every output sample and every field of the
end state, whole and with the state carried across two and three calls.  The oracle's modems on seven degenerate recordings follow
the FIR rule of test_oracle_chains.py."""
import numpy as np
import pytest

import loop_edges as E
from oracle import oracle as O

TOL = 1e-9


@pytest.mark.parametrize("name", sorted(E.CASES))
def test_loop_equals_the_reference(name):
    c = E.case(name)
    assert len(c["x0"]) == E.CASES[name]["n"]
    for cuts in E.cuts_of(name):
        o0, o1, state, br = E.oracle_case(name, cuts)
        assert np.array_equal(o0, c["out0"]), (name, cuts)
        if "out1" in c:
            assert np.array_equal(o1, c["out1"]), (name, cuts)
        for f, got, want in zip(E.STATE, state, c["state1"]):
            assert got == want, (name, cuts, f, got, want)
        if "branch1" in c:
            assert np.array_equal(br, c["branch1"]), (name, cuts)


def test_the_two_thirds_of_a_case_are_real_pieces():
    """Every case longer than two samples is really run in two and in three pieces, and carry_2pi ends pieces on the edge."""
    for name, s in E.CASES.items():
        if s["n"] >= 3:
            assert {0, 1, 2} <= {len(c) for c in E.cuts_of(name)}, name
    assert [1] in E.cuts_of("bpsk__carry_2pi") and [1, 5] in E.cuts_of("mpsk__carry_2pi") and [2, 6] in E.cuts_of("qpsk__carry_2pi_even")


def test_detector_grid():
    """phase_detector.py:124-149 on every pair of its grid: k/32 for |k| <= 66, +-0.0, +-5e-324, +-2, +-63/32, +-1e300."""
    c = E.case("mpsk__grid")
    vals = set(c["x0"].tolist())
    assert {k / 32 for k in range(-66, 67)} <= vals and {5e-324, -5e-324, 1e300, -1e300} <= vals
    assert len(c["x0"]) == 143 * 143 and np.any(np.signbit(c["x0"]) & (c["x0"] == 0)) and np.any(np.signbit(c["x1"]) & (c["x1"] == 0))
    assert np.array_equal(O.pd_lookup(c["x0"], c["x1"]), c["pd"])
    assert len(np.unique(c["pd"])) > 100


def test_every_edge_is_reached():
    """The floors of the generator, again from what it recorded: each edge in at least one case of each loop it applies to, the slow
    cases on the slow branch for a quarter of their samples, a hundred ties."""
    for edge in E.SUMMARY["edges"]:
        for kind in E.SUMMARY["applies"][edge]:
            assert any(s["loop"] == kind and s["counts"].get(edge, 0) > 0 for s in E.CASES.values()), (edge, kind)
    assert set(E.SUMMARY["applies"]["slow"]) == set(E.LOOPS) == set(E.SUMMARY["applies"]["idx256"]) == set(E.SUMMARY["applies"]["rail"])
    assert E.SUMMARY["applies"]["tie"] == ["mpsk"] == E.SUMMARY["applies"]["clip"]
    slow = [s for s in E.CASES.values() if s["kind"] == "slow"]
    assert sorted(s["loop"] for s in slow) == sorted(E.LOOPS)
    for s in slow:
        assert 4 * s["counts"]["slow"] >= s["n"], s
    for name, s in E.CASES.items():                            # the cases named after a rail reach it
        if "__int_" in name:
            assert s["counts"]["rail"] > 0, name
    ties = [s for s in E.CASES.values() if s["kind"] == "ties"]
    assert ties and all(s["counts"]["tie"] >= 100 for s in ties)
    for kind in E.LOOPS:                                       # the cases the issue names, for every loop
        for tag in ("idx256", "slow", "rails", "below_2pi", "carry_2pi", "carry_2pi_even", "step_lt_half_ulp", "step_gt_half_ulp",
                    "int_on_hi", "int_on_lo", "int_in_hi", "int_in_lo"):
            assert f"{kind}__{tag}" in E.CASES


RECORDINGS = sorted(E.SUMMARY["recordings"])


@pytest.mark.parametrize("name", RECORDINGS)
def test_modems_on_degenerate_recordings(name):
    """BPSKModem("300") and MPSKModem("qpsk_2400") at 48 kHz on zeros, both rails, a full-scale square, one impulse, a burst between
    silences and negative-only noise, in the reference's default FIR order, every sample: within 1e-9 of max|y| and the same sign wherever |y| exceeds
    that bound."""
    g, s = E.recordings(), E.SUMMARY["recordings"][name]
    audio = g[f"rec__{name}"]
    assert len(audio) == s["n"] and audio.dtype == np.int16
    b = O.BPSKModem(48000.0, "300").demod(audio)
    mi, mq = O.MPSKModem(48000.0, "qpsk_2400").demod(audio)
    assert len(b) == s["n_bpsk"] and len(mi) == len(mq) == s["n_mpsk"]
    for got, key in ((b, "bpsk"), (mi, "mpsk_i"), (mq, "mpsk_q")):
        want = g[f"rec__{name}__{key}"]
        assert len(want) == len(got)
        assert np.all(np.isfinite(got))
        bound = TOL * np.abs(want).max()
        assert np.abs(got - want).max() <= bound, (name, key)
        big = np.abs(want) > bound
        assert np.array_equal(got[big] >= 0, want[big] >= 0), (name, key)
