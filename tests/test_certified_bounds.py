"""The certified-sign bound of fir8_kernel (pymodem_amd/csrc/pm_fir8.hip) on the CPU, through its bit-faithful model
(tests/fir8_model.py): on inputs built so that every error term of the bound reaches its worst case at once, the approximate sum y~ must
stay within E of the canonical binary64 sum (oracle.fir_canon) -- the proof in the source comment, checked where it is tight -- and the
inputs must actually come near E and land outputs on both sides of it, or the GPU test that replays them
(tests/test_gpu_certified_edges.py) would prove nothing about the decision rule."""
import numpy as np
import pytest

import fir8_model as F
from oracle import oracle as O


@pytest.fixture(scope="module")
def cases():
    out = []
    for name, plan, rows, dirs in F.adversarial_cases(O.fir_canon):
        res = [plan.run(r) for r in rows]
        yt = np.array([r["yt"][0] for r in res])
        E = np.array([r["E"][0] for r in res])
        Eb = np.array([r["Ebound"][0] for r in res])
        fl = np.array([r["flagged"][0] for r in res])
        y = np.array([O.fir_canon(r, plan.h)[0] for r in rows])
        out.append((name, plan, rows, dirs, yt, E, Eb, fl, y))
    return out


def test_the_bound_holds_on_the_adversary_and_the_adversary_comes_near_it(cases):
    """|y~ - y| <= (c1 Xmax + c2 2^-s2) 2^-S for every output; the worst output reaches 0.97 of that bound when this was written
    (BPSK 300's 961 taps: 0.972; QPSK 2400's 241: 0.956; m = 16: 0.81) -- the floor is half of it, so that a generator that stops lining
    the terms up fails here instead of silently weakening the GPU test."""
    worst = 0.0
    for name, plan, rows, dirs, yt, E, Eb, fl, y in cases:
        assert np.isfinite(yt).all(), name
        err = yt - y
        assert (np.abs(err) <= Eb).all(), (name, float(np.max(np.abs(err) / Eb)))
        assert (Eb <= E).all(), name                          # what the kernel compares with is the bound, rounded up
        # the error goes the way the generator pushed it: the terms really are lined up
        assert (np.sign(err) == dirs).all(), name
        worst = max(worst, float(np.max(np.abs(err) / Eb)))
    assert worst >= 0.486, worst


def test_the_adversary_lands_outputs_on_both_sides_of_the_bound(cases):
    """At least K = 200 outputs the kernel must flag (|y~| <= E) and K it must certify with E < |y~| < 2E: the rule is exercised
    where a wrong constant or comparison changes it."""
    inside = sum(int(np.count_nonzero(np.abs(yt) <= E)) for *_, yt, E, Eb, fl, y in cases)
    band = sum(int(np.count_nonzero((np.abs(yt) > E) & (np.abs(yt) < 2 * E))) for *_, yt, E, Eb, fl, y in cases)
    assert inside >= 200 and band >= 200, (inside, band)
    for name, plan, rows, dirs, yt, E, Eb, fl, y in cases:
        assert np.array_equal(fl, ~(np.abs(yt) > E)), name
        # a certified output's sign is the canonical sum's
        assert np.array_equal((yt > 0)[~fl], (y >= 0)[~fl]), name
        # and some certified outputs sit on the other side of zero from y~ - y: only the bound keeps their sign right
        assert np.count_nonzero(fl & (np.sign(yt) != np.sign(y))) > 0, name


@pytest.mark.parametrize("m", [16, 241, 961, 1009])
def test_the_model_agrees_with_the_canonical_sum_on_noise(m):
    """Plain inputs, several workgroups per row (8192 outputs each), one window of zeros, one window with a NaN: wherever the model
    certifies, its sign is fir_canon's and its error within the bound; the exempt windows are flagged whole (or set, for zeros)."""
    rng = np.random.default_rng(m)
    h = F.window_taps(m, rng)
    plan = F.Plan(h)
    n = 3 * F.KWG_OUT + 1000 + m
    x = rng.standard_normal(n) * np.exp(rng.uniform(-3, 3))
    x[F.KWG_OUT:2 * F.KWG_OUT + plan.window] = 0.0           # the second workgroup's window is all zeros
    x[-500] = np.nan                                          # and the last one's holds a NaN
    r = plan.run(x)
    with np.errstate(invalid="ignore"):
        y = O.fir_canon(x, h)
    ok = ~r["flagged"]
    assert np.array_equal(r["sign"][ok], (y >= 0)[ok])
    fin = ok & np.isfinite(r["Ebound"]) & np.isfinite(y)
    assert (np.abs(r["yt"][fin] - y[fin]) <= r["Ebound"][fin]).all()
    wg = lambda k: slice(k * F.KWG_OUT, min((k + 1) * F.KWG_OUT, len(y)))
    assert r["sign"][wg(1)].all() and not r["flagged"][wg(1)].any()
    assert r["flagged"][wg(3)].all()
    assert np.count_nonzero(r["flagged"][wg(0)]) < 0.01 * F.KWG_OUT
