"""tests/fir_sign_inputs.py against the oracle alone: the inputs have the properties tests/test_gpu_fir_short.py relies on.  These are
conditions, not measurements: a later change to a family cannot quietly make it harmless.  (Measured with the families as they are, at
n = 4096 + m for m = 2..8: 2305 to 3826 of the 4097 plateau outputs are residues below 1e-6, every one of them with the other sign under
the descending sum, and 937 to 1877 differ in sign from numpy.convolve's; the palindromes give 65 lone exact zeros for every m.)"""
import numpy as np
import pytest

import fir_sign_inputs as F
from oracle import oracle as O

N_OUT = 4097


def one(cases):
    assert len(cases) == 1
    return cases[0]


@pytest.mark.parametrize("m", F.SHORT_M)
def test_plateau_outputs_are_residues_of_this_summation_order(m):
    _, x, h = one(F.plateau(m, N_OUT + m - 1))
    assert x.dtype == np.int16 and len(x) == N_OUT + m - 1 and len(h) == m and np.array_equal(h, -h[::-1])
    y = O.fir_canon(x, h)
    assert len(y) == N_OUT
    residue = (y != 0) & (np.abs(y) < 1e-6)
    assert np.count_nonzero(residue) >= N_OUT // 4 + 1, np.count_nonzero(residue)
    other = F.descending_sum(x, h)
    flipped = np.signbit(y) != np.signbit(other)
    assert np.count_nonzero(flipped) >= N_OUT // 4 + 1, np.count_nonzero(flipped)
    # and so the two flags' bitmaps are not each other's complement, and neither is the bitmap of another order
    assert not np.array_equal(F.want_bits(x, h, 0), other >= 0)


@pytest.mark.parametrize("m", F.SHORT_M)
def test_constant_inputs_give_plus_zero_everywhere(m):
    cases = F.rails(m, N_OUT + m - 1)
    assert sorted(int(c[1][0]) for c in cases) == [-32768, 0, 1, 32767]
    for name, x, h in cases:
        assert np.all(x == x[0]) and h.sum() == 0.0 and np.array_equal(h * 64, np.rint(h * 64)) and np.count_nonzero(h) >= 2, name
        y = O.fir_canon(x, h)
        assert len(y) == N_OUT and not y.any() and not np.signbit(y).any(), name
        assert F.want_bits(x, h, 0).all() and F.want_bits(x, h, 1).all(), name


@pytest.mark.parametrize("m", F.SHORT_M)
def test_palindromes_give_lone_exact_zeros(m):
    _, x, h = one(F.palindromes(m, N_OUT + m - 1))
    assert np.array_equal(h, -h[::-1]) and np.array_equal(h * 64, np.rint(h * 64)) and h.any()
    y = O.fir_canon(x, h)
    zero = y == 0
    lone = zero[1:-1] & ~zero[:-2] & ~zero[2:]
    assert np.count_nonzero(lone) >= 16, (m, np.count_nonzero(lone))
    assert not np.signbit(y[zero]).any()
    # both signs stand beside the zeros: a zero counted as negative, or as positive under NEGATE, would show
    assert (y < 0).any() and (y > 0).any()


@pytest.mark.parametrize("m", F.SHORT_M)
def test_silence_has_empty_windows_and_windows_with_one_sample(m):
    _, x, h = one(F.silence(m, N_OUT + m - 1))
    live = np.convolve((x != 0).astype(np.int64), np.ones(m, np.int64), "valid")
    assert len(live) == N_OUT and (live == 0).any() and (live == 1).any() and (live == m).any()
    edges = np.flatnonzero(np.diff(np.concatenate([[0], (x == 0).astype(np.int8), [0]])))
    assert set(range(1, 21)) <= set((edges[1::2] - edges[::2]).tolist())                     # runs shorter than, equal to and longer than m
    y = O.fir_canon(x, h)
    assert np.array_equal(y == 0, live == 0) and not np.signbit(y[live == 0]).any()


@pytest.mark.parametrize("m", F.SHORT_M)
def test_every_value_occurs(m):
    _, x, h = one(F.every_value(m))
    assert x.dtype == np.int16 and len(x) == 65536 * F.HOLD and len(np.unique(x)) == 65536
    held = x.reshape(-1, F.HOLD)
    assert (held == held[:, :1]).all()
    assert np.array_equal(h, F.plateau(m, 64)[0][2])


@pytest.mark.parametrize("m", F.SHORT_M)
def test_alternating_and_extreme_inputs_are_what_they_say(m):
    n = N_OUT + m - 1
    alt = F.alternating(m, n)
    assert len(alt) == 2 * len({2, 3, m})
    for name, x, h in alt:
        assert set(np.unique(x).tolist()) == {-32768, 32767} and len(x) == n and len(h) == m, name
    ext = dict((name, (x, h)) for name, x, h in F.extreme(m, n))
    tiny = ext["subnormal taps"][1]
    assert np.all(np.abs(tiny) < np.finfo(np.float64).tiny) and tiny.any()
    assert np.abs(ext["taps near 1e300"][1]).max() > 1e298 and np.isfinite(O.fir_canon(*ext["taps near 1e300"])).all()
    holes = ext["taps with zeros"][1]
    assert (holes == 0).any() and (holes != 0).any()
    for name, (x, h) in ext.items():
        assert np.isfinite(h).all(), name
        y = O.fir_canon(x, h)
        assert (y < 0).any() and (y > 0).any(), name


def test_squelch_has_silence_and_both_rails():
    x = F.squelch()
    assert x.dtype == np.int16 and len(x) == 30000
    assert (x == 32767).sum() > 10 and (x == -32768).sum() > 10
    zero = np.concatenate([[0], (x == 0).astype(np.int8), [0]])
    edges = np.flatnonzero(np.diff(zero))
    assert np.count_nonzero((edges[1::2] - edges[::2]) >= 200) == 2
    quiet = np.abs(x.astype(np.float64)) < 32767
    assert 3000 < x[quiet].std() < 6000
