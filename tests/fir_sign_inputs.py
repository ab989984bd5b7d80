"""Inputs on which the short-tap sign FIR (fir_short_signs_i16_kernel, pymodem_amd/csrc/pm_fir.hip, behind pm_fir_signs_i16 for 2 to 8 taps)
decides at a tie, at a rail or on a rounding residue -- for tests/test_gpu_fir_short.py, and for tests/test_fir_sign_inputs.py, which
holds without a GPU that the inputs have the properties the GPU tests rely on.

Every function returns cases (name, int16 audio of n samples, float64 taps of m entries); everything is seeded by the family and m, never
by n.  The expected bits are want_bits(): the sign of the oracle's canonical sum (O.fir_canon: one fma per tap, ascending input index,
from +0), which is not restated here.

  plateau       antisymmetric taps that are no binary fractions on noise held for 16 samples: on a constant window the true sum is 0 and
                the canonical sum is the rounding residue of the first products -- its sign belongs to this summation order alone
  every_value   the same taps on each of the 65536 int16 values once, held for 16 samples: the residue's sign depends on the exactly
                converted sample, for every sample value
  rails         binary-fraction taps that sum to 0 on constant -32768, 32767, 1 and 0: every product and partial sum is exact, every output
                is +0, and +0 is ">= 0" with and without NEGATE
  palindromes   antisymmetric binary-fraction taps on palindromes of noise, centred between two samples and on a sample: lone exact zeros
                between nonzero neighbours, for even and for odd tap counts
  silence       noise with runs of 1 to 20 exact zeros (a squelched receiver): windows that are all zero, and windows with one sample left
  alternating   the two rails in turn, with period 2, 3 and m; taps all ones, or random
  extreme       noise through subnormal taps, taps near 1e300, and taps of which some are exactly 0

Taps are finite by contract (they are designed filters): infinite and NaN taps are outside it and are in no family here.
"""
import numpy as np

from conftest import noise_i16
from oracle import oracle as O

SHORT_M = (2, 3, 4, 5, 6, 7, 8)            # the tap counts pm_fir_signs_i16 gives to fir_short_signs_i16_kernel
HOLD = 16                                  # samples per plateau: longer than any window of the short kernel's neighbours up to 15 taps
HI, LO = 32767, -32768


def want_bits(x, h, flags=0):
    """The bits pm_fir_signs_* must give: (-y if NEGATE else y) >= 0 of the canonical sum."""
    y = O.fir_canon(x, h)
    return (-y if flags else y) >= 0


def descending_sum(x, h):
    """The same FIR summed from the other end of the window (the canonical sum of the reversed problem, reversed back)."""
    return O.fir_canon(np.ascontiguousarray(x[::-1]), np.ascontiguousarray(h[::-1]))[::-1]


def _rng(family, m):
    return np.random.default_rng([family, m])


def antisymmetric_taps(m, rng):
    t = 0.3 * rng.standard_normal(m // 2)
    return np.concatenate([t, np.zeros(m % 2), -t[::-1]])


def dyadic(v):
    return np.rint(64.0 * v) / 64.0


def plateau(m, n):
    h = antisymmetric_taps(m, _rng(1, m))
    x = np.repeat(noise_i16((n + HOLD - 1) // HOLD, seed=1000 + m, sigma=9000.0), HOLD)[:n]
    return [("plateau", x, h)]


def every_value(m):
    """n = 65536 * 16 = 1 048 576."""
    rng = _rng(2, m)
    h = antisymmetric_taps(m, _rng(1, m))
    values = np.arange(LO, HI + 1, dtype=np.int32).astype(np.int16)
    return [("every-value", np.repeat(rng.permutation(values), HOLD), h)]


def rails(m, n):
    h = dyadic(_rng(3, m).standard_normal(m))
    h[-1] = -h[:-1].sum()
    return [(f"constant {v}", np.full(n, v, np.int16), h) for v in (LO, HI, 1, 0)]


def palindromes(m, n):
    """Tiles of fresh noise p (16 samples) as [p, p reversed] (32 samples, centred between two) and [p, p reversed without its first]
    (31 samples, centred on p's last) in turn: an even window meets the first centre, an odd one the second."""
    rng = _rng(4, m)
    a = dyadic(rng.standard_normal(m))
    h = a - a[::-1]
    tiles, have, k = [], 0, 0
    while have < n:
        p = noise_i16(HOLD, seed=4000 + 64 * m + k, sigma=9000.0)
        tiles.append(np.concatenate([p, p[::-1]]) if k % 2 == 0 else np.concatenate([p, p[-2::-1]]))
        have += len(tiles[-1])
        k += 1
    return [("palindromes", np.concatenate(tiles)[:n], h)]


def silence(m, n):
    x = noise_i16(n, seed=5000 + m)
    x[x == 0] = 1                                             # the only zeros are the runs'
    at, run = 9, 1
    while at < n:
        x[at:at + run] = 0
        at += run + 9
        run = run % 20 + 1
    return [("silence", x, _rng(5, m).standard_normal(m))]


def alternating(m, n):
    """Period p: the upper rail for the first (p + 1) // 2 samples of a period, the lower for the rest."""
    r = _rng(6, m).standard_normal(m)
    cases = []
    for p in sorted({2, 3, m}):
        x = np.where(np.arange(n) % p < (p + 1) // 2, HI, LO).astype(np.int16)
        cases += [(f"alternating period {p}, ones", x, np.ones(m)), (f"alternating period {p}, random", x, r)]
    return cases


def extreme(m, n):
    rng = _rng(7, m)
    x = noise_i16(n, seed=7000 + m)
    r = rng.standard_normal(m)
    holes = rng.standard_normal(m)
    holes[::2] = 0.0
    return [("subnormal taps", x, r * 1e-310), ("taps near 1e300", x, r * 1e300), ("taps with zeros", x, holes)]


FAMILIES = {"plateau": plateau, "rails": rails, "palindromes": palindromes, "silence": silence, "alternating": alternating,
            "extreme": extreme}


def squelch(n=30000, seed=96):
    """A receiver with its squelch at work: band-limited noise (N(0,1) through a 6-point Hann window, sigma about 4000), two stretches of
    200 exact zeros, and two bursts that clip at both rails."""
    rng = np.random.default_rng(seed)
    v = np.convolve(rng.standard_normal(n + 5), np.hanning(6), "valid")
    v *= 4000.0 / v.std()
    v[n // 5:n // 5 + 1500] *= 12.0
    v[3 * n // 5:3 * n // 5 + 1501] *= 40.0
    x = np.clip(np.rint(v), LO, HI).astype(np.int16)
    x[n // 3:n // 3 + 200] = 0
    x[4 * n // 5 + 3:4 * n // 5 + 203] = 0
    return x
