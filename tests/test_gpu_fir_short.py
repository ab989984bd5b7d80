"""The short-tap sign FIR -- fir_short_signs_i16_kernel<M, NEG> (pymodem_amd/csrc/pm_fir.hip), what pm_fir_signs_i16 launches for 2 to 8
taps on 16-byte aligned int16 audio, and the front of every FSK chain -- where tap counts, ties and rails decide: every template, both
flags, on the inputs of tests/fir_sign_inputs.py (rounding residues whose sign belongs to the canonical summation order alone, exact zeros
alone and in runs, both rails, every int16 value, subnormal and huge taps), at the lengths where the scalar tail, the last byte's valid
mask, the word, a round of a workgroup's lanes and a workgroup end.  tests/test_fir_sign_inputs.py holds without a GPU that the inputs
are what they claim.

Every comparison is exact, against the oracle's canonical sum (O.fir_canon: one fma per tap, ascending input index, from +0).  Every
call sees its audio in an allocation that goes on with 32 samples of 32767 behind the n it is given, and a bitmap pre-filled with a
pattern: the bits of [0, nout) are the oracle's, the padding bits up to the end of the last 64-bit word are 0, the word behind it is
untouched.  Then the FSK stage itself at the sample rates that give the '9600' preset 2 to 8 taps, through demod_signs(), the slicer, the
whole-chain C entry point and carried history."""
import functools

import numpy as np
import pytest

import fir_sign_inputs as F
from conftest import tuned
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SENTINELS = 32
FILL = 0xA5A5A5A5A5A5A5A5
FLAGS = [0, 1]                                  # PM_FIR_NEGATE
LENGTHS = (100, 4097, 2 * 16384 + 777)          # outputs: a partial tail, more than one round, more than two workgroups


@pytest.fixture(scope="module")
def ctx():
    import pymodem_amd
    if pymodem_amd.lib().pm_device_count() < 1:
        pytest.fail("no GPU visible: -m gpu tests need an MI355X")
    return pymodem_amd.Context.default()


def L():
    import pymodem_amd
    return pymodem_amd.lib()


def chk(rc):
    from pymodem_amd._native import check
    check(rc)


def upload_with_sentinels(ctx, x, offset=0):
    """x as a view `offset` samples into its allocation, with the sentinels behind it."""
    host = np.concatenate([np.full(offset, -12345, np.int16), x, np.full(SENTINELS, 32767, np.int16)])
    return ctx.upload(host).view(offset, len(x))


def signs_i16(ctx, x, h, flags=0, offset=0):
    """pm_fir_signs_i16 -> the bits of [0, nout); the padding bits and the word behind the bitmap are checked on the way."""
    n, m = len(x), len(h)
    nout = n - m + 1
    words = (nout + 63) // 64
    dx, dh = upload_with_sentinels(ctx, x, offset), ctx.upload(np.ascontiguousarray(h, dtype=np.float64))
    bits = ctx.upload(np.full(words + 1, FILL, np.uint64))
    chk(L().pm_fir_signs_i16(ctx.handle, dx.ptr, n, dh.ptr, m, bits.ptr, flags))
    got = bits.download()
    assert got[words] == FILL, ("the word behind the bitmap was written", m, n, flags, hex(int(got[words])))
    unpacked = np.unpackbits(got[:words].view(np.uint8), bitorder="little")
    assert not unpacked[nout:].any(), ("padding bits set", m, n, flags, np.flatnonzero(unpacked[nout:])[:8] + nout)
    return unpacked[:nout].astype(bool)


def valid_i16(ctx, x, h, flags=0):
    dx, dh = upload_with_sentinels(ctx, x), ctx.upload(np.ascontiguousarray(h, dtype=np.float64))
    y = ctx.empty(len(x) - len(h) + 1, np.float64)
    chk(L().pm_fir_valid_i16(ctx.handle, dx.ptr, len(x), dh.ptr, len(h), y.ptr, flags))
    return y.download()


@functools.lru_cache(maxsize=None)
def cases(family, m, nout):
    """[(name, audio, taps, canonical sum)] of a family: made once, shared by the tests, never written to."""
    out = []
    for name, x, h in F.FAMILIES[family](m, nout + m - 1):
        y = O.fir_canon(x, h)
        for a in (x, h, y):
            a.setflags(write=False)
        out.append((name, x, h, y))
    return out


@functools.lru_cache(maxsize=1)
def every_value_case(m):
    (name, x, h), = F.every_value(m)
    return name, x, h, O.fir_canon(x, h)


def want_of(y, flags):
    return (-y if flags else y) >= 0


def same_bits(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, "wrong bits:", bad.size, "first at", bad[:8])


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("m", F.SHORT_M)
@pytest.mark.parametrize("family", sorted(F.FAMILIES))
def test_every_family_at_every_tap_count(ctx, family, m, flags):
    for nout in LENGTHS:
        for name, x, h, y in cases(family, m, nout):
            same_bits(signs_i16(ctx, x, h, flags), want_of(y, flags), (name, m, nout, flags))


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("m", F.SHORT_M)
def test_every_int16_value_is_converted_exactly(ctx, m, flags):
    """65536 plateaus, one per sample value: the sign of a plateau's residue is that of the canonical sum only if the kernel's own
    int16 -> binary64 conversion gave (double)x."""
    name, x, h, y = every_value_case(m)
    same_bits(signs_i16(ctx, x, h, flags), want_of(y, flags), (name, m, flags))


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("m", F.SHORT_M)
def test_every_length_of_the_last_bytes(ctx, m, flags):
    """n = m .. m + 48: one to 49 outputs -- all eight valid masks of the last byte, and the byte at which the loads change from two
    16-byte ones to sample by sample moves through the stream."""
    (name, x, h, y), = cases("plateau", m, 49)
    for n in range(m, m + 49):
        nout = n - m + 1
        same_bits(signs_i16(ctx, x[:n], h, flags), want_of(y[:nout], flags), (name, m, "n", n, flags))


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("m", F.SHORT_M)
def test_word_round_and_workgroup_edges(ctx, m, flags):
    """Outputs up to, at and behind the end of a 64-bit word, of one round of a workgroup's lanes (2048) and of its eight rounds (16384)."""
    (name, x, h, y), = cases("plateau", m, 16385)
    for nout in (63, 64, 65, 127, 128, 129, 2047, 2048, 2049, 16383, 16384, 16385):
        same_bits(signs_i16(ctx, x[:nout + m - 1], h, flags), want_of(y[:nout], flags), (name, m, "nout", nout, flags))


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("m", F.SHORT_M)
def test_views_into_an_allocation(ctx, m, flags):
    """8 samples in, the start is still 16-byte aligned (the short kernel); 1 and 4 samples in it is not (the LDS kernel): the bits of
    the aligned call on the same samples."""
    for family in sorted(F.FAMILIES):
        for name, x, h, y in cases(family, m, 4097):
            base = signs_i16(ctx, x, h, flags)
            same_bits(base, want_of(y, flags), (name, m, flags, "offset", 0))
            for offset in (8, 1, 4):
                same_bits(signs_i16(ctx, x, h, flags, offset=offset), base, (name, m, flags, "offset", offset))


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("m", F.SHORT_M)
@pytest.mark.parametrize("family", sorted(F.FAMILIES))
def test_three_ways_one_answer(ctx, family, m, flags):
    """The short kernel, the LDS kernel (fir_no_short) and the float kernel's output through >= 0; the float output itself is the
    canonical sum, negated under the flag, zeros with their sign."""
    for name, x, h, y in cases(family, m, 4097):
        what = (name, m, flags)
        want = want_of(y, flags)
        same_bits(signs_i16(ctx, x, h, flags), want, what + ("short",))
        with tuned(ctx, fir_no_short=1):
            same_bits(signs_i16(ctx, x, h, flags), want, what + ("LDS",))
        out = valid_i16(ctx, x, h, flags)
        ref = -y if flags else y
        assert np.array_equal(out, ref), what + ("float", int(np.count_nonzero(out != ref)))
        assert np.array_equal(np.signbit(out), np.signbit(ref)), what + ("signs of the float zeros",)
        same_bits(out >= 0, want, what + ("float >= 0",))


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("m", [1, 9, 10, 11, 12, 13, 14, 15])
def test_ties_just_outside_the_short_kernels_window(ctx, m, flags):
    """The LDS kernel's int16 sign path at the tap counts next to the short kernel's ('4800' at 44.1 and 48 kHz is 14 and 15 taps)."""
    for family in ("rails", "palindromes", "plateau"):
        for name, x, h, y in cases(family, m, 4097):
            same_bits(signs_i16(ctx, x, h, flags), want_of(y, flags), (name, m, flags))


# ---- the FSK stage at every tap count ----------------------------------------------------------------------------------------------------
RATES = [16000, 19200, 24000, 32000, 38400, 44100, 48000]           # '9600': round(1.5 * rate / 9600) = 2 .. 8 taps


def fsk_pair(rate, invert):
    from pymodem_amd.modems import FSKModem
    from pymodem_amd.slicer import BinarySlicer
    modem = FSKModem(sample_rate=rate, config="9600")
    modem.StringOptionsRetune({"invert": "true" if invert else "false"})
    slicer = BinarySlicer(sample_rate=rate, config="9600")
    assert slicer.lock_rate == 0.88
    return modem, slicer


@functools.lru_cache(maxsize=None)
def fsk_oracle(rate, invert):
    """-> (audio, taps, the oracle's demodulated stream, its slicer bytes, their addresses)."""
    audio = F.squelch()
    om = O.FSKModem(rate, "9600", {"invert": "true" if invert else "false"})
    stream = om.demod(audio, canon=True)
    data, addr = O.BinarySlicer(rate, "9600").slice(stream)
    for a in (audio, stream, data, addr):
        a.setflags(write=False)
    return audio, om.input_lpf, stream, data, addr


def same_slices(got, data, addr, what):
    assert np.array_equal(got.data, data), (what, "bytes", len(got.data), len(data))
    assert np.array_equal(got.address, addr), (what, "addresses")


@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("rate", RATES)
def test_fsk_stage_at_every_tap_count(ctx, rate, invert):
    from pymodem_amd import chain_execute as ce
    m = 2 + RATES.index(rate)
    audio, taps, stream, data, addr = fsk_oracle(rate, invert)
    modem, slicer = fsk_pair(rate, invert)
    assert len(modem.input_lpf) == m and modem.invert == invert
    assert np.array_equal(modem.input_lpf, taps)
    assert len(data) >= 30000 * 9600 // (8 * rate) - 8 and len(addr) == len(data)
    # the stage: the bits of the oracle's stream
    sb = modem.demod_signs(audio)
    assert sb.n == len(audio) - m + 1 and sb.bits_q is None
    got = np.unpackbits(sb.bits_i.download().view(np.uint8), bitorder="little")[:sb.n].astype(bool)
    same_bits(got, stream >= 0, (rate, invert, "demod_signs"))
    # the slicer on them, as the executors hand them over
    same_slices(slicer.slice(sb), data, addr, (rate, invert, "slicer"))
    # the whole-chain entry point, from host audio and from a device buffer
    modem2, slicer2 = fsk_pair(rate, invert)
    nc = ce.NativeChain(modem2, slicer2)
    same_slices(nc.run(audio), data, addr, (rate, invert, "native, host audio"))
    nc.reset()
    same_slices(nc.run(ctx.upload(audio)), data, addr, (rate, invert, "native, device audio"))
    nc.close()


@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("rate", RATES)
def test_fsk_stage_in_pieces_with_carried_history(ctx, rate, invert):
    """carry_history: pieces of 1, m - 1, m, 7 and 4096 samples and the rest give the single call's slicer bytes and addresses; a piece
    that leaves [tail | piece] shorter than the filter gives nothing."""
    m = 2 + RATES.index(rate)
    audio, taps, stream, data, addr = fsk_oracle(rate, invert)
    modem, slicer = fsk_pair(rate, invert)
    assert len(modem.input_lpf) == m
    modem.carry_history = True
    got_d, got_a, fed, out = [], [], 0, 0
    sizes = [1, m - 1, m, 7, 4096]
    sizes.append(len(audio) - sum(sizes))
    for k, size in enumerate(sizes):
        sb = modem.demod_signs(audio[fed:fed + size])
        fed += size
        assert sb.n == max(0, fed - m + 1) - out, (rate, invert, "piece", k, size, sb.n)
        out += sb.n
        if k == 0:
            assert sb.n == 0                                  # one sample: starved for every m >= 2
        sliced = slicer.slice(sb)
        got_d.append(np.array(sliced.data))
        got_a.append(np.array(sliced.address))
    assert fed == len(audio) and out == len(stream)
    assert len(got_d[0]) == 0 and len(got_a[0]) == 0
    assert np.array_equal(np.concatenate(got_d), data), (rate, invert, "bytes")
    assert np.array_equal(np.concatenate(got_a), addr), (rate, invert, "addresses")
