"""What tests/test_gpu_fused_instances.py and tests/test_gpu_certified_edges.py share: chain groups that plan to each of the twelve
instances <KB, ONE0, NS, ONE1> of afsk_fused8_kernel (pm_afsk.hip: KB blocks of the band-pass plan, NS sweeps, ONEk: sweep k is a lone
tone-template chain) and to the two limits past which a group takes the split path, as config-line dicts made from a line of
golden/configs/afsk_1200.json (and lines of afsk_300_ax25.json as they are); the executor's partition of such a group worked out
without a device; the clipped two-tone signal, the 1e-10 term of a sweep's bound, and the comparison of a finished recording with the
oracle."""
import collections
import copy
import functools
import json
import os

import numpy as np

from conftest import GOLDEN
from oracle import oracle as O


def config_lines(name):
    with open(os.path.join(GOLDEN, "configs", name)) as f:
        return [l for l in (json.loads(s) for s in f if s.strip()) if l.get("object_type") == "demod_chain"]


BASE_1200 = config_lines("afsk_1200.json")[0]
LINES_300 = config_lines("afsk_300_ax25.json")


def line(**options):
    """BASE_1200 with modem options overridden (mark_freq, space_freq, space_gain, correlator_span, output_lpf_span, input_bpf_span)."""
    l = copy.deepcopy(BASE_1200)
    l["modem"]["options"].update({k: str(v) for k, v in options.items() if v is not None})
    return l


def sweep(gains, span, lpf_span=None, bpf_span=None):
    """One sweep's lines: a correlator of `span` symbols (m = 40 span at 48 kHz) on tones of its own -- sweeps of one shape differ in
    their mark templates, so each is a group of its own -- and a chain per gain."""
    mark, space = (1200.0, 2200.0) if span <= 1.0 else (1300.0, 2100.0)
    return [line(mark_freq=mark, space_freq=space, space_gain=g, correlator_span=span, output_lpf_span=lpf_span, input_bpf_span=bpf_span) for g in gains]


G2, G3, G8 = (1.0, 1.75), (0.5, 1.0, 1.75), (0.25, 0.5, 0.75, 1.0, 1.4, 1.75, 2.2, 2.8)
LONE = (1.0,)

# rate, lines in sweep order, band-pass taps, [(chains, m, ml)] per sweep, the instance (None: the group does not fuse)
Shape = collections.namedtuple("Shape", "rate lines mb sweeps instance")


def _shape(mb, bpf_span, parts, instance):
    """parts: [(gains, correlator span, m, low-pass span or None, ml)]"""
    lines = [l for gains, span, m, lpf_span, ml in parts for l in sweep(gains, span, lpf_span, bpf_span)]
    return Shape(48000, lines, mb, [(len(gains), m, ml) for gains, span, m, lpf_span, ml in parts], instance)


SHAPES = {
    "A": _shape(148, None, [(LONE, 1.0, 40, None, 100)], (3, True, 1, False)),
    "B": _shape(148, None, [(G2, 1.5, 60, None, 100)], (3, False, 1, False)),
    "C": _shape(148, None, [(G2, 1.5, 60, None, 100), (LONE, 1.0, 40, None, 100)], (3, False, 2, True)),        # sweep 0 has fewer outputs: the one skipped
    "D": _shape(148, None, [(LONE, 0.05, 2, None, 100), (LONE, 4.0, 160, None, 100)], (3, True, 2, True)),      # xs_span 2307: a tenth band-pass tile; mmax from sweep 1
    "E": _shape(177, 4.425, [(G8, 1.0, 40, 2.825, 113), (G2, 1.5, 60, 0.5, 20)], (3, False, 2, False)),         # last 3-block band-pass, largest ml, G = 8
    "F": _shape(178, 4.45, [(LONE, 1.0, 40, None, 100)], (4, True, 1, False)),                                  # first 4-block band-pass
    "G": _shape(241, 6.025, [(LONE, 1.0, 40, None, 100), (G3, 1.5, 60, None, 100)], (4, True, 2, False)),       # last band-pass with a plan
    "H": Shape(8000, [LINES_300[0], LINES_300[3], LINES_300[1]], 187, [(2, 8, 67), (1, 8, 67)], (4, False, 2, True)),
    "I": Shape(8000, [LINES_300[0], LINES_300[1]], 187, [(1, 8, 67), (1, 8, 67)], (4, True, 2, True)),
    # the two limits from the other side: a band-pass without a plan, a low-pass the matrix-pipe tile is not written for
    "J242": _shape(242, 6.05, [(LONE, 1.0, 40, None, 100), (LONE, 1.5, 60, None, 100)], None),
    "J114": _shape(148, None, [(LONE, 1.0, 40, 2.85, 114), (LONE, 1.5, 60, 2.85, 114)], None),
}
FUSED = [k for k, s in SHAPES.items() if s.instance is not None]
EDGES = (1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097)


def least(shape):
    """Samples for one output of a sweep with the shape's longest correlator and longest low-pass."""
    return shape.mb + max(m for _, m, _ in shape.sweeps) + max(ml for _, _, ml in shape.sweeps) - 2


def edge_outputs(shape):
    """k of the recordings of least + k - 1 samples: EDGES and, for two sweeps whose output counts differ by d, the lengths that put
    the other sweep's last output on the same boundaries: d, d + 1, 2048 + d, 2048 + d + 1."""
    out = set(EDGES)
    if len(shape.sweeps) == 2:
        d = abs((shape.sweeps[0][1] + shape.sweeps[0][2]) - (shape.sweeps[1][1] + shape.sweeps[1][2]))
        out |= {d, d + 1, 2048 + d, 2048 + d + 1}
    return sorted(k for k in out if k >= 1)


def build(shape):
    from pymodem_amd import chain_builder as cb
    return [cb.build_chain(shape.rate, l) for l in shape.lines]


def plan(chains):
    """[(chain indices, their modems)] as NativePipeline partitions the chains (chain_execute._plan_sweeps on the groups it forms),
    without a device: _sweep_prepare, which uploads constants, is stood in for by the one answer _plan_sweeps asks it for."""
    from pymodem_amd import chain_execute as ce
    from pymodem_amd.modems import AFSKModem
    groups = {}
    for k, ch in enumerate(chains):
        groups.setdefault(ch[1].mark_key(), []).append(k)
    real = AFSKModem.__dict__["_sweep_prepare"]
    AFSKModem._sweep_prepare = staticmethod(lambda mods: {"tones": mods[0]._tones(*mods[0].unit_space_correlators())})
    try:
        return ce._plan_sweeps(chains, groups)
    finally:
        AFSKModem._sweep_prepare = real


def rails_signal(n, rate=48000.0, seed=32768):
    """Two tones keyed every 40 samples at 60000 peak plus noise of sigma 20000, clipped to int16: long stretches on both rails."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = 60000.0 * np.sin(2 * np.pi * np.where((t // 40) % 2 == 0, 1300.0, 2100.0).cumsum() / rate) + 20000.0 * rng.standard_normal(n)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def e_combine(lpf, bpf, gains, m):
    """The 1e-10 term of the sweep's E (pm_afsk_sweep.h, sweep_bound): every mode's E is at least this."""
    x_bound = float(np.abs(bpf).sum()) * 32768.0
    return 1e-10 * float(np.abs(lpf).sum()) * (1.0 + max(gains)) * float(m) * 1.4143 * x_bound, x_bound


def oracle_of(shape, audio):
    return [O.run_chain(O.build_chain(shape.rate, l), audio, canon=True) for l in shape.lines]


@functools.lru_cache(maxsize=None)
def ends_case(name):
    """rails_signal over two tiles and a bit with least + 64 samples of digital silence at each end, the oracle's chains on it, and per
    sweep the (sample, chain) pairs with |demod| <= 0.99 E_combine -> (audio, [oracle result per chain], [pairs per sweep])."""
    shape = SHAPES[name]
    chains = build(shape)
    lo = least(shape)
    audio = rails_signal(lo + 2 * 2048 + 200, float(shape.rate))
    audio[: lo + 64] = 0
    audio[-(lo + 64):] = 0
    audio.flags.writeable = False
    want = oracle_of(shape, audio)
    pairs = []
    for part, mods in plan(chains):
        lead = mods[0]
        E, _ = e_combine(np.asarray(lead.output_lpf, np.float64), np.asarray(lead.input_bpf, np.float64), [float(md.space_gain) for md in mods], len(lead.mark_correlator_i))
        pairs.append(sum(int(np.count_nonzero(np.abs(np.asarray(want[c]["demod"])) <= 0.99 * E)) for c in part))
    return audio, want, pairs


def assert_is_the_oracle_s(pipe, ticket, want, tag, lfsr=False):
    """Every chain of a finished recording against the oracle's results `want`: the sign bitmap bit for bit demod >= 0, nothing set
    past the last output up to the end of its word, the slicer's bytes and addresses (and the LFSR's bytes)."""
    for c, w in enumerate(want):
        sliced, plain = pipe.slices(ticket, c)
        bits = np.asarray(w["demod"]) >= 0
        got = pipe.bitmap(ticket, c, (len(bits) + 63) // 64 * 64)
        wrong = np.flatnonzero(got[: len(bits)] != bits)
        assert not len(wrong), (tag, c, len(wrong), wrong[:8].tolist(), len(bits))
        assert not got[len(bits):].any(), (tag, c)
        assert np.array_equal(sliced.data, w["slice_data"]) and np.array_equal(sliced.address, w["slice_addr"]), (tag, c)
        if lfsr:
            assert np.array_equal(plain, np.asarray(w["lfsr"], dtype=np.uint8)), (tag, c)
