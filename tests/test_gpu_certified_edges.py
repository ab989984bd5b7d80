"""The certified-sign kernels where their bounds decide (a sign only a slicer reads may come from cheaper arithmetic under
a proven bound E, every output with |value| <= E recomputed in the canonical order):

  * fir8_kernel + fir8_exact_kernel on rows whose error terms are all at their worst (tests/fir8_model.py builds them and predicts,
    bit for bit, which outputs the kernel must flag): the bits are the canonical sum's and `h_recomputed` is the model's count exactly;
  * the AFSK gain sweeps of the headline config on audio that dwells at each chain's tie LPF(M) = g LPF(S): the oracle's own stream has
    samples inside the combine bound, every mode's bits are the oracle's and its counter sees at least those samples;
  * int16 -32768 (and 32767) through the native executor at the fused launch's tile edges;
  * exact zeros at the first and last outputs of a stream through the executor: the exact chain from the audio, in the workgroup and
    from the recording's list."""
import ctypes
import json
import os

import numpy as np
import pytest

import fir8_model as F
from conftest import GOLDEN, tuned
from fused_shapes import e_combine as _e_combine, rails_signal
from oracle import oracle as O
from test_gpu_fir8 import _both

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import pymodem_amd
    return pymodem_amd.Context.default()


def test_fir8_on_the_adversary_flags_exactly_what_the_model_flags(ctx):
    """One output per row, its error lined up to ~0.97 E, the canonical sum swept over [-2E, 2E]: a bound halved, a term left out or
    `>` for `>=` changes either a bit or the number of outputs recomputed."""
    for name, plan, rows, dirs in F.adversarial_cases(O.fir_canon):
        got, want, redo = _both(ctx, rows, plan.h)
        y = np.array([O.fir_canon(r, plan.h)[0] for r in rows])
        assert np.array_equal(got[:, 0], y >= 0), (name, int(np.count_nonzero(got[:, 0] != (y >= 0))))
        assert np.array_equal(got, want), name
        flagged = int(sum(plan.run(r)["flagged"].sum() for r in rows))
        assert 50 <= flagged < len(rows), (name, flagged)
        assert redo == flagged, (name, redo, flagged)


@pytest.mark.parametrize("m", [241, 961])
def test_fir8_flags_exactly_what_the_model_flags_on_plain_rows(ctx, m):
    """Noise at several levels, a workgroup of zeros, a NaN: the count of outputs sent to the exact kernel is the model's."""
    rng = np.random.default_rng(m + 1)
    h = F.window_taps(m, rng)
    plan = F.Plan(h)
    n = 3 * F.KWG_OUT + 777 + m
    rows = rng.standard_normal((4, n)) * np.array([[1.0], [3e4], [1e-6], [1.0]])
    rows[3, F.KWG_OUT:2 * F.KWG_OUT + plan.window] = 0.0
    rows[3, -300] = np.nan
    got, want, redo = _both(ctx, rows, h)
    assert np.array_equal(got, want)
    assert redo == int(sum(plan.run(r)["flagged"].sum() for r in rows))


# ---- AFSK gain sweeps at their ties ---------------------------------------------------------------------------------------------

def _lines():
    with open(os.path.join(GOLDEN, "configs", "afsk_1200_ax25_super_opt.json")) as f:
        return [l for l in (json.loads(s) for s in f if s.strip()) if l.get("object_type") == "demod_chain"]


SEG = 40000


def _tie_recording():
    """Eight stretches of SEG samples, one per chain of the headline config: a tone held at the frequency where that chain's
    LPF(M) - g LPF(S) crosses zero (found on the oracle by bisection), at an amplitude where the sum wanders around zero by less than
    its ripple at full scale would, each stretch opened by a burst clipped on both rails (32767 and -32768)."""
    out = []
    t = np.arange(SEG)
    for line in _lines():
        md = O.build_chain(48000, line)[0]
        lo, hi = md.p["mark_freq"], md.p["space_freq"]
        probe = lambda f: md.demod(np.rint(2000.0 * np.sin(2 * np.pi * f * np.arange(6000) / 48000.0)).astype(np.int16), canon=True)[500:].mean()
        up = probe(lo) > 0
        for _ in range(40):
            mid = 0.5 * (lo + hi)
            if (probe(mid) > 0) == up:
                lo = mid
            else:
                hi = mid
        seg = 300.0 * np.sin(2 * np.pi * mid * t / 48000.0)
        seg[:1500] = 40000.0 * np.sin(2 * np.pi * mid * t[:1500] / 48000.0)
        out.append(np.clip(np.rint(seg), -32768, 32767))
    a = np.concatenate(out).astype(np.int16)
    assert (a == 32767).any() and (a == -32768).any()
    return a


def _sweeps(lines):
    """[(chain indices, gains, mark pair, unit pair, low-pass, band-pass, correlator length)] as the executor groups them."""
    from pymodem_amd import chain_builder as cb
    groups = {}
    for c, line in enumerate(lines):
        md = cb.build_chain(48000, line)[1]
        key = (md.mark_freq, md.space_freq, len(md.mark_correlator_i))
        groups.setdefault(key, []).append((c, md))
    out = []
    for mods in groups.values():
        lead = mods[0][1]
        ui, uq = lead.unit_space_correlators()
        out.append(([c for c, _ in mods], [float(md.space_gain) for _, md in mods], (lead.mark_correlator_i, lead.mark_correlator_q), (ui, uq),
                    np.asarray(lead.output_lpf, np.float64), np.asarray(lead.input_bpf, np.float64), len(lead.mark_correlator_i)))
    return out


@pytest.fixture(scope="module")
def tie():
    audio = _tie_recording()
    lines = _lines()
    want = [O.run_chain(O.build_chain(48000, l), audio, canon=True) for l in lines]
    near = {}
    for chains, gains, mark, unit, lpf, bpf, m in _sweeps(lines):
        E, _ = _e_combine(lpf, bpf, gains, m)
        for c in chains:
            near[c] = int(np.count_nonzero(np.abs(np.asarray(want[c]["demod"])) <= 0.99 * E))
    return audio, lines, want, near


def test_the_tie_recording_reaches_the_combine_bound(tie):
    """(On the oracle alone) the recording is worth running: every chain's exact stream has samples inside 0.99 E_combine."""
    audio, lines, want, near = tie
    assert len(audio) <= 330000
    assert min(near.values()) >= 5 and sum(near.values()) >= 100, near


@pytest.mark.parametrize("mode", [False, True, "unfused", "lpf8", "lpf8-list"])
def test_gain_sweeps_at_their_ties_are_the_oracle_s(ctx, tie, mode):
    """Each sweep of the headline config through pm_afsk_sweep_signs(_tones) in the five modes of
    test_afsk_gain_sweep_signs_are_the_exact_chain_s, on the band-passed tie recording: every bitmap is the oracle's, and the sweep's
    uncertain count is at least the oracle's samples inside E_combine (|y~ - y| is far inside E, so each of them is flagged).  In "lpf8"
    the workgroups decide theirs without the counter: bits only there ("lpf8-list" counts the same kernel's)."""
    from test_gpu_kernels import _sweep
    audio, lines, want, near = tie
    with tuned(ctx, afsk_unfused=int(mode == "unfused"), afsk_lpf8=int(mode in ("lpf8", "lpf8-list")), sweep_no_tail=int(mode == "lpf8-list")):
        for chains, gains, mark, unit, lpf, bpf, m in _sweeps(lines):
            x = O.fir_canon(audio, bpf)
            _, x_bound = _e_combine(lpf, bpf, gains, m)
            got, redo, _ = _sweep(ctx, x, x_bound, mark, unit, gains, lpf, mode)
            for g, c in enumerate(chains):
                w = np.asarray(want[c]["demod"]) >= 0
                assert np.array_equal(got[g], w), (mode, c, int(np.count_nonzero(got[g] != w)))
            if mode != "lpf8":
                assert redo >= sum(near[c] for c in chains), (mode, chains, redo, [near[c] for c in chains])


def test_native_pipeline_at_the_ties_is_the_oracle_s(tie):
    """The executor (fused band-pass + sweeps on the matrix pipe, lockstep slicers, LFSRs) on the tie recording: every chain's bitmap,
    slicer bytes and addresses, and LFSR bytes are the oracle's."""
    import pymodem_amd
    from pymodem_amd import chain_builder as cb, chain_execute as ce
    audio, lines, want, near = tie
    ctx = pymodem_amd.Context.default()
    d = ctx.upload(audio)
    ctx.sync()
    pipe = ce.NativePipeline([cb.build_chain(48000, l) for l in lines], len(audio), 48000 / 40, ctx=ctx, keep_slices=True)
    for t in [pipe.submit(d) for _ in range(2)]:
        for c, w in enumerate(want):
            sliced, plain = pipe.slices(t, c)
            wb = np.asarray(w["demod"]) >= 0
            got = pipe.bitmap(t, c, len(wb))
            assert np.array_equal(got, wb), (c, int(np.count_nonzero(got != wb)))
            assert np.array_equal(sliced.data, w["slice_data"]) and np.array_equal(sliced.address, w["slice_addr"]), c
            assert np.array_equal(plain, np.asarray(w["lfsr"], dtype=np.uint8)), c
        pipe.release(t)
    pipe.close()


def test_both_rails_through_the_executor_at_the_tile_edges():
    """Audio clipped on both rails -- -32768 included, which no other recording brings to the executor -- at the lengths of
    test_fused_launch_at_the_edges_of_its_tiles: every chain's bitmap (nothing set past its last bit) and slicer bytes are the oracle's."""
    import pymodem_amd
    from pymodem_amd import chain_builder as cb, chain_execute as ce
    lines = _lines()
    chains = [cb.build_chain(48000, l) for l in lines]
    mb, ml = len(chains[0][1].input_bpf), len(chains[0][1].output_lpf)
    m0 = max(len(ch[1].mark_correlator_i) for ch in chains)
    least = mb + m0 + ml - 2
    base = rails_signal(least + 3 * 2048 + 200)
    assert np.count_nonzero(base == -32768) > 1000 and np.count_nonzero(base == 32767) > 1000
    outs = [1, 2, 20, 21, 63, 64, 65, 84, 85, 255, 256, 257, 276, 2047, 2048, 2049, 2068, 2069, 4096, 4097, 6143, 6144, 6165]
    ctx = pymodem_amd.Context.default()
    pipe = ce.NativePipeline(chains, len(base), 48000 / 40, ctx=ctx, keep_slices=True)
    dev = {k: ctx.upload(base[: least + k - 1].copy()) for k in outs}
    ctx.sync()
    for g0 in range(0, len(outs), 8):
        for k, tk in [(k, pipe.submit(dev[k])) for k in outs[g0:g0 + 8]]:
            audio = base[: least + k - 1]
            for c, line in enumerate(lines):
                w = O.run_chain(O.build_chain(48000, line), audio, canon=True)
                sliced, _ = pipe.slices(tk, c)
                assert np.array_equal(sliced.data, w["slice_data"]) and np.array_equal(sliced.address, w["slice_addr"]), (k, c)
                want = np.asarray(w["demod"]) >= 0
                words = (len(want) + 63) // 64 * 64
                got = pipe.bitmap(tk, c, words)
                assert np.array_equal(got[: len(want)], want), (k, c, int(np.count_nonzero(got[: len(want)] != want)))
                assert not got[len(want):].any(), (k, c)
            pipe.release(tk)
    pipe.close()


def test_uncertain_samples_at_the_ends_of_a_stream_through_the_executor():
    """The exact chain from the audio at a stream's first and last outputs.  The signal of
    test_both_rails_through_the_executor_at_the_tile_edges over two tiles and a bit, digital silence at both ends: the first and the
    last outputs of every chain are exact zeros, which no bound certifies, and each sweep has (sample, chain) pairs inside 0.99
    E_combine -- at most a sixteenth of the 65536-entry list, so the list path cannot turn into the overflow path (on the oracle: 180
    pairs for the lone chain, 130 to 132 for each of the other seven).  They are decided in the workgroup that found them, and -- with
    sweep_no_tail -- from the recording's list (pm_afsk_sweep_exact_list), behind the single fused launch and behind one launch per
    sweep: every chain's bitmap (nothing set past its last bit), slicer bytes and addresses are the oracle's."""
    import pymodem_amd
    from pymodem_amd import chain_builder as cb, chain_execute as ce
    lines = _lines()
    sweeps = _sweeps(lines)
    bpf, lpf = sweeps[0][5], sweeps[0][4]
    least = len(bpf) + max(m for *_, m in sweeps) + len(lpf) - 2
    n = least + 2 * 2048 + 200
    assert (least, n) == (306, 4602)
    audio = rails_signal(n)
    audio[: least + 64] = 0
    audio[-(least + 64):] = 0
    want = [O.run_chain(O.build_chain(48000, l), audio, canon=True) for l in lines]
    for chains, gains, mark, unit, lpf, bpf, m in sweeps:
        E, _ = _e_combine(lpf, bpf, gains, m)
        pairs = 0
        for c in chains:
            y = np.asarray(want[c]["demod"])
            assert y[0] == 0.0 and y[-1] == 0.0, c
            pairs += int(np.count_nonzero(np.abs(y) <= 0.99 * E))
        assert 1 <= pairs <= 4096, (chains, pairs)
    ctx = pymodem_amd.Context.default()
    d = ctx.upload(audio)
    ctx.sync()
    for switches in ({}, {"sweep_no_tail": 1}, {"afsk_split": 1, "sweep_no_tail": 1}):
        with tuned(ctx, **switches):
            pipe = ce.NativePipeline([cb.build_chain(48000, l) for l in lines], n, 48000 / 40, ctx=ctx, keep_slices=True)   # its demod contexts copy the switches
            tk = pipe.submit(d)
            for c, w in enumerate(want):
                sliced, _ = pipe.slices(tk, c)
                wb = np.asarray(w["demod"]) >= 0
                got = pipe.bitmap(tk, c, (len(wb) + 63) // 64 * 64)
                assert np.array_equal(got[: len(wb)], wb), (switches, c, int(np.count_nonzero(got[: len(wb)] != wb)))
                assert not got[len(wb):].any(), (switches, c)
                assert np.array_equal(sliced.data, w["slice_data"]) and np.array_equal(sliced.address, w["slice_addr"]), (switches, c)
            pipe.release(tk)
            pipe.close()
