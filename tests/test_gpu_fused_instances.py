"""The fused AFSK launch (afsk_fused8_kernel, dispatched by afsk_group_run_fused in pm_afsk.hip: band-pass, up to two certified sweeps
and the exact chain in one launch) in EVERY instance <KB, ONE0, NS, ONE1> it is compiled for.  The bundled configs reach five of the
twelve; tests/fused_shapes.py makes a chain group for each (its table, and which test reaches which instance):

  A <3,true,1>        B <3,false,1>        C <3,false,2,true>   D <3,true,2,true>    E <3,false,2,false>
  F <4,true,1>        G <4,true,2,false>   H <4,false,2,true>   I <4,true,2,true>
  <3,true,2,false>, <4,false,2,false>, <4,false,1>: the bundled configs (test_gpu_pipe_bitstream.py)

and with them what no bundled config has: a workgroup that skips sweep 0 and runs sweep 1 (C: sweep 0 has the longer correlator), a
tenth band-pass tile under a two-tap sliding sum (D), the band-pass lengths on both sides of the 3 / 4 block edge and the last with a
plan (E, F, G), the longest low-pass that fuses beside a short one and eight gains (E).  Every chain against the oracle (canonical FIR
order): sign bitmap bit for bit, nothing set past the last output, slicer bytes and addresses -- and the launches COUNTED, because a
shape that moved to the split path (band-pass + a launch per sweep) would still produce the oracle's bits."""
import numpy as np
import pytest

import fused_shapes as S
from conftest import tuned

GPU = pytest.mark.gpu
KTAILCAP, LIST = 48, 65536                                   # pm_afsk_sweep.h: kTailCap; pm_afsk.hip: kSweepCap


def test_the_table_is_what_it_claims():
    """Without a device: every shape's chains partition into the sweeps the table states, in its order; mb, m, ml are the table's;
    every lone chain's templates are tones (it is planned at all only then); the instance follows from that by afsk_group_run_fused's
    dispatch and pm_bpf8_plan_create's blocks (mb + 15 <= 192: 3, up to 241 taps: 4); and the nine fused shapes are nine instances."""
    for name, shape in S.SHAPES.items():
        chains = S.build(shape)
        planned = S.plan(chains)
        at = 0
        assert len(planned) == len(shape.sweeps), name
        for (part, mods), (count, m, ml) in zip(planned, shape.sweeps):
            assert part == list(range(at, at + count)), (name, part)
            at += count
            for md in mods:
                assert (len(md.input_bpf), len(md.mark_correlator_i), len(md.output_lpf)) == (shape.mb, m, ml), name
                assert md.front_end_key() == mods[0].front_end_key() == chains[0][1].front_end_key(), name
            assert mods[0]._tones(*mods[0].unit_space_correlators()) is not None, name      # (a lone chain is planned only then; the band-pass plan asks it of every sweep)
        assert at == len(chains), name
        ones = [count == 1 for count, _, _ in shape.sweeps]
        fits = all(ml + 15 <= 128 for _, _, ml in shape.sweeps) and shape.mb + 15 <= 256
        if shape.instance is None:
            assert not fits, name
        else:
            kb = 3 if shape.mb + 15 <= 192 else 4
            assert fits and shape.instance == (kb, ones[0], len(ones), len(ones) == 2 and ones[1]), name
    got = {S.SHAPES[k].instance for k in S.FUSED}
    assert len(got) == len(S.FUSED) == 9
    bundled = {(3, True, 2, False), (4, False, 2, False), (4, False, 1, False)}
    assert got | bundled == {(kb, o0, ns, o1) for kb in (3, 4) for o0 in (False, True) for ns, o1 in ((1, False), (2, False), (2, True))}
    # the edges the shapes are there for
    assert S.SHAPES["C"].sweeps[0][1] > S.SHAPES["C"].sweeps[1][1]                        # sweep 0 is the one with fewer outputs
    runs = lambda ml: -(-(2048 + ml - 1) // 12)
    assert max(runs(ml) * 12 + m - 1 for _, m, ml in S.SHAPES["D"].sweeps) == 2307         # lpf8_layout's xs_span: ten tiles of 256
    assert [S.SHAPES[k].mb for k in "EFG"] == [177, 178, 241] and S.SHAPES["J242"].mb == 242
    assert S.SHAPES["E"].sweeps[0][0] == 8 and {ml for _, _, ml in S.SHAPES["E"].sweeps} == {113, 20}
    assert {ml for _, _, ml in S.SHAPES["J114"].sweeps} == {114}


@pytest.mark.parametrize("name", S.FUSED)
def test_the_silent_ends_hold_uncertain_samples_for_both_paths(name):
    """(On the oracle alone) the recording of test_uncertain_samples_in_every_shape is worth running: every chain's first and last
    outputs are exact zeros, and each sweep has more (sample, chain) pairs inside 0.99 E_combine than a workgroup decides itself
    (kTailCap: the recording's list is used too) and at most a sixteenth of that list (the list path cannot become the overflow path)."""
    audio, want, pairs = S.ends_case(name)
    shape = S.SHAPES[name]
    assert len(audio) == S.least(shape) + 2 * 2048 + 200 and len(pairs) == len(shape.sweeps)
    for w in want:
        y = np.asarray(w["demod"])
        assert y[0] == 0.0 and y[-1] == 0.0
    print(name, "pairs per sweep", pairs)
    for p in pairs:
        assert KTAILCAP + 1 <= p <= LIST // 16, (name, pairs)


@pytest.fixture(scope="module")
def ctx():
    import pymodem_amd
    return pymodem_amd.Context.default()


class Watch:
    """Launch counts by kernel class over the caller's context and the contexts the pipeline owns, from here to read()."""
    def __init__(self, ctx, pipe):
        self.watched = [ctx] + pipe.side_contexts()
        for c in self.watched:
            c.profile(True)

    def read(self):
        out = {}
        for c in self.watched:
            for k, (_, n) in c.profile_read().items():
                out[k] = out.get(k, 0) + n
            c.profile(False)
        return out


def _pipe(ctx, shape, max_samples):
    from pymodem_amd import chain_execute as ce
    return ce.NativePipeline(S.build(shape), max_samples, shape.rate / 40, ctx=ctx, keep_slices=True)


def _run_lengths(ctx, shape, outs, tag):
    """Recordings of least + k - 1 samples of seeded Gaussian audio (sigma 6000), k in outs, eight in flight, each against the oracle
    -> (recordings submitted, launches by class)."""
    lo = S.least(shape)
    rng = np.random.default_rng(2048)
    base = np.clip(np.rint(rng.standard_normal(lo + max(outs) - 1) * 6000), -32768, 32767).astype(np.int16)
    pipe = _pipe(ctx, shape, len(base))
    dev = {k: ctx.upload(base[: lo + k - 1].copy()) for k in outs}
    ctx.sync()
    watch = Watch(ctx, pipe)
    try:
        for g0 in range(0, len(outs), 8):                     # (eight in flight: a bitmap slot is reused sixteen submissions later)
            for k, t in [(k, pipe.submit(dev[k])) for k in outs[g0:g0 + 8]]:
                S.assert_is_the_oracle_s(pipe, t, S.oracle_of(shape, base[: lo + k - 1]), (tag, k))
                pipe.release(t)
    finally:
        launches = watch.read()
        pipe.close()
    return len(outs), launches


@GPU
@pytest.mark.parametrize("name", S.FUSED)
def test_each_shape_at_the_edges_of_its_tiles_in_one_launch(ctx, name):
    """Lengths that put the last output of either sweep on, just before and just after a bitmap word (64), a matrix tile (256) and a
    workgroup (2048), down to a single output.  In C, k = 2047 and 2048 leave a second workgroup to sweep 1 alone.  One fused launch
    per recording (fir_f64) and no band-pass launch of its own (fir_i16: pm_bpf8_run and pm_fir_valid_i16 book it)."""
    shape = S.SHAPES[name]
    outs = S.edge_outputs(shape)
    if name == "C":                                           # sweep 0 has k outputs, sweep 1 twenty more: past k = 2048 - 20 the second workgroup is sweep 1's alone
        assert {2047, 2048} <= set(outs) and shape.sweeps[0][1] - shape.sweeps[1][1] == 20 and shape.sweeps[0][2] == shape.sweeps[1][2]
    recordings, launches = _run_lengths(ctx, shape, outs, name)
    print(name, shape.instance, recordings, launches)
    assert launches["fir_f64"] == recordings, (name, launches)
    assert launches["fir_i16"] == 0, (name, launches)


@GPU
@pytest.mark.parametrize("name", ["J242", "J114", "C-split"])
def test_past_the_limits_the_launches_are_made_apart(ctx, name):
    """A band-pass of 242 taps has no plan, a low-pass of 114 no matrix-pipe tile, and afsk_split asks for it: the band-pass launch of
    its own per recording, one launch per sweep behind it, and the oracle's bits all the same."""
    shape = S.SHAPES[name[0] if name == "C-split" else name]
    with tuned(ctx, afsk_split=int(name == "C-split")):        # (the pipeline's demod contexts copy the switches when it is made)
        recordings, launches = _run_lengths(ctx, shape, [64, 2048, 4097], name)
    print(name, recordings, launches)
    assert launches["fir_i16"] == recordings, (name, launches)
    assert launches["fir_f64"] == recordings * len(shape.sweeps), (name, launches)


@GPU
@pytest.mark.parametrize("name", S.FUSED)
def test_uncertain_samples_in_every_shape(ctx, name):
    """Exact zeros at the first and last outputs of every chain (test_the_silent_ends_hold_uncertain_samples_for_both_paths counts
    them): decided by the exact chain in the workgroup that found them, the rest from the recording's list; with sweep_no_tail all from
    the list."""
    audio, want, pairs = S.ends_case(name)
    shape = S.SHAPES[name]
    d = ctx.upload(np.array(audio))
    ctx.sync()
    for switches in ({}, {"sweep_no_tail": 1}):
        with tuned(ctx, **switches):
            pipe = _pipe(ctx, shape, len(audio))               # its demod contexts copy the switches
            watch = Watch(ctx, pipe)
            try:
                t = pipe.submit(d)
                S.assert_is_the_oracle_s(pipe, t, want, (name, switches))
                pipe.release(t)
            finally:
                launches = watch.read()
                pipe.close()
        assert (launches["fir_f64"], launches["fir_i16"]) == (1, 0), (name, switches, launches)


@GPU
def test_an_overflowed_list_behind_a_four_block_band_pass(ctx):
    """Shape G (241 band-pass taps) with 70 000 samples of digital silence inside a signal: more uncertain samples than the
    65 536-entry list holds, even for the lone chain's sweep, so the exact kernels decide the recording -- between two ordinary
    recordings in flight.  All three are the oracle's: bitmaps, slicer bytes and addresses, LFSR bytes."""
    shape = S.SHAPES["G"]
    n = 80000
    sig = S.rails_signal(n, seed=241)
    hush = sig.copy()
    hush[5000:75000] = 0
    other = np.negative(np.maximum(sig, -32767))
    recs = [sig, hush, other]
    want = [S.oracle_of(shape, a) for a in recs]
    for w in want[1]:
        assert int(np.count_nonzero(np.asarray(w["demod"]) == 0.0)) > LIST
    dev = [ctx.upload(a) for a in recs]
    ctx.sync()
    pipe = _pipe(ctx, shape, n)
    try:
        for k, t in enumerate([pipe.submit(b) for b in dev]):
            S.assert_is_the_oracle_s(pipe, t, want[k], ("G", k), lfsr=True)
            pipe.release(t)
    finally:
        pipe.close()
