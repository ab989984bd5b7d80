"""The walkers' event step (slice_walk_kernel<SlicerForm::Event, ...>, pymodem_amd/csrc/pm_slicer_event.h) against the step it
replaces (SlicerForm::Hand, step32a; switch slicer_no_event_step): every slicer byte, its stream address and the end state the slicer
object carries to its next call, bit for bit -- on the headline's recording through the pipeline bench.py times, on noise, on silence,
on band-limited streams, and with the wave-uniform fallback threshold (slicer_event_crossings) on both sides of the streams' crossing
counts."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, tuned

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import pymodem_amd
    if pymodem_amd.lib().pm_device_count() < 1:
        pytest.fail("no GPU visible: -m gpu tests need an MI355X")
    return pymodem_amd.Context.default()


def _stream(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.standard_normal(n)
    if kind == "silence":
        return np.zeros(n)
    if kind == "smooth":
        return np.convolve(rng.standard_normal(n + 63), np.hanning(64), "valid")
    if kind == "frames":          # NRZI-like symbols of 40 samples with jitter and a little noise: a demodulated AFSK 1200 stream
        lengths = np.maximum(1, np.round(40.0 + rng.normal(0.0, 0.7, n // 30 + 2)).astype(np.int64))
        levels = np.repeat(np.where(rng.random(lengths.size) < 0.5, 1.0, -1.0), lengths)[:n]
        return levels + 0.3 * rng.standard_normal(n)
    raise ValueError(kind)


def _slice(ctx, make, x, pieces, **switches):
    """Bytes, addresses and the carried state of one slicer object over `pieces` consecutive calls."""
    with tuned(ctx, **switches):
        s = make()
        out = []
        cuts = np.linspace(0, len(x), pieces + 1).astype(np.int64)
        for a, b in zip(cuts[:-1], cuts[1:]):
            got = s.slice(x[a:b])
            out.append((np.asarray(got.data).copy(), np.asarray(got.address).copy(), bytes(s._state)))
        return out


def _same(a, b, what):
    for k, ((da, aa, sa), (db, ab, sb)) in enumerate(zip(a, b)):
        assert np.array_equal(da, db) and np.array_equal(aa, ab), (what, k)
        assert sa == sb, (what, k, "end state")


BIN = [(48000, "1200", "0.77"), (8000, "1200", "0.75"), (44100, "1200", "0.75"), (11025, "300", "0.9"), (48000, "9600", "0.88")]


@pytest.mark.parametrize("kind", ["frames", "noise", "smooth", "silence"])
@pytest.mark.parametrize("rate,cfg,lock", BIN)
def test_binary_event_step_equals_step32a(ctx, rate, cfg, lock, kind):
    from pymodem_amd.slicer import BinarySlicer

    def make():
        s = BinarySlicer(sample_rate=rate, config=cfg)
        s.StringOptionsRetune({"lock_rate": lock})
        return s
    x = _stream(kind, 2_000_003 if kind != "silence" else 200_003, rate)
    old = _slice(ctx, make, x, 3, slicer_no_event_step=1)
    _same(_slice(ctx, make, x, 3), old, (rate, cfg, kind))


@pytest.mark.parametrize("cfg,lock", [("qpsk_2400", "0.98"), ("bpsk_300", "0.815")])
def test_quadrature_event_step_equals_step32a(ctx, cfg, lock):
    from pymodem_amd.data_classes import IQData
    from pymodem_amd.slicer import QuadratureSlicer
    n = 1_500_001
    iq = IQData()
    iq.i_data, iq.q_data = _stream("smooth", n, 1), _stream("smooth", n, 2)

    def run(**switches):
        with tuned(ctx, **switches):
            s = QuadratureSlicer(sample_rate=48000, config=cfg)
            s.StringOptionsRetune({"lock_rate": lock})
            got = s.slice(iq)
            return np.asarray(got.data).copy(), np.asarray(got.address).copy(), bytes(s._state)
    _same([run()], [run(slicer_no_event_step=1)], cfg)


@pytest.mark.parametrize("evt", [1, 4, 8, 16, 64])
def test_across_the_fallback_threshold(ctx, evt):
    """Waves whose words go to step32a (some lane has more than `evt` crossings) and waves that take events, side by side and word
    after word within one walker: streams of ~2 (frames) to ~20 (noise) crossings per word."""
    from pymodem_amd.slicer import BinarySlicer

    def make():
        s = BinarySlicer(sample_rate=48000, config="1200")
        s.StringOptionsRetune({"lock_rate": "0.77"})
        return s
    x = np.concatenate([_stream("frames", 600_000, 3), _stream("noise", 300_000, 4), _stream("frames", 600_000, 5)])
    old = _slice(ctx, make, x, 2, slicer_no_event_step=1)
    _same(_slice(ctx, make, x, 2, slicer_event_crossings=evt), old, evt)


_PIPE = r"""
import json, sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import pymodem_amd
from pymodem_amd import chain_builder as cb, chain_execute as ce, siggen
from conftest import GOLDEN
lines = [l for l in (json.loads(s) for s in open(GOLDEN + "/configs/afsk_1200_ax25_super_opt.json") if s.strip())
         if l.get("object_type") == "demod_chain"]
sig = siggen.recording("afsk1200_ax25", 48000, packets=6, seed=1234, noise_sigma=2000.0, payload_len=(20, 60))[0][:600000]
ctx = pymodem_amd.Context.default()
pipe = ce.NativePipeline([cb.build_chain(48000, l) for l in lines], len(sig), 48000 / 40, ctx=ctx, keep_slices=True)
dev = ctx.upload(sig)
ctx.sync()
out = {}
for r in range(2):
    t = pipe.submit(dev)
    for c in range(len(lines)):
        sl, _ = pipe.slices(t, c)
        out[f"d{r}_{c}"], out[f"a{r}_{c}"] = np.asarray(sl.data), np.asarray(sl.address)
    pipe.table(t)
pipe.close()
np.savez(sys.argv[2], **out)
"""


def test_headline_pipeline_slices_equal_step32a(tmp_path):
    """The pipeline bench.py times, on a packet-bearing AFSK 1200 recording of the headline's mode and noise level, all chains of the
    headline config: once with the event step and once with step32a (its slicer contexts read the switch from the environment, so
    each form runs in a process of its own)."""
    script = tmp_path / "pipe.py"
    script.write_text(_PIPE)
    res = {}
    for name, extra in (("event", {}), ("step32a", {"PM_SLICER_NO_EVENT_STEP": "1"})):
        env = {k: v for k, v in os.environ.items() if not k.startswith("PM_SLICER_")}
        env.update(extra, PM_SLICER_TRACE="1")
        out = tmp_path / f"{name}.npz"
        p = subprocess.run([sys.executable, str(script), ROOT, str(out)], env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        forms = {l.split()[1] for l in p.stderr.splitlines() if l.startswith("[slicer] ")}
        assert forms == {name}, forms                           # every batch of the run took the form asked for
        res[name] = np.load(out)
    a, b = res["event"], res["step32a"]
    assert sorted(a.files) == sorted(b.files) and len(a.files) >= 16
    for k in a.files:
        assert np.array_equal(a[k], b[k]), k
    assert sum(a[k].size for k in a.files if k.startswith("d0_")) > 1000
