"""The batch engine's row slicers (rowslice_kernel, pymodem_amd/csrc/pm_slicer.hip; driven through LoopBatch.run_sliced, they have no entry
point of their own) where the clock lands on the threshold: samples per symbol of exactly 25 (symbol rate 1920 at 48 kHz: an integer
threshold, digital silence ties at every symbol) and 48000/1800, lock rates 0.75, 0.77 and 0.45 -- the five row kernels
(tests/test_slicer_event_model.py holds that choice against the launcher's own) -- with the last engine chunk ending in a partial word, where
the scalar loop compares with thr and the full words with tp.  The reference is the oracle's C port of the reference slicers on the sign
streams the same engine returns from run(): bytes, addresses and every field of the rows' records, bit for bit."""
import numpy as np
import pytest

import slicer_ties as T
from conftest import noise_i16
from oracle import oracle as O
from test_gpu_loopbatch import bits_of, group_modems

pytestmark = pytest.mark.gpu

RATE = 48000
NOUT = 3 * 2048 + 5 * 64 + 50           # demodulated samples per stream: several chunks of 2048, and 50 samples in the last word


def recordings(n):
    t = np.arange(n)
    keyed = (6000 * np.sin(2 * np.pi * 1500.0 * t / RATE) * np.sign(np.sin(2 * np.pi * 37.0 * t / RATE))).astype(np.int16)
    return [np.zeros(n, np.int16), keyed, noise_i16(n, seed=77, sigma=4000.0)]      # digital silence, a keyed carrier, noise


@pytest.fixture(scope="module", params=["bpsk_300.json", "qpsk_2400.json"])
def engine(request):
    """One engine per config for all the slicer settings, and the sign streams of its run() -- the reference's input -- made once."""
    import pymodem_amd
    from pymodem_amd.loop_batch import LoopBatch
    ctx = pymodem_amd.Context.default()
    group = group_modems(request.param, RATE, [1500.0, 1510.0])
    eng = LoopBatch([m for _, m in group], recordings=3, ctx=ctx, chunk=2048)
    try:
        n = NOUT - eng.geometry(0)[0]
        dev = [ctx.upload(r) for r in recordings(n)]
        bitmaps = eng.run(dev)
        ctx.sync()
        assert bitmaps[0][0].n == NOUT and eng.geometry(n)[2] >= 3
        signs = [[(np.where(bits_of(b.bits_i, NOUT), 1.0, -1.0), np.where(bits_of(b.bits_q, NOUT), 1.0, -1.0) if b.bits_q is not None else None)
                  for b in row] for row in bitmaps]
        yield ctx, eng, group, dev, signs
    finally:
        eng.close()


def oracle_row(sl, xi, xq):
    if xq is None:
        o = O.BinarySlicer(RATE, "1200")
    else:
        o = O.QuadratureSlicer(RATE, "qpsk_2400" if sl.bits_per_symbol == 2 else "bpsk_300")
        assert list(o.demap[:len(sl.demap)]) == list(sl.demap) and o.mask == sl.state_mask and o.bps == sl.bits_per_symbol
    o.sps, o.lock_rate = sl.samples_per_symbol, sl.lock_rate
    d, a = o.slice(xi) if xq is None else o.slice((xi, xq))
    return d, a, o.state


def check_record(rec, d, a, s, quad, what):
    bits = int(s[4])
    want = {"count": len(d), "first_addr": int(a[0]) if len(a) else 0, "last_addr": int(a[-1]) if len(a) else 0, "seen": int(s[5]),
            "clk": T.bits_of(s[0]), "li_neg": int(s[1] < 0), "lq_neg": int(s[2] < 0) if quad else 0,
            "wbyte": int(s[3]) & ((1 << bits) - 1), "wbits": bits, "sreg": int(s[6]) & 3 if quad else 0}
    got = {k: (T.bits_of(rec[k]) if k == "clk" else int(rec[k])) for k in want}
    assert got == want, what


@pytest.mark.parametrize("symbol_rate,lock", T.ROW_CASES)
def test_row_slicers_at_ties(engine, symbol_rate, lock):
    from pymodem_amd import chain_builder as cb
    ctx, eng, group, dev, signs = engine
    slicers = [cb.build_chain(RATE, line)[2] for line, _ in group]
    for sl in slicers:
        sl.retune(symbol_rate=symbol_rate, lock_rate=lock)
    sps = slicers[0].samples_per_symbol
    assert sps == RATE / symbol_rate and T.choose([(sps, lock, 0.0)] * len(slicers), event=False) == T.ROW_FORMS[T.ROW_CASES.index((symbol_rate, lock))]
    if sps == 25.0:
        # precondition on the INPUT: the silence rows tie at every symbol, and at one in the partial last word of the last chunk
        for xi, xq in signs[0]:
            ties, syms, _ = T.reference(xi < 0, sps, lock, neg_q=None if xq is None else xq < 0)
            assert ties == syms and len(ties) >= NOUT / sps - 1 and ties[-1] >= NOUT // 64 * 64
    run = eng.run_sliced(dev, slicers)
    ctx.sync()
    assert run.ok() and run.nout == NOUT
    got, recs = run.fetch(0, run.rows), run.records()
    C, produced = len(group), 0
    for k in range(3):
        for c in range(C):
            xi, xq = signs[k][c]
            d, a, s = oracle_row(slicers[c], xi, xq)
            g = got[k * C + c]
            assert np.array_equal(g.data, d), (k, c, "data", len(g.data), len(d))
            assert np.array_equal(g.address, a), (k, c, "addresses")
            check_record(recs[k * C + c], d, a, s, xq is not None, (k, c))
            produced += len(d)
    assert produced > 3 * C * 10


def test_wide_address_steps_raise_the_rows_flag():
    """5 symbols per second: 9600 samples per symbol, a byte every 76 800 samples -- more than an address step of 16 bits holds.  Every row
    whose reference addresses step by more than 65 535 has bit 0 of pm_rowslice_rec.flags, no other row has it, and the run is not ok()."""
    import pymodem_amd
    from pymodem_amd import chain_builder as cb
    from pymodem_amd.loop_batch import LoopBatch
    ctx = pymodem_amd.Context.default()
    group = group_modems("bpsk_300.json", RATE, [1500.0, 1510.0])
    slicers = [cb.build_chain(RATE, line)[2] for line, _ in group]
    for sl in slicers:
        sl.retune(symbol_rate=5.0)
    assert slicers[0].samples_per_symbol == 9600.0
    n = 250000
    recs_in = [np.zeros(n, np.int16), noise_i16(n, seed=78, sigma=4000.0)]
    eng = LoopBatch([m for _, m in group], recordings=2, ctx=ctx, chunk=8192)
    try:
        dev = [ctx.upload(r) for r in recs_in]
        bitmaps = eng.run(dev)
        ctx.sync()
        nout = bitmaps[0][0].n
        signs = [[np.where(bits_of(b.bits_i, nout), 1.0, -1.0) for b in row] for row in bitmaps]
        run = eng.run_sliced(dev, slicers)
        ctx.sync()
        recs = run.records()
        wide = []
        for k in range(2):
            for c in range(len(group)):
                d, a, s = oracle_row(slicers[c], signs[k][c], None)
                rec = recs[k * len(group) + c]
                wide.append(bool((np.diff(a) > 65535).any()))
                assert bool(int(rec["flags"]) & 1) == wide[-1], (k, c, a, int(rec["flags"]))
                assert int(rec["flags"]) & ~1 == 0 and int(rec["count"]) == len(d) and T.bits_of(rec["clk"]) == T.bits_of(s[0]), (k, c)
                assert np.array_equal(run.data.download()[(k * len(group) + c) * run.cap:][:len(d)], d), (k, c)
                if len(a):
                    assert (int(rec["first_addr"]), int(rec["last_addr"])) == (int(a[0]), int(a[-1])), (k, c)
        assert wide[0] and wide[1] and len(oracle_row(slicers[0], signs[0][0], None)[0]) >= 3      # the silence rows: three bytes, wide steps
        assert not all(wide)                                                                        # ... and rows that stay narrow
        assert not run.ok()
    finally:
        eng.close()
