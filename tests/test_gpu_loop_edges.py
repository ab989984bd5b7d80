"""The carrier-loop kernels (pm_costas_bpsk, pm_pll_afsk, pm_costas_qpsk, pm_mpsk_loop) in every launch shape against the oracle on
the cases of tests/golden/loop_edges.npz -- table index 256, negative phases and several turns per sample, round()'s ties, the integral
on and next to its rails, the detector's clip and quadrant fold (every pair of its grid a lane of its own) -- which tests/test_oracle_loop_edges.py pins to the reference; the rows
AGC on its edge inputs; and the batch engine on degenerate recordings.

The bar is bytes: the oracle's loops are the reference's statements in binary64, so every output sample and every field of the pm_loop
struct is compared as a 64-bit pattern (a -0.0 where the oracle has +0.0 would fail).  One place is known where oracle and reference
differ in the sign of a zero and it is harmless: the MPSK control round(-0.0) is the integer 0 in Python and -0.0 from nearbyint();
the control is only ever added to the carrier frequency, and x + -0.0 == x + 0.0 for every x but -0.0, which no carrier is."""
import ctypes
import math

import numpy as np
import pytest

import loop_edges as E
from conftest import noise_i16, tuned
from oracle import oracle as O

pytestmark = pytest.mark.gpu

LENGTHS = [1, 7, 8, 9, 31, 32, 33, 255, 256, 257]
COUNTS = [1, 9, 64, 65, 150]
SENTINEL = -7.25e77                      # what the output buffers hold before a launch: nothing may be written past a row's n samples
MAX_TRIPS = 1024                         # pairs of (parameters, input) made here stay far below the kernels' 4096-trip guard


@pytest.fixture(scope="module")
def ctx():
    import pymodem_amd
    if pymodem_amd.lib().pm_device_count() < 1:
        pytest.fail("no GPU visible: -m gpu tests need an MI355X")
    return pymodem_amd.Context.default()


@pytest.fixture(scope="module")
def tables(ctx):
    return ctx.upload(O.nco_table()), ctx.upload(np.ascontiguousarray(O.pd_table().reshape(-1), dtype=np.int32))


def cases_of(kind, n):
    return [c for c in sorted(E.CASES) if E.CASES[c]["loop"] == kind and E.CASES[c]["n"] >= n]


def full_lengths(kind):
    return sorted({s["n"] for s in E.CASES.values() if s["loop"] == kind})


def trip_bound(kind, params, x0, x1):
    """An upper bound of the trips either loop of nco.py:36-39 can take in one sample: |control| <= |gain * p| * max|error| + limit,
    the error bounded through the loop filter's gain (b0 + b1) / (1 - a1)."""
    ps, _, freq, b0, b1, a1, p, _, limit, gain = [float(v) for v in params]
    top = max(float(np.abs(x0).max()), float(np.abs(x1).max()) if x1 is not None else 0.0)
    err = {"bpsk": top * top, "pll": top, "qpsk": 2 * top, "mpsk": 32 * 180.0}[kind]                 # (the table holds 32 x degrees)
    dc = (abs(b0) + abs(b1)) / (1 - abs(a1))
    return ps * (abs(freq) + abs(gain * p) * err * dc + limit + 1) / (2 * math.pi) + 2


_EXPECT = {}


def expect(pname, xname, n):
    """The oracle's loop with the parameters and initial state of case `pname` over the first n samples of case `xname`'s input rows:
    (out0, out1 or None, the 28 doubles of the pm_loop before, after)."""
    key = (pname, xname, n)
    if key not in _EXPECT:
        c, x = E.case(pname), E.case(xname)
        kind = E.CASES[pname]["loop"]
        x0, x1 = x["x0"][:n], (x["x1"][:n] if kind == "mpsk" else None)
        if pname != xname:
            assert trip_bound(kind, c["params"], x0, x1) <= MAX_TRIPS, key
        L, br = E.oracle_loop(c)
        before = np.concatenate([c["params"], c["state0"], br if br is not None else np.zeros(9)])
        o0, o1 = E.oracle_run(kind, L, br, x0, x1)
        after = np.concatenate([c["params"], [getattr(L, f) for f in E.STATE], br if br is not None else np.zeros(9)])
        _EXPECT[key] = (o0, o1, before, after)
    return _EXPECT[key]


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def first_difference(a, b):
    d = np.flatnonzero(np.ascontiguousarray(a).view(np.uint64).reshape(-1) != np.ascontiguousarray(b).view(np.uint64).reshape(-1))
    k = int(d[0])
    return f"{len(d)} differ, first at {k}: got {np.reshape(a, -1)[k]!r} want {np.reshape(b, -1)[k]!r}"


def call(ctx, tables, kind, loops, nl, x0, x1, x_stride, n, o0, o1, out_stride):
    import pymodem_amd
    from pymodem_amd._native import check
    L = pymodem_amd.lib()
    tab, pd = tables
    if kind == "bpsk":
        check(L.pm_costas_bpsk(ctx.handle, loops, nl, tab.ptr, x0.ptr, x_stride, n, o0.ptr, out_stride))
    elif kind == "pll":
        check(L.pm_pll_afsk(ctx.handle, loops, nl, tab.ptr, x0.ptr, x_stride, n, o0.ptr, out_stride))
    elif kind == "qpsk":
        check(L.pm_costas_qpsk(ctx.handle, loops, nl, tab.ptr, x0.ptr, x_stride, n, o0.ptr, o1.ptr, out_stride))
    else:
        check(L.pm_mpsk_loop(ctx.handle, loops, nl, tab.ptr, pd.ptr, x0.ptr, x1.ptr, x_stride, n, o0.ptr, o1.ptr, out_stride))


def shapes_of(kind, n):
    """(loop_wide, loop_vec): the eight-loop tiles, the 64-loop tiles, the direct shape -- for the two-output loops with plain stores
    and through the transposing tiles.  The library takes the tiles only for eight samples or more from 16-byte aligned rows: for
    n < 8 and for pieces that begin at an odd sample (2, 1) runs the plain stores again.  The rows here are an even stride apart, and
    the *carry_2pi_even cases carry the phase of 2 pi across EVEN cuts with eight samples behind them, so the tiles start from it."""
    two = kind in ("qpsk", "mpsk")
    return [(0, 1), (1, 1), (2, 0)] + ([(2, 1)] if two else [])


def run_launch(ctx, tables, kind, names, shared, n, wide, vec):
    """One launch: lane l runs case names[l]'s parameters over its own input row, or over `shared`'s row (x_stride = 0)."""
    from pymodem_amd._native import Loop
    nl = len(names)
    stride = (n + 1) // 2 * 2 + 2                                          # even (16-byte rows for the transposing tiles) and padded
    want = [expect(p, shared or p, n) for p in names]
    rows = np.ascontiguousarray(np.stack([w[2] for w in want]))
    assert rows.shape == (nl, ctypes.sizeof(Loop) // 8)
    loops = (Loop * nl).from_buffer(rows)
    two = kind in ("qpsk", "mpsk")
    if shared:
        xs = E.case(shared)
        h0, h1 = xs["x0"][:n], (xs["x1"][:n] if kind == "mpsk" else None)
        x_stride = 0
    else:
        h0 = np.zeros((nl, stride))
        h1 = np.zeros((nl, stride)) if kind == "mpsk" else None
        for l, p in enumerate(names):
            h0[l, :n] = E.case(p)["x0"][:n]
            if h1 is not None:
                h1[l, :n] = E.case(p)["x1"][:n]
        x_stride = stride
    d0 = ctx.upload(h0.reshape(-1))
    d1 = ctx.upload(h1.reshape(-1)) if h1 is not None else None
    o0 = ctx.upload(np.full(nl * stride, SENTINEL))
    o1 = ctx.upload(np.full(nl * stride, SENTINEL)) if two else None
    with tuned(ctx, loop_wide=wide, loop_vec=vec):
        call(ctx, tables, kind, loops, nl, d0, d1, x_stride, n, o0, o1, stride)
    where = (kind, n, nl, "shared" if shared else "own", wide, vec)
    g0 = o0.download().reshape(nl, stride)
    g1 = o1.download().reshape(nl, stride) if two else None
    for l, (w0, w1, _, after) in enumerate(want):
        assert same_bytes(g0[l, :n], w0), (where, l, names[l], "out0", first_difference(g0[l, :n], w0))
        if two:
            assert same_bytes(g1[l, :n], w1), (where, l, names[l], "out1", first_difference(g1[l, :n], w1))
        if not same_bytes(rows[l], after):
            bad = [(f, rows[l][k], after[k]) for k, (f, _) in enumerate(Loop._fields_) if not same_bytes(rows[l][k:k + 1], after[k:k + 1])]
            raise AssertionError((where, l, names[l], "pm_loop", bad))
    assert np.all(g0[:, n:] == SENTINEL) and (g1 is None or np.all(g1[:, n:] == SENTINEL)), (where, "wrote past the row")


def lanes(kind, n, nl, turn=0):
    """nl lanes over the cases of `kind` that are at least n long, a different case in neighbouring lanes."""
    names = cases_of(kind, n)
    return [names[(l + turn) % len(names)] for l in range(nl)]


def shared_row(kind, n, names):
    """The row every lane reads when x_stride = 0: the slow case's noise (every loop's parameters stay far below the trip guard on it:
    expect() checks), or for lengths only one case has, that case's own."""
    slow = f"{kind}__slow"
    return slow if E.CASES[slow]["n"] >= n else names[0]


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("kind", E.LOOPS)
def test_loop_kernels_round_the_tiles(ctx, tables, kind, n):
    """Every case's first n samples, n round the tiles (32, 256) and the direct shape's eight-sample blocks: 1, 9, 64, 65 and 150 loops
    per launch, different cases in neighbouring lanes, own rows and one shared row, every shape."""
    for nl in COUNTS:
        names = lanes(kind, n, nl, turn=n)
        for wide, vec in shapes_of(kind, n):
            run_launch(ctx, tables, kind, names, None, n, wide, vec)
            run_launch(ctx, tables, kind, names, shared_row(kind, n, names), n, wide, vec)


@pytest.mark.parametrize("kind", E.LOOPS)
def test_loop_kernels_full_length(ctx, tables, kind):
    """Every case at its full length (the fixture's own outputs and end state, bit for bit the oracle's: test_oracle_loop_edges.py),
    beside the longer cases cut to that length, in every shape and loop count."""
    for n in full_lengths(kind):
        exact = [c for c in cases_of(kind, n) if E.CASES[c]["n"] == n]
        for c in exact:                                                 # the fixture itself, not only the oracle, is what is matched
            f, w = E.case(c), expect(c, c, n)
            assert np.array_equal(w[0], f["out0"]) and np.array_equal(w[3][10:19], f["state1"])
        for nl in COUNTS:
            names = (exact + lanes(kind, n, nl))[:nl]
            if nl == 1:
                for c in exact:
                    for wide, vec in shapes_of(kind, n):
                        run_launch(ctx, tables, kind, [c], None, n, wide, vec)
                continue
            for wide, vec in shapes_of(kind, n):
                run_launch(ctx, tables, kind, names, None, n, wide, vec)
                run_launch(ctx, tables, kind, names, shared_row(kind, n, names), n, wide, vec)


@pytest.mark.parametrize("kind", E.LOOPS)
def test_loop_kernels_in_pieces(ctx, tables, kind):
    """Every case in two and three calls (and cut where the generator put the phase on 2 pi at a piece's last sample), the pm_loop
    structs carried from call to call: outputs and end state are those of the one call."""
    from pymodem_amd._native import Loop
    two = kind in ("qpsk", "mpsk")
    for n in full_lengths(kind):
        names = [c for c in cases_of(kind, n) if E.CASES[c]["n"] == n]
        nl = len(names)
        want = [expect(p, p, n) for p in names]
        stride = (n + 1) // 2 * 2 + 2
        h0, h1 = np.zeros((nl, stride)), np.zeros((nl, stride))
        for l, p in enumerate(names):
            h0[l, :n] = E.case(p)["x0"]
            if kind == "mpsk":
                h1[l, :n] = E.case(p)["x1"]
        d0, d1 = ctx.upload(h0.reshape(-1)), ctx.upload(h1.reshape(-1))
        all_cuts = [c for k, c in enumerate(sum((E.cuts_of(p) for p in names), [])) if c]
        all_cuts = [c for k, c in enumerate(all_cuts) if c not in all_cuts[:k]]
        assert all_cuts or n == 1
        for cuts in all_cuts:
            for wide, vec in shapes_of(kind, n):
                rows = np.ascontiguousarray(np.stack([w[2] for w in want]))
                loops = (Loop * nl).from_buffer(rows)
                o0, o1 = ctx.upload(np.full(nl * stride, SENTINEL)), ctx.upload(np.full(nl * stride, SENTINEL))
                with tuned(ctx, loop_wide=wide, loop_vec=vec):
                    for a, b in E.pieces(n, cuts):
                        rest = nl * stride - a
                        call(ctx, tables, kind, loops, nl, d0.view(a, rest), d1.view(a, rest), stride, b - a, o0.view(a, rest), o1.view(a, rest), stride)
                g0, g1 = o0.download().reshape(nl, stride), o1.download().reshape(nl, stride)
                where = (kind, n, cuts, wide, vec)
                for l, (w0, w1, _, after) in enumerate(want):
                    assert same_bytes(g0[l, :n], w0), (where, names[l], "out0", first_difference(g0[l, :n], w0))
                    if two:
                        assert same_bytes(g1[l, :n], w1), (where, names[l], "out1", first_difference(g1[l, :n], w1))
                    assert same_bytes(rows[l], after), (where, names[l], "pm_loop", first_difference(rows[l], after))
                assert np.all(g0[:, n:] == SENTINEL) and (not two or np.all(g1[:, n:] == SENTINEL)), (where, "wrote past the row")


@pytest.mark.parametrize("wide", [0, 1, 2])
def test_detector_grid_every_pair_on_the_device(ctx, tables, wide):
    """pd_lookup's result for EVERY pair of the grid, seen on the device.  Run as one 20449-sample row (the cases above) the detector's
    result only feeds the loop filter, whose end state forgets all but the last thousand or so pairs; the outputs are the inputs.  So
    here every pair is a lane of its own with one sample: the lane's loop filter then holds x0 == e bit for bit when the launch ends.
    x0 is compared with the reference's get_qpsk_angle_error (the fixture's `pd`), the whole struct with the oracle's.  4096 lanes per
    launch, in each shape (the transposing tiles need eight samples: they change how outputs are stored, not what a lane computes)."""
    from pymodem_amd._native import Loop
    c = E.case("mpsk__grid")
    re, im, pd = c["x0"], c["x1"], c["pd"]
    total = len(re)
    before = np.concatenate([c["params"], c["state0"], np.zeros(9)])
    x0_at = [f for f, _ in Loop._fields_].index("x0")
    for at in range(0, total, 4096):
        nl = min(4096, total - at)
        after = np.empty((nl, len(before)))
        for l in range(nl):
            L, _ = E.oracle_loop(c)
            O.mpsk_loop(L, re[at + l:at + l + 1], im[at + l:at + l + 1])
            after[l] = np.concatenate([c["params"], [getattr(L, f) for f in E.STATE], np.zeros(9)])
        assert np.array_equal(after[:, x0_at], pd[at:at + nl].astype(np.float64))          # the oracle's loop holds e there too
        rows = np.ascontiguousarray(np.tile(before, (nl, 1)))
        loops = (Loop * nl).from_buffer(rows)
        h0, h1 = np.zeros((nl, 2)), np.zeros((nl, 2))
        h0[:, 0], h1[:, 0] = re[at:at + nl], im[at:at + nl]
        d0, d1 = ctx.upload(h0.reshape(-1)), ctx.upload(h1.reshape(-1))
        o0, o1 = ctx.upload(np.full(2 * nl, SENTINEL)), ctx.upload(np.full(2 * nl, SENTINEL))
        with tuned(ctx, loop_wide=wide):
            call(ctx, tables, "mpsk", loops, nl, d0, d1, 2, 1, o0, o1, 2)
        got = rows[:, x0_at]
        bad = np.flatnonzero(got.view(np.uint64) != pd[at:at + nl].astype(np.float64).view(np.uint64))
        assert len(bad) == 0, (wide, len(bad), [(float(re[at + k]), float(im[at + k]), float(got[k]), int(pd[at + k])) for k in bad[:8]])
        assert same_bytes(rows, after), (wide, at, first_difference(rows, after))
        g0, g1 = o0.download().reshape(nl, 2), o1.download().reshape(nl, 2)
        assert np.array_equal(g0[:, 0], re[at:at + nl]) and np.array_equal(g1[:, 0], im[at:at + nl])
        assert np.all(g0[:, 1] == SENTINEL) and np.all(g1[:, 1] == SENTINEL)


def test_agc_rows_on_the_edge_inputs(ctx, golden):
    """pm_agc_rows_apply (the engine's AGC: a lane per row) on the goldens' edge inputs -- an all-negative row (normal = max < 0), a row
    that starts with zeros (the envelope == 0 branch) -- and a row of zeros, whole and in pieces, against oracle.agc_apply and the
    reference's own outputs, as test_agc_bit_exact does for pm_agc_apply."""
    import pymodem_amd
    from pymodem_amd._native import AGCParams, check
    L = pymodem_amd.lib()
    g = golden("primitives")
    x = np.stack([g["agc_neg_in"], g["agc_zero_in"], np.zeros(len(g["agc_neg_in"]))])
    rows, n = x.shape
    p = AGCParams(500.0, 50.0, 0.01, 8000.0, 1.0)
    want, wstate = [], []
    for r in range(rows):
        buf, st = x[r].copy(), np.zeros(2)
        O.agc_apply(buf, 8000.0, 500.0, 0.01, 50.0, 1.0, state=st)
        want.append(buf)
        wstate.append(st)
    assert np.array_equal(want[0], g["agc_neg_out"]) and np.array_equal(want[1], g["agc_zero_out"]) and np.array_equal(want[2], x[2])
    stride = n + 6
    d_x = ctx.upload(np.pad(x, ((0, 0), (0, 6))).reshape(-1))
    mx = (ctypes.c_double * rows)()
    check(L.pm_rows_max_f64(ctx.handle, d_x.ptr, stride, rows, n, mx))
    assert list(mx) == [x[r].max() for r in range(rows)] and mx[0] < 0 and mx[2] == 0
    for cut in ([n], [1, 7, 8, 255, 256, n]):
        d_y = ctx.upload(np.full(rows * stride, SENTINEL))
        state = (ctypes.c_double * (2 * rows))()
        at = 0
        for piece in cut:
            cnt = min(piece, n - at)
            rest = rows * stride - at
            check(L.pm_agc_rows_apply(ctx.handle, d_x.view(at, rest).ptr, stride, d_y.view(at, rest).ptr, stride, rows, cnt, ctypes.byref(p), mx, state))
            at += cnt
        assert at == n
        got = d_y.download().reshape(rows, stride)
        for r in range(rows):
            assert same_bytes(got[r, :n], want[r]), (cut, r, first_difference(got[r, :n], want[r]))
            assert state[2 * r] == wstate[r][0] and state[2 * r + 1] == wstate[r][1], (cut, r)
        assert np.all(got[:, n:] == SENTINEL)


# ---- the engine on degenerate recordings ----------------------------------------------------------------------------------------------
def bits_of(buf, n):
    words = buf.download((n + 63) // 64)
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:n]


def group_modems(cfg, carriers):
    """[(config line, modem)]: the first chain of the config at each carrier, as a run of the engine takes them."""
    import json
    import os
    from conftest import GOLDEN
    from pymodem_amd import chain_builder as cb
    with open(os.path.join(GOLDEN, "configs", cfg)) as f:
        line = [l for l in (json.loads(t) for t in f if t.strip()) if l.get("object_type") == "demod_chain"][0]
    out = []
    for freq in carriers:
        ln = json.loads(json.dumps(line))
        ln["modem"]["options"]["carrier_freq"] = str(freq)
        ln["object_name"] += f" {freq}"
        out.append((ln, cb.ModemConfigurator(48000, ln["modem"])))
    return out


def degenerate_recordings():
    g = E.recordings()
    names = sorted(E.SUMMARY["recordings"])
    recs = [np.ascontiguousarray(g[f"rec__{k}"]) for k in names]
    return names + ["noise"], recs + [noise_i16(len(recs[0]), seed=4321)]


ENGINE = [("bpsk_300.json", [1500.0], [dict(loop_agc=a, bpf8_max=b, fir8=f) for a in (0, 1) for b in (0, 1) for f in (0, 1)]),
          ("qpsk_2400.json", [1475.0, 1500.0, 1525.0], [dict(loop_agc=a, bpf8_max=b) for a in (0, 1) for b in (0, 1)])]


@pytest.mark.parametrize("wide", [-1, 2])
@pytest.mark.parametrize("cfg,carriers,switch_sets", ENGINE, ids=[e[0][:-5] for e in ENGINE])
def test_engine_on_degenerate_recordings(ctx, cfg, carriers, switch_sets, wide):
    """Silence, both rails, a full-scale square, one impulse, a burst between silences, negative-only noise and, beside them in the
    same run, ordinary noise through LoopBatch.run in chunks of 2048: every bitmap is `>= 0` of the oracle's canonical chain, and
    modem.demod_signs() on each recording agrees.  (On the constant rails the band-pass leaves only its rounding residue, which the AGC
    normalises to full scale: those streams depend on the summation order, so the canonical oracle, not the reference, is the yardstick.)"""
    from pymodem_amd import chain_builder as cb
    from pymodem_amd.loop_batch import LoopBatch
    names, recs = degenerate_recordings()
    group = group_modems(cfg, carriers)
    want = {}
    for c, (line, _) in enumerate(group):
        for k, audio in enumerate(recs):
            d = O.build_chain(48000, line)[0].demod(audio, canon=True)
            want[k, c] = tuple(a >= 0 for a in (d if isinstance(d, tuple) else (d,)))
            r = cb.ModemConfigurator(48000, line["modem"]).demod_signs(audio)              # the per-recording path, default switches
            assert r.n == len(want[k, c][0]), (cfg, names[k], c)
            assert np.array_equal(bits_of(r.bits_i, r.n).astype(bool), want[k, c][0]), (cfg, names[k], c, "demod_signs I")
            if r.bits_q is not None:
                assert np.array_equal(bits_of(r.bits_q, r.n).astype(bool), want[k, c][1]), (cfg, names[k], c, "demod_signs Q")
    for switches in switch_sets:
        with tuned(ctx, loop_wide=wide, **switches):
            eng = LoopBatch([m for _, m in group_modems(cfg, carriers)], recordings=len(recs), ctx=ctx, chunk=2048)
            try:
                got = eng.run([ctx.upload(r) for r in recs])
                ctx.sync()
                for k in range(len(recs)):
                    for c in range(len(group)):
                        n = len(want[k, c][0])
                        assert got[k][c].n == n, (cfg, switches, wide, names[k], c)
                        assert np.array_equal(bits_of(got[k][c].bits_i, n).astype(bool), want[k, c][0]), (cfg, switches, wide, names[k], c, "I")
                        if len(want[k, c]) > 1:
                            assert np.array_equal(bits_of(got[k][c].bits_q, n).astype(bool), want[k, c][1]), (cfg, switches, wide, names[k], c, "Q")
            finally:
                eng.close()
