"""pm_rows_scan with pm_rows_scan_chain.addrs (csrc/pm_bitscan.hip: the tile launch's sums, the combine's int64 carry, rows_addrs_kernel): the
address checkpoints at the end of every row's part against addrs_model's prefix sum over the row's 16-bit steps -- 300 rows, so that the
prepare launch takes a second trip, three chains of kinds 0, 1 and -1, counts at the table's and the tiles' edges, a count above the rows'
room, a row of 70 000 bytes whose steps are all 65535 (its prefix passes 32 bits), and a row that the records make longer than the host's
counts say, which is left out, and with it the two short rows behind it, whose first tiles the table clips to the limit -- with the rest of every part what pm_rows_scan writes without addrs; and the batch engine's executor with
addrs on against the executor with it off."""
import ctypes
import functools

import numpy as np
import pytest

import addrs_model as AM
from conftest import tuned
from pymodem_amd import _native as N
from pymodem_amd._native import lib

pytestmark = pytest.mark.gpu

CAP, ROWS = 70000, 300
FIRST = (1 << 40) + 3
EDGES = [0, 1, 63, 64, 65, 2047, 2048, 2049]
FULL, OVER, LEFT_OUT = 100, 200, ROWS - 3                      # all steps 65535; a count above cap; longer on the device than the host was told
CHAINS = [(0x1, 0, 1, 0, 0, 1, 0), (0x21001, 0x155, 1, 1, 1, 0, 1), (0x63003, 0x1234567, 0, -1, 0, 0, 0)]     # (poly, register, invert, kind, tol, frames, packets)


def _ctx():
    import pymodem_amd
    return pymodem_amd.Context.default()


@functools.lru_cache(maxsize=None)
def _rows():
    """-> (data, steps, records, the host's counts): made once, never changed"""
    rng = np.random.default_rng(300)
    counts = rng.integers(0, 3001, ROWS)
    for k, e in enumerate(EDGES * 3):                          # every edge in every kind
        counts[3 + k] = e
    counts[FULL], counts[OVER], counts[LEFT_OUT] = CAP, CAP + 100, 900
    counts[LEFT_OUT + 1:] = 5, 40                              # rows behind it: the sums in front of them have passed the limit already
    data = rng.integers(0, 256, ROWS * CAP, dtype=np.uint8)
    steps = rng.integers(0, 65536, ROWS * CAP, dtype=np.uint16)          # (what lies past a row's count must not be added)
    steps[FULL * CAP:(FULL + 1) * CAP] = 65535
    recs = np.zeros(ROWS, dtype=N.rowslice_dtype())
    recs["count"] = counts
    recs["first_addr"] = FIRST + 1000 * np.arange(ROWS)
    told = np.minimum(counts, CAP)
    told[LEFT_OUT] = 100                                       # the records say 900: the row's part would pass what the host sized
    return data, steps, recs, told


@functools.lru_cache(maxsize=None)
def _device():
    ctx = _ctx()
    data, steps, recs, _ = _rows()
    return ctx.upload(data), ctx.upload(steps), ctx.upload(recs.view(np.uint8))


def _desc(addrs):
    desc = (N.RowsScanChain * len(CHAINS))()
    for c, (d, (poly, reg, invert, kind, tol, frames, packets)) in enumerate(zip(desc, CHAINS)):
        d.lfsr_poly, d.lfsr_state, d.lfsr_invert, d.codec_kind, d.sync_tol, d.frames, d.packets = poly, reg, invert, kind, tol, frames, packets
        d.il2p_crc, d.addrs = 1, int(addrs[c])
    return desc


def _sizes(told, addrs):
    return [N.rows_scan_steps_bytes(int(n)) + N.scan_part_bytes(CHAINS[r % 3][3], CHAINS[r % 3][5], CHAINS[r % 3][6], int(n), addrs[r % 3]) for r, n in enumerate(told)]


def rows_scan(addrs, tile=0):
    """-> (host copy of the block, offsets, sizes)"""
    ctx = _ctx()
    d_data, d_steps, d_recs = _device()
    told = _rows()[3]
    sizes = _sizes(told, addrs)
    need = sum(sizes)
    block = ctx.upload(np.full(need + 64, 0xA5, dtype=np.uint8))
    h_counts = (ctypes.c_int64 * ROWS)(*[int(n) for n in told])
    offs, used = (ctypes.c_int64 * ROWS)(), ctypes.c_size_t()
    with tuned(ctx, bitscan_tile_words=tile):
        rc = lib().pm_rows_scan(ctx.handle, d_recs.ptr, d_data.ptr, d_steps.ptr, CAP, 0, ROWS, _desc(addrs), len(CHAINS), h_counts, block.ptr, need, offs,
                                ctypes.byref(used))
    assert rc == 0 and used.value == need
    ctx.sync()
    host = block.download()
    assert (host[need:] == 0xA5).all(), "nothing is written behind *h_used"
    assert list(offs) == [int(x) for x in np.concatenate(([0], np.cumsum(sizes)))[:-1]]
    return host, list(offs), sizes


@functools.lru_cache(maxsize=None)
def _without(tile):
    return rows_scan((0, 0, 0), tile)


@pytest.mark.parametrize("tile,addrs", [(0, (1, 1, 1)), (1, (1, 1, 1)), (3, (1, 1, 1)), (17, (1, 1, 1)), (255, (1, 1, 1)), (0, (0, 1, 0))])
def test_rows_checkpoints_equal_the_prefix_sum_and_the_rest_is_untouched(tile, addrs):
    _, steps, recs, told = _rows()
    host, offs, sizes = rows_scan(addrs, tile)
    bare, bare_offs, bare_sizes = _without(tile)
    places = 0
    for r in range(ROWS):
        n = int(told[r])
        got = host[offs[r]:offs[r] + sizes[r]]
        if r >= LEFT_OUT:
            assert (got == 0xA5).all(), (r, "nothing is stored for a row that the table leaves out, nor for the rows behind it")
            continue
        want = bare[bare_offs[r]:bare_offs[r] + bare_sizes[r]]
        assert len(got) == len(want) + (N.scan_addr_bytes(n) if addrs[r % 3] else 0), r
        assert np.array_equal(got[:len(want)], want), (r, "the steps and every piece of the scan part are what they are without addrs")
        if addrs[r % 3]:
            table = got[len(want):].view("<i8")
            assert np.array_equal(table, AM.checkpoints(int(recs["first_addr"][r]), steps[r * CAP:r * CAP + n])), (r, n, tile)
            places += len(table)
    assert places >= 1000
    if addrs[FULL % 3]:
        last = int(host[offs[FULL] + sizes[FULL] - 8:offs[FULL] + sizes[FULL]].view("<i8")[0])
        assert last - int(recs["first_addr"][FULL]) == 65535 * 64 * ((CAP - 1) // 64) > 1 << 32, "a stream's sum does not fit 32 bits"


def test_the_rows_are_what_the_checks_are_worth():
    """no GPU work"""
    _, _, recs, told = _rows()
    assert ROWS > 256 and {0, 1, 63, 64, 65, 2047, 2048, 2049, CAP} <= set(int(x) for x in told)
    assert int(recs["count"][OVER]) > CAP and int(told[OVER]) == CAP and int(recs["count"][LEFT_OUT]) > int(told[LEFT_OUT])
    assert {r % 3 for r in range(3, 3 + 3 * len(EDGES))} == {0, 1, 2}
    # the table leaves a row out when the sums up to its end pass what the host sized; the sums only grow, so the rows behind it go too
    assert LEFT_OUT == ROWS - 3 and 0 < int(told[-2]) < int(told[-1]) < int(told[LEFT_OUT]), "two rows with bytes lie behind the left-out row"


# ---- through the batch engine's executor ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("as_rows", [True, False])
@pytest.mark.parametrize("packets", [False, True])
@pytest.mark.parametrize("mode,cfg", [("qpsk2400_il2p", "qpsk_2400.json"), ("bpsk300_il2p", "bpsk_300.json")])
def test_executor_with_addrs_equals_the_executor_without(mode, cfg, packets, as_rows):
    import test_gpu_rows_scan as RS
    from pymodem_amd.loop_batch import process_recordings_device
    recs = RS._recordings(mode)
    want, registers, _ = RS._plainly(mode, cfg, as_rows)
    sets = RS._chain_sets(RS.lines_of(cfg), len(recs))
    stages = {}
    got = process_recordings_device(sets, recs, chunk=8192, rows=as_rows, stages=stages, scan=False, frames=False, packets=packets, addrs=True)
    assert stages.get("scanned") is True and stages.get("fused_slicers"), "addrs implies the scan"
    assert RS._rows_of(got, as_rows) == want
    assert [[ch[3].shift_register for ch in cs] for cs in sets] == registers
    assert sum(len(chain) // (N.packet_dtype().itemsize if as_rows else 1) for rec in want for chain in rec) >= 1, "at least one packet is decoded"
    lookups = 0
    for cs in sets:
        for ch in cs:
            a, b = ctypes.c_int64(), ctypes.c_int64()
            assert lib().pm_codec_addr_work(ch[4]._handle(), ctypes.byref(a), ctypes.byref(b)) == 0
            assert b.value <= 63 * a.value
            lookups += a.value
    assert lookups >= 1, "the addresses came from checkpoints"


def test_the_switch_defaults_to_the_context_s():
    import test_gpu_rows_scan as RS
    from pymodem_amd.loop_batch import process_recordings_device
    ctx = _ctx()
    mode, cfg = "bpsk300_il2p", "bpsk_300.json"
    recs = RS._recordings(mode)
    want, _, _ = RS._plainly(mode, cfg, True)
    with tuned(ctx, pipe_addrs=1):
        stages = {}
        assert RS._rows_of(process_recordings_device(RS._chain_sets(RS.lines_of(cfg), len(recs)), recs, chunk=8192, rows=True, stages=stages), True) == want
        assert stages.get("scanned") is True
