"""pm_stream_packets (csrc/pm_bitscan.hip with the rules of pm_rows_packets.h): the packets of the jobs of a pm_stream_scan call, finished
on the device in the dense form.  Synthetic streams are scanned into a device block and finished behind it; every record of every finished
job must be, bit for bit, what pm_codec_decode + pm_codec_fetch hand out for a just-created codec on the same descrambled bytes and
addresses, every entry's register the host LFSR's, and head, statuses, counts and offsets what tests/stream_packets_model.py says
(test_stream_packets_model.py holds that to the oracle's decoders and fixes which streams are handed over, and why).  The shapes are where the
kernels can go wrong: 0, 1, 63, 64, 65 and 129 listed events for the walk's trips and their carry, a first flag that closes nothing, a frame
longer than PM_PKT_MAX, short streams, bails, n = 0; the 49 IL2P streams in one call; 64 mixed jobs, one alone, two on one d_data; room
exact and 8 bytes short; d_out in device and in page-locked host memory; addresses with steps above 65 535; the scan's tile size and the
build's waves; the refusals."""
import ctypes
import functools

import numpy as np
import pytest

import bitscan_model as M
import rows_packets_model as RP
import stream_packets_model as SP
from conftest import tuned
from pymodem_amd import _native as N
from pymodem_amd._native import ScanJob, check, lib
from test_gpu_rows_scan import host_lfsr

pytestmark = pytest.mark.gpu

CANARY = 0xC7
G3RUH = 0x21001
ARG, CAPACITY = -2, -4                                      # PM_ERR_ARG, PM_ERR_CAPACITY


def _ctx():
    import pymodem_amd
    return pymodem_amd.Context.default()


@functools.lru_cache(maxsize=None)
def _raw(name, kind):
    """(slicer bytes, poly, register, invert) whose LFSR output is the job's stream: the long ones through the identity polynomial inverted,
    the short ones through G3RUH's with its seventeen bits of history"""
    plain = _by_name()[name]["plain"]
    if kind < 0:
        return plain, 0x1, 0, 0                             # (descramble only: the bytes are the slicer's, whatever they give)
    if len(plain) > 4096 or len(plain) == 0:
        return np.bitwise_not(plain), 0x1, 0, 1
    bits = M.siggen.lfsr_scramble(np.unpackbits(plain).tolist(), G3RUH, True)
    raw = np.packbits(np.array(bits, dtype=np.uint8))
    assert np.array_equal(host_lfsr(raw, G3RUH, 0, True)[0], plain)
    return raw, G3RUH, 0, 1


@functools.lru_cache(maxsize=None)
def _by_name():
    """the model's jobs by name, the IL2P ones with "il2p:" in front (both sets have a short0)"""
    out = {j["name"]: j for j in SP.ax25_jobs() + SP.events_jobs()}
    for j in SP.il2p_jobs():
        out["il2p:" + j["name"]] = dict(j, name="il2p:" + j["name"])
    assert len(out) == len(SP.ax25_jobs()) + len(SP.events_jobs()) + 49
    out["none"] = SP.job(-1, out["shared_zero"]["plain"], source=9)
    out["none"].update(name="none", disable_rs=False, min_dist=0)
    return out


@functools.lru_cache(maxsize=None)
def _walk(name):
    if name.startswith("il2p:"):
        return SP.il2p_walks()[IL2P.index(name)]
    return SP.job_packets(_by_name()[name])


@functools.lru_cache(maxsize=None)
def _host_decoder(name, source):
    """pm_codec_decode + pm_codec_fetch of a fresh codec on the stream's bytes and addresses -> the pm_packet rows"""
    j = _by_name()[name]
    h, pending, got = ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int64()
    check(lib().pm_codec_create(j["kind"], int(j["crc"]), int(j["disable_rs"]), int(j["min_dist"]), j["tol"], source, ctypes.byref(h)))
    plain, addr = np.ascontiguousarray(j["plain"]), np.ascontiguousarray(j["addr"], dtype=np.int64)
    check(lib().pm_codec_decode(h, plain.ctypes.data, addr.ctypes.data, len(plain), ctypes.byref(pending)))
    rows = np.zeros(max(1, pending.value), dtype=N.packet_dtype())
    check(lib().pm_codec_fetch(h, rows.ctypes.data, pending.value, ctypes.byref(got)))
    lib().pm_codec_destroy(h)
    assert got.value == pending.value
    return rows[:got.value]


class _Pinned:
    """page-locked host memory that the device reaches by the same pointer (the runtime's own host allocation, which the library links and
    the executor's host blocks are made of), filled with the canary"""

    def __init__(self, nbytes):
        rt = lib()                                          # (a symbol of a library that this one depends on is found through it)
        rt.hipHostMalloc.argtypes, rt.hipHostMalloc.restype = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t, ctypes.c_uint], ctypes.c_int
        rt.hipHostFree.argtypes, rt.hipHostFree.restype = [ctypes.c_void_p], ctypes.c_int
        self.ptr, self.nbytes = ctypes.c_void_p(), nbytes
        assert rt.hipHostMalloc(ctypes.byref(self.ptr), nbytes, 0) == 0 and self.ptr.value
        self.view()[:] = CANARY

    def view(self):
        return np.ctypeslib.as_array(ctypes.cast(self.ptr, ctypes.POINTER(ctypes.c_uint8)), shape=(self.nbytes,))

    def free(self):
        lib().hipHostFree(self.ptr)


def stream_packets(names, room, tile=0, waves=0, pinned=False, shared_data=False, host_block=False, carry=False, addrs=0, repeat_jobs=1):
    """pm_stream_scan of the named jobs into a device block and pm_stream_packets behind it, `room` bytes for records.
    -> (status, head, entries, records, bytes behind the room)"""
    ctx = _ctx()
    jobs = [_by_name()[n] for n in names]
    raws = [_raw(j["name"], j["kind"]) for j in jobs]
    shared, dbufs, abufs = {}, [], []
    for j, r in zip(jobs, raws):
        if not (shared_data and j["name"] in shared):
            shared[j["name"]] = ctx.upload(r[0] if len(r[0]) else np.zeros(8, np.uint8))
        dbufs.append(shared[j["name"]])
        abufs.append(ctx.upload(j["addr"] if len(j["addr"]) else np.zeros(1, np.int64)))
    arr = (ScanJob * len(jobs))()
    for q, b, a, j, r in zip(arr, dbufs, abufs, jobs, raws):
        q.d_data, q.n, q.lfsr_poly, q.lfsr_state, q.lfsr_invert, q.codec_kind, q.sync_tol = b.ptr.value, len(j["plain"]), r[1], r[2], r[3], j["kind"], j["tol"]
        q.frames, q.packets = int(j["kind"] == 0), int(j["kind"] == 1)
        q.il2p_crc, q.il2p_disable_rs, q.il2p_min_dist = int(j["crc"]), int(j["disable_rs"]), int(j["min_dist"])
        q.d_addr, q.addrs = a.ptr.value, addrs
    njobs = len(jobs) * repeat_jobs
    need = sum(N.scan_part_bytes(j["kind"], j["kind"] == 0, j["kind"] == 1, len(j["plain"]), addrs) for j in jobs)
    block = ctx.upload(np.full(need + 64, 0xA5, dtype=np.uint8))
    offs, used = (ctypes.c_int64 * max(njobs, 1))(), ctypes.c_size_t()
    sources = (ctypes.c_int32 * max(njobs, 1))(*[j["source"] for j in jobs])
    out_bytes = N.stream_packets_bytes(len(jobs), room)
    total = out_bytes + 64
    host = _Pinned(total) if pinned else None
    out = None if pinned else ctx.upload(np.full(total, CANARY, dtype=np.uint8))
    d_out = host.ptr if pinned else out.ptr
    with tuned(ctx, bitscan_tile_words=tile, bitscan_packet_waves=waves):
        check(lib().pm_stream_scan(ctx.handle, arr, len(jobs), block.ptr, need, offs, ctypes.byref(used)))
        assert used.value == need
        if carry:
            arr[len(jobs) - 1].d_carry = block.ptr.value
        here = np.zeros(64, dtype=np.uint8)
        rc = lib().pm_stream_packets(ctx.handle, arr, njobs, sources, here.ctypes.data if host_block else block.ptr, offs, d_out, out_bytes, ctypes.byref(used))
    ctx.sync()
    raw = host.view().copy() if pinned else out.download()
    if pinned:
        host.free()
    if rc != 0:
        return rc, used.value, None, None, None
    assert used.value == N.stream_packets_bytes(len(jobs))
    head = raw[:32].view(N.stream_packets_head_dtype())
    entries = raw[32:used.value].view(N.stream_packets_entry_dtype())
    kept = int(head["bytes"][0])
    assert 0 <= kept <= room and kept % 8 == 0
    return rc, head, entries, raw[:used.value + kept], raw[used.value + kept:]


def _compare(names, room, got):
    rc, head, entries, raw, behind = got
    jobs = [_by_name()[n] for n in names]
    want_head, want_entries, want_records = SP.model_call(jobs, room, [_walk(n) for n in names])
    assert rc == 0
    assert head.tobytes() == want_head.tobytes(), (head, want_head)
    for field in ("status", "packets", "first_byte", "corrected_left", "reserved"):
        bad = np.flatnonzero(entries[field] != want_entries[field])
        assert len(bad) == 0, (field, names[int(bad[0])], entries[bad[0]], want_entries[bad[0]])
    for j, e in zip(jobs, entries):
        r = _raw(j["name"], j["kind"])
        assert int(e["lfsr_state"]) == host_lfsr(r[0], *r[1:])[1], (j["name"], "the register behind the stream")
    assert (behind == CANARY).all(), "nothing is stored behind the records"
    base = N.stream_packets_bytes(len(jobs))
    assert raw[base:].tobytes() == want_records.tobytes(), "the records are the model's"
    # the reference: the host decoder on the same bytes and addresses, bit for bit
    for j, e in zip(jobs, entries):
        if e["status"] != RP.FINISHED:
            continue
        rows = _host_decoder(j["name"], j["source"])
        assert len(rows) == int(e["packets"]), j["name"]
        at = base + int(e["first_byte"])
        for q in range(len(rows)):
            size = N.stream_packets_record_bytes(int(rows["len"][q]))
            assert raw[at:at + size].tobytes() == rows[q:q + 1].tobytes()[:size], (j["name"], q)
            at += size
    return entries


AX25 = [j["name"] for j in SP.ax25_jobs()]
EVENTS = [j["name"] for j in SP.events_jobs()]
IL2P = ["il2p:" + j["name"] for j in SP.il2p_jobs()]
ROOM = 1 << 18


def _total(names):
    return int(SP.model_call([_by_name()[n] for n in names], 10 ** 9, [_walk(n) for n in names])[0]["bytes"][0])


def test_ax25_streams_at_the_trip_edges_and_the_rule_s():
    names = EVENTS + AX25
    entries = _compare(names, ROOM, stream_packets(names, ROOM))
    by = dict(zip(names, entries))
    assert [int(by[f"events{k}"]["packets"]) for k in SP.EVENT_COUNTS] == [0, 0, 62, 63, 64, 128], "a first flag that closes nothing, then a frame a flag"
    assert all(by[f"events{k}"]["status"] == RP.FINISHED for k in SP.EVENT_COUNTS)
    assert by["short23"]["status"] == RP.SHORT and by["short0"]["status"] == RP.SHORT and by["short24"]["status"] == RP.FINISHED
    assert by["bail_at_once"]["status"] == RP.BAIL and by["frame1100"]["status"] == RP.BAIL
    assert by["long_no_bail"]["status"] == RP.FINISHED and by["long_no_bail"]["packets"] == 1, "a frame longer than PM_PKT_MAX is cut, not handed over"
    assert by["first_closes"]["packets"] == 1


def test_the_49_il2p_streams_in_one_call():
    entries = _compare(IL2P, ROOM, stream_packets(IL2P, ROOM))
    assert int((entries["status"] == RP.FINISHED).sum()) == 40
    seen = {RP.STATUS[s] for s in entries["status"]}
    assert {"FINISHED", "INCOMPLETE", "NOT_PLACED", "LATE_HIT", "TABLE_FULL"} <= seen
    by = dict(zip(IL2P, entries))
    for name in ("il2p:back_to_back", "il2p:block_errors", "il2p:resync_tol2"):
        assert by[name]["status"] == RP.FINISHED and by[name]["packets"] >= 1
    assert any(not _by_name()[n]["crc"] and by[n]["packets"] for n in IL2P) and any(_by_name()[n]["crc"] and by[n]["packets"] for n in IL2P), "DONE with and without CRC"


@functools.lru_cache(maxsize=None)
def _mix():
    """64 jobs of mixed kinds, a descramble-only job among them now and then"""
    names = []
    for k in range(64):
        src = (IL2P, AX25 + EVENTS)[k % 2]
        names.append("none" if k % 7 == 3 else src[(5 * k) % len(src)])
    return names


def test_job_mixes():
    names = _mix()
    entries = _compare(names, ROOM, stream_packets(names, ROOM))
    assert int((entries["status"] == RP.NO_CODEC).sum()) == 9
    _compare(["random1"], ROOM, stream_packets(["random1"], ROOM))                                    # one job alone
    _compare(["shared_zero", "shared_zero"], ROOM, stream_packets(["shared_zero", "shared_zero"], ROOM, shared_data=True))      # two jobs on one d_data


@pytest.mark.parametrize("pinned", [False, True])
def test_room_exact_and_8_bytes_short_in_device_and_in_page_locked_host_memory(pinned):
    names = AX25 + EVENTS
    total = _total(names)
    entries = _compare(names, total, stream_packets(names, total, pinned=pinned))
    last = int(np.flatnonzero(entries["packets"] > 0)[-1])
    short = _compare(names, total - 8, stream_packets(names, total - 8, pinned=pinned))
    assert (short["status"][last:] == RP.NO_ROOM).all() and (short["status"][:last] != RP.NO_ROOM).all()
    _compare(names, total - 1, stream_packets(names, total - 1, pinned=pinned))
    _compare(names, 0, stream_packets(names, 0, pinned=pinned))
    rc, used, _, _, _ = stream_packets(names, -8, pinned=pinned)
    assert rc == CAPACITY and used == N.stream_packets_bytes(len(names))


def test_addresses_with_steps_above_65535_still_finish():
    for name in ("events65", IL2P[0]):
        assert int(np.diff(_by_name()[name]["addr"]).max()) > 65535
    entries = _compare(["events65", "il2p:back_to_back"], ROOM, stream_packets(["events65", "il2p:back_to_back"], ROOM, addrs=1))
    assert (entries["status"] == RP.FINISHED).all() and (entries["packets"] > 0).all()


@pytest.mark.parametrize("tile,waves", [(1, 0), (256, 0), (0, 1)])
def test_tile_size_and_build_waves_change_nothing(tile, waves):
    names = EVENTS + IL2P[:20] + AX25[:6]
    _compare(names, ROOM, stream_packets(names, ROOM, tile=tile, waves=waves))


def test_refusals():
    names = ["shared_zero", "il2p:back_to_back"]
    assert stream_packets(names, 4096, host_block=True)[0] == ARG, "a block in host memory"
    assert stream_packets(names, 4096, carry=True)[0] == ARG, "a job with a carry"
    assert stream_packets(names[:1], 4096, repeat_jobs=65)[0] == ARG, "65 jobs"
    ctx = _ctx()
    arr = (ScanJob * 1)()
    data = ctx.upload(np.zeros(64, np.uint8))
    offs, used = (ctypes.c_int64 * 1)(), ctypes.c_size_t()
    arr[0].d_data, arr[0].n, arr[0].lfsr_poly, arr[0].codec_kind, arr[0].d_addr = data.ptr.value, 64, 1, 0, data.ptr.value
    call = lambda out=data.ptr.value: lib().pm_stream_packets(ctx.handle, arr, 1, None, data.ptr, offs, out, 64, ctypes.byref(used))
    assert call() == ARG, "kind 0 without frames"
    arr[0].frames = 1
    assert call(data.ptr.value + 4) == ARG, "d_out not 8-byte aligned"
    arr[0].d_addr = None
    assert call() == ARG, "a codec without addresses"
    arr[0].codec_kind, arr[0].frames, arr[0].d_addr = 1, 0, data.ptr.value
    assert call() == ARG, "kind 1 without packets"
    ctx.sync()
