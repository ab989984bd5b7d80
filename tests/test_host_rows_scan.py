"""pm_host_decode_batch with h_data = NULL and h_scan given (the host half of pm_rows_scan's route: the block holds no raw slicer bytes, the
descrambled bytes and the register come from the scan part): the packets, the pending count and the register are those of the same job with
h_data set, on blocks written by the Python models (bitscan_model, frames_model, il2p_packets_model) -- scanned, framed and packets.  With
neither h_data nor h_scan the call still returns PM_ERR_ARG.  No GPU."""
import ctypes

import numpy as np
import pytest

import bitscan_model as M
import frames_model as FM
import il2p_packets_model as PM
from pymodem_amd._native import HostJob, check, lib, packet_dtype

REG = 0x1D2C3B4A59                                             # the register the model's record carries: it comes back from the block


def _codec(kind, tol=0, crc=True, disable_rs=False, min_dist=0):
    h = ctypes.c_void_p()
    check(lib().pm_codec_create(kind, int(crc), int(disable_rs), min_dist, tol, 3, ctypes.byref(h)))
    return h


def _fetch(h, pending):
    rows = np.zeros(max(1, pending), dtype=packet_dtype())
    got = ctypes.c_int64()
    check(lib().pm_codec_fetch(h, rows.ctypes.data, pending, ctypes.byref(got)))
    assert got.value == pending
    return [(int(r["streamaddress"]), bytes(r["data"][:r["len"]]), int(r["bytes_corrected"]), int(r["calculated_crc"]), int(r["carried_crc"]), int(r["valid_crc"]),
             int(r["valid_header"])) for r in rows[:pending]]


def _run(kind, codec_args, raw, steps, first, block, frames=0, packets=0, wide=False, copy=False):
    """one job through pm_host_decode_batch; raw None: h_data = NULL.  -> (status, register, pending, packets, copy of the bytes)"""
    h = _codec(kind, **codec_args)
    n = len(steps)
    seen = np.zeros(max(n, 1), dtype=np.uint8)
    addr = first + np.cumsum(steps.astype(np.int64))
    jobs = (HostJob * 1)()
    j = jobs[0]
    j.codec, j.n = h, n
    j.h_data = None if raw is None else raw.ctypes.data
    if wide:
        j.h_addr = addr.ctypes.data
    else:
        j.h_addr, j.h_addr_delta, j.addr_first = None, steps.ctypes.data, first
    j.lfsr_poly, j.lfsr_state, j.lfsr_invert = 0x1, 0, 1
    j.h_plain = seen.ctypes.data if copy else None
    j.h_scan = None if block is None else block.ctypes.data
    j.scan_frames, j.scan_packets = frames, packets
    rc = lib().pm_host_decode_batch(jobs, 1, 1)
    out = (rc, int(j.lfsr_state), int(j.pending), _fetch(h, int(j.pending)) if rc == 0 else None, seen[:n].tobytes())
    lib().pm_codec_destroy(h)
    return out


def _steps(n, seed):
    s = np.random.default_rng(seed).integers(300, 340, n).astype(np.uint16)
    if n:
        s[0] = 0
    return s


AX25 = ["random1", "len18_17_at3", "frame1100", "bail_after_a_flag", "short0", "short1", "short25", "survive_at2", "long_no_bail", "two_flags_one_word", "many_frames"]
IL2P = ["count240_crc", "count0_nocrc", "block_errors", "block_errors_min_dist1", "late_hit", "area_runs_out", "short4", "back_to_back"]


@pytest.mark.parametrize("name", AX25)
@pytest.mark.parametrize("frames", [0, 1])
def test_ax25_without_the_raw_bytes_equals_the_job_with_them(name, frames):
    plain = np.ascontiguousarray(FM.all_streams()[name])
    raw = np.bitwise_not(plain)                               # the identity polynomial, inverted
    steps = _steps(len(plain), len(plain))
    block = np.ascontiguousarray(FM.model_block_frames(plain, REG)[0] if frames else M.model_block(plain, 0, 0, REG))
    bare = _run(0, {}, None, steps, 77, block, frames=frames, copy=True)
    full = _run(0, {}, raw, steps, 77, block, frames=frames, copy=True)
    plainly = _run(0, {}, raw, steps, 77, None)
    assert bare[0] == 0 and bare == full
    assert bare[1] == REG, "the register is the record's"
    assert bare[4] == plain.tobytes(), "h_plain receives the block's bytes"
    assert bare[2:4] == plainly[2:4], "and the packets are those of the host's own LFSR and decoder"
    assert _run(0, {}, None, steps, 77, block, frames=frames, wide=True)[:4] == bare[:4], "wide addresses as well as steps"


@pytest.mark.parametrize("name", IL2P)
@pytest.mark.parametrize("packets", [0, 1])
def test_il2p_without_the_raw_bytes_equals_the_job_with_them(name, packets):
    plain, tol, o = PM.all_streams()[name]
    plain = np.ascontiguousarray(plain)
    raw = np.bitwise_not(plain)
    steps = _steps(len(plain), 5 + len(plain))
    block = np.ascontiguousarray(PM.model_block_packets(plain, tol, lfsr_state=REG, **o)[0] if packets else M.model_block(plain, 1, tol, REG))
    args = dict(tol=tol, **o)
    bare = _run(1, args, None, steps, 9000, block, packets=packets, copy=True)
    full = _run(1, args, raw, steps, 9000, block, packets=packets, copy=True)
    plainly = _run(1, args, raw, steps, 9000, None)
    assert bare[0] == 0 and bare == full and bare[1] == REG and bare[4] == plain.tobytes()
    assert bare[2:4] == plainly[2:4]


def test_the_streams_hold_packets():
    """what the comparisons above are worth: frames and packets are decoded"""
    frames = sum(_run(0, {}, None, _steps(len(FM.all_streams()[n]), 1), 0, np.ascontiguousarray(FM.model_block_frames(FM.all_streams()[n], 0)[0]), frames=1)[2] for n in AX25)
    assert frames >= 600
    done = 0
    for name in IL2P:
        plain, tol, o = PM.all_streams()[name]
        done += _run(1, dict(tol=tol, **o), None, _steps(len(plain), 2), 0, np.ascontiguousarray(PM.model_block_packets(plain, tol, lfsr_state=0, **o)[0]), packets=1)[2]
    assert done >= 130


def test_neither_bytes_nor_scan_is_an_argument_error():
    steps = _steps(64, 3)
    assert _run(1, {}, None, steps, 0, None)[0] == -2          # PM_ERR_ARG
    assert _run(0, {}, None, steps, 0, None, wide=True)[0] == -2
    # an empty job needs neither
    assert _run(1, {}, None, _steps(0, 3), 0, None)[0] == 0
    # and the addresses are still asked for
    h = _codec(1)
    block = np.ascontiguousarray(M.model_block(np.zeros(64, np.uint8), 1, 0, 0))
    jobs = (HostJob * 1)()
    jobs[0].codec, jobs[0].n, jobs[0].h_scan = h, 64, block.ctypes.data
    assert lib().pm_host_decode_batch(jobs, 1, 1) == -2
    lib().pm_codec_destroy(h)
