#!/usr/bin/env python3
"""The scanned host routes with and without address checkpoints on ONE core, no GPU: pm_host_decode_batch on the framed route (a 200 000-byte
AX.25 stream, two thirds of it frames of 60-250 bytes) and on the packets route (a 200 000-byte IL2P stream, a packet about every 400
bytes), the blocks from the tests' bit-serial models with the model's checkpoints behind them; the job with its 16-bit steps expanded
(scan_addrs = 0) against the job that resolves addresses from the checkpoints (scan_addrs = 1).  Then the places where a look-up is paid
for and no packet comes of it: the event-list route over the same two streams, and all three routes over 200 000 bytes of noise.
ns per stream byte, best of 7, three rounds.  Its figures are in profiles/scan_addrs_ab.txt."""
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import addrs_model as AM                                              # noqa: E402
import bitscan_model as M                                             # noqa: E402
import frames_model as FM                                             # noqa: E402
import il2p_packets_model as PM                                       # noqa: E402
from pymodem_amd import siggen                                        # noqa: E402
from pymodem_amd._native import HostJob, check, lib                   # noqa: E402

N = 200_000


def framed_plain(rng):
    bits = []
    while len(bits) < 8 * N:
        bits += (rng.random(int(rng.integers(2000, 6000))) < 0.5).astype(np.uint8).tolist()
        for _ in range(int(rng.integers(4, 9))):
            bits += siggen.ax25_hdlc_bits([int(b) for b in rng.integers(0, 256, int(rng.integers(60, 250)))], pre_flags=1, post_flags=0)
        bits += [0, 1, 1, 1, 1, 1, 1, 0]
    return np.packbits(np.array(bits[:8 * N], dtype=np.uint8))


def packets_plain(rng):
    data = rng.integers(0, 256, N, dtype=np.uint8)
    at = 100
    while at + 400 < N:
        frame = np.packbits(np.array(siggen.il2p_frame_bits("CQ", "N0CAL", [int(b) for b in rng.integers(0, 256, int(rng.integers(20, 251)))], preamble=4), dtype=np.uint8))
        data[at:at + len(frame)] = frame
        at += len(frame) + int(rng.integers(60, 420))
    return data


def measure(name, kind, plain, part, frames, packets, opts):
    steps = np.full(N, 320, dtype=np.uint16)
    steps[0] = 0
    block = AM.with_checkpoints(part, 100, steps)
    raw = np.bitwise_not(plain)
    for scan_addrs in (0, 1):
        rounds = []
        for _ in range(3):
            best = 1e9
            for _ in range(7):
                h = ctypes.c_void_p()
                check(lib().pm_codec_create(kind, *opts, 0, ctypes.byref(h)))
                jobs = (HostJob * 1)()
                j = jobs[0]
                j.codec, j.h_data, j.h_addr, j.n = h, raw.ctypes.data, None, N
                j.h_addr_delta, j.addr_first = steps.ctypes.data, 100
                j.lfsr_poly, j.lfsr_invert = 0x1, 1
                j.h_scan, j.scan_frames, j.scan_packets, j.scan_addrs = block.ctypes.data, frames, packets, scan_addrs
                t0 = time.perf_counter()
                check(lib().pm_host_decode_batch(jobs, 1, 1))
                best = min(best, time.perf_counter() - t0)
                pending = j.pending
                a, b = ctypes.c_int64(), ctypes.c_int64()
                check(lib().pm_codec_addr_work(h, ctypes.byref(a), ctypes.byref(b)))
                lib().pm_codec_destroy(h)
            rounds.append(best / N * 1e9)
        print(f"{name:15s} scan_addrs={scan_addrs}: {min(rounds):.3f}-{max(rounds):.3f} ns per stream byte, {pending} packets, {a.value} look-ups, {b.value} steps added")


def main():
    rng = np.random.default_rng(1)
    plain = framed_plain(rng)
    measure("framed", 0, plain, FM.model_block_frames(plain, lfsr_state=0)[0], 1, 0, (1, 0, 0, 0))
    measure("list", 0, plain, M.model_block(plain, 0, 0, lfsr_state=0), 0, 0, (1, 0, 0, 0))
    plain = packets_plain(rng)
    measure("packets", 1, plain, PM.model_block_packets(plain, 2, lfsr_state=0, crc=True, disable_rs=False, min_dist=0)[0], 0, 1, (1, 0, 0, 2))
    measure("il2p list", 1, plain, M.model_block(plain, 1, 2, lfsr_state=0), 0, 0, (1, 0, 0, 2))
    noise = rng.integers(0, 256, N, dtype=np.uint8)
    measure("framed/noise", 0, noise, FM.model_block_frames(noise, lfsr_state=0)[0], 1, 0, (1, 0, 0, 0))
    measure("list/noise", 0, noise, M.model_block(noise, 0, 0, lfsr_state=0), 0, 0, (1, 0, 0, 0))
    measure("packets/noise", 1, noise, PM.model_block_packets(noise, 2, lfsr_state=0, crc=True, disable_rs=False, min_dist=0)[0], 0, 1, (1, 0, 0, 2))
    measure("il2p list/noise", 1, noise, M.model_block(noise, 1, 2, lfsr_state=0), 0, 0, (1, 0, 0, 2))


if __name__ == "__main__":
    main()
