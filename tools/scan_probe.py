"""pm_stream_scan on its own, for a kernel trace: a slicer batch's worth of streams of fsk_9600's size (four recordings x three chains,
0.45 MB of slicer bytes each: IL2P plain and inverted, G3RUH AX.25), random bytes, `reps` calls behind each other.  --frames: the AX.25
jobs write their frames too (pm_scan_job.frames), and two thirds of their streams are frames of 60-250 bytes between single flags, as
the headline's streams are, instead of random bytes (whose frames are the few short ones that chance makes).  --packets: the IL2P jobs make
their attempts too (pm_scan_job.packets), on streams with a packet of 20-250 payload bytes every 400 bytes or so, as fsk_9600's dense
recordings have them.  --addrs: every job writes its address checkpoints too (pm_scan_job.addrs), from addresses eight symbol periods apart.
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/scan_probe.py [reps] [--frames] [--packets] [--addrs]"""
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pymodem_amd                                                    # noqa: E402
from pymodem_amd import siggen                                        # noqa: E402
from pymodem_amd._native import (SCAN_HEAD, ScanJob, check, lib, scan_addr_bytes, scan_frame_area_bytes, scan_frame_table_bytes,      # noqa: E402
                                 scan_list_bytes, scan_packet_area_bytes, scan_packet_table_bytes)


def framed_stream(rng, n, poly):
    """slicer bytes whose LFSR output is noise, then frames with a flag between them, over and over: a third and two thirds"""
    bits = []
    while len(bits) < 8 * n:
        bits += (rng.random(int(rng.integers(2000, 6000))) < 0.5).astype(np.uint8).tolist()
        for _ in range(int(rng.integers(4, 9))):
            bits += siggen.ax25_hdlc_bits([int(b) for b in rng.integers(0, 256, int(rng.integers(60, 250)))], pre_flags=1, post_flags=0)
        bits += [0, 1, 1, 1, 1, 1, 1, 0]
    return np.packbits(np.array(siggen.lfsr_scramble(bits[:8 * n], poly, True), dtype=np.uint8))


def packet_stream(rng, n, invert):
    """slicer bytes of an IL2P chain (the identity polynomial): noise with a packet about every 400 bytes, payloads of 20-250 bytes"""
    data = rng.integers(0, 256, n, dtype=np.uint8)
    at = 100
    while at + 400 < n:
        info = [int(b) for b in rng.integers(0, 256, int(rng.integers(20, 251)))]
        frame = np.packbits(np.array(siggen.il2p_frame_bits("CQ", "N0CAL", info, preamble=4), dtype=np.uint8))
        data[at:at + len(frame)] = frame
        at += len(frame) + int(rng.integers(60, 420))
    return np.bitwise_not(data) if invert else data


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    frames = "--frames" in sys.argv[1:]
    packets = "--packets" in sys.argv[1:]
    addrs = "--addrs" in sys.argv[1:]
    reps = int(args[0]) if args else 50
    ctx = pymodem_amd.Context.default()
    n = 450_000
    chains = [(0x1, 0, 1), (0x1, 1, 1), (0x63003, 1, 0)]           # (poly, invert, codec kind) of configs/fsk_9600.json
    rng = np.random.default_rng(1)
    framed = framed_stream(rng, n, 0x63003) if frames else None
    dense = {inv: packet_stream(rng, n, inv) for inv in (0, 1)} if packets else None
    bufs = [ctx.upload(framed if frames and chains[k % len(chains)][2] == 0 else dense[chains[k % len(chains)][1]] if packets and chains[k % len(chains)][2] == 1
                       else rng.integers(0, 256, n, dtype=np.uint8)) for k in range(4 * len(chains))]
    d_addr = ctx.upload(1000 + 40 * np.arange(n, dtype=np.int64)) if addrs else None
    jobs = (ScanJob * len(bufs))()
    need = 0
    for k, (q, b) in enumerate(zip(jobs, bufs)):
        poly, inv, kind = chains[k % len(chains)]
        q.d_data, q.n, q.lfsr_poly, q.lfsr_state, q.lfsr_invert, q.codec_kind, q.sync_tol = b.ptr.value, n, poly, 0, inv, kind, 2
        q.frames = int(frames and kind == 0)
        q.packets, q.il2p_crc = int(packets and kind == 1), 1
        need += SCAN_HEAD + scan_list_bytes(kind, n) + (n + 7) // 8 * 8 + (scan_frame_table_bytes(n) + scan_frame_area_bytes(n) if q.frames else 0)
        need += scan_packet_table_bytes(n) + scan_packet_area_bytes(n) if q.packets else 0
        if addrs:
            q.d_addr, q.addrs = d_addr.ptr.value, 1
            need += scan_addr_bytes(n)
    block = ctx.empty(need, np.uint8)
    offs, used = (ctypes.c_int64 * len(bufs))(), ctypes.c_size_t()
    for timed in (False, True):
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(reps if timed else 3):
            check(lib().pm_stream_scan(ctx.handle, jobs, len(bufs), block.ptr, need, offs, ctypes.byref(used)))
        ctx.sync()
        if timed:
            ms = (time.perf_counter() - t0) * 1e3 / reps
            print(f"pm_stream_scan{' with frames' if frames else ''}{' with packets' if packets else ''}{' with addrs' if addrs else ''}: {len(bufs)} streams x {n} bytes, {ms:.3f} ms per call (host clock around {reps} calls and a stream wait), "
                  f"{len(bufs) * n / ms / 1e6:.1f} GB/s of slicer bytes")


if __name__ == "__main__":
    main()
