"""What pm_stream_scan writes with pm_scan_job.frames, restated bit by bit from the definition in include/pymodem_amd.h (not from the
kernel or the host decoder), and the streams that test_host_frames.py and test_gpu_frames.py add to bitscan_model.ax25_streams()."""
import functools

import numpy as np

import bitscan_model as M
from pymodem_amd import siggen
from pymodem_amd._native import lib, scan_frame_area_bytes, scan_frame_table_bytes

CALM = M.CALM                                               # no run of six ones, no five ones before a zero


def frame_model(bits, P, F):
    """The frame that the flag at bit P closes in a decoder that starts cleared at bit F (bit 0 for F none), or None when it closes none.
    A zero behind exactly five ones is dropped.  The seventh one of a run and every one after it clear the bit and byte counters, the zero
    that ends such a run is not appended, the collected bytes stay.  Every other bit is appended: eight since the counters were last
    clear make a byte, first bit in bit 0."""
    ones = nbits = nbytes = byte = 0
    out = bytearray()
    for bit in bits[max(F, 0):P]:
        if bit:
            ones += 1
            if ones > 6:
                nbits = nbytes = byte = 0
                continue
        else:
            run, ones = ones, 0
            if run >= 5:                                   # five: stuffed; seven or more: the run's end (six cannot be: F is the last flag)
                assert run != 6
                continue
        byte |= bit << nbits
        nbits += 1
        if nbits == 8:
            out.append(byte)
            nbits = byte = 0
            nbytes += 1
    return bytes(out) if nbytes >= 18 and nbits == 7 else None


def crc16(data):
    """crc_functions.py:44-55 bit by bit"""
    crc = 0xFFFF
    for b in data:
        for i in range(8):
            crc = (crc >> 1) ^ 0x8408 if (crc ^ (b >> i)) & 1 else crc >> 1
    return crc ^ 0xFFFF


def frames_of(plain):
    """[(P, F, frame bytes or None)] for the events of bitscan_model.ax25_model"""
    events, _, _ = M.ax25_model(plain)
    bits = np.unpackbits(np.asarray(plain, dtype=np.uint8)).tolist()
    out = []
    for k, (P, F) in enumerate(events):
        frame = frame_model(bits, P, F)
        assert frame is not None or k == 0, "every listed flag but the stream's first closes a frame"
        out.append((P, F, frame))
    return out


def model_block_frames(plain, lfsr_state=0):
    """bitscan_model.model_block for an AX.25 job with frames: the frame table and the frame area behind the descrambled bytes.  Returns
    (block, covered): covered marks the area's bytes that a frame lies on (the others are not written)."""
    plain = np.asarray(plain, dtype=np.uint8)
    n = len(plain)
    table = np.zeros(scan_frame_table_bytes(n) // 8, dtype=[("len", "<i4"), ("crc", "<u4")])
    area = np.zeros(scan_frame_area_bytes(n), dtype=np.uint8)
    covered = np.zeros(len(area), dtype=bool)
    for e, (P, F, frame) in enumerate(frames_of(plain)):
        if frame is None:
            continue
        at = max(F, 0) >> 3
        assert at + len(frame) <= (P >> 3) + 1 and not covered[at:at + len(frame)].any()
        table[e] = (len(frame), crc16(frame[:-2]))
        area[at:at + len(frame)] = np.frombuffer(frame, dtype=np.uint8)
        covered[at:at + len(frame)] = True
    return np.concatenate([M.model_block(plain, 0, 0, lfsr_state), table.view(np.uint8), area]), covered


def split_frames(block, n):
    """(table entries [0, events) as (len, crc) pairs, frame area) of an AX.25 job's part of a block made with frames"""
    rec, _, _ = M.split_block(block, 0, n)
    at = M.SCAN_HEAD + M.scan_list_bytes(0, n) + (n + 7) // 8 * 8
    table = block[at:at + scan_frame_table_bytes(n)].view([("len", "<i4"), ("crc", "<u4")])
    return table[:max(0, int(rec["events"]))].copy(), block[at + scan_frame_table_bytes(n):at + scan_frame_table_bytes(n) + scan_frame_area_bytes(n)]


def _calm(seed, count):
    return np.unpackbits(np.random.default_rng(seed).choice(CALM, count)).tolist()


@functools.lru_cache(maxsize=None)
def frame_streams():
    """name -> descrambled bytes: what the frames add to bitscan_model.ax25_streams()"""
    out = {}
    body = siggen.ax25_hdlc_bits(M._frame(30, 5), pre_flags=0, post_flags=0)
    for o in range(8):
        # 40 bytes, three ones and a run of nine ones with its zero (the counters clear, the 40 bytes stay), then 30 bytes and the flag
        rng = np.random.default_rng(500 + o)
        out[f"survive_at{o}"] = M._pack(M._rand_bits(rng, o, 0.3) + M.FLAG + _calm(510 + o, 40) + [1, 1, 1] + [1] * 9 + [0] + body + M.FLAG)
    # a frame longer than a packet row, every segment short of the bail: 900 + 900 + 30 bytes
    out["long_no_bail"] = M._pack(M.FLAG + _calm(520, 900) + [1] * 8 + [0] + _calm(521, 900) + [1] * 7 + [0] + body + M.FLAG + M._rand_bits(np.random.default_rng(522), 100))
    out["first_closes"] = M._pack(body + M.FLAG + M._rand_bits(np.random.default_rng(523), 200))
    out["first_closes_after_run"] = M._pack([1] * 9 + [0] + body + M.FLAG + M._rand_bits(np.random.default_rng(524), 200))
    # the same with a second flag behind the first, both in one 64-bit word: the stream's first flag closes the frame begun at the run's end
    pad = next(p for p in range(64) if (p + 10 + len(body)) % 64 <= 48)
    out["two_flags_one_word"] = M._pack([1] * (9 + pad) + [0] + body + M.FLAG * 2 + M._rand_bits(np.random.default_rng(525), 200))
    return out


@functools.lru_cache(maxsize=None)
def all_streams():
    out = dict(M.ax25_streams())
    out.update(frame_streams())
    return out


def host_crc(data):
    data = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8))
    return int(lib().pm_crc16_ccitt(data.ctypes.data, len(data)))
