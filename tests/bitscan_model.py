"""What pm_stream_scan writes for a stream, restated in plain Python from the definitions in include/pymodem_amd.h (not from the
kernels or the host skim), and the bit-level test streams shared by test_host_scan.py and test_gpu_bitscan.py."""
import functools
import os

import numpy as np

from pymodem_amd import siggen
from pymodem_amd._native import SCAN_HEAD, scan_list_bytes, scan_record_dtype

SYNC24, SYNC32 = 0xF15E48, 0x5D57DF7F


def ax25_model(plain):
    """Bit by bit over the descrambled stream: ([(P, F), ...], bail_bit, last_flag).  A zero behind exactly five ones is dropped, one
    behind exactly six is a flag, one behind more ends a run: flags and run ends are resets.  Listed: the first flag, and every flag
    whose zero is counted bit T since the last reset (dropped zeros left out) with T & 7 == 7 and T >= 8 * 18 + 7."""
    ones, reset, dropped, last_flag, first = 0, 0, 0, -1, True
    events, bail = [], -1
    for P, bit in enumerate(np.unpackbits(np.asarray(plain, dtype=np.uint8)).tolist()):
        if bit:
            ones += 1
            continue
        if ones == 5:
            dropped += 1
        elif ones >= 6:
            if P - reset >= 8000:
                bail = P
                break
            if ones == 6:
                T = P - reset - dropped
                if first or (T & 7 == 7 and T >= 8 * 18 + 7):
                    events.append((P, last_flag))
                first = False
                last_flag = P + 1
            reset, dropped = P + 1, 0
        ones = 0
    return events, bail, last_flag


@functools.lru_cache(maxsize=None)
def _pop16():
    return np.array([bin(v).count("1") for v in range(65536)], dtype=np.int64)


def il2p_model(plain, tol):
    """One flag per byte k: some bit offset S of byte k has, in the 32 bits that end there, 24 bits within tol of the sync word or
    32 bits within tol of 0x5D57DF7F (il2p.py:367-376).  Bytes 0..3 have no flag."""
    d = np.asarray(plain, dtype=np.uint8).astype(np.uint64)
    n = len(d)
    hit = np.zeros(n, dtype=bool)
    if n < 5:
        return hit
    win = (d[0:n - 4] << np.uint64(32)) | (d[1:n - 3] << np.uint64(24)) | (d[2:n - 2] << np.uint64(16)) | (d[3:n - 1] << np.uint64(8)) | d[4:n]
    pop = _pop16()

    def popcount32(v):
        return pop[(v & np.uint64(0xFFFF)).astype(np.int64)] + pop[((v >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.int64)]
    for S in range(8):
        w = (win >> np.uint64(7 - S)) & np.uint64(0xFFFFFFFF)
        hit[4:] |= (popcount32((w & np.uint64(0xFFFFFF)) ^ np.uint64(SYNC24)) <= tol) | (popcount32(w ^ np.uint64(SYNC32)) <= tol)
    return hit


def model_block(plain, kind, tol=0, lfsr_state=0):
    """The job's part of a pm_stream_scan block in the documented layout: record, list, descrambled bytes (padded to 8)."""
    plain = np.asarray(plain, dtype=np.uint8)
    n = len(plain)
    rec = np.zeros(1, dtype=scan_record_dtype())
    rec["lfsr_state"], rec["bail_bit"], rec["last_flag"] = lfsr_state, -1, -1
    lst = np.zeros(scan_list_bytes(kind, n), dtype=np.uint8)
    if kind == 0:
        events, bail, last_flag = ax25_model(plain)
        assert len(events) <= n // 19 + 2
        rec["bail_bit"], rec["last_flag"], rec["events"] = bail, last_flag, len(events)
        pf = np.array([[p, f & 0xFFFFFFFF] for p, f in events], dtype="<u4").reshape(-1, 2)
        lst[:8 * len(events)] = pf.view(np.uint8).ravel()
    elif kind == 1:
        hit = il2p_model(plain, tol)
        rec["candidates"] = int(hit.sum())
        bits = np.zeros(len(lst) * 8, dtype=np.uint8)
        bits[:n] = hit
        lst[:] = np.packbits(bits, bitorder="little")
    body = np.zeros((n + 7) // 8 * 8, dtype=np.uint8)
    body[:n] = plain
    return np.concatenate([rec.view(np.uint8).ravel(), lst, body])


def split_block(block, kind, n):
    """(record, list as the model writes it -- unwritten places zeroed --, descrambled bytes) of a job's part of a block."""
    rec = block[:SCAN_HEAD].view(scan_record_dtype())[0]
    lb = scan_list_bytes(kind, n)
    lst = block[SCAN_HEAD:SCAN_HEAD + lb].copy()
    if kind == 0:
        lst[8 * max(0, int(rec["events"])):] = 0
    return rec, lst, block[SCAN_HEAD + lb:SCAN_HEAD + lb + n]


# ---- streams, built at bit level ------------------------------------------------------------------------------------------------
FLAG = [0, 1, 1, 1, 1, 1, 1, 0]


def _pack(bits):
    bits = list(bits)
    return np.packbits(np.array(bits + [0] * (-len(bits) % 8), dtype=np.uint8))


def _rand_bits(rng, n, p_one=0.5):
    return (rng.random(n) < p_one).astype(np.uint8).tolist()


def _frame(nbytes, seed=0):
    """AX.25 frame of nbytes including its two CRC bytes."""
    body = siggen.ax25_ui_frame("CQ", "N0CAL", [int(b) for b in np.random.default_rng(seed).integers(32, 127, max(0, nbytes - 18))])
    return body[:nbytes - 2]


@functools.lru_cache(maxsize=None)
def ax25_streams():
    """name -> descrambled bytes"""
    out = {}
    for seed in (1, 2, 3):
        out[f"random{seed}"] = np.random.default_rng(seed).integers(0, 256, 65536, dtype=np.uint8)
    out["dense"] = _pack(_rand_bits(np.random.default_rng(8), 8 * 65536, 0.8))
    for o in range(8):
        rng = np.random.default_rng(100 + o)
        bits = _rand_bits(rng, 64 + o) + siggen.ax25_hdlc_bits(_frame(18, o)) + _rand_bits(rng, 80) + siggen.ax25_hdlc_bits(_frame(17, o), pre_flags=3)
        out[f"len18_17_at{o}"] = _pack(bits + _rand_bits(rng, 300) + siggen.ax25_hdlc_bits(_frame(40, o)) + _rand_bits(rng, 99))
    shared = ([0] + [1] * 6) * 9 + [0]
    body = siggen.ax25_hdlc_bits(_frame(30, 5), pre_flags=0, post_flags=0)
    out["shared_zero"] = _pack([1, 0, 1] + shared + body + shared + body + FLAG + _rand_bits(np.random.default_rng(7), 333))
    half = body[:len(body) // 2]
    out["abort_then_flag"] = _pack([0, 0, 1] + [1] * 9 + [0] + FLAG + body + FLAG + half + [1] * 8 + [0] + FLAG * 2 + body + FLAG + [1] * 40 + [0] + body + FLAG * 3
                                   + [0] * 5)
    big = siggen.ax25_hdlc_bits([int(b) for b in np.random.default_rng(11).integers(0, 256, 1098)], pre_flags=6)
    out["frame1100"] = _pack(_rand_bits(np.random.default_rng(12), 777) + big + siggen.ax25_hdlc_bits(_frame(25, 1)) + _rand_bits(np.random.default_rng(13), 4001))
    calm = np.random.default_rng(14).choice(np.array([0x55, 0xAA, 0x33, 0x66, 0x5A, 0x24], dtype=np.uint8), 1200)      # no run of six ones
    tail = _pack(siggen.ax25_hdlc_bits(_frame(33, 2)) + _rand_bits(np.random.default_rng(15), 2000))
    out["bail_at_once"] = np.concatenate([calm, tail])
    out["bail_after_a_flag"] = np.concatenate([_pack(FLAG * 2 + body + FLAG), calm, tail])
    short = _pack([1, 1, 0] + FLAG * 2 + siggen.ax25_hdlc_bits(_frame(19, 3), pre_flags=1))
    for n in (0, 1, 23, 24, 25):
        out[f"short{n}"] = short[:n].copy()
    out.update(edge_streams())
    return out


# ---- streams for what the tiles, the bail and the stream's end decide -------------------------------------------------------------
CALM = np.array([0x55, 0xAA, 0x33, 0x66, 0x5A, 0x24], dtype=np.uint8)      # no run of four ones in any sequence of them
TILE_BITS = 8 * 2048                                                        # the default tile: 256 words
SPANS = (7999, 8000, 8001)                                                  # raw bits from a reset to the next flag's zero: the bail is at 8000
STRADDLE_OFFSETS = (-16, -8) + tuple(range(-7, 8)) + (8, 16)                # bits from a multiple of TILE_BITS


def _calm_bits(seed, nbits):
    """nbits bits that hold no run of four ones, the last one a zero"""
    bits = np.unpackbits(np.random.default_rng(seed).choice(CALM, nbits // 8 + 1)).tolist()[:nbits]
    if bits:
        bits[-1] = 0
    return bits


def _span_bits(S, stuffed, seed):
    """S bits without a reset that end in six ones: behind a reset and in front of a zero, that zero is a flag's, S raw bits behind
    the reset.  stuffed: 21 zeros behind five ones among them, so that the counted bits are 21 fewer than the raw ones."""
    fill = []
    if stuffed:
        for k in range(21):
            fill += _calm_bits(seed + k, 80) + [0, 1, 1, 1, 1, 1, 0]
    fill += _calm_bits(seed + 99, S - 6 - len(fill))
    return fill + [1] * 6


def _first_stuffed(bits):
    """index of the first zero behind five ones"""
    ones = 0
    for k, b in enumerate(bits):
        if not b and ones == 5:
            return k
        ones = ones + 1 if b else 0
    raise AssertionError("no stuffed zero")


def _straddle(piece, at, seed):
    """`piece` once per offset d of STRADDLE_OFFSETS, its bit `at` at bit k TILE_BITS + d of the stream for the k-th of them, random bits
    (a flag every 128 bits or so: no bail) in between"""
    rng = np.random.default_rng(seed)
    bits = []
    for k, d in enumerate(STRADDLE_OFFSETS):
        start = (k + 1) * TILE_BITS + d - at
        bits += _rand_bits(rng, start - 1 - len(bits)) + [0] + piece
    return bits + _rand_bits(rng, 2400)


def straddle_marks():
    """the bits of a straddle_* stream at which its piece.s marked bit lies, one per offset"""
    return [(k + 1) * TILE_BITS + d for k, d in enumerate(STRADDLE_OFFSETS)]


@functools.lru_cache(maxsize=None)
def edge_streams():
    """name -> descrambled bytes"""
    out = {}
    body = siggen.ax25_hdlc_bits(_frame(30, 5), pre_flags=0, post_flags=0)
    # the bail's boundary: a span of S raw bits from the stream's start or from a flag, calm or with stuffed zeros in it, and a whole
    # frame behind the flag that ends it -- listed for 7999, behind the bail for 8000 and 8001
    for S in SPANS:
        for start, lead in (("start", []), ("flag", [1, 0, 1] + FLAG * 2)):
            for kind in ("calm", "stuffed"):
                bits = lead + _span_bits(S, kind == "stuffed", 600 + S) + [0] + siggen.ax25_hdlc_bits(_frame(20, S & 15), pre_flags=1, post_flags=2)
                out[f"span{S}_{start}_{kind}"] = _pack(bits + _rand_bits(np.random.default_rng(S), 64))
    # a bail late in a long stream: frames, a span from 8 bytes short of the second default tile to 14 bytes into the third, frames
    rng = np.random.default_rng(41)
    bits = _rand_bits(rng, 500) + [0] + siggen.ax25_hdlc_bits(_frame(40, 6), pre_flags=2, post_flags=1) + _rand_bits(rng, 3000) + [0]
    bits += siggen.ax25_hdlc_bits(_frame(25, 7), pre_flags=1, post_flags=1)
    bits += _rand_bits(rng, TILE_BITS - 64 - 9 - len(bits)) + [0] + FLAG + _calm_bits(42, TILE_BITS + 8 * 14 + 64 - 8) + [1] * 6 + [0]
    bits += siggen.ax25_hdlc_bits(_frame(33, 2), pre_flags=1, post_flags=2) + _rand_bits(rng, 9000) + [0] + siggen.ax25_hdlc_bits(_frame(22, 3), pre_flags=2)
    out["late_bail"] = _pack(bits + _rand_bits(rng, 3 * TILE_BITS + 2000 - len(bits)))
    # what lies across the default tiles' boundaries, at every bit offset and a few whole bytes to either side of each
    shared = ([0] + [1] * 6) * 9 + [0]
    out["straddle_flag"] = _pack(_straddle(shared + body + shared + body + FLAG, len(shared) + len(body) + 7, 50))      # the zero of the flag that closes the first frame
    stuffy = siggen.ax25_hdlc_bits(siggen.ax25_ui_frame("CQ", "N0CAL", [0x7F, 0xFF, 0x41, 0xFF, 0x1F] + list(range(48, 60))), pre_flags=1, post_flags=1)
    out["straddle_stuffed"] = _pack(_straddle(stuffy, 8 + _first_stuffed(stuffy[8:-8]), 51))                            # the frame's first stuffed zero
    abort = FLAG + body[:len(body) // 2] + [0] + [1] * 7 + [0]
    out["straddle_run7"] = _pack(_straddle(abort + FLAG + body + FLAG, len(abort) - 1, 52))                              # the zero behind seven ones
    f18 = siggen.ax25_hdlc_bits(_frame(18, 4), pre_flags=1, post_flags=1)
    piece = f18 + _rand_bits(np.random.default_rng(53), 80) + [0] + siggen.ax25_hdlc_bits(_frame(17, 4), pre_flags=3, post_flags=1)
    out["straddle_bit151"] = _pack(_straddle(piece, len(f18) - 2, 54))           # the 151st counted bit of the 18-byte frame: its flag's last one
    # many frames back to back, one flag between some and two between others: more events than the frames launch has waves, twice over
    bits = list(FLAG)
    for k in range(640):
        bits += siggen.ax25_hdlc_bits(_frame(19 + k % 7, 1000 + k), pre_flags=0, post_flags=1) + (FLAG if k % 3 == 0 else [])
    out["many_frames"] = _pack(bits + [0] * 5)
    # the stream's end inside a word, at every length mod 8: the padding's first bit would complete a flag, a stuffed zero, a run's end
    for r in range(8):
        n = 8 * 4 + r + 1
        head = FLAG + siggen.ax25_hdlc_bits(_frame(19, 30 + r), pre_flags=0, post_flags=1)
        for name, ones in (("five", 5), ("six", 6), ("seven", 7)):
            tail = [0] + [1] * ones
            out[f"end{r}_{name}"] = _pack(head + _calm_bits(700 + r, 8 * n - len(head) - len(tail)) + tail)
            assert len(out[f"end{r}_{name}"]) == n
    return out


@functools.lru_cache(maxsize=None)
def ax25_block(name):
    """model_block of the AX.25 stream `name`, made once and shared: read-only"""
    block = model_block(ax25_streams()[name], 0)
    block.flags.writeable = False
    return block


def _il2p_bits(seed, flips=0, rng=None):
    bits = siggen.il2p_frame_bits("CQ", f"N0CAL{seed % 10}", [int(c) for c in np.random.default_rng(seed).integers(32, 127, 20 + seed % 30)], src_ssid=seed % 16)
    start = 16 * 8                                        # the sync word's 24 bits behind the preamble
    for k in (rng.choice(24, flips, replace=False) if flips else []):
        bits[start + int(k)] ^= 1
    return bits, start + 24


@functools.lru_cache(maxsize=None)
def il2p_streams():
    """name -> (descrambled bytes, sync_tol, {bit behind a planted sync word: flipped bits})"""
    out = {}
    for flips in range(4):
        rng = np.random.default_rng(200 + flips)
        bits, planted = _rand_bits(rng, 160), {}
        for o in range(8):                                  # frames are whole bytes: 321 bits of noise move the next one a bit on
            frame, end = _il2p_bits(10 * flips + o, flips, rng)
            planted[len(bits) + end] = flips
            bits += frame + _rand_bits(rng, 321)
        assert sorted(p % 8 for p in planted) == list(range(8))
        out[f"sync_flips{flips}"] = (_pack(bits), 2, planted)
    rng = np.random.default_rng(300)
    bits, planted = _rand_bits(rng, 200), {}
    for o in range(8):
        frame, _ = _il2p_bits(50 + o)
        frame[16 * 8 - 8:16 * 8 + 24] = [(SYNC32 >> (31 - i)) & 1 for i in range(32)]
        planted[len(bits) + 16 * 8 + 24] = 0
        bits += frame + _rand_bits(rng, 321)
    out["pattern32"] = (_pack(bits), 2, planted)
    for lead in (0, 3, 8, 13):                             # the sync word ends inside bytes 2, 3, 3 and 4
        frame, _ = _il2p_bits(70 + lead)
        rng = np.random.default_rng(400 + lead)
        out[f"sync_in_first_bytes{lead}"] = (_pack(_rand_bits(rng, lead) + frame[16 * 8:] + _rand_bits(rng, 500) + _il2p_bits(71 + lead)[0] + [0] * 64), 2, {lead + 24: 0})
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "il2p_resync.npz"))
    for tol in (0, 2):
        out[f"resync_tol{tol}"] = (g[f"tol{tol}_data"], tol, {})
    out["random"] = (np.random.default_rng(21).integers(0, 256, 65536, dtype=np.uint8), 2, {})
    for n in (0, 3, 4, 5):
        out[f"short{n}"] = (out["sync_in_first_bytes0"][0][:n].copy(), 2, {})
    return out
