"""What pm_stream_scan writes with pm_scan_job.packets, restated bit by bit from the definition in include/pymodem_amd.h with the oracle's
RS, _il2p_descramble and IL2PCodec._header (not from the kernels or the host decoder): the ATTEMPT behind every candidate, the packet table
and the packet area.  consume() is a consumer that chains the records by the rules of pm_codec_decode_packets on top of the oracle's own
decoder; tests hold it to IL2PCodec.decode, and with it the model.  The streams are shared by test_host_packets.py, test_packets_core.py and
test_gpu_packets.py."""
import functools
import os

import numpy as np

import bitscan_model as M
from oracle import oracle as O
from pymodem_amd import siggen
from pymodem_amd._native import scan_packet_area_bytes, scan_packet_dtype, scan_packet_table_bytes

INCOMPLETE, HEADER_FAIL, DONE, BLOCK_FAIL, NOT_PLACED = range(5)
NONE = 0xFFFFFFFF
IDENT = 3


def _bits(plain):
    return np.unpackbits(np.asarray(plain, dtype=np.uint8)).tolist()


def _take(bits, at, nbytes):
    """nbytes bytes from bit `at` on, first bit on top"""
    return [int("".join(map(str, bits[at + 8 * q:at + 8 * q + 8])), 2) for q in range(nbytes)]


def candidates(plain, tol):
    """[(k, S)]: the bytes of the bitmap and the smallest bit offset at which the sync test hits on the 32 true bits that end there"""
    bits = _bits(plain)
    out = []
    for k in np.flatnonzero(M.il2p_model(plain, tol)).tolist():
        for S in range(8):
            end = 8 * k + S + 1
            w = int("".join(map(str, bits[end - 32:end])), 2)
            if O.IL2PCodec._dist(w & 0xFFFFFF, M.SYNC24) <= tol or O.IL2PCodec._dist(w, M.SYNC32) <= tol:
                out.append((k, S))
                break
        else:
            raise AssertionError("a bitmap bit without an offset")
    return out


def block_sizes(count):
    """il2p.py:346-358: the big blocks first"""
    if count == 0:
        return []
    q = count / 239
    blocks = int(q) + (q % 1 > 0)
    size = int(count / blocks)
    big = count - blocks * size
    return [size + 1] * big + [size] * (blocks - big)


@functools.lru_cache(maxsize=None)
def _rs(roots):
    return O.RS(0, roots)


def attempt(bits, H, crc, disable_rs, min_dist):
    """What a decoder does from bit H, where it enters its header state with `corrected` 0, until it is back in sync search:
    dict(status, count, corrected, end, header (13 bytes), payload)."""
    total = len(bits)
    none = dict(status=INCOMPLETE, count=0, corrected=0, end=0, header=None, payload=None)
    if H + 120 > total:
        return none
    buf = _take(bits, H, 15)
    r = 0 if disable_rs else _rs(2).decode(buf, 15, min_dist)
    if r < 0:
        return dict(none, status=HEADER_FAIL, end=120)
    O._il2p_descramble(buf, 13)
    codec = O.IL2PCodec()
    codec.buf = buf
    count = codec._header()["count"]
    sizes = block_sizes(count)
    end = 120 + 8 * sum(s + 16 for s in sizes)
    if H + end + (32 if crc else 0) > total:
        return none
    corrected, payload, at = r, [], H + 120
    for s in sizes:
        blk = _take(bits, at, s + 16)
        at += 8 * (s + 16)
        r = 0 if disable_rs else _rs(16).decode(blk, s + 16, min_dist)
        if r < 0:
            return dict(status=BLOCK_FAIL, count=count, corrected=corrected, end=at - H, header=buf[:13], payload=None)
        corrected += r
        O._il2p_descramble(blk, s + 16)
        payload += blk[:s]
    return dict(status=DONE, count=count, corrected=corrected, end=end, header=buf[:13], payload=payload)


def model_packets(plain, tol, crc=True, disable_rs=False, min_dist=0):
    """(records as an array of scan_packet_dtype, placed, area bytes, covered mask) of a stream"""
    plain = np.asarray(plain, dtype=np.uint8)
    n = len(plain)
    bits = _bits(plain)
    places = n // 64 + 2
    area = np.zeros(scan_packet_area_bytes(n), dtype=np.uint8)
    covered = np.zeros(len(area), dtype=bool)
    recs, used, full, placed = [], 0, False, 0
    for k, S in candidates(plain, tol)[:places]:
        at = k << 3 | S
        a = attempt(bits, 8 * k + S + 1, crc, disable_rs, min_dist)
        off = NONE
        if a["status"] in (DONE, BLOCK_FAIL):
            need = (13 + a["count"] + 7) & ~7
            if full or used + need > len(area):
                # the headers launch knows of the header alone: it passed and the attempt is complete, but there is no room
                full = True
                hdr_corrected = a["corrected"] if a["status"] == DONE and not a["payload"] else None
                if hdr_corrected is None:
                    buf = _take(bits, 8 * k + S + 1, 15)
                    hdr_corrected = 0 if disable_rs else _rs(2).decode(buf, 15, min_dist)
                a = dict(a, status=NOT_PLACED, corrected=hdr_corrected, end=120)
            else:
                off, used, placed = used, used + need, placed + 1
                if a["status"] == DONE:
                    area[off:off + 13] = a["header"]
                    area[off + 13:off + 13 + a["count"]] = a["payload"]
                    covered[off:off + need] = True
        recs.append((at, off, a["count"], a["status"], a["corrected"], a["end"]))
    return np.array(recs, dtype=scan_packet_dtype()), placed, area, covered


def model_block_packets(plain, tol, crc=True, disable_rs=False, min_dist=0, lfsr_state=0):
    """(the job's part of a block made with `packets`, mask of its bytes that are written) -- table places past `records` and area bytes that
    no DONE record covers are not."""
    plain = np.asarray(plain, dtype=np.uint8)
    n = len(plain)
    front = M.model_block(plain, 1, tol, lfsr_state)
    recs, placed, area, covered = model_packets(plain, tol, crc, disable_rs, min_dist)
    table = np.zeros(scan_packet_table_bytes(n), dtype=np.uint8)
    table[:8] = np.array([len(recs), placed], dtype="<i4").view(np.uint8)
    table[16:16 + 16 * len(recs)] = recs.view(np.uint8)
    written = np.concatenate([np.ones(len(front) + 16 + 16 * len(recs), dtype=bool), np.zeros(len(table) - 16 - 16 * len(recs), dtype=bool), covered])
    return np.concatenate([front, table, area]), written


def split_packets(block, n):
    """(records, placed, table records array, area) of a job's part of a block"""
    at = M.SCAN_HEAD + M.scan_list_bytes(1, n) + (n + 7) // 8 * 8
    records, placed = (int(v) for v in block[at:at + 8].view("<i4"))
    tb = scan_packet_table_bytes(n)
    recs = block[at + 16:at + 16 + 16 * max(0, min(records, n // 64 + 2))].view(scan_packet_dtype())
    return records, placed, recs, block[at + tb:at + tb + scan_packet_area_bytes(n)]


# ---- the consumer: pm_codec_decode_packets' rules on top of the oracle's decoder ---------------------------------------------------
def _sync_bits(c, byte, first, count):
    """`count` bits of `byte` from bit `first` (0 = the top one) through the oracle's machine by hand -- it takes whole bytes only.  Only for
    the rest of the byte in which an attempt ends: the decoder is in sync search, and a hit leaves fewer than eight bits for the header."""
    hit = False
    for i in range(first, first + count):
        bit = (byte >> (7 - i)) & 1
        mask = 0xFFFFFFFF if c.state == "sync" else 0xFF
        c.word = ((c.word << 1) & mask) | bit
        c.nbits += 1
        if c.state == "sync" and (c._dist(c.word & 0xFFFFFF, M.SYNC24) <= c.sync_tol or c._dist(c.word, M.SYNC32) <= c.sync_tol):
            c.nbits = 0
            c.state = "header"
            hit = True
    return hit


def consume(plain, addr, tol, crc=True, disable_rs=False, min_dist=0, block=None, codec=None):
    """The packets [(streamaddress, data, BytesCorrected)] of the stream with the block's records used where the rules allow, and what the
    consumer saw: dict(used: [(record index, last bit + 1)], walked, late_hits).  block None: the model's."""
    plain = np.asarray(plain, dtype=np.uint8)
    n = len(plain)
    if block is None:
        block, _ = model_block_packets(plain, tol, crc, disable_rs, min_dist)
    _, _, recs, area = split_packets(block, n)
    by_k = {int(r["at"]) >> 3: (e, r) for e, r in enumerate(recs)}
    bitmap = M.il2p_model(plain, tol)
    bits = _bits(plain)
    c = codec or O.IL2PCodec(IDENT, crc, disable_rs, min_dist, tol)
    out, used, walked, late_hits, sync_run = [], [], 0, 0, 0
    k = 0
    while k < n:
        was_sync = c.state == "sync"
        if not was_sync or sync_run < 4 or k < 4 or k + 1 >= n or bitmap[k]:
            walked += 1
        sync_run = min(4, sync_run + 1) if was_sync else 0
        out += c.decode([int(plain[k])], [int(addr[k])])
        if was_sync and c.state == "header" and k in by_k:
            S = 7 - c.nbits                                  # the header has taken the byte's bits behind the hit
            e, r = by_k[k]
            if int(r["at"]) & 7 == S and int(r["status"]) in (HEADER_FAIL, DONE, BLOCK_FAIL):
                H = 8 * k + S + 1
                E = H + (120 if r["status"] == HEADER_FAIL else int(r["end"]))
                c.state, c.nbits, c.nbuf, c.fail, c.pkt = "sync", 0, 0, False, O.Packet()
                if r["status"] != HEADER_FAIL:
                    c.corrected += int(r["corrected"])
                if r["status"] == DONE:
                    off, count = int(r["off"]), int(r["count"])
                    c.buf[:13] = [int(v) for v in area[off:off + 13]]
                    c._ax25_header(c._header())
                    c.pkt.data += [int(v) for v in area[off + 13:off + 13 + count]]
                    if crc:
                        v = sum(O.HAMMING_74[b & 0x7F] << (12 - 4 * i) for i, b in enumerate(_take(bits, E, 4)))
                        E += 32
                    else:
                        v = O.crc16(c.pkt.data)
                    c.pkt.data += [v & 0xFF, v >> 8]
                    c.pkt.streamaddress, c.pkt.SourceDecoder = int(addr[(E - 1) >> 3]), c.ident
                    c._emit(out)
                ke = (E - 1) >> 3
                used.append((e, E))
                c.word = _take(bits, E - 8, 1)[0]
                late_hits += _sync_bits(c, int(plain[ke]), E - 8 * ke, 8 * (ke + 1) - E)
                sync_run = 0
                k = ke
        k += 1
    return [(int(p.streamaddress), bytes(bytearray(p.data)), int(p.BytesCorrected)) for p in out], dict(used=used, walked=walked, late_hits=late_hits, codec=c)


def oracle_packets(plain, addr, tol, crc=True, disable_rs=False, min_dist=0):
    c = O.IL2PCodec(IDENT, crc, disable_rs, min_dist, tol)
    return [(int(p.streamaddress), bytes(bytearray(p.data)), int(p.BytesCorrected)) for p in c.decode([int(b) for b in plain], [int(a) for a in addr])]


# ---- streams ----------------------------------------------------------------------------------------------------------------------
COUNTS = (0, 1, 238, 239, 240, 478, 479, 1023)              # the block-split edges of il2p.py:346-358
SYNC_AT = 8                                                 # a frame of _frame() begins with one preamble byte: its sync word's first bit


def _frame(count, seed, crc=True):
    """the bits of a packet with `count` payload bytes: one byte of preamble, the sync word, header, blocks, CRC"""
    info = [int(b) for b in np.random.default_rng(1000 + seed).integers(0, 256, count)]
    return siggen.il2p_frame_bits("CQ", f"N0CAL{seed % 10}", info, src_ssid=seed % 16, trailing_crc=crc, preamble=1)


def _hit(frame, byte, mask=0x10):
    """flip bits of the frame's byte `byte`, counted from the header's first byte"""
    at = SYNC_AT + 24 + 8 * byte
    for i in range(8):
        if mask & (0x80 >> i):
            frame[at + i] ^= 1
    return frame


def _calm(seed, nbits):
    return np.unpackbits(np.random.default_rng(seed).choice(M.CALM, nbits // 8 + 1)).tolist()[:nbits]


def _every_offset(count, crc, seed):
    """eight packets of `count` bytes whose sync words end at the eight bit offsets of a byte"""
    bits = _calm(seed, 40)
    for o in range(8):
        bits += _frame(count, seed + o, crc) + _calm(seed + 50 + o, 41 + (0 if count > 40 else 8 * 64))      # (a place per 64 bytes: every one gets its own)
    return M._pack(bits)


@functools.lru_cache(maxsize=None)
def all_streams():
    """name -> (descrambled bytes, sync_tol, dict(crc, disable_rs, min_dist))"""
    out = {}
    std = dict(crc=True, disable_rs=False, min_dist=0)
    for count in COUNTS:
        for crc in (True, False):
            out[f"count{count}_{'crc' if crc else 'nocrc'}"] = (_every_offset(count, crc, 7 * count + crc), 0, dict(std, crc=crc))
    # sync words with 0 .. 3 wrong bits, under three tolerances
    rng = np.random.default_rng(31)
    bits = _calm(32, 64)
    for flips in range(4):
        f = _frame(20 + flips, 40 + flips)
        for i in rng.choice(24, flips, replace=False).tolist():
            f[SYNC_AT + i] ^= 1
        bits += f + _calm(33 + flips, 77)
    for tol in (0, 1, 2):
        out[f"sync_flips_tol{tol}"] = (M._pack(bits), tol, std)
    # errors in the header: none, one, two
    bits = _calm(34, 50)
    for errs in range(3):
        f = _frame(30, 50 + errs)
        for e in range(errs):
            _hit(f, 3 + 7 * e)
        bits += f + _calm(35 + errs, 99)
    out["header_errors"] = (M._pack(bits), 0, std)
    # errors in a block: eight are corrected, nine fail; the Chien search's ends; the parity bytes; the second block only, behind a header
    # with an error of its own whose correction the next packet carries
    def damaged(count, seed, where, header_err=False):
        f = _frame(count, seed)
        for w in where:
            _hit(f, 15 + w, 0x42)
        return _hit(f, 5) if header_err else f
    pieces = [damaged(100, 60, range(0, 80, 10)), damaged(100, 61, range(0, 90, 10)), damaged(100, 62, [0]), damaged(100, 63, [115]), damaged(100, 64, [99]),
              damaged(100, 65, [100, 107, 115]), damaged(300, 66, [166 + 3 * i for i in range(9)], header_err=True), damaged(40, 67, [])]
    bits = _calm(36, 45)
    for i, f in enumerate(pieces):
        bits += f + _calm(37 + i, 83)
    block_errors = M._pack(bits)
    out["block_errors"] = (block_errors, 0, std)
    for md in (1, 2):
        out[f"block_errors_min_dist{md}"] = (block_errors, 0, dict(std, min_dist=md))
    out["block_errors_disable_rs"] = (block_errors, 0, dict(std, disable_rs=True))
    bits = _calm(38, 45)
    for i, nerr in enumerate((8, 7, 6)):
        bits += damaged(60, 70 + i, range(0, 5 * nerr, 5), header_err=i == 1) + _calm(39 + i, 61)
    for md in (0, 1, 2):
        out[f"errors876_min_dist{md}"] = (M._pack(bits), 0, dict(std, min_dist=md))
    # a two-block packet cut by the stream's end inside the header, inside each block and inside the CRC bytes
    whole = M._pack(_calm(41, 37) + _frame(300, 80))
    start = (37 + SYNC_AT + 24) // 8
    for name, cut in (("header", start + 9), ("block1", start + 15 + 100), ("block2", start + 15 + 166 + 30), ("crc", len(whole) - 2), ("whole", len(whole))):
        out[f"cut_in_{name}"] = (whole[:cut].copy(), 0, std)
    # candidates in byte 4 (the first that can be one) and in the stream's last byte
    f = _frame(12, 81)[SYNC_AT:]
    for lead in (9, 16):
        out[f"first_candidate_lead{lead}"] = (M._pack(_calm(42, lead) + f + _calm(43, 90) + _frame(5, 82)[:SYNC_AT + 24]), 0, std)
    # a sync word (and a packet behind it) that begins 0 .. 4 bytes behind a packet's end, where the register still holds zeros
    for gap in range(5):
        bits = _calm(44, 43) + _frame(25, 83 + gap) + _calm(45 + gap, 8 * gap) + _frame(18, 84 + gap)[SYNC_AT:] + _calm(46, 70)
        out[f"sync_{gap}_behind_a_packet"] = (M._pack(bits), 1, std)
    # a second hit in the byte in which an attempt ends: a header that fails, its last byte 0xBC, and seven bits of 0x48 -- with nine zeros in
    # front, as the register has them there, that is the sync word but for its five ones on top, and passes at tolerance 5.  A packet's header
    # and blocks follow.  (Calm bytes around it, picked so that chance leaves the places to these.)
    for seed in range(40):
        junk = np.unpackbits(np.random.default_rng(500 + seed).choice(M.CALM, 14)).tolist()
        bits = _calm(600 + seed, 41) + _frame(0, 0)[SYNC_AT:SYNC_AT + 24] + junk + [1, 0, 1, 1, 1, 1, 0, 0] + [1, 0, 0, 1, 0, 0, 0] + _frame(9, 85)[SYNC_AT + 24:]
        plain = M._pack(bits + _calm(700 + seed, 8 * 300))
        if consume(plain, np.arange(len(plain)), 5)[1]["late_hits"]:
            break
    else:
        raise AssertionError("no late hit")
    out["late_hit"] = (plain, 5, std)
    # 130 packets back to back: three trips of the headers launch
    bits = _calm(47, 40)
    for i in range(130):
        bits += _frame(45 + i % 9, 300 + i)
    out["back_to_back"] = (M._pack(bits + [0] * 35), 0, std)
    # more candidates than places
    out["random_tol8"] = (np.random.default_rng(48).integers(0, 256, 6000, dtype=np.uint8), 8, std)
    # 40 valid headers that claim 1023 bytes, 20 bytes apart: the area runs out in the middle of the list
    data = np.random.default_rng(49).integers(0, 256, 800 + 12000, dtype=np.uint8)
    f = _frame(1023, 86)
    head = M._pack(f[SYNC_AT:SYNC_AT + 24 + 120])
    for i in range(40):
        data[6 + 20 * i:6 + 20 * i + 18] = head
    out["area_runs_out"] = (data, 0, std)
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "il2p_resync.npz"))
    for tol in (0, 2):
        out[f"resync_tol{tol}"] = (g[f"tol{tol}_data"][:20000].copy(), tol, std)
    for n in (0, 3, 4, 5):
        out[f"short{n}"] = (whole[:n].copy(), 0, std)
    return out


@functools.lru_cache(maxsize=None)
def block_of(name):
    """(model block, written mask) of the stream `name`, made once and shared: read-only"""
    plain, tol, o = all_streams()[name]
    block, written = model_block_packets(plain, tol, **o)
    block.flags.writeable = False
    return block, written
