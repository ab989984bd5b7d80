"""A stream scanned in pieces (pm_scan_job.d_carry), restated bit by bit from the definitions in include/pymodem_amd.h: for a stream of
slicer bytes and its cut points, per piece, the part that pm_stream_scan writes -- record, list, descrambled bytes, frame table with its
"not made" entry and frame area, or packet table and area, address checkpoints, carry piece -- and the carry in front of and behind it.
The AX.25 lists come from one register walk over the piece's bits that starts from the carry's `ones` and `counted` and tracks both; nothing
is taken from the kernels, the shared headers or the host skim.  (The LFSR is pm_lfsr_unscramble, the host's, which test_host_codecs.py holds
to the reference; an IL2P piece depends on nothing in front of it, so its lists are il2p_packets_model's for the piece's bytes alone.)"""
import ctypes

import numpy as np

import bitscan_model as M
import frames_model as FM
from pymodem_amd._native import (SCAN_CARRY_BYTES, SCAN_CARRY_LOST, SCAN_CARRY_OK, SCAN_CARRY_START, check, lib, scan_addr_bytes, scan_carry_piece_dtype,
                                 scan_frame_area_bytes, scan_frame_table_bytes, scan_list_bytes, scan_record_dtype)

BAIL = 8000
NOT_MADE = (-1, 0)


def carry_start(reg=0):
    return dict(lfsr_state=reg, tail=0, counted=0, pieces=0, bytes=0, ones=0, state=SCAN_CARRY_START)


def carry_seeded(reg, ones, counted):
    """pm_scan_carry_set"""
    ones = min(ones, 7)
    tail = (0xFF << 56) if ones >= 7 else (((1 << ones) - 1) << (64 - ones)) if ones else 0
    state = SCAN_CARRY_LOST if counted < 0 else SCAN_CARRY_START if (ones, counted) == (0, 0) else SCAN_CARRY_OK
    return dict(lfsr_state=reg, tail=tail, counted=counted, pieces=0, bytes=0, ones=ones, state=state)


def host_lfsr(raw, poly, reg, invert):
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    plain = np.zeros(max(len(raw), 1), dtype=np.uint8)
    sr = ctypes.c_uint64(reg)
    check(lib().pm_lfsr_unscramble(raw.ctypes.data, len(raw), poly, int(invert), ctypes.byref(sr), plain.ctypes.data))
    return plain[:len(raw)], sr.value


def ax25_walk(bits, cin):
    """The decoder's pattern registers over one piece, from the carry: ([(P, F)], bail_bit, last_flag, ones_out, counted_out, state_out).
    `raw` are the bits since the last reset, `dropped` the stuffed zeros among them; a piece starts `counted` bits behind a reset (LOST:
    8000, so that its first reset is the bail).  Listed: the piece's first flag and every flag at counted bit T with T & 7 == 7, T >= 151.
    counted_out goes on behind a bail: what was counted behind the piece's last reset, 0 inside a run of seven ones or more."""
    state = cin["state"]
    ones = cin["ones"]
    raw = BAIL if state == SCAN_CARRY_LOST else cin["counted"] if state == SCAN_CARRY_OK else 0
    dropped, counted = 0, cin["counted"]
    events, bail, last_flag, first = [], -1, -1, True
    for P, bit in enumerate(bits):
        if bit:
            ones = min(ones + 1, 7)
            raw += 1
            counted = 0 if ones >= 7 else counted + 1
            continue
        if ones == 5:
            dropped += 1
            raw += 1
        elif ones >= 6:
            if bail < 0:
                if raw >= BAIL:
                    bail = P
                elif ones == 6:
                    T = raw - dropped
                    if first or (T & 7 == 7 and T >= 8 * 18 + 7):
                        events.append((P, last_flag))
                    first = False
                    last_flag = P + 1
            raw, dropped, counted = 0, 0, 0
        else:
            raw += 1
            counted += 1
        ones = 0
    return events, bail, last_flag, ones, counted, (SCAN_CARRY_LOST if bail >= 0 or state == SCAN_CARRY_LOST else SCAN_CARRY_OK)


def carry_piece(cin):
    p = np.zeros(1, dtype=scan_carry_piece_dtype())
    for f in ("state", "ones", "counted", "pieces", "bytes"):
        p[f] = cin[f]
    return p.view(np.uint8).ravel()


def model_piece(raw, cin, poly, invert, kind, tol=0, frames=False, packets=None, addr=None):
    """One piece: (the part as pm_stream_scan writes it, mask of its bytes that are written, the carry behind it, the descrambled bytes).
    packets: None, or dict(crc, disable_rs, min_dist); addr: None, or the piece's n stream addresses (checkpoints behind the rest)."""
    plain, reg = host_lfsr(raw, poly, cin["lfsr_state"], invert)
    n = len(plain)
    bits = np.unpackbits(plain).tolist()
    out = dict(cin, lfsr_state=reg, pieces=cin["pieces"] + 1, bytes=cin["bytes"] + n, state=SCAN_CARRY_OK if cin["state"] != SCAN_CARRY_LOST else SCAN_CARRY_LOST)
    joined = [(cin["tail"] >> i) & 1 for i in range(64)] + bits
    out["tail"] = sum(b << i for i, b in enumerate(joined[-64:]))
    run = 0
    for b in reversed(joined[-64:]):
        if not b:
            break
        run += 1
    out["ones"] = min(run, 7)
    if kind == 0:
        events, bail, last_flag, ones, counted, state = ax25_walk(bits, cin)
        assert ones == out["ones"], "the walk's ones counter and the tail agree"
        out["counted"], out["state"] = counted, state
        rec = np.zeros(1, dtype=scan_record_dtype())
        rec["lfsr_state"], rec["bail_bit"], rec["last_flag"], rec["events"] = reg, bail, last_flag, len(events)
        lst = np.zeros(scan_list_bytes(0, n), dtype=np.uint8)
        assert len(events) <= n // 19 + 2
        lst[:8 * len(events)] = np.array([[p, f & 0xFFFFFFFF] for p, f in events], dtype="<u4").reshape(-1, 2).view(np.uint8).ravel()
        body = np.zeros((n + 7) // 8 * 8, dtype=np.uint8)
        body[:n] = plain
        part = [rec.view(np.uint8).ravel(), lst, body]
        written = [np.ones(32 + 8 * len(events), dtype=bool), np.zeros(len(lst) - 8 * len(events), dtype=bool), np.ones(len(body), dtype=bool)]
        if frames:
            table = np.zeros(scan_frame_table_bytes(n) // 8, dtype=[("len", "<i4"), ("crc", "<u4")])
            area = np.zeros(scan_frame_area_bytes(n), dtype=np.uint8)
            covered = np.zeros(len(area), dtype=bool)
            for e, (P, F) in enumerate(events):
                if F < 0 and cin["state"] != SCAN_CARRY_START:
                    table[e] = NOT_MADE                    # what it closes began in an earlier piece
                    continue
                frame = FM.frame_model(bits, P, F)
                assert frame is not None or e == 0
                if frame is None:
                    continue
                at = max(F, 0) >> 3
                table[e] = (len(frame), FM.crc16(frame[:-2]))
                area[at:at + len(frame)] = np.frombuffer(frame, dtype=np.uint8)
                covered[at:at + len(frame)] = True
            part += [table.view(np.uint8), area]
            written += [np.repeat(np.arange(len(table)) < len(events), 8), covered]
    elif kind == 1:
        import il2p_packets_model as PM
        if packets is not None:
            block, mask = PM.model_block_packets(plain, tol, lfsr_state=reg, **packets)
        else:
            block = M.model_block(plain, 1, tol, reg)
            mask = np.ones(len(block), dtype=bool)
        part, written = [block], [mask]
    else:
        block = M.model_block(plain, -1, 0, reg)
        part, written = [block], [np.ones(len(block), dtype=bool)]
    if addr is not None:
        table = np.zeros(scan_addr_bytes(n) // 8, dtype="<i8")
        table[:] = np.asarray(addr, dtype=np.int64)[::64]
        part.append(table.view(np.uint8))
        written.append(np.ones(8 * len(table), dtype=bool))
    part.append(carry_piece(cin))
    written.append(np.ones(SCAN_CARRY_BYTES, dtype=bool))
    return np.concatenate(part), np.concatenate(written), out, plain


def model_pieces(raw, cuts, poly, invert, kind, tol=0, frames=False, packets=None, addr=None, carry=None, reseed=None):
    """The pieces raw[0:cuts[0]], raw[cuts[0]:cuts[1]], ... raw[cuts[-1]:] in order: [(part, written, carry in, carry out, plain)].
    reseed(k, carry) -> carry or None: what pm_scan_carry_set does in front of piece k (the caller's codec says with what)."""
    raw = np.asarray(raw, dtype=np.uint8)
    edges = [0] + list(cuts) + [len(raw)]
    carry = carry_start() if carry is None else carry
    out = []
    for k, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        if reseed is not None:
            carry = reseed(k, carry) or carry
        part, written, after, plain = model_piece(raw[a:b], carry, poly, invert, kind, tol, frames, packets, None if addr is None else addr[a:b])
        out.append((part, written, carry, after, plain))
        carry = after
    return out


def scramble(plain, poly=0x21001):
    """slicer bytes whose LFSR output, inverted, from register 0 is `plain` (G3RUH's polynomial: seventeen bits of history across every cut)"""
    bits = M.siggen.lfsr_scramble(np.unpackbits(np.asarray(plain, dtype=np.uint8)).tolist(), poly, True)
    return np.packbits(np.array(bits, dtype=np.uint8)) if len(bits) else np.zeros(0, np.uint8)


def walked_bound(part, n, frames):
    """Bytes that the host may take through its registers for an AX.25 piece: up to the first listed flag, and from the byte of the last
    flag's zero (a bail: of the last flag in front of it) to the end; without frames every listed frame besides, from the flag in front."""
    rec = part[:32].view(scan_record_dtype())[0]
    events = part[32:32 + 8 * int(rec["events"])].view("<u4").reshape(-1, 2)
    if n < 24:
        return n
    first = (int(events[0][0]) >> 3) + 1 if len(events) else 0
    last = int(rec["last_flag"])
    tail = n - ((last - 1) >> 3 if last > 0 else 0)
    mid = 0 if frames else sum((int(P) >> 3) + 1 - ((int(F) - 1) >> 3) for P, F in events[1:])
    return min(n, first) + tail + mid
