"""What pm_rows_packets writes, restated from the definition in include/pymodem_amd.h on top of the model blocks (bitscan_model, frames_model,
il2p_packets_model) and the oracle (header rebuild, Hamming table, CRC, PacketMeta's checks) -- not from pm_rows_packets.h or the host
decoder: the two rules that say whether a row's table tells everything about it, the packets of a finished row, the entries and the room.
A packet is (streamaddress, data bytes, BytesCorrected); test_rows_packets_model.py holds the finished rows to the oracle's decoders.
Shared by test_rows_packets_core.py and test_gpu_rows_packets.py."""
import functools

import numpy as np

import bitscan_model as M
import frames_model as FM
import il2p_packets_model as PM
from oracle import oracle as O
from pymodem_amd import _native as N

STATUS = N.ROWS_PACKETS_STATUS
FINISHED, NO_RECORD, INCOMPLETE, NOT_PLACED, LATE_HIT, TABLE_FULL, SHORT, BAIL, LONG_FRAME, LEFT_OUT, NO_ROOM, NO_CODEC = range(12)
PKT_MAX = N.PKT_MAX


def _hit(w, tol):
    return bin((w & 0xFFFFFF) ^ M.SYNC24).count("1") <= tol or bin(w ^ M.SYNC32).count("1") <= tol


def _true_hits(plain, tol):
    """per byte k >= 4 the smallest bit offset at which the test hits on the INPUT's last 32 bits, 8 where none does (from the bytes themselves)"""
    d = np.asarray(plain, dtype=np.uint8).astype(np.uint64)
    n = len(d)
    out = np.full(n, 8, dtype=np.int64)
    if n < 5:
        return out
    win = (d[0:n - 4] << np.uint64(32)) | (d[1:n - 3] << np.uint64(24)) | (d[2:n - 2] << np.uint64(16)) | (d[3:n - 1] << np.uint64(8)) | d[4:n]
    pop = M._pop16()

    def pop32(v):
        return pop[(v & np.uint64(0xFFFF)).astype(np.int64)] + pop[((v >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.int64)]
    for S in range(7, -1, -1):
        w = (win >> np.uint64(7 - S)) & np.uint64(0xFFFFFFFF)
        hit = (pop32((w & np.uint64(0xFFFFFF)) ^ np.uint64(M.SYNC24)) <= tol) | (pop32(w ^ np.uint64(M.SYNC32)) <= tol)
        out[4:][hit] = S
    return out


def il2p_row(block, plain, tol, crc):
    """The IL2P walk: (status, [(record index, E behind the CRC bytes, BytesCorrected)], corrected left over)."""
    plain = np.asarray(plain, dtype=np.uint8)
    n = len(plain)
    records, _, recs, _ = PM.split_packets(np.asarray(block), n)
    if records == n // 64 + 2:
        return TABLE_FULL, [], 0
    by_at = {int(r["at"]): (e, r) for e, r in enumerate(recs)}
    bits = PM._bits(plain)
    true_S = _true_hits(plain, tol)
    true_at = np.flatnonzero(true_S < 8)
    d = plain.tolist()
    word, corrected, k, run, out = 0xFFFFFF, 0, 0, 0, []
    while k < n:
        if run >= 4 and k >= 4:
            # four whole bytes into a search the register is the input's last 32 bits: no byte up to the next true hit can hit
            i = int(np.searchsorted(true_at, k))
            if i == len(true_at):
                break
            j = int(true_at[i])
            if j > k:
                word = d[j - 4] << 24 | d[j - 3] << 16 | d[j - 2] << 8 | d[j - 1]
                k = j
        win = word << 8 | d[k]
        run = min(4, run + 1)
        S = next((s for s in range(8) if _hit((win >> (7 - s)) & 0xFFFFFFFF, tol)), None)
        if S is None:
            word = win & 0xFFFFFFFF
            k += 1
            continue
        if (k << 3 | S) not in by_at:
            return NO_RECORD, [], 0
        e, r = by_at[k << 3 | S]
        status = int(r["status"])
        if status == PM.INCOMPLETE:
            return INCOMPLETE, [], 0
        if status == PM.NOT_PLACED:
            return NOT_PLACED, [], 0
        E = 8 * k + S + 1 + (120 if status == PM.HEADER_FAIL else int(r["end"]))
        if status != PM.HEADER_FAIL:
            corrected += int(r["corrected"])
        if status == PM.DONE:
            if crc:
                E += 32
            out.append((e, E, corrected))
            corrected = 0
        ke = (E - 1) >> 3
        word = PM._take(bits, E - 8, 1)[0]
        for b in range(E, 8 * (ke + 1)):
            word = (word << 1 | bits[b]) & 0xFFFFFFFF
            if _hit(word, tol):
                return LATE_HIT, [], 0
        run, k = 0, ke + 1
    return FINISHED, out, corrected


def il2p_packet(block, plain, addr, crc, e, E, corrected):
    """the packet of record e: the AX.25 header that the oracle rebuilds from its 13 bytes, the payload from the area, the CRC bytes"""
    n = len(plain)
    _, _, recs, area = PM.split_packets(np.asarray(block), n)
    off, count = int(recs[e]["off"]), int(recs[e]["count"])
    c = O.IL2PCodec(PM.IDENT, crc)
    c.buf[:13] = [int(v) for v in area[off:off + 13]]
    c._ax25_header(c._header())
    data = list(c.pkt.data) + [int(v) for v in area[off + 13:off + 13 + count]]
    if crc:
        v = sum(O.HAMMING_74[b & 0x7F] << (12 - 4 * i) for i, b in enumerate(PM._take(PM._bits(plain), E - 32, 4)))
    else:
        v = O.crc16(data)
    return int(addr[(E - 1) >> 3]), bytes(bytearray(data + [v & 0xFF, v >> 8])), corrected


def ax25_row(block, plain):
    """The AX.25 rule: (status, [(event, P, F, len, crc)])."""
    n = len(plain)
    if n < 24:
        return SHORT, []
    rec, lst, _ = M.split_block(np.asarray(block), 0, n)
    if int(rec["bail_bit"]) >= 0:
        return BAIL, []
    table, _ = FM.split_frames(np.asarray(block), n)
    pf = lst.view("<u4").reshape(-1, 2)
    return FINISHED, [(e, int(pf[e][0]), int(pf[e][1]), int(t["len"]), int(t["crc"])) for e, t in enumerate(table) if int(t["len"]) > 0]


def ax25_packet(block, plain, addr, P, F, length, crc):
    _, area = FM.split_frames(np.asarray(block), len(plain))
    at = 0 if F == 0xFFFFFFFF else F >> 3
    return int(addr[P >> 3]), bytes(bytearray(area[at:at + length].tolist())), 0, crc


def row_packets(kind, block, plain, addr, tol=0, crc=True):
    """(status, [(streamaddress, data, BytesCorrected, calculated CRC or None)], corrected left over) of a row"""
    if kind == 1:
        status, acc, left = il2p_row(block, plain, tol, crc)
        return status, [il2p_packet(block, plain, addr, crc, *a) + (None,) for a in acc], left
    if kind == 0:
        status, acc = ax25_row(block, plain)
        return status, [ax25_packet(block, plain, addr, *a[1:]) for a in acc], 0
    return NO_CODEC, [], 0


def packet_row(packet, source):
    """the pm_packet row of a packet: PacketMeta's checks by the oracle (the AX.25 frame's calculated CRC is the table's: the same number)"""
    addr, data, corrected, crc = packet
    p = O.Packet()
    p.data = list(data)
    p.check()
    assert crc is None or crc == p.CalculatedCRC
    row = np.zeros(1, dtype=N.packet_dtype())
    data = data[:PKT_MAX]                                    # a frame longer than a row: its first bytes, the whole frame's CRCs
    row["streamaddress"], row["len"], row["bytes_corrected"] = addr, len(data), corrected
    row["calculated_crc"], row["carried_crc"], row["valid_crc"], row["valid_header"] = p.CalculatedCRC, p.CarriedCRC, int(p.ValidCRC), int(p.ValidHeader)
    row["source_decoder"] = source
    row["data"][0, :len(data)] = np.frombuffer(data, dtype=np.uint8)
    return row


def model_call(rows, capacity):
    """rows: [dict(kind, block, plain, addr, tol, crc, source, register, left_out)] in row order; capacity: packet rows d_out has room for.
    -> (head, entries, packet rows) as pm_rows_packets leaves them."""
    entries = np.zeros(len(rows), dtype=N.rows_packets_entry_dtype())
    out, total, full = [], 0, False
    for r, row in enumerate(rows):
        if row.get("left_out"):
            status, pkts, left, register = LEFT_OUT, [], 0, 0
        else:
            status, pkts, left = row_packets(row["kind"], row["block"], row["plain"], row["addr"], row.get("tol", 0), row.get("crc", True))
            register = row.get("register", 0)
        full = full or total + len(pkts) > capacity
        if full:
            status, pkts, left = NO_ROOM, [], 0
        elif status != FINISHED:
            pkts, left = [], 0
        entries[r] = (register, status, len(pkts), total, left, 0)
        out += [packet_row(p, row.get("source", 0)) for p in pkts]
        total += len(pkts)
    head = np.zeros(1, dtype=N.rows_packets_head_dtype())
    head["rows"], head["handed"], head["packets"] = len(rows), int((entries["status"] != FINISHED).sum()), total
    return head, entries, np.concatenate(out) if out else np.zeros(0, dtype=N.packet_dtype())


@functools.lru_cache(maxsize=None)
def stream_walk(name):
    """(status, packets, corrected left over) of il2p_packets_model's stream `name` at addresses 0, 1, 2, ...: made once"""
    plain, tol, o = PM.all_streams()[name]
    block, _ = PM.block_of(name)
    return row_packets(1, block, plain, np.arange(len(plain)), tol, o["crc"])


# ---- the 600 rows of test_gpu_rows_scan._rows(): chains AX.25 with frames, IL2P with packets, descramble only ---------------------------------
def row_addresses(row, n):
    """the addresses of a row's bytes under test_gpu_rows_scan._device_rows' steps: first_addr 0, step i of row r = (7 r + 3 i) & 0xFFFF"""
    steps = (7 * row + 3 * np.arange(n, dtype=np.int64)) & 0xFFFF
    if n:
        steps[0] = 0
    return np.cumsum(steps)


@functools.lru_cache(maxsize=None)
def scan_rows_walks():
    """per row of test_gpu_rows_scan._rows(): (status, packets, corrected left over), made once"""
    import test_gpu_rows_scan as RS
    _, _, models, plains = RS._rows()
    return [row_packets((0, 1, -1)[row % 3], models[row][0], plains[row], row_addresses(row, len(plains[row])), RS.TOL, RS.OPTS["crc"]) for row in range(RS.ROWS)]


@functools.lru_cache(maxsize=None)
def scan_rows_call(row0, nrows, capacity, sources=(0, 1, 2), left_out=()):
    """(head, entries, packet rows) of pm_rows_packets for rows [row0, row0 + nrows) of them; the entries' registers are left 0.
    left_out: rows that the scan left out"""
    walks = list(scan_rows_walks())
    for row in left_out:
        walks[row] = (LEFT_OUT, [], 0)
    entries = np.zeros(nrows, dtype=N.rows_packets_entry_dtype())
    out, total, full = [], 0, False
    for r in range(nrows):
        status, pkts, left = walks[row0 + r]
        full = full or total + len(pkts) > capacity
        if full:
            status, pkts, left = NO_ROOM, [], 0
        elif status != FINISHED:
            pkts, left = [], 0
        entries[r] = (0, status, len(pkts), total, left, 0)
        out += [packet_row(p, sources[(row0 + r) % 3]) for p in pkts]
        total += len(pkts)
    head = np.zeros(1, dtype=N.rows_packets_head_dtype())
    head["rows"], head["handed"], head["packets"] = nrows, int((entries["status"] != FINISHED).sum()), total
    return head, entries, np.concatenate(out) if out else np.zeros(0, dtype=N.packet_dtype())


def part_of_row(block, plain, addr, steps):
    """a row's part of a pm_rows_scan block made with addrs: the steps, the scan part (the model block), the checkpoints"""
    n = len(plain)
    front = np.zeros(N.rows_scan_steps_bytes(n), dtype=np.uint8)
    front[:2 * n] = np.asarray(steps[:n], dtype="<u2").view(np.uint8)
    table = np.asarray(addr, dtype="<i8")[::64].copy().view(np.uint8)
    return np.concatenate([front, np.asarray(block), table])
