"""Rows scanned in pieces (pm_rows_scan_pieces), restated from the definitions in include/pymodem_amd.h: how a row is cut -- `upto`, `taken`,
the multiples of 8, the final rule -- where the pieces lie in a call's block (a plain loop over the rows), and each piece's part: the piece's
steps, the job form's part for its bytes from scan_carry_model.py (which restates pm_scan_job.d_carry's pieces), and the 40-byte tail with the
address in front of the piece.  Nothing is taken from the kernels or the shared headers."""
import numpy as np

import scan_carry_model as CM
from pymodem_amd import _native as N

TAIL = 40


def piece_bytes(count, cap, upto, taken, final):
    """n of the row's next piece (upto: None for the record's count)"""
    room = min(max(int(count), 0), cap)
    avail = room if upto is None else min(int(upto), room)
    if taken % 8:
        return 0                                              # the final piece has gone
    n = avail - taken
    if not final:
        n -= n % 8                                            # (Python's %: rounds down below zero too)
    return max(n, 0)


def plain_table(rows, chains, tile_words, cap, final, has_upto, short_by=0):
    """rows: (count, upto, taken, host_n); chains: (kind, frames, packets, addrs).  The plain loop: per row (off, ev0, pk0, from, n, tile0), then
    (used, tiles).  A row whose part would pass what host_n sized -- block (less short_by), tiles, events or places -- has off -1."""
    def sums(r, n):
        kind, frames, packets, addrs = chains[r % len(chains)]
        return (N.rows_scan_steps_bytes(n) + N.scan_part_bytes(kind, frames, packets, n, addrs) + TAIL, (-(-n // 8) + tile_words - 1) // tile_words,
                n // 19 + 2 if frames else 0, n // 64 + 2 if packets else 0)
    limit = [sum(sums(r, row[3])[i] for r, row in enumerate(rows)) for i in range(4)]
    limit[0] -= short_by
    out, at = [], [0, 0, 0, 0]
    for r, (count, upto, taken, _) in enumerate(rows):
        kind, frames, packets, addrs = chains[r % len(chains)]
        n = piece_bytes(count, cap, upto if has_upto else None, taken, final)
        end = [a + s for a, s in zip(at, sums(r, n))]
        fits = all(e <= l for e, l in zip(end, limit))
        out.append((at[0] if fits else -1, at[2] if frames else -1, at[3] if packets else -1, taken, n, min(at[1], limit[1])))
        at = end
    return out, (at[0], min(at[1], limit[1]))


def rows_carry_start(reg):
    return dict(scan=CM.carry_start(reg), taken=0, last_addr=0)


def model_row_piece(row_raw, row_steps, first_addr, carry, n, poly, invert, kind, tol=0, frames=False, packets=None, addrs=False):
    """The piece of n bytes that begins at carry['taken'] in a row (row_raw: its bytes, row_steps: its steps, at least to the next multiple of 8
    behind the piece).  -> (part, mask of its bytes that are written, the row's carry behind it, the descrambled bytes, addr_before)"""
    a = carry["taken"]
    steps = np.asarray(row_steps[a:a + n], dtype=np.uint16)
    addr_before = int(first_addr) if a == 0 else carry["last_addr"]
    addr = addr_before + np.cumsum(steps.astype(np.int64))   # the piece's first step counts
    scan, written, after, plain = CM.model_piece(np.asarray(row_raw[a:a + n], dtype=np.uint8), carry["scan"], poly, invert, kind, tol, frames, packets,
                                                 addr if addrs else None)
    words = N.rows_scan_steps_bytes(n) // 2                   # the steps go out in whole 8-byte words: the padding holds the row's next ones
    front = np.zeros(words, dtype=np.uint16)
    front[:min(words, len(row_steps) - a)] = row_steps[a:a + words]
    front_written = np.arange(words) < max(n, min(words, len(row_steps) - a))
    part = np.concatenate([front.view(np.uint8), scan, np.array([addr_before], dtype="<i8").view(np.uint8)])
    mask = np.concatenate([np.repeat(front_written, 2), written, np.ones(8, dtype=bool)])
    out = dict(scan=after, taken=a + n, last_addr=addr_before + int(steps.astype(np.int64).sum()))
    return part, mask, out, plain, addr_before


def split_piece(part, kind, frames, packets, n, addrs):
    """-> (steps, scan part with the carry piece, addr_before) of a row's part"""
    sw = N.rows_scan_steps_bytes(n)
    assert len(part) == N.rows_piece_part_bytes(kind, frames, packets, n, addrs)
    return part[:2 * n].view(np.uint16), part[sw:len(part) - 8], int(part[len(part) - 8:].view("<i8")[0])
