// Where things lie in pm_rows_scan's block and scratch (pm_bitscan.hip): a row's part size from its chain's kind, `frames`, `packets` and
// its byte count, the four running sums over the rows -- block offset, first tile, first place in the device-side event copy, first place
// in the candidate, record and work lists -- the entry of the device-side row table that the prepare launch makes from them, and the search
// for a tile's row.  Free of loads, LDS and launches, so that the same text runs on the host: the prepare kernel, the launcher and
// tests/rows_scan_core_check.cpp (which steps the prepare launch's trips of 256 rows against a plain prefix sum) all go by it.
// At the end: the same for rows taken in PIECES (pm_rows_scan_pieces) -- how a piece is cut, its part's size, its own table entry
// (tests/rows_pieces_core_check.cpp).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PM_ROWS_HD __host__ __device__ inline
#else
#define PM_ROWS_HD inline
#endif

namespace pm_rows {

constexpr int kMaxRows = 4096;              // rows of a call, as for pm_rows_gather
constexpr int kMaxChains = 64;
constexpr int kTrip = 256;                  // rows per trip of the prepare launch: a lane a row
constexpr int64_t kMaxBytes = (int64_t)1 << 29;     // bytes of a stream, as for pm_stream_scan
constexpr int kHead = 32;                   // PM_SCAN_HEAD

PM_ROWS_HD int64_t pad8(int64_t v) { return (v + 7) & ~(int64_t)7; }
// the n bytes of a row whose record counts `count` (beyond cap they are counted, not stored)
PM_ROWS_HD int64_t row_bytes(int64_t count, int64_t cap) { return count < 0 ? 0 : count < cap ? count : cap; }
PM_ROWS_HD int64_t steps_bytes(int64_t n) { return pad8(2 * n); }           // the address steps in front, uint16, as pm_rows_gather pads them
PM_ROWS_HD int64_t list_bytes(int kind, int64_t n) { return kind == 0 ? 8 * (n / 19 + 2) : kind == 1 ? 8 * ((n + 63) / 64) : 0; }      // PM_SCAN_LIST_BYTES
PM_ROWS_HD int64_t row_events(int frames, int64_t n) { return frames ? n / 19 + 2 : 0; }       // places in the device-side copy of the event list
PM_ROWS_HD int64_t row_places(int packets, int64_t n) { return packets ? n / 64 + 2 : 0; }     // places in the candidate, record and work lists
PM_ROWS_HD int64_t addr_bytes(int addrs, int64_t n) { return addrs ? 8 * ((n + 63) / 64) : 0; }     // PM_SCAN_ADDR_BYTES: the checkpoints, last in the part
// what pm_stream_scan writes for a job of these bytes: record, list, descrambled bytes, with frames or packets the table and the area,
// with addrs the address checkpoints behind all of them (scan_bytes(.., 0) is where they begin)
PM_ROWS_HD int64_t scan_bytes(int kind, int frames, int packets, int64_t n, int addrs = 0)
{
    int64_t b = kHead + list_bytes(kind, n) + pad8(n);
    if (frames) b += 8 * (n / 19 + 2) + pad8(n);            // PM_SCAN_FRAME_TABLE_BYTES, PM_SCAN_FRAME_AREA_BYTES
    if (packets) b += 16 + 16 * (n / 64 + 2) + pad8(n);     // PM_SCAN_PACKET_TABLE_BYTES, PM_SCAN_PACKET_AREA_BYTES
    return b + addr_bytes(addrs, n);
}
PM_ROWS_HD int64_t part_bytes(int kind, int frames, int packets, int64_t n, int addrs = 0)
{
    return steps_bytes(n) + scan_bytes(kind, frames, packets, n, addrs);
}
PM_ROWS_HD int64_t row_tiles(int64_t n, int tile_words) { return ((n + 7) / 8 + tile_words - 1) / tile_words; }

// The four running sums.  As a row's own: what it adds; as a prefix: where it begins; over all rows: the limits the call was sized for.
struct Sums {
    int64_t off, tiles, events, places;
};
PM_ROWS_HD Sums sums_zero() { return Sums{0, 0, 0, 0}; }
PM_ROWS_HD Sums sums_add(const Sums &a, const Sums &b) { return Sums{a.off + b.off, a.tiles + b.tiles, a.events + b.events, a.places + b.places}; }
PM_ROWS_HD Sums row_sums(int kind, int frames, int packets, int64_t n, int tile_words, int addrs = 0)
{
    return Sums{part_bytes(kind, frames, packets, n, addrs), row_tiles(n, tile_words), row_events(frames, n), row_places(packets, n)};
}

// A row of the device-side table.  Entry `nrows` holds the totals: its tile0 ends the last row's tiles.
struct Entry {
    int64_t off;                            // the row's part in the block (its steps; the scan part lies steps_bytes(n) behind), -1: the row is left out
    int64_t ev0;                            // first place in the device-side event copy, -1: no frames
    int64_t pk0;                            // first place in the candidate, record and work lists, -1: no packets
    int32_t n;                              // bytes
    int32_t tile0;                          // first tile of the row among the call's
};
// `before`: the sums over the rows in front; `limit`: what the host sized block and scratch for from its own copy of the counts.  A row
// that would pass any of them -- the records and the host's counts disagree -- is left out: no launch stores anything for it.
PM_ROWS_HD Entry row_entry(const Sums &before, int kind, int frames, int packets, int64_t n, int tile_words, const Sums &limit, int addrs = 0)
{
    const Sums end = sums_add(before, row_sums(kind, frames, packets, n < kMaxBytes ? n : kMaxBytes, tile_words, addrs));
    const bool ok = n <= kMaxBytes && end.off <= limit.off && end.tiles <= limit.tiles && end.events <= limit.events && end.places <= limit.places;
    return Entry{ok ? before.off : -1, frames ? before.events : -1, packets ? before.places : -1, (int32_t)(n < kMaxBytes ? n : kMaxBytes),
                 (int32_t)(before.tiles < limit.tiles ? before.tiles : limit.tiles)};
}
PM_ROWS_HD Entry total_entry(const Sums &all, const Sums &limit)
{
    return Entry{all.off, -1, -1, 0, (int32_t)(all.tiles < limit.tiles ? all.tiles : limit.tiles)};
}

// The row of a tile: the last of rows 0 .. nrows - 1 whose first tile is not behind it (row 0 if there is none) -- what the linear walk
// `j = 0; while (j + 1 < nrows && tile0[j + 1] <= tile) ++j;` of the job form ends at.  Rows of zero bytes have zero tiles, their tile0 equals
// the next row's, and both pass over them.  tile0(i): first tile of row i, ascending.
template <class Tile0>
PM_ROWS_HD int row_of_tile(Tile0 tile0, int nrows, int tile)
{
    int lo = 0, hi = nrows - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tile0(mid) <= tile) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// ---- rows in PIECES (pm_rows_scan_pieces) -------------------------------------------------------------------------------------------------
// A row is taken piece by piece: `taken` bytes have gone (pm_rows_carry.taken), the next piece begins there.  All but the final cut are
// multiples of 8, so that every piece's bytes and steps stay 8-byte aligned in their row (cap is a multiple of 8); a row whose `taken` is no
// multiple of 8 has had its final piece and gives empty pieces from then on.
constexpr int kPieceTail = 40;              // PM_ROWS_PIECE_TAIL_BYTES: the job form's carry piece (32) and int64 addr_before, last in the part

// what the row holds for this piece: the caller's `upto`, if it gave one, within the record's count and the row's room
PM_ROWS_HD int64_t piece_avail(int64_t count, int64_t cap, bool has_upto, int64_t upto)
{
    const int64_t room = row_bytes(count, cap);
    return has_upto && upto < room ? upto : room;
}
// the piece's bytes
PM_ROWS_HD int64_t piece_bytes(int64_t avail, int64_t taken, bool final)
{
    if (taken & 7) return 0;                // the final piece has gone
    int64_t n = avail - taken;
    if (!final) n &= ~(int64_t)7;           // (rounds down, below zero too)
    return n < 0 ? 0 : n;
}
PM_ROWS_HD int64_t piece_part_bytes(int kind, int frames, int packets, int64_t n, int addrs = 0) { return part_bytes(kind, frames, packets, n, addrs) + kPieceTail; }
PM_ROWS_HD Sums piece_sums(int kind, int frames, int packets, int64_t n, int tile_words, int addrs = 0)
{
    return Sums{piece_part_bytes(kind, frames, packets, n, addrs), row_tiles(n, tile_words), row_events(frames, n), row_places(packets, n)};
}
// A piece's row of the device-side table: Entry's fields, where in its row the piece begins, and the address in front of its first step.
struct PieceEntry {
    int64_t off, ev0, pk0;
    int32_t n, tile0;
    int64_t from;                           // bytes of the row in front of the piece: its bytes lie at row * cap + from, its steps likewise
    int64_t addr_before;                    // the stream address of byte from - 1 (the row's first address while from == 0, where the first step is 0)
};
PM_ROWS_HD PieceEntry piece_entry(const Sums &before, int kind, int frames, int packets, int64_t n, int tile_words, const Sums &limit, int addrs, int64_t from,
                                  int64_t addr_before)
{
    const Sums end = sums_add(before, piece_sums(kind, frames, packets, n < kMaxBytes ? n : kMaxBytes, tile_words, addrs));
    const bool ok = n <= kMaxBytes && end.off <= limit.off && end.tiles <= limit.tiles && end.events <= limit.events && end.places <= limit.places;
    return PieceEntry{ok ? before.off : -1, frames ? before.events : -1, packets ? before.places : -1, (int32_t)(n < kMaxBytes ? n : kMaxBytes),
                      (int32_t)(before.tiles < limit.tiles ? before.tiles : limit.tiles), from, addr_before};
}
PM_ROWS_HD PieceEntry piece_total_entry(const Sums &all, const Sums &limit)
{
    return PieceEntry{all.off, -1, -1, 0, (int32_t)(all.tiles < limit.tiles ? all.tiles : limit.tiles), 0, 0};
}

}  // namespace pm_rows
