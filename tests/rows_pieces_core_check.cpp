// Steps the piece arithmetic of pm_rows_scan_pieces on the host through csrc/pm_bitscan_rows.h and pm_bitscan_addrs.h.
// 1. The prepare launch -- trips of 256 rows, a lane a row, the lanes' scan as the kernel's block_scan does it, the carry from trip to trip --
//    with every row's piece cut from its record's count, `upto` and `taken`: every entry (off, ev0, pk0, n, tile0, from) and the totals
//    against the table that tests/test_rows_pieces_core.py made by a plain loop over the rows.
// 2. The step sums with the piece's step 0: per tile the lanes' sums (the tile launch), the int64 prefix from tile to tile (the combine
//    launch), the scan over a tile's lanes and the checkpoints (the checkpoint launch), and the piece's total that moves last_addr on,
//    against a plain prefix sum made there.
//   rows_pieces_core_check <cases.bin>
// cases.bin: int32 cases; per case int32 nrows, nchains, tile_words, short_by, final, has_upto; nchains x {int32 kind, frames, packets, addrs};
// int64 cap; nrows x {int64 count, upto, taken, host_n}; nrows x {int64 off, ev0, pk0, from, int32 n, tile0}; {int64 used, int32 tiles}.
// host_n: the piece length as the host has it, which sizes the limits (short_by: the block is that many bytes short besides).
// Then int32 sums; per item int32 tile_words, int64 n, int64 addr_before, pad8(n) x uint16 steps (those past n are not the piece's),
// (n + 63) / 64 x int64 checkpoints, int64 total.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pm_bitscan_addrs.h"
#include "pm_bitscan_rows.h"

using namespace pm_rows;

namespace {

template <class T>
bool get(FILE *f, T *v, size_t n = 1) { return n == 0 || fread(v, sizeof(T), n, f) == n; }

struct Chain {
    int32_t kind, frames, packets, addrs;
};
struct Row {
    int64_t count, upto, taken, host_n;
};
struct Want {
    int64_t off, ev0, pk0, from;
    int32_t n, tile0;
};

long mismatches = 0;

void prepare_case(FILE *f, int cs)
{
    int32_t head[6];
    if (!get(f, head, 6)) exit(2);
    const int nrows = head[0], nchains = head[1], tw = head[2], short_by = head[3];
    const bool final_piece = head[4] != 0, has_upto = head[5] != 0;
    std::vector<Chain> chains((size_t)nchains);
    std::vector<Row> rows((size_t)nrows);
    int64_t cap = 0;
    if (!get(f, chains.data(), chains.size()) || !get(f, &cap) || !get(f, rows.data(), rows.size())) exit(2);
    std::vector<Want> want((size_t)nrows);
    for (auto &w : want)
        if (!get(f, &w.off) || !get(f, &w.ev0) || !get(f, &w.pk0) || !get(f, &w.from) || !get(f, &w.n) || !get(f, &w.tile0)) exit(2);
    int64_t want_used = 0;
    int32_t want_tiles = 0;
    if (!get(f, &want_used) || !get(f, &want_tiles)) exit(2);

    // the launcher's sums over the host's piece lengths: the limits
    Sums limit = sums_zero();
    for (int r = 0; r < nrows; ++r) {
        const Chain &c = chains[(size_t)(r % nchains)];
        limit = sums_add(limit, piece_sums(c.kind, c.frames, c.packets, rows[(size_t)r].host_n, tw, c.addrs));
    }
    limit.off -= short_by;

    // the prepare launch: one workgroup, trips of kTrip rows
    std::vector<PieceEntry> table((size_t)nrows + 1);
    Sums carry = sums_zero();
    for (int r0 = 0; r0 < nrows; r0 += kTrip) {
        Sums lds[kTrip], v[kTrip];
        int64_t n[kTrip], from[kTrip];
        for (int t = 0; t < kTrip; ++t) {
            const int r = r0 + t;
            const Chain &c = chains[(size_t)(r % nchains)];
            n[t] = from[t] = 0;
            if (r < nrows) {
                const Row &q = rows[(size_t)r];
                from[t] = q.taken;
                n[t] = piece_bytes(piece_avail(q.count, cap, has_upto, has_upto ? q.upto : 0), from[t], final_piece);
            }
            v[t] = r < nrows ? piece_sums(c.kind, c.frames, c.packets, n[t] < kMaxBytes ? n[t] : kMaxBytes, tw, c.addrs) : sums_zero();
            lds[t] = v[t];
        }
        for (int d = 1; d < kTrip; d <<= 1) {               // block_scan: every lane reads before any lane writes
            Sums o[kTrip];
            for (int t = d; t < kTrip; ++t) o[t] = lds[t - d];
            for (int t = d; t < kTrip; ++t) lds[t] = v[t] = sums_add(o[t], v[t]);
        }
        for (int t = 0; t < kTrip && r0 + t < nrows; ++t) {
            const Chain &c = chains[(size_t)((r0 + t) % nchains)];
            const Sums before = sums_add(carry, t ? lds[t - 1] : sums_zero());
            table[(size_t)(r0 + t)] = piece_entry(before, c.kind, c.frames, c.packets, n[t], tw, limit, c.addrs, from[t], 1000 + r0 + t);
        }
        carry = sums_add(carry, lds[kTrip - 1]);
    }
    table[(size_t)nrows] = piece_total_entry(carry, limit);

    for (int r = 0; r < nrows; ++r) {
        const PieceEntry &e = table[(size_t)r];
        const Want &w = want[(size_t)r];
        if (e.off != w.off || e.ev0 != w.ev0 || e.pk0 != w.pk0 || e.n != w.n || e.tile0 != w.tile0 || e.from != w.from || e.addr_before != 1000 + r) {
            if (++mismatches <= 10)
                printf("case %d row %d: {%lld %lld %lld %d %d from %lld}, the plain loop says {%lld %lld %lld %d %d from %lld}\n", cs, r, (long long)e.off,
                       (long long)e.ev0, (long long)e.pk0, e.n, e.tile0, (long long)e.from, (long long)w.off, (long long)w.ev0, (long long)w.pk0, w.n, w.tile0,
                       (long long)w.from);
        }
        // what the kernels rely on: a piece with bytes begins at a multiple of 8 and ends inside the row
        if (e.n > 0 && ((e.from & 7) != 0 || e.from + e.n > cap || e.from < 0)) {
            if (++mismatches <= 10) printf("case %d row %d: piece %lld + %d in a row of %lld\n", cs, r, (long long)e.from, e.n, (long long)cap);
        }
    }
    if (table[(size_t)nrows].off != want_used || table[(size_t)nrows].tile0 != want_tiles) {
        if (++mismatches <= 10)
            printf("case %d: totals {%lld %d}, want {%lld %d}\n", cs, (long long)table[(size_t)nrows].off, table[(size_t)nrows].tile0, (long long)want_used, want_tiles);
    }
    // every tile's row, with the search the kernels use
    const PieceEntry *t = table.data();
    const int total = table[(size_t)nrows].tile0;
    int j = 0;
    for (int tile = 0; tile < total; ++tile) {
        while (j + 1 < nrows && table[(size_t)j + 1].tile0 <= tile) ++j;
        if (row_of_tile([t](int i) { return t[i].tile0; }, nrows, tile) != j) {
            if (++mismatches <= 10) printf("case %d tile %d: the search and the walk disagree\n", cs, tile);
        }
    }
}

long sums_item(FILE *f, int item)
{
    int32_t tw = 0;
    int64_t n = 0, addr_before = 0, want_total = 0;
    if (!get(f, &tw) || !get(f, &n) || !get(f, &addr_before)) exit(2);
    std::vector<uint16_t> steps((size_t)pad8(n));
    std::vector<int64_t> want((size_t)pm_addrs::table_places(n));
    if (!get(f, steps.data(), steps.size()) || !get(f, want.data(), want.size()) || !get(f, &want_total)) exit(2);
    const int64_t nw = (n + 7) / 8, tiles = row_tiles(n, tw);
    auto word = [&](int64_t i) {                            // step word i of the piece, little-endian as the lanes load it
        uint64_t v = 0;
        for (int k = 0; k < 4; ++k) v |= (uint64_t)steps[(size_t)(4 * i + k)] << (16 * k);
        return v;
    };
    long checked = 0;
    int64_t steps_before = 0;                               // the combine launch's prefix
    for (int64_t tile = 0; tile < tiles; ++tile) {
        uint32_t tile_sum = 0, lanes_before = 0;
        for (int lane = 0; lane < tw; ++lane) {
            const int64_t w = tile * tw + lane;
            if (w >= nw) break;
            const uint64_t lo = word(2 * w), hi = word(2 * w + 1);
            if (pm_addrs::owns_checkpoint(w)) {
                const int64_t a = pm_addrs::checkpoint(addr_before, steps_before, lanes_before, pm_addrs::piece_lane_first(lo));
                if (a != want[(size_t)(w >> 3)]) {
                    if (++mismatches <= 10) printf("sums %d (tile %d words): A[%lld] = %lld, the prefix sum says %lld\n", item, tw, (long long)(w >> 3), (long long)a, (long long)want[(size_t)(w >> 3)]);
                }
                ++checked;
            }
            const uint32_t mine = pm_addrs::piece_lane_sum(lo, hi, w, n);
            lanes_before += mine;
            tile_sum += mine;
        }
        if ((int64_t)(int32_t)tile_sum != (int64_t)tile_sum) ++mismatches;      // the tile's sum goes through an int32 atomic
        steps_before += (int64_t)tile_sum;
    }
    if (steps_before != want_total) {
        if (++mismatches <= 10) printf("sums %d: the piece's steps add to %lld, the plain sum says %lld\n", item, (long long)steps_before, (long long)want_total);
    }
    if (checked != (long)want.size()) ++mismatches;
    return checked;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t cases = 0, items = 0;
    if (!get(f, &cases)) return 2;
    for (int32_t cs = 0; cs < cases; ++cs) prepare_case(f, cs);
    if (!get(f, &items)) return 2;
    long checkpoints = 0;
    for (int32_t i = 0; i < items; ++i) checkpoints += sums_item(f, i);
    fclose(f);
    printf("%d cases, %d step sums, %ld checkpoints, %ld mismatches\n", cases, items, checkpoints, mismatches);
    return mismatches ? 1 : 0;
}
