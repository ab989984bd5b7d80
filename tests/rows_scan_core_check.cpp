// Steps pm_rows_scan's prepare launch on the host through csrc/pm_bitscan_rows.h -- trips of 256 rows, a lane a row, the lanes' scan as
// the kernel's block_scan does it, the carry from trip to trip -- and compares every row's entry and the totals with the table that
// tests/test_rows_scan_core.py made by a plain prefix sum; then, for every tile index of the batch, the binary search with the linear walk
// of the job form's job_of_tile.
//   rows_scan_core_check <cases.bin>
// cases.bin: int32 cases; per case int32 nrows, nchains, tile_words, short_by; nchains x {int32 kind, frames, packets}; nrows x int64 count;
// int64 cap; nrows x {int64 off, ev0, pk0, int32 n, tile0}; {int64 used, int32 tiles}.  short_by: the limits' block is that many bytes
// short of the need (0: everything fits).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pm_bitscan_rows.h"

using namespace pm_rows;

namespace {

template <class T>
bool get(FILE *f, T *v, size_t n = 1) { return fread(v, sizeof(T), n, f) == n; }

struct Chain {
    int32_t kind, frames, packets;
};
struct Want {
    int64_t off, ev0, pk0;
    int32_t n, tile0;
};

// the literal walk of the job form (pm_bitscan.hip: ScanJobs::job_of_tile)
int walk(const std::vector<Entry> &t, int nrows, int tile)
{
    int j = 0;
    while (j + 1 < nrows && t[(size_t)j + 1].tile0 <= tile) ++j;
    return j;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t cases = 0;
    if (!get(f, &cases)) return 2;
    long mismatches = 0, tiles_checked = 0;
    for (int32_t cs = 0; cs < cases; ++cs) {
        int32_t head[4];
        if (!get(f, head, 4)) return 2;
        const int nrows = head[0], nchains = head[1], tw = head[2], short_by = head[3];
        std::vector<Chain> chains((size_t)nchains);
        std::vector<int64_t> counts((size_t)nrows);
        int64_t cap = 0;
        if (!get(f, chains.data(), chains.size()) || !get(f, counts.data(), counts.size()) || !get(f, &cap)) return 2;
        std::vector<Want> want((size_t)nrows);
        for (auto &w : want)
            if (!get(f, &w.off) || !get(f, &w.ev0) || !get(f, &w.pk0) || !get(f, &w.n) || !get(f, &w.tile0)) return 2;
        int64_t want_used = 0;
        int32_t want_tiles = 0;
        if (!get(f, &want_used) || !get(f, &want_tiles)) return 2;

        // the launcher's sums over its own copy of the counts: the limits
        Sums limit = sums_zero();
        for (int r = 0; r < nrows; ++r) {
            const Chain &c = chains[(size_t)(r % nchains)];
            limit = sums_add(limit, row_sums(c.kind, c.frames, c.packets, row_bytes(counts[(size_t)r], cap), tw));
        }
        limit.off -= short_by;

        // the prepare launch: one workgroup, trips of kTrip rows
        std::vector<Entry> table((size_t)nrows + 1);
        Sums carry = sums_zero();
        for (int r0 = 0; r0 < nrows; r0 += kTrip) {
            Sums lds[kTrip], v[kTrip];
            int64_t n[kTrip];
            for (int t = 0; t < kTrip; ++t) {
                const int r = r0 + t;
                const Chain &c = chains[(size_t)(r % nchains)];
                n[t] = r < nrows ? row_bytes(counts[(size_t)r], cap) : 0;
                v[t] = r < nrows ? row_sums(c.kind, c.frames, c.packets, n[t] < kMaxBytes ? n[t] : kMaxBytes, tw) : sums_zero();
                lds[t] = v[t];
            }
            for (int d = 1; d < kTrip; d <<= 1) {           // block_scan: every lane reads before any lane writes
                Sums o[kTrip];
                for (int t = d; t < kTrip; ++t) o[t] = lds[t - d];
                for (int t = d; t < kTrip; ++t) lds[t] = v[t] = sums_add(o[t], v[t]);
            }
            for (int t = 0; t < kTrip && r0 + t < nrows; ++t) {
                const Chain &c = chains[(size_t)((r0 + t) % nchains)];
                const Sums before = sums_add(carry, t ? lds[t - 1] : sums_zero());
                table[(size_t)(r0 + t)] = row_entry(before, c.kind, c.frames, c.packets, n[t], tw, limit);
            }
            carry = sums_add(carry, lds[kTrip - 1]);
        }
        table[(size_t)nrows] = total_entry(carry, limit);

        for (int r = 0; r < nrows; ++r) {
            const Entry &e = table[(size_t)r];
            const Want &w = want[(size_t)r];
            if (e.off != w.off || e.ev0 != w.ev0 || e.pk0 != w.pk0 || e.n != w.n || e.tile0 != w.tile0) {
                if (++mismatches <= 10)
                    printf("case %d row %d: {%lld %lld %lld %d %d}, the prefix sum says {%lld %lld %lld %d %d}\n", cs, r, (long long)e.off, (long long)e.ev0,
                           (long long)e.pk0, e.n, e.tile0, (long long)w.off, (long long)w.ev0, (long long)w.pk0, w.n, w.tile0);
            }
        }
        if (table[(size_t)nrows].off != want_used || table[(size_t)nrows].tile0 != want_tiles) {
            if (++mismatches <= 10) printf("case %d: totals {%lld %d}, want {%lld %d}\n", cs, (long long)table[(size_t)nrows].off, table[(size_t)nrows].tile0, (long long)want_used, want_tiles);
        }

        // every tile: the search against the walk.  The walk is literal where the batch is small enough and at every 89th tile elsewhere;
        // in between it goes on from the tile before (the first tiles ascend, so it ends where the literal one does).
        const int total = table[(size_t)nrows].tile0;
        const bool literal = (double)total * nrows < 3e7;
        const Entry *t = table.data();
        int j = 0;
        for (int tile = 0; tile < total; ++tile, ++tiles_checked) {
            while (j + 1 < nrows && table[(size_t)j + 1].tile0 <= tile) ++j;
            const int found = row_of_tile([t](int i) { return t[i].tile0; }, nrows, tile);
            if (found != j || ((literal || tile % 89 == 0) && found != walk(table, nrows, tile))) {
                if (++mismatches <= 10) printf("case %d tile %d: the search says row %d, the walk %d\n", cs, tile, found, j);
            }
            // the row really holds the tile
            if (!(table[(size_t)found].tile0 <= tile && tile < table[(size_t)found + 1].tile0)) {
                if (++mismatches <= 10) printf("case %d tile %d: row %d holds tiles %d .. %d\n", cs, tile, found, table[(size_t)found].tile0, table[(size_t)found + 1].tile0);
            }
        }
        // a tile at or past the total: the kernels leave, but the search must stay inside the table
        for (int tile = total; tile < total + 3; ++tile) {
            const int found = row_of_tile([t](int i) { return t[i].tile0; }, nrows, tile);
            if (found != walk(table, nrows, tile) || found < 0 || found >= nrows) ++mismatches;
        }
    }
    fclose(f);
    printf("%d cases, %ld tiles, %ld mismatches\n", cases, tiles_checked, mismatches);
    return mismatches ? 1 : 0;
}
