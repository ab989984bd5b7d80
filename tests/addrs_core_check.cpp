// Steps the row form's address checkpoints on the host through csrc/pm_bitscan_addrs.h -- the tile launch's lane sums and tile sum, the
// combine launch's int64 carry from tile to tile (a plain variable here), the checkpoint launch's scan over a tile's 256 lanes (a loop, every
// lane reads before any lane writes, as the kernel's block_scan does it) and its stores -- for every tile size from 1 to 256, and compares
// the table with a plain prefix sum over the steps; then the host's look-up (pm_addrs::Lookup) at every byte of the stream, and what
// pm_addrs::table_fits lets pass and refuses.  The steps of a row are padded to eight with values that must never be added.
//   addrs_core_check            (no arguments: the inputs are made here)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pm_bitscan_addrs.h"

using namespace pm_addrs;

namespace {

constexpr int kLanes = 256;
long mismatches = 0, places_checked = 0, lookups_checked = 0;

void fail(const char *what, long long n, int tw, long long at, long long got, long long want)
{
    if (++mismatches <= 10) printf("n %lld tile words %d: %s at %lld: %lld, want %lld\n", n, tw, what, at, got, want);
}

uint64_t word_of(const std::vector<uint16_t> &steps, int64_t i)     // the four steps from step 4 i on, little-endian, as the lanes load them
{
    uint64_t v = 0;
    memcpy(&v, steps.data() + 4 * i, 8);
    return v;
}

void check_stream(const std::vector<uint16_t> &own, int64_t first)
{
    const int64_t n = (int64_t)own.size(), nw = (n + 7) / 8;
    // the plain prefix sum: the address of every byte
    std::vector<int64_t> addr((size_t)n);
    int64_t a = first;
    for (int64_t k = 0; k < n; ++k) addr[(size_t)k] = (a += k ? own[(size_t)k] : 0);
    // the row as it lies in device memory: room for whole words, what is past the stream (and step 0) set to what must not be added
    std::vector<uint16_t> steps((size_t)(8 * nw + 8), 0xABCD);
    for (int64_t k = 1; k < n; ++k) steps[(size_t)k] = own[(size_t)k];
    if (n) steps[0] = 0x1234;                               // (the slicer writes 0 there; the arithmetic must not depend on it)
    const int64_t places = table_places(n);
    for (int tw = 1; tw <= kLanes; ++tw) {
        const int64_t tiles = (nw + tw - 1) / tw;
        // the tile launch: each lane's sum, the tile's sum in 32 bits (an LDS atomic of int32 in the kernel)
        std::vector<uint32_t> tile_sum((size_t)tiles, 0);
        for (int64_t t = 0; t < tiles; ++t) {
            uint64_t sum = 0;
            for (int l = 0; l < tw; ++l) {
                const int64_t w = t * tw + l;
                if (w >= nw) break;
                const uint32_t s = lane_sum(word_of(steps, 2 * w), word_of(steps, 2 * w + 1), w, n);
                if (s > 8u * 65535u) fail("a lane's sum passes 8 x 65535", n, tw, w, s, 8 * 65535);
                sum += s;
            }
            if (sum > 0x7FFFFFFFull) fail("a tile's sum passes 31 bits", n, tw, t, (long long)sum, 0x7FFFFFFF);
            tile_sum[(size_t)t] = (uint32_t)sum;
        }
        // the combine launch: the carry
        std::vector<int64_t> before((size_t)tiles, 0);
        int64_t carry = 0;
        for (int64_t t = 0; t < tiles; ++t) {
            before[(size_t)t] = carry;
            carry += (int64_t)tile_sum[(size_t)t];
        }
        // the checkpoint launch
        std::vector<int64_t> table((size_t)places, INT64_MIN);
        std::vector<int> written((size_t)places, 0);
        for (int64_t t = 0; t < tiles; ++t) {
            uint32_t lds[kLanes], v[kLanes];
            uint64_t lo[kLanes];
            for (int l = 0; l < kLanes; ++l) {
                const int64_t w = t * tw + l;
                const bool active = l < tw && w < nw;
                lo[l] = active ? word_of(steps, 2 * w) : 0;
                lds[l] = v[l] = active ? lane_sum(lo[l], word_of(steps, 2 * w + 1), w, n) : 0u;
            }
            for (int d = 1; d < kLanes; d <<= 1) {
                uint32_t o[kLanes];
                for (int l = d; l < kLanes; ++l) o[l] = lds[l - d];
                for (int l = d; l < kLanes; ++l) lds[l] = v[l] = o[l] + v[l];
            }
            for (int l = 0; l < kLanes; ++l) {
                const int64_t w = t * tw + l;
                if (!(l < tw && w < nw) || !owns_checkpoint(w)) continue;
                const int64_t at = w >> 3;
                if (at < 0 || at >= places) {
                    fail("a store past the table", n, tw, at, at, places - 1);
                    continue;
                }
                table[(size_t)at] = checkpoint(first, before[(size_t)t], l ? lds[l - 1] : 0u, lane_first(lo[l], w));
                ++written[(size_t)at];
            }
        }
        for (int64_t p = 0; p < places; ++p, ++places_checked) {
            if (written[(size_t)p] != 1) fail("stores to a place", n, tw, p, written[(size_t)p], 1);
            if (table[(size_t)p] != addr[(size_t)(64 * p)]) fail("checkpoint", n, tw, p, table[(size_t)p], addr[(size_t)(64 * p)]);
        }
    }
    // the host's look-up at every byte, from the prefix sum's own table
    std::vector<int64_t> table((size_t)places);
    for (int64_t p = 0; p < places; ++p) table[(size_t)p] = addr[(size_t)(64 * p)];
    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(table.data());
    Lookup look{bytes, steps.data(), 0, 0};
    const Ref ref{&look};
    int64_t want_steps = 0;
    for (int64_t k = 0; k < n; ++k, ++lookups_checked) {
        const int64_t got = ref[k];
        if (got != addr[(size_t)k]) fail("look-up", n, 0, k, got, addr[(size_t)k]);
        want_steps += k & 63;
    }
    if (look.lookups != n || look.nsteps != want_steps || look.nsteps > 63 * look.lookups) fail("look-up work", n, 0, 0, look.nsteps, want_steps);
    // what the host accepts and refuses
    if (!table_fits(bytes, n, first)) fail("the table's own stream is refused", n, 0, 0, 0, 1);
    if (places) {
        if (table_fits(bytes, n, first + 1) || table_fits(bytes, n, first - 1)) fail("another first address passes", n, 0, 0, 1, 0);
    }
    if (places >= 2) {
        std::vector<int64_t> bad = table;
        bad[1] = bad[0] - 1;
        if (table_fits(reinterpret_cast<const uint8_t *>(bad.data()), n, first)) fail("a descending pair passes", n, 0, 1, 1, 0);
        bad[1] = bad[0] + kMaxGap + 1;
        if (table_fits(reinterpret_cast<const uint8_t *>(bad.data()), n, first)) fail("a gap above 64 x 65535 passes", n, 0, 1, 1, 0);
        bad = table;
        bad[1] = bad[0] + kMaxGap;                          // (what lies behind place 1 may now descend: only the first two are given)
        if (!table_fits(reinterpret_cast<const uint8_t *>(bad.data()), 128, first)) fail("a gap of exactly 64 x 65535 is refused", n, 0, 1, 0, 1);
    }
}

}  // namespace

int main()
{
    const int64_t sizes[] = {0, 1, 63, 64, 65, 127, 128, 2047, 2048, 2049, 70000};
    const int64_t first = ((int64_t)1 << 40) + 3;
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto next = [&rng]() {
        rng ^= rng << 13;
        rng ^= rng >> 7;
        rng ^= rng << 17;
        return rng;
    };
    int streams = 0;
    for (int64_t n : sizes) {
        std::vector<uint16_t> s((size_t)n);
        for (auto &v : s) v = (uint16_t)(next() >> 20);     // random steps
        check_stream(s, first);
        for (auto &v : s) v = 65535;                        // the most a stream can add: 65 537 steps reach 2^32 - 1, the next one passes 32 bits
        check_stream(s, first);
        check_stream(s, -first);
        streams += 3;
    }
    {
        std::vector<uint16_t> s(70000, 65535);
        int64_t a = 0;
        int64_t k = 0;
        while (a <= 0xFFFFFFFFll) a += s[(size_t)++k];
        if (k != 65538) fail("the 32-bit carry's place", 70000, 0, 0, k, 65538);
    }
    printf("%d streams, %ld places, %ld look-ups, %ld mismatches\n", streams, places_checked, lookups_checked, mismatches);
    return mismatches ? 1 : 0;
}
