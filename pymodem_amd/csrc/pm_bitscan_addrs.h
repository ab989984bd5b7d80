// The address checkpoints behind a scanned stream (pm_scan_job.addrs, pm_rows_scan_chain.addrs): A[w], an int64 per 64 data bytes, is the
// stream address of data byte 64 w.  Here: the table's size, what a lane and a tile of the row form add up from the 16-bit address steps
// (pm_bitscan.hip: the tile launch sums, the combine launch carries an int64 prefix from tile to tile, the checkpoint launch scans the
// lanes), and the host's look-up that resolves one address from the nearest checkpoint and at most 63 steps (pm_codec.cpp).  Free of
// loads from device memory, LDS and launches, so that the same text runs on the host: tests/addrs_core_check.cpp steps the row form lane
// by lane and tile by tile against a plain prefix sum.
//   address of byte k = first + steps[1] + ... + steps[k]          (steps[0], "the first one 0", is never added)
//   A[w]              = address of byte 64 w
// A piece of a row (pm_rows_scan_pieces) counts from the address in front of it, its step 0 included: piece_lane_sum, piece_lane_first.
// A lane's sum fits 32 bits (8 x 65535), a tile's does at 256 words (2048 x 65535 < 2^28); a stream's does not.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define PM_AD_HD __host__ __device__ inline
#else
#define PM_AD_HD inline
#endif

namespace pm_addrs {

constexpr int kStride = 64;                                 // PM_SCAN_ADDR_STRIDE
constexpr int64_t kMaxGap = (int64_t)kStride * 65535;       // the most that 64 steps of 16 bits add

PM_AD_HD int64_t table_places(int64_t n) { return (n + kStride - 1) / kStride; }
PM_AD_HD int64_t table_bytes(int64_t n) { return 8 * table_places(n); }                 // PM_SCAN_ADDR_BYTES

// ---- the row form: the lane of data word w holds steps 8 w .. 8 w + 7 as two little-endian words (lo: the first four) -------------------
PM_AD_HD uint32_t step_of(uint64_t lo, uint64_t hi, int i) { return (uint32_t)(((i < 4 ? lo : hi) >> (16 * (i & 3))) & 0xFFFFu); }
// the lane's steps that belong to a stream of n bytes, step 0 left out
PM_AD_HD uint32_t lane_sum(uint64_t lo, uint64_t hi, int64_t w, int64_t n)
{
    uint32_t s = 0;
    for (int i = 0; i < 8; ++i) {
        const int64_t k = 8 * w + i;
        if (k >= 1 && k < n) s += step_of(lo, hi, i);
    }
    return s;
}
// the step that leads to the lane's own first byte
PM_AD_HD uint32_t lane_first(uint64_t lo, int64_t w) { return w ? (uint32_t)(lo & 0xFFFFu) : 0u; }
PM_AD_HD bool owns_checkpoint(int64_t w) { return (w & 7) == 0; }                       // data word w begins with byte 64 (w / 8)
// A[w / 8] from the row's first address, the sums of the tiles in front (the combine launch's carry), the sums of the tile's lanes in front
// (the in-tile scan) and the lane's own first step
PM_AD_HD int64_t checkpoint(int64_t first, int64_t tiles_before, uint32_t lanes_before, uint32_t own_first)
{
    return first + tiles_before + (int64_t)lanes_before + (int64_t)own_first;
}

// ---- a PIECE of a row (pm_rows_scan_pieces): the address in front of the piece is that of the byte before it, so the piece's step 0 counts:
//   address of the piece's byte k = addr_before + steps[0] + ... + steps[k],   A[w] = address of its byte 64 w
// (checkpoint() above with addr_before for `first`, these sums and this first step)
PM_AD_HD uint32_t piece_lane_sum(uint64_t lo, uint64_t hi, int64_t w, int64_t n)
{
    uint32_t s = 0;
    for (int i = 0; i < 8; ++i)
        if (8 * w + i < n) s += step_of(lo, hi, i);
    return s;
}
PM_AD_HD uint32_t piece_lane_first(uint64_t lo) { return (uint32_t)(lo & 0xFFFFu); }

// the address of byte k from the checkpoint in front of it and at most 63 of the stream's steps (A and steps aligned: device memory, or a
// host copy that is)
PM_AD_HD int64_t resolve(const int64_t *A, const uint16_t *steps, int64_t k)
{
    int64_t a = A[k >> 6];
    for (int64_t i = (k & ~(int64_t)63) + 1; i <= k; ++i) a += steps[i];
    return a;
}

// ---- the host's side --------------------------------------------------------------------------------------------------------------------
// One stream's table and steps; [k]: the address of byte k.  Counts what it did (pm_codec_addr_work).
struct Lookup {
    const uint8_t *table;                                   // the checkpoints (8-byte places, read bytewise: a block may lie anywhere)
    const uint16_t *steps;
    int64_t lookups, nsteps;
    int64_t operator[](int64_t k)
    {
        int64_t a;
        memcpy(&a, table + 8 * (k >> 6), 8);
        for (int64_t i = (k & ~(int64_t)63) + 1; i <= k; ++i) a += steps[i];
        ++lookups;
        nsteps += k & 63;
        return a;
    }
};
// what the decoders take in a pointer's place: by value, as a pointer is
struct Ref {
    Lookup *to;
    int64_t operator[](int64_t k) const { return (*to)[k]; }
};
// can the table belong to a stream of n bytes that begins at `first`: A[0] the first address, ascending, no gap above 64 steps' worth
inline bool table_fits(const uint8_t *table, int64_t n, int64_t first)
{
    int64_t before = first;
    for (int64_t w = 0; w < table_places(n); ++w) {
        int64_t a;
        memcpy(&a, table + 8 * w, 8);
        if (w == 0 ? a != first : (a < before || (uint64_t)a - (uint64_t)before > (uint64_t)kMaxGap)) return false;
        before = a;
    }
    return true;
}

}  // namespace pm_addrs
