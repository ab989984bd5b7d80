// What decides pm_stream_scan's AX.25 event list (pm_bitscan.hip): a word's marks, the segment that the tile's scan joins, the walk over a
// word's events, a tile's summary, the step that combines the summaries in stream order and the emit's walk -- free of loads, shuffles,
// LDS and atomics, so that the same text runs on the host (tests/bitscan_core_check.cpp steps the three launches lane by lane and tile
// by tile against the bit-serial model).  The kernels keep the loads, the LFSR, the scans over the lanes, the stores and the launches.
// Bits are in stream order: bit i of word w is stream bit 64 w + i.  A RESET is a flag's zero or the zero that ends a run of seven ones
// or more; what a flag closes depends on the last reset in front of it and on the stuffed zeros dropped since.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PM_EV_HD __host__ __device__ inline
#else
#define PM_EV_HD inline
#endif

namespace pm_events {

constexpr int kBailSpan = 8000;             // bits without a reset after which the host's skim gives up (pm_codec.cpp: feed_many)
constexpr int kCloseBits = 8 * 18 + 7;      // a closing flag's zero is counted bit 8 k + 7, k >= 18 (ax25.py:74-81)
constexpr int32_t kNoBail = 0x7FFFFFFF;     // TileSum.bail while the tile launch looks for the least candidate

// One tile as the tiles in front of it see it.  Positions are bits from the tile's start, -1: none.  Events at or behind `bail` (the
// first event of the tile whose span since a reset INSIDE the tile reaches kBailSpan) are left out of last_flag, first_flag and closing.
struct TileSum {
    int32_t dropped;                        // stuffed zeros in the tile
    int32_t first_reset, dropped_to_first;  // the first reset and the stuffed zeros in front of it
    int32_t last_reset, dropped_after_last;
    int32_t first_flag, last_flag;
    int32_t closing;                        // AX.25: closing flags whose reset lies inside the tile; IL2P: candidates
    int32_t bail;
    int32_t bits;                           // 1: the first reset is a flag, 2: the first flag is counted in `closing`
    int32_t steps;                          // the row form's addrs: the sum of the tile's 16-bit steps (at most 2048 x 65535), else 0
    int32_t pad;                            // (keeps the summary at 48 bytes)
};
PM_EV_HD TileSum tile_sum_empty() { return TileSum{0, -1, 0, -1, 0, -1, -1, 0, -1, 0, 0, 0}; }

// What a tile starts from, left by the combine launch for the emit launch.
struct TileCarry {
    int64_t after_reset;                    // first bit after the last reset in front of the tile (0: none yet)
    int64_t after_flag;                     // first bit after the last flag in front of it, -1: none
    int64_t bail;                           // the stream's bail bit if it lies in this tile, -1 otherwise
    int32_t dropped;                        // stuffed zeros between after_reset and the tile
    int32_t events;                         // events of the tiles in front; -1: the stream has bailed before this tile
};

// the bits of word w of a stream of n bytes that belong to the stream (the last word's padding does not)
PM_EV_HD uint64_t valid_bits(int64_t n, int64_t w)
{
    const int64_t have = n - 8 * w;
    return have >= 8 ? ~0ull : (1ull << (8 * have)) - 1;
}

// segment of consecutive words for the tile's one scan: stuffed zeros, the last reset with the zeros up to it, the last flag
struct Seg {
    int32_t s, ev, cs, fl;
};
PM_EV_HD Seg seg_none() { return Seg{0, -1, 0, -1}; }
PM_EV_HD Seg seg_join(const Seg &a, const Seg &b)
{
    Seg r;
    r.s = a.s + b.s;
    r.ev = b.ev >= 0 ? b.ev : a.ev;
    r.cs = b.ev >= 0 ? a.s + b.cs : a.cs;
    r.fl = b.fl >= 0 ? b.fl : a.fl;
    return r;
}

// the AX.25 patterns of one word (pm_codec.cpp: feed_many): stuffed zeros, resets, flags
struct Marks {
    uint64_t S, ev, flag;
};
PM_EV_HD Marks ax25_marks(uint64_t w, uint64_t prev, uint64_t valid)
{
    const uint64_t e1 = (w << 1) | (prev >> 63), e2 = (w << 2) | (prev >> 62), e3 = (w << 3) | (prev >> 61), e4 = (w << 4) | (prev >> 60),
                   e5 = (w << 5) | (prev >> 59), e6 = (w << 6) | (prev >> 58), e7 = (w << 7) | (prev >> 57);
    const uint64_t o5 = e1 & e2 & e3 & e4 & e5;
    Marks m;
    m.S = ~w & o5 & ~e6 & valid;
    m.ev = ~w & o5 & e6 & valid;
    m.flag = m.ev & ~e7;
    return m;
}

// Lane state for its word's events: where the tile's last reset / flag in front of the word lie (bits from the tile's start; -1: none
// inside the tile) and the stuffed zeros up to there and up to the word.  fn(P, is_flag, R, dropped, F): the event at bit P; R: first
// bit after the reset in front of it inside the tile (-1: none, `dropped` then counts from the tile's start); F likewise for flags.
struct LaneIn {
    Marks m;
    int32_t base, R, sR, exS, F;
};
template <class Fn>
PM_EV_HD void walk_events(const LaneIn &in, Fn fn)
{
    int32_t R = in.R, sR = in.sR, F = in.F;
    for (uint64_t e = in.m.ev; e; e &= e - 1) {
        const int i = __builtin_ctzll(e);
        const int32_t P = in.base + i, here = in.exS + __builtin_popcountll(in.m.S & ((1ull << i) - 1));
        const bool is_flag = (in.m.flag >> i) & 1;
        if (!fn(P, is_flag, R, here - sR, F)) return;
        R = P + 1;
        sR = here;
        if (is_flag) F = P + 1;
    }
}

// the lane's own segment: its word's marks (lane: the word's place in the tile)
PM_EV_HD Seg lane_seg(const Marks &m, bool active, int lane)
{
    Seg mine = seg_none();
    if (active) {
        mine.s = __builtin_popcountll(m.S);
        if (m.ev) {
            const int hi = 63 - __builtin_clzll(m.ev);
            mine.ev = lane * 64 + hi;
            mine.cs = __builtin_popcountll(m.S & ((2ull << hi) - 1));
        }
        if (m.flag) mine.fl = lane * 64 + 63 - __builtin_clzll(m.flag);
    }
    return mine;
}
// the lane's state from the joined segments of the lanes in front of it (seg_none() for lane 0)
PM_EV_HD LaneIn lane_in(const Marks &m, bool active, int lane, const Seg &before)
{
    LaneIn in;
    in.m = m;
    if (!active) in.m.ev = 0;
    in.base = lane * 64;
    in.R = before.ev >= 0 ? before.ev + 1 : -1;
    in.sR = before.ev >= 0 ? before.cs : 0;
    in.exS = before.s;
    in.F = before.fl >= 0 ? before.fl + 1 : -1;
    return in;
}

PM_EV_HD bool closes(int64_t T) { return (T & 7) == 7 && T >= kCloseBits; }

// ---- the tile launch ----------------------------------------------------------------------------------------------------------------
// First walk: the lane's first event whose span since a reset inside the tile reaches kBailSpan, kNoBail if it has none.  The least of
// the lanes' candidates is the tile's `bail`.
PM_EV_HD int32_t tile_bail_candidate(const LaneIn &in)
{
    int32_t cand = kNoBail;
    walk_events(in, [&](int32_t P, bool, int32_t R, int32_t, int32_t) {
        if (R >= 0 && P - R >= kBailSpan) {
            cand = P;
            return false;
        }
        return true;
    });
    return cand;
}
// Second walk: the lane's events in front of `limit` (the tile's bail, kNoBail if none) into the tile's summary through `acc`, which
// several lanes may call at once:
//   acc.first_reset(P, dropped, is_flag)   the tile's first reset (one lane meets it)
//   acc.first_flag(P, closing)             the tile's first flag (one lane meets it)
//   acc.closing(count)                     closing flags of the lane whose reset lies inside the tile (count > 0)
//   acc.last_flag(P)                       the lane's last flag
template <class Acc>
PM_EV_HD void tile_summarise(const LaneIn &in, int32_t limit, Acc &acc)
{
    int closing = 0, last_flag = -1;
    walk_events(in, [&](int32_t P, bool is_flag, int32_t R, int32_t dropped, int32_t F) {
        if (P >= limit) return false;
        if (R < 0) acc.first_reset(P, dropped, is_flag);
        if (is_flag) {
            const bool c = R >= 0 && closes((int64_t)(P - R) - dropped);
            if (F < 0) acc.first_flag(P, c);
            closing += c;
            last_flag = P;
        }
        return true;
    });
    if (closing) acc.closing(closing);
    if (last_flag >= 0) acc.last_flag(last_flag);
}
// what the whole tile's segment adds to the summary
PM_EV_HD void tile_totals(TileSum &ts, const Seg &total)
{
    ts.dropped = total.s;
    ts.last_reset = total.ev;
    ts.dropped_after_last = total.ev >= 0 ? total.s - total.cs : total.s;
}

// ---- the combine launch -------------------------------------------------------------------------------------------------------------
// The stream in front of a tile: first bit after the last reset and after the last flag, the bail bit, stuffed zeros since the reset,
// events so far.
struct Combine {
    int64_t R, LF, bail;
    int32_t since, events;
};
PM_EV_HD Combine combine_start() { return Combine{0, -1, -1, 0, 0}; }
PM_EV_HD TileCarry combine_carry(const Combine &st) { return TileCarry{st.R, st.LF, -1, st.since, st.bail >= 0 ? -1 : st.events}; }
// One AX.25 tile: its summary `s` and its first bit B onto the state; returns what the tile starts from.
PM_EV_HD TileCarry combine_step(Combine &st, const TileSum &s, int64_t B)
{
    TileCarry c = combine_carry(st);
    if (st.bail >= 0) return c;
    if (s.first_reset >= 0) {
        const int64_t P0 = B + s.first_reset, span = P0 - st.R;
        if (span >= kBailSpan) {
            st.bail = c.bail = P0;
        } else {
            if (s.bits & 1) {
                if (st.LF < 0 || closes(span - (st.since + s.dropped_to_first))) ++st.events;
            } else if (st.LF < 0 && s.first_flag >= 0 && !(s.bits & 2)) {
                ++st.events;                                // the stream's first flag, whatever it closes
            }
            st.events += s.closing;
            if (s.last_flag >= 0) st.LF = B + s.last_flag + 1;
            if (s.bail >= 0) {
                st.bail = c.bail = B + s.bail;
            } else {
                st.R = B + s.last_reset + 1;
                st.since = s.dropped_after_last;
            }
        }
    } else {
        st.since += s.dropped;
    }
    return c;
}
// the record's AX.25 fields behind the stream's last tile
struct Record {
    int64_t bail_bit, last_flag;
    int32_t events;
};
PM_EV_HD Record combine_record(const Combine &st) { return Record{st.bail, st.LF, st.events}; }

// ---- the emit launch ----------------------------------------------------------------------------------------------------------------
// The lane's listed flags {P, F} in stream order.  A closing flag has 151 counted bits behind it, so a word holds one at most, and the
// stream's first flag beside it: two places.  `wanted` counts what the walk would have listed; bitscan_core_check.cpp fails on a lane
// that wanted more than two (tests/test_bitscan_core.py runs it over every stream at every tile size).
struct Listed {
    uint32_t P0, F0, P1, F1;                // (no array: one indexed by `wanted` would be given a place in LDS on the device)
    int32_t wanted;
    int32_t nothing;                        // bit k set when place k closes no frame (the stream's first flag only)
};
PM_EV_HD int listed_count(const Listed &l) { return l.wanted < 2 ? l.wanted : 2; }
PM_EV_HD uint32_t listed_P(const Listed &l, int k) { return k ? l.P1 : l.P0; }
PM_EV_HD uint32_t listed_F(const Listed &l, int k) { return k ? l.F1 : l.F0; }
// c: what the tile starts from; B: the tile's first bit
PM_EV_HD Listed emit_lane(const LaneIn &in, const TileCarry &c, int64_t B)
{
    uint32_t P0 = 0, F0 = 0, P1 = 0, F1 = 0;
    int32_t wanted = 0, nothing = 0;
    const int64_t limit = c.bail >= 0 ? c.bail : INT64_MAX;
    walk_events(in, [&](int32_t P, bool is_flag, int32_t R, int32_t dropped, int32_t F) {
        const int64_t Pa = B + P;
        if (Pa >= limit) return false;
        if (!is_flag) return true;
        const int64_t T = R >= 0 ? (int64_t)(P - R) - dropped : (Pa - c.after_reset) - ((int64_t)c.dropped + dropped);
        const int64_t Fa = F >= 0 ? B + F : c.after_flag;
        if (Fa < 0 || closes(T)) {
            if (wanted < 2 && !closes(T)) nothing |= 1 << wanted;
            const bool first = wanted == 0, second = wanted == 1;
            P0 = first ? (uint32_t)Pa : P0;
            F0 = first ? (uint32_t)Fa : F0;
            P1 = second ? (uint32_t)Pa : P1;
            F1 = second ? (uint32_t)Fa : F1;
            ++wanted;
        }
        return true;
    });
    return Listed{P0, F0, P1, F1, wanted, nothing};
}

// ---- a stream scanned in pieces (pm_scan_carry) -------------------------------------------------------------------------------------
// A piece starts from what the piece before left: the bits in front of word 0 (`tail`, the last 64 descrambled bits, bit 63 the last) are
// word 0's `prev`, and the combine starts `counted` bits behind a reset -- R = -counted, so that combine_step's span = P - R and
// emit_lane's T are feed_many's T0 + (P - R) and span - dropped as they stand.  LOST starts kBailSpan bits behind one: the first reset bails.
constexpr int kCarryStart = 0, kCarryOk = 1, kCarryLost = 2;        // PM_SCAN_CARRY_START / _OK / _LOST
PM_EV_HD Combine combine_start_carried(int state, int64_t counted)
{
    Combine st = combine_start();
    st.R = state == kCarryLost ? -(int64_t)kBailSpan : state == kCarryOk ? -counted : 0;
    return st;
}
// The piece's last reset and the stuffed zeros behind it, over every tile, wherever a bail fell (TileSum's dropped, last_reset and
// dropped_after_last do not depend on the bail).
struct PieceEnd {
    int64_t R, since;
};
PM_EV_HD PieceEnd piece_end_start(int64_t counted) { return PieceEnd{-counted, 0}; }
PM_EV_HD void piece_end_step(PieceEnd &e, const TileSum &s, int64_t B)
{
    if (s.last_reset >= 0) {
        e.R = B + s.last_reset + 1;
        e.since = s.dropped_after_last;
    } else {
        e.since += s.dropped;
    }
}
// `counted` behind a piece of n bytes that ends in `ones` ones (capped at 7).  The decoder clears its counters at the seventh one of a run
// and at every one after it, in front of the zero that is the reset here: a piece that ends inside such a run hands on 0, as the
// decoder's registers say, and the run's end in the next piece is a reset whatever was counted.
PM_EV_HD int64_t piece_counted(const PieceEnd &e, int64_t n, int ones) { return ones >= 7 ? 0 : 8 * n - e.R - e.since; }
// the state behind a piece: LOST if it started LOST or bailed
PM_EV_HD int piece_state(int state_in, const Combine &st) { return state_in == kCarryLost || st.bail >= 0 ? kCarryLost : kCarryOk; }
// the tail behind a piece: `last` holds the piece's last min(64, 8 n) bits, the stream's last bit on top of them (n >= 8: all 64)
PM_EV_HD uint64_t tail_join(uint64_t tail, uint64_t last, int64_t n)
{
    if (n >= 8) return last;
    if (n <= 0) return tail;
    return (tail >> (8 * n)) | (last << (64 - 8 * n));
}
PM_EV_HD int tail_ones(uint64_t tail)
{
    const uint64_t z = ~tail;
    const int k = z ? __builtin_clzll(z) : 64;
    return k < 7 ? k : 7;
}
// the tail of a decoder with `ones` ones behind a zero (pm_codec.cpp: feed_many's prev)
PM_EV_HD uint64_t tail_of_ones(int ones) { return ones >= 7 ? 0xFFull << 56 : ones > 0 ? ~0ull << (64 - ones) : 0; }

}  // namespace pm_events
