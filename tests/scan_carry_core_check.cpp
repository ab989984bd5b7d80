// pm_stream_scan's three AX.25 launches for a stream scanned in PIECES (pm_scan_job.d_carry, csrc/pm_bitscan.hip), stepped on the host as
// bitscan_core_check.cpp steps them for a whole stream: word 0's predecessor is the carry's tail, the combine starts from the carry
// (combine_start_carried) and keeps the piece's end beside it (PieceEnd), and what its lane 0 writes -- tail, ones, counted, state -- goes
// on to the next piece.  What decides is the kernels' own text (csrc/pm_bitscan_events.h).  test_scan_carry_core.py compiles this, feeds
// it the pieces' descrambled bytes with the records, lists and carries of the bit-serial model (scan_carry_model.py), and expects them
// at every tile size it names.  The first piece starts from the file's carry, every later one from what this program left.
//   scan_carry_core_check <file> <tile size> [<tile size> ...]      (words per tile, 1..256)
//   file: int32 streams; per stream int32 pieces; per piece
//         int32 n, n descrambled bytes, the carry in front {int32 state, int32 ones, int64 counted, uint64 tail},
//         int64 bail_bit, int64 last_flag, int32 events, per event uint32 P, uint32 F, the carry behind (as in front)
#include "pm_bitscan_events.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace pm_events;

constexpr int kLanes = 256;

template <class T>
static T take(FILE *f)
{
    T v;
    if (fread(&v, sizeof(T), 1, f) != 1) exit(2);
    return v;
}

struct Carry {
    int32_t state, ones;
    int64_t counted;
    uint64_t tail;
};
static bool same(const Carry &a, const Carry &b) { return a.state == b.state && a.ones == b.ones && a.counted == b.counted && a.tail == b.tail; }
static Carry take_carry(FILE *f)
{
    Carry c;
    c.state = take<int32_t>(f);
    c.ones = take<int32_t>(f);
    c.counted = take<int64_t>(f);
    c.tail = take<uint64_t>(f);
    return c;
}
struct Event {
    uint32_t P, F;
};
struct Piece {
    int64_t n, nw;
    std::vector<uint64_t> x;                // the words as the kernels see them: stream order, the padding masked
    Carry in, out;
    int64_t bail, last_flag;
    std::vector<Event> events;
};

struct HostAcc {                            // plain updates where the kernel's lanes use LDS atomics
    TileSum &ts;
    int &races;
    int resets = 0, flags = 0;
    void first_reset(int32_t P, int32_t dropped, bool is_flag)
    {
        races += resets++ > 0;
        ts.first_reset = P;
        ts.dropped_to_first = dropped;
        if (is_flag) ts.bits |= 1;
    }
    void first_flag(int32_t P, bool c)
    {
        races += flags++ > 0;
        ts.first_flag = P;
        if (c) ts.bits |= 2;
    }
    void closing(int count) { ts.closing += count; }
    void last_flag(int32_t P) { ts.last_flag = P > ts.last_flag ? P : ts.last_flag; }
};

// the lanes' words, marks and states of a tile; word 0 of the piece has the carry's tail in front of it
static Seg prepare(const Piece &s, uint64_t tail, int tw, int64_t tile, LaneIn *in)
{
    Seg upto = seg_none();
    for (int lane = 0; lane < kLanes; ++lane) {
        const int64_t w = tile * tw + lane;
        const bool active = lane < tw && w < s.nw;
        uint64_t x = 0, xp = 0, valid = 0;
        if (active) {
            valid = valid_bits(s.n, w);
            x = s.x[(size_t)w] & valid;
            xp = w ? s.x[(size_t)(w - 1)] : tail;
        }
        const Marks m = ax25_marks(x, xp, valid);
        in[lane] = lane_in(m, active, lane, upto);
        upto = seg_join(upto, lane_seg(m, active, lane));
    }
    return upto;
}

// the piece's last min(64, 8 n) bits, the last one on top of them (pm_bitscan.hip: stream_bits64 from bit 8 n - 64)
static uint64_t last_bits(const Piece &s)
{
    if (s.n <= 0) return 0;
    if (s.n < 8) return s.x[0] & valid_bits(s.n, 0);
    const int64_t B = 8 * s.n - 64, w = B >> 6;
    const int sh = (int)(B & 63);
    const uint64_t lo = s.x[(size_t)w] >> sh;
    return sh ? lo | (s.x[(size_t)(w + 1)] << (64 - sh)) : lo;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<int> sizes;
    for (int a = 2; a < argc; ++a) {
        const int tw = atoi(argv[a]);
        if (tw < 1 || tw > kLanes) return 2;
        sizes.push_back(tw);
    }
    std::vector<std::vector<Piece>> streams((size_t)take<int32_t>(f));
    for (auto &pieces : streams) {
        pieces.resize((size_t)take<int32_t>(f));
        for (Piece &s : pieces) {
            s.n = take<int32_t>(f);
            s.nw = (s.n + 7) / 8;
            std::vector<uint8_t> d((size_t)s.n);
            if (s.n && fread(d.data(), 1, d.size(), f) != d.size()) return 2;
            s.x.assign((size_t)s.nw, 0);
            for (int64_t t = 0; t < 8 * s.n; ++t)
                if ((d[(size_t)(t >> 3)] >> (7 - (t & 7))) & 1) s.x[(size_t)(t >> 6)] |= 1ull << (t & 63);
            s.in = take_carry(f);
            s.bail = take<int64_t>(f);
            s.last_flag = take<int64_t>(f);
            s.events.resize((size_t)take<int32_t>(f));
            for (Event &e : s.events) {
                e.P = take<uint32_t>(f);
                e.F = take<uint32_t>(f);
            }
            s.out = take_carry(f);
        }
    }
    int bad = 0, third = 0, races = 0, runs = 0;
    LaneIn in[kLanes];
    for (int tw : sizes) {
        for (size_t si = 0; si < streams.size(); ++si) {
            Carry carry = streams[si].empty() ? Carry{0, 0, 0, 0} : streams[si][0].in;
            for (size_t pi = 0; pi < streams[si].size(); ++pi) {
                const Piece &s = streams[si][pi];
                const int64_t tiles = (s.nw + tw - 1) / tw, cap = s.n / 19 + 2;
                ++runs;
                const bool in_ok = same(carry, s.in);
                // launch 1: a summary per tile
                std::vector<TileSum> sums((size_t)tiles);
                for (int64_t t = 0; t < tiles; ++t) {
                    const Seg total = prepare(s, carry.tail, tw, t, in);
                    TileSum ts = tile_sum_empty();
                    ts.bail = kNoBail;
                    for (int lane = 0; lane < kLanes; ++lane) {
                        const int32_t cand = tile_bail_candidate(in[lane]);
                        if (cand < ts.bail) ts.bail = cand;
                    }
                    HostAcc acc{ts, races};
                    const int32_t limit = ts.bail;
                    for (int lane = 0; lane < kLanes; ++lane) tile_summarise(in[lane], limit, acc);
                    tile_totals(ts, total);
                    if (ts.bail == kNoBail) ts.bail = -1;
                    sums[(size_t)t] = ts;
                }
                // launch 2: the summaries in order, from the carry; the piece's end beside them
                std::vector<TileCarry> carries((size_t)tiles);
                Combine st = combine_start_carried(carry.state, carry.counted);
                PieceEnd pe = piece_end_start(carry.counted);
                for (int64_t t = 0; t < tiles; ++t) {
                    carries[(size_t)t] = combine_step(st, sums[(size_t)t], t * tw * 64);
                    piece_end_step(pe, sums[(size_t)t], t * tw * 64);
                }
                const Record rec = combine_record(st);
                Carry out;
                out.tail = tail_join(carry.tail, last_bits(s), s.n);
                out.ones = tail_ones(out.tail);
                out.counted = piece_counted(pe, s.n, out.ones);
                out.state = piece_state(carry.state, st);
                // launch 3: the list, every place written once
                std::vector<Event> list((size_t)cap, Event{0, 0});
                std::vector<int> written((size_t)cap, 0);
                int twice = 0;
                for (int64_t t = 0; t < tiles; ++t) {
                    const TileCarry c = carries[(size_t)t];
                    if (c.events < 0) continue;
                    prepare(s, carry.tail, tw, t, in);
                    int64_t at = c.events;
                    for (int lane = 0; lane < kLanes; ++lane) {
                        const Listed l = emit_lane(in[lane], c, t * tw * 64);
                        third += l.wanted > 2;
                        for (int k = 0; k < listed_count(l); ++k, ++at) {
                            if (at >= cap) continue;
                            twice += written[(size_t)at]++;
                            list[(size_t)at] = Event{listed_P(l, k), listed_F(l, k)};
                        }
                    }
                }
                bool ok = in_ok && rec.bail_bit == s.bail && rec.last_flag == s.last_flag && rec.events == (int32_t)s.events.size() && !twice && same(out, s.out);
                for (int64_t k = 0; k < cap && ok; ++k) {
                    if (k < (int64_t)s.events.size()) ok = written[(size_t)k] && list[(size_t)k].P == s.events[(size_t)k].P && list[(size_t)k].F == s.events[(size_t)k].F;
                    else ok = !written[(size_t)k];          // nothing is written behind the list
                }
                if (!ok && ++bad <= 20)
                    printf("stream %zu piece %zu, tile of %d words: carry in %s, bail %lld (model %lld), last flag %lld (%lld), events %d (%zu), %d places twice, "
                           "carry out {%d %d %lld %016llx} (model {%d %d %lld %016llx})\n",
                           si, pi, tw, in_ok ? "ok" : "differs", (long long)rec.bail_bit, (long long)s.bail, (long long)rec.last_flag, (long long)s.last_flag, rec.events,
                           s.events.size(), twice, out.state, out.ones, (long long)out.counted, (unsigned long long)out.tail, s.out.state, s.out.ones,
                           (long long)s.out.counted, (unsigned long long)s.out.tail);
                carry = out;
            }
        }
    }
    printf("%d runs, %d mismatches, %d lanes wanted a third event, %d racing stores\n", runs, bad, third, races);
    return bad || third || races;
}
