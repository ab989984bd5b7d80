// pm_stream_scan's three AX.25 launches (csrc/pm_bitscan.hip) stepped on the host: the tile launch's lanes one after the other (the scan
// over the lanes a loop, the LDS atomics plain updates), the combine tile by tile, then the emit's lanes.  What decides the list is the
// kernels' own text (csrc/pm_bitscan_events.h).  test_bitscan_core.py compiles this, feeds it descrambled streams with the record and
// the list that the bit-serial model finds, and expects both at every tile size.
//   bitscan_core_check <file> <first tile size> <last tile size>      (words per tile, 1..256)
//   file: int32 streams; per stream int32 n, n descrambled bytes, int64 bail_bit, int64 last_flag, int32 events;
//         per event uint32 P, uint32 F, int32 closes (0: the stream's first flag, closing nothing)
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

struct Event {
    uint32_t P, F;
    int32_t closes;
};
struct Stream {
    int64_t n, nw;
    std::vector<uint64_t> x;                // the words as the kernels see them: stream order, the padding masked
    int64_t bail, last_flag;
    std::vector<Event> events;
};

// plain updates where the kernel's lanes use LDS atomics; a second "one lane meets it" is the kernel's plain stores racing
struct HostAcc {
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

// what both the tile launch and the emit launch do first: the lanes' words, marks and states, the tile's whole segment
static Seg prepare(const Stream &s, int tw, int64_t tile, LaneIn *in)
{
    Seg upto = seg_none();
    for (int lane = 0; lane < kLanes; ++lane) {
        const int64_t w = tile * tw + lane;
        const bool active = lane < tw && w < s.nw;
        uint64_t x = 0, xp = 0, valid = 0;
        if (active) {
            valid = valid_bits(s.n, w);
            x = s.x[(size_t)w] & valid;
            xp = w ? s.x[(size_t)(w - 1)] : 0;
        }
        const Marks m = ax25_marks(x, xp, valid);
        in[lane] = lane_in(m, active, lane, upto);          // upto: the lanes in front
        upto = seg_join(upto, lane_seg(m, active, lane));
    }
    return upto;
}

int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    FILE *f = fopen(argv[1], "rb");
    const int tw_first = atoi(argv[2]), tw_last = atoi(argv[3]);
    if (!f || tw_first < 1 || tw_last > kLanes || tw_first > tw_last) return 2;
    std::vector<Stream> streams((size_t)take<int32_t>(f));
    for (Stream &s : streams) {
        s.n = take<int32_t>(f);
        s.nw = (s.n + 7) / 8;
        std::vector<uint8_t> d((size_t)s.n);
        if (s.n && fread(d.data(), 1, d.size(), f) != d.size()) return 2;
        s.x.assign((size_t)s.nw, 0);
        for (int64_t t = 0; t < 8 * s.n; ++t)
            if ((d[(size_t)(t >> 3)] >> (7 - (t & 7))) & 1) s.x[(size_t)(t >> 6)] |= 1ull << (t & 63);
        s.bail = take<int64_t>(f);
        s.last_flag = take<int64_t>(f);
        s.events.resize((size_t)take<int32_t>(f));
        for (Event &e : s.events) {
            e.P = take<uint32_t>(f);
            e.F = take<uint32_t>(f);
            e.closes = take<int32_t>(f);
        }
    }
    int bad = 0, third = 0, most = 0, races = 0, runs = 0;
    LaneIn in[kLanes];
    for (int tw = tw_first; tw <= tw_last; ++tw) {
        for (size_t si = 0; si < streams.size(); ++si) {
            const Stream &s = streams[si];
            const int64_t tiles = (s.nw + tw - 1) / tw, cap = s.n / 19 + 2;
            ++runs;
            // launch 1: a summary per tile
            std::vector<TileSum> sums((size_t)tiles);
            for (int64_t t = 0; t < tiles; ++t) {
                const Seg total = prepare(s, tw, t, in);
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
            // launch 2: the summaries in order
            std::vector<TileCarry> carries((size_t)tiles);
            Combine st = combine_start();
            for (int64_t t = 0; t < tiles; ++t) carries[(size_t)t] = combine_step(st, sums[(size_t)t], t * tw * 64);
            const Record rec = combine_record(st);
            // launch 3: the list, every place written once
            std::vector<Event> list((size_t)cap, Event{0, 0, -1});
            int twice = 0;
            for (int64_t t = 0; t < tiles; ++t) {
                const TileCarry c = carries[(size_t)t];
                if (c.events < 0) continue;
                prepare(s, tw, t, in);
                int64_t at = c.events;                      // (the kernel: a scan of the lanes' counts)
                for (int lane = 0; lane < kLanes; ++lane) {
                    const Listed l = emit_lane(in[lane], c, t * tw * 64);
                    third += l.wanted > 2;
                    most = l.wanted > most ? l.wanted : most;
                    for (int k = 0; k < listed_count(l); ++k, ++at) {
                        if (at >= cap) continue;
                        twice += list[(size_t)at].closes >= 0;
                        list[(size_t)at] = Event{listed_P(l, k), listed_F(l, k), !((l.nothing >> k) & 1)};
                    }
                }
            }
            bool ok = rec.bail_bit == s.bail && rec.last_flag == s.last_flag && rec.events == (int32_t)s.events.size() && !twice;
            for (int64_t k = 0; k < cap && ok; ++k) {
                const Event &g = list[(size_t)k];
                if (k < (int64_t)s.events.size()) {
                    const Event &w = s.events[(size_t)k];
                    ok = g.P == w.P && g.F == w.F && g.closes == w.closes;
                } else {
                    ok = g.closes < 0;                      // nothing is written behind the list
                }
            }
            if (!ok) {
                if (++bad <= 20)
                    printf("stream %zu, tile of %d words: bail %lld (model %lld), last flag %lld (%lld), events %d (%zu), %d places written twice\n", si, tw,
                           (long long)rec.bail_bit, (long long)s.bail, (long long)rec.last_flag, (long long)s.last_flag, rec.events, s.events.size(), twice);
            }
        }
    }
    printf("%d runs, %d mismatches, %d lanes wanted a third event (most in a lane: %d), %d racing stores\n", runs, bad, third, most, races);
    return bad || third || races;
}
