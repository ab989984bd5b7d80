// pm_rows_packets without a GPU: the three launches of pm_bitscan.hip stepped on the host, lane by lane, with the rules of
// csrc/pm_rows_packets.h -- the walk launch's workgroups (the sums of the rows in front, the scan of their own 256, the row's rule), the
// room launch's trips of 256 with their carry, the build launch's search for a packet's row and the packet itself -- over calls that
// tests/test_rows_packets_core.py writes to a file from the model blocks.  Every entry and every packet row must be the model's
// (tests/rows_packets_model.py), byte for byte.  Then every finished row's bytes go through the host decoder (pm_codec_decode +
// pm_codec_fetch, pm_codec.cpp, compiled into this program): the rows it hands out must be the same rows, which holds the shared header
// rebuild and Hamming table of pm_il2p_core.h to both sides.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pm_rows_packets.h"

int pm_set_error(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
    return code;
}

namespace {

template <class T>
T get(FILE *f)
{
    T v;
    if (fread(&v, sizeof(T), 1, f) != 1) exit(2);
    return v;
}

struct Chain {
    int32_t kind, tol, crc, source, disable_rs, min_dist;
};
constexpr int kLanes = 256;

int bad = 0;
void fail(int call, int row, const char *what)
{
    if (++bad <= 20) printf("call %d row %d: %s\n", call, row, what);
}

int run_call(FILE *f, int call, long *finished_rows, long *decoded_rows)
{
    using namespace pm_rows;
    using namespace pm_rpk;
    const int32_t nrows = get<int32_t>(f), nchains = get<int32_t>(f);
    const int64_t row0 = get<int64_t>(f), capacity = get<int64_t>(f), cap = get<int64_t>(f);
    std::vector<Chain> chains((size_t)nchains);
    for (auto &c : chains) c = get<Chain>(f);
    std::vector<int64_t> rec_count((size_t)nrows), host_count((size_t)nrows), offs((size_t)nrows);
    std::vector<uint64_t> block;                            // 8-byte aligned, as the device's is
    auto chain_of = [&](int r) -> const Chain & { return chains[(size_t)((row0 + r) % nchains)]; };
    Sums all = sums_zero();
    for (int r = 0; r < nrows; ++r) {
        rec_count[(size_t)r] = get<int64_t>(f);
        host_count[(size_t)r] = get<int64_t>(f);
        const int64_t bytes = get<int64_t>(f);
        const Chain &c = chain_of(r);
        const int64_t want = part_bytes(c.kind, c.kind == 0, c.kind == 1, host_count[(size_t)r], c.kind >= 0);
        if (bytes != want) {
            printf("call %d row %d: a part of %lld bytes, the layout says %lld\n", call, r, (long long)bytes, (long long)want);
            return 2;
        }
        offs[(size_t)r] = all.off;
        block.resize((size_t)(all.off + bytes) / 8);
        if (bytes && fread(reinterpret_cast<uint8_t *>(block.data()) + all.off, 1, (size_t)bytes, f) != (size_t)bytes) return 2;
        all = sums_add(all, row_sums(c.kind, c.kind == 0, c.kind == 1, host_count[(size_t)r], kLanes, c.kind >= 0));
    }
    const uint8_t *blk = reinterpret_cast<const uint8_t *>(block.data());
    const pm_rows_packets_head want_head = get<pm_rows_packets_head>(f);
    std::vector<pm_rows_packets_entry> want_entries((size_t)nrows);
    if (fread(want_entries.data(), sizeof(pm_rows_packets_entry), (size_t)nrows, f) != (size_t)nrows) return 2;
    std::vector<pm_packet> want_rows((size_t)want_head.packets);
    if (want_head.packets && fread(want_rows.data(), sizeof(pm_packet), want_rows.size(), f) != want_rows.size()) return 2;

    // ---- launch 1: workgroup by workgroup, lane by lane
    struct Info {
        int64_t scan, acc0;
        int32_t n;
    };
    std::vector<pm_rows_packets_entry> entries((size_t)nrows);
    std::vector<Info> info((size_t)nrows);
    std::vector<Accepted> acc((size_t)(all.events + all.places));
    auto sums_of = [&](int r) {
        const Chain &c = chain_of(r);
        const int64_t n = row_bytes(rec_count[(size_t)r], cap);
        return row_sums(c.kind, c.kind == 0, c.kind == 1, n, kLanes, c.kind >= 0);
    };
    for (int r0 = 0; r0 < nrows; r0 += kLanes) {
        Sums lane_front[kLanes];
        for (int t = 0; t < kLanes; ++t) {
            lane_front[t] = sums_zero();
            for (int r = t; r < r0; r += kLanes) lane_front[t] = sums_add(lane_front[t], sums_of(r));
        }
        Sums front = sums_zero();
        for (int t = 0; t < kLanes; ++t) front = sums_add(front, lane_front[t]);
        Sums upto = sums_zero();                            // the scan over the workgroup's lanes
        for (int t = 0; t < kLanes && r0 + t < nrows; ++t) {
            const int r = r0 + t;
            const Chain &c = chain_of(r);
            const Sums before = sums_add(front, upto);
            upto = sums_add(upto, sums_of(r));
            const Entry e = row_entry(before, c.kind, c.kind == 0, c.kind == 1, row_bytes(rec_count[(size_t)r], cap), kLanes, all, c.kind >= 0);
            pm_rows_packets_entry out{0, PM_ROWS_PACKETS_LEFT_OUT, 0, 0, 0, 0};
            Info ri{-1, before.events + before.places, e.n};
            if (e.off >= 0) {
                if (e.off != offs[(size_t)r] || e.n != host_count[(size_t)r]) fail(call, r, "the row's part is not where the host's offsets put it");
                ri.scan = e.off + steps_bytes(e.n);
                const Part p = part_of(blk + ri.scan, c.kind, e.n);
                out.lfsr_state = ld64(p.rec);
                Accepted *mine = acc.data() + ri.acc0;
                const int64_t room = (c.kind == 0 ? row_events(1, e.n) : row_places(c.kind == 1, e.n));
                auto emit = [&](int i, const Accepted &a) {
                    if (i >= room) fail(call, r, "more accepted than the row has places");
                    else mine[i] = a;
                };
                if (c.kind == 1) out.status = il2p_walk(p, c.tol, c.crc != 0, &out.packets, &out.corrected_left, emit);
                else if (c.kind == 0) out.status = ax25_walk(p, &out.packets, emit);
                else out.status = PM_ROWS_PACKETS_NO_CODEC;
                if (out.status != PM_ROWS_PACKETS_FINISHED) out.packets = out.corrected_left = 0;
            }
            entries[(size_t)r] = out;
            info[(size_t)r] = ri;
        }
    }
    // ---- launch 2: trips of 256, the carry from trip to trip
    int64_t carry = 0, kept = 0;
    int32_t handed = 0;
    for (int r0 = 0; r0 < nrows; r0 += kLanes) {
        int64_t incl[kLanes], run = 0;
        for (int t = 0; t < kLanes; ++t) {
            run += r0 + t < nrows ? entries[(size_t)(r0 + t)].packets : 0;
            incl[t] = carry + run;
        }
        carry += run;
        for (int t = 0; t < kLanes && r0 + t < nrows; ++t)
            if (!no_room(incl[t], capacity) && incl[t] > kept) kept = incl[t];
        for (int t = 0; t < kLanes && r0 + t < nrows; ++t) {
            pm_rows_packets_entry &e = entries[(size_t)(r0 + t)];
            const bool over = no_room(incl[t], capacity);
            if (over || e.status != PM_ROWS_PACKETS_FINISHED) ++handed;
            e.first = over ? kept : incl[t] - e.packets;
            if (over) {
                e.status = PM_ROWS_PACKETS_NO_ROOM;
                e.packets = e.corrected_left = 0;
            }
        }
    }
    if (nrows != want_head.rows || handed != want_head.handed || kept != want_head.packets) fail(call, -1, "the head");
    for (int r = 0; r < nrows; ++r) {
        pm_rows_packets_entry w = want_entries[(size_t)r];
        w.lfsr_state = entries[(size_t)r].lfsr_state;      // (the model's blocks carry no register)
        if (memcmp(&w, &entries[(size_t)r], sizeof(w))) {
            printf("call %d row %d: entry {%d, %d, %lld, %d}, the model says {%d, %d, %lld, %d}\n", call, r, entries[(size_t)r].status, entries[(size_t)r].packets,
                   (long long)entries[(size_t)r].first, entries[(size_t)r].corrected_left, w.status, w.packets, (long long)w.first, w.corrected_left);
            ++bad;
        }
    }
    if (bad) return 1;
    // ---- launch 3: packet by packet
    std::vector<pm_packet> rows((size_t)kept);
    for (int64_t q = 0; q < kept; ++q) {
        const int r = row_of_packet([&](int i) { return entries[(size_t)i].first; }, nrows, q);
        const pm_rows_packets_entry &e = entries[(size_t)r];
        if (q < e.first || q >= e.first + e.packets) {
            fail(call, r, "the search for a packet's row");
            continue;
        }
        const Chain &c = chain_of(r);
        const Info ri = info[(size_t)r];
        const Part p = part_of(blk + ri.scan, c.kind, ri.n);
        memset(&rows[(size_t)q], 0xEE, sizeof(pm_packet));
        packet_build(p, c.kind, acc[(size_t)(ri.acc0 + (q - e.first))], c.crc != 0, reinterpret_cast<const uint16_t *>(blk + offs[(size_t)r]), c.source,
                     reinterpret_cast<uint8_t *>(&rows[(size_t)q]));
        if (memcmp(&rows[(size_t)q], &want_rows[(size_t)q], sizeof(pm_packet))) fail(call, r, "a packet row is not the model's");
    }
    // ---- the host decoder on every finished row
    for (int r = 0; r < nrows; ++r) {
        const pm_rows_packets_entry &e = entries[(size_t)r];
        if (e.status != PM_ROWS_PACKETS_FINISHED) continue;
        ++*finished_rows;
        const Chain &c = chain_of(r);
        const Info ri = info[(size_t)r];
        const Part p = part_of(blk + ri.scan, c.kind, ri.n);
        const uint16_t *steps = reinterpret_cast<const uint16_t *>(blk + offs[(size_t)r]);
        std::vector<int64_t> addr((size_t)ri.n);
        for (int64_t k = 0; k < ri.n; ++k) addr[(size_t)k] = pm_addrs::resolve(p.addrs, steps, k);
        pm_codec *codec = nullptr;
        if (pm_codec_create(c.kind, c.crc, c.disable_rs, c.min_dist, c.tol, c.source, &codec)) return 2;
        int64_t pending = 0, got = 0;
        if (pm_codec_decode(codec, p.plain, addr.data(), ri.n, &pending)) return 2;
        std::vector<pm_packet> fetched((size_t)pending + 1);
        if (pm_codec_fetch(codec, fetched.data(), pending, &got)) return 2;
        pm_codec_destroy(codec);
        if (got != e.packets) {
            fail(call, r, "the host decoder finds another number of packets");
            continue;
        }
        for (int64_t i = 0; i < got; ++i)
            if (memcmp(&fetched[(size_t)i], &rows[(size_t)(e.first + i)], sizeof(pm_packet))) fail(call, r, "pm_codec_fetch hands out another row");
        *decoded_rows += got;
    }
    return bad ? 1 : 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const int32_t calls = get<int32_t>(f);
    long finished = 0, decoded = 0;
    for (int c = 0; c < calls; ++c)
        if (int rc = run_call(f, c, &finished, &decoded)) {
            printf("call %d: %d\n", c, rc);
            return rc;
        }
    fclose(f);
    printf("%d calls, %ld finished rows, %ld packets through the host decoder, %d bad\n", calls, finished, decoded, bad);
    return bad ? 1 : 0;
}
