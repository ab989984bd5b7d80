// pm_stream_packets without a GPU: the three launches of pm_bitscan.hip stepped on the host with the rules of csrc/pm_rows_packets.h -- the
// walk launch's wave (AX.25: trips of 64 listed events, a lane an event, the ballot, the count of the lanes in front and the prefix sum of
// the record sizes emulated lane by lane, with their carries; IL2P: the rule on one lane), the room launch's scan over the jobs, the build
// launch's search for a record's job and the record itself -- over calls that tests/test_stream_packets_core.py writes to a file from the
// model blocks.  Every entry and every record must be the model's (tests/stream_packets_model.py), byte for byte; the wave walk's accepted
// list must be pm_rpk::ax25_walk's.  Then every finished stream goes through the host decoder (pm_codec_decode + pm_codec_fetch,
// pm_codec.cpp, compiled into this program): the packets it hands out must be the same records.
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

struct JobDesc {
    int32_t kind, tol, crc, source, disable_rs, min_dist;
    int64_t n, part_bytes;
};
constexpr int kWave = 64;

int bad = 0;
void fail(int call, int job, const char *what)
{
    if (++bad <= 20) printf("call %d job %d: %s\n", call, job, what);
}

int run_call(FILE *f, int call, long *finished_jobs, long *decoded)
{
    using namespace pm_rpk;
    const int32_t njobs = get<int32_t>(f);
    const int64_t room = get<int64_t>(f);
    if (njobs < 1 || njobs > kWave) return 2;
    std::vector<JobDesc> jobs((size_t)njobs);
    std::vector<std::vector<uint64_t>> parts((size_t)njobs);        // 8-byte aligned, as the device's are
    std::vector<std::vector<int64_t>> addrs((size_t)njobs);
    std::vector<int64_t> acc0((size_t)njobs);
    int64_t places = 0;
    for (int j = 0; j < njobs; ++j) {
        JobDesc &d = jobs[(size_t)j];
        d = get<JobDesc>(f);
        const int64_t want = pm_rows::scan_bytes(d.kind, d.kind == 0, d.kind == 1, d.n);
        if (d.part_bytes != want) {
            printf("call %d job %d: a part of %lld bytes, the layout says %lld\n", call, j, (long long)d.part_bytes, (long long)want);
            return 2;
        }
        parts[(size_t)j].resize((size_t)d.part_bytes / 8);
        if (d.part_bytes && fread(parts[(size_t)j].data(), 1, (size_t)d.part_bytes, f) != (size_t)d.part_bytes) return 2;
        addrs[(size_t)j].resize((size_t)d.n);
        if (d.n && fread(addrs[(size_t)j].data(), 8, (size_t)d.n, f) != (size_t)d.n) return 2;
        acc0[(size_t)j] = places;
        places += d.kind == 0 ? d.n / 19 + 2 : d.kind == 1 ? d.n / 64 + 2 : 0;
    }
    const pm_stream_packets_head want_head = get<pm_stream_packets_head>(f);
    std::vector<pm_stream_packets_entry> want_entries((size_t)njobs);
    if (fread(want_entries.data(), sizeof(pm_stream_packets_entry), (size_t)njobs, f) != (size_t)njobs) return 2;
    std::vector<uint8_t> want_records((size_t)want_head.bytes);
    if (want_head.bytes && fread(want_records.data(), 1, want_records.size(), f) != want_records.size()) return 2;
    auto part = [&](int j) {
        const JobDesc &d = jobs[(size_t)j];
        Part p = part_of(reinterpret_cast<const uint8_t *>(parts[(size_t)j].data()), d.kind, d.n);
        p.addrs = addrs[(size_t)j].data();
        return p;
    };

    // ---- launch 1: a wave a job
    std::vector<pm_stream_packets_entry> entries((size_t)njobs);
    std::vector<int64_t> bytes_of((size_t)njobs), first((size_t)njobs);
    std::vector<Accepted> acc((size_t)places + 1);
    std::vector<int64_t> recoff((size_t)places + 1);
    for (int j = 0; j < njobs; ++j) {
        const JobDesc &d = jobs[(size_t)j];
        const Part p = part(j);
        Accepted *mine = acc.data() + acc0[(size_t)j];
        int64_t *offs = recoff.data() + acc0[(size_t)j];
        const int64_t my_places = d.kind == 0 ? d.n / 19 + 2 : d.n / 64 + 2;
        pm_stream_packets_entry out{ld64(p.rec), PM_ROWS_PACKETS_NO_CODEC, 0, 0, 0, 0};
        int64_t bytes = 0;
        if (d.kind == 0) {
            int32_t events, count = 0;
            out.status = ax25_start(p, &events);
            for (int32_t e0 = 0; e0 < events; e0 += kWave) {
                Ax25Event ev[kWave];
                bool any_bad = false;
                uint64_t taken = 0;
                for (int lane = 0; lane < kWave; ++lane) {
                    ev[lane] = Ax25Event{false, false, 0, 0};
                    if (e0 + lane < events) ev[lane] = ax25_event(p, e0 + lane);
                    any_bad = any_bad || ev[lane].bad;
                    if (ev[lane].take) taken |= (uint64_t)1 << lane;
                }
                if (any_bad) {
                    out.status = PM_ROWS_PACKETS_LONG_FRAME;
                    break;
                }
                int64_t incl[kWave], run = 0;
                for (int lane = 0; lane < kWave; ++lane) {
                    run += ev[lane].take ? record_bytes(ev[lane].len) : 0;
                    incl[lane] = run;
                }
                for (int lane = 0; lane < kWave; ++lane) {
                    if (!ev[lane].take) continue;
                    const int place = count + lanes_before(taken, lane);
                    if (place >= my_places) {
                        fail(call, j, "more accepted than the job has places");
                        continue;
                    }
                    mine[place] = Accepted{(uint32_t)(e0 + lane), ev[lane].P, 0, 0};
                    offs[place] = bytes + incl[lane] - record_bytes(ev[lane].len);
                }
                count += __builtin_popcountll(taken);
                bytes += incl[kWave - 1];
            }
            out.packets = count;
            // the rule as one thread takes it: the same status, the same list
            std::vector<Accepted> serial;
            int32_t serial_count = 0;
            const int32_t serial_status = ax25_walk(p, &serial_count, [&](int, const Accepted &a) { serial.push_back(a); });
            if (serial_status != out.status) fail(call, j, "the wave walk's status is not ax25_walk's");
            if (serial_status == PM_ROWS_PACKETS_FINISHED &&
                (serial_count != count || (count && memcmp(serial.data(), mine, sizeof(Accepted) * (size_t)count))))
                fail(call, j, "the wave walk's accepted list is not ax25_walk's");
        } else if (d.kind == 1) {
            out.status = il2p_walk(p, d.tol, d.crc != 0, &out.packets, &out.corrected_left, [&](int i, const Accepted &a) {
                if (i >= my_places) {
                    fail(call, j, "more accepted than the job has places");
                    return;
                }
                mine[i] = a;
                offs[i] = bytes;
                bytes += record_bytes(il2p_len(p, ld_rec(p, (int32_t)a.index)));
            });
        }
        if (out.status != PM_ROWS_PACKETS_FINISHED) {
            out.packets = out.corrected_left = 0;
            bytes = 0;
        }
        bytes_of[(size_t)j] = bytes;
        entries[(size_t)j] = out;
    }
    // ---- launch 2: one wave, a lane a job
    const int64_t capacity = room & ~(int64_t)7;
    int64_t incl_b[kWave], incl_p[kWave], run_b = 0, run_p = 0, kept_b = 0, kept_p = 0;
    int32_t handed = 0;
    for (int j = 0; j < njobs; ++j) {
        run_b += bytes_of[(size_t)j];
        run_p += entries[(size_t)j].packets;
        incl_b[j] = run_b;
        incl_p[j] = run_p;
    }
    for (int j = 0; j < njobs; ++j)
        if (!no_room(incl_b[j], capacity)) {
            if (incl_b[j] > kept_b) kept_b = incl_b[j];
            if (incl_p[j] > kept_p) kept_p = incl_p[j];
        }
    for (int j = 0; j < njobs; ++j) {
        pm_stream_packets_entry &e = entries[(size_t)j];
        const bool over = no_room(incl_b[j], capacity);
        if (over || e.status != PM_ROWS_PACKETS_FINISHED) ++handed;
        e.first_byte = over ? kept_b : incl_b[j] - bytes_of[(size_t)j];
        first[(size_t)j] = over ? kept_p : incl_p[j] - e.packets;
        if (over) {
            e.status = PM_ROWS_PACKETS_NO_ROOM;
            e.packets = e.corrected_left = 0;
        }
    }
    if (njobs != want_head.jobs || handed != want_head.handed || kept_p != want_head.packets || kept_b != want_head.bytes || want_head.reserved) fail(call, -1, "the head");
    for (int j = 0; j < njobs; ++j) {
        pm_stream_packets_entry w = want_entries[(size_t)j];
        w.lfsr_state = entries[(size_t)j].lfsr_state;      // (the model's blocks carry no register)
        if (memcmp(&w, &entries[(size_t)j], sizeof(w))) {
            printf("call %d job %d: entry {%d, %d, %lld, %d}, the model says {%d, %d, %lld, %d}\n", call, j, entries[(size_t)j].status, entries[(size_t)j].packets,
                   (long long)entries[(size_t)j].first_byte, entries[(size_t)j].corrected_left, w.status, w.packets, (long long)w.first_byte, w.corrected_left);
            ++bad;
        }
    }
    if (bad) return 1;
    // ---- launch 3: record by record, each into its own place of a buffer of exactly the kept bytes
    std::vector<uint8_t> records((size_t)kept_b, 0xEE);
    for (int64_t q = 0; q < kept_p; ++q) {
        const int j = row_of_packet([&](int i) { return first[(size_t)i]; }, njobs, q);
        const pm_stream_packets_entry &e = entries[(size_t)j];
        if (q < first[(size_t)j] || q >= first[(size_t)j] + e.packets) {
            fail(call, j, "the search for a record's job");
            continue;
        }
        const JobDesc &d = jobs[(size_t)j];
        const int64_t i = acc0[(size_t)j] + (q - first[(size_t)j]), at = e.first_byte + recoff[(size_t)i];
        const int64_t end = q + 1 < first[(size_t)j] + e.packets ? e.first_byte + recoff[(size_t)i + 1] : e.first_byte + bytes_of[(size_t)j];
        std::vector<uint8_t> one((size_t)(end - at), 0xEE);  // (its own buffer: a byte too many is the sanitizer's to find)
        record_build(part(j), d.kind, acc[(size_t)i], d.crc != 0, addrs[(size_t)j].data(), d.source, one.data());
        memcpy(records.data() + at, one.data(), one.size());
    }
    if (!records.empty() && memcmp(records.data(), want_records.data(), records.size())) fail(call, -1, "the records are not the model's");
    // ---- the host decoder on every finished stream
    for (int j = 0; j < njobs; ++j) {
        const pm_stream_packets_entry &e = entries[(size_t)j];
        const JobDesc &d = jobs[(size_t)j];
        if (e.status != PM_ROWS_PACKETS_FINISHED || d.kind < 0) continue;
        ++*finished_jobs;
        const Part p = part(j);
        pm_codec *codec = nullptr;
        if (pm_codec_create(d.kind, d.crc, d.disable_rs, d.min_dist, d.tol, d.source, &codec)) return 2;
        int64_t pending = 0, got = 0;
        if (pm_codec_decode(codec, p.plain, addrs[(size_t)j].data(), d.n, &pending)) return 2;
        std::vector<pm_packet> fetched((size_t)pending + 1);
        if (pm_codec_fetch(codec, fetched.data(), pending, &got)) return 2;
        pm_codec_destroy(codec);
        if (got != e.packets) {
            fail(call, j, "the host decoder finds another number of packets");
            continue;
        }
        int64_t at = e.first_byte;
        for (int64_t i = 0; i < got; ++i) {
            const pm_packet &w = fetched[(size_t)i];
            const int64_t size = record_bytes(w.len);
            if (at + size > kept_b || memcmp(&w, records.data() + at, (size_t)size)) fail(call, j, "pm_codec_fetch hands out another packet");
            at += size;
        }
        *decoded += got;
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
    printf("%d calls, %ld finished streams, %ld packets through the host decoder, %d bad\n", calls, finished, decoded, bad);
    return bad ? 1 : 0;
}
