// Finished packet rows from a row's scan part (pm_rows_packets, pm_bitscan.hip): the rules that say when the frame table or the packet table
// of a row of pm_rows_scan tells everything about the row, which packets it then holds, and what every field of their pm_packet rows is --
// exactly the rows pm_codec_fetch hands out for a just-created codec that is fed the row.  Plain C++ that compiles for the host and the
// device, free of LDS and launches: the walk launch runs a row's rule on a lane, the build launch restates packet_build for a wave, and
// tests/rows_packets_core_check.cpp steps all of it on the host against tests/rows_packets_model.py.
//   IL2P   Il2p::feed_search + take_record (pm_codec.cpp) for a just-created decoder, with "decode it by the machine" replaced by "hand
//          the row over": a hit of the register test without a record for exactly that place, or with an INCOMPLETE or NOT_PLACED one,
//          a second hit in the byte in which an attempt ends, a table that is full.
//   AX.25  Ax25::framed: every listed event with a frame is a packet (a frame longer than a row is cut as pm_codec_fetch cuts it); a row of
//          fewer than 24 bytes and a bail are handed over.
// pm_stream_packets (the job form, for pm_pipe) goes by the same rules: its walk launch gives a lane an AX.25 event (ax25_start, ax25_event)
// and runs il2p_walk as it stands, its records are packet_build_to's with the stream's own addresses and a dense output
// (tests/stream_packets_core_check.cpp steps that on the host against tests/stream_packets_model.py).
// A part lies in device memory at a multiple of 8, and so does every piece of it: words are loaded as words.
#pragma once
#include <stdint.h>
#include "../../include/pymodem_amd.h"
#include "pm_bitscan_addrs.h"
#include "pm_bitscan_rows.h"
#include "pm_il2p_core.h"

#if defined(__HIPCC__)
#define PM_RPK_HD __host__ __device__ inline
#else
#define PM_RPK_HD inline
#endif

namespace pm_rpk {

constexpr int kEntryBytes = 32, kHeadBytes = 16, kStreamHeadBytes = 32;
static_assert(sizeof(pm_rows_packets_entry) == kEntryBytes && sizeof(pm_rows_packets_head) == kHeadBytes && sizeof(pm_packet) % 8 == 0, "the layout of d_out");
static_assert(sizeof(pm_stream_packets_entry) == kEntryBytes && sizeof(pm_stream_packets_head) == kStreamHeadBytes, "the layout of pm_stream_packets' d_out");

// what a row's walk accepts: IL2P -- the record, the last bit of the attempt's last block (the CRC bytes begin behind it; below 2^32 as
// every bit of a stream is), the decoder's count of corrected bytes when the packet is queued; AX.25 -- the event, the flag's bit P, 0
struct Accepted {
    uint32_t index, bit;
    int32_t corrected, reserved;
};

// the pieces of a row's scan part (what pm_rows_scan writes behind the row's steps)
struct Part {
    const uint8_t *rec, *list, *plain, *table, *area;
    const int64_t *addrs;
    int64_t n;
};
PM_RPK_HD Part part_of(const uint8_t *scan, int kind, int64_t n)
{
    Part p;
    p.rec = scan;
    p.list = scan + pm_rows::kHead;
    p.plain = p.list + pm_rows::list_bytes(kind, n);
    p.table = p.plain + pm_rows::pad8(n);
    p.area = p.table + (kind == 0 ? 8 * (n / 19 + 2) : 16 + 16 * (n / 64 + 2));
    p.addrs = reinterpret_cast<const int64_t *>(p.area + pm_rows::pad8(n));
    p.n = n;
    return p;
}
PM_RPK_HD uint32_t ld32(const uint8_t *p) { return *reinterpret_cast<const uint32_t *>(p); }
PM_RPK_HD uint64_t ld64(const uint8_t *p) { return *reinterpret_cast<const uint64_t *>(p); }
PM_RPK_HD pm_il2p::Rec ld_rec(const Part &p, int32_t i)
{
    const uint64_t a = ld64(p.table + 16 + 16 * (int64_t)i), b = ld64(p.table + 24 + 16 * (int64_t)i);
    return pm_il2p::Rec{(uint32_t)a, (uint32_t)(a >> 32), (uint16_t)b, (uint8_t)(b >> 16), (uint8_t)(b >> 24), (uint32_t)(b >> 32)};
}
// the eight bits from stream bit `bit` on, the first on top (bit + 8 <= 8 n)
PM_RPK_HD unsigned byte_at(const uint8_t *d, int64_t bit)
{
    const int s = (int)(bit & 7);
    const unsigned v = d[bit >> 3];
    return s ? ((v << s) | ((unsigned)d[(bit >> 3) + 1] >> (8 - s))) & 0xFF : v;
}
PM_RPK_HD bool sync_hit(uint32_t w, int tol)
{
    return __builtin_popcount((w & 0xFFFFFFu) ^ 0xF15E48u) <= tol || __builtin_popcount(w ^ 0x5D57DF7Fu) <= tol;       // il2p.py:367-376
}
// first set bit of the candidate bitmap at or behind byte k, n if there is none
PM_RPK_HD int64_t next_candidate(const uint8_t *list, int64_t k, int64_t n)
{
    while (k < n) {
        const uint64_t w = ld64(list + 8 * (k >> 6)) >> (k & 63);
        if (w) {
            const int64_t j = k + __builtin_ctzll(w);
            return j < n ? j : n;
        }
        k = (k | 63) + 1;
    }
    return n;
}

// The IL2P rule.  emit(i, Accepted): the row's packet i.  Returns the status; *packets and *corrected_left (the decoder's count of corrected
// bytes behind the row's last byte) mean something for PM_ROWS_PACKETS_FINISHED only.
template <class Emit>
PM_RPK_HD int32_t il2p_walk(const Part &p, int tol, bool crc, int32_t *packets, int32_t *corrected_left, Emit emit)
{
    using namespace pm_il2p;
    const int64_t n = p.n, places = n / 64 + 2;
    *packets = 0;
    *corrected_left = 0;
    const int32_t said = (int32_t)ld32(p.table);
    if (said < 0 || said >= places) return PM_ROWS_PACKETS_TABLE_FULL;
    const int32_t records = said;
    const uint8_t *d = p.plain;
    uint32_t word = 0xFFFFFF;                               // il2p.py:120
    int32_t corrected = 0, cursor = 0, count = 0;
    int run = 0;                                            // whole bytes of this search, up to four: then the register is the input's last 32 bits
    for (int64_t k = 0; k < n; ++k) {
        if (run >= 4 && k >= 4) {
            const int64_t j = next_candidate(p.list, k, n);
            if (j >= n) break;
            if (j > k) {
                word = (uint32_t)d[j - 4] << 24 | (uint32_t)d[j - 3] << 16 | (uint32_t)d[j - 2] << 8 | d[j - 1];
                k = j;
            }
        }
        const uint64_t win = (uint64_t)word << 8 | d[k];
        if (run < 4) ++run;
        int S = 0;
        while (S < 8 && !sync_hit((uint32_t)(win >> (7 - S)), tol)) ++S;
        if (S == 8) {
            word = (uint32_t)win;
            continue;
        }
        const uint32_t at = (uint32_t)(k << 3) | (uint32_t)S;
        Rec r = rec_incomplete(0);
        for (; cursor < records; ++cursor) {
            r = ld_rec(p, cursor);
            if ((int64_t)(r.at >> 3) >= k) break;
        }
        if (cursor >= records || r.at != at) return PM_ROWS_PACKETS_NO_RECORD;
        if (r.status == kIncomplete) return PM_ROWS_PACKETS_INCOMPLETE;
        if (r.status == kNotPlaced) return PM_ROWS_PACKETS_NOT_PLACED;
        int64_t E = 8 * k + S + 1 + (r.status == kHeaderFail ? (int64_t)kHeaderBits : (int64_t)r.end);
        // (a record that cannot belong to the stream -- pm_codec_decode_packets refuses such a table -- is no record: nothing is read past the part)
        if (r.status > kNotPlaced || r.count > 1023 || E + (crc && r.status == kDone ? 32 : 0) > 8 * n) return PM_ROWS_PACKETS_NO_RECORD;
        if (r.status == kDone && ((r.off & 7) || (int64_t)r.off + rec_need(r.count) > pm_rows::pad8(n))) return PM_ROWS_PACKETS_NO_RECORD;
        if (r.status != kHeaderFail) corrected += r.corrected;
        if (r.status == kDone) {
            emit(count++, Accepted{(uint32_t)cursor, (uint32_t)(E - 1), corrected, 0});
            corrected = 0;
            if (crc) E += 32;
        }
        const int64_t ke = (E - 1) >> 3;
        word = byte_at(d, E - 8);
        for (int64_t b = E; b < 8 * (ke + 1); ++b) {        // the rest of the byte in which the attempt ends, through the register
            word = word << 1 | ((d[ke] >> (7 - (int)(b & 7))) & 1u);
            if (sync_hit(word, tol)) return PM_ROWS_PACKETS_LATE_HIT;
        }
        run = 0;
        k = ke;
    }
    *packets = count;
    *corrected_left = corrected;
    return PM_ROWS_PACKETS_FINISHED;
}

// The AX.25 rule, in the two steps that a walk of any shape takes: what the stream as a whole says (FINISHED: go on, with `events` listed
// events to look at), and what one listed event says -- a packet or none, its flag's bit P and its frame's bytes, or a table that cannot be
// the stream's.  ax25_walk below takes the events one after the other; pm_stream_packets' walk launch gives a lane an event.
struct Ax25Event {
    bool take, bad;
    uint32_t P;
    int32_t len;
};
PM_RPK_HD int32_t ax25_start(const Part &p, int32_t *events)
{
    const int64_t n = p.n, places = n / 19 + 2;
    *events = 0;
    if (n < 24) return PM_ROWS_PACKETS_SHORT;
    if ((int64_t)ld64(p.rec + 8) >= 0) return PM_ROWS_PACKETS_BAIL;
    const int32_t said = (int32_t)ld32(p.rec + 24);
    *events = said > places ? (int32_t)places : said;
    return PM_ROWS_PACKETS_FINISHED;
}
PM_RPK_HD Ax25Event ax25_event(const Part &p, int32_t e)
{
    Ax25Event ev{false, false, 0, (int32_t)ld32(p.table + 8 * (int64_t)e)};
    if (ev.len > 0) {
        // (a frame longer than the span between its flags cannot belong to the stream -- pm_codec_decode_framed refuses such a table -- and
        // hands the row over: nothing is read past the part)
        const uint32_t P = ld32(p.list + 8 * (int64_t)e), F = ld32(p.list + 8 * (int64_t)e + 4);
        const int64_t from = F == 0xFFFFFFFFu ? 0 : (int64_t)F;
        ev.P = P;
        ev.bad = (int64_t)(P >> 3) >= p.n || from > (int64_t)P || ev.len > ((int64_t)P - from) / 8;
        ev.take = !ev.bad;
    }
    return ev;
}
template <class Emit>
PM_RPK_HD int32_t ax25_walk(const Part &p, int32_t *packets, Emit emit)
{
    *packets = 0;
    int32_t events, count = 0;
    if (const int32_t status = ax25_start(p, &events)) return status;
    for (int32_t e = 0; e < events; ++e) {
        const Ax25Event ev = ax25_event(p, e);
        if (ev.bad) return PM_ROWS_PACKETS_LONG_FRAME;
        if (ev.take) emit(count++, Accepted{(uint32_t)e, ev.P, 0, 0});
    }
    *packets = count;
    return PM_ROWS_PACKETS_FINISHED;
}

// ---- the dense form (pm_stream_packets): a record is the 40-byte head and the packet's bytes, padded with zeros to a multiple of 8
PM_RPK_HD int32_t record_bytes(int32_t len) { return 40 + (int32_t)pm_rows::pad8(len < PM_PKT_MAX ? len : PM_PKT_MAX); }
// the bytes of the packet that IL2P record `r` of a part stands for: the rebuilt AX.25 header, the payload, the two CRC bytes
PM_RPK_HD int32_t il2p_len(const Part &p, const pm_il2p::Rec &r) { return pm_il2p::ax25_header_len(p.area + r.off) + (int32_t)r.count + 2; }
// a lane's place among the lanes of a ballot that are set in front of it
PM_RPK_HD int lanes_before(uint64_t ballot, int lane) { return __builtin_popcountll(ballot & (((uint64_t)1 << lane) - 1)); }

// ---- room: rows take their places in row order; the first whose packets would pass the capacity takes none, nor does any row behind it.
// incl: the packets of rows 0 .. r as the walks counted them (a sum that only grows, so "passes" stays true from the first such row on)
PM_RPK_HD bool no_room(int64_t incl, int64_t capacity) { return incl > capacity; }
// the row of packet p: the last row whose `first` is not behind it (rows without packets share the next row's; NO_ROOM rows lie at the total)
template <class First>
PM_RPK_HD int row_of_packet(First first, int nrows, int64_t p)
{
    int lo = 0, hi = nrows - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (first(mid) <= p) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// ---- a packet's fields (packet_meta.py:197-208, 21-41; pm_codec.cpp: finalize) -----------------------------------------------------
// crc_functions.py:44-55 bit by bit
PM_RPK_HD int crc16(const uint8_t *d, int64_t n)
{
    unsigned crc = 0xFFFF;
    for (int64_t k = 0; k < n; ++k) {
        crc ^= d[k];
        for (int i = 0; i < 8; ++i) crc = (crc & 1) ? (crc >> 1) ^ 0x8408u : crc >> 1;
    }
    return (int)(crc ^ 0xFFFF);
}
// packet_meta.py:21-41.  The loop there never resets its sub-field index, so only bytes 0..6 are examined.
PM_RPK_HD bool valid_header(const uint8_t *d, int len)
{
    if (len <= 15) return false;
    for (int k = 0; k < 7; ++k) {
        const int ch = d[k] >> 1;
        if ((ch < 32 || ch > 126) && ch != 0) return false;
    }
    return true;
}
// the 40 bytes in front of a row's data, as five words: d the row's bytes, len how many; calculated: the CRC of the packet less its last two
// bytes, carried: what those two say (a frame longer than a row: the whole frame's, as pm_codec_fetch has them)
struct HeadWords {
    uint64_t w[5];
};
PM_RPK_HD HeadWords head_words(int64_t addr, const uint8_t *d, int len, int corrected, int calculated, uint32_t carried, int source)
{
    const uint32_t valid_crc = carried == (uint32_t)calculated, header = valid_header(d, len);
    return HeadWords{{(uint64_t)addr, (uint64_t)(uint32_t)len | (uint64_t)(uint32_t)corrected << 32, (uint64_t)(uint32_t)calculated | (uint64_t)carried << 32,
                      (uint64_t)valid_crc | (uint64_t)header << 32, (uint64_t)(uint32_t)source}};
}

// One packet, whole, by one thread: what the build launch makes with a wave.  addr_of(k): the stream address of data byte k; data_bytes(len):
// how many bytes follow the 40 of the head in `out`, every one written (zeros behind the packet).
template <class AddrOf, class DataBytes>
PM_RPK_HD void packet_build_to(const Part &p, int kind, const Accepted &a, bool crc, AddrOf addr_of, DataBytes data_bytes, int source, uint8_t *out)
{
    uint8_t *data = out + 40;
    int len, calculated, corrected = a.corrected;
    uint32_t carried;
    int64_t k;
    if (kind == 1) {
        const pm_il2p::Rec r = ld_rec(p, (int32_t)a.index);
        const uint8_t *src = p.area + r.off;
        const int hl = pm_il2p::ax25_header(src, data);
        for (int q = 0; q < r.count; ++q) data[hl + q] = src[13 + q];
        len = hl + r.count + 2;
        calculated = crc16(data, len - 2);
        int64_t E = (int64_t)a.bit + 1;
        carried = (uint32_t)calculated;                     // il2p.py:427-431: without the trailing CRC the computed one is appended
        if (crc) {
            carried = (uint32_t)pm_il2p::hamming_crc(byte_at(p.plain, E), byte_at(p.plain, E + 8), byte_at(p.plain, E + 16), byte_at(p.plain, E + 24));
            E += 32;
        }
        data[len - 2] = (uint8_t)(carried & 0xFF);
        data[len - 1] = (uint8_t)(carried >> 8);
        k = (E - 1) >> 3;
    } else {
        const uint32_t F = ld32(p.list + 8 * (int64_t)a.index + 4);
        const int64_t at = F == 0xFFFFFFFFu ? 0 : (int64_t)(F >> 3);
        const int whole = (int32_t)ld32(p.table + 8 * (int64_t)a.index);
        len = whole < PM_PKT_MAX ? whole : PM_PKT_MAX;      // ax25.py:41-47 can close a frame of any length: the row keeps its first bytes
        calculated = (int)ld32(p.table + 8 * (int64_t)a.index + 4);
        carried = (uint32_t)p.area[at + whole - 1] * 256u + p.area[at + whole - 2];
        for (int q = 0; q < len; ++q) data[q] = p.area[at + q];
        k = (int64_t)(a.bit >> 3);
    }
    for (int q = len, end = data_bytes(len); q < end; ++q) data[q] = 0;
    const HeadWords h = head_words(addr_of(k), data, len, corrected, calculated, carried, source);
    for (int q = 0; q < 5; ++q)
        for (int i = 0; i < 8; ++i) out[8 * q + i] = (uint8_t)(h.w[q] >> (8 * i));
}
// the row form: a whole pm_packet (sizeof(pm_packet) bytes), the address from the part's checkpoints and the row's 16-bit steps
PM_RPK_HD void packet_build(const Part &p, int kind, const Accepted &a, bool crc, const uint16_t *steps, int source, uint8_t *out)
{
    packet_build_to(p, kind, a, crc, [&p, steps](int64_t k) { return pm_addrs::resolve(p.addrs, steps, k); }, [](int) { return (int)PM_PKT_MAX; }, source, out);
}
// the dense form: a record of record_bytes(len) bytes, the address the stream's own (pm_scan_job.d_addr: no checkpoints, no steps)
PM_RPK_HD void record_build(const Part &p, int kind, const Accepted &a, bool crc, const int64_t *addr, int source, uint8_t *out)
{
    packet_build_to(p, kind, a, crc, [addr](int64_t k) { return addr[k]; }, [](int len) { return (int)pm_rows::pad8(len); }, source, out);
}

}  // namespace pm_rpk
