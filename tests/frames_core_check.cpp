// bitscan_frames_kernel's trip (csrc/pm_bitscan.hip) with the wave's lanes stepped one after the other on the host: the per-word code is
// the kernel's own (csrc/pm_bitscan_frames.h), the scan over the lanes a loop, the line in LDS an array.  test_frames_core.py compiles
// this, feeds it streams with their events and the frames the bit-serial model finds, and expects every frame byte for byte.
//   frames_core_check <file> <words per trip>
//   file: int32 streams; per stream int32 n, n descrambled bytes, int32 events; per event int64 P, int64 F, int32 len (-1: closes nothing), bytes
#include "pm_bitscan_frames.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace pm_frames;

static uint64_t stream_word(const std::vector<uint8_t> &d, int64_t w)
{
    uint64_t v = 0;
    for (int i = 0; i < 64 && w >= 0; ++i) {
        const int64_t t = 64 * w + i;
        if (t / 8 < (int64_t)d.size() && ((d[(size_t)(t / 8)] >> (7 - (t & 7))) & 1)) v |= 1ull << i;
    }
    return v;
}

template <class T>
static T take(FILE *f)
{
    T v;
    if (fread(&v, sizeof(T), 1, f) != 1) exit(2);
    return v;
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    const int fw = atoi(argv[2]);
    if (!f || fw < 1 || fw > 64) return 2;
    constexpr int kLineWords = 136;
    uint16_t crc_table[256];
    for (unsigned v = 0; v < 256; ++v) crc_table[v] = (uint16_t)crc_times_x(v, 8);
    int bad = 0, total = 0;
    const int streams = take<int32_t>(f);
    for (int si = 0; si < streams; ++si) {
        const int32_t n = take<int32_t>(f);
        std::vector<uint8_t> d((size_t)n);
        if (n && fread(d.data(), 1, (size_t)n, f) != (size_t)n) return 2;
        const int32_t events = take<int32_t>(f);
        std::vector<int> owner((size_t)(n + 8), -1);        // which event wrote an area byte: frames must not overlap
        for (int e = 0; e < events; ++e) {
            const int64_t P = take<int64_t>(f), F = take<int64_t>(f);
            const int32_t want_len = take<int32_t>(f);
            std::vector<uint8_t> want((size_t)(want_len > 0 ? want_len : 0)), got;
            if (want_len > 0 && fread(want.data(), 1, want.size(), f) != want.size()) return 2;
            const int64_t s = F < 0 ? 0 : F, w_first = s >> 6, w_last = (P - 1) >> 6, at0 = s >> 3;
            State carry{0, 0};
            int64_t out = 0;
            uint32_t left = 0, line[kLineWords], crc = 0xFFFF, held0 = 0, held1 = 0;
            for (int64_t wt = w_first; wt <= w_last; wt += fw) {
                uint64_t x[64];
                WordMarks k[64];
                Span mine[64], before[64];
                State st[64];
                int32_t closes_at[64];
                uint64_t resets = 0;
                Span upto{0, 0, 0, 0};
                for (int l = 0; l < 64; ++l) {
                    const int64_t w = wt + l;
                    x[l] = 0;
                    k[l] = WordMarks{0, 0};
                    mine[l] = Span{0, 0, 0, 0};
                    if (l < fw && w <= w_last) {
                        x[l] = stream_word(d, w);
                        const uint64_t span = low_mask(w == w_last ? (int)((P - 1) & 63) + 1 : 64) & ~low_mask(w == w_first ? (int)(s & 63) : 0);
                        k[l] = word_marks(x[l], stream_word(d, w - 1), span);
                        mine[l] = word_span(k[l]);
                    }
                    before[l] = upto;
                    upto = join(upto, mine[l]);
                    st[l] = advance(carry, before[l]);
                    closes_at[l] = st[l].open + mine[l].a;
                    if (mine[l].r) resets |= 1ull << l;
                }
                const State next = advance(carry, upto);
                const int32_t head = closes_at[resets ? __builtin_ctzll(resets) : 0];
                const int sh = (int)((at0 + out) & 7);
                memset(line, 0, sizeof(line));
                if (left && !(resets && (head >> 3) == (carry.open >> 3))) line[sh >> 2] = left << (8 * (sh & 3));
                for (int l = 0; l < 64; ++l) {
                    const uint64_t behind = l < 63 ? resets & ~low_mask(l + 1) : 0;
                    put_word(x[l], k[l], st[l], 8 * ((int64_t)sh - out), behind ? closes_at[__builtin_ctzll(behind)] : kOpenEnded, [&](int at, uint32_t v) {
                        if (at < 0 || at >= kLineWords) {
                            printf("stream %d event %d: the line is written at word %d\n", si, e, at);
                            exit(1);
                        }
                        line[at] |= v;
                    });
                }
                const int64_t upto_bytes = next.bytes + (next.open >> 3);
                const int nb = (int)(upto_bytes - out);
                for (int q = sh; q < sh + nb; ++q) {
                    got.push_back((uint8_t)(line[q >> 2] >> (8 * (q & 3))));
                    int &o = owner[(size_t)(at0 + out + (q - sh))];
                    if (o >= 0 && o != e && want_len > 0) {
                        printf("stream %d event %d: byte %lld belongs to event %d\n", si, e, (long long)(at0 + out + (q - sh)), o);
                        ++bad;
                    }
                    if (want_len > 0) o = e;
                }
                {   // the CRC two bytes behind, the lanes' pieces joined as the kernel's shuffles join them
                    const int64_t lo = out > 2 ? out - 2 : 0, hi = upto_bytes > 2 ? upto_bytes - 2 : 0;
                    const int len = (int)(hi - lo), old = (int)(out - lo);
                    auto byte = [&](int k) -> uint32_t {
                        if (k < old) return k + 2 - old ? held1 : held0;
                        const int q = sh + (k - old);
                        return (line[q >> 2] >> (8 * (q & 3))) & 0xFF;
                    };
                    if (len == 1) {
                        crc = (crc >> 8) ^ crc_table[(crc ^ byte(0)) & 0xFF];
                    } else if (len >= 2) {
                        const int per = (len + 63) >> 6;
                        uint32_t piece[64], f = crc_times_x(0x8000u, 8 * per);
                        for (int l = 0; l < 64; ++l) piece[l] = crc_piece(crc_table, l, len, per, crc, byte);
                        for (int dl = 1; dl < 64; dl <<= 1) {
                            for (int l = 63; l >= dl; --l) piece[l] ^= crc_mul(f, piece[l - dl]);
                            f = crc_mul(f, f);
                        }
                        crc = piece[63];
                    }
                    if (nb >= 2) {
                        held0 = (line[(sh + nb - 2) >> 2] >> (8 * ((sh + nb - 2) & 3))) & 0xFF;
                        held1 = (line[(sh + nb - 1) >> 2] >> (8 * ((sh + nb - 1) & 3))) & 0xFF;
                    } else if (nb == 1) {
                        held0 = held1;
                        held1 = (line[sh >> 2] >> (8 * (sh & 3))) & 0xFF;
                    }
                }
                const int qe = sh + nb;
                left = (line[qe >> 2] >> (8 * (qe & 3))) & 0xFF & (uint32_t)low_mask(next.open & 7);
                out = upto_bytes;
                carry = next;
            }
            const bool closing = (carry.open & 7) == 7 && carry.open >= 8 * 18 + 7;
            ++total;
            if (closing != (want_len >= 0) || (closing && got != want)) {
                printf("stream %d event %d: closing %d with %zu bytes, the model has %d\n", si, e, (int)closing, got.size(), want_len);
                ++bad;
            } else if (closing) {
                uint32_t ref = 0xFFFF;                      // bit by bit over the model's frame less its last two bytes
                for (size_t k = 0; k + 2 < want.size(); ++k) ref = crc_times_x(ref ^ want[k], 8);
                if (ref != crc) {
                    printf("stream %d event %d: CRC register %04x, bit by bit %04x\n", si, e, crc, ref);
                    ++bad;
                }
            }
        }
    }
    printf("%d events, %d bad\n", total, bad);
    return bad != 0;
}
