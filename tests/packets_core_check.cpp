// bitscan_headers_kernel's and bitscan_blocks_kernel's trips (csrc/pm_bitscan.hip) with the wave's lanes stepped one after the other on the
// host: the per-lane code is the kernels' own (csrc/pm_il2p_core.h), the scans and ballots over the lanes are loops, LDS is arrays.
// test_packets_core.py compiles this and feeds it streams with their candidates and the records and area of the bit-serial model.
//   packets_core_check streams <file>
//       file: int32 streams; per stream int32 n, n descrambled bytes, int32 crc, disable_rs, min_dist, int32 candidates, uint32 at each (all of
//       the stream's, in order), int32 records, 16 bytes each, area bytes (n padded to 8), as many bytes of mask (1: a DONE record covers it)
//   packets_core_check random <blocks>
//       what the blocks launch restates for lanes -- the syndromes over segments, the Chien search a position at a time, the descrambler byte
//       by byte -- against the shared rs_decode and descramble and a bit-serial descrambler, on random blocks: lengths 17 .. 255, 0 .. 10
//       errors, 2 and 16 roots, min_dist 0 .. 2
#include "pm_il2p_core.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace pm_il2p;

static GF256 g;

template <class T>
static T take(FILE *f)
{
    T v;
    if (fread(&v, sizeof(T), 1, f) != 1) exit(2);
    return v;
}

static unsigned byte_at(const std::vector<uint8_t> &d, int64_t bit)
{
    unsigned v = 0;
    for (int i = 0; i < 8; ++i) {
        const int64_t t = bit + i;
        v = v << 1 | (t / 8 < (int64_t)d.size() ? (d[(size_t)(t / 8)] >> (7 - (t & 7))) & 1u : 0u);
    }
    return v;
}

// the wave's syndromes of buf[0 .. nb): every lane's share, XORed
static void wave_syndromes(const uint8_t *buf, int nb, int num_roots, int *syn)
{
    for (int i = 0; i < num_roots; ++i) syn[i] = 0;
    for (int lane = 0; lane < 64; ++lane) {
        int cnt = nb - 4 * lane;
        cnt = cnt < 0 ? 0 : cnt > 4 ? 4 : cnt;
        if (!cnt) continue;
        const int tail = nb - 4 * lane - cnt;
        for (int i = 0; i < num_roots; ++i) syn[i] ^= (int)syn_segment(&g, i, buf + 4 * lane, cnt, tail);
    }
}

// a block through the blocks launch's steps; the corrected count or -1
static int wave_rs(uint8_t *buf, int nb, int num_roots, int min_dist)
{
    int syn[16], loc[17], where[17] = {0};
    wave_syndromes(buf, nb, num_roots, syn);
    bool any = false;
    for (int i = 0; i < num_roots; ++i) any = any || syn[i];
    if (!any) return 0;
    rs_berlekamp(&g, num_roots, syn, loc);
    int fixed = 0;
    for (int t = 0; t < 4; ++t)
        for (int lane = 0; lane < 64; ++lane) {
            const int pos = 64 * t + lane;
            if (pos < nb && rs_chien_at(&g, num_roots, loc, nb, pos) == 0) {
                if (fixed < 17) where[fixed] = pos;
                ++fixed;
            }
        }
    if (fixed <= num_roots / 2 - min_dist) rs_forney(&g, num_roots, syn, loc, where, fixed, nb, buf);
    wave_syndromes(buf, nb, num_roots, syn);
    for (int i = 0; i < num_roots; ++i)
        if (syn[i]) return -1;
    return fixed;
}

static int check_streams(const char *path)
{
    FILE *f = fopen(path, "rb");
    if (!f) return 2;
    int bad = 0, total = 0;
    const int streams = take<int32_t>(f);
    for (int si = 0; si < streams; ++si) {
        const int32_t n = take<int32_t>(f);
        std::vector<uint8_t> d((size_t)n);
        if (n && fread(d.data(), 1, (size_t)n, f) != (size_t)n) return 2;
        Opts o;
        o.crc = take<int32_t>(f);
        o.disable_rs = take<int32_t>(f);
        o.min_dist = take<int32_t>(f);
        const int32_t ncand = take<int32_t>(f);
        std::vector<uint32_t> cands((size_t)ncand);
        for (auto &c : cands) c = take<uint32_t>(f);
        const int32_t nwant = take<int32_t>(f);
        std::vector<Rec> want((size_t)nwant);
        for (auto &r : want) r = take<Rec>(f);
        const size_t area_bytes = ((size_t)n + 7) / 8 * 8;
        std::vector<uint8_t> want_area(area_bytes), mask(area_bytes), area(area_bytes, 0xA5);
        if (area_bytes && (fread(want_area.data(), 1, area_bytes, f) != area_bytes || fread(mask.data(), 1, area_bytes, f) != area_bytes)) return 2;
        // ---- the headers launch
        const int64_t places = n / 64 + 2;
        const int32_t records = (int32_t)(ncand < places ? ncand : places);
        struct Copy {
            Rec r;
            uint8_t hdr[16];
        };
        std::vector<Copy> recs((size_t)records);
        std::vector<int32_t> work;
        std::vector<Rec> table((size_t)records, Rec{0xA5A5A5A5u, 0xA5A5A5A5u, 0xA5A5, 0xA5, 0xA5, 0xA5A5A5A5u});
        int64_t used = 0;
        bool full = false;
        for (int32_t r0 = 0; r0 < records; r0 += 64) {
            Copy pr[64];
            uint32_t need[64];
            for (int lane = 0; lane < 64; ++lane) {
                const int32_t e = r0 + lane;
                memset(&pr[lane], 0, sizeof(Copy));
                need[lane] = 0;
                if (e >= records) continue;
                const uint32_t at = cands[(size_t)e];
                const int64_t H = rec_H(at);
                pr[lane].r = rec_incomplete(at);
                if (H + kHeaderBits <= 8 * (int64_t)n) {
                    for (int q = 0; q < 15; ++q) pr[lane].hdr[q] = (uint8_t)byte_at(d, H + 8 * q);
                    pr[lane].r = header_attempt(&g, at, pr[lane].hdr, o, 8 * (int64_t)n);
                    if (pr[lane].r.status == kDone) need[lane] = rec_need(pr[lane].r.count);
                }
            }
            int first_over = 64;
            int64_t upto = 0;
            int64_t off[64];
            for (int lane = 0; lane < 64; ++lane) {
                off[lane] = used + upto;
                upto += need[lane];
                if (need[lane] && off[lane] + need[lane] > (int64_t)area_bytes && first_over == 64) first_over = lane;
            }
            for (int lane = 0; lane < 64; ++lane) {
                const int32_t e = r0 + lane;
                if (e >= records) continue;
                const bool placed = need[lane] && !full && lane < first_over;
                if (placed) pr[lane].r.off = (uint32_t)off[lane];
                else if (need[lane]) pr[lane].r = rec_not_placed(pr[lane].r);
                recs[(size_t)e] = pr[lane];
                if (placed && pr[lane].r.count > 0) {
                    work.push_back(e);
                } else {
                    table[(size_t)e] = pr[lane].r;
                    if (placed) {
                        for (int q = 0; q < 13; ++q) area[(size_t)off[lane] + q] = pr[lane].hdr[q];
                        for (int q = 13; q < 16; ++q) area[(size_t)off[lane] + q] = 0;
                    }
                }
            }
            used += upto;
            full = full || first_over < 64;
        }
        // ---- the blocks launch
        for (const int32_t e : work) {
            const Copy &pr = recs[(size_t)e];
            const int count = pr.r.count, need = (int)rec_need(count);
            const Split split = block_split(count);
            std::vector<uint8_t> pkt((size_t)need, 0);
            memcpy(pkt.data(), pr.hdr, 13);
            int corrected = pr.r.corrected, appended = 0;
            uint32_t end = kHeaderBits;
            bool fail = false;
            for (int b = 0; b < split.blocks && !fail; ++b) {
                const int bs = block_bytes(split, b), nb = bs + 16;
                uint8_t buf[256] = {0};
                for (int lane = 0; lane < 64; ++lane)
                    if (4 * lane < nb)
                        for (int q = 0; q < 4; ++q) buf[4 * lane + q] = (uint8_t)byte_at(d, rec_H(pr.r.at) + end + 32 * lane + 8 * q);
                const int fixed = o.disable_rs ? 0 : wave_rs(buf, nb, 16, o.min_dist > 9 ? 9 : o.min_dist < 0 ? 0 : o.min_dist);
                end += 8u * (uint32_t)nb;
                if (fixed < 0) {
                    fail = true;
                    break;
                }
                corrected += fixed;
                for (int k = 0; k < bs; ++k) pkt[(size_t)(13 + appended + k)] = (uint8_t)descramble_at(buf[k], k >= 1 ? buf[k - 1] : 0u, k >= 2 ? buf[k - 2] : 0u, k);
                appended += bs;
            }
            if (!fail) memcpy(area.data() + pr.r.off, pkt.data(), (size_t)need);
            table[(size_t)e] = Rec{pr.r.at, pr.r.off, (uint16_t)count, (uint8_t)(fail ? kBlockFail : kDone), (uint8_t)corrected, end};
        }
        // ---- against the model
        ++total;
        bool ok = records == nwant;
        for (int32_t e = 0; ok && e < records; ++e) ok = memcmp(&table[(size_t)e], &want[(size_t)e], sizeof(Rec)) == 0;
        for (size_t q = 0; ok && q < area_bytes; ++q) ok = mask[q] ? area[q] == want_area[q] : area[q] == 0xA5;
        if (!ok) {
            ++bad;
            printf("stream %d: %d records (model %d)\n", si, records, nwant);
            for (int32_t e = 0; e < records && e < nwant; ++e)
                if (memcmp(&table[(size_t)e], &want[(size_t)e], sizeof(Rec)))
                    printf("  record %d: at %u off %u count %d status %d corrected %d end %u, model at %u off %u count %d status %d corrected %d end %u\n", e, table[(size_t)e].at,
                           table[(size_t)e].off, table[(size_t)e].count, table[(size_t)e].status, table[(size_t)e].corrected, table[(size_t)e].end, want[(size_t)e].at, want[(size_t)e].off,
                           want[(size_t)e].count, want[(size_t)e].status, want[(size_t)e].corrected, want[(size_t)e].end);
        }
    }
    printf("%d streams, %d bad\n", total, bad);
    return bad != 0;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

static int check_random(int blocks)
{
    int bad = 0, failed = 0, corrected = 0;
    for (int v = 1; v < 256; ++v) bad += gf_mul(&g, v, g.inverse[v]) != 1;
    for (int a = 0; a < 256; ++a)
        for (int b = 0; b < 256; ++b) bad += (int)gf_mul_bits((unsigned)a, (unsigned)b) != gf_mul(&g, a, b);
    for (int t = 0; t < blocks; ++t) {
        const int num_roots = t & 1 ? 16 : 2, n = 17 + (int)(rnd() % 239), errors = (int)(rnd() % 11), min_dist = (int)(rnd() % 3);
        // a codeword: the data, and the remainder of data x^roots by the generator (x - table[0]) .. (x - table[roots - 1])
        int gen[17] = {1};
        for (int i = 0; i < num_roots; ++i) {
            for (int k = i + 1; k > 0; --k) gen[k] = gen[k - 1] ^ gf_mul(&g, gen[k], g.table[i]);
            gen[0] = gf_mul(&g, gen[0], g.table[i]);
        }
        uint8_t word[255];
        int rem[16] = {0};
        for (int j = 0; j < n - num_roots; ++j) {
            word[j] = (uint8_t)rnd();
            const int fb = word[j] ^ rem[num_roots - 1];
            for (int k = num_roots - 1; k > 0; --k) rem[k] = rem[k - 1] ^ gf_mul(&g, fb, gen[k]);
            rem[0] = gf_mul(&g, fb, gen[0]);
        }
        for (int k = 0; k < num_roots; ++k) word[n - 1 - k] = (uint8_t)rem[k];
        int syn[16], syn2[16];
        SerialSyndromes{&g, num_roots}(word, n, syn);
        for (int i = 0; i < num_roots; ++i) bad += syn[i] != 0;
        for (int e = 0; e < errors; ++e) word[rnd() % (unsigned)n] ^= (uint8_t)(1 + rnd() % 255);
        SerialSyndromes{&g, num_roots}(word, n, syn);
        wave_syndromes(word, n, num_roots, syn2);
        bad += memcmp(syn, syn2, sizeof(int) * (size_t)num_roots) != 0;
        uint8_t a[255], b[255];
        memcpy(a, word, (size_t)n);
        memcpy(b, word, (size_t)n);
        const int ra = rs_decode(&g, num_roots, a, n, min_dist, SerialSyndromes{&g, num_roots}), rb = wave_rs(b, n, num_roots, min_dist);
        if (ra != rb || (ra >= 0 && memcmp(a, b, (size_t)n))) {
            ++bad;
            printf("block %d: roots %d n %d errors %d min_dist %d: %d by the shared decoder, %d by lanes\n", t, num_roots, n, errors, min_dist, ra, rb);
        }
        failed += ra < 0;
        corrected += ra > 0;
        // the descrambler: the shared one, byte by byte as the lanes take it, and the reference's bit-serial loop
        uint8_t serial[255], lanes[255], shared[255];
        unsigned reg = 0x1F0, w = 0;
        for (int k = 0; k < n; ++k) {
            unsigned byte = word[k];
            for (int i = 0; i < 8; ++i) {
                w = (w << 1) & 0xFE;
                if (byte & 0x80) reg ^= 0x211;
                w |= reg & 1;
                byte <<= 1;
                reg >>= 1;
            }
            serial[k] = (uint8_t)w;
            lanes[k] = (uint8_t)descramble_at(word[k], k >= 1 ? word[k - 1] : 0u, k >= 2 ? word[k - 2] : 0u, k);
        }
        memcpy(shared, word, (size_t)n);
        descramble(shared, n);
        bad += memcmp(serial, lanes, (size_t)n) != 0 || memcmp(serial, shared, (size_t)n) != 0;
    }
    printf("%d blocks, %d corrected, %d failed, %d bad\n", blocks, corrected, failed, bad);
    return bad != 0;
}

int main(int argc, char **argv)
{
    gf_build(&g);
    if (argc == 3 && !strcmp(argv[1], "streams")) return check_streams(argv[2]);
    if (argc == 3 && !strcmp(argv[1], "random")) return check_random(atoi(argv[2]));
    return 2;
}
