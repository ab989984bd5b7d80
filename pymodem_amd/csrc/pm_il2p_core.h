// What an IL2P decoder does behind a sync word, in the pieces that the host decoder (pm_codec.cpp) and pm_stream_scan's packets launches
// (pm_bitscan.hip) share: GF(2^8), the Reed-Solomon decoder of rs_functions.py:33-150, the descrambler of il2p.py:160-163, the header's
// payload count and the block split of il2p.py:346-358, the AX.25 header that a decoded IL2P header stands for (il2p.py:214-344) and the
// Hamming(7,4) table of the trailing CRC (for the host decoder and pm_rows_packets' build launch), and the record of an ATTEMPT -- what Il2p::feed_bits does from the bit H at which
// it enters kHeader until it is back in kSync, which depends on nothing but the descrambled bits from H on and the codec's options.
// Compiles for the host and the device; the tables come through a pointer (an object on the host, LDS on the device).  The serial parts
// (Berlekamp, Forney, the serial Chien search and syndromes) are the host's own statements; what the blocks launch restates for lanes --
// syndromes over segments joined with powers of the root, the Chien search a position at a time, the descrambler as
// out[t] = in[t] ^ in[t - 4] ^ in[t - 9] plus the preset's share of the first nine bits -- is held to them by tests/packets_core_check.cpp.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PM_IL2P_HD __host__ __device__
#else
#define PM_IL2P_HD
#endif

namespace pm_il2p {

// ---- GF(2^8) -------------------------------------------------------------------------------------
// gf_functions.py:47-74 fills its table with a Galois LFSR stepped down from a^0 with 0x11D: table[i] is x^i in the polynomial basis
// modulo x^8 + x^4 + x^3 + x^2 + 1, index its logarithm, and the product of the reference is the ordinary one of that field.
struct GF256 {
    uint8_t table[256], index[256], inverse[256];           // table[255] repeats table[0]; index[0] and inverse[0] are 0
};

PM_IL2P_HD inline void gf_build(GF256 *g)
{
    unsigned reg = 1;
    for (int i = 0; i < 256; ++i) g->index[i] = 0;
    for (int i = 254; i >= 0; --i) {
        const unsigned fb = reg & 1;
        reg >>= 1;
        if (fb) reg ^= 0x11D >> 1;
        g->table[i] = (uint8_t)reg;
        g->index[reg] = (uint8_t)i;
    }
    g->table[255] = g->table[0];
    g->inverse[0] = 0;
    for (int i = 1; i < 256; ++i) g->inverse[i] = g->table[(255 - g->index[i]) % 255];      // the one j with mul(i, j) == 1
}

PM_IL2P_HD inline int gf_mul(const GF256 *g, int a, int b)
{
    if (a == 0 || b == 0) return 0;
    int r = g->index[a] + g->index[b];
    if (r > 254) r -= 255;
    return g->table[r];
}

// the same product without a table: eight shifted copies of a, reduced as they go (for lanes, whose unrelated addresses would collide in LDS)
PM_IL2P_HD inline unsigned gf_mul_bits(unsigned a, unsigned b)
{
    unsigned r = 0;
    for (int k = 0; k < 8; ++k) {
        r ^= (0u - ((b >> k) & 1u)) & a;
        a = (a << 1) ^ ((0u - (a >> 7)) & 0x11Du);
    }
    return r & 0xFF;
}

PM_IL2P_HD inline int wrap255(int x)
{
    while (x > 254) x -= 255;
    return x;
}

// ---- Reed-Solomon, rs_functions.py:33-150 (first_root is 0 for both IL2P codes) ------------------------------------------------
// Berlekamp: the locator loc[0 .. num_roots / 2] from the syndromes (loc must hold 17)
PM_IL2P_HD inline void rs_berlekamp(const GF256 *g, int num_roots, const int *syn, int *loc)
{
    const int half = num_roots / 2;
    int nxt[17] = {0}, corr[18] = {0};
    for (int i = 0; i < 17; ++i) loc[i] = 0;
    loc[0] = 1;
    corr[1] = 1;
    int order = 0;
    for (int step = 1; step <= num_roots; ++step) {
        const int y = step - 1;
        int e = syn[y];
        for (int i = 1; i <= order; ++i) e ^= gf_mul(g, loc[i], syn[y - i]);
        if (e != 0) {
            for (int i = 0; i <= order; ++i) nxt[i] = loc[i] ^ gf_mul(g, e, corr[i]);
            e = g->inverse[e];
            for (int i = 0; i <= half; ++i) corr[i] = gf_mul(g, loc[i], e);
            for (int i = 0; i <= half; ++i) loc[i] = nxt[i];
        }
        if (2 * order < step) order = step - order;
        for (int i = num_roots; i > 0; --i) corr[i] = corr[i - 1];
        corr[0] = 0;
    }
}

// Chien search over all n positions.  The exponent of term i at position j is ((j + 256 - n) i + index[loc[i]]) mod 255: kept per term and
// advanced by i from one position to the next.  where (17 places) takes the first 17 roots; returns how many there are.
PM_IL2P_HD inline int rs_chien(const GF256 *g, int num_roots, const int *loc, int n, int *where)
{
    const int half = num_roots / 2;
    int count = 0, ex[9], ni = 0, which[9];
    for (int i = 1; i <= half; ++i)
        if (loc[i]) {
            ex[ni] = wrap255((256 - n) * i + g->index[loc[i]]);
            which[ni++] = i;
        }
    for (int j = 0; j < n; ++j) {
        int x = 0;
        for (int k = 0; k < ni; ++k) {
            x ^= g->table[ex[k]];
            ex[k] += which[k];
            if (ex[k] > 254) ex[k] -= 255;
        }
        x ^= loc[0];
        if (x == 0) {
            if (count < 17) where[count] = j;
            ++count;
        }
    }
    return count;
}

// the same for one position: the locator's value at position j (a root where it is 0)
PM_IL2P_HD inline int rs_chien_at(const GF256 *g, int num_roots, const int *loc, int n, int j)
{
    int x = loc[0];
    for (int i = 1; i <= num_roots / 2; ++i)
        if (loc[i]) x ^= g->table[((j + 256 - n) * i + g->index[loc[i]]) % 255];
    return x;
}

// Forney: the error values at the `count` roots, applied to buf
PM_IL2P_HD inline void rs_forney(const GF256 *g, int num_roots, const int *syn, const int *loc, const int *where, int count, int n, uint8_t *buf)
{
    const int half = num_roots / 2;
    int corr[18] = {0};
    for (int i = 0; i < count; ++i) {
        corr[i] = syn[i];
        for (int j = 1; j <= i; ++j) corr[i] ^= gf_mul(g, syn[i - j], loc[j]);
    }
    for (int i = 0; i < count; ++i) {
        const int e = n - where[i] - 1;
        int z = corr[0];
        for (int j = 1; j < count; ++j) {
            int x = wrap255(e * j);
            x = wrap255(256 - x - 1);
            z ^= gf_mul(g, corr[j], g->table[x]);
        }
        z = gf_mul(g, z, g->table[e]);
        int y = loc[1];
        for (int j = 3; j <= half; j += 2) {
            int x = wrap255(e * (j - 1));
            x = wrap255(256 - x - 1);
            y ^= gf_mul(g, loc[j], g->table[x]);
        }
        y = g->index[y];
        y = 256 - y - 1;
        if (y == 255) y = 0;
        y = g->table[y];
        buf[where[i]] ^= (uint8_t)gf_mul(g, y, z);
    }
}

// Horner in root i over buf[0 .. n), one root after the other (the host has a faster one, pm_codec.cpp)
struct SerialSyndromes {
    const GF256 *g;
    int num_roots;
    PM_IL2P_HD void operator()(const uint8_t *buf, int n, int *syn) const
    {
        for (int i = 0; i < num_roots; ++i) {
            const int x = g->table[i];
            int v = 0;
            for (int j = 0; j < n - 1; ++j) v = gf_mul(g, v ^ buf[j], x);
            syn[i] = v ^ buf[n - 1];
        }
    }
};

// Corrects buf[0 .. n) in place; the corrected count, or -1 (the buffer is then not to be looked at).  syndromes(buf, n, syn) fills syn[0 .. num_roots).
template <class Syn>
PM_IL2P_HD inline int rs_decode(const GF256 *g, int num_roots, uint8_t *buf, int n, int min_distance, const Syn &syndromes)
{
    const int half = num_roots / 2;
    int syn[16];
    syndromes(buf, n, syn);
    {
        // All syndromes zero: the locator stays {1}, the Chien search finds no root (x = loc[0] = 1), nothing is corrected and
        // the closing check passes -- the reference's algorithm returns 0 with the data untouched.  Skip straight there.
        bool clean = true;
        for (int i = 0; i < num_roots; ++i) clean &= syn[i] == 0;
        if (clean) return 0;
    }
    int loc[17], where[17] = {0};
    rs_berlekamp(g, num_roots, syn, loc);
    const int count = rs_chien(g, num_roots, loc, n, where);
    if (count <= half - min_distance) rs_forney(g, num_roots, syn, loc, where, count, n, buf);
    syndromes(buf, n, syn);
    for (int i = 0; i < num_roots; ++i)
        if (syn[i] != 0) return -1;
    return count;
}

// A lane's share of syndrome i: its `cnt` bytes seg[0 .. cnt) with `tail` bytes of the block behind them.  The syndrome is the sum over
// the bytes of buf[j] r^(n - 1 - j) with r = table[i]: Horner inside the segment, then r^tail = table[i tail mod 255].  XOR over the
// segments gives SerialSyndromes' value.
PM_IL2P_HD inline unsigned syn_segment(const GF256 *g, int i, const uint8_t *seg, int cnt, int tail)
{
    const unsigned r = g->table[i];
    unsigned v = 0;
    for (int q = 0; q < cnt; ++q) v = gf_mul_bits(v, r) ^ seg[q];
    return gf_mul_bits(v, g->table[(i * tail) % 255]);
}

// ---- the descrambler, il2p.py:160-163 with lfsr.py:54-92: x^9 + x^4 + 1 (0x211), register preset 0x1F0 ----------------------------
// Byte k of the output from bytes k, k - 1, k - 2 of the input (zero in front of the block): output bit t is in[t] ^ in[t - 4] ^ in[t - 9],
// and the preset puts a one under bits 4 .. 8.
PM_IL2P_HD inline unsigned descramble_at(unsigned in, unsigned prev1, unsigned prev2, int k)
{
    const unsigned w = (prev2 << 16) | (prev1 << 8) | in;
    return ((w ^ (w >> 4) ^ (w >> 9)) & 0xFF) ^ (k == 0 ? 0x0Fu : k == 1 ? 0x80u : 0u);
}

PM_IL2P_HD inline void descramble(uint8_t *p, int n)
{
    for (int k = n - 1; k >= 0; --k) p[k] = (uint8_t)descramble_at(p[k], k >= 1 ? p[k - 1] : 0u, k >= 2 ? p[k - 2] : 0u, k);     // from the back: in place
}

// ---- the header and the block split -----------------------------------------------------------------------------------------------
PM_IL2P_HD inline int header_count(const uint8_t *b)        // il2p.py:214-290, the payload byte count of 13 descrambled header bytes
{
    int count = 0;
    for (int i = 0; i < 10; ++i)
        if (b[i + 2] & 0x80) count |= 0x200 >> i;
    return count;
}

// the fields of the 13 descrambled header bytes that decide how long the AX.25 header is: ax25_header and ax25_header_len share them
PM_IL2P_HD inline int header_type(const uint8_t *b) { return (b[1] & 0x80) >> 7; }
PM_IL2P_HD inline int header_pid(const uint8_t *b)
{
    int pid = 0;
    for (int i = 0; i < 4; ++i)
        if (b[i + 1] & 0x40) pid |= 0x8 >> i;
    return pid;
}
PM_IL2P_HD inline unsigned header_pid_byte(int pid)
{
    // {0, 0, 0x10, 0x01, 0x06, 0x07, 0x08, 0xC3, 0xC4, 0xCA, 0xCB, 0xCC, 0xCD, 0xCE, 0xCF, 0xF0}
    return (unsigned)((pid < 8 ? 0xC308070601100000ull : 0xF0CFCECDCCCBCAC4ull) >> (8 * (pid & 7))) & 0xFF;
}
// how many bytes ax25_header makes of the 13 header bytes, without making them: two addresses and the control byte, and the PID byte of
// the types that have one
PM_IL2P_HD inline int ax25_header_len(const uint8_t *b) { return header_type(b) != 1 ? 0 : 15 + (header_pid_byte(header_pid(b)) != 0); }
// il2p.py:214-344: the AX.25 header that the 13 descrambled header bytes stand for, into out (16 bytes at the most); returns how many.
// Type 0 is transparent encapsulation: nothing.  The two small tables are packed into words, a byte an entry: no table in memory.
PM_IL2P_HD inline int ax25_header(const uint8_t *b, uint8_t *out)
{
    const int type = header_type(b), pid = header_pid(b);
    int ctl = 0;
    for (int i = 0; i < 7; ++i)
        if (b[i + 5] & 0x40) ctl |= 0x40 >> i;
    enum { UI, S, U, I } kind = (b[0] & 0x40) ? UI : (pid == 0 ? S : (pid == 1 ? U : I));
    const unsigned pid_byte = header_pid_byte(pid);
    const bool pf = ctl & 0x40;
    bool cbit = false;
    int nr = 0, ns = 0, op = 0;
    if (kind == I) {
        ns = ctl & 0x7;
        nr = (ctl >> 3) & 0x7;
        cbit = true;
    } else if (kind == S) {
        nr = (ctl >> 3) & 0x7;
        cbit = ctl & 0x4;
        op = ctl & 0x3;
    } else {
        cbit = ctl & 0x4;
        op = (ctl >> 3) & 0x7;
    }
    if (type != 1) return 0;
    int at = 0;                                             // il2p.py:292-340
    for (int i = 0; i < 6; ++i) out[at++] = (uint8_t)(((b[i] & 0x3F) + 0x20) << 1);
    out[at++] = (uint8_t)(((b[12] >> 4) << 1) + 0x60 + (cbit ? 0x80 : 0));
    for (int i = 0; i < 6; ++i) out[at++] = (uint8_t)(((b[i + 6] & 0x3F) + 0x20) << 1);
    out[at++] = (uint8_t)(((b[12] & 0xF) << 1) + 0x60 + (cbit ? 0 : 0x80) + 1);
    int cb;
    // {0x2F, 0x43, 0x0F, 0x63, 0x87, 0x03, 0xAF, 0xE3}
    if (kind == U || kind == UI) cb = (int)((0xE3AF0387630F432Full >> (8 * op)) & 0xFF) | (pf ? 0x10 : 0);
    else if (kind == S) cb = 0x1 | (op << 2) | (nr << 5) | (pf ? 0x10 : 0);
    else cb = (ns << 1) | (nr << 5) | (pf ? 0x10 : 0);
    out[at++] = (uint8_t)cb;
    if (pid_byte != 0) out[at++] = (uint8_t)pid_byte;
    return at;
}

// il2p.py:23-40, the Hamming(7,4) decode table: 128 entries of four bits, sixteen to a word
PM_IL2P_HD inline unsigned hamming74(unsigned v)
{
    v &= 0x7F;
    const unsigned q = v >> 4;
    const uint64_t w = q == 0 ? 0xEEDEBE907E503000ull : q == 1 ? 0xDEDD3AD836D43330ull : q == 2 ? 0xBE5CBBB85655B250ull : q == 3 ? 0xF6D8B88866563618ull
                     : q == 4 ? 0x7E9C9A9977747290ull : q == 5 ? 0xFAD4AA9A74443A14ull : q == 6 ? 0xFCCCB29C725C2212ull : 0xFFFCFA18F6141211ull;
    return (unsigned)(w >> (4 * (v & 15))) & 0xF;
}
// il2p.py:509-512: the CRC that four Hamming-coded bytes carry
PM_IL2P_HD inline int hamming_crc(unsigned b0, unsigned b1, unsigned b2, unsigned b3)
{
    return (int)(hamming74(b0) << 12) + (int)(hamming74(b1) << 8) + (int)(hamming74(b2) << 4) + (int)hamming74(b3);
}

struct Split {
    int blocks, size, big;                                // il2p.py:346-358: `big` blocks of size + 1 bytes first, then blocks - big of `size`
};
PM_IL2P_HD inline Split block_split(int count)
{
    Split s{0, 0, 0};
    if (count <= 0) return s;
    s.blocks = (count + 238) / 239;
    s.size = count / s.blocks;
    s.big = count - s.blocks * s.size;
    return s;
}
PM_IL2P_HD inline int block_bytes(const Split &s, int b) { return s.size + (b < s.big ? 1 : 0); }
PM_IL2P_HD inline uint32_t body_bits(int count)             // the bits of all blocks with their parity
{
    const Split s = block_split(count);
    return 8u * (uint32_t)(count + 16 * s.blocks);
}

// ---- the record of an attempt (a place of the packet table, include/pymodem_amd.h) ----------------------------------------------
enum Status : uint8_t { kIncomplete = 0, kHeaderFail = 1, kDone = 2, kBlockFail = 3, kNotPlaced = 4 };
constexpr uint32_t kNoOffset = 0xFFFFFFFFu;
constexpr int kHeaderBits = 120;
struct Rec {
    uint32_t at, off;
    uint16_t count;
    uint8_t status, corrected;
    uint32_t end;
};
struct Opts {
    int crc, disable_rs, min_dist;
};

PM_IL2P_HD inline uint32_t rec_need(int count) { return (uint32_t)(13 + count + 7) & ~7u; }
PM_IL2P_HD inline int64_t rec_H(uint32_t at) { return 8 * (int64_t)(at >> 3) + (at & 7) + 1; }

// The header step of the attempt at `at` on its 15 bytes (hdr: corrected and descrambled in place; the stream holds them, H + 120 <= bits).
// kDone here means "passed and complete": the blocks decide the rest, and the place in the area (off) is the caller's.
PM_IL2P_HD inline Rec header_attempt(const GF256 *g, uint32_t at, uint8_t *hdr, const Opts &o, int64_t bits)
{
    Rec r{at, kNoOffset, 0, kHeaderFail, 0, (uint32_t)kHeaderBits};
    const int c = o.disable_rs ? 0 : rs_decode(g, 2, hdr, 15, o.min_dist, SerialSyndromes{g, 2});
    if (c < 0) return r;
    descramble(hdr, 13);
    const int count = header_count(hdr);
    const uint32_t end = (uint32_t)kHeaderBits + body_bits(count);
    if (rec_H(at) + end + (o.crc ? 32 : 0) > bits) return Rec{at, kNoOffset, 0, kIncomplete, 0, 0};
    r.count = (uint16_t)count;
    r.status = kDone;
    r.corrected = (uint8_t)c;
    r.end = end;
    return r;
}

PM_IL2P_HD inline Rec rec_incomplete(uint32_t at) { return Rec{at, kNoOffset, 0, kIncomplete, 0, 0}; }
PM_IL2P_HD inline Rec rec_not_placed(const Rec &r) { return Rec{r.at, kNoOffset, r.count, kNotPlaced, r.corrected, (uint32_t)kHeaderBits}; }

}  // namespace pm_il2p
