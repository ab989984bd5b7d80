// What one lane of bitscan_frames_kernel (pm_bitscan.hip) does with its 64-bit word of a frame's span, free of cross-lane operations so
// that the same text runs on the host (tests/frames_core_check.cpp steps through it lane by lane against the bit-serial model).
// Between the flag in front of a frame and the flag that closes it the decoder (ax25.py:30-89) appends every bit but
//   - a zero behind exactly five ones (stuffed: dropped),
//   - the seventh one of a run and every one after it, and the zero that ends such a run: each of these clears the bit and byte counters,
//     the bytes collected so far stay (ax25.py:36-39).
// So the span falls into SEGMENTS that end at the seventh one of a run; a segment of T appended bits gives T / 8 bytes and its T % 8 last
// bits are lost.  Bits are in stream order: bit i of a word is stream bit 64 w + i, and the first appended bit of a byte is its bit 0.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PM_FR_HD __host__ __device__ inline
#else
#define PM_FR_HD inline
#endif

namespace pm_frames {

PM_FR_HD uint64_t low_mask(int k) { return k >= 64 ? ~0ull : k <= 0 ? 0ull : (1ull << k) - 1; }

// keep: the bits of `span` that are appended; reset: the bits of `span` that clear the counters (they come in unbroken groups)
struct WordMarks {
    uint64_t keep, reset;
};
PM_FR_HD WordMarks word_marks(uint64_t w, uint64_t prev, uint64_t span)
{
    const uint64_t e1 = (w << 1) | (prev >> 63), e2 = (w << 2) | (prev >> 62), e3 = (w << 3) | (prev >> 61), e4 = (w << 4) | (prev >> 60),
                   e5 = (w << 5) | (prev >> 59), e6 = (w << 6) | (prev >> 58), e7 = (w << 7) | (prev >> 57);
    const uint64_t o5 = e1 & e2 & e3 & e4 & e5;
    const uint64_t stuffed = ~w & o5 & ~e6, late_one = w & o5 & e6, run_end = ~w & o5 & e6 & e7;
    WordMarks m;
    m.reset = (late_one | run_end) & span;
    m.keep = span & ~(stuffed | late_one | run_end);
    return m;
}

// A stretch of consecutive words as the counters see it.  r: it holds a reset; a: appended bits in front of its first reset; m: bytes of the
// segments that begin and end inside it; t: appended bits behind its last reset.  Without a reset a = t = all its appended bits.
struct Span {
    int32_t r, a, m, t;
};
PM_FR_HD Span join(const Span &A, const Span &B)
{
    Span o;
    o.r = A.r | B.r;
    o.a = A.r ? A.a : A.a + B.a;
    o.t = B.r ? B.t : A.t + B.t;
    o.m = A.m + B.m + ((A.r && B.r) ? (A.t + B.a) >> 3 : 0);
    return o;
}

// The counters in front of a word: bytes of the segments that are closed, appended bits of the open one.
struct State {
    int64_t bytes;
    int32_t open;
};
PM_FR_HD State advance(State s, const Span &e)
{
    if (!e.r) {
        s.open += e.t;
    } else {
        s.bytes += ((s.open + e.a) >> 3) + e.m;
        s.open = e.t;
    }
    return s;
}

// The pieces of a word in stream order, fn(appended bits of the piece, it is the word's first piece, a reset ends it).
template <class Fn>
PM_FR_HD void word_pieces(uint64_t keep, uint64_t reset, Fn fn)
{
    int cur = 0;
    bool first = true;
    for (uint64_t rem = reset; rem;) {
        const int q = __builtin_ctzll(rem);
        fn(keep & low_mask(q) & ~low_mask(cur), first, true);
        first = false;
        const uint64_t above = ~(rem >> q);                 // the group of resets that begins at q ends at above's lowest bit
        cur = q + (above ? __builtin_ctzll(above) : 64 - q);
        rem = cur < 64 ? rem & ~low_mask(cur) : 0;
    }
    fn(cur < 64 ? keep & ~low_mask(cur) : 0, first, false);
}

PM_FR_HD Span word_span(const WordMarks &k)
{
    Span s{0, 0, 0, 0};
    word_pieces(k.keep, k.reset, [&](uint64_t piece, bool first, bool closed) {
        const int c = __builtin_popcountll(piece);
        if (first) s.a = c;
        if (!closed) s.t = c;
        if (closed) s.r = 1;
        if (closed && !first) s.m += c >> 3;
    });
    return s;
}

// The bits of `piece` (positions in word x), squeezed together, to bit `at` of a line of 32-bit words and on, `room` bits at most: the
// stuffed zeros split a piece into a handful of unbroken runs, each of which is a shift and up to three ORs.
template <class Or>
PM_FR_HD void put_piece(uint64_t x, uint64_t piece, int64_t at, int32_t room, Or or_word)
{
    while (piece && room > 0) {
        const int i = __builtin_ctzll(piece);
        const uint64_t above = ~(piece >> i);
        const int run = above ? __builtin_ctzll(above) : 64 - i;
        const int l = run < room ? run : room;
        const uint64_t chunk = (x >> i) & low_mask(l);
        const int d = (int)(at >> 5), o = (int)(at & 31);
        const uint64_t lo = chunk << o;
        if ((uint32_t)lo) or_word(d, (uint32_t)lo);
        if ((uint32_t)(lo >> 32)) or_word(d + 1, (uint32_t)(lo >> 32));
        if (o && (chunk >> (64 - o))) or_word(d + 2, (uint32_t)(chunk >> (64 - o)));
        at += l;
        room -= l;
        piece = i + run < 64 ? piece & ~low_mask(i + run) : 0;
    }
}

constexpr int32_t kOpenEnded = 0x7FFFFFFF;

// A lane's word into the line.  st: the counters in front of the word; bit0: the line's bit of the frame's bit 0 (may be negative: what
// lies in front of the line has gone out); later: the appended bits that the segment open behind the word has when it closes, kOpenEnded
// if it does not close in this trip.  A segment's bits are written only as far as its whole bytes go.
template <class Or>
PM_FR_HD void put_word(uint64_t x, const WordMarks &k, State st, int64_t bit0, int32_t later, Or or_word)
{
    word_pieces(k.keep, k.reset, [&](uint64_t piece, bool, bool closed) {
        const int c = __builtin_popcountll(piece);
        const int32_t len = closed ? st.open + c : later;
        const int32_t room = len == kOpenEnded ? 64 : (len & ~7) - st.open;
        put_piece(x, piece, bit0 + 8 * st.bytes + st.open, room, or_word);
        if (closed) {
            st.bytes += (st.open + c) >> 3;
            st.open = 0;
        } else {
            st.open += c;
        }
    });
}

// ---- CRC-16 (crc_functions.py:44-55: reflected, polynomial 0x8408) over a trip's bytes, a lane a piece ---------------------------------
// The register is a polynomial over GF(2) modulo the CRC's, bit 15 the coefficient of x^0; a zero bit fed in multiplies it by x.  Fed
// from a clear register a message's leading zero bytes change nothing, and a register S in front of a message of two bytes or more is
// the clear register in front of the same message with S's two bytes XORed into its first two.  So a trip's `len` bytes are cut into 64
// pieces of `per` bytes that END at the trip's last byte, every lane feeds its piece to a clear register, and the pieces are joined by
// a scan: (register of the lanes in front) * x^(8 * per * lanes behind) + (register of the lanes behind).
PM_FR_HD uint32_t crc_times_x(uint32_t s, int bits)
{
    for (int i = 0; i < bits; ++i) s = (s & 1) ? (s >> 1) ^ 0x8408u : s >> 1;
    return s;
}
PM_FR_HD uint32_t crc_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 15; i >= 0; --i) {
        if ((a >> i) & 1) p ^= b;
        b = (b & 1) ? (b >> 1) ^ 0x8408u : b >> 1;
    }
    return p;
}
// lane's piece: byte(k) is the trip's byte k (0 <= k < len), table the 256 one-byte steps, crc the register in front of the trip
template <class Byte>
PM_FR_HD uint32_t crc_piece(const uint16_t *table, int lane, int len, int per, uint32_t crc, Byte byte)
{
    uint32_t s = 0;
    for (int k = len - per * (64 - lane), end = k + per; k < end; ++k) {
        if (k < 0) continue;
        const uint32_t b = byte(k) ^ (k == 0 ? crc & 0xFF : k == 1 ? crc >> 8 : 0);
        s = (s >> 8) ^ table[(s ^ b) & 0xFF];
    }
    return s;
}

}  // namespace pm_frames
