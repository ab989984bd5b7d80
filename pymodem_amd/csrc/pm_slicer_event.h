// The slicer's event step (slice_walk_kernel<SlicerForm::Event, ...>): the samples of a word at which the reference recurrence does
// anything but an exact clk += 1.0, found ahead of time, and the runs between them taken as one addition; and the host's choice of a
// batch's step form (pm_slicer_choose).  Plain C++ so that the host model (tests/slicer_event_model.cpp) runs the very code the kernel
// and its launchers run.
//
// Per sample the walker executes (step32a in pm_slicer.hip, which says why each operation is the reference's own):
//     s = clk >= tp;  a = clk + 1.0;  c = a + (s ? -sps : +0);  clk = fma(c, crossing ? lock - 1 : +0, c).
// A sample is an EVENT if it is a crossing, or takes a symbol (clk >= tp), or its addition rounds (fl(clk + 1.0) != clk + 1.0).
// Every other sample leaves clk + 1.0 exactly (c = a + (+0) = a, fma(a, +0, a) = a), so a run of k of them is clk + k, and when
// every clk + j (0 <= j <= k) is a double, the one addition fl(clk + k) is that value too: bit for bit the k steps.
//
// pm_event_run(clk, tpe) returns a k such that the next k samples, if none of them is a crossing, are such a run.  Only a LOWER
// bound is needed: a run cut short is followed by a real step of the reference's operations, which is never wrong.
//   Symbols.  Needs clk + j < tp for 0 <= j < k, i.e. k - 1 < tp - clk.  With tpe = fl(tp - 2^-20) the kernel takes
//     k = ceil(fl(tpe - clk)): |tp| <= 1024, |clk| <= 2048 (pm_event_ok) make both roundings < 2^-40, so fl(tpe - clk) < tp - clk and
//     k - 1 < fl(tpe - clk) < tp - clk.
//   Exactness.  Let g = min(1, lowest set bit of clk).  Every clk + j is a multiple of g, and a multiple of g below 2^53 g in
//     magnitude is a double; |clk| < 2^53 g holds for every double (53 significand bits), and the run only climbs, so all of
//     clk .. clk + k are doubles if clk + k < L = 2^53 g.  The kernel takes k = ceil(fl(fl(L - (1 + 2^-20)) - clk)): both roundings
//     are < 2^-38 (L <= 2^13), so k < fl(...) + 1 < L - clk.  L is clamped to [2^-7, 2^13]: above, a smaller L is a smaller k;
//     below, |clk| < L < 2^-7 and the bound is ceil(of something in (-1, 0)) = 0.  Zero, either sign, has no set bit and lands on
//     the lower clamp (k = 0: one real step, which takes it to 1.0); subnormals land there too.
// k is the minimum of the two, and the kernel takes the minimum with the distance to the next crossing and to the word's end.
// A run of k = 0 adds +0.0, which changes only a clock of -0.0 -- and no real step leaves -0.0 (an exact zero sum is +0.0), a
// carried-in -0.0 is followed by a real step at once, and -0.0 and +0.0 step identically.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define PM_EVENT_HD __host__ __device__ __forceinline__
#else
#define PM_EVENT_HD inline
#endif

constexpr double kEventMargin = 0x1p-20;
constexpr double kEventClockLimit = 2048.0;
constexpr double kEventSpsMax = 1024.0;
constexpr double kEventTpLimit = 1024.0;

// The job-level preconditions of the bounds above, proven once per job on the host.  0.5 <= lock <= 1: lock - 1 is exact (Sterbenz,
// needed by the fma form) and the crossing's multiplication never grows |clk|.  1 <= sps <= 1024, |tp| <= 1024, |clk0| <= 2048: by
// induction |clk| <= 2048 before every sample of a full word -- a symbol takes clk in [tp, 2048] to fl(fl(clk + 1) - sps), within
// [tp + 1 - sps, 2048] and tp + 1 - sps >= -2047; no symbol takes clk in [-2048, tp) to fl(clk + 1), within [-2047, 1025]; rounding
// is monotone and 2048 a double.  Then |tpe - clk| < 2^12 and |lim - clk| < 2^14, which is what the error bounds above assumed.  The
// stream's partial last word compares with thr instead; its end state comes back as a later call's clk0 and is checked again.
PM_EVENT_HD bool pm_event_ok(double sps, double lock, double tp, double clk0)
{
    return sps >= 1.0 && sps <= kEventSpsMax && lock >= 0.5 && lock <= 1.0 && tp >= -kEventTpLimit && tp <= kEventTpLimit &&
           clk0 >= -kEventClockLimit && clk0 <= kEventClockLimit;     // (NaN fails every comparison)
}

PM_EVENT_HD uint64_t pm_event_bits(double v)
{
    uint64_t b;
    memcpy(&b, &v, 8);
    return b;
}

PM_EVENT_HD double pm_event_double(uint64_t b)
{
    double v;
    memcpy(&v, &b, 8);
    return v;
}

// Samples, from the clock clk on, that are certainly plain exact clk += 1.0 unless a crossing comes first (see above).  tpe = fl(tp - 2^-20).
PM_EVENT_HD int pm_event_run(double clk, double tpe)
{
    const uint64_t b = pm_event_bits(clk);
    const uint32_t hi = (uint32_t)(b >> 32), lo = (uint32_t)b;
    const int e = (int)((hi >> 20) & 0x7ffu);                                      // biased exponent
    const int t = lo ? __builtin_ctz(lo) : 32 + __builtin_ctz(hi | 0x100000u);     // trailing zeros of the significand, implicit bit included
    // lowest set bit 2^(e - 1075 + t); L = 2^53 min(1, that): biased exponent e + t + 1, clamped to [2^-7, 2^13]
    int le = e + t + 1;
    le = le < 1016 ? 1016 : le > 1036 ? 1036 : le;
    const double lim = pm_event_double((uint64_t)le << 52) - (1.0 + kEventMargin);
    const double x = fmin(tpe, lim) - clk;
    const double k = ceil(x);
    return k > 0.0 ? (int)k : 0;                                                   // k < 2^15
}

// One word (64 samples, bit b = sample b) of event stepping: returns the symbol flags, clk updated in place, and adds the number of
// real steps taken to `steps` (the host model counts them; in the kernel it is dead code).
PM_EVENT_HD uint64_t pm_event_word(double &clk, uint64_t zc, double tp, double tpe, double neg_sps, double lm1, int &steps)
{
    uint64_t sym = 0, zm = zc;                                     // zm: the crossings after the last real step
    int p = 0;
    for (;;) {
        const int qc = zm ? __builtin_ctzll(zm) : 64;
        const int run = pm_event_run(clk, tpe);
        const int q = qc < p + run ? qc : p + run;                  // the next real step (64: none in this word)
        clk = clk + (double)(q - p);
        if (q >= 64) break;
        ++steps;
        const bool s = clk >= tp;                                  // slicer.py:77-79
        const double a = clk + 1.0;                                // slicer.py:77
        const double c = a + (s ? neg_sps : 0.0);                  // slicer.py:81
        clk = fma(c, ((zc >> q) & 1) ? lm1 : 0.0, c);              // slicer.py:99-104 (step32a: the rounded product clk * lock)
        sym |= (uint64_t)s << q;
        zm = zc & (~1ull << q);
        p = q + 1;
    }
    return sym;
}

// The smallest double x with fl(x + 1.0) >= thr (NaN if it cannot be pinned down: the batch then keeps the compare on the sum).
inline double symbol_clock_threshold(double thr)
{
    if (!(thr - thr == 0.0)) return NAN;
    volatile double x = thr - 1.0;
    for (int k = 0; k < 64; ++k) {                       // down while the predecessor still reaches thr
        volatile double p = nextafter((double)x, -INFINITY);
        volatile double sum = p + 1.0;
        if (!(sum >= thr)) break;
        x = p;
        if (k == 63) return NAN;
    }
    for (int k = 0; k < 64; ++k) {                       // up until it does
        volatile double sum = x + 1.0;
        if (sum >= thr) return x;
        x = nextafter((double)x, INFINITY);
    }
    return NAN;
}

// The forms of a word's 64 steps (pm_slicer.hip): Compare = step32, the reference's compare and select, for any parameters;
// Hand = step32a, the decision read off the clock and the crossing's product as an fma; Event = the event step above, with step32a
// for the words in which some lane of the wave has too many crossings (walkers only).  LM0 / NS0: the low words of lock_rate - 1 /
// of sps are zero in every job (step32a saves an instruction per sample on each).
enum class SlicerForm { Compare, Hand, Event };
struct SlicerStep {
    SlicerForm form;
    bool lm0, ns0;
};
struct SlicerJob {
    double sps, lock, tp, clk0;
};
constexpr double kEventMinSps = 16.0;   // samples per symbol below which a batch keeps step32a (at most four symbols per word with events)

// One form for a whole batch.  Hand needs lock_rate - 1 exact (the fma form; it is for 0.5 <= lock_rate <= 2), lock_rate > 0 and finite
// sps, clk0 and tp -- lock_rate - 1 is exact for 0.0, -0.5, -1.0 as well, but there fma(c, lock - 1, c) and the reference's c * lock
// differ in the sign of a zero (lock 0: c * 0.0 is -0.0 for c < 0, the fma's exact zero sum +0.0; lock < 0: the other way round at
// c = +0.0), and a stream that ends on such a sample hands that sign out in its phase_clock; Event on top of it, where `event` allows it, every job meets pm_event_ok and takes few enough symbols per word for it to pay
// (a trip costs ~7 samples of step32a; fsk_9600 at 5 samples per symbol ran its walkers twice as long).
inline SlicerStep pm_slicer_choose(const SlicerJob *jobs, int njobs, bool event)
{
    bool hand = true, lm0 = true, ns0 = true;
    for (int j = 0; j < njobs; ++j) {
        const SlicerJob &d = jobs[j];
        const volatile double lm1 = d.lock - 1.0;
        hand = hand && lm1 + 1.0 == d.lock && d.lock > 0.0 && d.sps - d.sps == 0.0 && d.clk0 - d.clk0 == 0.0 && d.tp - d.tp == 0.0;
        lm0 = lm0 && (uint32_t)pm_event_bits(lm1) == 0;
        ns0 = ns0 && (uint32_t)pm_event_bits(d.sps) == 0;
        event = event && pm_event_ok(d.sps, d.lock, d.tp, d.clk0) && d.sps >= kEventMinSps;
    }
    if (!hand) return {SlicerForm::Compare, false, false};
    return {event ? SlicerForm::Event : SlicerForm::Hand, lm0, ns0};
}
