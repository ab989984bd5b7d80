// Host model of the slicer walkers' event step (tests/test_slicer_event_model.py): the kernel's own pm_slicer_event.h, compiled for the
// CPU, beside the reference recurrence (slicer.py:59-107) sample by sample, and the launchers' choice of step form.  Built as a shared
// library and driven through ctypes.
#include "../pymodem_amd/csrc/pm_slicer_event.h"
#include <cstdint>

extern "C" {

int model_ok(double sps, double lock, double tp, double clk0) { return pm_event_ok(sps, lock, tp, clk0) ? 1 : 0; }

int model_run(double clk, double tpe) { return pm_event_run(clk, tpe); }

double model_threshold(double thr) { return symbol_clock_threshold(thr); }

// pm_slicer_choose over njobs jobs (tp from the header's symbol_clock_threshold, as the launchers take it): form * 4 + lm0 + 2 ns0
int model_choose(const double *sps, const double *lock, const double *clk0, int njobs, int event)
{
    SlicerJob jobs[64];
    if (njobs < 1 || njobs > 64) return -1;
    for (int j = 0; j < njobs; ++j) jobs[j] = {sps[j], lock[j], symbol_clock_threshold(sps[j] / 2.0 - 0.5), clk0[j]};
    const SlicerStep f = pm_slicer_choose(jobs, njobs, event != 0);
    return (int)f.form * 4 + (f.lm0 ? 1 : 0) + (f.ns0 ? 2 : 0);
}

// The reference: per sample clk += 1.0; clk >= thr takes a symbol and clk -= sps; a crossing multiplies by lock_rate.
// zc: crossing flags, bit b of word w = sample 64 w + b.  ck[w] = the clock entering word w, sym[w] = its symbol flags.
double model_plain(double clk, const uint64_t *zc, int64_t nwords, double thr, double sps, double lock, uint64_t *sym, double *ck)
{
    for (int64_t w = 0; w < nwords; ++w) {
        ck[w] = clk;
        uint64_t s = 0;
        for (int b = 0; b < 64; ++b) {
            clk += 1.0;
            if (clk >= thr) {
                clk -= sps;
                s |= 1ull << b;
            }
            if ((zc[w] >> b) & 1) clk = clk * lock;
        }
        sym[w] = s;
    }
    return clk;
}

// The walker's full words: the event step, or -- in a word with more than `evt` crossings -- step32a's operations sample by sample
// (the kernel's wave-uniform fallback, seen from one lane).  `events` counts the real steps the event form took.
double model_event(double clk, const uint64_t *zc, int64_t nwords, double tp, double sps, double lock, int evt, uint64_t *sym, double *ck,
                   int64_t *events)
{
    const double tpe = tp - kEventMargin, neg_sps = -sps, lm1 = lock - 1.0;
    int64_t ev = 0;
    for (int64_t w = 0; w < nwords; ++w) {
        ck[w] = clk;
        if (__builtin_popcountll(zc[w]) > evt) {
            uint64_t s = 0;
            for (int b = 0; b < 64; ++b) {
                const bool t = clk >= tp;
                const double a = clk + 1.0;
                const double c = a + (t ? neg_sps : 0.0);
                clk = fma(c, ((zc[w] >> b) & 1) ? lm1 : 0.0, c);
                s |= (uint64_t)t << b;
            }
            sym[w] = s;
        } else {
            int steps = 0;
            sym[w] = pm_event_word(clk, zc[w], tp, tpe, neg_sps, lm1, steps);
            ev += steps;
        }
    }
    *events = ev;
    return clk;
}

}  // extern "C"
