// The host arithmetic a certified AFSK sweep's decision rests on (pm_afsk.hip), in ONE copy: the bound E, the matrix-pipe constants, the
// dynamic-LDS layouts of afsk_slide_lpf_kernel / afsk_slide_lpf8_kernel / afsk_fused8_kernel and the choice of the launch a sweep takes.
// Plain C++17, no HIP types: tests/afsk_sweep_core_check.cpp checks it on the host -- a wrong E, layout or route fails no bitmap test,
// only the count of uncertain samples or the launch path moves.
#pragma once
#include <algorithm>
#include <cstddef>
#include "../../include/pymodem_amd.h"

namespace pm_sweep {

constexpr int kLanes = 256, kTile = kLanes * 8;      // a workgroup and the low-pass outputs it owns
constexpr int kSlideRun = 16;            // run length of afsk_slide_kernel
constexpr int kFuseRun = 12;             // measured (g = 7 / g = 1, 28.8 M samples): runs of 10: 0.416 / 0.289 ms, 12: 0.395 / 0.264, 16: 0.411 / 0.277, 34 (one wave slides): 0.471 / 0.317
constexpr int kTailCap = 48;             // uncertain (sample, modem) pairs a workgroup decides itself (0.06 per workgroup on average); more go to the list
constexpr int kL8Plane = 2176;           // bytes of a digit plane: 2048 outputs + (ml - 1 <= 112) + what the last tile's band reads beyond
constexpr int kL8Dig = 3;                // digits of a magnitude and of a tap
constexpr int kL8Acc = 4;                // accumulators: the weights 256^1 .. 256^4
constexpr int kL8Band = 2 * kL8Dig * 64 * 16, kL8List = (kTailCap + 4) * 4, kL8Max = 32;      // bytes: band operands, workgroup list + count, wave maxima

// Bound on |sliding magnitude - magnitude of the direct sums| for runs of `steps`: the value at step i of a run that started from the
// reference's own sum (same taps, same order: no difference at i = 0).  With Z_model the exact sums of the power filter r^j:  the run
// follows Z_model from a start that is off it by (tap deviation + the start sum's rounding), rotated, and the reference's sum at step i
// is off Z_model by the same two kinds of term:  2 sqrt2 m tap_dev X  +  2 sqrt2 m^2 u X.  On top, per step, 6 roundings of sums bounded
// by (m + 2) X and r^m being off by sqrt2 u:  < 16 u (m + 1) X, over at most `steps` steps.  The magnitude is 1-Lipschitz in the pair of
// sums and its own three roundings are the same on both sides up to 3 u m X.
static inline double slide_bound(const pm_afsk_tones *tones, int m, double x_bound, int steps = kSlideRun)
{
    const double u = 1.1102230246251565e-16;
    // (last term: slide_sqrt's one Newton step, relative 1.5e-12 of a magnitude that is at most sqrt2 m x_bound)
    return (16.0 * steps * u * (m + 1) + 3.0 * m * tones->tap_dev + 3.0 * u * m * m + 6.0 * u * m + 1.5e-12 * 1.4143 * m) * x_bound;
}

// E of a sweep (derivation: pm_afsk.hip, "gain sweep").  tones: nullptr for the direct correlator sums; steps: the sliding sums' run
// length; e_x: 0, or the bound on |the sweep's input - the reference's band-pass output| (pm_bpf8.hip).
static inline double sweep_bound(int m, double lpf_abs_sum, double gmax, double x_bound, const pm_afsk_tones *tones, int steps, double e_x)
{
    double e_slide = tones && m >= 2 ? slide_bound(tones, m, x_bound, steps) : 0.0;
    // magnitudes are 1-Lipschitz in the pair of correlator sums, each of which moves by at most m e_x; the sliding sums' own
    // bound is stated for inputs up to x_bound, which the approximate stream exceeds by at most e_x
    if (e_x != 0.0) e_slide = e_slide * (1.0 + e_x / x_bound) + 1.4143 * m * e_x;
    return 1e-10 * lpf_abs_sum * (1.0 + gmax) * (double)m * 1.4143 * x_bound + lpf_abs_sum * (1.0 + gmax) * e_slide;
}

// What the matrix pipe adds to E depends on the workgroup's own largest magnitude (its digits are scaled to it): the kernel computes
// it from these constants (lpf8_sweep_tile, Ecmp).  From a pm_lpf8_plan's S, tapq_int, qabs, dlow.
struct Lpf8Consts {
    int S;                               // taps: q = rint(h 2^S)
    double c_tap;                        // sum |h 2^S - q|: the taps' quantisation, in units of 2^-S
    double c_q;                          // sum |q| / 2 (the magnitudes' rounding) + the digit product that is left out: units of 2^-(S+s2)
    double gfac;                         // 1 + the largest gain (two streams: |a - g b|'s error), 1 for one stream
    double qabs;                         // sum |q|: what a unit of error in every magnitude's integer costs (PM_LPF8_F32MAG: the binary32 roots)
};
static inline Lpf8Consts lpf8_consts(int S, double tapq_int, double qabs, double dlow, double gmax, bool one) { return Lpf8Consts{S, tapq_int, 0.5 * qabs + dlow, one ? 1.0 : 1.0 + gmax, qabs}; }

// sliding runs of a workgroup: it needs the ml - 1 magnitudes past its kTile outputs too
static inline int sweep_runs(int ml) { return (kTile + ml - 1 + kFuseRun - 1) / kFuseRun; }
// doubles of LDS the exact chain of one (sample, modem) pair works in (sweep_tail_entry)
static inline size_t sweep_tail_doubles(int mc, int ml, int mb) { return (size_t)2 * ml + (size_t)(ml + mc - 1) * 2 + 2 * (size_t)mb + 4 * (size_t)mc; }

// The dynamic LDS block of the matrix-pipe kernels:  window | planes | templates | band operands | workgroup list | wave maxima.
// kb == 0: afsk_slide_lpf8_kernel, one sweep, its digit planes laid OVER the window (dead by then).  kb = 3 / 4 (the band-pass plan's
// blocks): afsk_fused8_kernel, up to two sweeps behind one window, the planes behind it -- two audio digit planes first, each sweep's
// low-pass planes later in their place.  mb: band-pass taps the exact chain goes back through (0: it reads the window's own stream).
struct SweepShape { int m, ml; bool one; };
struct Lpf8Layout {
    int xs_span, mmax;                   // band-passed values the workgroup needs: the largest runs * L + m - 1; the longest correlator
    int xw_doubles, aplane, plane_bytes; // the window; an audio digit plane (fused); the planes' region
    int region0;                         // doubles in front of the templates
    size_t off_planes, off_tpl, off_band, off_list, off_max, lds;      // bytes
    bool lds_ok;                         // the exact chain's work space fits in front of the templates
    bool fuses;                          // pure arithmetic of "this group takes the fused launch": ml + 15 <= 128, runs <= lanes, lds <= 64 KiB
};
static inline Lpf8Layout lpf8_layout(const SweepShape *s, int nsweeps, int mb, int kb)
{
    Lpf8Layout Y{};
    size_t tail = 0;
    int streams = 1;
    Y.fuses = true;
    for (int k = 0; k < nsweeps; ++k) {
        Y.fuses = Y.fuses && s[k].ml + 15 <= 128 && sweep_runs(s[k].ml) <= kLanes;
        Y.xs_span = std::max(Y.xs_span, sweep_runs(s[k].ml) * kFuseRun + s[k].m - 1);
        Y.mmax = std::max(Y.mmax, s[k].m);
        tail = std::max(tail, sweep_tail_doubles(s[k].m, s[k].ml, mb));
        if (!s[k].one) streams = 2;
    }
    Y.xw_doubles = (Y.xs_span + Y.xs_span / kFuseRun + 2 + 1) / 2 * 2;
    Y.plane_bytes = streams * kL8Dig * kL8Plane;
    if (kb) {
        Y.aplane = ((Y.xs_span + 255) / 256 * 256 + 64 * kb + 15) / 16 * 16;      // what the last tile's band reads: 256 (tile) + 64 kb - 16 bytes past its first
        Y.plane_bytes = (std::max(Y.plane_bytes, 2 * Y.aplane) + 15) / 16 * 16;
        Y.off_planes = (size_t)Y.xw_doubles * 8;
    }
    Y.region0 = kb ? Y.xw_doubles + Y.plane_bytes / 8 : std::max(Y.xw_doubles, Y.plane_bytes / 8);
    Y.off_tpl = (size_t)Y.region0 * 8;
    Y.off_band = Y.off_tpl + 4 * (size_t)Y.mmax * 8;
    Y.off_list = Y.off_band + kL8Band;
    Y.off_max = Y.off_list + kL8List;
    Y.lds = Y.off_max + kL8Max;
    Y.lds_ok = tail <= (size_t)Y.region0;
    Y.fuses = Y.fuses && Y.lds <= 64 * 1024;
    return Y;
}

// The dynamic LDS block of afsk_slide_lpf_kernel (low-passes in binary64):  window of x, later the space image | mark image | templates.
// The window in slide_slot's layout (a pad slot per run), the images in the FIR's (slot<8>(p) = p + p / 8).
static inline size_t fuse_region0(int m, int ml)
{
    const int nmag = kTile + ml - 1, p = sweep_runs(ml) * kFuseRun + m - 1;
    const int a = p + p / kFuseRun + 2, b = nmag + nmag / 8 + 2;
    return (size_t)(std::max(a, b) + 1) / 2 * 2;
}
static inline size_t fuse_image(int ml) { return (size_t)(kTile + ml - 1 + (kTile + ml - 1) / 8 + 3) / 2 * 2; }
static inline size_t fuse_lds_bytes(int m, int ml) { return (fuse_region0(m, ml) + fuse_image(ml) + 4 * (size_t)m) * sizeof(double); }

// ---- which launch a sweep takes -----------------------------------------------------------------------------------------------------
// kDirect: direct correlator sums, two low-passes, fir_sweep_kernel.  kSlide: sliding sums (afsk_slide_kernel) in front of the same.
// kFused64: afsk_slide_lpf_kernel.  kFused8: afsk_slide_lpf8_kernel, the low-passes on the matrix pipe.
enum SweepRoute { kDirect, kSlide, kFused64, kFused8 };
struct SweepSwitches { bool afsk_unfused, afsk_lpf8, sweep_no_tail, afsk_split; };      // pm_tuning's, as the launchers read them
struct SweepRouting {
    SweepRoute route;
    bool one;                            // one chain with tone templates: its mark - gain * space difference is ONE stream with ONE low-pass
    bool call_plan;                      // kFused8 on a low-pass plan made for this call (afsk_lpf8), not the caller's
    bool lds_ok;                         // kFused8: the workgroups decide their own uncertain samples (SweepTail::lds_ok)
    bool ends;                           // the sweep's own launch is its last: no exact launch behind it, the caller mails the count
};
// tones: the templates are tone models (sliding sums apply); mb: band-pass taps of the source the exact chain goes back to (0: none);
// plan_ml: taps of the caller's low-pass plan (0: none); own_list: the recording's own list (pm_sweep_cells::d_list)
static inline SweepRouting sweep_route(int m, int ml, int groups, bool tones, int mb, int plan_ml, bool own_list, const SweepSwitches &sw)
{
    const bool slide = tones && m >= 2;
    SweepRouting R{slide ? kSlide : kDirect, slide && groups == 1, false, false, false};
    if (!slide || sweep_runs(ml) > kLanes || fuse_lds_bytes(m, ml) > 120 * 1024 || sw.afsk_unfused) return R;
    R.route = kFused64;
    R.call_plan = plan_ml == 0 && sw.afsk_lpf8;
    if (ml + 15 > 128 || !(R.call_plan || plan_ml == ml)) { R.call_plan = false; return R; }
    R.route = kFused8;
    const SweepShape shape{m, ml, R.one};
    R.lds_ok = lpf8_layout(&shape, 1, mb, 0).lds_ok && !sw.sweep_no_tail;
    R.ends = own_list;
    return R;
}

// A recording's whole demod stage as afsk_fused8_kernel's single launch.  planned: a band-pass plan (of kb blocks), the recording's own
// list, and one or two sweeps that each take kFused8 on a plan of the caller's (which afsk_unfused rules out); aligned: the audio is on
// a 16-byte boundary; Y: lpf8_layout of the group, a layout the kernel is written for; and afsk_split does not ask for the launches apart.
static inline bool group_fuses(const Lpf8Layout &Y, int kb, bool planned, bool aligned, const SweepSwitches &sw)
{
    return planned && aligned && (kb == 3 || kb == 4) && !sw.afsk_split && Y.fuses;
}

}  // namespace pm_sweep
