// The AFSK stage of the demod_chain path on the FIR tile of pm_fir_dev.h: the direct correlators (pm_afsk_correlate, SURVEY K2;
// afsk.py:153-162) and their group form, the sliding sums, the certified gain sweeps in their three generations (fir_sweep_kernel,
// afsk_slide_lpf_kernel, afsk_slide_lpf8_kernel), the whole stage in one launch (afsk_fused8_kernel), the exact chain for single
// samples, and the sweeps' counter ring and tickets.  The bound, the matrix-pipe constants and the LDS layout the certified decision
// rests on are host arithmetic in pm_afsk_sweep.h.  Arithmetic and tiling of the canonical sums: pm_fir.hip.
#include "pm_fir_dev.h"
#include "pm_bpf8_dev.h"
#include "pm_afsk_sweep.h"
#include <cmath>
#include <cstring>

namespace {
using namespace pm_sweep;

// Four correlators over one staged window; R outputs x 4 filters = 4R accumulators per thread.
// SPLIT: write the two magnitudes as separate streams (y = mark, y2 = space) instead of their difference (pm_afsk_sweep_signs).
template <int R, bool VEC, bool SPLIT = false>
__global__ __launch_bounds__(kThreads) void afsk_correlate_kernel(const double *__restrict__ x, int64_t n,
                                                                  const double *__restrict__ mi, const double *__restrict__ mq,
                                                                  const double *__restrict__ si, const double *__restrict__ sq,
                                                                  int m, double *__restrict__ y, int64_t nout, double *__restrict__ y2 = nullptr)
{
    extern __shared__ double xs[];
    constexpr int T = kThreads * R;
    const int t = threadIdx.x;
    const int span = T + m - 1;
    const int64_t tile0 = (int64_t)blockIdx.x * T;
    if (VEC) {
        stage_vec<R>(x, n, tile0, span, t, xs);
    } else {
        for (int idx = t; idx < span; idx += kThreads) {
            int64_t gi = tile0 + idx;
            xs[slot<R>(idx)] = gi < n ? x[gi] : 0.0;
        }
    }
    lds_barrier();

    double a[R], b[R], c[R], d[R];
#pragma unroll
    for (int r = 0; r < R; ++r) a[r] = b[r] = c[r] = d[r] = 0.0;
    static_assert(R == 4, "the block schedule below is written for 4 outputs per thread and 4 taps per block");
    double s0[R], s1[R];                     // alternating carry / new window sets, as in fir_valid_kernel
    const double *lp = xs + t * (R + 1);
#pragma unroll
    for (int j = 0; j < R - 1; ++j) s1[j + 1] = lp[j];
    const double *pa = mi + (m - 4), *pb = mq + (m - 4), *pc = si + (m - 4), *pd = sq + (m - 4);
    int i0 = 0;
#define PM_CORR_BLOCK(CARRY, NEW)                                                                  \
    {                                                                                              \
        NEW[0] = lp[3];                                                                            \
        _Pragma("unroll") for (int q = 1; q < 4; ++q) NEW[q] = lp[4 + q];                          \
        _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                            \
            const double ga = pa[3 - q], gb = pb[3 - q], gc = pc[3 - q], gd = pd[3 - q];           \
            _Pragma("unroll") for (int r = 0; r < R; ++r) {                                        \
                const double v = (r + q < 3) ? CARRY[r + q + 1] : NEW[r + q - 3];                  \
                a[r] = __builtin_fma(ga, v, a[r]);                                                 \
                b[r] = __builtin_fma(gb, v, b[r]);                                                 \
                c[r] = __builtin_fma(gc, v, c[r]);                                                 \
                d[r] = __builtin_fma(gd, v, d[r]);                                                 \
            }                                                                                      \
        }                                                                                          \
        lp += R + 1;                                                                               \
        pa -= 4; pb -= 4; pc -= 4; pd -= 4;                                                        \
    }
    for (; i0 + 8 <= m; i0 += 8) {
        PM_CORR_BLOCK(s1, s0)
        PM_CORR_BLOCK(s0, s1)
    }
    if (i0 + 4 <= m) {
        PM_CORR_BLOCK(s1, s0)
        i0 += 4;
    }
#undef PM_CORR_BLOCK
    if (i0 < m) {                            // m % 4 leftover taps, compile-time count, carry moved into s1
        if ((i0 >> 2) & 1) {
#pragma unroll
            for (int j = 1; j < R; ++j) s1[j] = s0[j];
        }
        const int left = m - i0;
#define PM_CORR_TAIL(K)                                                                            \
        case K: {                                                                                  \
            s0[0] = lp[3];                                                                         \
            _Pragma("unroll") for (int q = 1; q < K; ++q) s0[q] = lp[4 + q];                       \
            _Pragma("unroll") for (int q = 0; q < K; ++q) {                                        \
                const int k = left - 1 - q;                                                        \
                const double ga = mi[k], gb = mq[k], gc = si[k], gd = sq[k];                       \
                _Pragma("unroll") for (int r = 0; r < R; ++r) {                                    \
                    const double v = (r + q < 3) ? s1[r + q + 1] : s0[r + q - 3];                  \
                    a[r] = __builtin_fma(ga, v, a[r]);                                             \
                    b[r] = __builtin_fma(gb, v, b[r]);                                             \
                    c[r] = __builtin_fma(gc, v, c[r]);                                             \
                    d[r] = __builtin_fma(gd, v, d[r]);                                             \
                }                                                                                  \
            }                                                                                      \
        } break;
        switch (left) {
            PM_CORR_TAIL(1) PM_CORR_TAIL(2) PM_CORR_TAIL(3)
        default: break;
        }
#undef PM_CORR_TAIL
    }
    double markv[R], spacev[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        // afsk.py:153-162: sqrt(i**2 + q**2) with separately rounded squares and sum, then mark - space
        markv[r] = __builtin_sqrt(a[r] * a[r] + b[r] * b[r]);
        spacev[r] = __builtin_sqrt(c[r] * c[r] + d[r] * d[r]);
    }
    // results go back through the LDS image so that the global stores are lane-contiguous
    auto emit = [&](const double (&v)[R], double *__restrict__ dst) {
        lds_barrier();
#pragma unroll
        for (int r = 0; r < R; ++r) xs[t * (R + 1) + r] = v[r];
        lds_barrier();
        if (VEC) {
#pragma unroll
            for (int r = 0; r < R / 2; ++r) {
                const int idx = 2 * (r * kThreads + t);
                const int64_t go = tile0 + idx;
                const int s0i = slot<R>(idx);
                const double2v w = {xs[s0i], xs[s0i + 1]};
                if (go + 1 < nout) *reinterpret_cast<double2v *>(dst + go) = w;
                else if (go < nout) dst[go] = w.x;
            }
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int idx = r * kThreads + t;
                const int64_t go = tile0 + idx;
                if (go < nout) dst[go] = xs[slot<R>(idx)];
            }
        }
    };
    if (SPLIT) {
        emit(markv, y);
        emit(spacev, y2);
    } else {
        double diff[R];
#pragma unroll
        for (int r = 0; r < R; ++r) diff[r] = markv[r] - spacev[r];
        emit(diff, y);
    }
}

// Mark and unit-space magnitudes by a sliding sum (pm_afsk_sweep_signs_tones): the correlator taps of afsk.py:134-144 are the
// powers of one rotation, h[j] = r^j with r = e^{iw} (real part = the cos template, imaginary part = the sin template), so the
// complex correlator sum Z(k) = sum_j r^j x[k + m - 1 - j] obeys
//     Z(k + 1) = x[k + m] + r Z(k) - r^m x[k]
// -- 6 fused operations per tone and sample instead of 2m.  The result is NOT the reference's sum, only within a bound of it
// (L steps of rounding, r^m rounded once, the taps' own deviation from exact powers, measured by the host), which is
// all a certified-sign path needs.  A thread starts its run of L consecutive outputs from the direct sum with the real taps and
// slides from there; runs are short so that the error does not build up and so that the 4m fmas of a start are spread over L
// outputs.  x is staged through LDS with one pad slot per L (lane t's run starts at slot t(L+1)).
struct SlideTones {
    double mr, ms, mer, mes;       // mark:  r = mr + i ms,  r^m = mer + i mes
    double sr, ss, ser, ses;       // space (unit gain)
};
constexpr int kSlideThreads = 128;
template <int L>
__host__ __device__ __forceinline__ int slide_slot(int p) { return p + p / L; }
template <int L>
size_t slide_lds_bytes(int m) { return (size_t)(slide_slot<L>(kSlideThreads * L + m - 1) + 2 + 4 * m) * sizeof(double); }

// sqrt for the sliding sums: reciprocal-square-root seed and ONE coupled Newton step.  With the seed y = (1 + d) / sqrt(v), g = v y and
// h = y / 2 give r = 1/2 - h g = -d - d^2/2 and g (1 + r) = sqrt(v) (1 - 3/2 d^2 + O(d^3)): a seed good to 2^-20 (the ISA manuals give
// V_RSQ_F64 2^29 units in the last place, 2^-23) leaves a relative error below 1.5e-12, which slide_bound() adds to the bound of the
// certified decision (0.1 % of its thousandfold slack) -- the decision needs a value and a bound, not the last bit.  Round 2 took a
// second step (2 units in the last place): three more dependent fma per root, two roots per output, 2 % of the fused kernel.  A v
// below 1e-300 (0 on digital silence, where the seed would be infinite) is raised to that: a root of 1e-150 at most instead of 0.  The IEEE sqrt costs twice the
// instructions again (scaling of subnormal and huge arguments, class checks).
__device__ __forceinline__ double slide_sqrt(double v)
{
    v = __builtin_fmax(v, 1e-300);                            // one instruction where a compare and two selects stood
    const double y = __builtin_amdgcn_rsq(v);
    const double g = v * y, h = 0.5 * y;
    const double r = __builtin_fma(-h, g, 0.5);
    return __builtin_fma(g, r, g);
}

// One run: the direct sums of output k0 of the staged tile with the real taps, ascending input index (afsk.py:153-160; every lane
// reads the same four taps per step, an LDS broadcast), then L - 1 sliding steps; the 2 x L magnitudes stay in registers.
template <int L>
__device__ __forceinline__ void slide_run(const double *__restrict__ xs, const double *__restrict__ tp, int run, int m, const SlideTones &T,
                                          double (&mv)[L], double (&sv)[L])
{
    // run starts at input run * L = slot run * (L + 1); input run * L + j sits j + j / L slots further, and j is the same in every lane:
    // the division stays on the scalar unit (as slide_slot(run * L + j) it was a dozen vector instructions per read)
    const double *xr = xs + run * (L + 1);
    double a = 0.0, b = 0.0, c = 0.0, d = 0.0;
    {
        const double2v *tq = reinterpret_cast<const double2v *>(tp);
        int i = 0;
        for (; i + 4 <= m; i += 4) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double v = xr[slide_slot<L>(i + q)];
                const double2v h01 = tq[2 * (i + q)], h23 = tq[2 * (i + q) + 1];
                a = __builtin_fma(h01.x, v, a);
                b = __builtin_fma(h01.y, v, b);
                c = __builtin_fma(h23.x, v, c);
                d = __builtin_fma(h23.y, v, d);
            }
        }
        for (; i < m; ++i) {
            const double v = xr[slide_slot<L>(i)];
            const double2v h01 = tq[2 * i], h23 = tq[2 * i + 1];
            a = __builtin_fma(h01.x, v, a);
            b = __builtin_fma(h01.y, v, b);
            c = __builtin_fma(h23.x, v, c);
            d = __builtin_fma(h23.y, v, d);
        }
    }
#pragma unroll
    for (int i = 0; i < L; ++i) {
        mv[i] = slide_sqrt(a * a + b * b);                   // afsk.py:157
        sv[i] = slide_sqrt(c * c + d * d);
        if (i + 1 < L) {
            const double xk = xr[i], xn = xr[slide_slot<L>(i + m)];
            const double a2 = __builtin_fma(T.mr, a, __builtin_fma(-T.ms, b, __builtin_fma(-T.mer, xk, xn)));
            const double b2 = __builtin_fma(T.ms, a, __builtin_fma(T.mr, b, -T.mes * xk));
            const double c2 = __builtin_fma(T.sr, c, __builtin_fma(-T.ss, d, __builtin_fma(-T.ser, xk, xn)));
            const double d2 = __builtin_fma(T.ss, c, __builtin_fma(T.sr, d, -T.ses * xk));
            a = a2; b = b2; c = c2; d = d2;
        }
    }
}

// The same run with the two roots in binary32: v_sqrt_f32 of the binary64 sum of squares rounded to binary32 -- for afsk_slide_lpf8_kernel,
// whose magnitudes end as integers of 22 bits anyway.  What that costs in accuracy is a relative 2^-23 (the instruction: within one unit
// in the last place for every one of the 2^24 significands of a binade, checked exhaustively on the device by
// tests/test_gpu_kernels.py::test_v_sqrt_f32_is_within_one_ulp, pm_ubench_sqrt_f32) + 2^-25 (the conversion of the radicand), which the
// kernel adds to its bound in units of its integers; what it saves is the binary64 reciprocal-square-root seed and its Newton step (six
// instructions of which one is quarter-rate) -- twice per sample.  Radicands below binary32's normal range give roots below 2^-63 either
// way: the kernel only scales workgroups whose largest magnitude is above 2^-21, so that is below 2^-20 of a unit.
// (tg: nullptr, or the same four templates -- reversed and interleaved, tg[4 i + f] = h_f[m - 1 - i] -- in DEVICE memory, read through the
// constant address space: uniform addresses, so the loads are scalar loads and the taps reach the fma as scalar operands.  From LDS every
// lane of a wave fetched the same 32 bytes per tap beside its own 8 of the window: 40 bytes per lane and tap against an LDS pipe of 128
// bytes per cycle for the whole CU -- 20 cycles per tap and wave for 16 cycles of fma; the start sums were bound by that, not by the
// vector pipe (taking 15 % of the kernel's vector instructions out of them changed nothing: round 5, gpurun_out r5aa).)
typedef const double __attribute__((address_space(4))) *const_f64_ptr;
template <int L>
__device__ __forceinline__ void slide_run_f32(const double *__restrict__ xs, const double *__restrict__ tp, int run, int m, const SlideTones &T,
                                              float (&mv)[L], float (&sv)[L], const double *tg = nullptr)
{
    const double *xr = xs + run * (L + 1);
    double a = 0.0, b = 0.0, c = 0.0, d = 0.0;
    if (tg) {
        const_f64_ptr tq = (const_f64_ptr)tg;                 // NOLINT: only a C-style cast changes the address space
        const double *xb = xr;
        int i = 0;
        for (; i + L <= m; i += L, xb += L + 1, tq += 4 * L) {
#pragma unroll
            for (int j = 0; j < L; ++j) {
                const double v = xb[j];
                a = __builtin_fma(tq[4 * j + 0], v, a);
                b = __builtin_fma(tq[4 * j + 1], v, b);
                c = __builtin_fma(tq[4 * j + 2], v, c);
                d = __builtin_fma(tq[4 * j + 3], v, d);
            }
        }
        for (int j = 0; i + j < m; ++j) {
            const double v = xb[j];
            a = __builtin_fma(tq[4 * j + 0], v, a);
            b = __builtin_fma(tq[4 * j + 1], v, b);
            c = __builtin_fma(tq[4 * j + 2], v, c);
            d = __builtin_fma(tq[4 * j + 3], v, d);
        }
    } else {
        // The run's window starts on a block boundary of the padded layout (slot(L run) = (L + 1) run), so its taps go in blocks of L
        // whose L values are CONSECUTIVE doubles, one pad apart from block to block: every LDS address of a block is the block's base
        // plus an immediate.  (Round 5: as slide_slot(i + q) per tap -- a division by 12 each -- the start sums spent 20 vector
        // instructions on addresses for every 16 fma, 15 % of the fused kernel's vector instructions.)  Same taps, same order, same sums.
        const double2v *tq = reinterpret_cast<const double2v *>(tp);
        const double *xb = xr;
        int i = 0;
        for (; i + L <= m; i += L, xb += L + 1, tq += 2 * L) {
#pragma unroll
            for (int j = 0; j < L; ++j) {
                const double v = xb[j];
                const double2v h01 = tq[2 * j], h23 = tq[2 * j + 1];
                a = __builtin_fma(h01.x, v, a);
                b = __builtin_fma(h01.y, v, b);
                c = __builtin_fma(h23.x, v, c);
                d = __builtin_fma(h23.y, v, d);
            }
        }
        for (int j = 0; i + j < m; ++j) {                    // fewer than L taps left: inside one block
            const double v = xb[j];
            const double2v h01 = tq[2 * j], h23 = tq[2 * j + 1];
            a = __builtin_fma(h01.x, v, a);
            b = __builtin_fma(h01.y, v, b);
            c = __builtin_fma(h23.x, v, c);
            d = __builtin_fma(h23.y, v, d);
        }
    }
#pragma unroll
    for (int i = 0; i < L; ++i) {
        mv[i] = __builtin_amdgcn_sqrtf((float)__builtin_fma(a, a, b * b));       // afsk.py:157
        sv[i] = __builtin_amdgcn_sqrtf((float)__builtin_fma(c, c, d * d));
        if (i + 1 < L) {
            const double xk = xr[i], xn = xr[slide_slot<L>(i + m)];
            const double a2 = __builtin_fma(T.mr, a, __builtin_fma(-T.ms, b, __builtin_fma(-T.mer, xk, xn)));
            const double b2 = __builtin_fma(T.ms, a, __builtin_fma(T.mr, b, -T.mes * xk));
            const double c2 = __builtin_fma(T.sr, c, __builtin_fma(-T.ss, d, __builtin_fma(-T.ser, xk, xn)));
            const double d2 = __builtin_fma(T.ss, c, __builtin_fma(T.sr, d, -T.ses * xk));
            a = a2; b = b2; c = c2; d = d2;
        }
    }
}

template <int L>
__global__ __launch_bounds__(kSlideThreads) void afsk_slide_kernel(const double *__restrict__ x, int64_t n, const double *__restrict__ mi,
                                                                   const double *__restrict__ mq, const double *__restrict__ ui,
                                                                   const double *__restrict__ uq, int m, SlideTones T,
                                                                   double *__restrict__ M, double *__restrict__ S, int64_t nout, double gain)
{
    extern __shared__ double xs[];
    constexpr int TILE = kSlideThreads * L;
    const int t = threadIdx.x;
    const int span = TILE + m - 1;
    const int64_t tile0 = (int64_t)blockIdx.x * TILE;
    double *tp = xs + (slide_slot<L>(span) + 2) / 2 * 2;   // the four templates, reversed and interleaved: tp[4i + f] = h_f[m - 1 - i]
    if (((uintptr_t)x & 15) == 0 && tile0 + TILE <= n) {
        // the tile's own TILE inputs: L / 2 independent 16-byte loads per lane, all in flight before the first LDS write
        double2v v[L / 2];
#pragma unroll
        for (int q = 0; q < L / 2; ++q) v[q] = *reinterpret_cast<const double2v *>(x + tile0 + 2 * (q * kSlideThreads + t));
#pragma unroll
        for (int q = 0; q < L / 2; ++q) {
            const int s0 = slide_slot<L>(2 * (q * kSlideThreads + t));     // even position: its pair never straddles a pad slot
            xs[s0] = v[q].x;
            xs[s0 + 1] = v[q].y;
        }
        for (int p = TILE + t; p < span; p += kSlideThreads) {
            const int64_t gi = tile0 + p;
            xs[slide_slot<L>(p)] = gi < n ? x[gi] : 0.0;
        }
    } else {
        for (int p = t; p < span; p += kSlideThreads) {
            const int64_t gi = tile0 + p;
            xs[slide_slot<L>(p)] = gi < n ? x[gi] : 0.0;
        }
    }
    for (int i = t; i < m; i += kSlideThreads) {
        tp[4 * i + 0] = mi[m - 1 - i];
        tp[4 * i + 1] = mq[m - 1 - i];
        tp[4 * i + 2] = ui[m - 1 - i];
        tp[4 * i + 3] = uq[m - 1 - i];
    }
    lds_barrier();
    // The run's 2 x L results stay in registers; once every lane is done with the staged inputs, the LDS image is reused to turn
    // "L consecutive outputs per lane" into coalesced stores, one stream after the other.
    double mv[L], sv[L];
    slide_run<L>(xs, tp, t, m, T, mv, sv);
    if (!S) {                                                // one chain: its mark - space difference (afsk.py:162) in ONE stream
#pragma unroll
        for (int i = 0; i < L; ++i) mv[i] = __builtin_fma(-gain, sv[i], mv[i]);
    }
    const bool full = tile0 + TILE <= nout && ((((uintptr_t)M) | ((uintptr_t)S)) & 15) == 0;      // uniform over the workgroup
    auto emit = [&](const double (&v)[L], double *__restrict__ dst) {
        lds_barrier();
        double *op = xs + t * (L + 1);                       // = slide_slot(k0): this lane's L results in L consecutive slots
#pragma unroll
        for (int i = 0; i < L; ++i) op[i] = v[i];
        lds_barrier();
        if (full) {
#pragma unroll
            for (int q = 0; q < L / 2; ++q) {
                const int p = 2 * (q * kSlideThreads + t);
                const int s0 = slide_slot<L>(p);
                *reinterpret_cast<double2v *>(dst + tile0 + p) = double2v{xs[s0], xs[s0 + 1]};
            }
        } else {
            for (int p = t; p < TILE; p += kSlideThreads)
                if (tile0 + p < nout) dst[tile0 + p] = xs[slide_slot<L>(p)];
        }
    };
    emit(mv, M);
    if (S) emit(sv, S);
}

// G correlator banks that share their mark filters (the chains of afsk_1200_ax25_super_opt.json differ in space gain only):
// F = 2 + 2G filters over one staged window, the mark pair (and its square root) computed once.  w holds the filters interleaved
// and reversed, w[i * F + f] = h_f[m - 1 - i], so that the F coefficients of one tap step are one contiguous scalar load.
// R = 2 outputs per thread: F * R accumulators, one LDS read per F * R fmas, and each lane's results are 16 contiguous bytes,
// so the G output streams are stored straight from registers.
__global__ void pack_group_taps_kernel(const double *__restrict__ mi, const double *__restrict__ mq, const double *__restrict__ sp,
                                       int m, int F, double *__restrict__ w)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= m * F) return;
    const int i = idx / F, f = idx % F, k = m - 1 - i;
    w[idx] = f == 0 ? mi[k] : f == 1 ? mq[k] : sp[(size_t)(f - 2) * m + k];
}

// tg[4 i + f] = h_f[m - 1 - i], f = mark i, mark q, unit-gain space i, space q: the sliding sums' templates as one table (afsk_fused8_kernel)
__global__ void pack_templates_kernel(const double *__restrict__ mi, const double *__restrict__ mq, const double *__restrict__ ui, const double *__restrict__ uq, int m,
                                      double *__restrict__ tg)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 4 * m) return;
    const int i = idx >> 2, f = idx & 3, k = m - 1 - i;
    tg[idx] = f == 0 ? mi[k] : f == 1 ? mq[k] : f == 2 ? ui[k] : uq[k];
}

template <int G, bool VEC>
__global__ __launch_bounds__(kThreads) void afsk_group_kernel(const double *__restrict__ x, int64_t n, const double *__restrict__ w,
                                                              int m, double *__restrict__ y, int64_t y_stride, int64_t nout,
                                                              const int *__restrict__ gate = nullptr, int gate_above = 0)
{
    extern __shared__ double xs[];
    if (gate && *gate <= gate_above) return;                          // see fir_signs_batch_kernel
    constexpr int R = 2, F = 2 + 2 * G, T = kThreads * R;
    const int t = threadIdx.x;
    const int span = T + m - 1;
    const double *const w_all = w;
    for (int64_t tile = blockIdx.x; tile * T < nout; tile += gridDim.x) {     // one trip, except for a gated launch's small grid
    w = w_all;
    const int64_t tile0 = tile * T;
    if (VEC) {
        stage_vec<R>(x, n, tile0, span, t, xs);
    } else {
        for (int idx = t; idx < span; idx += kThreads) {
            int64_t gi = tile0 + idx;
            xs[slot<R>(idx)] = gi < n ? x[gi] : 0.0;
        }
    }
    lds_barrier();

    double acc[F][R];
#pragma unroll
    for (int f = 0; f < F; ++f)
#pragma unroll
        for (int r = 0; r < R; ++r) acc[f][r] = 0.0;
    const double *lp = xs + t * (R + 1);       // block b of this lane's window: lp[b * (R + 1) + 0 .. R-1]
    double A[R], B[R];
#pragma unroll
    for (int q = 0; q < R; ++q) A[q] = lp[q];
#define PM_GROUP_BLOCK(CUR, NXT, TAPS)                                                             \
    {                                                                                              \
        _Pragma("unroll") for (int q = 0; q < R; ++q) NXT[q] = lp[(R + 1) + q];                    \
        _Pragma("unroll") for (int q = 0; q < TAPS; ++q) {                                         \
            _Pragma("unroll") for (int f = 0; f < F; ++f) {                                        \
                const double g = w[q * F + f];                                                     \
                _Pragma("unroll") for (int r = 0; r < R; ++r) {                                    \
                    const double v = (q + r < R) ? CUR[q + r] : NXT[q + r - R];                    \
                    acc[f][r] = __builtin_fma(g, v, acc[f][r]);                                    \
                }                                                                                  \
            }                                                                                      \
        }                                                                                          \
        lp += R + 1;                                                                               \
        w += TAPS * F;                                                                             \
    }
    int i0 = 0;
    for (; i0 + 2 * R <= m; i0 += 2 * R) {
        PM_GROUP_BLOCK(A, B, R)
        PM_GROUP_BLOCK(B, A, R)
    }
    if (i0 + R <= m) {
        PM_GROUP_BLOCK(A, B, R)
        i0 += R;
#pragma unroll
        for (int q = 0; q < R; ++q) A[q] = B[q];
    }
    if (i0 < m) PM_GROUP_BLOCK(A, B, 1)       // R = 2: at most one tap left
#undef PM_GROUP_BLOCK
    static_assert(R == 2, "tail and stores are written for two outputs per thread");

    const int64_t go = tile0 + (int64_t)t * R;
    double mark[R];
#pragma unroll
    for (int r = 0; r < R; ++r) mark[r] = __builtin_sqrt(acc[0][r] * acc[0][r] + acc[1][r] * acc[1][r]);
#pragma unroll
    for (int g = 0; g < G; ++g) {
        double o[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const double si = acc[2 + 2 * g][r], sq = acc[3 + 2 * g][r];
            o[r] = mark[r] - __builtin_sqrt(si * si + sq * sq);          // afsk.py:153-162
        }
        double *yg = y + (size_t)g * y_stride;
        if (VEC && go + 1 < nout) {
            *reinterpret_cast<double2v *>(yg + go) = double2v{o[0], o[1]};
        } else {
            if (go < nout) yg[go] = o[0];
            if (go + 1 < nout) yg[go + 1] = o[1];
        }
    }
    lds_barrier();                                                   // the next tile restages the LDS image
    }
}

// ---- gain sweep: G AFSK modems that differ in space_gain only, sign bitmaps certified against the exact chain --------------------
// The chains of afsk_1200_ax25_super_opt.json share tones and span and sweep space_gain, which the reference folds into the space
// taps (afsk.py:144-145: taps_g = fl(g * c)).  In exact arithmetic chain g's output is LPF(M) - g * LPF(S), with M the mark
// magnitude and S the space magnitude for the UNIT taps c -- two correlator pairs and two low-passes for the whole sweep instead
// of 2 + 2G pairs and G low-passes.  In binary64 the two routes differ by rounding only, and the slicer reads nothing but the sign:
//     y~_g = fma(-g, B, A),  A = LPF(M), B = LPF(S)   (both by the canonical kernels)
// satisfies |y~_g - y_g| <= E for the bound below, so wherever |y~_g| > E the sign of the exact chain's output y_g is the sign of
// y~_g, and the few samples with |y~_g| <= E are recomputed by the exact chain itself (every fma in its canonical order, one thread
// per sample).  Every bit of every bitmap is therefore the bit the exact kernels write; tests compare them over whole recordings.
//
// Bound.  u = 2^-53, mc / ml = correlator / low-pass taps, X >= max|x|.  Space sums: the taps differ by relative u and each chain of
// mc fmas has relative error <= mc u/(1 - mc u) in sum|t x|, so |sum_g - g sum_1| <= (2 mc + 2) u g mc X; the magnitude sqrt(a^2+b^2)
// is 1-Lipschitz in (a, b) and adds 3 roundings, so |space_g - g S| <= (2 mc + 6) sqrt2 u g mc X; y = M - space adds u |y|.  The
// low-pass is linear up to (ml + 2) u sum|h|(|M| + g|S|) of its own rounding (three canonical sums), and fma(-g, B, A) adds one
// more.  With |M|, |S| <= sqrt2 mc X everything is below  (2 mc + ml + 12) * 2.9 u * sum|h| (1 + g) mc X  ~ 1e-13 * scale; E is
// taken as 1e-10 * sum|h| (1 + g_max) mc sqrt2 X, a thousand times that, which still flags only ~1e-8 of the samples.
constexpr int kSweepMax = 8;
struct SweepArgs {
    double gain[kSweepMax];
    uint64_t *bits[kSweepMax];
};

// The combine step of a thread's R = 8 consecutive outputs: y_g = A - g B (ONE: y = A as it stands), one bitmap byte per modem, and
// the (sample, modem) pairs that cannot be certified (|y| <= E, NaN too) to the list, whose bits sweep_exact_kernel decides afterwards.
// A wave whose outputs all lie inside the stream and are all certified -- all but one in ~1e5 -- spends three vector instructions per
// output and modem: the fma, the sign bit shifted into the byte from the high word (v_alignbit; y != 0 there, so the sign bit is
// `y >= 0` negated) and one compare whose lane mask is folded into a scalar; otherwise the wave goes through its modems once more, lane
// by lane (same bytes for the certified outputs).
template <int R, bool ONE>
__device__ __forceinline__ void sweep_combine(const double (&a)[R], const double (&b)[R], int64_t go, int64_t nout, int G, const SweepArgs &P,
                                              double E, unsigned long long *__restrict__ list, int *__restrict__ count, int cap)
{
    static_assert(R == 8, "one bitmap byte per thread");
    const bool whole = __all(go + R <= nout);
    unsigned long long unsure_any = 0;
    if (whole) {
        for (int g = 0; g < G; ++g) {
            const double mg = -P.gain[g];
            unsigned neg = 0;
#pragma unroll
            for (int r = R - 1; r >= 0; --r) {
                const double y = ONE ? a[r] : __builtin_fma(mg, b[r], a[r]);
                neg = __builtin_amdgcn_alignbit(neg, (unsigned)__double2hiint(y), 31);      // (neg << 1) | sign bit
                unsure_any |= __ballot(!(fabs(y) > E));
            }
            reinterpret_cast<uint8_t *>(P.bits[g])[go >> 3] = (uint8_t)~neg;
        }
        if (unsure_any == 0) return;
    }
    for (int g = 0; g < G; ++g) {                            // the stream's last outputs, or something in this wave is uncertain
        const double mg = -P.gain[g];
        unsigned byte = 0, unsure = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const double y = ONE ? a[r] : __builtin_fma(mg, b[r], a[r]);
            const bool in = go + r < nout;
            byte |= (unsigned)(in && y >= 0.0) << r;
            unsure |= (unsigned)(in && !(fabs(y) > E)) << r;                 // cannot be certified (NaN lands here too)
        }
        reinterpret_cast<uint8_t *>(P.bits[g])[go >> 3] = (uint8_t)byte;     // bits past nout: 0 up to the end of the last word
        while (unsure) {
            const int r = __ffs((int)unsure) - 1;
            unsure &= unsure - 1;
            const int idx = atomicAdd(count, 1);
            if (idx < cap) list[idx] = ((unsigned long long)g << 48) | (unsigned long long)(go + r);
        }
    }
}

// The second low-pass of the sweep with the combine step as its epilogue: B = LPF(S) stays in registers, A = LPF(M) is read back
// (the thread's eight consecutive values), and what leaves the kernel is one bitmap byte per modem and thread plus the list of
// samples that could not be certified.
template <int R, bool VEC>
__global__ __launch_bounds__(kThreads) void fir_sweep_kernel(const double *__restrict__ S, int64_t n, const double *__restrict__ h, int m,
                                                             const double *__restrict__ A, int64_t nout, int G, SweepArgs P, double E,
                                                             unsigned long long *__restrict__ list, int *__restrict__ count, int cap)
{
    static_assert(R == 8, "one bitmap byte per thread");
    double b[R];
    fir_tile_acc<double, R, VEC>(S, n, h, m, (int64_t)blockIdx.x, b);
    const int64_t go = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * R;
    if (go >= ((nout + 63) >> 6) * 64) return;
    double a[R];
#pragma unroll
    for (int r = 0; r < R; ++r) a[r] = A && go + r < nout ? A[go + r] : 0.0;
    if (A) sweep_combine<R, false>(a, b, go, nout, G, P, E, list, count, cap);
    else sweep_combine<R, true>(b, b, go, nout, G, P, E, list, count, cap);      // no A: the input already is mark - gain * space (one chain)
}

// Sliding sums, low-pass(es) and the certified combine in ONE kernel: the magnitude streams never reach memory.  A workgroup owns
// 2048 low-pass outputs; it needs the ml - 1 magnitudes past them too, computes all of them as runs of L = 12 from one staged window of
// x (the first ceil((2047 + ml) / L) lanes do, e.g. 179 of 256 for ml = 100: three waves with short runs beat two with long ones), lays them out as the FIR's padded LDS images -- the
// space image over the window of x, which is dead by then -- and every thread takes its 8 outputs of each low-pass from there.
// ONE: a single chain, its mark - gain * space difference as the only image.  Arithmetic and bound: afsk_slide_kernel + fir_valid_kernel
// + fir_sweep_kernel, value for value.  LDS: fuse_region0 / fuse_image / fuse_lds_bytes (pm_afsk_sweep.h).
template <bool ONE, int L = kFuseRun>
__global__ __launch_bounds__(kThreads) void afsk_slide_lpf_kernel(const double *__restrict__ x, int64_t n, const double *__restrict__ mi,
                                                                  const double *__restrict__ mq, const double *__restrict__ ui,
                                                                  const double *__restrict__ uq, int m, SlideTones T,
                                                                  const double *__restrict__ h, int ml, int64_t nout, int G, SweepArgs P, double E,
                                                                  unsigned long long *__restrict__ list, int *__restrict__ count, int cap,
                                                                  int region0, int image)
{
    extern __shared__ double xs[];
    constexpr int R = 8, TILE = kThreads * R;
    const int t = threadIdx.x;
    const int64_t tile0 = (int64_t)blockIdx.x * TILE;
    const int nmag = TILE + ml - 1, nruns = (nmag + L - 1) / L, xspan = nruns * L + m - 1;
    double *im = xs + region0, *tp = im + image;
    if (((uintptr_t)x & 15) == 0 && tile0 + TILE <= n) {
        double2v v[R / 2];
#pragma unroll
        for (int q = 0; q < R / 2; ++q) v[q] = *reinterpret_cast<const double2v *>(x + tile0 + 2 * (q * kThreads + t));
#pragma unroll
        for (int q = 0; q < R / 2; ++q) {
            const int s0 = slide_slot<L>(2 * (q * kThreads + t));
            xs[s0] = v[q].x;
            xs[s0 + 1] = v[q].y;
        }
        for (int p = TILE + t; p < xspan; p += kThreads) {
            const int64_t gi = tile0 + p;
            xs[slide_slot<L>(p)] = gi < n ? x[gi] : 0.0;
        }
    } else {
        for (int p = t; p < xspan; p += kThreads) {
            const int64_t gi = tile0 + p;
            xs[slide_slot<L>(p)] = gi < n ? x[gi] : 0.0;
        }
    }
    for (int i = t; i < m; i += kThreads) {
        tp[4 * i + 0] = mi[m - 1 - i];
        tp[4 * i + 1] = mq[m - 1 - i];
        tp[4 * i + 2] = ui[m - 1 - i];
        tp[4 * i + 3] = uq[m - 1 - i];
    }
    lds_barrier();
    double mv[L], sv[L];
    if (t < nruns) slide_run<L>(xs, tp, t, m, T, mv, sv);
    lds_barrier();                                           // every lane is done with the window of x
    if (t < nruns) {
        const double g0 = P.gain[0];
#pragma unroll
        for (int i = 0; i < L; ++i) {
            const int p = t * L + i;
            if (p < nmag) {
                if (ONE) {
                    im[slot<R>(p)] = __builtin_fma(-g0, sv[i], mv[i]);       // afsk.py:162 on the approximate magnitudes
                } else {
                    im[slot<R>(p)] = mv[i];
                    xs[slot<R>(p)] = sv[i];
                }
            }
        }
    }
    lds_barrier();
    double a[R], b[R];
    fir_acc_image<R>(im, h, ml, a);
    if (!ONE) fir_acc_image<R>(xs, h, ml, b);
    const int64_t go = tile0 + (int64_t)t * R;
    if (go >= ((nout + 63) >> 6) * 64) return;
    sweep_combine<R, ONE>(a, b, go, nout, G, P, E, list, count, cap);
}

// The exact chain for single samples needs to know where the sweep's input came from.  AUDIO (src.audio != nullptr): the band-passed
// stream the sweep saw was itself a value with a bound (pm_bpf8.hip), so the recomputation starts one stage earlier -- the mc + ml - 1
// band-pass outputs under the entry from the int16 audio, the reference's sum in fir_valid_kernel's order.
struct SweepSource {
    const int16_t *audio;            // nullptr: d_x is the reference's band-passed stream
    const double *bpf;
    int mb;
    double e_x;                      // |d_x[k] - reference's band-pass output|
};

// What the fused matrix-pipe kernel needs to decide its own uncertain samples (round 5): the exact chain's operands.
struct SweepTail {
    const double *space;             // the modems' own space taps (gain folded in, afsk.py:144-145): modem g at space + 2 g mc
    const double *lpf;               // the low-pass taps in binary64
    int lds_ok;                      // the exact chain's work space fits the kernel's LDS image: uncertain samples are decided in place
    SweepSource src;
};

// The exact chain of ONE (sample, modem) pair by a whole workgroup, every sum in the canonical order of fir_valid_kernel /
// afsk_correlate_kernel (sweep_exact_kernel below runs it per list entry, a wave each): the mc + ml - 1 band-pass outputs under the entry (one thread
// each, from the audio; or read from x), the ml correlator-bank outputs (one thread each, four sums side by side), the low-pass sum
// (thread 0).  `dd`: (2 ml + 2 mc + 2 mb - 2 + 4 mc + ...) doubles of LDS nobody else uses any more.  Ends with a barrier.
template <int THREADS>
__device__ __forceinline__ void sweep_tail_entry(double *__restrict__ dd, int t, const double *__restrict__ x, const double *__restrict__ mi,
                                                 const double *__restrict__ mq, const double *__restrict__ si, const double *__restrict__ sq, int mc,
                                                 const double *__restrict__ lpf, int ml, const SweepSource &src, int64_t k, unsigned long long *__restrict__ bits)
{
    const int nw = ml + mc - 1, mb = src.audio ? src.mb : 0, na = src.audio ? nw + mb - 1 : 0;
    double *xw = dd + ml, *aw = xw + nw, *tb = aw + na, *tc = tb + mb, *tl = tc + 4 * mc;
    if (src.audio) {
        for (int p = t; p < na; p += THREADS) aw[p] = (double)src.audio[k + p];
        for (int i = t; i < mb; i += THREADS) tb[i] = src.bpf[mb - 1 - i];
    } else {
        for (int p = t; p < nw; p += THREADS) xw[p] = x[k + p];
    }
    for (int i = t; i < mc; i += THREADS) {
        tc[4 * i + 0] = mi[mc - 1 - i];
        tc[4 * i + 1] = mq[mc - 1 - i];
        tc[4 * i + 2] = si[mc - 1 - i];
        tc[4 * i + 3] = sq[mc - 1 - i];
    }
    for (int i = t; i < ml; i += THREADS) tl[i] = lpf[ml - 1 - i];
    __syncthreads();
    if (src.audio) {
        for (int p = t; p < nw; p += THREADS) {
            // (unrolled: the operands of the next fmas are on their way from LDS while the chain waits for its own latency -- a
            // workgroup with an entry holds its slot for as long as this takes, and alone the kernel ends with its last such workgroup)
            double acc = 0.0;
#pragma unroll 8
            for (int i = 0; i < mb; ++i) acc = __builtin_fma(tb[i], aw[p + i], acc);
            xw[p] = acc;
        }
        __syncthreads();
    }
    for (int j = t; j < ml; j += THREADS) {
        double a = 0.0, b = 0.0, c = 0.0, d = 0.0;
#pragma unroll 4
        for (int i = 0; i < mc; ++i) {
            const double v = xw[j + i];
            a = __builtin_fma(tc[4 * i + 0], v, a);
            b = __builtin_fma(tc[4 * i + 1], v, b);
            c = __builtin_fma(tc[4 * i + 2], v, c);
            d = __builtin_fma(tc[4 * i + 3], v, d);
        }
        dd[j] = __builtin_sqrt(a * a + b * b) - __builtin_sqrt(c * c + d * d);
    }
    __syncthreads();
    if (t == 0) {
        double acc = 0.0;
#pragma unroll 8
        for (int j = 0; j < ml; ++j) acc = __builtin_fma(tl[j], dd[j], acc);
        unsigned long long *w = bits + (k >> 6);
        const unsigned long long bit = 1ull << (k & 63);
        if (acc >= 0.0) atomicOr(w, bit); else atomicAnd(w, ~bit);
    }
    __syncthreads();
}

// The same kernel with its low-passes on the int8 matrix pipe (v_mfma_i32_16x16x64_i8; the band-pass went there first: pm_bpf8.hip).
// The low-pass sums are 2/3 of afsk_slide_lpf_kernel's vector instructions and feed nothing but the certified decision, and the int8
// MFMA is the one matrix instruction that was measured to run BESIDE vector f64 work (tools/ubench/mfma_i8.hip).  So: the magnitudes a
// run leaves in registers are rounded to integers |X| <= 2^22 -- scaled by the power of two that fits the WORKGROUP's largest
// magnitude, so a quiet recording keeps its bits -- and written as three planes of signed base-256 digits; the taps come as three
// digits (pm_lpf8_plan: q = rint(h 2^S), |q| <= 2^22); a tile of 256 outputs is  out[16 i + j] = sum_c A[i][c] B[c][j],  A[i][c] = digit
// plane [tile + 16 i + c] (one ds_read_b128 per lane), B = the Toeplitz band of a tap digit -- 2 blocks x the 8 digit pairs of weight
// 256 and up = 16 MFMA per stream and tile, four int32 sums by weight, recombined exactly in binary64 (an integer below 2^50).
// The integer sums are exact, so what separates the value from the reference's low-pass output is  sum|h - q 2^-S| * the largest
// magnitude  +  2^-(S+s2) (sum|q| / 2 + the digit pair left out)  on top of E -- computed by the workgroup from its own scale
// (Ecmp).  Round 3 had 4 x 5 digits, all 20 pairs, and a scale fixed by the caller's bound on the audio: 40 MFMA per stream and tile,
// eight accumulators to clear and recombine, 20 uncertain decisions per recording; now several hundred of 230 M (the exact
// recomputation takes them in its stride) for 40 % of the matrix work and half of the recombination (profiles/r04_sweep_probe.txt;
// with the six pairs of weight 256^2 and up: 2600 uncertain decisions, and the exact kernel behind them cost what the matrix pipe saved).
// Lane (r, g) of a tile holds outputs 64 g + 16 v + r, v = 0..3: sign and bound tests become four ballots per modem, and the tile's
// four bitmap words are put together from their 16-bit pieces.
struct Lpf8Args {                        // Lpf8Consts (pm_afsk_sweep.h) and the plan's band table
    int S;
    double c_tap, c_q, gfac, qabs;
    const int4v *btab;
};
static_assert(kLanes == kThreads, "pm_afsk_sweep.h describes these kernels");

#ifndef PM_LPF8_F32MAG
#define PM_LPF8_F32MAG 1         // the sliding sums' roots in binary32 (slide_run_f32): g = 7 0.203 -> 0.188 ms, g = 1 0.133 -> 0.124, 752 -> 891 / 20 -> 221 uncertain decisions
#endif

#ifndef PM_LPF8_RECOMB32
#define PM_LPF8_RECOMB32 1       // pairs of accumulators recombined as 32-bit integers first (two conversions per output instead of four): 0.206 -> 0.203 ms
#endif
#ifndef PM_LPF8_WAVES
#define PM_LPF8_WAVES 4          // waves per SIMD the fused matrix-pipe kernel is compiled for (-DPM_LPF8_WAVES=5: measured, profiles/r04_lpf8_occupancy.txt)
#endif
// One workgroup's tile of a certified sweep from the band-passed window in LDS (xs, slide_slot layout): sliding sums, digit planes,
// low-pass(es) on the matrix pipe, certified combine -- the body of afsk_slide_lpf8_kernel, and of afsk_fused8_kernel once per sweep.
// planes: kL8Dig digit planes per stream (may lie over xs: nobody reads the window after the sliding sums); tp: 4 m doubles; bl: the
// band operands; wl: the workgroup's list of uncertain (sweep, modem, sample) entries, wl[kTailCap] their count; wmax8: 8 floats.
template <bool ONE>
__device__ __forceinline__ void lpf8_sweep_tile(double *__restrict__ xs, unsigned char *__restrict__ planes, double *__restrict__ tp, int4v *__restrict__ bl,
                                                unsigned *__restrict__ wl, float *__restrict__ wmax8, int sweep, bool lds_ok, int t, int64_t tile0,
                                                const double *__restrict__ mi, const double *__restrict__ mq, const double *__restrict__ ui,
                                                const double *__restrict__ uq, int m, const SlideTones &T, const Lpf8Args &Q, int ml, int64_t nout, int G,
                                                const SweepArgs &P, double E, unsigned long long *__restrict__ list, int *__restrict__ count, int cap,
                                                const double *tg = nullptr)
{
    constexpr int L = kFuseRun, TILE = kThreads * 8;
    const int nmag = TILE + ml - 1, nruns = (nmag + L - 1) / L;
    if (!tg)
        for (int i = t; i < m; i += kThreads) {
            tp[4 * i + 0] = mi[m - 1 - i];
            tp[4 * i + 1] = mq[m - 1 - i];
            tp[4 * i + 2] = ui[m - 1 - i];
            tp[4 * i + 3] = uq[m - 1 - i];
        }
    lds_barrier();
#if PM_LPF8_F32MAG
    float mv[L], sv[L];
    if (t < nruns) slide_run_f32<L>(xs, tp, t, m, T, mv, sv, tg);
    // the workgroup's largest value (what the planes will hold) and, for one stream, the largest mark + gain * space (what its roots'
    // errors scale with: the difference may be far smaller than either)
    float vmaxf = 0.0f, vsumf = 0.0f;
    if (t < nruns) {
        if (ONE) {
            const float g0 = (float)P.gain[0], ag0 = fabsf(g0);
#pragma unroll
            for (int i = 0; i < L; ++i) {
                vsumf = fmaxf(vsumf, fmaf(ag0, sv[i], mv[i]));
                mv[i] = fmaf(-g0, sv[i], mv[i]);             // afsk.py:162 on the approximate magnitudes
            }
        }
#pragma unroll
        for (int i = 0; i < L; ++i) vmaxf = fmaxf(vmaxf, ONE ? fabsf(mv[i]) : fmaxf(mv[i], sv[i]));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        vmaxf = fmaxf(vmaxf, __shfl_xor(vmaxf, off));
        if (ONE) vsumf = fmaxf(vsumf, __shfl_xor(vsumf, off));
    }
    float (*wmaxf)[kThreads / 64] = reinterpret_cast<float (*)[kThreads / 64]>(wmax8);      // (dynamic block: a static array would move its start)
    if ((t & 63) == 0) {
        wmaxf[0][t >> 6] = vmaxf;
        wmaxf[1][t >> 6] = vsumf;
    }
    lds_barrier();                                           // every lane is done with the window of x: the planes take its place
    static_assert(kThreads == 256, "four waves");
    const double vmax = (double)fmaxf(fmaxf(wmaxf[0][0], wmaxf[0][1]), fmaxf(wmaxf[0][2], wmaxf[0][3]));
    const double vsum = ONE ? (double)fmaxf(fmaxf(wmaxf[1][0], wmaxf[1][1]), fmaxf(wmaxf[1][2], wmaxf[1][3])) : vmax;
    int e2 = 0;
    (void)frexp(vmax, &e2);                                  // vmax < 2^e2
    // (not: NaN, infinities, all zeros, and what binary32 cannot carry: magnitudes below 2^-21 or above 2^60 -- everything goes to the list then)
    const bool scalable = vmax < 1.0e18 && vmax > 4.8e-7 && vsum < 1.0e18;
    const int s2 = scalable ? 22 - e2 : 0;
    const double scale = ldexp(1.0, s2);
    const float scalef = (float)scale;
    // A root is within (2^-23 + 2^-25) of itself of the true one (slide_run_f32), the one-stream difference adds the gain's and its own
    // binary32 roundings (2^-24 each, of mark + gain space at most): in units of the integers, per magnitude; 1e-6: vmax and vsum are
    // themselves rounded values
    const double root_units = (ONE ? 2.13 : 1.13) * 1.1920928955078125e-07 * (vsum * scale) * (1.0 + 1e-6) + 1e-5;
    // |sum h v - 2^-(S+s2) 256 val| <= sum|h - q 2^-S| vmax + 2^-(S+s2) (sum|q| (1/2 + the roots' share) + the product left out), times
    // 1 + gmax for a - g b; plus E, what separates sum h v from the reference's low-pass output: all in the units of `val`, rounded up
    const double Ecmp = scalable ? ceil((ldexp(E, Q.S + s2) + Q.gfac * (Q.c_tap * (vmax * scale) * (1.0 + 1e-6) + Q.c_q + Q.qabs * root_units)) *
                                        (1.0 + 1e-9) * (1.0 / 256.0)) + 2.0
                                 : __builtin_inf();
#else
    double mv[L], sv[L];
    if (t < nruns) slide_run<L>(xs, tp, t, m, T, mv, sv);
    // The largest magnitude of the workgroup (what the planes will hold): the digits are scaled to IT, not to the largest the audio
    // could produce -- a quiet recording keeps its 22 bits (round 4; a fixed scale cost a bit of certainty per halving of the level)
    double vmax = 0.0;
    if (t < nruns) {
        if (ONE) {
            const double g0 = P.gain[0];
#pragma unroll
            for (int i = 0; i < L; ++i) mv[i] = __builtin_fma(-g0, sv[i], mv[i]);       // afsk.py:162 on the approximate magnitudes
        }
#pragma unroll
        for (int i = 0; i < L; ++i) vmax = fmax(vmax, ONE ? fabs(mv[i]) : fmax(fabs(mv[i]), fabs(sv[i])));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) vmax = fmax(vmax, __shfl_xor(vmax, off));
    __shared__ double wmax[kThreads / 64];
    if ((t & 63) == 0) wmax[t >> 6] = vmax;
    lds_barrier();                                           // every lane is done with the window of x: the planes take its place
    vmax = fmax(fmax(wmax[0], wmax[1]), fmax(wmax[2], wmax[3]));
    static_assert(kThreads == 256, "four waves");
    int e2 = 0;
    (void)frexp(vmax, &e2);                                  // vmax < 2^e2 (0 for no signal at all)
    const bool scalable = vmax < 1.0e300 && vmax > 1.0e-280;  // (not: NaN, infinities, all zeros -- everything goes to the list then)
    const int s2 = scalable ? 22 - e2 : 0;
    const double scale = ldexp(1.0, s2);
    // |sum h v - 2^-(S+s2) 256 val| <= sum|h - q 2^-S| vmax + 2^-(S+s2) (sum|q| / 2 + the product left out), times 1 + gmax for
    // a - g b; plus E, what separates sum h v from the reference's low-pass output: all in the units of `val`, rounded up
    const double Ecmp = scalable ? ceil((ldexp(E, Q.S + s2) + Q.gfac * (Q.c_tap * (vmax * scale) + Q.c_q)) * (1.0 + 1e-9) * (1.0 / 256.0)) + 2.0
                                 : __builtin_inf();
#endif
    if (t < nruns) {
        static_assert(L % 4 == 0, "four magnitudes per plane word");
        auto put = [&](const auto (&val)[L], int stream) {
#pragma unroll
            for (int q = 0; q < L / 4; ++q) {
                unsigned w[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    // v 2^s2 is exact, |..| <= 2^22; adding 1.5 2^52 leaves its nearest integer in the low word (two's complement);
                    // the bytes of (X + 0x808080) ^ 0x808080 are X's three balanced base-256 digits
#if PM_LPF8_F32MAG
                    // (binary32: 1.5 2^23, the integer in the low 23 bits of the significand)
                    const float sc = scalable ? fmaf(val[4 * q + i], scalef, 12582912.0f) : 12582912.0f;
                    w[i] = ((unsigned)((int)__float_as_uint(sc) - 0x4B400000) + 0x808080u) ^ 0x808080u;
#else
                    const double sc = scalable ? __builtin_fma(val[4 * q + i], scale, 6755399441055744.0) : 6755399441055744.0;
                    w[i] = ((unsigned)__double2loint(sc) + 0x808080u) ^ 0x808080u;
#endif
                }
                const unsigned a01 = __builtin_amdgcn_perm(w[1], w[0], 0x05010400u), a23 = __builtin_amdgcn_perm(w[3], w[2], 0x05010400u);
                unsigned char *at = planes + (size_t)stream * kL8Dig * kL8Plane + L * t + 4 * q;
                *reinterpret_cast<unsigned *>(at) = __builtin_amdgcn_perm(a23, a01, 0x05040100u);
                *reinterpret_cast<unsigned *>(at + kL8Plane) = __builtin_amdgcn_perm(a23, a01, 0x07060302u);
                *reinterpret_cast<unsigned *>(at + 2 * kL8Plane) =
                    __builtin_amdgcn_perm(w[1], w[0], 0x0c0c0602u) | __builtin_amdgcn_perm(w[3], w[2], 0x06020c0cu);
            }
        };
        put(mv, 0);
        if (!ONE) put(sv, 1);
    }
    const int lane = t & 63, wave = t >> 6, r = lane & 15, g4 = lane >> 4;
    // the band operands (3 digits x 2 blocks x 64 lanes x 16 bytes) behind the templates
    for (int i = t; i < 2 * kL8Dig * 64; i += kThreads) bl[i] = Q.btab[i];
    lds_barrier();
    const int64_t nout64 = ((nout + 63) >> 6) * 64;
#pragma unroll 1
    for (int q = 0; q < 2; ++q) {
        const int tl = (wave * 2 + q) * 256;
        const int64_t go = tile0 + tl;
        if (go >= nout64) break;
        double a[4], b[4];
#pragma unroll
        for (int stream = 0; stream < (ONE ? 1 : 2); ++stream) {
            // the eight digit products of weight 256 and up (accumulator i + j - 1); the ninth, x_0 q_0, is bounded in c_q
            int4v acc[kL8Acc];
#pragma unroll
            for (int w = 0; w < kL8Acc; ++w) acc[w] = int4v{0, 0, 0, 0};
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                const unsigned char *at = planes + (size_t)stream * kL8Dig * kL8Plane + tl + 16 * r + 64 * kb + 16 * g4;
                int4v d[kL8Dig];
#pragma unroll
                for (int i = 0; i < kL8Dig; ++i) d[i] = *reinterpret_cast<const int4v *>(at + i * kL8Plane);
#pragma unroll
                for (int bb = 0; bb < kL8Dig; ++bb) {
                    const int4v band = bl[(bb * 2 + kb) * 64 + lane];
#pragma unroll
                    for (int i = 0; i < kL8Dig; ++i)
                        if (i + bb >= 1)
                            acc[i + bb - 1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(d[i], band, acc[i + bb - 1], 0, 0, 0);
                }
            }
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                // W_1 + 256 W_2 + 256^2 W_3 + 256^3 W_4, an integer below 2^50, exact: the pairs first, as 32-bit integers (ml <= 113
                // taps and at most three digit pairs per weight keep |W_w| below 5.6 M, so W + 256 W' stays inside 2^31) -- two
                // integer-to-double conversions per output instead of four (they are quarter-rate instructions)
#if PM_LPF8_RECOMB32
                const int lo = acc[0][v] + acc[1][v] * 256, hi = acc[2][v] + acc[3][v] * 256;
                const double val = __builtin_fma((double)hi, 65536.0, (double)lo);
#else
                const double val = __builtin_fma(__builtin_fma(__builtin_fma((double)acc[3][v], 256.0, (double)acc[2][v]), 256.0, (double)acc[1][v]), 256.0,
                                                 (double)acc[0][v]);
#endif
                if (stream == 0) a[v] = val; else b[v] = val;
            }
        }
        // lane (r, g4) holds outputs go + 64 g4 + 16 v + r
        const int64_t left = nout - go - (64 * g4 + r);
        const int lim = left > 1024 ? 1024 : (int)left;          // output v is inside the stream iff 16 v < lim
        unsigned long long in[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) in[v] = __ballot(16 * v < lim);
        for (int g = 0; g < G; ++g) {
            const double mg = -P.gain[g];
            double y[4];
            unsigned long long pos[4], uns = 0;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                y[v] = ONE ? a[v] : __builtin_fma(mg, b[v], a[v]);
                pos[v] = __ballot(y[v] >= 0.0) & in[v];
                uns |= ~__ballot(fabs(y[v]) > Ecmp) & in[v];                  // cannot be certified (NaN lands here too)
            }
            // the tile's four bitmap words from the 16-bit pieces of the four ballots: scalar arithmetic (the ballots are uniform), then
            // lane w < 4 picks word w -- with per-lane shifts of 64-bit values this was a dozen vector instructions per modem and tile
            // (putting the words together with scalar arithmetic and a select per lane, as fir8_kernel does for its one bitmap, was measured
            // here and is slower: seven modems' worth of 64-bit scalar shifts per tile, 0.233 against 0.206 ms -- profiles/r04_sweep_probe.txt)
            const int sh = 16 * (lane & 3);
            const unsigned lo = ((unsigned)(pos[0] >> sh) & 0xFFFFu) | ((unsigned)(pos[1] >> sh) << 16);
            const unsigned hi = ((unsigned)(pos[2] >> sh) & 0xFFFFu) | ((unsigned)(pos[3] >> sh) << 16);
            if (lane < 4 && go + 64 * lane < nout64)
                reinterpret_cast<unsigned long long *>(P.bits[g])[(go >> 6) + lane] = (unsigned long long)lo | ((unsigned long long)hi << 32);
            if (uns) {
#pragma unroll
                for (int v = 0; v < 4; ++v)
                    if (16 * v < lim && !(fabs(y[v]) > Ecmp)) {
                        const unsigned mine = lds_ok ? atomicAdd(&wl[kTailCap], 1u) : (unsigned)kTailCap;
                        if (mine < (unsigned)kTailCap) {
                            wl[mine] = ((unsigned)sweep << 20) | ((unsigned)g << 16) | (unsigned)(tl + 64 * g4 + 16 * v + r);
                        } else {
                            const int idx = atomicAdd(count, 1);
                            if (idx < cap) list[idx] = ((unsigned long long)g << 48) | (unsigned long long)(go + 64 * g4 + 16 * v + r);
                        }
                    }
            }
        }
    }
}

template <bool ONE>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(PM_LPF8_WAVES, PM_LPF8_WAVES))) void afsk_slide_lpf8_kernel(const double *__restrict__ x, int64_t n, const double *__restrict__ mi,
                                                                   const double *__restrict__ mq, const double *__restrict__ ui,
                                                                   const double *__restrict__ uq, int m, SlideTones T, Lpf8Args Q, int ml,
                                                                   int64_t nout, int G, SweepArgs P, double E, unsigned long long *__restrict__ list,
                                                                   int *__restrict__ count, int cap, int region0, SweepTail TL)
{
    extern __shared__ double xs[];
    constexpr int L = kFuseRun, TILE = kThreads * 8;
    const int t = threadIdx.x;
    const int64_t tile0 = (int64_t)blockIdx.x * TILE;
    const int nmag = TILE + ml - 1, nruns = (nmag + L - 1) / L, xspan = nruns * L + m - 1;
    double *tp = xs + region0;
    // the workgroup's own list of uncertain (sample, modem) pairs, decided by the exact chain before the workgroup ends (sweep_tail_entry):
    // behind the band operands in the dynamic block -- as a static array it moved the block's start off its 16-byte boundary (232 bytes
    // of static LDS) and every ds_read_b128 of the planes went the slow way: this kernel 0.33 -> 1.4 ms in the pipeline
    int4v *const bl = reinterpret_cast<int4v *>(tp + 4 * m);
    unsigned *const wl = reinterpret_cast<unsigned *>(bl + 2 * kL8Dig * 64);
    float *const wmax8 = reinterpret_cast<float *>(wl + kTailCap + 4);
    if (t == 0) wl[kTailCap] = 0;
    if (((uintptr_t)x & 15) == 0 && tile0 + TILE <= n) {
        double2v v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = *reinterpret_cast<const double2v *>(x + tile0 + 2 * (q * kThreads + t));
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int s0 = slide_slot<L>(2 * (q * kThreads + t));
            xs[s0] = v[q].x;
            xs[s0 + 1] = v[q].y;
        }
        for (int p = TILE + t; p < xspan; p += kThreads) {
            const int64_t gi = tile0 + p;
            xs[slide_slot<L>(p)] = gi < n ? x[gi] : 0.0;
        }
    } else {
        for (int p = t; p < xspan; p += kThreads) {
            const int64_t gi = tile0 + p;
            xs[slide_slot<L>(p)] = gi < n ? x[gi] : 0.0;
        }
    }
    lpf8_sweep_tile<ONE>(xs, reinterpret_cast<unsigned char *>(xs), tp, bl, wl, wmax8, 0, TL.lds_ok != 0, t, tile0, mi, mq, ui, uq, m, T, Q, ml, nout, G, P, E,
                         list, count, cap);
    // The workgroup's own uncertain samples, by the reference's chain, here: one in sixteen workgroups has one (750 + 220 per recording of
    // 28 000 workgroups), and it costs that workgroup a few microseconds -- as a launch of its own behind this one the same work sat on the demod
    // stream's critical path, twice per recording, waiting for slots among the other stream's workgroups (86 us per launch against 11 alone).
    __syncthreads();                                         // (vmcnt too: this workgroup's bitmap words are in memory before an atomic touches them)
    const int ne = (int)(wl[kTailCap] < (unsigned)kTailCap ? wl[kTailCap] : (unsigned)kTailCap);
    for (int e = 0; e < ne; ++e) {
        const unsigned ent = wl[e];
        const int g = (int)(ent >> 16) & 15;
        const double *si = TL.space + (size_t)g * 2 * m;
        sweep_tail_entry<kThreads>(xs, t, x, mi, mq, si, si + m, m, TL.lpf, ml, TL.src, tile0 + (int64_t)(ent & 0xFFFFu),
                                   reinterpret_cast<unsigned long long *>(P.bits[g]));
    }
}

// ---- ONE launch per recording for the AFSK stage of a chain group (round 5): band-pass, every sweep, every uncertain sample -------------
// Round 4's stage was three launches and 0.78 GB of traffic per recording: bpf8_kernel wrote the band-passed stream (230 MB of binary64),
// each of the two sweep kernels read it back -- an intermediate SURVEY 8(d) prices at zero.  Here a workgroup owns 2048 outputs of every
// sweep: it stages the int16 audio under them ONCE as digit planes, runs the band-pass on the matrix pipe (bpf8_kernel's arithmetic,
// pm_bpf8_dev.h) for the 2048 + (ml - 1) + (m - 1) values the longest sweep needs -- straight into the sliding sums' LDS window, never into
// memory -- then each sweep's tile from that window (lpf8_sweep_tile: the sweeps differ in tones, span and gains, not in their input),
// then the exact chain for whatever it could not certify.  What crosses HBM: 2 bytes per sample in, one bit per sample and chain out;
// the halo (mb + m + ml - 3 = 305 samples per 2048, 15 %) is band-passed twice, which costs 2 of the 9 + 16 + 8 matrix tiles per workgroup.
struct FusedSweep {
    const double *mi, *mq, *ui, *uq;     // templates (mark pair, unit-gain space pair)
    const double *space, *lpf;           // the exact chain's operands: the modems' own space taps, the low-pass in binary64
    const double *tg;                    // the four templates reversed and interleaved (pm_lpf8_plan::d_tpl): scalar loads in the sliding sums
    int m, ml, G, one;
    SlideTones T;
    Lpf8Args Q;
    SweepArgs P;
    double E;
    unsigned long long *list;
    int *count;
    int64_t nout;
};
struct FusedArgs {
    FusedSweep s[2];
    const int16_t *audio;
    int64_t n, nb;                       // samples; band-pass outputs (n - mb + 1)
    const pm_bpf8_dev::i4 *bp_btab;
    pm_bpf8_dev::Scales sc;
    SweepSource src;
    int xs_span;                         // band-passed values a workgroup needs: the largest runs * L + m - 1 of the sweeps
    int aplane;                          // bytes of an audio digit plane
    int xw_doubles, plane_bytes, mmax;   // LDS layout: window | planes | templates | band operands | list | maxima
    int lds_ok, cap;
};

#ifndef PM_FUSED8_WAVES
#define PM_FUSED8_WAVES 5       // compiled for five waves per SIMD (96 registers): the LDS block admits four workgroups, and four of its waves then leave a SIMD room for a slicer wave (slice_walk_kernel: 88 registers) beside them
#endif
template <int KB, bool ONE0, int NS, bool ONE1>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(PM_FUSED8_WAVES, PM_FUSED8_WAVES))) void afsk_fused8_kernel(FusedArgs A)
{
    extern __shared__ double xs[];
#if defined(PM_FUSED8_PRIO) && PM_FUSED8_PRIO > 0
    __builtin_amdgcn_s_setprio(PM_FUSED8_PRIO);              // (measurement builds: this kernel's waves above the slicers' walkers at the issue port -- profiles/r05_executor_knobs.txt)
#endif
    constexpr int L = kFuseRun, TILE = kThreads * 8;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t tile0 = (int64_t)blockIdx.x * TILE;
    unsigned char *const planes = reinterpret_cast<unsigned char *>(xs + A.xw_doubles);
    double *const tp = reinterpret_cast<double *>(planes + A.plane_bytes);
    int4v *const bl = reinterpret_cast<int4v *>(tp + 4 * A.mmax);
    unsigned *const wl = reinterpret_cast<unsigned *>(bl + 2 * kL8Dig * 64);
    float *const wmax8 = reinterpret_cast<float *>(wl + kTailCap + 4);
    if (t == 0) wl[kTailCap] = 0;
    // the audio under the workgroup as two digit planes (in the low-pass planes' place: those come later); the band's operands come from
    // the plan's table block by block (in registers for the kernel's life they took it from 97 to 121: no room left on a SIMD for a
    // slicer wave beside four of these, and the slicers are the other half of the pipeline)
    unsigned char *const ap0 = planes, *const ap1 = planes + A.aplane;
    pm_bpf8_dev::stage_planes_rt(A.audio, A.n, tile0, t, kThreads, ap0, ap1, A.aplane);
    {
        lds_barrier();
        // band-pass tiles of 256 values, waves taking turns, into the window (positions past the stream: 0.0, as the split kernels stage them)
        const int r = lane & 15, g = lane >> 4;
        const int ntiles = (A.xs_span + 255) >> 8;
        for (int q = wave; q < ntiles; q += kThreads / 64) {
            double val[4];
            const pm_bpf8_dev::i4 *bt = A.bp_btab;
            asm volatile("" : "+s"(bt));                     // (opaque per tile: hoisted out of this loop the operands are 48 registers again)
            pm_bpf8_dev::tile_values_tab<KB, 4>(ap0, ap1, bt, q * 256, lane, A.sc, val);
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int p = q * 256 + 16 * (4 * g + v) + r;
                if (p < A.xs_span) xs[slide_slot<L>(p)] = tile0 + p < A.nb ? val[v] : 0.0;
            }
        }
    }
    lds_barrier();
    {
        const FusedSweep &S = A.s[0];
        if (tile0 < ((S.nout + 63) >> 6) * 64)               // (uniform: a sweep with a longer correlator has fewer outputs)
            lpf8_sweep_tile<ONE0>(xs, planes, tp, bl, wl, wmax8, 0, A.lds_ok != 0, t, tile0, S.mi, S.mq, S.ui, S.uq, S.m, S.T, S.Q, S.ml, S.nout, S.G, S.P, S.E,
                                  S.list, S.count, A.cap, S.tg);
    }
    if (NS == 2) {
        lds_barrier();                                       // every wave is through with the first sweep's templates, planes and band
        const FusedSweep &S = A.s[1];
        if (tile0 < ((S.nout + 63) >> 6) * 64)
            lpf8_sweep_tile<ONE1>(xs, planes, tp, bl, wl, wmax8, 1, A.lds_ok != 0, t, tile0, S.mi, S.mq, S.ui, S.uq, S.m, S.T, S.Q, S.ml, S.nout, S.G, S.P, S.E,
                                  S.list, S.count, A.cap, S.tg);
    }
    // the workgroup's own uncertain samples, by the reference's chain from the audio (see afsk_slide_lpf8_kernel)
    __syncthreads();
    const int ne = (int)(wl[kTailCap] < (unsigned)kTailCap ? wl[kTailCap] : (unsigned)kTailCap);
    for (int e = 0; e < ne; ++e) {
        const unsigned ent = wl[e];
        const int g = (int)(ent >> 16) & 15;
        const int64_t k = tile0 + (int64_t)(ent & 0xFFFFu);
        if (NS == 1 || (ent >> 20) == 0) {
            const FusedSweep &S = A.s[0];
            const double *si = S.space + (size_t)g * 2 * S.m;
            sweep_tail_entry<kThreads>(xs, t, nullptr, S.mi, S.mq, si, si + S.m, S.m, S.lpf, S.ml, A.src, k, reinterpret_cast<unsigned long long *>(S.P.bits[g]));
        } else {
            const FusedSweep &S = A.s[1];
            const double *si = S.space + (size_t)g * 2 * S.m;
            sweep_tail_entry<kThreads>(xs, t, nullptr, S.mi, S.mq, si, si + S.m, S.m, S.lpf, S.ml, A.src, k, reinterpret_cast<unsigned long long *>(S.P.bits[g]));
        }
    }
}

// every sweep's counter into its page-locked word, and the counters back to zero for the block's next recording (the fused launch has
// no band-pass kernel in front of it to clear them); `keep` holds the counts for whoever works a list off later
__global__ void sweep_mail_reset_kernel(int *__restrict__ count, int *__restrict__ keep, int *__restrict__ mail, int n)
{
    if ((int)threadIdx.x < n) {
        const int c = count[threadIdx.x];
        keep[threadIdx.x] = c;
        mail[threadIdx.x] = c;
        count[threadIdx.x] = 0;
    }
    __threadfence_system();
}

// The exact chain for single samples: correlator bank of modem g at the ml positions the low-pass needs, then the low-pass, every
// sum in the canonical order of afsk_correlate_kernel / fir_valid_kernel.  Runs after fir_sweep_kernel (its bitmap bytes are final).
// AUDIO: the band-passed stream the sweep saw was itself a value with a bound (pm_bpf8.hip), so the recomputation starts one stage
// earlier -- the mc + ml - 1 band-pass outputs under the entry from the int16 audio, the reference's sum in fir_valid_kernel's order:
// sweep_tail_entry with the wave as its workgroup (LDS: sweep_tail_doubles).
template <bool AUDIO>
__global__ __launch_bounds__(64) void sweep_exact_kernel(const double *__restrict__ x, const double *__restrict__ mi, const double *__restrict__ mq,
                                                         const double *__restrict__ space, int mc, const double *__restrict__ lpf, int ml,
                                                         SweepArgs P, const unsigned long long *__restrict__ list, const int *__restrict__ count, int cap,
                                                         int *__restrict__ reset, int *__restrict__ mail, SweepSource src)
{
    // deferred fallback (pm_afsk_sweep_mode): this is the sweep's last launch and clears the next sweep's counter (see d_sweep);
    // it also leaves the counter in a page-locked host word, so that the caller who waits for the recording's event anyway reads it
    // without a copy and a stream wait of its own
#ifndef PM_EXACT_PRIO
#define PM_EXACT_PRIO 3
#endif
    // a few hundred lone waves, each a chain of dependent sums, between a recording's two sweeps on the demod stream: every issue slot
    // they lose to the filter and slicer waves beside them is time the whole recording waits (measured in the pipeline: 0.10 ms per
    // launch at the default priority against 0.011 alone)
    __builtin_amdgcn_s_setprio(PM_EXACT_PRIO);
    if (reset && blockIdx.x == 0 && threadIdx.x == 0) *reset = 0;
    if (mail && blockIdx.x == 0 && threadIdx.x == 0) {
        *mail = *count;
        __threadfence_system();
    }
    // One wave per listed sample: the ml correlator-bank outputs the low-pass needs are independent of each other and go to the
    // lanes (each in the canonical tap order); the low-pass sum itself is sequential and stays with lane 0.  (One LANE per sample
    // took 0.25-0.5 ms for a single entry -- 4 mc ml dependent fmas -- and the demod stream waits for it.)
    extern __shared__ double dd[];
    const int lane = threadIdx.x;
    const int cnt = min(*count, cap);
    for (int e = blockIdx.x; e < cnt; e += gridDim.x) {
        const int g = (int)(list[e] >> 48);
        const int64_t k = (int64_t)(list[e] & 0xFFFFFFFFFFFFull);
        if (g >= kSweepMax || P.bits[g] == nullptr) continue;                    // not an entry of this sweep (cannot happen: see sweep_signs)
        const double *si = space + (size_t)g * 2 * mc, *sq = si + mc;
        if (AUDIO) {
            sweep_tail_entry<64>(dd, lane, x, mi, mq, si, sq, mc, lpf, ml, src, k, reinterpret_cast<unsigned long long *>(P.bits[g]));
            continue;
        }
        for (int j = lane; j < ml; j += 64) {
            const double *xp = x + k + j;
            double a = 0.0, b = 0.0, c = 0.0, d = 0.0;
            for (int t = 0; t < mc; ++t) {
                const double v = xp[t];
                a = __builtin_fma(mi[mc - 1 - t], v, a);
                b = __builtin_fma(mq[mc - 1 - t], v, b);
                c = __builtin_fma(si[mc - 1 - t], v, c);
                d = __builtin_fma(sq[mc - 1 - t], v, d);
            }
            const double mark = __builtin_sqrt(a * a + b * b);
            const double spc = __builtin_sqrt(c * c + d * d);
            dd[j] = mark - spc;
        }
        __syncthreads();
        if (lane == 0) {
            double acc = 0.0;
            for (int j = 0; j < ml; ++j) acc = __builtin_fma(lpf[ml - 1 - j], dd[j], acc);
            unsigned long long *w = reinterpret_cast<unsigned long long *>(P.bits[g]) + (k >> 6);
            const unsigned long long bit = 1ull << (k & 63);
            if (acc >= 0.0) atomicOr(w, bit); else atomicAnd(w, ~bit);
        }
        __syncthreads();
    }
}

// ---- what slide_run_f32 relies on: v_sqrt_f32 within one unit in the last place, for EVERY significand ---------------------------------
// All 2^23 significands of the binades 2^e and 2^(e+1) (a root's significand depends on the radicand's significand and on the parity of
// its exponent only): the largest |v_sqrt_f32(x) - sqrt(x)| in units of the result's last place, sqrt(x) in binary64 (correctly rounded,
// 29 bits to spare).  *h_worst_ulp_1024 = that, times 1024, rounded up.
__global__ __launch_bounds__(256) void sqrt_f32_ulp_kernel(int e, unsigned long long *worst)
{
    const unsigned k = blockIdx.x * 256u + threadIdx.x;       // 2^24 threads: significand k & (2^23 - 1), exponent e + (k >> 23)
    const unsigned bits = ((unsigned)(e + (int)(k >> 23) + 127) << 23) | (k & 0x7FFFFFu);
    const float x = __uint_as_float(bits);
    const float r = __builtin_amdgcn_sqrtf(x);
    const double exact = __builtin_sqrt((double)x);
    int re = 0;
    (void)frexp((double)r, &re);                              // r = f 2^re, f in [0.5, 1): its last place is 2^(re - 24)
    const double ulps = fabs((double)r - exact) * ldexp(1.0, 24 - re);
    unsigned long long mine = (unsigned long long)ceil(ulps * 1024.0);
    if (!(ulps == ulps)) mine = ~0ull;
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(mine, off);
        mine = o > mine ? o : mine;
    }
    if ((threadIdx.x & 63) == 0) atomicMax(worst, mine);
}

}  // namespace

template <int G>
static int afsk_group_go(pm_ctx *ctx, const double *d_x, int64_t n, const double *d_w, int m, double *d_y, int64_t y_stride, int64_t nout,
                         const int *gate = nullptr, int gate_above = 0)
{
    constexpr int R = 2;
    const int64_t ntiles = pm_cdiv(nout, (int64_t)kThreads * R);
    PM_ARG(ntiles < (1LL << 31));
    const size_t lds = lds_bytes<R>(m) + 4 * (R + 1) * sizeof(double);        // the last block's look-ahead load
    const bool vec = ((((uintptr_t)d_x | (uintptr_t)d_y) & 15) == 0) && (y_stride % 2 == 0);
    // a gated launch (the certified path's overflow fallback, normally every workgroup leaves at once) is booked with the
    // fallback machinery, not with the correlators
    PmProf prof(ctx, gate ? PM_K_SIGNS : PM_K_AFSK_CORR);
    if (!gate) prof.work((double)n * 8 + (double)G * nout * 8, 2.0 * (2 + 2 * G) * m * (double)nout);
    const unsigned grid = (unsigned)(gate ? std::min<int64_t>(ntiles, kGatedGrid) : ntiles);
    auto go = [&](auto kernel) -> int {
        if (int rc = allow_lds(kernel, lds)) return rc;
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(kThreads), lds, ctx->stream, d_x, n, d_w, m, d_y, y_stride, nout, gate, gate_above);
        return PM_OK;
    };
    if (int rc = vec ? go(afsk_group_kernel<G, true>) : go(afsk_group_kernel<G, false>)) return rc;
    PM_HIP(hipGetLastError());
    return PM_OK;
}

static int afsk_group_dispatch(pm_ctx *ctx, int groups, const double *d_x, int64_t n, const double *d_w, int m, double *d_y, int64_t y_stride,
                               int64_t nout, const int *gate = nullptr, int gate_above = 0)
{
#define PM_GROUP_GO(G) case G: return afsk_group_go<G>(ctx, d_x, n, d_w, m, d_y, y_stride, nout, gate, gate_above);
    switch (groups) { PM_GROUP_GO(1) PM_GROUP_GO(2) PM_GROUP_GO(3) PM_GROUP_GO(4) PM_GROUP_GO(5) PM_GROUP_GO(6) PM_GROUP_GO(7) }
#undef PM_GROUP_GO
    return afsk_group_go<8>(ctx, d_x, n, d_w, m, d_y, y_stride, nout, gate, gate_above);
}

static SlideTones slide_tones(const pm_afsk_tones *t)
{
    return SlideTones{t->mark_rot[0], t->mark_rot[1], t->mark_end[0], t->mark_end[1], t->space_rot[0], t->space_rot[1], t->space_end[0], t->space_end[1]};
}

// the gains and bitmaps of a sweep's modems as the kernels take them, and the largest gain; false: a bitmap is missing or a gain out of range
static bool sweep_args(const double *h_gains, uint64_t *const *h_bits, int groups, SweepArgs *P, double *gmax)
{
    memset(P, 0, sizeof(*P));
    *gmax = 0.0;
    for (int g = 0; g < groups; ++g) {
        if (!h_bits[g] || !(h_gains[g] >= 0.0 && h_gains[g] < 1e100)) return false;
        P->gain[g] = h_gains[g]; P->bits[g] = h_bits[g];
        *gmax = std::max(*gmax, h_gains[g]);
    }
    return true;
}

static Lpf8Args lpf8_args(const pm_lpf8_plan *q, double gmax, bool one)
{
    const Lpf8Consts c = lpf8_consts(q->S, q->tapq_int, q->qabs, q->dlow, gmax, one);
    return Lpf8Args{c.S, c.c_tap, c.c_q, c.gfac, c.qabs, (const int4v *)q->d_btab};
}

// every sweep's count into its page-locked word behind the recording's last sweep, and the counters back to zero
static int sweep_mail_reset(pm_ctx *ctx, const pm_sweep_cells *cells, int nsweeps)
{
    hipLaunchKernelGGL(sweep_mail_reset_kernel, dim3(1), dim3(64), 0, ctx->stream, cells->d_count, cells->d_count + nsweeps, cells->h_mail, nsweeps);
    PM_HIP(hipGetLastError());
    return PM_OK;
}

extern "C" {

int pm_afsk_correlate(pm_ctx *ctx, const double *d_x, int64_t n, const double *d_mark_i, const double *d_mark_q,
                      const double *d_space_i, const double *d_space_q, int m, double *d_y)
{
    PM_CTX(ctx);
    PM_ARG(ctx && d_x && d_mark_i && d_mark_q && d_space_i && d_space_q && d_y);
    PM_ARG(m >= 1 && m <= kMaxTaps);
    PM_ARG(n >= m);
    constexpr int R = 4;
    const int64_t nout = n - m + 1;
    const int64_t ntiles = pm_cdiv(nout, (int64_t)kThreads * R);
    PM_ARG(ntiles < (1LL << 31));
    const size_t lds = lds_bytes<R>(m);
    PmProf prof(ctx, PM_K_AFSK_CORR);
    prof.work((double)n * 8 + (double)nout * 8, 2.0 * 4 * m * (double)nout);
    const bool vec = (((uintptr_t)d_x | (uintptr_t)d_y) & 15) == 0;
    auto go = [&](auto kernel) -> int {
        if (int rc = allow_lds(kernel, lds)) return rc;
        hipLaunchKernelGGL(kernel, dim3((unsigned)ntiles), dim3(kThreads), lds, ctx->stream, d_x, n, d_mark_i, d_mark_q, d_space_i, d_space_q, m, d_y, nout, (double *)nullptr);
        return PM_OK;
    };
    if (int rc = vec ? go(afsk_correlate_kernel<R, true>) : go(afsk_correlate_kernel<R, false>)) return rc;
    PM_HIP(hipGetLastError());
    return PM_OK;
}

int pm_afsk_correlate_group(pm_ctx *ctx, const double *d_x, int64_t n, const double *d_mark_i, const double *d_mark_q,
                            const double *d_space, int groups, int m, double *d_y, int64_t y_stride)
{
    PM_CTX(ctx);
    PM_ARG(d_x && d_mark_i && d_mark_q && d_space && d_y);
    PM_ARG(groups >= 1 && groups <= PM_AFSK_GROUP_MAX);
    PM_ARG(m >= 1 && m <= kMaxTaps);
    PM_ARG(n >= m);
    const int64_t nout = n - m + 1;
    PM_ARG(groups == 1 || y_stride >= nout);
    const int F = 2 + 2 * groups;
    if (int rc = pm_scratch_reserve(ctx, (size_t)F * m * sizeof(double))) return rc;
    double *d_w = (double *)ctx->d_scratch;
    hipLaunchKernelGGL(pack_group_taps_kernel, dim3((unsigned)pm_cdiv((int64_t)F * m, 256)), dim3(256), 0, ctx->stream,
                       d_mark_i, d_mark_q, d_space, m, F, d_w);
    PM_HIP(hipGetLastError());
    return afsk_group_dispatch(ctx, groups, d_x, n, d_w, m, d_y, y_stride, nout);
}

// M = |mark correlators|, S = |unit-gain space correlators| over x, one stream each (nc = n - m + 1 values): by the sliding sum when
// `tones` describes the templates (within slide_bound() of the direct value then), else by the direct sums.
static int afsk_magnitudes(pm_ctx *ctx, const double *d_x, int64_t n, double x_bound, const double *d_mark_i, const double *d_mark_q,
                           const double *d_unit_i, const double *d_unit_q, int m, const pm_afsk_tones *tones, double *M, double *S,
                           double diff_gain = 0.0)
{
    PM_ARG(S || (tones && m >= 2));                          // the one-stream difference exists for the sliding sums only
    const int64_t nc = n - m + 1;
    if (tones && m >= 2) {
        PM_ARG(tones->tap_dev >= 0.0 && tones->tap_dev < 1e-6);
        const SlideTones T = slide_tones(tones);
        const int64_t ntiles = pm_cdiv(nc, (int64_t)kSlideThreads * kSlideRun);
        PM_ARG(ntiles < (1LL << 31));
        const size_t lds = slide_lds_bytes<kSlideRun>(m);
        if (lds > 160 * 1024) return pm_set_error(PM_ERR_ARG, "sliding correlator sums: %d taps do not fit the LDS tile", m);
        PmProf prof(ctx, PM_K_AFSK_CORR);
        prof.work((double)n * 8 + (S ? 2.0 : 1.0) * nc * 8, (4.0 * m / kSlideRun + 18.0) * (double)nc);
        if (int rc = allow_lds(afsk_slide_kernel<kSlideRun>, lds)) return rc;
        hipLaunchKernelGGL((afsk_slide_kernel<kSlideRun>), dim3((unsigned)ntiles), dim3(kSlideThreads), lds, ctx->stream, d_x, n, d_mark_i, d_mark_q,
                           d_unit_i, d_unit_q, m, T, M, S, nc, diff_gain);
        PM_HIP(hipGetLastError());
        return PM_OK;
    }
    constexpr int R = 4;
    const int64_t ntiles = pm_cdiv(nc, (int64_t)kThreads * R);
    PM_ARG(ntiles < (1LL << 31));
    const size_t lds = lds_bytes<R>(m);
    PmProf prof(ctx, PM_K_AFSK_CORR);
    prof.work((double)n * 8 + 2.0 * nc * 8, 2.0 * 4 * m * (double)nc);
    auto go = [&](auto kernel) -> int {
        if (int rc = allow_lds(kernel, lds)) return rc;
        hipLaunchKernelGGL(kernel, dim3((unsigned)ntiles), dim3(kThreads), lds, ctx->stream, d_x, n, d_mark_i, d_mark_q, d_unit_i, d_unit_q, m, M, nc, S);
        return PM_OK;
    };
    if (int rc = (((uintptr_t)d_x) & 15) == 0 ? go(afsk_correlate_kernel<R, true, true>) : go(afsk_correlate_kernel<R, false, true>)) return rc;
    PM_HIP(hipGetLastError());
    return PM_OK;
}

}  // extern "C"

// ---- one certified sweep as every launcher sees it ---------------------------------------------------------------------------------------
// Made by sweep_plan() from the caller's description, which performs EVERY check that can refuse a sweep: a refused sweep has touched
// neither the stream nor a counter.
struct SweepPlan {
    pm_afsk_sweep_desc w;
    int64_t nc, nl;                  // magnitudes per stream; low-pass outputs = bits per modem
    SweepArgs P;
    double gmax;
    SlideTones T;                    // with tones
    SweepSource src;                 // audio == nullptr: the input is the reference's band-passed stream
    SweepRouting R;
    double E;
    Lpf8Args Q;                      // kFused8 on the caller's plan: its constants
};

static SweepSwitches sweep_switches(const pm_tuning &t) { return SweepSwitches{t.afsk_unfused != 0, t.afsk_lpf8 == 1, t.sweep_no_tail != 0, t.afsk_split != 0}; }

// n: length of the sweep's input; src: nullptr, or where a band-passed stream that is only near the reference's came from; lpf8: nullptr or
// the caller's matrix-pipe plan of the low-pass; own_list: the counts go to a recording's own list (pm_sweep_cells::d_list)
static int sweep_plan(const pm_tuning &tune, const pm_afsk_sweep_desc &w, int64_t n, double x_bound, const SweepSource *src, const pm_lpf8_plan *lpf8,
                      bool own_list, SweepPlan *S)
{
    PM_ARG(w.d_mark_i && w.d_mark_q && w.d_unit_i && w.d_unit_q && w.d_space && w.h_gains && w.d_lpf && w.h_bits);
    // a band-passed stream that is only near the reference's: tone templates only, and the exact recomputation goes back to the audio
    PM_ARG(!src || (src->audio && src->bpf && src->mb >= 1 && src->e_x >= 0.0 && src->e_x < 1e-6 * x_bound && w.h_tones));
    PM_ARG(!w.h_tones || (w.h_tones->tap_dev >= 0.0 && w.h_tones->tap_dev < 1e-6));
    PM_ARG(w.groups >= 1 && w.groups <= kSweepMax && w.m >= 1 && w.m <= kMaxTaps && w.ml >= 1 && w.ml <= kMaxTaps);
    PM_ARG(x_bound > 0.0 && x_bound < 1e300 && w.lpf_abs_sum > 0.0 && w.lpf_abs_sum < 1e300);
    PM_ARG(n >= (int64_t)w.m + w.ml - 1);
    S->w = w;
    S->nc = n - w.m + 1;
    S->nl = S->nc - w.ml + 1;
    PM_ARG(pm_cdiv(S->nl, kTile) < (1LL << 31));
    PM_ARG(sweep_args(w.h_gains, w.h_bits, w.groups, &S->P, &S->gmax));
    S->T = w.h_tones ? slide_tones(w.h_tones) : SlideTones{};
    S->src = src ? *src : SweepSource{nullptr, nullptr, 0, 0.0};
    S->R = sweep_route(w.m, w.ml, w.groups, w.h_tones != nullptr, S->src.mb, lpf8 ? lpf8->ml : 0, own_list, sweep_switches(tune));
    S->E = sweep_bound(w.m, w.lpf_abs_sum, S->gmax, x_bound, w.h_tones, S->R.route >= kFused64 ? kFuseRun : kSlideRun, S->src.e_x);
    if (S->R.route == kFused8 && !S->R.call_plan) S->Q = lpf8_args(lpf8, S->gmax, S->R.one);
    return PM_OK;
}

// ---- who owns a sweep's counter -------------------------------------------------------------------------------------------------------------
struct SweepCounters {
    int *count;                      // uncertain samples the sweep could not decide itself
    int *next;                       // the ring's next slot, which this sweep's LAST launch clears (nullptr: a recording's own cells)
    int *mail;                       // page-locked word the sweep's last launch leaves the count in (nullptr: none)
    unsigned long long *list;        // the recording's own list (nullptr: one in the context's scratch block)
};

// The context's ring (not in the scratch block, which the next call on this context re-carves and may re-allocate: pm_afsk_sweep_last
// reads the counter later).  All slots start at zero; the last launch of a sweep clears the slot the next sweep will use, so there is
// no memset on the stream.  A sweep that takes its slot and then launches nothing would leave the NEXT sweep's slot uncleared, and
// that sweep would start from whatever count the slot held 64 sweeps ago -- up to 65536 stale list entries to "recompute": whatever
// can refuse a sweep is checked before this is called (sweep_plan), and RingGuard covers a launch that fails afterwards.
static int sweep_ring_take(pm_ctx *ctx, bool deferred, SweepCounters *C)
{
    if (!ctx->d_sweep) {
        PM_HIP(hipMalloc((void **)&ctx->d_sweep, kSweepRing * sizeof(int)));
        PM_HIP(hipMemset(ctx->d_sweep, 0, kSweepRing * sizeof(int)));
        PM_HIP(hipHostMalloc((void **)&ctx->h_sweep, kSweepRing * sizeof(int), hipHostMallocDefault));
        memset(ctx->h_sweep, 0, kSweepRing * sizeof(int));
    }
    const int slot = (int)(ctx->sweep_seq % kSweepRing);
    *C = SweepCounters{ctx->d_sweep + slot, ctx->d_sweep + (slot + 1) % kSweepRing, deferred ? ctx->h_sweep + slot : nullptr, nullptr};
    ctx->sweep_mail[slot] = deferred ? ctx->sweep_seq + 1 : 0;
    ctx->sweep_seq++;
    ctx->sweep_count = C->count;
    return PM_OK;
}

// a sweep that fails behind sweep_ring_take has not run its last launch: the next sweep's counter is cleared by hand
struct RingGuard {
    hipStream_t st; int *next; bool ok;
    ~RingGuard() { if (!ok && next) (void)hipMemsetAsync(next, 0, sizeof(int), st); }
};

extern "C" {

int pm_afsk_sweep_mode(pm_ctx *ctx, int deferred)
{
    PM_ARG(ctx != nullptr);
    ctx->sweep_deferred = deferred != 0;
    return PM_OK;
}

int pm_afsk_sweep_last(pm_ctx *ctx, int64_t *h_uncertain)
{
    PM_CTX(ctx);
    PM_ARG(h_uncertain != nullptr);
    *h_uncertain = -1;
    if (!ctx->sweep_count) return PM_OK;
    int v = 0;
    PM_HIP(hipMemcpyAsync(&v, ctx->sweep_count, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    PM_HIP(hipStreamSynchronize(ctx->stream));
    *h_uncertain = v;
    return PM_OK;
}

int pm_afsk_sweep_ticket(pm_ctx *ctx, int64_t *h_ticket)
{
    PM_ARG(ctx != nullptr && h_ticket != nullptr);
    *h_ticket = ctx->sweep_seq - 1;                    // -1: no sweep yet
    return PM_OK;
}

int pm_afsk_sweep_results(pm_ctx *ctx, const int64_t *tickets, int n, pm_ctx *via, int64_t *h_uncertain, int64_t *h_capacity)
{
    PM_CTX(ctx);
    PM_ARG(h_uncertain != nullptr && tickets != nullptr && n >= 1 && ctx->d_sweep != nullptr);
    for (int k = 0; k < n; ++k) {
        PM_ARG(tickets[k] >= 0 && tickets[k] < ctx->sweep_seq);
        if (ctx->sweep_seq - tickets[k] >= kSweepRing)
            return pm_set_error(PM_ERR_ARG, "pm_afsk_sweep_results: ticket %lld is %lld sweeps old, the ring holds %d", (long long)tickets[k],
                                (long long)(ctx->sweep_seq - tickets[k]), kSweepRing);
    }
    // deferred sweeps have left their counters in the page-locked mailbox (sweep_exact_kernel): the caller knows they have finished
    bool mailed = ctx->h_sweep != nullptr;
    for (int k = 0; k < n && mailed; ++k) mailed = ctx->sweep_mail[tickets[k] % kSweepRing] == tickets[k] + 1;
    if (mailed) {
        for (int k = 0; k < n; ++k) h_uncertain[k] = ((volatile int *)ctx->h_sweep)[tickets[k] % kSweepRing];
        if (h_capacity) *h_capacity = kSweepCap;
        return PM_OK;
    }
    // the caller knows the sweeps have finished; the whole ring (256 bytes) comes over in ONE copy on `via`'s stream (the caller's own:
    // a slicer worker must not queue behind the demod stream's next recordings, nor take the device-wide wait of a synchronous copy)
    pm_ctx *c = via ? via : ctx;
    int *h = (int *)c->h_pinned + 16;                      // past the words other entry points use as flags
    PM_HIP(hipMemcpyAsync(h, ctx->d_sweep, kSweepRing * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    PM_HIP(hipStreamSynchronize(c->stream));
    for (int k = 0; k < n; ++k) h_uncertain[k] = h[tickets[k] % kSweepRing];
    if (h_capacity) *h_capacity = kSweepCap;
    return PM_OK;
}

int pm_afsk_sweep_result(pm_ctx *ctx, int64_t ticket, pm_ctx *via, int64_t *h_uncertain, int64_t *h_capacity)
{
    return pm_afsk_sweep_results(ctx, &ticket, 1, via, h_uncertain, h_capacity);
}

}  // extern "C"

// ---- the launchers ----------------------------------------------------------------------------------------------------------------------------
// one wave per uncertain decision at a time: as many workgroups as a sweep usually has entries (several hundred; an idle one costs a
// dispatch slot for a microsecond), so that the launch lasts one entry's latency and not three
constexpr int kExactGrid = 4096;

// The exact chain over min(*count, kSweepCap) entries of a sweep's list: from the audio where the sweep's input was a value with a bound
// (src.audio), else from d_x.  reset / mail: nullptr, or the words the launch clears / leaves the count in.
static int sweep_exact_launch(pm_ctx *ctx, const double *d_x, const pm_afsk_sweep_desc &w, const SweepArgs &P, const SweepSource &src,
                              const unsigned long long *list, const int *count, int *reset, int *mail)
{
    PmProf prof(ctx, PM_K_SIGNS);
    if (src.audio)
        hipLaunchKernelGGL(sweep_exact_kernel<true>, dim3(kExactGrid), dim3(64), sweep_tail_doubles(w.m, w.ml, src.mb) * sizeof(double), ctx->stream, d_x, w.d_mark_i,
                           w.d_mark_q, w.d_space, w.m, w.d_lpf, w.ml, P, list, count, kSweepCap, reset, mail, src);
    else
        hipLaunchKernelGGL(sweep_exact_kernel<false>, dim3(kExactGrid), dim3(64), (size_t)w.ml * sizeof(double), ctx->stream, d_x, w.d_mark_i, w.d_mark_q, w.d_space,
                           w.m, w.d_lpf, w.ml, P, list, count, kSweepCap, reset, mail, src);
    PM_HIP(hipGetLastError());
    return PM_OK;
}

// One certified sweep over d_x (n values).  deferred: the overflow fallback is the caller's (pm_afsk_sweep_mode), the three gated
// launches at the end are not enqueued.  cells: nullptr (the context's ring) or the recording's own counters, sweep k of them.
static int sweep_signs(pm_ctx *ctx, const double *d_x, int64_t n, double x_bound, const pm_afsk_sweep_desc &w, const SweepSource *src,
                       const pm_lpf8_plan *lpf8, bool deferred, const pm_sweep_cells *cells = nullptr, int k = 0)
{
    PM_CTX(ctx);
    // the gated exact launches read d_x and clear the ring's next slot: neither fits a stream with a source or a recording's own cells
    PM_ARG(d_x && (deferred || (!src && !cells)));
    SweepPlan S;
    if (int rc = sweep_plan(ctx->tune, w, n, x_bound, src, lpf8, cells && cells->d_list, &S)) return rc;
    const SweepRouting &R = S.R;
    const int groups = w.groups, m = w.m, ml = w.ml;
    const int64_t nc = S.nc, nl = S.nl;
    const int cap = kSweepCap;                             // more uncertain samples than this: the gated exact path below takes over
    const int F = 2 + 2 * groups;
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const int64_t stride = (nc + 63) / 64 * 64;
    const size_t b_m = up((size_t)nc * 8), b_a = up((size_t)nl * 8), b_list = up((size_t)cap * 8), b_w = up((size_t)F * m * 8),
                 b_c = up((size_t)stride * groups * 8);
    if (int rc = pm_scratch_reserve(ctx, 2 * b_m + b_a + b_list + 256 + b_w + b_c)) return rc;
    char *base = (char *)ctx->d_scratch;
    double *M = (double *)base, *Sp = (double *)(base + b_m), *A = (double *)(base + 2 * b_m);
    double *d_w = (double *)(base + 2 * b_m + b_a + b_list + 256);
    double *C = (double *)(base + 2 * b_m + b_a + b_list + 256 + b_w);
    // a recording's own cells (zeroed by an earlier launch on this stream, read by their owner when the stream has passed the sweep:
    // the context's ring stays where it is), or the ring
    SweepCounters cn{nullptr, nullptr, nullptr, nullptr};
    if (cells) cn = SweepCounters{cells->d_count + k, nullptr, cells->h_mail + k, cells->d_list ? cells->d_list + (size_t)k * kSweepCap : nullptr};
    else if (int rc = sweep_ring_take(ctx, deferred, &cn)) return rc;
    if (!cn.list) cn.list = (unsigned long long *)(base + 2 * b_m + b_a);
    RingGuard ring{ctx->stream, cn.next, false};
    // Low-passes on the int8 matrix pipe from a plan of this call's own, for tests and measurements (PM_AFSK_LPF8=1)
    pm_lpf8_plan *own8 = nullptr;
    if (R.call_plan) {
        std::vector<double> hl((size_t)ml);
        PM_HIP(hipMemcpyAsync(hl.data(), w.d_lpf, hl.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        PM_HIP(hipStreamSynchronize(ctx->stream));
        if (int rc = pm_lpf8_plan_create(ctx, hl.data(), ml, &own8)) return rc;
    }
    struct Own8 { pm_ctx *c; pm_lpf8_plan *p; ~Own8() { if (p) { (void)hipStreamSynchronize(c->stream); pm_lpf8_plan_destroy(p); } } } own8_guard{ctx, own8};
    if (R.route == kFused64 || R.route == kFused8) {
        // sliding sums, low-pass(es) and combine in one kernel: nothing but the bitmaps is written
        const int64_t ntiles = pm_cdiv(nl, kTile);
        PmProf prof(ctx, PM_K_FIR_F64);
        prof.work((double)n * 8 + (double)groups * nl / 8,
                  (4.0 * m / kFuseRun + 18.0) * (double)nc + (R.one ? 1.0 : 2.0) * 2.0 * ml * (double)nl + 2.0 * groups * (double)nl);
        int rc;
        if (R.route == kFused8) {
            const Lpf8Args Q = own8 ? lpf8_args(own8, S.gmax, R.one) : S.Q;
            const SweepShape shape{m, ml, R.one};
            const Lpf8Layout Y = lpf8_layout(&shape, 1, S.src.mb, 0);
            const SweepTail TL{w.d_space, w.d_lpf, R.lds_ok, S.src};
            auto go8 = [&](auto kernel) -> int {
                if (int rc = allow_lds(kernel, Y.lds)) return rc;
                hipLaunchKernelGGL(kernel, dim3((unsigned)ntiles), dim3(kThreads), Y.lds, ctx->stream, d_x, n, w.d_mark_i, w.d_mark_q, w.d_unit_i, w.d_unit_q, m, S.T,
                                   Q, ml, nl, groups, S.P, S.E, cn.list, cn.count, cap, Y.region0, TL);
                return PM_OK;
            };
            rc = R.one ? go8(afsk_slide_lpf8_kernel<true>) : go8(afsk_slide_lpf8_kernel<false>);
        } else {
            const size_t lds = fuse_lds_bytes(m, ml);
            const int region0 = (int)fuse_region0(m, ml), image = (int)fuse_image(ml);
            auto go = [&](auto kernel) -> int {
                if (int rc = allow_lds(kernel, lds)) return rc;
                hipLaunchKernelGGL(kernel, dim3((unsigned)ntiles), dim3(kThreads), lds, ctx->stream, d_x, n, w.d_mark_i, w.d_mark_q, w.d_unit_i, w.d_unit_q, m, S.T,
                                   w.d_lpf, ml, nl, groups, S.P, S.E, cn.list, cn.count, cap, region0, image);
                return PM_OK;
            };
            rc = R.one ? go(afsk_slide_lpf_kernel<true, kFuseRun>) : go(afsk_slide_lpf_kernel<false, kFuseRun>);
        }
        if (rc) return rc;
        PM_HIP(hipGetLastError());
        if (R.ends) { ring.ok = true; return PM_OK; }      // nothing follows on this stream: the caller mails the count
    } else {
        // One chain with tone templates: its mark - gain * space difference leaves the sliding kernel as ONE stream and takes ONE
        // low-pass (the reference's own dataflow, afsk.py:162-166, on approximate magnitudes); a sweep takes two for all its chains.
        if (int rc = afsk_magnitudes(ctx, d_x, n, x_bound, w.d_mark_i, w.d_mark_q, w.d_unit_i, w.d_unit_q, m, w.h_tones, M, R.one ? nullptr : Sp, S.P.gain[0])) return rc;
        if (!R.one)
            if (int rc = pm_fir_valid_f64(ctx, M, nc, w.d_lpf, ml, A, 0)) return rc;
        // B = LPF(S) and the combine step in one pass: B never reaches memory
        const double *lp_in = R.one ? M : Sp, *lp_a = R.one ? nullptr : A;
        constexpr int R8 = 8;
        const int64_t ntiles = pm_cdiv(nl, (int64_t)kThreads * R8);
        const size_t lds = lds_bytes<R8>(ml);
        PmProf prof(ctx, PM_K_FIR_F64);
        prof.work((double)nc * 8 + (R.one ? 0.0 : (double)nl * 8) + (double)groups * nl / 8, 2.0 * ml * (double)nl + 2.0 * groups * (double)nl);
        auto go = [&](auto kernel) -> int {
            if (int rc = allow_lds(kernel, lds)) return rc;
            hipLaunchKernelGGL(kernel, dim3((unsigned)ntiles), dim3(kThreads), lds, ctx->stream, lp_in, nc, w.d_lpf, ml, lp_a, nl, groups, S.P, S.E, cn.list, cn.count, cap);
            return PM_OK;
        };
        if (int rc = (((uintptr_t)lp_in) & 15) == 0 ? go(fir_sweep_kernel<R8, true>) : go(fir_sweep_kernel<R8, false>)) return rc;
        PM_HIP(hipGetLastError());
    }
    // deferred: this is the sweep's last launch, which clears the next sweep's counter and mails its own
    if (int rc = sweep_exact_launch(ctx, d_x, w, S.P, S.src, cn.list, cn.count, deferred ? cn.next : nullptr, cn.mail)) return rc;
    // Deferred fallback: the caller looks at the counter once the sweep has finished (pm_afsk_sweep_result) and runs the exact
    // chains itself in the (degenerate) overflow case; the three gated launches below -- which in the normal case only look at
    // the counter and leave, but cost the demod stream three dispatches per sweep -- are not enqueued.
    if (deferred) { ring.ok = true; return PM_OK; }
    // More uncertain samples than the list holds (degenerate input: silence, amplitudes far below the caller's bound): the exact
    // chain of every modem runs after all -- the same launches as pm_afsk_correlate_group + pm_fir_signs_f64_batch, each workgroup
    // of which first looks at the counter and leaves at once in the normal case.  No host round trip either way.
    hipLaunchKernelGGL(pack_group_taps_kernel, dim3((unsigned)pm_cdiv((int64_t)F * m, 256)), dim3(256), 0, ctx->stream, w.d_mark_i, w.d_mark_q,
                       w.d_space, m, F, d_w);
    if (int rc = afsk_group_dispatch(ctx, groups, d_x, n, d_w, m, C, stride, nc, cn.count, cap)) return rc;
    const double *cx[kSweepMax];
    int64_t cnn[kSweepMax];
    for (int g = 0; g < groups; ++g) { cx[g] = C + (size_t)g * stride; cnn[g] = nc; }
    if (int rc = pm_fir_signs_batch(ctx, groups, cx, cnn, w.d_lpf, ml, w.h_bits, 0, cn.count, cap, cn.next)) return rc;
    ring.ok = true;
    return PM_OK;
}

extern "C" {

int pm_afsk_sweep_signs(pm_ctx *ctx, const double *d_x, int64_t n, double x_bound, const double *d_mark_i, const double *d_mark_q,
                        const double *d_unit_i, const double *d_unit_q, const double *d_space, const double *h_gains, int groups, int m,
                        const double *d_lpf, int ml, double lpf_abs_sum, uint64_t *const *h_bits)
{
    PM_ARG(ctx != nullptr);
    const pm_afsk_sweep_desc w{d_mark_i, d_mark_q, d_unit_i, d_unit_q, d_space, h_gains, groups, m, d_lpf, ml, 0, lpf_abs_sum, h_bits, nullptr};
    return sweep_signs(ctx, d_x, n, x_bound, w, nullptr, nullptr, ctx->sweep_deferred);
}

int pm_afsk_sweep_signs_tones(pm_ctx *ctx, const double *d_x, int64_t n, double x_bound, const double *d_mark_i, const double *d_mark_q,
                              const double *d_unit_i, const double *d_unit_q, const double *d_space, const double *h_gains, int groups, int m,
                              const double *d_lpf, int ml, double lpf_abs_sum, uint64_t *const *h_bits, const pm_afsk_tones *h_tones)
{
    if (!h_tones) return pm_set_error(PM_ERR_ARG, "pm_afsk_sweep_signs_tones: no tones");
    PM_ARG(ctx != nullptr);
    const pm_afsk_sweep_desc w{d_mark_i, d_mark_q, d_unit_i, d_unit_q, d_space, h_gains, groups, m, d_lpf, ml, 0, lpf_abs_sum, h_bits, h_tones};
    return sweep_signs(ctx, d_x, n, x_bound, w, nullptr, nullptr, ctx->sweep_deferred);
}

int pm_afsk_magnitudes(pm_ctx *ctx, const double *d_x, int64_t n, double x_bound, const double *d_mark_i, const double *d_mark_q,
                       const double *d_space_i, const double *d_space_q, int m, const pm_afsk_tones *h_tones, double *d_mark_mag,
                       double *d_space_mag, double *h_bound)
{
    PM_CTX(ctx);
    PM_ARG(d_x && d_mark_i && d_mark_q && d_space_i && d_space_q && d_mark_mag && d_space_mag);
    PM_ARG(m >= 1 && m <= kMaxTaps && n >= m && x_bound > 0.0 && x_bound < 1e300);
    if (int rc = afsk_magnitudes(ctx, d_x, n, x_bound, d_mark_i, d_mark_q, d_space_i, d_space_q, m, h_tones, d_mark_mag, d_space_mag)) return rc;
    if (h_bound) *h_bound = h_tones && m >= 2 ? slide_bound(h_tones, m, x_bound) : 0.0;
    return PM_OK;
}

int pm_afsk_group_run(pm_ctx *ctx, const int16_t *d_audio, int64_t n, const double *d_bpf, int mb, double *d_bpf_out, double x_bound,
                      const pm_afsk_sweep_desc *h_sweeps, int nsweeps, int64_t *h_tickets)
{
    return pm_afsk_group_run_plan(ctx, d_audio, n, d_bpf, mb, d_bpf_out, x_bound, h_sweeps, nsweeps, h_tickets, nullptr, nullptr);
}

}  // extern "C"

// The four templates of a sweep as ONE reversed, interleaved table (pack_group_taps_kernel's layout with F = 4), made the first time the
// low-pass plan meets these templates and kept with it: afsk_fused8_kernel reads it through the scalar cache
static int lpf8_plan_templates(pm_ctx *ctx, pm_lpf8_plan *q, const pm_afsk_sweep_desc &w)
{
    if (q->d_tpl && q->tpl_m == w.m && q->tpl_src[0] == w.d_mark_i && q->tpl_src[1] == w.d_mark_q && q->tpl_src[2] == w.d_unit_i && q->tpl_src[3] == w.d_unit_q)
        return PM_OK;
    if (q->d_tpl) { PM_HIP(hipStreamSynchronize(ctx->stream)); (void)hipFree(q->d_tpl); q->d_tpl = nullptr; }
    PM_HIP(hipMalloc(&q->d_tpl, sizeof(double) * 4 * (size_t)w.m + 256));
    hipLaunchKernelGGL(pack_templates_kernel, dim3((unsigned)pm_cdiv(4 * (int64_t)w.m, 256)), dim3(256), 0, ctx->stream, w.d_mark_i, w.d_mark_q, w.d_unit_i,
                       w.d_unit_q, w.m, (double *)q->d_tpl);
    PM_HIP(hipGetLastError());
    PM_HIP(hipStreamSynchronize(ctx->stream));     // once per plan: another context's launch may be the table's next reader
    q->tpl_m = w.m;
    q->tpl_src[0] = w.d_mark_i; q->tpl_src[1] = w.d_mark_q; q->tpl_src[2] = w.d_unit_i; q->tpl_src[3] = w.d_unit_q;
    return PM_OK;
}

// The fused launch of pm_afsk_group_run_plan (afsk_fused8_kernel), each sweep from its SweepPlan.  -> PM_OK and *fused = true when the
// launch was made; *fused = false (and nothing enqueued) when the group does not qualify (group_fuses; a sweep that cannot be planned
// does not) and the caller takes the split path, which plans each sweep again -- once more per recording, on that path only -- and
// reports what is wrong with one that cannot be planned (sweep_plan has left the same message here already).
static int afsk_group_run_fused(pm_ctx *ctx, const int16_t *d_audio, int64_t n, const double *d_bpf, int mb, double x_bound, const pm_afsk_sweep_desc *h_sweeps,
                                int nsweeps, const pm_bpf8_plan *plan, const pm_lpf8_plan *const *lpf8, const pm_sweep_cells *cells, bool *fused)
{
    *fused = false;
    int kb = 0;
    const void *btab = nullptr;
    double sc6[6];
    // planned: a band-pass plan, the recording's own list, and one or two sweeps that each take the matrix pipe on a plan of the caller's
    bool planned = plan && lpf8 && cells && cells->d_list && nsweeps <= 2 && pm_bpf8_plan_view(plan, &kb, &btab, sc6) == PM_OK;
    const int64_t nb = n - mb + 1;
    const SweepSource src{d_audio, d_bpf, mb, planned ? pm_bpf8_error(plan) : 0.0};      // the band-passed stream is a value within e_x of the reference's
    SweepPlan pl[2];
    SweepShape shape[2];
    for (int k = 0; planned && k < nsweeps; ++k) {
        shape[k] = SweepShape{h_sweeps[k].m, h_sweeps[k].ml, h_sweeps[k].groups == 1};
        planned = lpf8[k] && sweep_plan(ctx->tune, h_sweeps[k], nb, x_bound, &src, lpf8[k], true, &pl[k]) == PM_OK && pl[k].R.route == kFused8;
    }
    const Lpf8Layout Y = planned ? lpf8_layout(shape, nsweeps, mb, kb) : Lpf8Layout{};
    const SweepSwitches sw = sweep_switches(ctx->tune);
    if (!group_fuses(Y, kb, planned, ((uintptr_t)d_audio & 15) == 0, sw)) return PM_OK;
    FusedArgs A;
    memset(&A, 0, sizeof(A));
    for (int k = 0; k < nsweeps; ++k) {
        const pm_afsk_sweep_desc &w = pl[k].w;
        if (int rc = lpf8_plan_templates(ctx, const_cast<pm_lpf8_plan *>(lpf8[k]), w)) return rc;
        FusedSweep &S = A.s[k];
        S.mi = w.d_mark_i; S.mq = w.d_mark_q; S.ui = w.d_unit_i; S.uq = w.d_unit_q;
        S.space = w.d_space; S.lpf = w.d_lpf;
        S.tg = ctx->tune.sweep_lds_templates ? nullptr : (const double *)lpf8[k]->d_tpl;
        S.m = w.m; S.ml = w.ml; S.G = w.groups;
        S.one = pl[k].R.one;
        S.P = pl[k].P;
        S.T = pl[k].T;
        S.E = pl[k].E;
        S.Q = pl[k].Q;
        S.list = cells->d_list + (size_t)k * kSweepCap;
        S.count = cells->d_count + k;
        S.nout = pl[k].nl;
    }
    A.audio = d_audio;
    A.n = n;
    A.nb = nb;
    A.bp_btab = (const pm_bpf8_dev::i4 *)btab;
    for (int i = 0; i < 5; ++i) A.sc.s[i] = sc6[i];
    A.sc.c0 = sc6[5];
    A.src = src;
    A.xs_span = Y.xs_span; A.aplane = Y.aplane; A.mmax = Y.mmax;
    A.xw_doubles = Y.xw_doubles; A.plane_bytes = Y.plane_bytes;
    A.cap = kSweepCap;
    A.lds_ok = Y.lds_ok && !sw.sweep_no_tail;
    const size_t lds_launch = Y.lds + (size_t)std::max(0, ctx->tune.fused_lds_pad);      // (PM_FUSED_LDS_PAD: fewer workgroups per CU, to measure what occupancy is worth)
    int64_t tiles = 0;
    double bits_out = 0.0, flops = 2.0 * mb * (double)nb;
    for (int k = 0; k < nsweeps; ++k) {
        tiles = std::max(tiles, pm_cdiv(A.s[k].nout, (int64_t)kThreads * 8));
        bits_out += (double)A.s[k].G * (double)A.s[k].nout / 8;
        flops += (4.0 * A.s[k].m / kFuseRun + 18.0) * (double)(nb - A.s[k].m + 1) + (A.s[k].one ? 1.0 : 2.0) * 2.0 * A.s[k].ml * (double)A.s[k].nout +
                 2.0 * A.s[k].G * (double)A.s[k].nout;
    }
    PM_ARG(tiles >= 1 && tiles < (1LL << 31));
    {
        PmProf prof(ctx, PM_K_FIR_F64);
        prof.work((double)n * 2 + bits_out, flops);          // the recording in, the bitmaps out: nothing else crosses HBM
        auto go = [&](auto kernel) -> int {
            if (int rc = allow_lds(kernel, lds_launch)) return rc;
            hipLaunchKernelGGL(kernel, dim3((unsigned)tiles), dim3(kThreads), lds_launch, ctx->stream, A);
            return PM_OK;
        };
        int rc = PM_OK;
        const bool o0 = A.s[0].one != 0, o1 = nsweeps == 2 && A.s[1].one != 0;
#define PM_FUSED_GO(KB)                                                                                                             \
        rc = nsweeps == 1 ? (o0 ? go(afsk_fused8_kernel<KB, true, 1, false>) : go(afsk_fused8_kernel<KB, false, 1, false>))              \
                          : (o0 ? (o1 ? go(afsk_fused8_kernel<KB, true, 2, true>) : go(afsk_fused8_kernel<KB, true, 2, false>))          \
                                : (o1 ? go(afsk_fused8_kernel<KB, false, 2, true>) : go(afsk_fused8_kernel<KB, false, 2, false>)));
        if (kb == 3) { PM_FUSED_GO(3) } else { PM_FUSED_GO(4) }
#undef PM_FUSED_GO
        if (rc) return rc;
        PM_HIP(hipGetLastError());
    }
    if (int rc = sweep_mail_reset(ctx, cells, nsweeps)) return rc;
    *fused = true;
    return PM_OK;
}

int pm_afsk_group_run_plan(pm_ctx *ctx, const int16_t *d_audio, int64_t n, const double *d_bpf, int mb, double *d_bpf_out, double x_bound,
                           const pm_afsk_sweep_desc *h_sweeps, int nsweeps, int64_t *h_tickets, const pm_bpf8_plan *plan,
                           const pm_lpf8_plan *const *lpf8, const pm_sweep_cells *cells)
{
    // The demod stage of a whole AFSK chain group in ONE call: the shared band-pass (afsk.py:151) and every certified sweep on its
    // output (afsk.py:153-166, sign bitmaps only), overflow fallback deferred to the caller (pm_afsk_sweep_results).  The same
    // launches pm_fir_valid_i16 + pm_afsk_sweep_signs[_tones] would make -- a pipelined Python host saves nine boundary crossings
    // per recording, each of which waits for the interpreter lock on the way back.
    PM_CTX(ctx);
    PM_ARG(d_audio && d_bpf && d_bpf_out && h_sweeps && nsweeps >= 1 && nsweeps <= 64 && mb >= 1 && n >= mb);
    const SweepSource src{d_audio, d_bpf, mb, plan ? pm_bpf8_error(plan) : 0.0};
    PM_ARG(!cells || (cells->d_count && cells->h_mail));
    if (plan) {
        PM_ARG(pm_bpf8_taps(plan) == mb);
        for (int k = 0; k < nsweeps; ++k) PM_ARG(h_sweeps[k].h_tones != nullptr);
    }
    // one launch for the whole stage where the group qualifies (all sweeps on the matrix pipe, at most two): afsk_fused8_kernel
    bool fused = false;
    if (int rc = afsk_group_run_fused(ctx, d_audio, n, d_bpf, mb, x_bound, h_sweeps, nsweeps, plan, lpf8, cells, &fused)) return rc;
    if (fused) return PM_OK;
    if (plan) {
        if (int rc = pm_bpf8_run(ctx, plan, d_audio, n, d_bpf_out, cells ? cells->d_count : nullptr, cells ? nsweeps : 0)) return rc;
    } else {
        if (cells) PM_HIP(hipMemsetAsync(cells->d_count, 0, sizeof(int) * (size_t)nsweeps, ctx->stream));
        if (int rc = pm_fir_valid_i16(ctx, d_audio, n, d_bpf, mb, d_bpf_out, 0)) return rc;
    }
    for (int k = 0; k < nsweeps; ++k) {
        if (int rc = sweep_signs(ctx, d_bpf_out, n - mb + 1, x_bound, h_sweeps[k], plan ? &src : nullptr, lpf8 ? lpf8[k] : nullptr, true, cells, k)) return rc;
        if (h_tickets && !cells) h_tickets[k] = ctx->sweep_seq - 1;
    }
    // One wave behind the recording's last sweep leaves every sweep's count in its page-locked word (a sweep that ended with a launch
    // of its own has written the same value there already): no launch between the sweeps for this or for the recomputation
    if (cells && cells->d_list) return sweep_mail_reset(ctx, cells, nsweeps);
    return PM_OK;
}

int pm_afsk_sweep_exact_list(pm_ctx *ctx, const int16_t *d_audio, const double *d_bpf, int mb, const pm_afsk_sweep_desc *w, uint64_t *const *h_bits,
                             const unsigned long long *d_list, const int *d_count)
{
    PM_CTX(ctx);
    // (not through sweep_plan: whoever works a list off has neither the stream's length nor its bound, and brings the bitmaps apart)
    PM_ARG(d_audio && d_bpf && mb >= 1 && w && h_bits && d_list && d_count && w->groups >= 1 && w->groups <= kSweepMax);
    SweepArgs P;
    double gmax = 0.0;
    PM_ARG(w->h_gains && sweep_args(w->h_gains, h_bits, w->groups, &P, &gmax));
    return sweep_exact_launch(ctx, nullptr, *w, P, SweepSource{d_audio, d_bpf, mb, 0.0}, d_list, d_count, nullptr, nullptr);
}

// int8 digit products per tap and output of the matrix-pipe kernels, from the kernels' own constants (bench.py prices the launches with them)
extern "C" int pm_matrix_digit_pairs(int stage)
{
    switch (stage) {
    case 0: return pm_bpf8_digit_pairs();                    // bpf8_kernel: the certified sweeps' band-pass
    case 1: return kL8Dig * kL8Dig - 1;                      // afsk_slide_lpf8_kernel, per low-pass stream: all pairs but x0 q0
    case 2: return pm_fir8_digit_pairs();                    // fir8_kernel: the batch engine's matched filters
    default: return pm_set_error(PM_ERR_ARG, "pm_matrix_digit_pairs: no stage %d", stage);
    }
}

extern "C" int pm_ubench_sqrt_f32(pm_ctx *ctx, int exponent, int64_t *h_worst_ulp_1024)
{
    PM_CTX(ctx);
    PM_ARG(h_worst_ulp_1024 != nullptr && exponent >= -125 && exponent <= 125);
    void *q = nullptr;
    if (int rc = pm_malloc(ctx, 8, &q)) return rc;
    int rc = PM_OK;
    unsigned long long worst = 0;
    if (hipMemsetAsync(q, 0, 8, ctx->stream) != hipSuccess) rc = pm_set_error(PM_ERR_HIP, "pm_ubench_sqrt_f32: memset failed");
    if (!rc) {
        hipLaunchKernelGGL(sqrt_f32_ulp_kernel, dim3(1u << 16), dim3(256), 0, ctx->stream, exponent, (unsigned long long *)q);
        if (hipMemcpyAsync(&worst, q, 8, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess)
            rc = pm_set_error(PM_ERR_HIP, "pm_ubench_sqrt_f32: the launch failed");
    }
    (void)pm_free(ctx, q);
    *h_worst_ulp_1024 = (int64_t)worst;
    return rc;
}
