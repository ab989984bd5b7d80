// FIR stages of the demod_chain path as LDS-staged sliding-window kernels for gfx950.
//
//   pm_fir_valid_{i16,f64}  numpy.convolve(x, h, 'valid')          (19 call sites in the reference)
//   pm_signs_f64            (x >= 0) bitmap, the slicers' only input (slicer.py:85,99-102)
//
// Arithmetic: binary64, one fma per tap, taps visited in ascending input index.  That order is the
// build's canonical order; oracle/pm_oracle.c:pmo_fir_* uses the same one, so GPU and oracle agree
// bit for bit.  Built with -ffp-contract=off: only the fma() written below fuses.
//
// Tiling: a 256-thread workgroup produces T = 256*R consecutive outputs.  The T+m-1 inputs it needs
// are staged once in LDS as f64 (int16 converted on the way in); each thread then owns R consecutive
// outputs and slides a register window over the taps, so one LDS read feeds R fmas.  The LDS image
// carries one spare double after every 8 so that lane t's window starts 9 doubles after lane t-1's
// (18 dwords: conflict-free for ds_read_b64).  Results go back through the same LDS image so that
// the global stores are coalesced (lane-contiguous 8 B).
#include "pm_fir_dev.h"
#include <algorithm>
#include <cstring>

namespace {

// SIGNS: instead of the float64 outputs, write only their (y >= 0) bitmap -- all a slicer reads of them.
template <typename InT, int R, bool NEG, bool VEC, bool SIGNS>
__device__ __forceinline__ void fir_tile(const InT *__restrict__ x, int64_t n, const double *__restrict__ h, int m,
                                         double *__restrict__ y, int64_t nout, uint64_t *__restrict__ bits, int64_t tile)
{
    extern __shared__ double xs[];
    constexpr int T = kThreads * R;
    const int t = threadIdx.x;
    const int64_t tile0 = tile * T;
    double acc[R];
    fir_tile_acc<InT, R, VEC>(x, n, h, m, tile, acc);
    if (SIGNS) {
        // This thread's 8 consecutive outputs are exactly one byte of the little-endian bitmap (tile0 is a multiple of 2048): no
        // trip through LDS, the 64 lanes of a wave store 64 consecutive bytes.  Bits past nout are written as 0 up to the end of
        // the last 64-bit word.
        static_assert(R == 8, "one bitmap byte per thread");
        const int64_t go = tile0 + (int64_t)t * R;
        unsigned byte = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const double v = NEG ? -acc[r] : acc[r];
            byte |= (unsigned)(v >= 0.0 && go + r < nout) << r;
        }
        const int64_t bi = go >> 3;
        if (bi < ((nout + 63) >> 6) * 8) reinterpret_cast<uint8_t *>(bits)[bi] = (uint8_t)byte;
        return;
    }
    lds_barrier();
    {
        double *op = xs + t * (R + 1);     // this thread's R outputs occupy R consecutive slots
#pragma unroll
        for (int r = 0; r < R; ++r) op[r] = NEG ? -acc[r] : acc[r];
    }
    lds_barrier();
    if (VEC) {
#pragma unroll
        for (int r = 0; r < R / 2; ++r) {
            const int idx = 2 * (r * kThreads + t);            // even: idx and idx+1 sit in adjacent slots
            const int64_t go = tile0 + idx;
            const int s0i = slot<R>(idx);
            const double2v v = {xs[s0i], xs[s0i + 1]};
            if (go + 1 < nout) *reinterpret_cast<double2v *>(y + go) = v;
            else if (go < nout) y[go] = v.x;
        }
    } else {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int idx = r * kThreads + t;
            const int64_t go = tile0 + idx;
            if (go < nout) y[go] = xs[slot<R>(idx)];
        }
    }
}

template <typename InT, int R, bool NEG, bool VEC, bool SIGNS>
__global__ __launch_bounds__(kThreads) void fir_valid_kernel(const InT *__restrict__ x, int64_t n,
                                                             const double *__restrict__ h, int m,
                                                             double *__restrict__ y, int64_t nout, uint64_t *__restrict__ bits)
{
    fir_tile<InT, R, NEG, VEC, SIGNS>(x, n, h, m, y, nout, bits, (int64_t)blockIdx.x);
}

// Short FIR (M <= 8 taps) on int16 audio with only the sign bitmap kept (fsk.py:149-159 feeding slicer.slice: the fsk_9600 chain):
// the whole window of a lane's 8 outputs is 8 + M - 1 <= 15 samples, i.e. TWO 16-byte loads (its own eight samples and the eight
// after them, which are the next lane's own: the second load is served by the cache), converted once in registers.  No LDS image, no
// barrier: per 8 outputs 2 loads, 15 conversions, 8 M fma and one byte stored -- the kernel is bound by HBM (2 B in and 1/8 B out
// per sample) as long as the conversions keep up.  Sums as everywhere: one fma per tap, ascending input index, from +0.
typedef unsigned int uint4v __attribute__((ext_vector_type(4)));

// int16 -> binary64 without v_cvt_f64_i32 (a quarter-rate instruction: fifteen of them cost as much as the 64 fma of the sums):
// u = v + 32768 is the sample with its sign bit flipped, {0x43300000, u} is the double 2^52 + u, and (2^52 + u) - (2^52 + 32768)
// is exact -- the sample itself, +0 for 0.
__device__ __forceinline__ double i16_biased_to_f64(uint32_t u) { return __hiloint2double(0x43300000, (int)u) - 4503599627403264.0; }

constexpr int kShortIter = 8;      // bitmap bytes per lane: a wave that lives for one byte costs more to launch than to run

template <int M, bool NEG>
__global__ __launch_bounds__(kThreads) void fir_short_signs_i16_kernel(const int16_t *__restrict__ x, int64_t n, const double *__restrict__ h,
                                                                       int64_t nout, uint64_t *__restrict__ bits)
{
    const int64_t nbytes = ((nout + 63) >> 6) * 8;                             // the bitmap is written in whole 64-bit words
    double g[M];
#pragma unroll
    for (int j = 0; j < M; ++j) g[j] = h[M - 1 - j];                           // uniform: scalar loads
    // the workgroup's lanes take consecutive bytes (coalesced loads and stores), kShortIter rounds of them
    const int64_t byte0 = (int64_t)blockIdx.x * (kThreads * kShortIter) + threadIdx.x;
    uint4v a, b;
    auto fetch = [&](int64_t by, uint4v &qa, uint4v &qb) {
        const int64_t go = by * 8;                                             // this byte's first output = its first input
        qa = uint4v{0, 0, 0, 0};
        qb = uint4v{0, 0, 0, 0};
        if (by >= nbytes) return;
        if (go + 15 < n) {
            qa = *reinterpret_cast<const uint4v *>(x + go);
            qb = *reinterpret_cast<const uint4v *>(x + go + 8);
        } else {                                                               // the last bytes of the stream: sample by sample
            for (int k = 0; k < 16; ++k) {
                const uint32_t v = go + k < n ? (uint32_t)(uint16_t)x[go + k] : 0u;
                if (k < 8) qa[k >> 1] |= v << ((k & 1) * 16);
                else qb[(k - 8) >> 1] |= v << ((k & 1) * 16);
            }
        }
    };
    fetch(byte0, a, b);
#pragma unroll 1
    for (int it = 0; it < kShortIter; ++it) {
        const int64_t by = byte0 + (int64_t)it * kThreads;
        uint4v na, nb;
        fetch(by + kThreads, na, nb);                                          // the next round's loads fly during this round's sums
        if (by < nbytes) {
            double w[16];
#pragma unroll
            for (int d = 0; d < 8; ++d) {
                const uint32_t q = (d < 4 ? a[d] : b[d - 4]) ^ 0x80008000u;
                w[2 * d] = i16_biased_to_f64(q & 0xFFFFu);
                w[2 * d + 1] = i16_biased_to_f64(q >> 16);
            }
            uint32_t sign = 0;                                                 // bit r = sign bit of output r
            uint32_t zero = 0;                                                 // bit r = output r is zero (NEG only)
            double acc[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) acc[r] = 0.0;
            // tap by tap across the eight outputs: eight independent chains in flight, each in ascending input order
#pragma unroll
            for (int j = 0; j < M; ++j)
#pragma unroll
                for (int r = 0; r < 8; ++r) acc[r] = __builtin_fma(g[j], w[r + j], acc[r]);
#pragma unroll
            for (int r = 7; r >= 0; --r) {
                // a sum is never -0 (it starts from +0), so acc >= 0 is "sign bit clear"; negated (fsk.py:153-154) it is "set, or zero"
                sign = __builtin_amdgcn_alignbit(sign, (uint32_t)__double2hiint(acc[r]), 31);     // (sign << 1) | sign bit
                if (NEG) zero = (zero << 1) | (acc[r] == 0.0 ? 1u : 0u);
            }
            const int64_t left = nout - by * 8;
            const uint32_t valid = left >= 8 ? 0xFFu : left <= 0 ? 0u : (1u << left) - 1u;
            const uint32_t byte = (NEG ? (sign | zero) : ~sign) & valid;
            reinterpret_cast<uint8_t *>(bits)[by] = (uint8_t)byte;
        }
        a = na;
        b = nb;
    }
}

// Several sign-only FIRs with the same taps in ONE launch (blockIdx.y = stream): the output low-passes of a chain group.  One ramp
// and one tail for the whole stage instead of one per chain.
constexpr int kFirBatchMax = 16;
struct FirBatch {
    const double *x[kFirBatchMax];
    uint64_t *bits[kFirBatchMax];
    int64_t n[kFirBatchMax];
};

template <int R, bool NEG, bool VEC>
__global__ __launch_bounds__(kThreads) void fir_signs_batch_kernel(FirBatch B, const double *__restrict__ h, int m,
                                                                   const int *__restrict__ gate = nullptr, int gate_above = 0,
                                                                   int *__restrict__ reset = nullptr)
{
    // the last launch of a certified sweep clears the counter the NEXT sweep on this context will use (pm_ctx::d_sweep is a ring)
    if (reset && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *reset = 0;
    if (gate && *gate <= gate_above) return;                          // a launch that only matters if an earlier kernel said so
    const int s = blockIdx.y;
    const int64_t n = B.n[s], nout = n - m + 1;
    // the grid is sized for the longest stream; a gated launch comes with a small grid and walks the tiles (in the normal case
    // it only has to leave, and leaving costs by the workgroup)
    for (int64_t tile = blockIdx.x; tile * (kThreads * R) < nout; tile += gridDim.x) {
        fir_tile<double, R, NEG, VEC, true>(B.x[s], n, h, m, nullptr, nout, B.bits[s], tile);
        lds_barrier();                                               // the next tile restages the LDS image
    }
}

// The same FIR over `rows` streams of equal length in ONE launch (blockIdx.y = row): the band-pass, Hilbert and matched filters of
// a batch of recordings x chains (pm_lbatch, pm_loopbatch.hip).  A row's input is x + row * x_stride, or x_ptrs[row] + x_off when
// the rows are separate allocations (the recordings of a batch); outputs are rows of one 2-D array.
struct FirRows {
    const void *x;
    int64_t x_stride;
    const void *const *x_ptrs;
    int64_t x_off;
    double *y;
    int64_t y_stride;
    uint64_t *bits;
    int64_t bits_stride;          // 64-bit words
};

template <typename InT, int R, bool NEG, bool VEC, bool SIGNS>
__global__ __launch_bounds__(kThreads) void fir_rows_kernel(FirRows A, int64_t n, const double *__restrict__ h, int m, int64_t nout)
{
    const int64_t r = blockIdx.y;
    const InT *x = A.x_ptrs ? reinterpret_cast<const InT *>(A.x_ptrs[r]) + A.x_off : reinterpret_cast<const InT *>(A.x) + r * A.x_stride;
    fir_tile<InT, R, NEG, VEC, SIGNS>(x, n, h, m, SIGNS ? nullptr : A.y + r * A.y_stride, nout, SIGNS ? A.bits + r * A.bits_stride : nullptr,
                                      (int64_t)blockIdx.x);
}

// One 64-bit word per wave per step: lane l tests sample 64*w + l, the ballot is the word.
__global__ __launch_bounds__(kThreads) void signs_kernel(const double *__restrict__ x, int64_t n,
                                                         uint64_t *__restrict__ bits, int64_t nwords)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t w = wave; w < nwords; w += nwaves) {
        const int64_t k = w * 64 + lane;
        const bool p = (k < n) && (x[k] >= 0.0);
        const uint64_t mask = __ballot(p);
        if (lane == 0) bits[w] = mask;
    }
}

template <typename InT, bool NEG>
int fir_launch2(pm_ctx *ctx, const InT *d_x, int64_t n, const double *d_taps, int m, double *d_y, uint64_t *d_bits)
{
    constexpr int R = 8;
    const int64_t nout = n - m + 1;
    const int64_t ntiles = pm_cdiv(nout, (int64_t)kThreads * R);
    PM_ARG(ntiles < (1LL << 31));
    const size_t lds = lds_bytes<R>(m);
    PmProf prof(ctx, sizeof(InT) == 2 ? PM_K_FIR_I16 : PM_K_FIR_F64);
    prof.work((double)n * sizeof(InT) + (d_bits ? (double)nout / 8 : (double)nout * 8), 2.0 * m * (double)nout);
    const bool vec = (((uintptr_t)d_x | (uintptr_t)d_y) & 15) == 0;          // 16-byte loads and stores
    if (sizeof(InT) == 2 && d_bits && !d_y && vec && m >= 2 && m <= 8 && !ctx->tune.fir_no_short) {
        // the register path for short taps (fir_short_signs_i16_kernel): one lane per bitmap byte
        const int64_t lanes = ((nout + 63) >> 6) * 8;
        const unsigned grid = (unsigned)pm_cdiv(lanes, (int64_t)kThreads * kShortIter);
        const int16_t *xs16 = reinterpret_cast<const int16_t *>(d_x);
#define PM_FIR_SHORT(MM) case MM: hipLaunchKernelGGL((fir_short_signs_i16_kernel<MM, NEG>), dim3(grid), dim3(kThreads), 0, ctx->stream, xs16, n, d_taps, nout, d_bits); break;
        switch (m) { PM_FIR_SHORT(2) PM_FIR_SHORT(3) PM_FIR_SHORT(4) PM_FIR_SHORT(5) PM_FIR_SHORT(6) PM_FIR_SHORT(7) PM_FIR_SHORT(8) }
#undef PM_FIR_SHORT
        PM_HIP(hipGetLastError());
        return PM_OK;
    }
    auto go = [&](auto kernel) -> int {
        if (int rc = allow_lds(kernel, lds)) return rc;
        hipLaunchKernelGGL(kernel, dim3((unsigned)ntiles), dim3(kThreads), lds, ctx->stream, d_x, n, d_taps, m, d_y, nout, d_bits);
        return PM_OK;
    };
    if (int rc = d_bits ? (vec ? go(fir_valid_kernel<InT, R, NEG, true, true>) : go(fir_valid_kernel<InT, R, NEG, false, true>))
                        : (vec ? go(fir_valid_kernel<InT, R, NEG, true, false>) : go(fir_valid_kernel<InT, R, NEG, false, false>))) return rc;
    PM_HIP(hipGetLastError());
    return PM_OK;
}

template <typename InT>
int fir_launch(pm_ctx *ctx, const InT *d_x, int64_t n, const double *d_taps, int m, double *d_y, uint64_t *d_bits, int flags)
{
    PM_CTX(ctx);
    PM_ARG(d_x && d_taps && (d_y || d_bits));
    PM_ARG(m >= 1 && m <= kMaxTaps);
    PM_ARG(n >= m);
    return (flags & PM_FIR_NEGATE) ? fir_launch2<InT, true>(ctx, d_x, n, d_taps, m, d_y, d_bits)
                                   : fir_launch2<InT, false>(ctx, d_x, n, d_taps, m, d_y, d_bits);
}

template <typename InT, bool NEG>
int fir_rows_launch2(pm_ctx *ctx, const FirRows &A, bool vec, int rows, int64_t n, const double *d_taps, int m)
{
    constexpr int R = 8;
    const int64_t nout = n - m + 1;
    const int64_t ntiles = pm_cdiv(nout, (int64_t)kThreads * R);
    PM_ARG(ntiles < (1LL << 31) && rows >= 1 && rows <= 65535);
    const size_t lds = lds_bytes<R>(m);
    PmProf prof(ctx, sizeof(InT) == 2 ? PM_K_FIR_I16 : PM_K_FIR_F64);
    prof.work(rows * ((double)n * sizeof(InT) + (A.bits ? (double)nout / 8 : (double)nout * 8)), 2.0 * m * (double)nout * rows);
    auto go = [&](auto kernel) -> int {
        if (int rc = allow_lds(kernel, lds)) return rc;
        hipLaunchKernelGGL(kernel, dim3((unsigned)ntiles, (unsigned)rows), dim3(kThreads), lds, ctx->stream, A, n, d_taps, m, nout);
        return PM_OK;
    };
    if (int rc = A.bits ? (vec ? go(fir_rows_kernel<InT, R, NEG, true, true>) : go(fir_rows_kernel<InT, R, NEG, false, true>))
                        : (vec ? go(fir_rows_kernel<InT, R, NEG, true, false>) : go(fir_rows_kernel<InT, R, NEG, false, false>))) return rc;
    PM_HIP(hipGetLastError());
    return PM_OK;
}

}  // namespace

// Internal (pm_common.h): what pm_fir_rows_* and the batch engine launch.  `x_aligned16`: every input row starts on a 16-byte boundary.
int pm_fir_rows(pm_ctx *ctx, bool i16, const void *d_x, int64_t x_stride, const void *const *d_x_ptrs, int64_t x_off, bool x_aligned16, int rows,
                int64_t n, const double *d_taps, int m, double *d_y, int64_t y_stride, uint64_t *d_bits, int64_t bits_stride, int flags)
{
    PM_CTX(ctx);
    PM_ARG((d_x || d_x_ptrs) && d_taps && ((d_y != nullptr) != (d_bits != nullptr)));
    PM_ARG(m >= 1 && m <= kMaxTaps && n >= m && rows >= 1);
    PM_ARG(d_x_ptrs || rows == 1 || x_stride >= n);
    const int64_t nout = n - m + 1;
    PM_ARG(rows == 1 || (d_y ? y_stride >= nout : bits_stride >= (nout + 63) / 64));
    const bool vec = x_aligned16 && (!d_y || ((((uintptr_t)d_y) & 15) == 0 && y_stride % 2 == 0));
    const bool neg = (flags & PM_FIR_NEGATE) != 0;
    // rows are the grid's y dimension: more than 65535 of them (the batch engine's R x C streams go up to 2^20) in several launches
    constexpr int kRowsPerLaunch = 65535;
    for (int r0 = 0; r0 < rows; r0 += kRowsPerLaunch) {
        const int nr = std::min(kRowsPerLaunch, rows - r0);
        FirRows A{d_x ? (const void *)((const char *)d_x + (size_t)r0 * (size_t)x_stride * (i16 ? 2 : 8)) : nullptr, x_stride, d_x_ptrs ? d_x_ptrs + r0 : nullptr, x_off,
                  d_y ? d_y + (int64_t)r0 * y_stride : nullptr, y_stride, d_bits ? d_bits + (int64_t)r0 * bits_stride : nullptr, bits_stride};
        const int rc = i16 ? (neg ? fir_rows_launch2<int16_t, true>(ctx, A, vec, nr, n, d_taps, m) : fir_rows_launch2<int16_t, false>(ctx, A, vec, nr, n, d_taps, m))
                           : (neg ? fir_rows_launch2<double, true>(ctx, A, vec, nr, n, d_taps, m) : fir_rows_launch2<double, false>(ctx, A, vec, nr, n, d_taps, m));
        if (rc) return rc;
    }
    return PM_OK;
}

// Internal (pm_common.h): pm_fir_signs_f64_batch, and with a gate the last launch of a certified sweep's overflow fallback (pm_afsk.hip).
int pm_fir_signs_batch(pm_ctx *ctx, int count, const double *const *h_x, const int64_t *h_n, const double *d_taps, int m, uint64_t *const *h_bits,
                       int flags, const int *d_gate, int gate_above, int *d_reset)
{
    PM_CTX(ctx);
    PM_ARG(count >= 1 && count <= kFirBatchMax && h_x && h_n && d_taps && h_bits);
    PM_ARG(m >= 1 && m <= kMaxTaps);
    constexpr int R = 8;
    FirBatch B;
    memset(&B, 0, sizeof(B));
    int64_t longest = 0;
    bool vec = true;
    double bytes = 0, flops = 0;
    for (int k = 0; k < count; ++k) {
        PM_ARG(h_x[k] && h_bits[k] && h_n[k] >= m);
        B.x[k] = h_x[k];
        B.bits[k] = h_bits[k];
        B.n[k] = h_n[k];
        longest = std::max(longest, h_n[k] - m + 1);
        vec = vec && (((uintptr_t)h_x[k]) & 15) == 0;
        bytes += (double)h_n[k] * 8 + (double)(h_n[k] - m + 1) / 8;
        flops += 2.0 * m * (double)(h_n[k] - m + 1);
    }
    const int64_t ntiles = pm_cdiv(longest, (int64_t)kThreads * R);
    PM_ARG(ntiles < (1LL << 31));
    const size_t lds = lds_bytes<R>(m);
    const bool neg = (flags & PM_FIR_NEGATE) != 0;
    // a gated launch (normally every workgroup leaves at once) comes with a small grid and is booked with the fallback machinery
    PmProf prof(ctx, d_gate ? PM_K_SIGNS : PM_K_FIR_F64);
    if (!d_gate) prof.work(bytes, flops);
    const dim3 grid((unsigned)(d_gate ? std::min<int64_t>(ntiles, kGatedGrid) : ntiles), (unsigned)count);
    auto go = [&](auto kernel) -> int {
        if (int rc = allow_lds(kernel, lds)) return rc;
        hipLaunchKernelGGL(kernel, grid, dim3(kThreads), lds, ctx->stream, B, d_taps, m, d_gate, gate_above, d_reset);
        return PM_OK;
    };
    if (int rc = neg ? (vec ? go(fir_signs_batch_kernel<R, true, true>) : go(fir_signs_batch_kernel<R, true, false>))
                     : (vec ? go(fir_signs_batch_kernel<R, false, true>) : go(fir_signs_batch_kernel<R, false, false>))) return rc;
    PM_HIP(hipGetLastError());
    return PM_OK;
}

extern "C" {

int pm_fir_valid_i16(pm_ctx *ctx, const int16_t *d_x, int64_t n, const double *d_taps, int m, double *d_y, int flags)
{
    return fir_launch<int16_t>(ctx, d_x, n, d_taps, m, d_y, nullptr, flags);
}

int pm_fir_signs_i16(pm_ctx *ctx, const int16_t *d_x, int64_t n, const double *d_taps, int m, uint64_t *d_bits, int flags)
{
    return fir_launch<int16_t>(ctx, d_x, n, d_taps, m, nullptr, d_bits, flags);
}

int pm_fir_signs_f64(pm_ctx *ctx, const double *d_x, int64_t n, const double *d_taps, int m, uint64_t *d_bits, int flags)
{
    return fir_launch<double>(ctx, d_x, n, d_taps, m, nullptr, d_bits, flags);
}

int pm_fir_signs_f64_batch(pm_ctx *ctx, int count, const double *const *h_x, const int64_t *h_n, const double *d_taps, int m,
                           uint64_t *const *h_bits, int flags)
{
    return pm_fir_signs_batch(ctx, count, h_x, h_n, d_taps, m, h_bits, flags, nullptr, 0, nullptr);
}

int pm_fir_valid_f64(pm_ctx *ctx, const double *d_x, int64_t n, const double *d_taps, int m, double *d_y, int flags)
{
    return fir_launch<double>(ctx, d_x, n, d_taps, m, d_y, nullptr, flags);
}

static bool rows_aligned16(const void *base, int64_t stride_elems, size_t elem, int rows)
{
    return (((uintptr_t)base) & 15) == 0 && (rows == 1 || (stride_elems * (int64_t)elem) % 16 == 0);
}

int pm_fir_rows_i16(pm_ctx *ctx, const int16_t *d_x, int64_t x_stride, int rows, int64_t n, const double *d_taps, int m, double *d_y,
                    int64_t y_stride, int flags)
{
    PM_ARG(d_x != nullptr);
    return pm_fir_rows(ctx, true, d_x, x_stride, nullptr, 0, rows_aligned16(d_x, x_stride, 2, rows), rows, n, d_taps, m, d_y, y_stride, nullptr, 0, flags);
}

int pm_fir_rows_i16_ptrs(pm_ctx *ctx, const int16_t *const *d_x_ptrs, int64_t x_off, int x_aligned16, int rows, int64_t n, const double *d_taps,
                         int m, double *d_y, int64_t y_stride, int flags)
{
    PM_ARG(d_x_ptrs != nullptr);
    return pm_fir_rows(ctx, true, nullptr, 0, (const void *const *)d_x_ptrs, x_off, x_aligned16 != 0, rows, n, d_taps, m, d_y, y_stride, nullptr, 0, flags);
}

int pm_fir_rows_f64(pm_ctx *ctx, const double *d_x, int64_t x_stride, int rows, int64_t n, const double *d_taps, int m, double *d_y,
                    int64_t y_stride, int flags)
{
    PM_ARG(d_x != nullptr);
    return pm_fir_rows(ctx, false, d_x, x_stride, nullptr, 0, rows_aligned16(d_x, x_stride, 8, rows), rows, n, d_taps, m, d_y, y_stride, nullptr, 0, flags);
}

int pm_fir_rows_signs_f64(pm_ctx *ctx, const double *d_x, int64_t x_stride, int rows, int64_t n, const double *d_taps, int m, uint64_t *d_bits,
                          int64_t bits_stride, int flags)
{
    PM_ARG(d_x != nullptr);
    return pm_fir_rows(ctx, false, d_x, x_stride, nullptr, 0, rows_aligned16(d_x, x_stride, 8, rows), rows, n, d_taps, m, nullptr, 0, d_bits, bits_stride, flags);
}

int pm_signs_f64(pm_ctx *ctx, const double *d_x, int64_t n, uint64_t *d_bits)
{
    PM_CTX(ctx);
    PM_ARG(ctx && d_bits && n >= 0);
    if (n == 0) return PM_OK;
    PM_ARG(d_x != nullptr);
    const int64_t nwords = pm_cdiv(n, 64);
    int64_t grid = pm_cdiv(nwords, kThreads / 64);
    if (grid > 8192) grid = 8192;
    PmProf prof(ctx, PM_K_SIGNS);
    prof.work((double)n * 8 + (double)n / 8, 0.0);
    hipLaunchKernelGGL(signs_kernel, dim3((unsigned)grid), dim3(kThreads), 0, ctx->stream, d_x, n, d_bits, nwords);
    PM_HIP(hipGetLastError());
    return PM_OK;
}

}  // extern "C"
