// Device helpers of the LDS-staged FIR tile that pm_fir.hip and pm_afsk.hip both build on: the padded LDS image (slot), staging,
// the canonical sums over an image (fir_acc_image) and the launchers' LDS arithmetic.  Tiling and arithmetic: see pm_fir.hip.
#pragma once
#include "pm_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kGatedGrid = 1024;       // workgroups (per stream) of a gated fallback launch: it walks the tiles if it ever has to run
constexpr int kMaxTaps = 8192;

// one spare double after every R: lane t's window (R consecutive outputs) starts R+1 doubles after lane t-1's,
// an odd number of 8-byte bank pairs, so the 32 lanes of a ds_read_b64 group hit 32 different pairs
template <int R>
__host__ __device__ __forceinline__ int slot(int p) { return p + p / R; }

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also waits for vmcnt(0), which would drain the
// next tile's prefetch and this tile's global stores at every barrier; the barriers in these kernels protect nothing
// but the LDS image.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

typedef double double2v __attribute__((ext_vector_type(2)));
typedef int int4v __attribute__((ext_vector_type(4)));
typedef short short8v __attribute__((ext_vector_type(8)));

// Stage inputs [tile0, tile0 + span) of x into the padded LDS image, 16 bytes per global load.  Input pairs (f64) / octets
// (int16) start at even / multiple-of-8 positions, so they never straddle a pad slot: their LDS slots are consecutive.
template <int R>
__device__ __forceinline__ void stage_vec(const double *__restrict__ x, int64_t n, int64_t tile0, int span, int t, double *xs)
{
    for (int p = 2 * t; p < span; p += 2 * kThreads) {
        const int64_t gi = tile0 + p;
        double2v v = {0.0, 0.0};
        if (gi + 1 < n) v = *reinterpret_cast<const double2v *>(x + gi);
        else if (gi < n) v.x = x[gi];
        const int s0 = slot<R>(p);
        xs[s0] = v.x;
        xs[s0 + 1] = v.y;
    }
}

template <int R>
__device__ __forceinline__ void stage_vec(const int16_t *__restrict__ x, int64_t n, int64_t tile0, int span, int t, double *xs)
{
    for (int p = 8 * t; p < span; p += 8 * kThreads) {
        const int64_t gi = tile0 + p;
        short8v v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (gi + 7 < n) v = *reinterpret_cast<const short8v *>(x + gi);
        else {
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (gi + k < n) v[k] = x[gi + k];
        }
        const int s0 = slot<R>(p);                 // p % 8 == 0 (R == 8): the eight slots are consecutive
#pragma unroll
        for (int k = 0; k < 8; ++k) xs[s0 + k] = (double)v[k];
    }
}

template <int R>
__device__ __forceinline__ void fir_acc_image(const double *__restrict__ xs, const double *__restrict__ h, int m, double (&acc)[R]);

// The sums of one tile: acc[r] = output tile*T + t*R + r of the valid-mode FIR, every sum in ascending input order, one fma per tap.
template <typename InT, int R, bool VEC>
__device__ __forceinline__ void fir_tile_acc(const InT *__restrict__ x, int64_t n, const double *__restrict__ h, int m, int64_t tile,
                                             double (&acc)[R])
{
    extern __shared__ double xs[];
    constexpr int T = kThreads * R;
    const int t = threadIdx.x;
    const int span = T + m - 1;
    const int64_t tile0 = tile * T;
    if (VEC) {
        stage_vec<R>(x, n, tile0, span, t, xs);
    } else {
        for (int idx = t; idx < span; idx += kThreads) {
            int64_t gi = tile0 + idx;
            xs[slot<R>(idx)] = gi < n ? (double)x[gi] : 0.0;
        }
    }
    lds_barrier();
    fir_acc_image<R>(xs, h, m, acc);
}

// The sums over an LDS image of the tile's inputs in the padded layout slot<R>() (thread t's window starts at slot t(R+1)).
template <int R>
__device__ __forceinline__ void fir_acc_image(const double *__restrict__ xs, const double *__restrict__ h, int m, double (&acc)[R])
{
    const int t = threadIdx.x;
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.0;
    // Window registers: two sets of R that alternate between "carry" (last R-1 values of the previous block) and "new".
    // With base = t*R the padded LDS index of input p = base + k is t*(R+1) + k + k/R: the lane part is constant and the
    // tap part is the same for every lane, so each read is lane_base + compile-time offset and only lp advances per block.
    static_assert(R == 8, "the block schedule below is written for 8 outputs per thread and 8 taps per block");
    double s0[R], s1[R];
    const double *lp = xs + t * (R + 1);
#pragma unroll
    for (int j = 0; j < R - 1; ++j) s1[j + 1] = lp[j];
    const double *hp = h + (m - 8);          // hp[7 - b] = h[m - 1 - (i0 + b)]: eight contiguous taps per block
    int i0 = 0;
#define PM_FIR_BLOCK(CARRY, NEW)                                                                   \
    {                                                                                              \
        NEW[0] = lp[7];                                                                            \
        _Pragma("unroll") for (int b = 1; b < 8; ++b) NEW[b] = lp[8 + b];                          \
        _Pragma("unroll") for (int b = 0; b < 8; ++b) {                                            \
            const double g = hp[7 - b];                                                            \
            _Pragma("unroll") for (int r = 0; r < R; ++r)                                          \
                acc[r] = __builtin_fma(g, (r + b < 7) ? CARRY[r + b + 1] : NEW[r + b - 7], acc[r]); \
        }                                                                                          \
        lp += R + 1;                                                                               \
        hp -= 8;                                                                                   \
    }
    for (; i0 + 16 <= m; i0 += 16) {
        PM_FIR_BLOCK(s1, s0)
        PM_FIR_BLOCK(s0, s1)
    }
    if (i0 + 8 <= m) {
        PM_FIR_BLOCK(s1, s0)
        i0 += 8;
    }
#undef PM_FIR_BLOCK
    // m % 8 leftover taps: same register-window block with a compile-time tap count (carry is in s0 after an odd number
    // of blocks, else in s1; both cases are handled by copying the carry into s1 first -- seven moves, once per tile)
    if (i0 < m) {
        if ((i0 >> 3) & 1) {
#pragma unroll
            for (int j = 1; j < R; ++j) s1[j] = s0[j];
        }
        const int left = m - i0;
#define PM_FIR_TAIL(K)                                                                             \
        case K: {                                                                                  \
            s0[0] = lp[7];                                                                         \
            _Pragma("unroll") for (int b = 1; b < K; ++b) s0[b] = lp[8 + b];                       \
            _Pragma("unroll") for (int b = 0; b < K; ++b) {                                        \
                const double g = h[left - 1 - b];                                                  \
                _Pragma("unroll") for (int r = 0; r < R; ++r)                                      \
                    acc[r] = __builtin_fma(g, (r + b < 7) ? s1[r + b + 1] : s0[r + b - 7], acc[r]); \
            }                                                                                      \
        } break;
        switch (left) {
            PM_FIR_TAIL(1) PM_FIR_TAIL(2) PM_FIR_TAIL(3) PM_FIR_TAIL(4) PM_FIR_TAIL(5) PM_FIR_TAIL(6) PM_FIR_TAIL(7)
        default: break;
        }
#undef PM_FIR_TAIL
    }
}

template <int R>
size_t lds_bytes(int m) { return (size_t)(slot<R>(kThreads * R + m - 1) + 2) * sizeof(double); }

template <typename K>
int allow_lds(K kernel, size_t bytes)
{
    if (bytes > 64 * 1024)
        PM_HIP(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return PM_OK;
}

}  // namespace
