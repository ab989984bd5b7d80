/*
 * pymodem_amd.h -- C ABI of libpymodem_amd.so: the MI355X (gfx950) implementation of pymodem's
 * demod_chain sample-processing path.  Plain pointers and sizes only; no C++ or torch types.
 *
 * The reference (ninocarrillo/pymodem, pure Python) has no FFI: the "binding" a maintainer adds is
 * a ctypes stub inside each stage class.  Every entry point below names the
 * reference code it replaces (file:line relative to the reference checkout).
 *
 * Conventions
 *   - every function returns 0 on success, a negative pm_status on failure; pm_last_error() gives text
 *   - HIP is initialised in pm_ctx_create(), never at dlopen() time (the reference forks one process
 *     per chain after building its stage objects, pymodem.py:144-151)
 *   - `const T *d_*` / `T *d_*` arguments are DEVICE pointers (from pm_malloc or any HIP allocation of
 *     the same process, e.g. a torch tensor's data_ptr()); `h_*` arguments are HOST pointers
 *   - a pm_ctx owns one HIP stream; calls on one ctx are ordered; a ctx is not thread-safe
 *   - all floating point is IEEE binary64, evaluated in the reference's operation order; FIR sums use
 *     the build's canonical order: ascending input index, one fused multiply-add per tap
 */
#ifndef PYMODEM_AMD_H
#define PYMODEM_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PM_VERSION 100          /* 0.1.0 */

typedef enum pm_status {
    PM_OK = 0,
    PM_ERR_HIP = -1,            /* a HIP runtime call failed (text in pm_last_error) */
    PM_ERR_ARG = -2,            /* bad argument (null pointer, n < taps, unsupported size) */
    PM_ERR_NODEV = -3,          /* no gfx950 device visible */
    PM_ERR_CAPACITY = -4,       /* caller's output buffer too small; required size reported */
    PM_ERR_NOCONVERGE = -5      /* internal: slicer walkers still alive after the launch cap (cannot happen: a walker ends with its stream) */
} pm_status;

typedef struct pm_ctx pm_ctx;

/* ---- library / device ------------------------------------------------------------------------ */
int pm_version(void);
int pm_device_count(void);                               /* 0 when no GPU; never throws */
int pm_last_error(char *buf, size_t cap);                /* copies the calling thread's last message */

int pm_ctx_create(int device, pm_ctx **out);
/* Same, with the stream at one of three priority levels: 1 the device's highest, 0 a plain stream, -1 the device's lowest (both ends
 * from hipDeviceGetStreamPriorityRange; a device with one level gives a plain stream for all three).  Any other level: PM_ERR_ARG.
 * Several ctx may exist on one device: each has its own stream, scratch and profiler, device memory is shared.  The pipelined executor
 * runs the slicer (a few resident waves, dependent-latency bound) on a high-priority ctx while the FIR/correlator kernels of the next
 * recording fill the ALUs.  The level also decides whose hardware queue the stream shares: the runtime pools its queues per priority,
 * so a stream at a level nothing else in the process uses has a queue to itself ("Hardware queues"). */
int pm_ctx_create_prio(int device, int level, pm_ctx **out);
int pm_ctx_stream_priority(pm_ctx *ctx, int *h_priority);      /* hipStreamGetPriority of the context's stream (numerically lower = higher) */
/* A context whose stream may only use the compute units whose bit is set in cu_mask (nwords x 32 bits; bit i goes to XCD
 * i mod 8, so a run of 8 k consecutive bits takes k CUs from every XCD).  The pipelined executor keeps the slicers' few, long-lived,
 * latency-bound waves on a handful of CUs of their own and the FIR kernels on the rest: a FIR workgroup that shares a SIMD with a
 * slicer wave runs at the pace of its slowest wave (its barriers couple the four SIMDs of the CU). */
int pm_ctx_create_cumask(int device, const uint32_t *cu_mask, int nwords, pm_ctx **out);
int pm_device_cus(int device);      /* compute units of the device (0 if it cannot be queried) */
/* Diagnostic switches of a context's launchers (kernel shapes kept for comparison, traces; README.md lists them).  A context reads
 * its switches from the environment (PM_<NAME>) once, when it is made; this call sets one afterwards.  No switch changes a result. */
int pm_ctx_tune(pm_ctx *ctx, const char *name, int64_t value);
int pm_ctx_tuned(pm_ctx *ctx, const char *name, int64_t *h_value);      /* the switch's value as the context holds it now */
int pm_ctx_destroy(pm_ctx *ctx);
/* Cross-stream ordering without a host wait.  pm_event_record marks the point reached by ctx's stream (creating the event when
 * *event is NULL); pm_event_wait makes everything submitted to ctx AFTER the call wait for that point.  Same device only. */
int pm_event_record(pm_ctx *ctx, void **event);
int pm_event_wait(pm_ctx *ctx, void *event);
int pm_event_query(void *event);     /* 1 = everything before the record has finished, 0 = not yet, < 0 = error */
int pm_event_sync(void *event);      /* host wait for the event */
int pm_event_sync_relaxed(void *event, int poll_us);   /* the same without spinning: polls every poll_us microseconds (waits of seconds) */
int pm_event_destroy(void *event);
int pm_ctx_sync(pm_ctx *ctx);                            /* hipStreamSynchronize on the ctx stream */
void *pm_ctx_stream(pm_ctx *ctx);                        /* the hipStream_t, for interop */

int pm_malloc(pm_ctx *ctx, size_t bytes, void **d_out);
int pm_free(pm_ctx *ctx, void *d_ptr);
int pm_h2d(pm_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);   /* async on the ctx stream */
int pm_d2h(pm_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);   /* synchronous */
/* Page-lock a host block the caller owns (and release it again before freeing the block): copies to and from pinned memory go
 * straight over the link instead of through the runtime's bounce buffers.  For blocks that are used many times (the executor's
 * pool of result blocks); pinning costs about as much as one copy of the block. */
int pm_host_pin(pm_ctx *ctx, void *h_block, size_t bytes);
int pm_host_unpin(void *h_block);
/* The context's internal work block (slicer state, sweep intermediates): grow it to at least reserve_bytes now (0: leave it) and
 * report its size.  A host that knows how large its batches will get reserves once instead of paying a free + malloc on the way. */
int pm_ctx_scratch(pm_ctx *ctx, size_t reserve_bytes, size_t *h_bytes);
int pm_d2d(pm_ctx *ctx, void *d_dst, const void *d_src, size_t bytes);        /* device to device, on the context's stream */
int pm_memset(pm_ctx *ctx, void *d_dst, int value, size_t bytes);

/* HIP-event timer on the ctx stream: start, enqueue work, stop -> elapsed milliseconds. */
int pm_timer_start(pm_ctx *ctx);
int pm_timer_stop(pm_ctx *ctx, float *ms);

/* Per-kernel-class timing with HIP events on the ctx stream, for bench.py's roofline line.  While enabled, every
 * launch of a tracked kernel class is bracketed by an event pair; pm_prof_read sums the elapsed times. */
enum { PM_K_FIR_I16 = 0, PM_K_FIR_F64 = 1, PM_K_AFSK_CORR = 2, PM_K_SIGNS = 3, PM_K_SLICE_ITER = 4, PM_K_SLICE_EMIT = 5,
       PM_K_AGC = 6, PM_K_LOOP = 7, PM_K_COUNT = 8 };
int pm_prof_enable(pm_ctx *ctx, int on);                 /* also resets the accumulators */
int pm_prof_read(pm_ctx *ctx, int kernel_class, double *total_ms, int64_t *launches);
/* Algorithmic work of the same launches, summed: compulsory HBM bytes (every input element read once, every output element
 * written once, at their stored width) and f64 flops (2 per fused multiply-add of the FIR sums; epilogues not counted).
 * Zero for the classes that are neither (slicer iterations, carrier loops, AGC). */
int pm_prof_work(pm_ctx *ctx, int kernel_class, double *bytes, double *flops);
/* When each tracked launch of the class began and ended, in milliseconds since one reference event per device (recorded when
 * profiling is first enabled there): launches of several contexts of a device can be laid over each other -- a host that runs
 * the same kernel class on several streams at once learns how many were in flight together and for how long the class kept
 * the GPU busy at all.  *h_n = intervals held (the first min(*h_n, cap) are written). */
int pm_prof_intervals(pm_ctx *ctx, int kernel_class, double *h_start_ms, double *h_end_ms, int64_t cap, int64_t *h_n);

/* ---- FIR stages -------------------------------------------------------------------------------
 * numpy.convolve(x, h, 'valid'): y[k] = sum_j h[j] * x[k+m-1-j], k = 0 .. n-m.  Replaces the 19
 * numpy.convolve call sites (afsk.py:151-166, fsk.py:151, psk.py:165,193,710-751, afsk_pll.py:143,168).
 * d_taps holds h in the reference's order.  flags: PM_FIR_NEGATE writes -y (fsk.py:153-154). */
#define PM_FIR_NEGATE 1
int pm_fir_valid_i16(pm_ctx *ctx, const int16_t *d_x, int64_t n, const double *d_taps, int m, double *d_y, int flags);
/* The same sum for callers that need a value with a bound, not the reference's rounding (the certified AFSK sweeps inside pm_pipe_*):
 * taps quantised to 32-bit integers, samples and taps as signed base-256 digits, exact int32 products on the int8 matrix pipe
 * (v_mfma_i32_16x16x64_i8), recombined in binary64.  |d_y[k] - reference sum| <= *h_bound (~1e-9 of sum|taps| * 32768).  m <= 241,
 * d_x 16-byte aligned, h_taps on the HOST; synchronous (plans its tables per call: the pipeline keeps them).  Test and measurement entry. */
int pm_fir_valid_i16_limbs(pm_ctx *ctx, const int16_t *d_x, int64_t n, const double *h_taps, int m, double *d_y, double *h_bound);
/* What the certified AFSK sweeps' binary32 roots rely on (csrc/pm_afsk.hip: slide_run_f32): the largest error of the device's v_sqrt_f32
 * over ALL 2^24 binary32 values of the binades 2^exponent and 2^(exponent + 1), in units of the result's last place x 1024 (rounded up),
 * against the correctly rounded binary64 root.  Test entry. */
int pm_ubench_sqrt_f32(pm_ctx *ctx, int exponent, int64_t *h_worst_ulp_1024);
/* int8 digit products (v_mfma_i32_16x16x64_i8 operand pairs) per tap and output that the matrix-pipe kernels compute: stage 0 = the
 * certified sweeps' band-pass (sample digits x tap digits), 1 = their low-pass, per stream, 2 = the batch engine's matched filters.
 * From the kernels' own constants: what a measurement prices their launches with.  < 0: no such stage. */
int pm_matrix_digit_pairs(int stage);
/* max(numpy.convolve(row, h, 'valid')) per row -- AGC.apply's `normal` (agc.py:67) over the band-passed recording (psk.py:165, :710) --
 * WITHOUT writing the band-passed rows: matrix-pipe values with the bound above pick the outputs that could be the maximum, the
 * reference's own sum (one fma per tap, ascending input index) decides among them; h_max[r] is bit for bit max() of pm_fir_valid_i16.
 * Rows x_stride samples apart (a multiple of 8) from a 16-byte aligned d_x; *h_redone (may be null) = outputs recomputed.  m <= 241.
 * Test and measurement entry: pm_lbatch_* keeps a plan for its band-pass. */
int pm_bpf8_rows_max_i16(pm_ctx *ctx, const int16_t *d_x, int64_t x_stride, int rows, int64_t n, const double *h_taps, int m, double *h_max,
                         int64_t *h_redone);
int pm_fir_valid_f64(pm_ctx *ctx, const double *d_x, int64_t n, const double *d_taps, int m, double *d_y, int flags);

/* The same FIRs fused with the slicer's sign test: only the (y >= 0) bitmap of the n-m+1 outputs is written (bit k of the
 * little-endian uint64 array; (n-m+1+63)/64 words), not the float64 stream.  For the last FIR of a chain, whose output
 * feeds slicer.slice() and nothing else (afsk.py:166, fsk.py:151, psk.py:193,750-751, afsk_pll.py:168). */
int pm_fir_signs_i16(pm_ctx *ctx, const int16_t *d_x, int64_t n, const double *d_taps, int m, uint64_t *d_bits, int flags);
int pm_fir_signs_f64(pm_ctx *ctx, const double *d_x, int64_t n, const double *d_taps, int m, uint64_t *d_bits, int flags);
/* The same for up to 16 streams that share their taps, in ONE launch: the output low-passes of a chain group (every chain of
 * afsk_1200_ax25_super_opt.json has the same output_lpf).  h_x / h_n / h_bits are HOST arrays of `count` device pointers / lengths. */
int pm_fir_signs_f64_batch(pm_ctx *ctx, int count, const double *const *h_x, const int64_t *h_n, const double *d_taps, int m,
                           uint64_t *const *h_bits, int flags);

/* The same FIRs over `rows` streams of equal length in ONE launch (the band-pass, Hilbert and matched filters of a batch of
 * recordings x chains, pm_lbatch below).  Input row r is d_x + r * x_stride (elements), or -- pm_fir_rows_i16_ptrs, rows that are
 * separate allocations -- d_x_ptrs[r] + x_off with d_x_ptrs a DEVICE array of `rows` device pointers (x_aligned16: every row
 * pointer + x_off is 16-byte aligned, which the library cannot see).  Output row r is d_y + r * y_stride (n - m + 1 doubles) or
 * d_bits + r * bits_stride words.  Every row's result is bit-identical to the single-stream call. */
int pm_fir_rows_i16(pm_ctx *ctx, const int16_t *d_x, int64_t x_stride, int rows, int64_t n, const double *d_taps, int m, double *d_y,
                    int64_t y_stride, int flags);
int pm_fir_rows_i16_ptrs(pm_ctx *ctx, const int16_t *const *d_x_ptrs, int64_t x_off, int x_aligned16, int rows, int64_t n, const double *d_taps,
                         int m, double *d_y, int64_t y_stride, int flags);
int pm_fir_rows_f64(pm_ctx *ctx, const double *d_x, int64_t x_stride, int rows, int64_t n, const double *d_taps, int m, double *d_y,
                    int64_t y_stride, int flags);
int pm_fir_rows_signs_f64(pm_ctx *ctx, const double *d_x, int64_t x_stride, int rows, int64_t n, const double *d_taps, int m, uint64_t *d_bits,
                          int64_t bits_stride, int flags);
/* The same bitmap for LONG filters whose output feeds only a slicer (BPSK / MPSK matched filters, psk.py:193, :750-751): the sums as
 * int8 digit products on the matrix pipe, each sign certified against a proven bound, the undecided outputs recomputed with the
 * canonical binary64 chain (csrc/pm_fir8.hip; 16 <= m <= 1009).  Bit for bit pm_fir_rows_signs_f64's result for every input; this
 * entry point makes its plan per call (tests, measurements) -- the batch engine keeps one.  *h_recomputed: outputs that took the
 * exact path. */
int pm_fir8_rows_signs_f64(pm_ctx *ctx, const double *d_x, int64_t x_stride, int rows, int64_t n, const double *h_taps, int m,
                           uint64_t *d_bits, int64_t bits_stride, int64_t *h_recomputed);

/* AFSK mark/space quadrature correlators fused with magnitude and difference (afsk.py:153-162):
 * y[k] = sqrt(mi*x ^2 + mq*x ^2) - sqrt(si*x ^2 + sq*x ^2), each product a 'valid' convolution. */
int pm_afsk_correlate(pm_ctx *ctx, const double *d_x, int64_t n, const double *d_mark_i, const double *d_mark_q,
                      const double *d_space_i, const double *d_space_q, int m, double *d_y);

/* `groups` AFSK modems over the same band-passed stream that share their MARK correlators and differ in the space correlators
 * only (the chains of afsk_1200_ax25_super_opt.json: same tones and span, space_gain 1.25 ... 2.75, afsk.py:144-145): the mark
 * sums and magnitude are computed once.  d_space = [groups][2][m] (space_i then space_q of modem g); output g is written at
 * d_y + g*y_stride (n-m+1 values each).  Every output is bit-identical to pm_afsk_correlate with that modem's four filters. */
#define PM_AFSK_GROUP_MAX 8
int pm_afsk_correlate_group(pm_ctx *ctx, const double *d_x, int64_t n, const double *d_mark_i, const double *d_mark_q,
                            const double *d_space, int groups, int m, double *d_y, int64_t y_stride);

/* Gain sweep: `groups` (<= 8) AFSK modems over the same band-passed stream that share their mark correlators and whose space
 * correlators are ONE unit pair (d_unit_i/q, space_gain 1.0) scaled by each modem's space_gain (afsk.py:144-145), all with the same
 * output low-pass: writes every modem's slicer sign bitmap (what afsk.py:148-167 followed by `>= 0` gives) from two correlator
 * pairs and two low-passes for the whole sweep.  The bitmaps are certified: a sample whose sign the shared computation cannot
 * guarantee is recomputed by the exact chain of that modem (d_space = [groups][2][m], the modems' own space taps), and if there are
 * more such samples than a fixed list holds (degenerate input) the exact chains of all modems run instead, decided on the device:
 * every bit equals pm_afsk_correlate + pm_fir_signs_f64 for that modem, and the call never waits for the GPU.  x_bound: a bound on
 * |d_x| the caller vouches for (sum|input_bpf| * 32768 for int16 audio); lpf_abs_sum = sum|output_lpf|.
 * pm_afsk_sweep_last (diagnostics; waits for the stream): how many samples the last sweep on this ctx could not certify (above
 * 65536 the exact chains ran). */
int pm_afsk_sweep_signs(pm_ctx *ctx, const double *d_x, int64_t n, double x_bound, const double *d_mark_i, const double *d_mark_q,
                        const double *d_unit_i, const double *d_unit_q, const double *d_space, const double *h_gains, int groups, int m,
                        const double *d_lpf, int ml, double lpf_abs_sum, uint64_t *const *h_bits);
/* The same sweep when the correlator templates are what afsk.py:134-144 makes them, the powers of one rotation per tone
 * (template[j] = cos / sin of j*w): the two magnitude streams come from a sliding sum, Z(k+1) = x[k+m] + r Z(k) - r^m x[k], 6 fused
 * operations per tone and sample instead of 2m, restarted from the direct sum every 16 outputs.  Nothing changes in what is
 * guaranteed: the sliding sums only feed the certified decision, whose bound grows by their (small) error, and every bit still
 * equals the exact chain's.  rot = r = (template_i[1], template_q[1]); end = r^m rounded to double; tap_dev = the largest
 * |template[j] - r^j| over both templates of both tones, measured by the host in extended precision (pymodem_amd.taps.tone_model).
 * Fails with PM_ERR_ARG if tap_dev >= 1e-6: such templates are not tones, use pm_afsk_sweep_signs.  groups == 1 is the lone
 * chain: its mark - gain * space difference takes ONE low-pass.  Sliding sums, low-pass(es) and the certified combine run as one
 * kernel (nothing but the bitmaps is written) unless the low-pass is longer than 2049 taps. */
typedef struct pm_afsk_tones {
    double mark_rot[2], mark_end[2];
    double space_rot[2], space_end[2];     /* of the unit-gain space templates */
    double tap_dev;
} pm_afsk_tones;
int pm_afsk_sweep_signs_tones(pm_ctx *ctx, const double *d_x, int64_t n, double x_bound, const double *d_mark_i, const double *d_mark_q,
                              const double *d_unit_i, const double *d_unit_q, const double *d_space, const double *h_gains, int groups,
                              int m, const double *d_lpf, int ml, double lpf_abs_sum, uint64_t *const *h_bits,
                              const pm_afsk_tones *h_tones);
/* The two magnitude streams the sweep works from, on their own (tests, diagnostics): d_mark_mag[k] = sqrt(I^2 + Q^2) of the mark
 * templates at output k, d_space_mag likewise (n - m + 1 values each; afsk.py:153-160 without the subtraction).  h_tones NULL:
 * the direct sums in the reference's order.  h_tones given: the sliding sums; *h_bound receives the bound on their distance
 * from the direct sums that the certified decision uses (0 for the direct sums). */
int pm_afsk_magnitudes(pm_ctx *ctx, const double *d_x, int64_t n, double x_bound, const double *d_mark_i, const double *d_mark_q,
                       const double *d_space_i, const double *d_space_q, int m, const pm_afsk_tones *h_tones, double *d_mark_mag,
                       double *d_space_mag, double *h_bound);
int pm_afsk_sweep_last(pm_ctx *ctx, int64_t *h_uncertain);
/* Deferred fallback for pipelined hosts.  By default every certified sweep ends with three launches that look at its counter of
 * uncertain samples and -- only if the list overflowed (65536: digital silence, input far below the stated bound) -- run the exact
 * chains after all; in the normal case they leave at once but still cost the stream three dispatches per sweep.  With
 * pm_afsk_sweep_mode(ctx, 1) they are not enqueued: take a ticket after the call, and once the sweep has FINISHED (stream or event
 * synchronised) ask pm_afsk_sweep_result; if *h_uncertain > *h_capacity the sweep's bitmaps are not valid and the caller runs the
 * exact path for those modems (pm_afsk_correlate + pm_fir_signs_f64).  Tickets stay valid for 63 further sweeps on the context. */
/* WHO COUNTS WHERE.  The entry points of this block -- pm_afsk_sweep_signs, pm_afsk_sweep_signs_tones, pm_afsk_group_run,
 * pm_afsk_sweep_last / _ticket / _result / _results -- count a sweep's uncertain samples in a ring of 64 counters that belongs to the
 * CONTEXT (a ticket is a sequence number into it).  They are for one thread per context: submitting sweeps on a context from one
 * thread and asking for their results from another is not supported, and a result must be asked for within 63 further sweeps.
 * The pipelined executor (pm_pipe_*) does NOT use the ring: each of its recordings owns its counters, mailbox words and overflow
 * list from submission until its slicer batch has read them (csrc/pm_common.h: pm_sweep_cells), its matrix-pipe sweeps decide their
 * uncertain samples inside the workgroup that found them, and nothing is shared between its threads. */
/* One chain group's demod stage in one call: band-pass on the int16 audio into d_bpf_out (n - mb + 1 doubles), then every sweep of
 * h_sweeps on it (as pm_afsk_sweep_signs / _tones would run them, fallback deferred), h_tickets[k] = the ticket of sweep k. */
typedef struct pm_afsk_sweep_desc {
    const double *d_mark_i, *d_mark_q, *d_unit_i, *d_unit_q, *d_space;
    const double *h_gains;
    int32_t groups, m;
    const double *d_lpf;
    int32_t ml, reserved;
    double lpf_abs_sum;
    uint64_t *const *h_bits;
    const pm_afsk_tones *h_tones;      /* NULL: direct correlator sums */
} pm_afsk_sweep_desc;
int pm_afsk_group_run(pm_ctx *ctx, const int16_t *d_audio, int64_t n, const double *d_bpf, int mb, double *d_bpf_out, double x_bound,
                      const pm_afsk_sweep_desc *h_sweeps, int nsweeps, int64_t *h_tickets);
int pm_afsk_sweep_mode(pm_ctx *ctx, int deferred);
int pm_afsk_sweep_ticket(pm_ctx *ctx, int64_t *h_ticket);
int pm_afsk_sweep_result(pm_ctx *ctx, int64_t ticket, pm_ctx *via, int64_t *h_uncertain, int64_t *h_capacity);
int pm_afsk_sweep_results(pm_ctx *ctx, const int64_t *h_tickets, int n, pm_ctx *via, int64_t *h_uncertain, int64_t *h_capacity);   /* several sweeps of one context, one copy */   /* via: the context whose stream carries the 4-byte copy (NULL: ctx) */

/* Sign bitmap of a float64 stream: bit k of the little-endian uint64 array = (x[k] >= 0), the only
 * property of a sample the slicers read (slicer.py:85,99-102,210-232).  d_bits holds (n+63)/64 words. */
int pm_signs_f64(pm_ctx *ctx, const double *d_x, int64_t n, uint64_t *d_bits);

/* ---- AGC and carrier loops -------------------------------------------------------------------- */
typedef struct pm_agc_params {       /* AGC.__init__, agc.py:7-24 */
    double attack_rate, decay_rate, sustain_time, sample_rate, target_amplitude;
} pm_agc_params;
/* AGC.apply in place (agc.py:61-80): normal = max(buf), envelope follower, buf[i] = target*s/env.
 * h_state[2] = {envelope, sustain_count}, read and written (carried like self.* in the reference). */
int pm_agc_apply(pm_ctx *ctx, double *d_buf, int64_t n, const pm_agc_params *h_params, double *h_state);

/* The envelope follower and normalisation of AGC.apply (agc.py:68-80) for `rows` streams, each CONTINUED from h_state[2r..] =
 * {envelope, sustain_count} over n more samples, out of place (y may be x): what a recording processed in time chunks needs, where
 * `normal` = max(buffer) over the WHOLE buffer (agc.py:67) is known before the first chunk (h_normal[r]; pm_rows_max_f64 gives the
 * maxima of the rows of a chunk).  Pieces of a buffer run through this one after the other give the bits of pm_agc_apply on the
 * whole.  One lane per row (64 rows per wave) steps the recurrence and divides. */
int pm_agc_rows_apply(pm_ctx *ctx, const double *d_x, int64_t x_stride, double *d_y, int64_t y_stride, int rows, int64_t n,
                      const pm_agc_params *h_params, const double *h_normal, double *h_state);
int pm_rows_max_f64(pm_ctx *ctx, const double *d_x, int64_t x_stride, int rows, int64_t n, double *h_max);

typedef struct pm_loop {             /* one carrier loop = NCO (nco.py) + IIR_1 (iir.py) + PI (pi_control.py) */
    double phase_scaling;            /* 2*pi / sample_rate                       nco.py:31 */
    double index_scaling;            /* 256 / (2*pi)                             nco.py:27 */
    double set_frequency;            /* carrier_freq                             nco.py:13 */
    double b0, b1, a1;               /* gain*b0, gain*b1, a1                     iir.py:15-29 */
    double p_rate, i_rate, i_limit, gain;                                     /* pi_control.py:8-12 */
    /* state, read and written */
    double phase, control, sine, cosine;
    double x0, x1, y0;
    double integral, proportional;
    /* QPSK Costas loop only (psk.py:223-240): the two branch low-pass filters share coefficients; their states */
    double bb0, bb1, ba1;            /* Cosine_LPF / Sine_LPF coefficients       iir.py:15-29 */
    double cx0, cx1, cy0;            /* Cosine_LPF state */
    double sx0, sx1, sy0;            /* Sine_LPF state */
} pm_loop;

/* nloops independent loops over the SAME input (chains that differ only in carrier_freq, e.g.
 * configs/qpsk_2400.json) or, with x_stride != 0, over nloops inputs x + l*x_stride.  One lane per loop.
 * d_table: the 256-entry wavetable amplitude*sin(2*pi*i/256) computed by the caller with libm sin (nco.py:22-24).
 * Outputs are laid out [loop][n] with stride out_stride (elements). */
int pm_costas_bpsk(pm_ctx *ctx, pm_loop *h_loops, int nloops, const double *d_table,
                   const double *d_x, int64_t x_stride, int64_t n, double *d_out, int64_t out_stride);      /* psk.py:173-189 */
int pm_pll_afsk(pm_ctx *ctx, pm_loop *h_loops, int nloops, const double *d_table,
                const double *d_x, int64_t x_stride, int64_t n, double *d_out, int64_t out_stride);         /* afsk_pll.py:153-165 */
/* d_pd_table: int32[64*64] phase-detector table, row-major [real][imag] (phase_detector.py:36-44). */
int pm_mpsk_loop(pm_ctx *ctx, pm_loop *h_loops, int nloops, const double *d_table, const int32_t *d_pd_table,
                 const double *d_re, const double *d_im, int64_t x_stride, int64_t n,
                 double *d_i_out, double *d_q_out, int64_t out_stride);                                     /* psk.py:734-747 */

/* QPSKModem's Costas loop (psk.py:434-467): both mixer products are low-passed (Cosine_LPF, Sine_LPF); the phase detector is
 * cos_lp*sgn(sin_lp) - sin_lp*sgn(cos_lp).  d_i_out receives the SINE branch and d_q_out the COSINE branch, as the reference
 * appends them (psk.py:452-453). */
int pm_costas_qpsk(pm_ctx *ctx, pm_loop *h_loops, int nloops, const double *d_table,
                   const double *d_x, int64_t x_stride, int64_t n, double *d_i_out, double *d_q_out, int64_t out_stride);

/* ---- slicers ----------------------------------------------------------------------------------
 * Symbol-timing PLL + bit decision + byte packing.  Input is the sign bitmap(s) of the demodulated
 * stream.  Output: bytes and their 1-based stream addresses (index of the sample that completed the
 * byte), exactly the AddressedData list of the reference.  Evaluated chunk-parallel: one walker per chunk runs the
 * reference's recurrence, leaves a clock checkpoint per 64-sample word and walks on into the next chunks until it meets the
 * trail in front of it; when no walker is left the result is bitwise the sequential run's (pm_slicer.hip). */
typedef struct pm_slicer_params {
    double samples_per_symbol;       /* sample_rate / symbol_rate              slicer.py:51 */
    double lock_rate;                /*                                         slicer.py:22-33,124-165 */
    int32_t bits_per_symbol;         /* 1 (binary, bpsk) or 2 (qpsk)            slicer.py:127-158 */
    int32_t state_mask;              /* 0x3 or 0xF                              slicer.py:126-157 */
    int32_t demap[16];               /* symbol demap table                      slicer.py:128 */
} pm_slicer_params;
/* h_count receives the number of bytes produced; if it exceeds cap the call returns PM_ERR_CAPACITY
 * (the first cap entries are valid).  A safe cap is n*bits_per_symbol/8 + 1. */
int pm_slice_binary(pm_ctx *ctx, const uint64_t *d_bits, int64_t n, const pm_slicer_params *h_params,
                    uint8_t *d_data, int64_t *d_addr, int64_t cap, int64_t *h_count);                       /* slicer.py:59-107 */
int pm_slice_quadrature(pm_ctx *ctx, const uint64_t *d_bits_i, const uint64_t *d_bits_q, int64_t n,
                        const pm_slicer_params *h_params, uint8_t *d_data, int64_t *d_addr, int64_t cap,
                        int64_t *h_count);                                                                  /* slicer.py:193-242 */
/* Many streams in one launch sequence (chains are independent; batching them shares the iteration launches and the
 * host checks).  d_bits_q == NULL selects the binary slicer for that stream.  `count` is written per job. */
/* What a slicer object carries from one slice() call to the next (slicer.py:49-56,193-202): a second call on the same object
 * continues the first, mid-byte if need be.  All zero (last samples counting as >= 0) is the just-tuned state. */
typedef struct pm_slicer_state {
    double phase_clock;
    int32_t last_i_negative;         /* 1 if the previous call's last I (or only) sample was < 0 */
    int32_t last_q_negative;
    int32_t working_byte;            /* the bits shifted in since the last emitted byte (low working_bits bits are meaningful) */
    int32_t working_bits;
    int32_t state_register;          /* quadrature: previous symbol(s), slicer.py:210 */
    int32_t reserved;
    int64_t streamaddress;           /* samples seen so far: the next sample's address is streamaddress + 1 */
} pm_slicer_state;

typedef struct pm_slice_job {
    const uint64_t *d_bits_i;
    const uint64_t *d_bits_q;
    int64_t n;
    pm_slicer_params params;
    uint8_t *d_data;
    int64_t *d_addr;
    int64_t cap;
    int64_t count;                   /* out */
    pm_slicer_state *h_state;        /* in/out; NULL = start from the just-tuned state and do not report the end state */
} pm_slice_job;
int pm_slice_batch(pm_ctx *ctx, pm_slice_job *h_jobs, int njobs);           /* njobs <= 64 */
/* The output of a finished pm_slice_batch in the form that is cheapest to bring to the host (3 bytes per data byte instead of 9, no
 * unused capacity in between): for job j, at d_block + h_offsets[j]: {first address, last address} (2 x int64), 64 flag bytes,
 * count[j] address steps as uint16 (address[i] - address[i-1], the first one 0; padded to a multiple of 8 bytes), count[j] data
 * bytes (padded likewise) -- PM_COMPACT_HEAD = 80 bytes before the steps.  *h_used = bytes written; PM_ERR_CAPACITY (with *h_used
 * set) if block_bytes is less.  A step is eight symbol periods unless the input keeps the clock from its threshold; if any of the
 * flag bytes is non-zero a step of that stream did not fit 16 bits: take its addresses from its d_addr instead.  Runs on the ctx
 * stream, after the batch; h_jobs are the batch's jobs as pm_slice_batch left them (count filled in). */
#define PM_COMPACT_HEAD 80
int pm_slice_compact(pm_ctx *ctx, const pm_slice_job *h_jobs, int njobs, void *d_block, size_t block_bytes, int64_t *h_offsets,
                     size_t *h_used);
/* The bitstream stage behind the slicers, on the device: what the host stage otherwise does byte by byte with every stream -- the LFSR
 * (lfsr.py:22-52) and the search for the places where a decoder has something to do (ax25.py:36-50,69-89, il2p.py:367-376).  A job is
 * the `n` data bytes a slicer job left on the device (pm_slice_job.d_data, 8-byte aligned), the chain's LFSR (any 64-bit polynomial,
 * the register it starts from) and its codec kind (pm_codec_create; -1: descramble only) with the IL2P codec's sync_tol.  Runs on
 * the ctx stream behind whatever produced the bytes; d_block (8-byte aligned) may be page-locked host memory that the device reaches.
 * For job j, at d_block + h_offsets[j]:
 *   the record, PM_SCAN_HEAD = 32 bytes:
 *       uint64  the LFSR's register behind the stream
 *       int64   bail_bit: the first reset (a flag, or the zero that ends a run of seven ones or more) that lies 8000 bits or more behind
 *               the reset before it (or the stream's start), -1: none.  The list ends in front of it: from the last flag before it
 *               the host decodes byte by byte.  AX.25 only (else -1).
 *       int64   the first bit after the last flag in front of the stream's end (or of the bail bit), -1: no flag.  AX.25 only.
 *       int32   events in the list (AX.25), int32 set bits in the bitmap (IL2P)
 *   the list,
 *       kind 0: n / 19 + 2 places of 8 bytes, the first `events` of them {uint32 P, uint32 F}, ascending: P = the bit (0 = the top bit
 *               of byte 0) of a flag's closing zero, F = the first bit after the flag in front of it (0xFFFFFFFF: none).  Listed are the
 *               stream's first flag and every later flag whose zero is counted bit T of the bits since the last reset, stuffed zeros
 *               left out, with (T & 7) == 7 and T >= 8 * 18 + 7: the flags that close a frame of 18 bytes or more in a decoder that
 *               starts from its just-created state.  Places past `events` are not written.
 *       kind 1: (n + 63) / 64 words of 8 bytes, bit k & 63 of word k >> 6 set when descrambled bytes k - 4 .. k (k >= 4) hold, ending at
 *               one of byte k's eight bits, 24 bits within sync_tol of 0xF15E48 or 32 bits within sync_tol of 0x5D57DF7F
 *       kind -1: nothing
 *   the n descrambled bytes, padded with zeros to a multiple of 8.
 * With pm_scan_job.frames = 1 (kind 0 only; PM_ERR_ARG otherwise) two more pieces follow, for pm_codec_decode_framed:
 *   the frame table, PM_SCAN_FRAME_TABLE_BYTES(n): n / 19 + 2 places of 8 bytes parallel to the list, the first `events` of them
 *       {int32 len, uint32 crc}: the frame that the flag at P closes in a decoder that starts, with everything cleared, at F (at bit 0 when
 *       F is none) -- a zero behind exactly five ones dropped; the seventh one of a run and every one after it clear the bit and byte
 *       counters and the zero that ends the run is not appended, the bytes collected so far stay; every other bit appended, eight appended
 *       bits since the counters were last clear a byte, the first in bit 0.  len: all its bytes (it may exceed PM_PKT_MAX), 0: the flag
 *       closes nothing (the stream's first flag only); crc: pm_crc16_ccitt of the frame less its last two bytes.  Places past `events`
 *       are not written.
 *   the frame area, PM_SCAN_FRAME_AREA_BYTES(n): frame e lies at byte max(F, 0) >> 3 (it ends in front of byte (P >> 3) + 1, so frames
 *       do not overlap); bytes that no frame covers are not written.
 * One more launch, a wave per event, pm_ctx_tune(ctx, "bitscan_frame_words", 1 .. 64) words of the span per trip (0: 64); results do
 * not depend on it.
 * With pm_scan_job.packets = 1 (kind 1 only; PM_ERR_ARG otherwise) two more pieces follow the descrambled bytes, for
 * pm_codec_decode_packets; the pieces in front are byte for byte what they are without it.  An ATTEMPT is what an IL2P decoder with the job's
 * il2p_crc, il2p_disable_rs and il2p_min_dist does from the bit H at which it enters its header state until it is back in sync search; it
 * depends on nothing but the descrambled bits from H on.  For a candidate byte k of the bitmap let S be the smallest of its bit offsets
 * 0 .. 7 at which the sync test hits on the 32 bits that end there: H = 8 k + S + 1.
 *   the packet table, PM_SCAN_PACKET_TABLE_BYTES(n): {int32 records, int32 placed, 8 bytes zero}, then n / 64 + 2 places of 16 bytes, the first
 *       `records` of them one per candidate in ascending order (candidates behind the last place get none; places past `records` are not
 *       written):
 *           uint32 at       k << 3 | S
 *           uint32 off      where the packet lies in the area, a multiple of 8 (0xFFFFFFFF: nowhere)
 *           uint16 count    the header's payload byte count
 *           uint8  status   0 INCOMPLETE  the stream ends before the attempt's last bit (the header's 120 bits; with a good header its blocks
 *                                         and, with il2p_crc, the four CRC bytes): nothing but `at` is filled
 *                           1 HEADER_FAIL the header's RS(2) fails: the attempt ends 120 bits behind H
 *                           2 DONE        header and every block decode: 13 descrambled header bytes and `count` payload bytes lie at `off`
 *                           3 BLOCK_FAIL  a block's RS(16) fails: the attempt ends at that block's last bit
 *                           4 NOT_PLACED  a good, complete header that found no room in the area (this record's and every later one's)
 *           uint8  corrected  what the attempt adds to the decoder's count of corrected bytes
 *           uint32 end      the bits from H to where the attempt ends, the CRC bytes not counted
 *       placed: the records with a place in the area (DONE and BLOCK_FAIL).
 *   the packet area, PM_SCAN_PACKET_AREA_BYTES(n): records take (13 + count + 7) & ~7 bytes each in ascending order, zeros behind the payload;
 *       bytes that no DONE record covers are not written.  (A real packet takes more of the stream than of the area, so real packets always
 *       fit; chance headers and planted overlaps can run the area out.)
 * Two more launches: one wave per job takes the candidates 64 at a time, a lane a header; pm_ctx_tune(ctx, "bitscan_packet_waves", 1 .. 1024)
 * waves per job (0: 64) share the placed records' blocks.  Results do not depend on it.
 * With pm_scan_job.addrs = 1 (any kind; d_addr: the n stream addresses that the slicer job left beside its bytes, pm_slice_job.d_addr;
 * PM_ERR_ARG when it is NULL) one more piece follows everything above -- behind the frame or packet pieces when they are on -- and the
 * pieces in front are byte for byte what they are without it:
 *   the address checkpoints, PM_SCAN_ADDR_BYTES(n): (n + 63) / 64 places of 8 bytes, A[w] = the int64 stream address of data byte
 *       PM_SCAN_ADDR_STRIDE * w.  With them and the 16-bit steps of pm_slice_compact the host resolves the address of byte k as A[k >> 6] plus
 *       steps (k & ~63) + 1 .. k -- 63 additions at most -- where a decoder asks for one, and expands nothing (pm_codec_decode_addrs).
 * No launch of its own: the tile launch's lanes store them, for tiles behind a bail too.
 * *h_used = bytes the batch needs; PM_ERR_CAPACITY (with *h_used set) if block_bytes is less.  n <= 2^29, njobs <= 64.  Tiles of
 * pm_ctx_tune(ctx, "bitscan_tile_words", 1 .. 256) 64-bit words (0: the default, 256); results do not depend on it. */
#define PM_SCAN_HEAD 32
#define PM_SCAN_LIST_BYTES(kind, n) ((kind) == 0 ? 8 * ((n) / 19 + 2) : (kind) == 1 ? 8 * (((n) + 63) / 64) : 0)     /* the list's bytes: the descrambled bytes lie behind it */
#define PM_SCAN_FRAME_TABLE_BYTES(n) (8 * ((n) / 19 + 2))       /* frames: behind the descrambled bytes (padded to 8) ... */
#define PM_SCAN_FRAME_AREA_BYTES(n) (((n) + 7) / 8 * 8)         /* ... and behind the table */
#define PM_SCAN_PACKET_TABLE_BYTES(n) (16 + 16 * ((n) / 64 + 2))  /* packets: behind the descrambled bytes (padded to 8) ... */
#define PM_SCAN_PACKET_AREA_BYTES(n) (((n) + 7) / 8 * 8)          /* ... and behind the table */
#define PM_SCAN_ADDR_STRIDE 64                                    /* addrs: a checkpoint per this many data bytes ... */
#define PM_SCAN_ADDR_BYTES(n) (8 * (((n) + 63) / 64))             /* ... behind everything else of the job's part */
typedef struct pm_scan_job {
    const uint8_t *d_data;
    int64_t n;
    uint64_t lfsr_poly;
    uint64_t lfsr_state;             /* the register in front of the stream (a stream scanned in pieces: the record's of the piece before) */
    int32_t lfsr_invert;
    int32_t codec_kind;              /* 0 AX.25, 1 IL2P, -1 none */
    int32_t sync_tol;
    int32_t frames;                  /* 1 (kind 0 only): the frame table and the frame area behind the descrambled bytes */
    int32_t packets;                 /* 1 (kind 1 only): the packet table and the packet area behind the descrambled bytes ... */
    int32_t il2p_crc, il2p_disable_rs, il2p_min_dist;      /* ... for a codec with these options (pm_codec_create) */
    const int64_t *d_addr;           /* with addrs: the stream addresses of the n bytes, on the device */
    int32_t addrs;                   /* 1 (any kind): the address checkpoints behind everything else of the part */
    struct pm_scan_carry *d_carry;   /* NULL, or the stream's carry (below): the job is the next PIECE of a stream; lfsr_state is ignored */
} pm_scan_job;
int pm_stream_scan(pm_ctx *ctx, const pm_scan_job *h_jobs, int njobs, void *d_block, size_t block_bytes, int64_t *h_offsets, size_t *h_used);
/* A stream scanned in PIECES: what one piece hands to the next, in device memory, owned by the caller, one per stream (8-byte aligned).  A job
 * with d_carry starts from it instead of from a just-created decoder's state -- word 0's LFSR term is `lfsr_state`, the bits in front of
 * word 0 are `tail`, the bits counted since the last reset are `counted` -- and leaves it as the stream stands behind the piece, so that
 * the records, lists, frames and packets of the pieces are what a decoder that is fed the pieces one after the other has to do.  The pieces
 * of a stream go in stream order through calls on the same context's stream; nothing waits for the host in between.  Two jobs of one call
 * that name the same carry are PM_ERR_ARG.
 *   state   START: nothing scanned yet, the decoder is just created.  OK: `ones` and `counted` are the decoder's.  LOST: the piece before
 *           bailed (or the carry was seeded so): the decoder's counters are not known, the first reset of the next piece is its bail bit and
 *           the host takes that piece through its table; pm_scan_carry_set from the codec's registers (pm_codec_scan_state) makes it OK again.
 *   counted behind the piece's last reset: 8 n - (last reset + 1) - the stuffed zeros dropped behind it; without a reset in the piece what
 *           it was plus 8 n - the piece's dropped zeros -- wherever a bail fell.  AX.25 jobs only (others leave it as it is).
 * What differs from a job without a carry in a piece that does not start in START: the stream's first listed flag (F none) may close a
 * frame that began in an earlier piece, whose bytes the device does not have: with `frames` its table entry is {len -1, crc 0}, "not made",
 * and the host takes the bytes up to that flag through its registers.  An IL2P attempt that runs past the piece's end is INCOMPLETE.
 * A part made with a carry ends with one more piece, the CARRY PIECE, PM_SCAN_CARRY_BYTES behind everything else (behind the address
 * checkpoints when those are on): what the job started from,
 *       int32 state, int32 ones, int64 counted, int64 pieces, int64 bytes
 * for the host to hold its codec against (pm_codec_decode_carried).  Everything in front of it lies where it lies without a carry, and for a
 * START carry is byte for byte the same. */
#define PM_SCAN_CARRY_START 0
#define PM_SCAN_CARRY_OK 1
#define PM_SCAN_CARRY_LOST 2
#define PM_SCAN_CARRY_BYTES 32
typedef struct pm_scan_carry {
    uint64_t lfsr_state;             /* the LFSR's register behind the last piece */
    uint64_t tail;                   /* the last 64 descrambled bits (after invert) in stream order: bit 63 is the stream's last bit */
    int64_t counted;                 /* bits appended since the last reset, stuffed zeros left out: the decoder's nbytes * 8 + nbits */
    int64_t pieces, bytes;           /* pieces and bytes taken so far */
    int32_t ones;                    /* the run of ones that ends the stream so far, capped at 7 */
    int32_t state;                   /* PM_SCAN_CARRY_START / _OK / _LOST */
} pm_scan_carry;
/* Seed a carry, enqueued on the ctx stream: (reg, 0, 0) starts a stream -- state START, for a just-created codec; other values seed OK from a
 * decoder that has been fed (ones, counted: pm_codec_scan_state), with `ones` ones behind a zero as the tail; counted < 0 seeds LOST.
 * pieces and bytes start at 0. */
int pm_scan_carry_set(pm_ctx *ctx, pm_scan_carry *d_carry, uint64_t lfsr_state, int32_t ones, int64_t counted);
/* How many chunks (= walkers) a batch is cut into on this ctx, within 1024..16384 samples per chunk; 0 restores the default 16384.
 * Lane-steps are N (1 + m/L) for merge length m (10-20 k samples) and chunk length L, the depth is (L + longest merge) x the
 * step time: long chunks are cheap, short ones are quick.  Results do not depend on it. */
int pm_slicer_tune(pm_ctx *ctx, int64_t target_lanes);
/* The longest chunk, in 64-sample words (0 restores the default 384 = 24.6 k samples: the optimum when a batch is a few dozen streams
 * and its depth matters, as in the pipelined executor).  A host that slices thousands of streams after a run of the batch engine has
 * its parallelism in the streams and several calls in flight: long chunks (thousands of words) do N (1 + m/L) lane-steps with m/L
 * close to nothing instead of 0.6.  Results do not depend on it. */
int pm_slicer_limits(pm_ctx *ctx, int64_t max_chunk_words);
/* Diagnostics of the last slicer call on this ctx: lockstep launches until no walker was left, chunk length, chunks. */
int pm_slicer_stats(pm_ctx *ctx, int32_t *iterations, int32_t *chunk_len, int64_t *chunks);

/* ---- whole chain: modem + slicer in one call ---------------------------------------------------
 * chain_execute.process_chain up to and including slicer.slice (chain_execute.py:8-14) for one demod_chain: the stage entry points
 * above, strung together in the order of the reference's demod() (afsk.py:148-167, fsk.py:149-159, psk.py:162-195, psk.py:705-773,
 * afsk_pll.py:140-170) with every intermediate kept on the device.  The host designs the taps (firwin / RRC / Hilbert / tones) and
 * hands them over; pointers inside the desc are read during pm_chain_create only.  A chain carries the AGC envelope and the
 * carrier-loop state from one pm_chain_run to the next, like the reference's stage objects; pm_chain_reset returns it to the
 * just-created state.  Output: the slicer's bytes and 1-based stream addresses; when more than `cap` were produced the call
 * returns PM_ERR_CAPACITY with the required size in *h_count -- the run HAS happened (AGC, loop and slicer state have moved on
 * with the stream) and its output is kept on the device: call pm_chain_fetch with buffers of that size, do not run again. */
enum { PM_MODEM_AFSK = 0, PM_MODEM_FSK = 1, PM_MODEM_BPSK = 2, PM_MODEM_MPSK = 3, PM_MODEM_AFSK_PLL = 4, PM_MODEM_QPSK = 5 };
#define PM_CHAIN_INVERT 1       /* FSK: negate the filter output (fsk.py:153-154) */
/* Opt-in: every FIR of the chain continues from the tail of its own input stream instead of starting afresh with every run as the
 * reference's per-call numpy.convolve(..., 'valid') does (afsk.py:151-166, fsk.py:151, psk.py:165,193,710-751, afsk_pll.py:143,168).
 * AFSK / FSK (FIRs and pointwise operations only): the last sum(M - 1) input samples of a run go in front of the next run's input, and
 * a recording fed in pieces gives the bytes, addresses and packets of the single call on the whole.  Carrier-loop
 * modems (BPSK, MPSK, QPSK, AFSK-PLL): band-pass, Hilbert pair and matched / output filter each keep M - 1 samples of their input
 * (on the device); AGC envelope and loop registers are carried anyway; AGC.apply still normalises by the maximum of each run's
 * band-passed samples (agc.py:67), so pieces are what the reference's primitives give when fed this way, not the single call.
 * A run that does not bring a stage up to its filter length produces nothing yet (*h_count = 0). */
#define PM_CHAIN_CARRY_HISTORY 2
typedef struct pm_chain_desc {
    int32_t modem;                                   /* PM_MODEM_* */
    int32_t flags;
    const double *input_fir;  int32_t n_input_fir;   /* input_bpf (afsk, bpsk, mpsk, afsk_pll) or input_lpf (fsk) */
    const double *mark_i, *mark_q, *space_i, *space_q; int32_t n_corr;      /* afsk */
    const double *hilbert;    int32_t n_hilbert, hilbert_delay;             /* mpsk: Hilbert taps; delay = (n_hilbert-1)/2 */
    const double *output_fir; int32_t n_output_fir;  /* output_lpf (afsk, afsk_pll) or the RRC matched filter (bpsk; mpsk both arms) */
    int32_t use_agc;          pm_agc_params agc;     /* bpsk, mpsk, afsk_pll */
    pm_loop loop;                                    /* carrier loop parameters and initial state */
    const double *wavetable;                         /* 256 entries (nco.py:22-24) */
    const int32_t *pd_table;                         /* 64 x 64 (phase_detector.py:36-44), mpsk */
    int32_t quadrature;                              /* 1: QuadratureSlicer (mpsk, qpsk), 0: BinarySlicer */
    pm_slicer_params slicer;
} pm_chain_desc;
typedef struct pm_chain pm_chain;
int pm_chain_create(pm_ctx *ctx, const pm_chain_desc *desc, pm_chain **out);
int pm_chain_run(pm_chain *chain, const int16_t *audio, int64_t n, int audio_on_device,
                 uint8_t *h_data, int64_t *h_addr, int64_t cap, int64_t *h_count);
int pm_chain_fetch(pm_chain *chain, uint8_t *h_data, int64_t *h_addr, int64_t cap, int64_t *h_count);   /* the last run's output, again */
int pm_chain_reset(pm_chain *chain);
int pm_chain_destroy(pm_chain *chain);

/* ---- batch engine for the carrier-loop modems: many recordings x chains in flight -----------------
 * A carrier loop (psk.py:173-189, psk.py:734-747, afsk_pll.py:153-165) is one dependent chain per sample: a GPU lane cannot make it
 * faster than a host core, it can only run hundreds at once.  pm_lbatch runs `recordings` recordings of equal length through
 * `chains` chains that share their front end (band-pass, AGC, Hilbert pair: the chains of configs/qpsk_2400.json differ in
 * carrier_freq only) in time chunks, all recordings x chains loops in ONE launch per chunk, every sequential state (AGC envelope,
 * loop registers, FIR histories) carried in device memory from chunk to chunk.  Output: the sign bitmap(s) of every chain's
 * demodulated stream (what modem.demod() followed by `>= 0` gives: psk.py:162-195, psk.py:705-773, afsk_pll.py:140-170,
 * psk.py:426-476), stream s = recording * chains + chain at d_bits_i + s * bits_stride words (and d_bits_q for the quadrature
 * modems), ready for pm_slice_batch.  Bit-identical to the per-recording entry points for every chunk length. */
typedef struct pm_lbatch_desc {
    int32_t modem;                                   /* PM_MODEM_BPSK | PM_MODEM_MPSK | PM_MODEM_AFSK_PLL | PM_MODEM_QPSK */
    int32_t recordings;                              /* most recordings a run will bring */
    int32_t chains;                                  /* carrier loops per recording */
    int32_t chunk;                                   /* final-filter outputs per chunk (rounded up to 2048s; 0 = 262144) */
    const double *input_fir;  int32_t n_input_fir;   /* input_bpf */
    const double *hilbert;    int32_t n_hilbert, hilbert_delay;             /* mpsk */
    const double *output_fir; int32_t n_output_fir;  /* RRC matched filter (bpsk, qpsk; mpsk both arms) or output_lpf (afsk_pll) */
    pm_agc_params agc;
    const pm_loop *loops;                            /* `chains` loops: parameters and initial state (the same for every recording) */
    const double *wavetable;                         /* 256 entries (nco.py:22-24) */
    const int32_t *pd_table;                         /* 64 x 64 (phase_detector.py:36-44), mpsk */
} pm_lbatch_desc;
typedef struct pm_lbatch pm_lbatch;
int pm_lbatch_create(pm_ctx *ctx, const pm_lbatch_desc *desc, pm_lbatch **out);      /* pointers inside desc are read here only */
/* samples per demodulated stream, outputs per chunk and chunks for recordings of n samples */
int pm_lbatch_geometry(pm_lbatch *batch, int64_t n, int64_t *h_nout, int64_t *h_chunk, int64_t *h_chunks);
/* h_d_audio: HOST array of `recordings` device pointers to int16 recordings of n samples each (they may be the same buffer).
 * Everything is enqueued (three streams: the context's and two of the engine's own); nothing waits for the GPU: the bitmaps are
 * complete when the context's stream has reached the end of the call.  Every run starts from fresh AGC and loop states.
 * bits_stride >= (nout + 63) / 64 + 1 words. */
int pm_lbatch_run(pm_lbatch *batch, const int16_t *const *h_d_audio, int recordings, int64_t n, uint64_t *d_bits_i, uint64_t *d_bits_q,
                  int64_t bits_stride, int64_t *h_nout);
/* The same run with the slicers inside it (slicer.py:59-107, :193-242): every stream (recording r, chain c: row r * chains + c) is
 * sliced chunk by chunk behind its matched filter by a lane of its own that carries the slicer's state through the run, so no sign
 * bitmap of a whole recording exists (16 384 streams of ten minutes: 59 GB each for I and Q) and nothing is left to slice when the run
 * ends.  h_params: one parameter set per chain; every stream starts from the just-tuned slicer state.  Output, per row: up to `cap`
 * (a multiple of 8) data bytes at d_data + row * cap, their address steps (address[i] - address[i-1], the first 0) at d_steps + row * cap,
 * and the row's record: count (bytes produced -- beyond cap they are counted, not stored, and flags has bit 1), the first and last
 * address, the slicer's end state (pm_slicer_state's fields) and flags (bit 0: a step did not fit 16 bits -- slice that run the
 * other way).  Results equal pm_lbatch_run + pm_slice_batch on every stream, byte for byte and address for address. */
typedef struct pm_rowslice_rec {
    int64_t count, first_addr, last_addr, seen;      /* seen: samples consumed (streamaddress) */
    double clk;                                      /* phase_clock */
    int32_t li_neg, lq_neg, wbyte, wbits, sreg, flags;
} pm_rowslice_rec;
int pm_lbatch_run_sliced(pm_lbatch *batch, const int16_t *const *h_d_audio, int recordings, int64_t n, const pm_slicer_params *h_params, int nparams,
                         uint8_t *d_data, uint16_t *d_steps, int64_t cap, pm_rowslice_rec *d_recs, int64_t *h_nout);
/* Rows [row0, row0 + nrows) of such a run as one dense block for the way to the host: row k at the sum of the sizes before it, its
 * min(count, cap) steps (padded to 8 bytes) then its data bytes (padded to 8).  On the ctx stream; nrows <= 4096. */
int pm_rows_gather(pm_ctx *ctx, const pm_rowslice_rec *d_recs, const uint8_t *d_data, const uint16_t *d_steps, int64_t cap, int64_t row0, int nrows,
                   void *d_block, size_t block_bytes);
/* pm_stream_scan for rows [row0, row0 + nrows) of such a run, one call for the lot: row row0 + r is a stream of chain (row0 + r) % nchains
 * (what pm_scan_job says about a stream apart from where it lies), its bytes the n = min(count, cap) bytes at d_data + (row0 + r) * cap.
 * For row r, at d_block + h_offsets[r]: the row's n address steps (uint16, padded to 8 bytes, as pm_rows_gather writes them) and directly
 * behind them exactly what pm_stream_scan writes for a job with these bytes and this chain -- PM_SCAN_HEAD, the list, the descrambled
 * bytes, with frames or packets the table and the area.  The raw slicer bytes are not repeated.  h_counts[r]: that n as the host read it
 * from the records, for the grids, *h_used and h_offsets; the kernels go by a row table that a first small launch makes on the device
 * from d_recs itself (block offset, n, first tile, first places in the device-side lists; pm_bitscan_rows.h), and a row whose part would
 * pass block_bytes or what h_counts sized is left out.  Nothing is uploaded, allocated beyond the context's scratch or waited for;
 * d_block (8-byte aligned) may be page-locked host memory.  nrows <= 4096, nchains <= 64, n <= 2^29; PM_ERR_CAPACITY with *h_used set as in
 * pm_stream_scan.  The tunes bitscan_tile_words, bitscan_frame_words and bitscan_packet_waves mean what they mean there (by default a row's
 * events are shared by 16 waves and its placed records by 8); results do not depend on them.
 * With pm_rows_scan_chain.addrs = 1 the rows of that chain get the address checkpoints of pm_scan_job.addrs at the end of their part,
 * PM_SCAN_ADDR_BYTES(n): A[w] = d_recs[row].first_addr + steps[1] + ... + steps[64 w] over the row's steps at d_steps + row * cap -- a prefix
 * sum in three steps: the tile launch sums each tile's steps, the combine launch carries an int64 prefix from tile to tile, one more small
 * launch scans the lanes of every tile and stores.  A row that is left out gets none; the checkpoints of a row whose record has flag bit 0
 * mean as little as its steps do. */
typedef struct pm_rows_scan_chain {
    uint64_t lfsr_poly, lfsr_state;
    int32_t lfsr_invert, codec_kind, sync_tol, frames, packets, il2p_crc, il2p_disable_rs, il2p_min_dist;
    int32_t addrs;                   /* 1: the address checkpoints at the end of the row's part */
} pm_rows_scan_chain;
int pm_rows_scan(pm_ctx *ctx, const pm_rowslice_rec *d_recs, const uint8_t *d_data, const uint16_t *d_steps, int64_t cap, int64_t row0, int nrows,
                 const pm_rows_scan_chain *h_chains, int nchains, const int64_t *h_counts, void *d_block, size_t block_bytes, int64_t *h_offsets,
                 size_t *h_used);
/* Rows scanned in PIECES: pm_rows_scan with pm_stream_scan's carry (pm_scan_job.d_carry) per row, so that the rows of a run can be taken
 * time chunk by time chunk with nothing waiting for the host.  d_carries: one pm_rows_carry per row of the RUN, in device memory, owned by
 * the caller, 8-byte aligned, indexed by row (row0 + r).  pm_rows_carry_start sets rows [row0, row0 + nrows) to state START with their
 * chain's lfsr_state and taken = 0, in one launch on the ctx stream.  pm_scan_carry_set on &d_carries[row].scan re-seeds a row (behind a
 * bail: state LOST) and leaves taken and last_addr alone.
 * The piece of row row0 + r is decided on the device, in the call's first launch, from the record's count and the carry:
 *       avail = min(d_upto ? d_upto[r] : count, min(count, cap)),  from = taken,
 *       n = avail - from, rounded down to a multiple of 8 unless `final`, never below 0.
 * All but the final cut are multiples of 8: a row begins on an 8-byte boundary (cap is a multiple of 8), so every piece's bytes and its
 * steps at d_steps + row * cap + from keep their 8-byte alignment; up to seven bytes held back go with the next piece.  A row whose
 * `taken` is no multiple of 8 has had its final piece and gives empty pieces from then on.  An empty piece is a piece: record, carry piece,
 * scan.pieces + 1.  d_upto (device, int64 per r, 8-byte aligned) may be NULL: the records' counts.  h_counts[r] must be that same n -- the
 * host knows what it passed as upto, the counts where they matter, and what it has taken; a row whose part would pass what h_counts sized is
 * left out: no launch stores anything for it, in block, scratch or carry.
 * For row r, at d_block + h_offsets[r]: what pm_rows_scan writes for a row of these n bytes -- the piece's n steps padded to 8, the scan part,
 * with addrs the checkpoints -- and behind it PM_ROWS_PIECE_TAIL_BYTES: the job form's carry piece (the carry-in echoed, PM_SCAN_CARRY_BYTES)
 * and int64 addr_before, the stream address of the byte in front of the piece: d_recs[row].first_addr while taken == 0 (where the row's
 * first step is 0), last_addr after that.  The address of the piece's byte i is addr_before + steps[0] + ... + steps[i] -- the piece's first
 * step counts -- and a checkpoint is A[w] = addr_before + steps[0 .. 64 w].
 * Every launch takes from the carry what pm_stream_scan's launches take from pm_scan_job.d_carry, the tile and combine launches from the
 * carry itself, those behind them from a copy in context scratch: the register in front of word 0, the tail, START or not, the counted
 * bits, the "not made" entry for a first listed flag that closes a frame from an earlier piece; an IL2P attempt that runs past the piece is
 * INCOMPLETE; a bail writes LOST as the carry-out.  Lane 0 of the combine wave is the carry's only writer: scan as the job form leaves it,
 * taken += n, last_addr = addr_before + the piece's steps.
 * Arguments as for pm_rows_scan; d_carries non-NULL and 8-byte aligned, d_upto 8-byte aligned when given.  nrows <= 4096, nchains <= 64,
 * PM_ERR_CAPACITY with *h_used set, nothing uploaded, allocated beyond context scratch or waited for.  Two calls for the same rows must
 * follow each other on one context's stream. */
#define PM_ROWS_PIECE_TAIL_BYTES 40
typedef struct pm_rows_carry {
    pm_scan_carry scan;              /* exactly the job form's carry */
    int64_t taken;                   /* bytes of the row that earlier pieces took: where the next piece begins */
    int64_t last_addr;               /* stream address of byte taken - 1 (meaningless while taken == 0) */
} pm_rows_carry;
int pm_rows_carry_start(pm_ctx *ctx, pm_rows_carry *d_carries, int64_t row0, int nrows, const pm_rows_scan_chain *h_chains, int nchains);
int pm_rows_scan_pieces(pm_ctx *ctx, const pm_rowslice_rec *d_recs, const uint8_t *d_data, const uint16_t *d_steps, int64_t cap, int64_t row0, int nrows,
                        const pm_rows_scan_chain *h_chains, int nchains, pm_rows_carry *d_carries, const int64_t *d_upto, int32_t final,
                        const int64_t *h_counts, void *d_block, size_t block_bytes, int64_t *h_offsets, size_t *h_used);
/* FINISHED ROWS: the pm_packet rows of rows [row0, row0 + nrows) of a sliced run, made on the device from the block that pm_rows_scan has
 * just written for the same rows -- exactly the rows that pm_codec_fetch hands out for a just-created codec that is fed the row
 * (pm_codec_decode_addrs), wherever the row's frame table or packet table says everything about it.  Enqueued on the ctx stream behind that
 * pm_rows_scan; d_recs, d_steps, cap, row0, nrows, h_chains, nchains, h_counts, d_block and h_offsets are its arguments and results, unchanged.
 * Every chain with a codec must have been scanned with the table of its kind (frames for AX.25, packets for IL2P) and with addrs;
 * PM_ERR_ARG otherwise.  (A chain of kind -1 has no packets: its rows are entered as NO_CODEC.)  h_sources[c]: what goes into
 * pm_packet.source_decoder for chain c, NULL: c.
 * d_block must be DEVICE memory: these launches read it -- the record, the list, the descrambled bytes, the table, the area and the
 * checkpoints of every row.  If the runtime says it is host memory the call returns PM_ERR_ARG.  (pm_rows_scan's own launches never read
 * the block: what they need of their own results they keep in context scratch, which is why its block may be page-locked host memory.)
 * d_out (8-byte aligned, out_bytes of device memory) receives
 *     pm_rows_packets_head                 16 bytes: the rows of the call, how many of them are not FINISHED, the packet rows that follow
 *     pm_rows_packets_entry[nrows]         32 bytes a row
 *     pm_packet[head.packets]              in row order; a row's packets lie at `first`, consecutively, in stream order
 * so that the rows of a recording lie chain after chain in config order.  An entry holds the LFSR register behind the row (the scan
 * record's), a status, the row's packet count, its first packet row, and for a FINISHED IL2P row the decoder's count of corrected bytes
 * that no packet has taken (il2p.py:203-212 never clears it when a block fails).  Status FINISHED: the packets are all there is to say about
 * the row.  Every other status names why the row is handed over -- it has no packet rows and is decoded the existing way:
 *     IL2P   NO_RECORD   the decoder's sync test hits where the table has no record (a place its register finds and the bitmap does not)
 *            INCOMPLETE / NOT_PLACED   the record at a hit is one
 *            LATE_HIT    a second hit in the byte in which an attempt ends
 *            TABLE_FULL  the table has no free place left: candidates may have gone without a record
 *     AX.25  SHORT       fewer than 24 bytes (pm_codec_decode_framed walks such a stream)
 *            BAIL        the record has a bail bit: frames may lie behind it
 *            LONG_FRAME  a table entry with more bytes than the span between its flags holds (pm_codec_decode_framed refuses such a table).
 *                        A frame longer than PM_PKT_MAX is no reason: its row is cut as pm_codec_fetch cuts it.
 *     any    LEFT_OUT    pm_rows_scan left the row out (records and h_counts disagree)
 *            NO_ROOM     see below
 *            NO_CODEC    the row's chain has codec_kind -1
 * The packet capacity is what out_bytes leaves behind the entries, in whole rows.  The first row whose packets would pass it takes none and
 * is NO_ROOM, and so is every row behind it, whatever its walk said; their `first` is head.packets.  *h_used = the smallest out_bytes that
 * holds head and entries (PM_ERR_CAPACITY, with it set, when out_bytes is less).  Nothing is uploaded, allocated beyond context scratch or
 * waited for.  nrows <= 4096, nchains <= 64.  Three launches: a lane a row walks the row's table by the rule (pm_rows_packets.h) and lists
 * what it accepts in context scratch; one workgroup scans the rows' counts, trips of 256 with a carry, for `first`, NO_ROOM and the head;
 * a fixed grid of waves builds the packet rows, wave w the packets w, w + waves, ... */
#define PM_ROWS_PACKETS_FINISHED 0
#define PM_ROWS_PACKETS_NO_RECORD 1
#define PM_ROWS_PACKETS_INCOMPLETE 2
#define PM_ROWS_PACKETS_NOT_PLACED 3
#define PM_ROWS_PACKETS_LATE_HIT 4
#define PM_ROWS_PACKETS_TABLE_FULL 5
#define PM_ROWS_PACKETS_SHORT 6
#define PM_ROWS_PACKETS_BAIL 7
#define PM_ROWS_PACKETS_LONG_FRAME 8
#define PM_ROWS_PACKETS_LEFT_OUT 9
#define PM_ROWS_PACKETS_NO_ROOM 10
#define PM_ROWS_PACKETS_NO_CODEC 11
typedef struct pm_rows_packets_head {
    int32_t rows, handed;
    int64_t packets;
} pm_rows_packets_head;
typedef struct pm_rows_packets_entry {
    uint64_t lfsr_state;
    int32_t status, packets;
    int64_t first;
    int32_t corrected_left, reserved;
} pm_rows_packets_entry;
int pm_rows_packets(pm_ctx *ctx, const pm_rowslice_rec *d_recs, const uint16_t *d_steps, int64_t cap, int64_t row0, int nrows,
                    const pm_rows_scan_chain *h_chains, int nchains, const int32_t *h_sources, const int64_t *h_counts, const void *d_block,
                    const int64_t *h_offsets, void *d_out, size_t out_bytes, size_t *h_used);
/* FINISHED STREAMS: the same last step for the job form.  The packets of the jobs of a pm_stream_scan call, made on the device from the block
 * that the call has just written -- for every job exactly the packets that pm_codec_fetch hands out for a just-created codec that is fed the
 * job's stream (pm_codec_decode), wherever the job's frame table (AX.25) or packet table (IL2P) says everything about the stream.  The rules
 * are pm_rows_packets' (pm_rows_packets.h), and so are the statuses.  Enqueued on the ctx stream behind that pm_stream_scan; h_jobs, njobs,
 * d_block and h_offsets are its arguments and results, unchanged.  A job of kind 0 must have been scanned with frames, one of kind 1 with
 * packets, and either needs d_addr, the stream's n int64 addresses on the device (pm_slice_job.d_addr): a packet's address is read there,
 * whole -- no checkpoints, no 16-bit steps, so `addrs` is not needed and an address step of any size is no obstacle.  A job with d_carry is
 * refused (the tables of a piece say nothing about the packets that began in front of it).  All of these PM_ERR_ARG, nothing enqueued.
 * h_sources[j]: what goes into source_decoder for job j, NULL: j.  d_block must be DEVICE memory, as for pm_rows_packets: the launches read it.
 * d_out (8-byte aligned, out_bytes) receives the DENSE form:
 *     pm_stream_packets_head               32 bytes: the jobs of the call, how many of them are not FINISHED, the records and their bytes
 *     pm_stream_packets_entry[njobs]       32 bytes a job: the LFSR register behind the stream, the status, the job's records, where the
 *                                          first of them begins (counted from the first record of the call), corrected_left as above
 *     the records                          job after job, in stream order within a job: the 40-byte pm_packet_head, `len` data bytes, zeros
 *                                          up to a multiple of 8
 * This is NOT pm_packets_pack's wire form, which is unpadded: here every record begins at a multiple of 8.  A frame longer than PM_PKT_MAX
 * is cut as in a pm_packet.  The statuses are PM_ROWS_PACKETS_*; LEFT_OUT does not occur.  The room for records is what out_bytes leaves
 * behind the entries: the first job whose records would pass it takes none and is NO_ROOM, and so is every job behind it; their first_byte
 * is head.bytes.  *h_used = the bytes of head and entries (PM_ERR_CAPACITY, with it set, when out_bytes is less).
 * d_out is only ever WRITTEN, in whole aligned words of 8 bytes: it may be page-locked host memory that the device reaches.  What a later
 * launch reads of an earlier one's results -- the accepted lists, the record offsets, the entries -- stays in context scratch.
 * Three launches.  Walk: a wave a job; AX.25 -- the lanes take the listed events 64 per trip, each lane makes the rule's checks for its own
 * event, a ballot and a count of the lanes in front give the places in the accepted list, a prefix sum over the wave the record offsets, both
 * carried from trip to trip; IL2P -- one lane walks the packet table by the rule, whose register makes it sequential.  Room: one wave scans
 * the jobs' bytes and writes head and entries.  Build: a fixed grid of waves, wave w the records w, w + waves, ... */
typedef struct pm_stream_packets_head {
    int32_t jobs, handed;
    int64_t packets;
    int64_t bytes;
    int64_t reserved;
} pm_stream_packets_head;
typedef struct pm_stream_packets_entry {
    uint64_t lfsr_state;
    int32_t status, packets;
    int64_t first_byte;
    int32_t corrected_left, reserved;
} pm_stream_packets_entry;
int pm_stream_packets(pm_ctx *ctx, const pm_scan_job *h_jobs, int njobs, const int32_t *h_sources, const void *d_block, const int64_t *h_offsets,
                      void *d_out, size_t out_bytes, size_t *h_used);
/* MARKS:a sliced run that says, chunk by chunk, how far every row has got -- what pm_rows_scan_pieces' d_upto is shaped for, so that the
 * rows of a run can be taken and decoded BESIDE the run instead of behind it.  A pm_lbatch_marks object (made for one engine and up to
 * max_chunks chunks; destroy it before the engine) holds for each chunk t of a run:
 *   - an int64 per row in device memory (8-byte aligned, mark t's row r at index t * rows + r, rows = recordings * chains of that run):
 *     min(count, cap) of the row's record as it stood when the row slicers of chunk t were through;
 *   - the same values in page-locked host memory;
 *   - one int32 with the OR of the rows' flags at that point (page-locked host memory; non-zero: a row has outgrown its room or its 16-bit
 *     steps and the run is to be redone the other way, as pm_rowslice_rec.flags says at the end);
 *   - one event (hipEventDisableTiming), recorded on the slicers' stream behind all of it.
 * pm_lbatch_run_sliced_marked is pm_lbatch_run_sliced with such an object: directly behind the row slicers of chunk t, on their stream, one
 * more small launch (a lane a row, plain vector stores to both copies; the flags OR-ed over the wave and by one lane a wave into the chunk's
 * word, which a memset on the same stream cleared when the run began), a four-byte copy of the word to the host, and the event.  The run's
 * own launches, streams and results are those of pm_lbatch_run_sliced, byte for byte; the engine never waits for a reader, let alone for the
 * host.  *h_chunks: the run's chunk count.  PM_ERR_CAPACITY, with nothing enqueued, for a run of more than max_chunks chunks.
 * pm_lbatch_run_sliced itself enqueues exactly what it did before marks existed.  A marks object serves one run at a time: the next marked
 * run with it overwrites the marks (its caller is through with the previous run's, as with d_data, d_steps and d_recs).
 *
 * Readers.  Every one of them refuses (PM_ERR_ARG) a t below 0 or at or beyond the chunk count of the last marked call that SUCCEEDED with
 * this object; while a marked call is being made and after one that failed that count is 0.  So no reader can wait for an event that no
 * call has recorded -- such a wait would never end.
 *   pm_lbatch_marks_ready    no waiting (hipEventQuery): *h_latest = the newest mark whose event has completed, -1 if none.
 *   pm_lbatch_marks_wait     host wait for mark t as pm_event_sync_relaxed waits (polls every poll_us microseconds); mark t's host copies
 *                            may be read afterwards.
 *   pm_lbatch_marks_wait_on  what is submitted to ctx from now on waits, on the GPU, for mark t (hipStreamWaitEvent).
 *   pm_lbatch_marks_view     mark t's pointers (any of the three may be NULL): the rows' int64 on the device and on the host, the flag word.
 *
 * Reading rows under a running engine.  A piece taken at mark t (pm_rows_scan_pieces with d_upto = mark t's device values + row0, on a
 * context that did pm_lbatch_marks_wait_on(t) first) runs while the row slicers of chunks t + 1 ... write the same rows and records.  That is
 * sound without any further synchronisation, because of what is written and what is read:
 *   - the row slicers store a data byte and its step only at index `count` and above (count itself grows behind the store), so every byte
 *     and step below a mark is final when the mark is made;
 *   - mark t's event orders those stores, and the mark's own, in front of everything on a stream that waited for it;
 *   - the piece launches read two fields of a record and no others, both in the prepare launch: count and first_addr (the launches behind
 *     it take the address in front of the piece from the prepare launch's table);
 *   - count only grows and is only ever compared against d_upto: with a mark below it the piece is the mark's, whatever count says by then;
 *   - first_addr is final once count >= 1 (later chunks store the same value again) and is used only while the carry's taken == 0, for a
 *     piece that then either has d_upto >= 1 -- the value was final at the mark -- or is empty and has no address;
 *   - last_addr never comes from the record: it is the carry's (pm_rows_carry.last_addr), which only the pieces write.
 * The bytes between the mark and the moving count are simply not looked at.  The records as a whole (end states, flags, final counts) are
 * for the end of the run, as before. */
typedef struct pm_lbatch_marks pm_lbatch_marks;
int pm_lbatch_marks_create(pm_lbatch *batch, int64_t max_chunks, pm_lbatch_marks **out);
int pm_lbatch_marks_destroy(pm_lbatch_marks *marks);
int pm_lbatch_run_sliced_marked(pm_lbatch *batch, const int16_t *const *h_d_audio, int recordings, int64_t n, const pm_slicer_params *h_params,
                                int nparams, uint8_t *d_data, uint16_t *d_steps, int64_t cap, pm_rowslice_rec *d_recs, int64_t *h_nout,
                                pm_lbatch_marks *marks, int64_t *h_chunks);
int pm_lbatch_marks_ready(pm_lbatch_marks *marks, int64_t *h_latest);
int pm_lbatch_marks_wait(pm_lbatch_marks *marks, int64_t t, int poll_us);
int pm_lbatch_marks_wait_on(pm_lbatch_marks *marks, int64_t t, pm_ctx *ctx);
int pm_lbatch_marks_view(pm_lbatch_marks *marks, int64_t t, const int64_t **d_upto, const int64_t **h_upto, const int32_t **h_flags);
pm_ctx *pm_lbatch_front_ctx(pm_lbatch *batch);       /* the engine's own contexts, for pm_prof_*: band-pass, AGC, Hilbert of chunk t + 1 ... */
pm_ctx *pm_lbatch_tail_ctx(pm_lbatch *batch);        /* ... and the matched filters of chunk t - 1, beside the loops of chunk t on the caller's */
pm_ctx *pm_lbatch_loop_ctx(pm_lbatch *batch);        /* ... or on the engine's loop context, when the loops have compute units of their own (else NULL) */
pm_ctx *pm_lbatch_slice_ctx(pm_lbatch *batch);       /* ... and the slicers of a sliced run, beside the matched filters of the next chunk */
int pm_lbatch_destroy(pm_lbatch *batch);

/* ---- host-integer stages (native C++, no GPU) --------------------------------------------------
 * These consume the slicer's byte stream; they are bit-serial state machines over KBs of data. */
/* LFSR.stream_unscramble_8bit (lfsr.py:22-52).  *h_shift_register is read and written.  h_out must not alias h_in. */
int pm_lfsr_unscramble(const uint8_t *h_in, int64_t n, uint64_t poly, int invert, uint64_t *h_shift_register, uint8_t *h_out);

/* Packet record shared by the codecs and the de-dup (PacketMeta, packet_meta.py:178-195).  IL2P packets are at most 1023 + 2 bytes
 * and AX.25 frames between flags likewise on any signal; the reference's AX.25 decoder can however close a frame of any length after
 * a long stretch without a flag (its byte counter wraps at 1023, the collected bytes stay: ax25.py:41-47).  Such a frame's row holds
 * its first PM_PKT_MAX bytes (len = PM_PKT_MAX); its CRC fields and valid_crc are those of the whole frame. */
#define PM_PKT_MAX 1280
typedef struct pm_packet {
    int64_t streamaddress;
    int32_t len;
    int32_t bytes_corrected;
    int32_t calculated_crc, carried_crc;
    int32_t valid_crc, valid_header;
    int32_t source_decoder;          /* chain index */
    int32_t correlated_count;        /* filled by pm_correlate */
    uint8_t data[PM_PKT_MAX];
} pm_packet;

/* The first 40 bytes of pm_packet: everything the de-dup reads.  Arrays of heads stand in for arrays of full rows wherever a
 * stride is passed (pm_correlate_strided), so rank 0 of a multi-GPU job never expands the payloads it gathers. */
typedef struct pm_packet_head {
    int64_t streamaddress;
    int32_t len;
    int32_t bytes_corrected;
    int32_t calculated_crc, carried_crc;
    int32_t valid_crc, valid_header;
    int32_t source_decoder;
    int32_t correlated_count;
} pm_packet_head;

typedef struct pm_codec pm_codec;
/* kind 0 = AX25Codec (ax25.py:11-93), 1 = IL2PCodec (il2p.py:110-519). */
int pm_codec_create(int kind, int crc, int disable_rs, int min_dist, int sync_tol, int source_decoder, pm_codec **out);
int pm_codec_destroy(pm_codec *c);
/* The index pm_codec_fetch writes into pm_packet.source_decoder from now on (the chain's place in the config: what the reference's
 * SourceDecoder name stands for, packet_meta.py:181). */
int pm_codec_set_source(pm_codec *c, int32_t source_decoder);
/* Feed n descrambled bytes with their stream addresses (state carries over between calls, like the reference's
 * codec objects); decoded packets queue inside the codec, *h_pending = packets waiting.  pm_codec_fetch moves up to
 * cap of them out, oldest first, with CRC and header validity filled (packet_meta.py:197-208). */
int pm_codec_decode(pm_codec *c, const uint8_t *h_data, const int64_t *h_addr, int64_t n, int64_t *h_pending);
int pm_codec_fetch(pm_codec *c, pm_packet *h_out, int64_t cap, int64_t *h_count);
/* pm_codec_decode for a codec in its just-created state (PM_ERR_ARG otherwise) with the stream's pm_stream_scan record and list at
 * h_scan (kind as the codec's; h_plain: the n descrambled bytes, inside the block or a copy).  AX.25 takes the places to start decoding
 * from the event list instead of searching for them, IL2P jumps from sync candidate to sync candidate of the bitmap instead of testing
 * every byte; packets, *h_pending and the state the decoder is left in are pm_codec_decode's. */
int pm_codec_decode_scanned(pm_codec *c, const uint8_t *h_plain, const int64_t *h_addr, int64_t n, const void *h_scan, int64_t *h_pending);
/* The same for an AX.25 codec and a block made with pm_scan_job.frames: every listed flag's frame is taken from the frame area as it is
 * (address h_addr[P >> 3], the table's CRC as the calculated one) and nothing in front of the stream's last flag goes through the decoder;
 * from there to the end it decodes byte by byte, which leaves the registers as pm_codec_decode would and finds what lies behind a bail.
 * PM_ERR_ARG for a table that cannot belong to the stream (len < 0, more bytes than the span from F to P holds, a frame past byte n). */
int pm_codec_decode_framed(pm_codec *c, const uint8_t *h_plain, const int64_t *h_addr, int64_t n, const void *h_scan, int64_t *h_pending);
/* The same for an IL2P codec (created with the job's crc, disable_rs and min_dist) and a block made with pm_scan_job.packets: the decoder
 * searches as pm_codec_decode_scanned does, and where its own sync test hits at byte k, bit offset S, and the table has a record with
 * at == k << 3 | S, the record is taken for the attempt -- HEADER_FAIL and BLOCK_FAIL pass over it, DONE queues the packet from the area (the
 * AX.25 header rebuilt from its 13 bytes; the Hamming-coded CRC from the descrambled bytes behind the last block, or the computed one; the
 * address that of the byte with the attempt's last bit) -- and the rest of the byte in which it ends goes through the decoder.  Every other
 * hit (no record, another offset, INCOMPLETE, NOT_PLACED) is decoded bit by bit as ever.  PM_ERR_ARG, with the codec untouched, for a table
 * that cannot belong to the stream: records above the places or placed above records, `at` not ascending or k outside [4, n), count > 1023,
 * a placed record outside the area, an attempt that ends behind the stream, a DONE record whose header bytes say another count. */
int pm_codec_decode_packets(pm_codec *c, const uint8_t *h_plain, const int64_t *h_addr, int64_t n, const void *h_scan, int64_t *h_pending);
/* The three above for a part made with pm_scan_job.addrs (or pm_rows_scan_chain.addrs), without the n addresses: h_steps are the stream's n
 * address steps in pm_slice_compact's form (uint16, address[i] - address[i - 1], the first one 0), addr_first the address of byte 0, and
 * h_scan the part, whose last piece is the checkpoint table.  frames, packets: how the part was made (pm_scan_job.frames / .packets; at most
 * one of them, and for the codec's kind) -- they say where the table lies and which way the codec goes: 0, 0 pm_codec_decode_scanned's,
 * frames pm_codec_decode_framed's, packets pm_codec_decode_packets'.  Wherever those read h_addr[k], this resolves A[k >> 6] plus steps
 * (k & ~63) + 1 .. k; packets, *h_pending and the codec's state are the same.  PM_ERR_ARG, with the codec untouched, for a table that
 * cannot belong to the stream: A[0] != addr_first, a place below the one in front of it, or more than 64 * 65535 above it. */
int pm_codec_decode_addrs(pm_codec *c, const uint8_t *h_plain, const uint16_t *h_steps, int64_t addr_first, int64_t n, const void *h_scan, int32_t frames,
                          int32_t packets, int64_t *h_pending);
/* The scanned routes for a part made with pm_scan_job.d_carry, for a codec in ANY state: the next piece of a stream that is scanned in
 * pieces.  frames, packets, addrs: how the part was made; the addresses come as h_addr (n of them), or, with h_addr NULL, as h_steps and
 * addr_first (with addrs they are resolved from the checkpoints as in pm_codec_decode_addrs, without addrs they are expanded).  Here
 * h_steps[0] counts: byte 0's address is addr_first + h_steps[0], and that is what A[0] must be -- 0 for a stream's first piece, not 0 for
 * a later piece of a row (pm_rows_scan_pieces), whose addr_first is its addr_before.  The part
 * ends with the carry piece, which must agree with the codec: for an AX.25 codec state START goes with a codec that has never been fed and
 * state OK with one whose `ones` and `counted` (pm_codec_scan_state) are the carry piece's -- compared only while both counts are below
 * 8000 bits; state LOST goes with any.  (An IL2P codec's attempts depend on nothing in front of the piece: only the piece number counts.)
 * The piece number must be the next one for this codec: 0 (a carry just seeded) or one more than the last piece taken.  A disagreement is
 * PM_ERR_ARG with the codec untouched.  Piece 0 is taken at any time, because a carry may be seeded at any time: a REPLAYED first piece is
 * refused only where the state gives it away (an AX.25 codec that has been fed, with a START piece; registers that have moved on from an OK
 * piece's).  An IL2P codec cannot tell a replayed piece 0 from a new seed and decodes it again: feeding each part once is the caller's.  The routes are the three above: from byte 0 to the first listed flag the AX.25 decoder runs on its
 * own registers, and a "not made" first entry of the frame table does the same; the IL2P search starts in whatever state the codec is in. */
int pm_codec_decode_carried(pm_codec *c, const uint8_t *h_plain, const int64_t *h_addr, const uint16_t *h_steps, int64_t addr_first, int64_t n,
                            const void *h_scan, int32_t frames, int32_t packets, int32_t addrs, int64_t *h_pending);
/* The AX.25 decoder's two registers that a carry is seeded from (pm_scan_carry_set): the run of ones that ends what it has been fed, capped
 * at 7, and the bits counted since the last reset (nbytes * 8 + nbits).  An IL2P codec gives 0, 0. */
int pm_codec_scan_state(pm_codec *c, int32_t *h_ones, int64_t *h_counted);
/* Addresses this codec has resolved from a checkpoint so far, and the 16-bit steps it added for them (either may be NULL): at most 63 steps
 * per look-up, and a look-up per queued packet or walked byte at the most. */
int pm_codec_addr_work(pm_codec *c, int64_t *h_lookups, int64_t *h_steps);
/* Bytes this codec has taken through its byte-by-byte machine so far, and bytes it has passed over (either may be NULL). */
int pm_codec_walked(pm_codec *c, int64_t *h_walked, int64_t *h_jumped);

/* The host half of a whole chain group in two calls (chain_execute.py:20-26 for every chain of the group at once): per job
 * pm_lfsr_unscramble into a library-owned buffer, then pm_codec_decode; per codec pm_codec_fetch into consecutive row blocks
 * of h_out (counts[j] rows each).  One chain per task on up to `threads` threads (the caller's included) that belong to the
 * library, so a language binding crosses the boundary twice per recording, not 3 x chains times.  No two jobs may share a
 * codec.  The first failing job's code is returned (its status field holds it too). */
typedef struct pm_host_job {
    pm_codec *codec;
    const uint8_t *h_data;        /* the slicer's bytes ... (may be NULL with h_scan: bytes and register come from the block) */
    const int64_t *h_addr;        /* ... and their stream addresses               */
    int64_t n;
    uint64_t lfsr_poly;
    uint64_t lfsr_state;          /* in/out: LFSR.shift_register                  */
    int64_t pending;              /* out: packets waiting in the codec            */
    int32_t lfsr_invert;
    int32_t status;               /* out */
    const uint16_t *h_addr_delta; /* with h_addr == NULL: the addresses in pm_slice_compact's form, address[i] = addr_first +  */
    int64_t addr_first;           /* delta[0] + ... + delta[i] (delta[0] = 0)                                                   */
    uint8_t *h_plain;             /* NULL, or n bytes: the LFSR's output is written here (and decoded from here) instead of a    */
                                  /* library-owned buffer -- for callers that want to see what the codec saw                    */
    const void *h_scan;           /* NULL, or the job's part of a pm_stream_scan block (record, list, bytes), made from the same */
                                  /* h_data, LFSR and codec kind: the descrambled bytes and the register come from there and the */
                                  /* codec goes through pm_codec_decode_scanned (h_plain, if given, receives a copy of the bytes) */
    int32_t scan_frames;          /* with h_scan, AX.25 codecs only: the block was made with pm_scan_job.frames -> pm_codec_decode_framed */
    int32_t scan_packets;         /* with h_scan, IL2P codecs only: the block was made with pm_scan_job.packets -> pm_codec_decode_packets */
    int32_t scan_addrs;           /* with h_scan, h_addr == NULL and h_addr_delta: the block was made with pm_scan_job.addrs -> the same route */
                                  /* through pm_codec_decode_addrs: no address is expanded, each comes from its checkpoint where it is asked for */
    int32_t scan_carry;           /* with h_scan: the block was made with pm_scan_job.d_carry -> pm_codec_decode_carried, for a codec in any state */
} pm_host_job;
int pm_host_decode_batch(pm_host_job *jobs, int njobs, int threads);
int pm_codec_fetch_batch(pm_codec *const *codecs, const int64_t *counts, int n, pm_packet *h_out, int threads);
int pm_crc16_ccitt(const uint8_t *h_data, int64_t n);                    /* crc_functions.py:44-55 */

/* Wire form of packet rows for the one exchange step of the multi-GPU path (the reference hands PacketMeta lists through a
 * multiprocessing.Queue, pymodem.py:140,157-163): per packet the 40-byte record header followed by its `len` payload bytes.
 * pm_packets_pack returns the bytes the n rows need and writes them when they fit in cap (returns the need either way);
 * pm_packets_unpack rebuilds full rows (payload tails zeroed) and returns how many it wrote, or < 0 on a malformed stream. */
int64_t pm_packets_pack(const pm_packet *h_rows, int64_t n, uint8_t *h_out, int64_t cap);
int64_t pm_packets_unpack(const uint8_t *h_in, int64_t bytes, pm_packet *h_rows, int64_t cap_rows);

/* Split a wire stream without expanding it: the record heads go to h_heads (dense), h_payload_at[k] is the offset of record
 * k's payload inside h_in.  Returns the number of records or < 0. */
int64_t pm_packets_index(const uint8_t *h_in, int64_t bytes, pm_packet_head *h_heads, int64_t *h_payload_at, int64_t cap_rows);

/* PacketMetaArray.Correlate (packet_meta.py:230-271): h_pkts hold all chains' packets in config order
 * (h_chain_counts[c] packets for chain c).  Writes indices of the unique packets, sorted by stream address,
 * to h_unique_idx and sets correlated_count on them.  Returns the number of unique packets or < 0. */
int64_t pm_correlate(pm_packet *h_pkts, const int64_t *h_chain_counts, int nchains, double address_distance,
                     int64_t *h_unique_idx, int32_t *h_corr_decoders, int64_t corr_cap);
/* Same on records `stride` bytes apart that each begin with a pm_packet_head (stride = sizeof(pm_packet) for full rows,
 * sizeof(pm_packet_head) for a dense array of heads). */
int64_t pm_correlate_strided(void *h_records, int64_t stride, const int64_t *h_chain_counts, int nchains, double address_distance,
                             int64_t *h_unique_idx, int32_t *h_corr_decoders, int64_t corr_cap);

/* ---- pipelined executor for an AFSK chain group: one call per recording -------------------------
 * What pymodem.py:140-163 does with a process per chain and a queue -- every chain of the config on the same recording, the
 * packets of all of them de-duplicated -- as a pipeline over RECORDINGS that lives entirely inside the library:
 *   pm_pipe_submit   launches the recording's demod stage on one of the demod streams -- for an AFSK group of up to two certified
 *                    sweeps ONE kernel: band-pass, every sweep and the exact chain for whatever it cannot certify, the int16 audio read
 *                    once and one bit per sample and chain written (csrc/pm_afsk.hip: afsk_fused8_kernel; other groups: band-pass + a
 *                    launch per sweep) -- records an event, returns; blocks only while all bitmap slots are in use
 *   slicer threads   (own high-priority streams) wait for the event, take up to `slice_group` consecutive recordings, work off what a
 *                    sweep left on its list (normally nothing; an overflowed list: the exact kernels), run pm_slice_batch +
 *                    pm_slice_compact, whose output the kernel writes into a page-locked host block
 *   host threads     pm_host_decode_batch + pm_codec_fetch_batch (LFSR + AX.25/IL2P per chain, fresh stage objects per recording
 *                    as chain_builder.py makes them) and pm_correlate over the chains in config order
 *   pm_pipe_wait     the recording's packet rows, per-chain counts and the de-dup result, in the library's memory until
 *                    pm_pipe_release
 * With the context's switch pipe_scan (pm_ctx_tune, PM_PIPE_SCAN; read by pm_pipe_create, default 0) the slicer threads run pm_stream_scan
 * behind pm_slice_compact, into the same block, and the host threads decode from its lists (pm_host_job.h_scan); results are the same.
 * The switch pipe_frames (PM_PIPE_FRAMES, default 0) implies pipe_scan and has the AX.25 chains' jobs write their frames too
 * (pm_scan_job.frames, pm_host_job.scan_frames); IL2P chains go the pipe_scan way.  The switch pipe_packets (PM_PIPE_PACKETS, default 0),
 * independent of pipe_frames, implies pipe_scan and has the IL2P chains' jobs make their attempts on the device (pm_scan_job.packets with the
 * chain's codec options, pm_host_job.scan_packets).  The switch pipe_addrs (PM_PIPE_ADDRS, default 0), independent of both, implies pipe_scan
 * and has every scan job write its address checkpoints (pm_scan_job.addrs from the slice job's d_addr, pm_host_job.scan_addrs): the host
 * stage expands no addresses.  A recording whose flag bytes say that a step did not fit 16 bits keeps its full addresses, and keep_slices
 * hands out full addresses as ever.
 * Results equal process_chain on every chain + PacketMetaArray.Correlate, recording by recording.  One submitting thread.  The
 * device pointers inside the descs (taps) must stay valid for the pipeline's life; host arrays are copied by pm_pipe_create. */
typedef struct pm_pipe_fir {         /* a sign-FIR group: sign(FIR(int16 audio)) as one bitmap (pm_fir_signs_i16) -- FSKModem.demod, fsk.py:149-159 */
    const double *d_taps;
    int32_t m, flags;                /* PM_FIR_NEGATE: the modem's `invert` */
} pm_pipe_fir;
typedef struct pm_pipe_chain {
    int32_t sweep, slot;             /* which sweep of pm_pipe_desc.sweeps demodulates this chain, and its place in it (gain index);
                                        sweep = -(f + 1): the chain slices the bitmap of sign-FIR group f (slot ignored) */
    pm_slicer_params slicer;         /* binary slicer */
    uint64_t lfsr_poly;              /* lfsr.py:10-20 */
    int32_t lfsr_invert;
    int32_t codec_kind, crc, disable_rs, min_dist, sync_tol;   /* pm_codec_create */
    int32_t source_decoder;          /* the chain's place in the config */
} pm_pipe_chain;
typedef struct pm_pipe_desc {
    const double *d_bpf; int32_t mb; /* the group's shared input_bpf (device) */
    int32_t nsweeps;
    double x_bound;                  /* sum|input_bpf| * 32768 */
    const pm_afsk_sweep_desc *sweeps;/* h_bits ignored: the pipeline owns the bitmaps */
    const pm_pipe_chain *chains;     /* config order */
    int32_t nchains;
    int32_t slots;                   /* recordings between demod and slicer at most (0 = 16) */
    int32_t slice_workers;           /* 0 = 2 */
    int32_t slice_group;             /* most recordings per slicer batch (0 = 4) */
    int32_t slice_min_group;         /* a batch waits for this many recordings while later ones are queued (0 = slice_group) */
    int32_t demod_streams;           /* recordings take turns on this many demod streams of the pipeline's own (each starts a recording
                                        behind the point the caller's stream had reached at its submission), each with its own
                                        band-passed stream and sweep state (0 = 2) */
    int32_t host_threads;            /* recordings in the host stage at once (0 = min(12, 36 / chains), at least 2) */
    int32_t decode_threads;          /* threads inside one recording's host stage (0 = one per chain) */
    double address_distance;         /* PacketMetaArray.Correlate (packet_meta.py:230); < 0: no de-dup here (the chains are a part of
                                        the config: the rows go to the exchange, rank 0 de-duplicates), unique = 0 */
    int64_t max_samples;             /* longest recording */
    const pm_pipe_fir *firs;         /* sign-FIR groups (may be the only demodulators: nsweeps = 0, d_bpf / sweeps unused) */
    int32_t nfirs;
    int32_t keep_slices;             /* != 0: every finished recording keeps its slicers' bytes + addresses and the LFSR output of
                                        every chain for pm_pipe_slices (parity tests of the bitstream, slicer.py:59-107) */
} pm_pipe_desc;
typedef struct pm_pipe_result {
    int64_t ticket;
    int32_t status, reserved;        /* PM_OK or the stage error (pm_pipe_wait returns it too, message in pm_last_error) */
    int64_t rows;                    /* packets of all chains */
    const pm_packet *h_rows;         /* chain by chain, config order; correlated_count set on the unique ones */
    const int64_t *h_counts;         /* [nchains] */
    int64_t unique;
    const int64_t *h_unique_idx;     /* [unique] row indices by stream address */
    const int32_t *h_corr_decoders;  /* correlated decoders, consecutive runs of correlated_count per unique packet */
    double ms_to_demod_done, ms_to_sliced, ms_to_done;   /* from submit, host clock */
    double done_at_ms;               /* when the recording left the last stage, host clock since pm_pipe_create */
} pm_pipe_result;
typedef struct pm_pipe pm_pipe;
int pm_pipe_create(pm_ctx *ctx, const pm_pipe_desc *desc, pm_pipe **out);
/* d_audio stays untouched until the recording is sliced.  A recording refused for its shape (PM_ERR_ARG) takes no ticket; one whose
 * launches fail has a ticket (*h_ticket) that is finished with that error: pm_pipe_wait returns it, pm_pipe_release frees it. */
int pm_pipe_submit(pm_pipe *pipe, const int16_t *d_audio, int64_t n, int64_t *h_ticket);
/* `count` recordings in order from one call (blocks as pm_pipe_submit does, for the whole run): tickets *h_first_ticket ..
 * + count - 1, known before the call returns to anyone who read the next ticket -- pm_pipe_wait on a promised ticket waits for its
 * submission.  For hosts whose submitting thread would otherwise queue for an interpreter lock between recordings.  One submitter. */
int pm_pipe_submit_many(pm_pipe *pipe, const int16_t *const *d_audio, const int64_t *n, int count, int64_t *h_first_ticket);
/* Announces the next `count` tickets (a pm_pipe_submit_many that another thread is about to start): pm_pipe_wait on them waits. */
int pm_pipe_promise(pm_pipe *pipe, int count, int64_t *h_first_ticket);
int pm_pipe_wait(pm_pipe *pipe, int64_t ticket, pm_pipe_result *out);
/* A finished recording's slicer output for one chain (pipelines made with keep_slices): the bytes slicer.slice would return with
 * their stream addresses (slicer.py:59-107), and what stream_unscramble_8bit made of them (lfsr.py:22-52), *h_count entries each,
 * in the library's memory until pm_pipe_release.  Any of the three pointers may be NULL. */
int pm_pipe_slices(pm_pipe *pipe, int64_t ticket, int chain, const uint8_t **h_data, const int64_t **h_addr, const uint8_t **h_plain, int64_t *h_count);
/* A finished recording's SIGN BITMAP for one chain -- bit k = (modem.demod(audio)[k] >= 0), what its slicer read (slicer.py:85) -- copied
 * to h_words (`words` 64-bit words from the bitmap's start).  Pipelines made with keep_slices only, and only while the recording's
 * bitmap slot has not been taken by a later submission (fewer than pm_pipe_slots() submissions since): PM_ERR_ARG otherwise.  Test entry:
 * the demod stage's output compared bit by bit, whatever the slicer makes of it. */
int pm_pipe_bitmap(pm_pipe *pipe, int64_t ticket, int chain, uint64_t *h_words, int64_t words);
int pm_pipe_slots(pm_pipe *pipe);                        /* recordings between demod and slicer at most, as pm_pipe_create settled it */
int pm_pipe_release(pm_pipe *pipe, int64_t ticket);      /* the result's memory */
int pm_pipe_drain(pm_pipe *pipe);                        /* every recording submitted so far is through */
int pm_pipe_stats(pm_pipe *pipe, int64_t *h_batches, int64_t *h_batch_recordings, double *h_slice_busy_ms, double *h_host_busy_ms);
/* FINISHED CHAINS: a pipeline made on a context with the switch pipe_done (PM_PIPE_DONE, default 0; implies pipe_scan, pipe_frames and
 * pipe_packets) keeps its scan parts in a device block of the slicer worker's and has pm_stream_packets finish every group of 64 scan
 * jobs into the batch's host block, behind the compact forms.  A chain whose entry is FINISHED gets no codec: its records are copied into the
 * recording's rows between those that the codecs of the other chains deliver; every other chain is decoded from the compact bytes, the
 * unscanned way.  Results are those of the pipeline without the switch, field for field.  The room of a group is the sum over its jobs of
 * what a stream of n bytes can hold at the most -- AX.25: n / 19 + 2 records of 40 + pad8(len) <= len + 48 bytes with frames that do not
 * overlap, pad8(n) + 48 (n / 19 + 2); IL2P: n / 64 + 2 records of at most 72 bytes and a payload each, payloads that do not overlap,
 * pad8(n) + 72 (n / 64 + 2) -- so NO_ROOM does not occur, unless pipe_done_room (PM_PIPE_DONE_ROOM, bytes of records per group) says less.
 * pm_pipe_done_stats: the chains since creation that were FINISHED on the device, those handed over, and the latter by status
 * (h_status_counts[12], indexed by PM_ROWS_PACKETS_*; entry 0 stays 0).  All zero for a pipeline without the switch.  Any pointer may be NULL. */
int pm_pipe_done_stats(pm_pipe *pipe, int64_t *h_finished, int64_t *h_handed, int64_t *h_status_counts);
pm_ctx *pm_pipe_side_ctx(pm_pipe *pipe, int worker);     /* a slicer worker's context (NULL past the last): for pm_prof_* */
pm_ctx *pm_pipe_demod_ctx(pm_pipe *pipe, int k);         /* demod stream k (NULL past the last); the pipeline's own, except stream 0 under pipe_queue_plan 0: the caller's context */
int pm_pipe_destroy(pm_pipe *pipe);                      /* drains first */

#ifdef __cplusplus
}
#endif
#endif /* PYMODEM_AMD_H */
