// The bitstream stage behind the slicers, on the device (pm_stream_scan): per stream of slicer bytes
//   - the LFSR's output (lfsr.py:22-52): output bit t = XOR over the set bits k of poly of input bit t - k, one lane per 64-bit word,
//   - AX.25 streams: the flags at which Ax25::feed_many (pm_codec.cpp) calls take_from_last_flag -- the first flag and every flag that
//     closes a frame of at least 18 bytes (ax25.py:36-50,69-89) -- as a list, in stream order,
//   - IL2P streams: one bit per byte, set where the sync test of il2p.py:367-376 hits at one of the byte's eight bit offsets.
// A stream is cut into tiles of at most 256 words, a workgroup a tile, a lane a word.  What a flag closes depends on the last RESET in
// front of it (a flag, or the zero that ends a run of seven ones or more) and on the stuffed zeros dropped since: the tile launch leaves a
// summary per tile, one wave per stream combines the summaries in order (what every tile starts from, the stream's record), the emit
// launch writes the list.  No workgroup waits for another inside a launch; every write is a plain store at a place that follows from
// prefix counts, so the lists come out sorted and nothing has to be cleared beforehand.
// Bits are handled in STREAM order: bit i of a word is stream bit 64 w + i (the bytes' bits from the top, as the slicer packs them).
// With pm_scan_job.frames a fourth launch writes, for every listed flag, the frame it closes -- the de-stuffed bytes the decoder would have
// collected since the flag in front, and their CRC-16 -- a wave per event, from a copy of the list that the emit launch leaves on the device.
// With pm_scan_job.packets (IL2P) the emit launch lists the candidates {k, S} in context scratch and two more launches make the ATTEMPT
// behind each (pm_il2p_core.h): the headers launch, a wave per job and a lane per candidate, decodes the 15 header bytes, counts out the
// places in the packet area and finishes what ends with the header; the blocks launch, a fixed number of waves per job, decodes the payload
// blocks of the placed ones -- syndromes, Chien search and descrambler across the lanes, Berlekamp and Forney on one -- and writes packet
// and record.  Both read the slicer bytes and the scratch, never the block.
// The kernels take their jobs from a source that is a template parameter: pm_stream_scan's table of up to 64 jobs, passed by value, or
// pm_rows_scan's row table for up to 4096 rows of a sliced engine run, which a small prepare launch makes in scratch from the rows' records
// (pm_bitscan_rows.h).  Either hands a kernel one Job; the launches, their order and what they write for a job are the same.
// With pm_scan_job.addrs / pm_rows_scan_chain.addrs the part ends with the address checkpoints (pm_bitscan_addrs.h), an int64 per 64 data
// bytes.  The job form has the slicer's full addresses on the device: the tile launch's lane of every eighth word stores its byte's.  The
// row form has 16-bit steps: the tile launch leaves each tile's sum of steps with its summary, the combine launch's wave carries an int64
// prefix from tile to tile, and a small launch of its own scans the lanes of every tile and stores (rows_addrs_kernel).
// With pm_scan_job.d_carry a job is the next PIECE of a stream (pm_scan_carry, in device memory): word 0's LFSR term and the bits in front
// of it come from the carry, the combine launch starts from the carry's counted bits instead of from a just-created decoder's state, and
// its lane 0 echoes the carry-in into the carry piece at the part's end and into scratch, then writes the carry-out.  The launches behind
// it read the scratch copy, never d_carry, so the pieces of a stream follow each other on the stream without the host in between.
// pm_rows_scan_pieces is the row form with such a carry per row (pm_rows_carry): a third source, RowPieceJobs, whose table entries say where in
// its row a piece begins and which address lies in front of it; the prepare launch cuts the pieces from the carries' `taken`, and the combine
// launch's lane 0 moves `taken` and `last_addr` on beside the carry-out.
// pm_rows_packets, behind pm_rows_scan on the same stream, READS a block in device memory: a lane a row walks the row's frame table or packet
// table by the rules of pm_rows_packets.h, one workgroup gives the accepted packets their places, and a fixed grid of waves builds the
// pm_packet rows that pm_codec_fetch would hand out; a row whose table does not say everything about it is named with the reason.
// pm_stream_packets is the same last step for the jobs of a pm_stream_scan call, into a dense form that may lie in page-locked host memory:
// a wave a job walks the table (AX.25: the lanes take the listed events 64 per trip, places from a ballot, record offsets from a prefix sum
// over the wave), one wave gives the jobs their room, and the build launch is the row form's, a template on where a part lies, where an
// address comes from and what the output looks like.
#include "pm_common.h"
#include "pm_bitscan_addrs.h"
#include "pm_bitscan_events.h"
#include "pm_bitscan_frames.h"
#include "pm_bitscan_rows.h"
#include "pm_il2p_core.h"
#include "pm_rows_packets.h"
#include <algorithm>
#include <cstring>

namespace {

using namespace pm_events;        // what decides the event list: pm_bitscan_events.h, which also compiles for the host

constexpr int kScanJobs = 64;
constexpr int kLanes = 256;                 // lanes of a workgroup = most words of a tile

// A job as the kernels see it, whichever table it comes from: pm_stream_scan's by-value ScanJobs or pm_rows_scan's row table (RowJobs)
struct Job {
    const uint8_t *data;
    uint64_t poly, reg0;
    int64_t off;                            // the job's record in the block
    int64_t ev0, pk0;
    int32_t n, tile0, tile_end;
    int kind, invert, tol;
    int pkopt;
    bool ok;                                // false: the job is left out, nothing is stored for it (rows only)
    const int64_t *addr;                    // the job form's addrs: the n stream addresses, nullptr: no checkpoints
    bool ckpt;                              // the row form's addrs: checkpoints from the row's steps
    uint64_t tail;                          // the descrambled bits in front of word 0 (a just-created decoder: zeros)
    pm_scan_carry *carry;                   // the piece's carry (pm_scan_job.d_carry), nullptr: none.  Read by the tile and combine launches only
    bool started;                           // a piece whose carry is not START: its first listed flag's frame is not made
};

struct ScanJobs {
    const uint8_t *data[kScanJobs];
    uint64_t poly[kScanJobs], reg0[kScanJobs];
    int64_t off[kScanJobs];                 // the job's record in the block
    int32_t n[kScanJobs];                   // bytes (<= 2^29)
    int32_t tile0[kScanJobs + 1];           // first tile of the job among the batch's
    int8_t kind[kScanJobs], invert[kScanJobs], tol[kScanJobs];
    int32_t njobs, tile_words;
    int32_t ev0[kScanJobs];                 // frames: the job's first place in the device-side copy of the lists (below 64 (2^29 / 19 + 2)), -1: no frames
    int32_t frame_words;
    int32_t pk0[kScanJobs];                 // packets: the job's first place in the device-side candidate list, records and work list, -1: no packets
    uint8_t pkopt[kScanJobs];               // packets: the codec's crc | disable_rs << 1 | min_dist (0 .. 9) << 2
    int8_t carried[kScanJobs];              // 1: reg0 holds pm_scan_job.d_carry instead of a register
    const int64_t *addr[kScanJobs];         // addrs: the job's stream addresses, nullptr: no checkpoints
    // The carries as the jobs found them, copied to scratch by the combine launch before it writes the carry-out: the launches behind it
    // (late = 1) take register, tail and state from there, the tile and combine launches (late = 0) from d_carry itself.
    const pm_scan_carry *carry_in;
    int32_t late;

    __device__ int tiles() const { return tile0[njobs]; }
    __device__ int job_of_tile(int tile) const
    {
        int j = 0;
        while (j + 1 < njobs && tile0[j + 1] <= tile) ++j;
        return j;
    }
    __device__ Job job(int j) const
    {
        Job jb{data[j], poly[j], reg0[j], off[j], ev0[j], pk0[j], n[j], tile0[j], tile0[j + 1], kind[j], invert[j], tol[j], pkopt[j], true,
               addr[j], false, 0, nullptr, false};
        if (carried[j]) {
            jb.carry = reinterpret_cast<pm_scan_carry *>(reg0[j]);
            const pm_scan_carry *c = late ? carry_in + j : jb.carry;
            jb.reg0 = c->lfsr_state;
            jb.tail = c->tail;
            jb.started = c->state != PM_SCAN_CARRY_START;
        }
        return jb;
    }
    __device__ void copy_steps(uint8_t *, const Job &, int, int64_t) const {}      // (the job form's block has no steps)
    __device__ void load_steps(int, int64_t, uint64_t *, uint64_t *) const {}
    static constexpr bool kPieces = false;  // (rows in pieces: RowPieceJobs)
    __device__ static uint32_t lane_sum(uint64_t lo, uint64_t hi, int64_t w, int64_t n) { return pm_addrs::lane_sum(lo, hi, w, n); }
    __device__ void piece_end(int, int64_t *, int64_t, int64_t) const {}
};
static_assert(sizeof(ScanJobs) + 64 <= 4096, "the table goes to the kernels by value, with up to eight pointers beside it");

// pm_rows_scan's source: the row table that the prepare launch leaves in scratch (pm_bitscan_rows.h), the rows' bytes where
// pm_lbatch_run_sliced left them, and the chains' parameters by value.  Row r of the call is a stream of chain (row0 + r) % nchains.
struct RowJobs {
    const pm_rows::Entry *table;            // nrows + 1 entries, the last one the totals
    const uint8_t *data;
    const uint16_t *steps;
    int64_t cap, row0;
    uint64_t poly[pm_rows::kMaxChains], reg0[pm_rows::kMaxChains];
    int8_t kind[pm_rows::kMaxChains], invert[pm_rows::kMaxChains], tol[pm_rows::kMaxChains], frames[pm_rows::kMaxChains], packets[pm_rows::kMaxChains];
    uint8_t pkopt[pm_rows::kMaxChains];
    int32_t nrows, nchains, tile_words, frame_words;
    int8_t addrs[pm_rows::kMaxChains];
    const pm_rowslice_rec *recs;            // addrs: the rows' first addresses

    __device__ int tiles() const { return table[nrows].tile0; }
    __device__ int job_of_tile(int tile) const
    {
        const pm_rows::Entry *t = table;
        return pm_rows::row_of_tile([t](int i) { return t[i].tile0; }, nrows, tile);
    }
    __device__ Job job(int j) const
    {
        const pm_rows::Entry e = table[j];
        const int c = (int)((row0 + j) % nchains);
        return Job{data + (row0 + j) * cap, poly[c], reg0[c], e.off + pm_rows::steps_bytes(e.n), e.ev0, e.pk0, e.n, e.tile0, table[j + 1].tile0,
                   kind[c], invert[c], tol[c], pkopt[c], e.off >= 0, nullptr, addrs[c] != 0, 0, nullptr, false};
    }
    // the eight steps of data word w of row j (8 w < n <= cap, and cap is a multiple of 8: they lie inside the row)
    __device__ void load_steps(int j, int64_t w, uint64_t *lo, uint64_t *hi) const
    {
        const uint64_t *src = reinterpret_cast<const uint64_t *>(steps + (row0 + j) * cap);
        *lo = src[2 * w];
        *hi = src[2 * w + 1];
    }
    // the row's address steps in front of its scan part, as pm_rows_gather writes them: the lane of data word w takes step words 2 w and 2 w + 1
    __device__ void copy_steps(uint8_t *block, const Job &jb, int j, int64_t w) const
    {
        const int64_t sw = pm_rows::steps_bytes(jb.n) >> 3;
        const uint64_t *src = reinterpret_cast<const uint64_t *>(steps + (row0 + j) * cap);      // cap is a multiple of 8: rows are aligned
        uint64_t *dst = reinterpret_cast<uint64_t *>(block + jb.off) - sw;
        for (int64_t i = 2 * w; i < 2 * w + 2 && i < sw; ++i) dst[i] = src[i];
    }
    static constexpr bool kPieces = false;
    __device__ static uint32_t lane_sum(uint64_t lo, uint64_t hi, int64_t w, int64_t n) { return pm_addrs::lane_sum(lo, hi, w, n); }
    __device__ static uint32_t lane_first(uint64_t lo, int64_t w) { return pm_addrs::lane_first(lo, w); }
    __device__ int64_t addr_before(int j) const { return recs[row0 + j].first_addr; }      // (the row's first step is not added: the first byte's own)
    __device__ void piece_end(int, int64_t *, int64_t, int64_t) const {}
};

// pm_rows_scan_pieces' source: RowJobs' fields, with a table whose entries say where in its row a piece begins (pm_rows::PieceEntry) and the
// rows' carries.  A job is the piece of row row0 + j that begins `from` bytes into the row, with &carries[row0 + j].scan for its d_carry.
struct RowPieceJobs : RowJobs {
    const pm_rows::PieceEntry *ptable;      // nrows + 1 entries, the last one the totals
    pm_rows_carry *carries;                 // indexed by row
    const pm_scan_carry *carry_in;          // the carries as the pieces found them, indexed by j (ScanJobs::carry_in) ...
    int32_t late;                           // ... for the launches behind the combine

    __device__ int tiles() const { return ptable[nrows].tile0; }
    __device__ int job_of_tile(int tile) const
    {
        const pm_rows::PieceEntry *t = ptable;
        return pm_rows::row_of_tile([t](int i) { return t[i].tile0; }, nrows, tile);
    }
    __device__ Job job(int j) const
    {
        const pm_rows::PieceEntry e = ptable[j];
        const int c = (int)((row0 + j) % nchains);
        Job jb{data + (row0 + j) * cap + e.from, poly[c], reg0[c], e.off + pm_rows::steps_bytes(e.n), e.ev0, e.pk0, e.n, e.tile0, ptable[j + 1].tile0,
               kind[c], invert[c], tol[c], pkopt[c], e.off >= 0, nullptr, addrs[c] != 0, 0, nullptr, false};
        jb.carry = &carries[row0 + j].scan;
        const pm_scan_carry *cy = late ? carry_in + j : jb.carry;
        jb.reg0 = cy->lfsr_state;
        jb.tail = cy->tail;
        jb.started = cy->state != PM_SCAN_CARRY_START;
        return jb;
    }
    // (a piece with bytes begins at a multiple of 8 and ends inside the row: 8 w < n gives from + 8 w + 8 <= cap)
    __device__ void load_steps(int j, int64_t w, uint64_t *lo, uint64_t *hi) const
    {
        const uint64_t *src = reinterpret_cast<const uint64_t *>(steps + (row0 + j) * cap + ptable[j].from);
        *lo = src[2 * w];
        *hi = src[2 * w + 1];
    }
    __device__ void copy_steps(uint8_t *block, const Job &jb, int j, int64_t w) const
    {
        const int64_t sw = pm_rows::steps_bytes(jb.n) >> 3;
        const uint64_t *src = reinterpret_cast<const uint64_t *>(steps + (row0 + j) * cap + ptable[j].from);
        uint64_t *dst = reinterpret_cast<uint64_t *>(block + jb.off) - sw;
        for (int64_t i = 2 * w; i < 2 * w + 2 && i < sw; ++i) dst[i] = src[i];
    }
    static constexpr bool kPieces = true;   // the tile launch sums every row's steps, with step 0: last_addr needs them
    __device__ static uint32_t lane_sum(uint64_t lo, uint64_t hi, int64_t w, int64_t n) { return pm_addrs::piece_lane_sum(lo, hi, w, n); }
    __device__ static uint32_t lane_first(uint64_t lo, int64_t) { return pm_addrs::piece_lane_first(lo); }
    __device__ int64_t addr_before(int j) const { return ptable[j].addr_before; }
    // the combine launch's lane 0, behind the carry-out: addr_before behind the carry piece, and where the row's next piece begins
    __device__ void piece_end(int j, int64_t *piece, int64_t n, int64_t steps_sum) const
    {
        const pm_rows::PieceEntry e = ptable[j];
        piece[4] = e.addr_before;
        pm_rows_carry *c = carries + row0 + j;
        c->taken = e.from + n;
        c->last_addr = e.addr_before + steps_sum;
    }
};
struct PkRec {                              // the headers launch's copy of a record for the blocks launch, with the 13 descrambled header bytes
    pm_il2p::Rec r;
    uint8_t hdr[16];
};
constexpr int kFrameWaves = 256;            // waves that share a job's events in the frames launch (a wave a workgroup: the others leave at once)
constexpr int kPacketWaves = 64;            // waves that share a job's placed records in the blocks launch
constexpr int kRowFrameWaves = 16;          // the same for a row of pm_rows_scan: thousands of rows of tens to hundreds of KB each
constexpr int kRowPacketWaves = 8;
constexpr uint32_t kClosesNothing = 0xFFFFFFFEu;   // F of the stream's first flag in the device-side copy when no frame ends there
constexpr uint32_t kNotMade = 0xFFFFFFFDu;         // F of a later piece's first listed flag there: what it closes began in an earlier piece

__device__ inline uint64_t load_word(const uint8_t *d, int64_t n, int64_t w)
{
    // input word w in stream order; bytes past the stream's end read as zero
    if (w < 0 || 8 * w >= n) return 0;
    uint64_t v = 0;
    if (8 * w + 8 <= n) {
        v = *reinterpret_cast<const uint64_t *>(d + 8 * w);
    } else {
        for (int i = 0; i < (int)(n - 8 * w); ++i) v |= (uint64_t)d[8 * w + i] << (8 * i);
    }
    return __brevll(__builtin_bswap64(v));
}

__device__ inline uint64_t plain_word(const Job &jb, int64_t w, uint64_t cur, uint64_t prev)
{
    // the LFSR's output word from input word w and the one before it
    uint64_t o = 0;
    for (uint64_t p = jb.poly; p; p &= p - 1) {
        const int k = __builtin_ctzll(p);
        o ^= k ? (cur << k) | (prev >> (64 - k)) : cur;
    }
    if (w == 0) o ^= jb.reg0;             // bit t of the incoming register meets stream bit t
    return jb.invert ? ~o : o;
}

// the descrambled stream's word w (zeros outside the stream), and 64 / 32 of its bits from any bit B on, the first in bit 0
__device__ inline uint64_t stream_word(const Job &jb, int64_t n, int64_t w)
{
    if (w < 0 || 8 * w >= n) return 0;
    return plain_word(jb, w, load_word(jb.data, n, w), load_word(jb.data, n, w - 1));
}
__device__ inline uint64_t stream_bits64(const Job &jb, int64_t n, int64_t B)
{
    const int64_t w = B >> 6;
    const int s = (int)(B & 63);
    const uint64_t lo = stream_word(jb, n, w);
    return s ? (lo >> s) | (stream_word(jb, n, w + 1) << (64 - s)) : lo;
}
__device__ inline unsigned stream_byte(uint64_t bits, int q) { return __brev((unsigned)(bits >> (8 * q)) & 0xFFu) >> 24; }     // byte q of them, its first bit on top

// il2p.py:367-376 at the eight bit offsets of byte b of a word: bit s set where the 32 bits that end at offset s hit.  C, P: the word and the
// one in front, most significant bit first (byte 0 on top)
__device__ inline unsigned il2p_byte_hits(uint64_t C, uint64_t P, int b, int tol)
{
    const int sh = 8 * (7 - b);
    const uint64_t win = (sh ? (C >> sh) | (P << (64 - sh)) : C) & 0xFFFFFFFFFFull;
    unsigned hits = 0;
    for (int s = 0; s < 8; ++s) {
        const uint32_t v = (uint32_t)(win >> (7 - s));
        // (__popc is unsigned: compared as such, a tol of -1 would let every byte through)
        hits |= (unsigned)((int)__popc((v & 0xFFFFFFu) ^ 0xF15E48u) <= tol || (int)__popc(v ^ 0x5D57DF7Fu) <= tol) << s;
    }
    return hits;
}

template <class T, class Op>
__device__ inline T block_scan(T v, T *lds, Op op)      // inclusive over the workgroup's lanes; lds[t] holds lane t's result afterwards
{
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int d = 1; d < kLanes; d <<= 1) {
        const bool has = t >= d;
        T o = v;
        if (has) o = lds[t - d];
        __syncthreads();
        if (has) {
            v = op(o, v);
            lds[t] = v;
        }
        __syncthreads();
    }
    return v;
}

// The lanes' segments joined by one scan: every lane's state for its word's events, and the whole tile's segment.
__device__ inline LaneIn lane_prepare(const Marks &m, bool active, Seg *lds, Seg *total)
{
    block_scan(lane_seg(m, active, (int)threadIdx.x), lds, [](const Seg &a, const Seg &b) { return seg_join(a, b); });
    const Seg before = threadIdx.x ? lds[threadIdx.x - 1] : seg_none();
    *total = lds[kLanes - 1];
    __syncthreads();
    return lane_in(m, active, (int)threadIdx.x, before);
}

// the tile launch's accumulator for pm_events::tile_summarise: the summary in LDS, the lanes' shares through LDS atomics
struct TileSumLds {
    TileSum *ts;
    __device__ void first_reset(int32_t P, int32_t dropped, bool is_flag)
    {
        ts->first_reset = P;
        ts->dropped_to_first = dropped;
        if (is_flag) atomicOr(&ts->bits, 1);
    }
    __device__ void first_flag(int32_t P, bool c)
    {
        ts->first_flag = P;
        if (c) atomicOr(&ts->bits, 2);
    }
    __device__ void closing(int count) { atomicAdd(&ts->closing, count); }
    __device__ void last_flag(int32_t P) { atomicMax(&ts->last_flag, P); }
};

__host__ __device__ inline int64_t list_bytes(int kind, int64_t n) { return PM_SCAN_LIST_BYTES(kind, n); }
// the job's checkpoint table: behind everything else of its part
__device__ inline int64_t *addr_table(uint8_t *block, const Job &jb)
{
    return reinterpret_cast<int64_t *>(block + jb.off + pm_rows::scan_bytes(jb.kind, jb.ev0 >= 0, jb.pk0 >= 0, jb.n));
}

// Launch 1: per tile the descrambled bytes, the IL2P bitmap, the tile's summary.
template <class Jobs>
__global__ __launch_bounds__(kLanes) void bitscan_tile_kernel(Jobs J, uint8_t *block, TileSum *sums)
{
    __shared__ Seg lds[kLanes];
    __shared__ TileSum ts;
    const int tile = blockIdx.x, tw = J.tile_words;
    if (tile >= J.tiles()) return;
    const int j = J.job_of_tile(tile);
    const Job jb = J.job(j);
    if (!jb.ok) return;
    const int64_t n = jb.n, nw = (n + 7) / 8;
    const int64_t w = (int64_t)(tile - jb.tile0) * tw + threadIdx.x;
    const bool active = (int)threadIdx.x < tw && w < nw;
    const int kind = jb.kind;
    const uint8_t *d = jb.data;
    uint8_t *base = block + jb.off, *list = base + PM_SCAN_HEAD, *plain = list + list_bytes(kind, n);
    uint64_t x = 0, xp = 0, valid = 0;
    uint32_t steps_sum = 0;                                 // the row form's addrs: the lane's eight steps
    if (active) {
        const uint64_t i0 = load_word(d, n, w), i1 = load_word(d, n, w - 1), i2 = load_word(d, n, w - 2);
        valid = valid_bits(n, w);
        x = plain_word(jb, w, i0, i1) & valid;
        xp = w ? plain_word(jb, w - 1, i1, i2) : jb.tail;     // (a fresh decoder: zeros in front of the stream; a later piece: the carry's tail)
        *reinterpret_cast<uint64_t *>(plain + 8 * w) = __builtin_bswap64(__brevll(x));       // the bytes are padded to 8: the last store is whole
        J.copy_steps(block, jb, j, w);
        // the job form's checkpoints: byte 8 w is byte 64 (w / 8) and 8 w < n, so the place is one of the table's (n + 63) / 64
        if (jb.addr && pm_addrs::owns_checkpoint(w)) addr_table(block, jb)[w >> 3] = jb.addr[8 * w];
        if (jb.ckpt || Jobs::kPieces) {
            uint64_t lo = 0, hi = 0;
            J.load_steps(j, w, &lo, &hi);
            steps_sum = Jobs::lane_sum(lo, hi, w, n);
        }
    }
    if (threadIdx.x == 0) {
        ts = tile_sum_empty();
        ts.bail = kNoBail;
    }
    __syncthreads();
    if (steps_sum) atomicAdd(&ts.steps, (int32_t)steps_sum);     // (at most 2048 x 65535: it fits)
    if (kind == 1) {
        // il2p.py:367-376 at the eight bit offsets of every byte k >= 4: the 32 bits in front of each against both patterns
        if (active) {
            const uint64_t C = __brevll(x), P = __brevll(xp);   // most significant bit first: byte 0 on top
            const int tol = jb.tol;
            unsigned bits = 0;
            for (int b = 0; b < 8; ++b) {
                const int64_t k = 8 * w + b;
                if (k < 4 || k >= n) continue;
                bits |= (unsigned)(il2p_byte_hits(C, P, b, tol) != 0) << b;
            }
            list[w] = (uint8_t)bits;
            if (w == nw - 1)
                for (int64_t q = nw; q < ((nw + 7) & ~int64_t(7)); ++q) list[q] = 0;
            if (bits) atomicAdd(&ts.closing, __popc(bits));
        }
    } else if (kind == 0) {
        Seg total;
        const LaneIn in = lane_prepare(ax25_marks(x, xp, valid), active, lds, &total);
        const int32_t cand = tile_bail_candidate(in);
        if (cand != kNoBail) atomicMin(&ts.bail, cand);
        __syncthreads();
        TileSumLds acc{&ts};
        tile_summarise(in, ts.bail, acc);
        if (threadIdx.x == 0) tile_totals(ts, total);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (ts.bail == kNoBail) ts.bail = -1;
        sums[tile] = ts;
    }
}

// Launch 2: a wave per stream takes the summaries in order, 64 at a time (a lane loads one, all lanes step through them together).
template <class Jobs>
__global__ __launch_bounds__(64) void bitscan_combine_kernel(Jobs J, uint8_t *block, const TileSum *sums, TileCarry *carries, int32_t *counts,
                                                             int64_t *steps_before, pm_scan_carry *carry_copy)
{
    const int j = blockIdx.x, lane = threadIdx.x, tw = J.tile_words;
    const Job jb = J.job(j);
    if (!jb.ok) return;
    const int t0 = jb.tile0, nt = jb.tile_end - t0;
    const int kind = jb.kind;
    // a piece of a stream starts from its carry: this wave reads it here and, whole, at the end, where its lane 0 writes it
    int32_t cstate = kCarryStart;
    int64_t ccounted = 0;
    if (jb.carry) {
        cstate = jb.carry->state;
        ccounted = jb.carry->counted;
    }
    Combine st = jb.carry && kind == 0 ? combine_start_carried(cstate, ccounted) : combine_start();
    PieceEnd pe = piece_end_start(ccounted);
    int32_t cands = 0;
    const bool ckpt = steps_before && jb.ckpt;              // the row form's addrs: the steps of the tiles in front of each tile, in 64 bits
    int64_t steps = 0;
    for (int r0 = 0; r0 < nt; r0 += 64) {
        TileSum s = tile_sum_empty();
        if (r0 + lane < nt) s = sums[t0 + r0 + lane];
        TileCarry mine{0, -1, -1, 0, -1};
        for (int l = 0; l < 64 && r0 + l < nt; ++l) {
            const TileSum of{__shfl(s.dropped, l), __shfl(s.first_reset, l), __shfl(s.dropped_to_first, l), __shfl(s.last_reset, l), __shfl(s.dropped_after_last, l),
                             __shfl(s.first_flag, l), __shfl(s.last_flag, l), __shfl(s.closing, l), __shfl(s.bail, l), __shfl(s.bits, l), 0, 0};
            TileCarry c = kind == 0 ? combine_step(st, of, (int64_t)(r0 + l) * tw * 64) : combine_carry(st);
            piece_end_step(pe, of, (int64_t)(r0 + l) * tw * 64);
            if (kind == 1) c.events = cands;                // an IL2P tile: the candidates in front of it
            cands += of.closing;
            if (l == lane) mine = c;
        }
        if (r0 + lane < nt) carries[t0 + r0 + lane] = mine;
        if (ckpt || Jobs::kPieces) {
            int64_t mine_steps = 0;
            for (int l = 0; l < 64 && r0 + l < nt; ++l) {
                if (l == lane) mine_steps = steps;
                steps += (int64_t)__shfl(s.steps, l);
            }
            if (ckpt && r0 + lane < nt) steps_before[t0 + r0 + lane] = mine_steps;
        }
    }
    if (lane == 0) {
        // the register as the stream leaves it (lfsr.py:30-51): what is left of the incoming one, and the taps of the last 63 input bits
        const int64_t n = jb.n, T = 8 * n;
        uint64_t reg = T < 64 ? jb.reg0 >> T : 0;
        for (int64_t t = T > 63 ? T - 63 : 0; t < T; ++t)
            if ((jb.data[t >> 3] >> (7 - (t & 7))) & 1) reg ^= jb.poly >> (T - t);
        uint8_t *rec = block + jb.off;
        *reinterpret_cast<uint64_t *>(rec) = reg;
        const Record r = combine_record(st);
        *reinterpret_cast<int64_t *>(rec + 8) = r.bail_bit;
        *reinterpret_cast<int64_t *>(rec + 16) = kind == 0 ? r.last_flag : -1;
        *reinterpret_cast<int32_t *>(rec + 24) = kind == 0 ? r.events : 0;
        *reinterpret_cast<int32_t *>(rec + 28) = kind == 1 ? cands : 0;
        if (counts) counts[j] = kind == 0 ? r.events : kind == 1 ? cands : 0;      // for the frames and packets launches: the block may be host memory, nothing is read back from it
        if (jb.carry) {
            // the carry-in into the carry piece, behind everything else of the part, and into scratch for the launches behind this one;
            // then the carry-out.  This lane is d_carry's only writer, and the tile launch has finished.
            const pm_scan_carry cin = *jb.carry;
            int64_t *piece = reinterpret_cast<int64_t *>(rec + pm_rows::scan_bytes(kind, jb.ev0 >= 0, jb.pk0 >= 0, n, jb.addr != nullptr || jb.ckpt));
            piece[0] = (int64_t)(((uint64_t)(uint32_t)cin.ones << 32) | (uint32_t)cin.state);
            piece[1] = cin.counted;
            piece[2] = cin.pieces;
            piece[3] = cin.bytes;
            carry_copy[j] = cin;
            uint64_t last = 0;
            if (n >= 8) last = stream_bits64(jb, n, 8 * n - 64);
            else if (n > 0) last = stream_word(jb, n, 0) & valid_bits(n, 0);
            pm_scan_carry out = cin;
            out.lfsr_state = reg;
            out.tail = tail_join(cin.tail, last, n);
            out.ones = tail_ones(out.tail);
            if (kind == 0) out.counted = piece_counted(pe, n, out.ones);
            out.state = piece_state(cin.state, st);
            out.pieces = cin.pieces + 1;
            out.bytes = cin.bytes + n;
            *jb.carry = out;
            J.piece_end(j, piece, n, steps);
        }
    }
}

// Launch 3: the events of every AX.25 tile, at the places the combine counted out; packets: the candidates {k, S} of every IL2P tile likewise,
// into the device-side list.
template <class Jobs>
__global__ __launch_bounds__(kLanes) void bitscan_emit_kernel(Jobs J, uint8_t *block, const TileCarry *carries, uint2 *copies, uint32_t *cands)
{
    __shared__ Seg lds[kLanes];
    __shared__ int32_t cnt[kLanes];
    const int tile = blockIdx.x, tw = J.tile_words;
    if (tile >= J.tiles()) return;
    const Job jb = J.job(J.job_of_tile(tile));
    if (!jb.ok) return;
    if (jb.kind == 1 && jb.pk0 >= 0) {
        const int64_t n = jb.n, nw = (n + 7) / 8, w = (int64_t)(tile - jb.tile0) * tw + threadIdx.x, places = n / 64 + 2;
        unsigned bits = 0, offs = 0;                        // the word's candidate bytes, and the smallest offset that hits in each (3 bits a byte)
        if ((int)threadIdx.x < tw && w < nw) {
            const uint8_t *d = jb.data;
            const uint64_t i0 = load_word(d, n, w), i1 = load_word(d, n, w - 1), i2 = load_word(d, n, w - 2);
            const uint64_t C = __brevll(plain_word(jb, w, i0, i1) & valid_bits(n, w)), P = __brevll(w ? plain_word(jb, w - 1, i1, i2) : jb.tail);
            for (int b = 0; b < 8; ++b) {
                const int64_t k = 8 * w + b;
                if (k < 4 || k >= n) continue;
                const unsigned hits = il2p_byte_hits(C, P, b, jb.tol);
                if (hits) {
                    bits |= 1u << b;
                    offs |= (unsigned)__builtin_ctz(hits) << (3 * b);
                }
            }
        }
        block_scan((int32_t)__popc(bits), cnt, [](int32_t a, int32_t b) { return a + b; });
        int64_t at = (int64_t)carries[tile].events + (threadIdx.x ? cnt[threadIdx.x - 1] : 0);
        for (unsigned m = bits; m; m &= m - 1, ++at) {
            const int b = __builtin_ctz(m);
            if (at < places) cands[jb.pk0 + at] = (uint32_t)((8 * w + b) << 3) | ((offs >> (3 * b)) & 7u);
        }
        return;
    }
    if (jb.kind != 0) return;
    const TileCarry c = carries[tile];
    if (c.events < 0) return;
    const int64_t n = jb.n, nw = (n + 7) / 8;
    const int64_t tbase = (int64_t)(tile - jb.tile0) * tw, w = tbase + threadIdx.x, B = tbase * 64;
    const bool active = (int)threadIdx.x < tw && w < nw;
    uint64_t x = 0, xp = 0, valid = 0;
    if (active) {
        const uint8_t *d = jb.data;
        const uint64_t i0 = load_word(d, n, w), i1 = load_word(d, n, w - 1), i2 = load_word(d, n, w - 2);
        valid = valid_bits(n, w);
        x = plain_word(jb, w, i0, i1) & valid;
        xp = w ? plain_word(jb, w - 1, i1, i2) : jb.tail;
    }
    Seg total;
    const LaneIn in = lane_prepare(ax25_marks(x, xp, valid), active, lds, &total);
    // two places: a word holds one closing flag at most, and the stream's first flag beside it (pm_events::Listed; held by
    // tests/test_bitscan_core.py, where no lane of any stream at any tile size wants a third)
    const Listed l = emit_lane(in, c, B);
    const int nfound = listed_count(l);
    block_scan((int32_t)nfound, cnt, [](int32_t a, int32_t b) { return a + b; });
    const int64_t at = (int64_t)c.events + (threadIdx.x ? cnt[threadIdx.x - 1] : 0), cap = n / 19 + 2;
    uint2 *events = reinterpret_cast<uint2 *>(block + jb.off + PM_SCAN_HEAD);
    for (int k = 0; k < nfound; ++k)
        if (at + k < cap) events[at + k] = make_uint2(listed_P(l, k), listed_F(l, k));
    if (jb.ev0 >= 0)
        for (int k = 0; k < nfound; ++k)
            if (at + k < cap)
                copies[jb.ev0 + at + k] = make_uint2(listed_P(l, k), jb.started && listed_F(l, k) == 0xFFFFFFFFu ? kNotMade : (l.nothing >> k) & 1 ? kClosesNothing : listed_F(l, k));
}

// The CRC-16 of pm_bitscan_frames.h across a wave, for the frames launch and for pm_rows_packets' build launch: the 256 one-byte steps into
// LDS (crc_functions.py:44-55, eight bits at a time), and the register behind `len` >= 2 bytes that follow the register `crc`: 64 pieces
// that end at the last byte, a lane a piece, joined by a scan with powers of x.
__device__ inline void wave_crc_table(uint16_t *crc_table, int lane)
{
    for (int v = lane; v < 256; v += 64) {
        unsigned c = (unsigned)v;
        for (int i = 0; i < 8; ++i) c = (c & 1) ? (c >> 1) ^ 0x8408u : c >> 1;
        crc_table[v] = (uint16_t)c;
    }
}
template <class Byte>
__device__ inline uint32_t wave_crc(const uint16_t *crc_table, int lane, int len, uint32_t crc, Byte byte)
{
    using namespace pm_frames;
    const int per = (len + 63) >> 6;
    uint32_t piece = crc_piece(crc_table, lane, len, per, crc, byte), f = crc_times_x(0x8000u, 8 * per);
    for (int dl = 1; dl < 64; dl <<= 1) {
        const uint32_t o = __shfl_up(piece, dl);
        if (lane >= dl) piece ^= crc_mul(f, o);
        f = crc_mul(f, f);
    }
    return __shfl(piece, 63);
}

// Launch 4 (pm_scan_job.frames): a wave per listed flag {P, F} -- the events e, e + waves, ... of its job, the count read from the combine
// launch's device-side copy -- writes the frame that ends there.  The span from F (or the stream's start) to P is taken `frame_words`
// words per trip, a lane a word: the lane's word as the counters see it (pm_bitscan_frames.h), a scan over the lanes for the counters in
// front of each word, the word's appended bits squeezed together and ORed into a line in LDS at the place their byte has in the frame, the
// line's whole bytes out to the frame area, the CRC continued over them, a lane a piece.  The line is laid out so that its 8-byte words are
// the area's: whole words go out as one store, the bytes at a frame's two ends one by one (the neighbouring frames' bytes share those
// words).  Up to seven bits of a byte that the trip leaves unfinished stay in the line for the next trip.
template <class Jobs>
__global__ __launch_bounds__(64) void bitscan_frames_kernel(Jobs J, uint8_t *block, const uint2 *copies, const int32_t *counts)
{
    using namespace pm_frames;
    constexpr int kLineWords = 136;                         // 7 bytes of alignment, 7 bits left over, 64 words of 64 bits, and the OR's reach
    __shared__ uint32_t line[kLineWords];
    __shared__ uint16_t crc_table[256];
    const int j = blockIdx.y, lane = threadIdx.x;
    const Job jb = J.job(j);
    if (!jb.ok || jb.ev0 < 0) return;
    const int64_t n = jb.n, cap = n / 19 + 2;
    const int32_t count = (int32_t)(counts[j] < cap ? counts[j] : cap);
    if ((int)blockIdx.x >= count) return;
    wave_crc_table(crc_table, lane);
    const uint8_t *d = jb.data;
    uint8_t *table = block + jb.off + PM_SCAN_HEAD + list_bytes(0, n) + ((n + 7) & ~int64_t(7)), *area = table + PM_SCAN_FRAME_TABLE_BYTES(n);
    const int fw = J.frame_words;
    auto or_word = [&](int at, uint32_t v) { atomicOr(&line[at], v); };
    for (int32_t e = (int32_t)blockIdx.x; e < count; e += (int32_t)gridDim.x) {
        const uint2 pf = copies[jb.ev0 + e];
        if (pf.y == kNotMade) {                             // the frame began in an earlier piece: the host's registers have it
            if (lane == 0) *reinterpret_cast<uint2 *>(table + 8 * (int64_t)e) = make_uint2(0xFFFFFFFFu, 0u);
            continue;
        }
        const int64_t P = pf.x, s = pf.y >= kClosesNothing ? 0 : (int64_t)pf.y;
        if (pf.y == kClosesNothing || P >= 8 * n || s >= P) {
            if (lane == 0) *reinterpret_cast<uint2 *>(table + 8 * (int64_t)e) = make_uint2(0u, 0u);
            continue;
        }
        const int64_t w_first = s >> 6, w_last = (P - 1) >> 6, at0 = s >> 3;        // at0: the frame's first byte in the area
        State carry{0, 0};                                  // the counters in front of the trip
        int64_t out = 0;                                    // bytes of the frame that have gone out: carry.bytes + carry.open / 8
        uint32_t left = 0;                                  // the carry.open % 8 bits of the unfinished byte
        uint32_t crc = 0xFFFF, held0 = 0, held1 = 0;        // the CRC's register for the frame less its last two bytes, which are held back
        for (int64_t wt = w_first; wt <= w_last; wt += fw) {
            const int64_t w = wt + lane;
            const bool active = lane < fw && w <= w_last;
            uint64_t x = 0;
            WordMarks k{0, 0};
            if (active) {
                const uint64_t i0 = load_word(d, n, w), i1 = load_word(d, n, w - 1), i2 = load_word(d, n, w - 2);
                x = plain_word(jb, w, i0, i1);
                const uint64_t xp = w ? plain_word(jb, w - 1, i1, i2) : jb.tail;
                const uint64_t span = low_mask(w == w_last ? (int)((P - 1) & 63) + 1 : 64) & ~low_mask(w == w_first ? (int)(s & 63) : 0);
                k = word_marks(x, xp, span);
            }
            const Span mine = active ? word_span(k) : Span{0, 0, 0, 0};
            Span upto = mine;                               // inclusive over the lanes
            for (int dl = 1; dl < 64; dl <<= 1) {
                Span o{__shfl_up(upto.r, dl), __shfl_up(upto.a, dl), __shfl_up(upto.m, dl), __shfl_up(upto.t, dl)};
                if (lane >= dl) upto = join(o, upto);
            }
            Span before{__shfl_up(upto.r, 1), __shfl_up(upto.a, 1), __shfl_up(upto.m, 1), __shfl_up(upto.t, 1)};
            if (lane == 0) before = Span{0, 0, 0, 0};
            const Span all{__shfl(upto.r, 63), __shfl(upto.a, 63), __shfl(upto.m, 63), __shfl(upto.t, 63)};
            const State st = advance(carry, before), next = advance(carry, all);
            // what the segment open behind a word has when it closes: the lane of the next reset knows
            const uint64_t resets = __ballot(mine.r != 0);
            const int32_t closes_at = st.open + mine.a;
            const uint64_t behind = lane < 63 ? resets & ~low_mask(lane + 1) : 0;
            const int32_t from_next = __shfl(closes_at, behind ? __builtin_ctzll(behind) : lane);
            const int32_t later = behind ? from_next : kOpenEnded;
            const int32_t head = __shfl(closes_at, resets ? __builtin_ctzll(resets) : 0);
            const int sh = (int)((at0 + out) & 7);          // the line's byte sh is the frame's byte `out`
            __syncthreads();
            for (int v = lane; v < kLineWords; v += 64) line[v] = 0;
            __syncthreads();
            // the unfinished byte is the frame's if its segment gets that far; otherwise the next segment's first byte takes its place
            if (lane == 0 && left && !(resets && (head >> 3) == (carry.open >> 3))) line[sh >> 2] = left << (8 * (sh & 3));
            __syncthreads();
            if (active) put_word(x, k, st, 8 * ((int64_t)sh - out), later, or_word);
            __syncthreads();
            const int64_t total = next.bytes + (next.open >> 3);
            const int nb = (int)(total - out);              // whole bytes of this trip: the line's bytes sh .. sh + nb
            // the CRC runs two bytes behind the frame: over this trip's bytes but the last two, behind the two held back from the trip before
            {
                const int64_t lo = out > 2 ? out - 2 : 0, hi = total > 2 ? total - 2 : 0;
                const int len = (int)(hi - lo), old = (int)(out - lo);            // old: how many of them are held-back bytes
                auto byte = [&](int k) -> uint32_t {
                    if (k < old) return k + 2 - old ? held1 : held0;
                    const int q = sh + (k - old);
                    return (line[q >> 2] >> (8 * (q & 3))) & 0xFF;
                };
                if (len == 1) {
                    crc = (crc >> 8) ^ crc_table[(crc ^ byte(0)) & 0xFF];
                } else if (len >= 2) {
                    crc = wave_crc(crc_table, lane, len, crc, byte);
                }
                if (nb >= 2) {
                    held0 = (line[(sh + nb - 2) >> 2] >> (8 * ((sh + nb - 2) & 3))) & 0xFF;
                    held1 = (line[(sh + nb - 1) >> 2] >> (8 * ((sh + nb - 1) & 3))) & 0xFF;
                } else if (nb == 1) {
                    held0 = held1;
                    held1 = (line[sh >> 2] >> (8 * (sh & 3))) & 0xFF;
                }
            }
            uint8_t *dst = area + at0 + out - sh;           // 8-byte aligned: the line's byte 0
            for (int q0 = 8 * lane; q0 < sh + nb; q0 += 512) {
                const uint64_t v = line[q0 >> 2] | (uint64_t)line[(q0 >> 2) + 1] << 32;
                if (q0 >= sh && q0 + 8 <= sh + nb) {
                    *reinterpret_cast<uint64_t *>(dst + q0) = v;
                } else {
                    for (int q = q0 > sh ? q0 : sh; q < q0 + 8 && q < sh + nb; ++q) dst[q] = (uint8_t)(v >> (8 * (q - q0)));
                }
            }
            const int qe = sh + nb;
            left = (line[qe >> 2] >> (8 * (qe & 3))) & 0xFF & (uint32_t)low_mask(next.open & 7);
            out = total;
            carry = next;
        }
        // the flag closes a frame when the last segment holds 18 bytes or more and the flag's own seven bits (ax25.py:74-81)
        const bool closing = (carry.open & 7) == 7 && carry.open >= kCloseBits;
        if (lane == 0) *reinterpret_cast<uint2 *>(table + 8 * (int64_t)e) = closing ? make_uint2((uint32_t)out, (crc ^ 0xFFFF) & 0xFFFF) : make_uint2(0u, 0u);
    }
}

// Launch 5 (pm_scan_job.packets): a wave per job takes its candidates 64 at a time, a lane a candidate: the 15 header bytes from bit H, RS(2),
// the descrambler, the count, where the attempt would end (pm_il2p::header_attempt).  A scan over the lanes, carried from trip to trip, gives
// every passed and complete header its place in the area in candidate order; from the first that does not fit on, none is placed.  What ends
// here -- INCOMPLETE, HEADER_FAIL, NOT_PLACED, DONE without payload -- goes to the table at once; every record is copied to scratch, and the
// placed ones with payload are listed there for the blocks launch.
template <class Jobs>
__global__ __launch_bounds__(64) void bitscan_headers_kernel(Jobs J, uint8_t *block, const int32_t *counts, const uint32_t *cands, PkRec *recs, int32_t *work,
                                                             int32_t *pkcounts)
{
    using namespace pm_il2p;
    using pm_frames::low_mask;
    __shared__ GF256 g;
    const int j = blockIdx.x, lane = threadIdx.x;
    const Job jb = J.job(j);
    if (!jb.ok || jb.pk0 < 0) return;
    if (lane == 0) gf_build(&g);
    __syncthreads();
    const int64_t n = jb.n, places = n / 64 + 2, area_bytes = PM_SCAN_PACKET_AREA_BYTES(n);
    const int32_t records = (int32_t)(counts[j] < places ? counts[j] : places), base = jb.pk0;
    uint8_t *table = block + jb.off + PM_SCAN_HEAD + list_bytes(1, n) + ((n + 7) & ~int64_t(7)), *area = table + PM_SCAN_PACKET_TABLE_BYTES(n);
    const Opts o{jb.pkopt & 1, (jb.pkopt >> 1) & 1, jb.pkopt >> 2};
    int64_t used = 0;                                       // bytes of the area counted out so far
    int32_t nwork = 0, nplaced = 0;
    bool full = false;
    for (int32_t r0 = 0; r0 < records; r0 += 64) {
        const int32_t e = r0 + lane;
        const bool active = e < records;
        PkRec pr;
        for (int q = 0; q < 16; ++q) pr.hdr[q] = 0;
        pr.r = rec_incomplete(0);
        uint32_t need = 0;
        if (active) {
            const uint32_t at = cands[base + e];
            const int64_t H = rec_H(at);
            pr.r = rec_incomplete(at);
            if (H + kHeaderBits <= 8 * n) {
                const uint64_t b0 = stream_bits64(jb, n, H), b1 = stream_bits64(jb, n, H + 64);
                for (int q = 0; q < 8; ++q) pr.hdr[q] = (uint8_t)stream_byte(b0, q);
                for (int q = 0; q < 7; ++q) pr.hdr[8 + q] = (uint8_t)stream_byte(b1, q);
                pr.r = header_attempt(&g, at, pr.hdr, o, 8 * n);
                if (pr.r.status == kDone) need = rec_need(pr.r.count);
            }
        }
        uint32_t upto = need;                               // inclusive over the lanes
        for (int dl = 1; dl < 64; dl <<= 1) {
            const uint32_t v = __shfl_up(upto, dl);
            if (lane >= dl) upto += v;
        }
        const int64_t off = used + upto - need;
        const uint64_t over = __ballot(need && off + need > area_bytes);
        const bool placed = need && !full && !(over && lane >= __builtin_ctzll(over));
        const uint64_t with_blocks = __ballot(placed && pr.r.count > 0);
        if (placed) pr.r.off = (uint32_t)off;
        else if (need) pr.r = rec_not_placed(pr.r);
        if (active) {
            if (placed && pr.r.count > 0) work[base + nwork + __popcll(with_blocks & low_mask(lane))] = e;
            recs[base + e] = pr;
            if (!(placed && pr.r.count > 0)) {
                uint2 *place = reinterpret_cast<uint2 *>(table + 16 + 16 * (int64_t)e);
                place[0] = make_uint2(pr.r.at, pr.r.off);
                place[1] = make_uint2((uint32_t)pr.r.count | (uint32_t)pr.r.status << 16 | (uint32_t)pr.r.corrected << 24, pr.r.end);
                if (placed) {                               // a packet of its header alone: 13 bytes and three zeros
                    uint64_t v0 = 0, v1 = 0;
                    for (int q = 0; q < 8; ++q) v0 |= (uint64_t)pr.hdr[q] << (8 * q);
                    for (int q = 0; q < 5; ++q) v1 |= (uint64_t)pr.hdr[8 + q] << (8 * q);
                    uint64_t *dst = reinterpret_cast<uint64_t *>(area + off);
                    dst[0] = v0;
                    dst[1] = v1;
                }
            }
        }
        used += __shfl(upto, 63);
        nwork += __popcll(with_blocks);
        nplaced += __popcll(__ballot(placed));
        full = full || over != 0;
    }
    if (lane == 0) {
        uint2 *head = reinterpret_cast<uint2 *>(table);
        head[0] = make_uint2((uint32_t)records, (uint32_t)nplaced);
        head[1] = make_uint2(0u, 0u);
        pkcounts[2 * j] = records;
        pkcounts[2 * j + 1] = nwork;
    }
}

// Launch 6 (pm_scan_job.packets): wave x of a job takes the work list's records x, x + waves, ...: the placed records with payload.  Per block:
// the lanes load the block's bytes at its bit offset, four a lane, into LDS; each lane's share of the 16 syndromes (pm_il2p::syn_segment),
// XORed over the wave; if any is set, Berlekamp on lane 0, the Chien search a position per lane, Forney on lane 0, and the syndromes again;
// the descrambler a byte per lane into the packet, which is put together in LDS behind its 13 header bytes and goes out in whole words once
// every block has passed.  The wave writes the record whole at the end.
template <class Jobs>
__global__ __launch_bounds__(64) void bitscan_blocks_kernel(Jobs J, uint8_t *block, const PkRec *recs, const int32_t *work, const int32_t *pkcounts)
{
    using namespace pm_il2p;
    using pm_frames::low_mask;
    __shared__ GF256 g;
    __shared__ uint32_t buf32[64], pkt32[264];              // a block of up to 255 bytes; the packet: 13 + 1023 bytes, padded to 8
    __shared__ int syn[16], loc[17], where[17];
    const int j = blockIdx.y, lane = threadIdx.x;
    const Job jb = J.job(j);
    if (!jb.ok || jb.pk0 < 0) return;
    if (lane == 0) gf_build(&g);
    __syncthreads();
    const int64_t n = jb.n;
    const int32_t nwork = pkcounts[2 * j + 1], base = jb.pk0;
    uint8_t *table = block + jb.off + PM_SCAN_HEAD + list_bytes(1, n) + ((n + 7) & ~int64_t(7)), *area = table + PM_SCAN_PACKET_TABLE_BYTES(n);
    const bool disable_rs = (jb.pkopt >> 1) & 1;
    const int min_dist = jb.pkopt >> 2;
    uint8_t *buf = reinterpret_cast<uint8_t *>(buf32), *pkt = reinterpret_cast<uint8_t *>(pkt32);
    // the wave's syndromes of the nb bytes in buf, four to a word, the same in every lane
    auto syndromes = [&](int nb, uint32_t *s4) {
        int cnt = nb - 4 * lane;
        cnt = cnt < 0 ? 0 : cnt > 4 ? 4 : cnt;
        const uint32_t mine = buf32[lane];
        const uint8_t seg[4] = {(uint8_t)mine, (uint8_t)(mine >> 8), (uint8_t)(mine >> 16), (uint8_t)(mine >> 24)};
        const int tail = nb - 4 * lane - cnt;
        for (int q = 0; q < 4; ++q) {
            uint32_t v = 0;
            if (cnt)
                for (int i = 0; i < 4; ++i) v |= syn_segment(&g, 4 * q + i, seg, cnt, tail) << (8 * i);
            for (int dl = 32; dl; dl >>= 1) v ^= __shfl_xor(v, dl);
            s4[q] = v;
        }
    };
    for (int32_t wi = (int32_t)blockIdx.x; wi < nwork; wi += (int32_t)gridDim.x) {
        const int32_t e = work[base + wi];
        const PkRec pr = recs[base + e];
        const int count = pr.r.count;
        const Split split = block_split(count);
        const int need = (int)rec_need(count);
        __syncthreads();
        for (int v = lane; v < need / 4; v += 64) pkt32[v] = 0;
        __syncthreads();
        if (lane < 13) pkt[lane] = pr.hdr[lane];
        int corrected = pr.r.corrected, appended = 0;
        uint32_t end = (uint32_t)kHeaderBits;
        bool fail = false;
        for (int b = 0; b < split.blocks && !fail; ++b) {
            const int bs = block_bytes(split, b), nb = bs + 16;
            __syncthreads();
            {
                const uint32_t v = 4 * lane < nb ? (uint32_t)stream_bits64(jb, n, rec_H(pr.r.at) + end + 32 * lane) : 0u;
                buf32[lane] = stream_byte(v, 0) | stream_byte(v, 1) << 8 | stream_byte(v, 2) << 16 | stream_byte(v, 3) << 24;
            }
            __syncthreads();
            int fixed = 0;
            uint32_t s4[4] = {0, 0, 0, 0};
            if (!disable_rs) syndromes(nb, s4);
            if (!disable_rs && (s4[0] | s4[1] | s4[2] | s4[3])) {
                if (lane == 0) {
                    for (int i = 0; i < 16; ++i) syn[i] = (int)((s4[i >> 2] >> (8 * (i & 3))) & 0xFF);
                    rs_berlekamp(&g, 16, syn, loc);
                }
                __syncthreads();
                for (int t = 0; t < 4; ++t) {               // a position per lane, in ascending order
                    const int pos = 64 * t + lane;
                    const bool root = pos < nb && rs_chien_at(&g, 16, loc, nb, pos) == 0;
                    const uint64_t m = __ballot(root);
                    const int idx = fixed + __popcll(m & low_mask(lane));
                    if (root && idx < 17) where[idx] = pos;
                    fixed += __popcll(m);
                }
                __syncthreads();
                if (lane == 0 && fixed <= 8 - min_dist) rs_forney(&g, 16, syn, loc, where, fixed, nb, buf);
                __syncthreads();
                syndromes(nb, s4);
                fail = (s4[0] | s4[1] | s4[2] | s4[3]) != 0;
            }
            end += 8u * (uint32_t)nb;
            if (fail) break;
            corrected += fixed;
            for (int k = lane; k < bs; k += 64) pkt[13 + appended + k] = (uint8_t)descramble_at(buf[k], k >= 1 ? buf[k - 1] : 0u, k >= 2 ? buf[k - 2] : 0u, k);
            appended += bs;
        }
        __syncthreads();
        if (!fail) {
            uint64_t *dst = reinterpret_cast<uint64_t *>(area + pr.r.off);
            for (int v = lane; v < need / 8; v += 64) dst[v] = pkt32[2 * v] | (uint64_t)pkt32[2 * v + 1] << 32;
        }
        if (lane == 0) {
            uint2 *place = reinterpret_cast<uint2 *>(table + 16 + 16 * (int64_t)e);
            place[0] = make_uint2(pr.r.at, pr.r.off);
            place[1] = make_uint2((uint32_t)count | (uint32_t)(fail ? kBlockFail : kDone) << 16 | (uint32_t)corrected << 24, end);
        }
    }
}

// The checkpoint launch of pm_rows_scan (pm_rows_scan_chain.addrs), behind the combine: a workgroup a tile, a lane a data word, as in the tile
// launch.  The lanes load their eight steps again, one scan over the lanes gives each the steps of the tile's lanes in front, and the lane of
// every eighth word stores A[w / 8] = the row's first address + the combine's prefix for the tile + that + the step to its own first byte
// (pm_bitscan_addrs.h).  Every tile of every kind, behind a bail too; the emit launch covers neither.
template <class Jobs>
__global__ __launch_bounds__(kLanes) void rows_addrs_kernel(Jobs J, uint8_t *block, const int64_t *steps_before)
{
    __shared__ uint32_t lds[kLanes];
    const int tile = blockIdx.x, tw = J.tile_words;
    if (tile >= J.tiles()) return;
    const int j = J.job_of_tile(tile);
    const Job jb = J.job(j);
    if (!jb.ok || !jb.ckpt) return;
    const int64_t n = jb.n, nw = (n + 7) / 8;
    const int64_t w = (int64_t)(tile - jb.tile0) * tw + threadIdx.x;
    const bool active = (int)threadIdx.x < tw && w < nw;
    uint64_t lo = 0, hi = 0;
    if (active) J.load_steps(j, w, &lo, &hi);
    block_scan(active ? Jobs::lane_sum(lo, hi, w, n) : 0u, lds, [](uint32_t a, uint32_t b) { return a + b; });
    const uint32_t before = threadIdx.x ? lds[threadIdx.x - 1] : 0u;
    // (8 w < n: the place is one of the table's (n + 63) / 64)
    if (active && pm_addrs::owns_checkpoint(w))
        addr_table(block, jb)[w >> 3] = pm_addrs::checkpoint(J.addr_before(j), steps_before[tile], before, Jobs::lane_first(lo, w));
}

// The prepare launch of pm_rows_scan: the row table from the records' counts and the chains' kinds (pm_bitscan_rows.h) -- one workgroup,
// trips of 256 rows, a lane a row: an inclusive scan of the rows' four sums over the lanes, the carry from trip to trip.
__global__ __launch_bounds__(kLanes) void rows_prepare_kernel(RowJobs J, const pm_rowslice_rec *recs, pm_rows::Entry *table, pm_rows::Sums limit)
{
    using namespace pm_rows;
    static_assert(kTrip == kLanes, "a lane a row");
    __shared__ Sums lds[kLanes];
    Sums carry = sums_zero();
    for (int r0 = 0; r0 < J.nrows; r0 += kTrip) {
        const int r = r0 + (int)threadIdx.x, c = (int)((J.row0 + r) % J.nchains);
        const bool active = r < J.nrows;
        const int64_t n = active ? row_bytes(recs[J.row0 + r].count, J.cap) : 0;
        const Sums mine = active ? row_sums(J.kind[c], J.frames[c], J.packets[c], n < kMaxBytes ? n : kMaxBytes, J.tile_words, J.addrs[c]) : sums_zero();
        const Sums upto = block_scan(mine, lds, [](const Sums &a, const Sums &b) { return sums_add(a, b); });
        const Sums before = sums_add(carry, threadIdx.x ? lds[threadIdx.x - 1] : sums_zero());
        carry = sums_add(carry, lds[kLanes - 1]);
        (void)upto;
        if (active) table[r] = row_entry(before, J.kind[c], J.frames[c], J.packets[c], n, J.tile_words, limit, J.addrs[c]);
        __syncthreads();
    }
    if (threadIdx.x == 0) table[J.nrows] = total_entry(carry, limit);
}

// The prepare launch of pm_rows_scan_pieces: the same trips, with each row's piece cut from its record's count, the caller's `upto` and its
// carry's `taken` (pm_rows::piece_bytes), and the address in front of the piece from the record or the carry.
__global__ __launch_bounds__(kLanes) void rows_pieces_prepare_kernel(RowPieceJobs J, const pm_rowslice_rec *recs, const int64_t *upto, int32_t final_piece,
                                                                     pm_rows::PieceEntry *table, pm_rows::Sums limit)
{
    using namespace pm_rows;
    __shared__ Sums lds[kLanes];
    Sums carry = sums_zero();
    for (int r0 = 0; r0 < J.nrows; r0 += kTrip) {
        const int r = r0 + (int)threadIdx.x, c = (int)((J.row0 + r) % J.nchains);
        const bool active = r < J.nrows;
        int64_t n = 0, from = 0, addr_before = 0;
        if (active) {
            const pm_rowslice_rec *q = recs + J.row0 + r;
            const pm_rows_carry *cy = J.carries + J.row0 + r;
            from = cy->taken;
            n = piece_bytes(piece_avail(q->count, J.cap, upto != nullptr, upto ? upto[r] : 0), from, final_piece != 0);
            addr_before = from ? cy->last_addr : q->first_addr;
        }
        const Sums mine = active ? piece_sums(J.kind[c], J.frames[c], J.packets[c], n < kMaxBytes ? n : kMaxBytes, J.tile_words, J.addrs[c]) : sums_zero();
        block_scan(mine, lds, [](const Sums &a, const Sums &b) { return sums_add(a, b); });
        const Sums before = sums_add(carry, threadIdx.x ? lds[threadIdx.x - 1] : sums_zero());
        carry = sums_add(carry, lds[kLanes - 1]);
        if (active) table[r] = piece_entry(before, J.kind[c], J.frames[c], J.packets[c], n, J.tile_words, limit, J.addrs[c], from, addr_before);
        __syncthreads();
    }
    if (threadIdx.x == 0) table[J.nrows] = piece_total_entry(carry, limit);
}

// pm_rows_carry_start: a lane a row
struct ChainRegs {
    uint64_t reg0[pm_rows::kMaxChains];
};
__global__ __launch_bounds__(kLanes) void rows_carry_start_kernel(pm_rows_carry *carries, int64_t row0, int nrows, ChainRegs regs, int nchains)
{
    const int r = (int)(blockIdx.x * kLanes + threadIdx.x);
    if (r >= nrows) return;
    pm_rows_carry v;
    v.scan.lfsr_state = regs.reg0[(row0 + r) % nchains];
    v.scan.tail = 0;
    v.scan.counted = 0;
    v.scan.pieces = 0;
    v.scan.bytes = 0;
    v.scan.ones = 0;
    v.scan.state = PM_SCAN_CARRY_START;
    v.taken = 0;
    v.last_addr = 0;
    carries[row0 + r] = v;
}

// ---- pm_rows_packets: finished pm_packet rows from the rows' scan parts, behind pm_rows_scan (the rules: pm_rows_packets.h) -------------------
// What the three launches know of the call: the chains by value, the rows' records and steps.  Where a row's part lies in the block follows
// from the records as in rows_prepare_kernel, with the same limits: a row that the scan left out is left out here.
struct RowPk {
    const pm_rowslice_rec *recs;
    const uint16_t *steps;
    int64_t cap, row0;
    int32_t nrows, nchains, tile_words;
    int8_t kind[pm_rows::kMaxChains], frames[pm_rows::kMaxChains], packets[pm_rows::kMaxChains], addrs[pm_rows::kMaxChains], tol[pm_rows::kMaxChains];
    uint8_t pkopt[pm_rows::kMaxChains];
    int32_t source[pm_rows::kMaxChains];
};
struct RowPkInfo {                          // the walk launch's note of a row for the build launch
    int64_t scan;                           // the row's scan part in the block (behind its steps), -1: left out
    int64_t acc0;                           // the row's first place in the accepted list
    int32_t n, reserved;
};
constexpr int kBuildWaves = 1024;           // waves that share a call's packets in the build launch

// Launch 1: a lane a row.  A workgroup first adds up the sums of the rows in front of its own (a lane 16 rows at the most), then scans its
// 256 rows as the prepare launch does: the row's part, and its place in the accepted list -- the events and places in front of it, of
// which a row accepts no more than it has.  Then the row's rule.
__global__ __launch_bounds__(kLanes) void rows_packets_walk_kernel(RowPk K, const uint8_t *block, pm_rows_packets_entry *entries, RowPkInfo *info,
                                                                   pm_rpk::Accepted *acc, pm_rows::Sums limit)
{
    using namespace pm_rows;
    __shared__ Sums lds[kLanes];
    const int r0 = (int)blockIdx.x * kLanes, t = (int)threadIdx.x;
    auto add = [](const Sums &a, const Sums &b) { return sums_add(a, b); };
    auto bytes_of = [&](int r) { return row_bytes(K.recs[K.row0 + r].count, K.cap); };
    auto sums_of = [&](int r) {
        const int c = (int)((K.row0 + r) % K.nchains);
        const int64_t n = bytes_of(r);
        return row_sums(K.kind[c], K.frames[c], K.packets[c], n < kMaxBytes ? n : kMaxBytes, K.tile_words, K.addrs[c]);
    };
    Sums front = sums_zero();
    for (int r = t; r < r0; r += kLanes) front = sums_add(front, sums_of(r));
    block_scan(front, lds, add);
    front = lds[kLanes - 1];
    __syncthreads();
    const int r = r0 + t;
    const bool active = r < K.nrows;
    block_scan(active ? sums_of(r) : sums_zero(), lds, add);
    const Sums before = sums_add(front, t ? lds[t - 1] : sums_zero());
    if (!active) return;
    const int c = (int)((K.row0 + r) % K.nchains), kind = K.kind[c];
    const Entry e = row_entry(before, kind, K.frames[c], K.packets[c], bytes_of(r), K.tile_words, limit, K.addrs[c]);
    pm_rows_packets_entry out{0, PM_ROWS_PACKETS_LEFT_OUT, 0, 0, 0, 0};
    RowPkInfo ri{-1, before.events + before.places, e.n, 0};
    if (e.off >= 0) {
        ri.scan = e.off + steps_bytes(e.n);
        const pm_rpk::Part p = pm_rpk::part_of(block + ri.scan, kind, e.n);
        out.lfsr_state = pm_rpk::ld64(p.rec);
        pm_rpk::Accepted *mine = acc + ri.acc0;
        auto emit = [mine](int i, const pm_rpk::Accepted &a) { mine[i] = a; };
        if (kind == 1) out.status = pm_rpk::il2p_walk(p, K.tol[c], K.pkopt[c] & 1, &out.packets, &out.corrected_left, emit);
        else if (kind == 0) out.status = pm_rpk::ax25_walk(p, &out.packets, emit);
        else out.status = PM_ROWS_PACKETS_NO_CODEC;
        if (out.status != PM_ROWS_PACKETS_FINISHED) out.packets = out.corrected_left = 0;
    }
    entries[r] = out;
    info[r] = ri;
}

// Launch 2: one workgroup, trips of 256 rows, a lane a row: an inclusive scan of the rows' counts over the lanes, the carry from trip to
// trip.  A row whose packets would pass the capacity takes none, and no row behind it does (the sum only grows): NO_ROOM, at the total.
__global__ __launch_bounds__(kLanes) void rows_packets_room_kernel(int nrows, pm_rows_packets_head *head, pm_rows_packets_entry *entries, int64_t capacity)
{
    __shared__ int64_t lds[kLanes];
    __shared__ unsigned long long kept;     // the packets of the rows that have room
    __shared__ int handed;
    const int t = (int)threadIdx.x;
    if (t == 0) {
        kept = 0;
        handed = 0;
    }
    __syncthreads();
    int64_t carry = 0;
    for (int r0 = 0; r0 < nrows; r0 += kLanes) {
        const int r = r0 + t;
        const bool active = r < nrows;
        pm_rows_packets_entry e{0, 0, 0, 0, 0, 0};
        if (active) e = entries[r];
        const int64_t incl = carry + block_scan((int64_t)e.packets, lds, [](int64_t a, int64_t b) { return a + b; });
        carry += lds[kLanes - 1];
        const bool over = pm_rpk::no_room(incl, capacity);
        if (active && !over) atomicMax(&kept, (unsigned long long)incl);
        if (active && (over || e.status != PM_ROWS_PACKETS_FINISHED)) atomicAdd(&handed, 1);
        __syncthreads();                    // (a row without room has no row with room behind it: `kept` is final for it)
        if (active) {
            e.first = over ? (int64_t)kept : incl - e.packets;
            if (over) {
                e.status = PM_ROWS_PACKETS_NO_ROOM;
                e.packets = e.corrected_left = 0;
            }
            entries[r] = e;
        }
    }
    __syncthreads();
    if (t == 0) *head = pm_rows_packets_head{nrows, handed, (int64_t)kept};
}

// Launch 3: a fixed grid, a wave a workgroup; wave w takes the packets w, w + waves, ... up to the call's total.  The packet's row by binary
// search over `first`; its bytes put together in LDS -- IL2P: the AX.25 header that lane 0 rebuilds from the 13 bytes in the area, the
// payload a byte a lane, the CRC of both by the frames launch's join, the carried CRC from the Hamming-coded bytes behind the last block
// or the computed one; AX.25: the frame from the area, its CRC from the table -- then the address, the data bytes as whole words with zeros
// behind the packet, and the 40-byte head by lane 0 (pm_rpk::packet_build_to says the same for one thread).
// What differs between the row form and the job form is the source S: which row (or job) a packet belongs to and where that one's part
// lies, where the address of a byte comes from, and where the packet goes and how many words of data it takes there.
struct BuildItem {
    pm_rpk::Part p;
    pm_rpk::Accepted a;
    int kind, crc, source;
    uint8_t *dst;
};
template <class Src>
__device__ inline void packets_build(const Src &S, const uint8_t *block)
{
    using namespace pm_rpk;
    __shared__ uint64_t pkt64[PM_PKT_MAX / 8];
    __shared__ uint16_t crc_table[256];
    const int lane = (int)threadIdx.x;
    uint8_t *pkt = reinterpret_cast<uint8_t *>(pkt64);
    const int64_t total = S.total();
    if ((int64_t)blockIdx.x >= total) return;
    wave_crc_table(crc_table, lane);
    for (int64_t q = (int64_t)blockIdx.x; q < total; q += (int64_t)gridDim.x) {
        const int r = S.row_of(q);
        const BuildItem it = S.item(block, r, q);
        const Part &p = it.p;
        const Accepted &a = it.a;
        __syncthreads();
        for (int v = lane; v < PM_PKT_MAX / 8; v += 64) pkt64[v] = 0;
        __syncthreads();
        int len, calculated;
        uint32_t carried;
        int64_t k;
        if (it.kind == 1) {
            const pm_il2p::Rec rec = ld_rec(p, (int32_t)a.index);
            const uint8_t *src = p.area + rec.off;
            int hl = 0;
            if (lane == 0) hl = pm_il2p::ax25_header(src, pkt);
            hl = __shfl(hl, 0);
            for (int v = lane; v < (int)rec.count; v += 64) pkt[hl + v] = src[13 + v];
            __syncthreads();
            const int body = hl + (int)rec.count;
            uint32_t crc = 0xFFFF;
            if (body == 1) crc = (crc >> 8) ^ crc_table[(crc ^ pkt[0]) & 0xFF];
            else if (body >= 2) crc = wave_crc(crc_table, lane, body, crc, [pkt](int i) -> uint32_t { return pkt[i]; });
            calculated = (int)((crc ^ 0xFFFF) & 0xFFFF);
            int64_t E = (int64_t)a.bit + 1;
            carried = (uint32_t)calculated;                 // il2p.py:427-431: without the trailing CRC the computed one is appended
            if (it.crc) {
                carried = (uint32_t)pm_il2p::hamming_crc(byte_at(p.plain, E), byte_at(p.plain, E + 8), byte_at(p.plain, E + 16), byte_at(p.plain, E + 24));
                E += 32;
            }
            len = body + 2;
            if (lane == 0) {
                pkt[body] = (uint8_t)(carried & 0xFF);
                pkt[body + 1] = (uint8_t)(carried >> 8);
            }
            k = (E - 1) >> 3;
        } else {
            const uint32_t F = ld32(p.list + 8 * (int64_t)a.index + 4);
            const int64_t at = F == 0xFFFFFFFFu ? 0 : (int64_t)(F >> 3);
            const int whole = (int32_t)ld32(p.table + 8 * (int64_t)a.index);
            len = whole < PM_PKT_MAX ? whole : PM_PKT_MAX;  // (a frame longer than a row: its first bytes, the whole frame's CRCs)
            calculated = (int)ld32(p.table + 8 * (int64_t)a.index + 4);
            carried = (uint32_t)p.area[at + whole - 1] * 256u + p.area[at + whole - 2];
            for (int v = lane; v < len; v += 64) pkt[v] = p.area[at + v];
            k = (int64_t)(a.bit >> 3);
        }
        __syncthreads();
        const int64_t addr = S.address(p, r, k, lane);
        for (int v = lane, words = S.data_words(len); v < words; v += 64) reinterpret_cast<uint64_t *>(it.dst + 40)[v] = pkt64[v];
        if (lane == 0) {
            const HeadWords h = head_words(addr, pkt, len, a.corrected, calculated, carried, it.source);
            for (int v = 0; v < 5; ++v) reinterpret_cast<uint64_t *>(it.dst)[v] = h.w[v];
        }
    }
}

// the row form: head and entries are read where the room launch left them, in d_out; a packet is a whole pm_packet row; the address is the
// checkpoint in front plus up to 63 of the row's steps, a lane a step (pm_addrs::resolve across the wave: steps (k & ~63) + 1 .. k)
struct RowBuild {
    const RowPk &K;
    uint8_t *out;
    const RowPkInfo *info;
    const pm_rpk::Accepted *acc;
    __device__ const pm_rows_packets_entry *entries() const { return reinterpret_cast<const pm_rows_packets_entry *>(out + pm_rpk::kHeadBytes); }
    __device__ int64_t total() const { return reinterpret_cast<const pm_rows_packets_head *>(out)->packets; }
    __device__ int row_of(int64_t q) const
    {
        const pm_rows_packets_entry *e = entries();
        return pm_rpk::row_of_packet([e](int i) { return e[i].first; }, K.nrows, q);
    }
    __device__ BuildItem item(const uint8_t *block, int r, int64_t q) const
    {
        const RowPkInfo ri = info[r];
        const int c = (int)((K.row0 + r) % K.nchains), kind = K.kind[c];
        uint8_t *rows = out + pm_rpk::kHeadBytes + (size_t)pm_rpk::kEntryBytes * (size_t)K.nrows;
        return BuildItem{pm_rpk::part_of(block + ri.scan, kind, ri.n), acc[ri.acc0 + (q - entries()[r].first)], kind, K.pkopt[c] & 1, K.source[c],
                         rows + (size_t)q * sizeof(pm_packet)};
    }
    __device__ int64_t address(const pm_rpk::Part &p, int r, int64_t k, int lane) const
    {
        const uint16_t *steps = K.steps + (K.row0 + r) * K.cap;
        const int64_t i = (k & ~(int64_t)63) + 1 + lane;
        uint32_t gone = i <= k ? steps[i] : 0u;
        for (int dl = 32; dl; dl >>= 1) gone += __shfl_xor(gone, dl);
        return p.addrs[k >> 6] + (int64_t)gone;
    }
    __device__ static int data_words(int) { return PM_PKT_MAX / 8; }
};
__global__ __launch_bounds__(64) void rows_packets_build_kernel(RowPk K, const uint8_t *block, uint8_t *out, const RowPkInfo *info, const pm_rpk::Accepted *acc)
{
    packets_build(RowBuild{K, out, info, acc}, block);
}

// ---- pm_stream_packets: the same last step for the jobs of a pm_stream_scan call, into the dense form (the rules: pm_rows_packets.h) ---------
// What the three launches know of the call, by value: where a job's part lies (the host's offsets), its bytes, its addresses.
struct StreamPk {
    int64_t off[kScanJobs];
    const int64_t *addr[kScanJobs];
    int32_t n[kScanJobs];
    int32_t acc0[kScanJobs];                // the job's first place in the accepted list and the record offsets
    int32_t source[kScanJobs];
    int8_t kind[kScanJobs], tol[kScanJobs];
    uint8_t crc[kScanJobs];
    int32_t njobs;
};
static_assert(sizeof(StreamPk) + 64 <= 4096, "the table goes to the kernels by value");
// What the launches leave for each other, in context scratch (d_out is never read).  entry[j].first_byte: behind the walk launch the bytes
// of job j's records, behind the room launch where they begin.
struct StreamPkNotes {
    pm_stream_packets_entry entry[kScanJobs];
    int64_t first[kScanJobs];               // the job's first record among the call's
    int64_t packets, bytes;                 // the records that have room, and their bytes
};
__device__ inline int64_t wave_incl_sum(int64_t v, int lane)
{
    for (int dl = 1; dl < 64; dl <<= 1) {
        const int64_t o = __shfl_up(v, dl);
        if (lane >= dl) v += o;
    }
    return v;
}

// Launch 1: a wave a job.  AX.25: trips of 64 listed events, a lane an event -- the rule's checks for that event, the lane's place in the
// accepted list from a ballot and the count of the lanes in front, its record's offset from a prefix sum of the record sizes over the wave,
// both on top of what the trips before counted.  A table that cannot be the stream's ends the walk at the trip that finds it (what the
// trips before listed is never looked at: the job has no packets).  IL2P: lane 0 walks the packet table by the rule.
__global__ __launch_bounds__(64) void stream_packets_walk_kernel(StreamPk K, const uint8_t *block, StreamPkNotes *notes, pm_rpk::Accepted *acc, int64_t *recoff)
{
    using namespace pm_rpk;
    const int j = (int)blockIdx.x, lane = (int)threadIdx.x, kind = K.kind[j];
    const Part p = part_of(block + K.off[j], kind, K.n[j]);
    Accepted *mine = acc + K.acc0[j];
    int64_t *offs = recoff + K.acc0[j];
    pm_stream_packets_entry out{ld64(p.rec), PM_ROWS_PACKETS_NO_CODEC, 0, 0, 0, 0};
    int64_t bytes = 0;
    if (kind == 0) {
        int32_t events, count = 0;
        out.status = ax25_start(p, &events);
        for (int32_t e0 = 0; e0 < events; e0 += 64) {
            const int32_t e = e0 + lane;
            Ax25Event ev{false, false, 0, 0};
            if (e < events) ev = ax25_event(p, e);
            if (__any(ev.bad)) {
                out.status = PM_ROWS_PACKETS_LONG_FRAME;
                break;
            }
            const uint64_t taken = __ballot(ev.take);
            const int64_t size = ev.take ? record_bytes(ev.len) : 0, incl = wave_incl_sum(size, lane);
            if (ev.take) {
                const int place = count + lanes_before(taken, lane);
                mine[place] = Accepted{(uint32_t)e, ev.P, 0, 0};
                offs[place] = bytes + incl - size;
            }
            count += __popcll(taken);
            bytes += __shfl(incl, 63);
        }
        out.packets = count;
    } else if (kind == 1 && lane == 0) {
        const Part &pp = p;
        int64_t *sum = &bytes;
        out.status = il2p_walk(p, K.tol[j], K.crc[j] != 0, &out.packets, &out.corrected_left, [mine, offs, sum, &pp](int i, const Accepted &a) {
            mine[i] = a;
            offs[i] = *sum;
            *sum += record_bytes(il2p_len(pp, ld_rec(pp, (int32_t)a.index)));
        });
    }
    if (lane == 0) {
        if (out.status != PM_ROWS_PACKETS_FINISHED) {
            out.packets = out.corrected_left = 0;
            bytes = 0;
        }
        out.first_byte = bytes;
        notes->entry[j] = out;
    }
}

// Launch 2: one wave, a lane a job: an inclusive scan of the jobs' bytes and of their counts.  A job whose records would pass the room takes
// none, and no job behind it does (the sum only grows): NO_ROOM, at the total.  Head and entries go out as whole words.
__global__ __launch_bounds__(64) void stream_packets_room_kernel(int njobs, StreamPkNotes *notes, uint64_t *out, int64_t capacity)
{
    const int j = (int)threadIdx.x;
    const bool active = j < njobs;
    pm_stream_packets_entry e{0, 0, 0, 0, 0, 0};
    if (active) e = notes->entry[j];
    const int64_t bytes = e.first_byte, incl_b = wave_incl_sum(bytes, j), incl_p = wave_incl_sum((int64_t)e.packets, j);
    const bool over = pm_rpk::no_room(incl_b, capacity);
    int64_t kept_b = active && !over ? incl_b : 0, kept_p = active && !over ? incl_p : 0;
    for (int dl = 32; dl; dl >>= 1) {
        kept_b = max(kept_b, (int64_t)__shfl_xor(kept_b, dl));
        kept_p = max(kept_p, (int64_t)__shfl_xor(kept_p, dl));
    }
    const int handed = __popcll(__ballot(active && (over || e.status != PM_ROWS_PACKETS_FINISHED)));
    if (active) {
        e.first_byte = over ? kept_b : incl_b - bytes;
        if (over) {
            e.status = PM_ROWS_PACKETS_NO_ROOM;
            e.packets = e.corrected_left = 0;
        }
        notes->entry[j] = e;
        notes->first[j] = over ? kept_p : incl_p - e.packets;
        uint64_t *w = out + 4 + 4 * j;
        w[0] = e.lfsr_state;
        w[1] = (uint64_t)(uint32_t)e.status | (uint64_t)(uint32_t)e.packets << 32;
        w[2] = (uint64_t)e.first_byte;
        w[3] = (uint64_t)(uint32_t)e.corrected_left;
    }
    if (j == 0) {
        notes->packets = kept_p;
        notes->bytes = kept_b;
        out[0] = (uint64_t)(uint32_t)njobs | (uint64_t)(uint32_t)handed << 32;
        out[1] = (uint64_t)kept_p;
        out[2] = (uint64_t)kept_b;
        out[3] = 0;
    }
}

// Launch 3, the job form: the notes are read from scratch; a packet is a record of 40 + pad8(len) bytes at the job's first byte plus the
// walk's offset; the address is the stream's own, whole
struct StreamBuild {
    const StreamPk &K;
    uint8_t *records;
    const StreamPkNotes *notes;
    const pm_rpk::Accepted *acc;
    const int64_t *recoff;
    __device__ int64_t total() const { return notes->packets; }
    __device__ int row_of(int64_t q) const
    {
        const int64_t *first = notes->first;
        return pm_rpk::row_of_packet([first](int i) { return first[i]; }, K.njobs, q);
    }
    __device__ BuildItem item(const uint8_t *block, int r, int64_t q) const
    {
        const int kind = K.kind[r];
        const int64_t i = K.acc0[r] + (q - notes->first[r]);
        pm_rpk::Part p = pm_rpk::part_of(block + K.off[r], kind, K.n[r]);
        p.addrs = K.addr[r];
        return BuildItem{p, acc[i], kind, K.crc[r], K.source[r], records + notes->entry[r].first_byte + recoff[i]};
    }
    __device__ static int64_t address(const pm_rpk::Part &p, int, int64_t k, int) { return p.addrs[k]; }
    __device__ static int data_words(int len) { return (len + 7) >> 3; }
};
__global__ __launch_bounds__(64) void stream_packets_build_kernel(StreamPk K, const uint8_t *block, uint8_t *records, const StreamPkNotes *notes,
                                                                  const pm_rpk::Accepted *acc, const int64_t *recoff)
{
    packets_build(StreamBuild{K, records, notes, acc, recoff}, block);
}

// what the launches share in context scratch, cut for `jobs` jobs (or rows)
struct ScanScratch {
    TileSum *sums;
    TileCarry *carries;
    int32_t *counts;
    uint2 *lists;
    uint32_t *cands;
    int32_t *work, *pkcounts;
    PkRec *recs;
    uint8_t *extra;                         // `extra_bytes` behind everything, 64-byte aligned (the row table)
    int64_t *steps_before;                  // the row form's addrs: per tile the steps of its row's tiles in front, nullptr: no checkpoints
    pm_scan_carry *carry_in;                // the carries as the jobs (or the rows' pieces) found them, one per job, nullptr: none is carried
};
int scan_scratch(pm_ctx *ctx, size_t jobs, int64_t tiles, int64_t copies, int64_t places, size_t extra_bytes, ScanScratch *out, bool steps_before = false,
                 size_t carries = 0)
{
    const size_t sums_bytes = ((size_t)tiles * sizeof(TileSum) + 63) & ~(size_t)63;
    // (frames: the event counts and a copy of the lists stay on the device for the frames launch, behind the carries)
    const size_t carries_bytes = ((size_t)tiles * sizeof(TileCarry) + 63) & ~(size_t)63, counts_bytes = copies || places ? jobs * sizeof(int32_t) : 0;
    // (packets: the candidates, a copy of every record with its header bytes, the list of those with blocks to decode, and the two counts per job)
    const size_t lists_bytes = (size_t)copies * sizeof(uint2), cands_bytes = ((size_t)places * sizeof(uint32_t) + 63) & ~(size_t)63, recs_bytes = (size_t)places * sizeof(PkRec);
    const size_t pk_bytes = places ? 2 * cands_bytes + recs_bytes + 2 * jobs * sizeof(int32_t) : 0;
    const size_t extra_padded = (extra_bytes + 63) & ~(size_t)63, before_bytes = steps_before ? (size_t)tiles * sizeof(int64_t) : 0;
    const size_t carry_bytes = carries * sizeof(pm_scan_carry);
    if (int rc = pm_scratch_reserve(ctx, sums_bytes + carries_bytes + counts_bytes + lists_bytes + pk_bytes + extra_padded + before_bytes + carry_bytes + 256)) return rc;
    uint8_t *base = static_cast<uint8_t *>(ctx->d_scratch);
    out->sums = reinterpret_cast<TileSum *>(base);
    out->carries = reinterpret_cast<TileCarry *>(base + sums_bytes);
    out->counts = copies || places ? reinterpret_cast<int32_t *>(base + sums_bytes + carries_bytes) : nullptr;
    out->lists = reinterpret_cast<uint2 *>(base + sums_bytes + carries_bytes + counts_bytes);
    uint8_t *pk = reinterpret_cast<uint8_t *>(((uintptr_t)out->lists + lists_bytes + 63) & ~(uintptr_t)63);
    out->cands = reinterpret_cast<uint32_t *>(pk);
    out->work = reinterpret_cast<int32_t *>(pk + cands_bytes);
    out->pkcounts = reinterpret_cast<int32_t *>(pk + 2 * cands_bytes);
    out->recs = reinterpret_cast<PkRec *>(pk + 2 * cands_bytes + 2 * jobs * sizeof(int32_t));
    out->extra = reinterpret_cast<uint8_t *>(((uintptr_t)pk + pk_bytes + 63) & ~(uintptr_t)63);
    out->steps_before = steps_before ? reinterpret_cast<int64_t *>(out->extra + extra_padded) : nullptr;
    out->carry_in = carries ? reinterpret_cast<pm_scan_carry *>(out->extra + extra_padded + before_bytes) : nullptr;     // (64-byte aligned: extra is, and the others are multiples of 64 or 8)
    return PM_OK;
}

// the launches behind either table: `emit`: some job has a list to write; frame_waves, packet_waves: the waves that share a job
// (L: the table for the launches behind the combine -- the job form's with `late` set, see ScanJobs::carry_in)
template <class Jobs>
void scan_launch(pm_ctx *ctx, const Jobs &J, const Jobs &L, int njobs, int64_t tiles, int64_t copies, int64_t places, bool emit, uint8_t *block, const ScanScratch &s,
                 int frame_waves, int packet_waves)
{
    if (tiles) hipLaunchKernelGGL(bitscan_tile_kernel<Jobs>, dim3((unsigned)tiles), dim3(kLanes), 0, ctx->stream, J, block, s.sums);
    hipLaunchKernelGGL(bitscan_combine_kernel<Jobs>, dim3(njobs), dim3(64), 0, ctx->stream, J, block, s.sums, s.carries, s.counts, s.steps_before, s.carry_in);
    if (emit && tiles) hipLaunchKernelGGL(bitscan_emit_kernel<Jobs>, dim3((unsigned)tiles), dim3(kLanes), 0, ctx->stream, L, block, s.carries, s.lists, s.cands);
    if (copies) hipLaunchKernelGGL(bitscan_frames_kernel<Jobs>, dim3(frame_waves, njobs), dim3(64), 0, ctx->stream, L, block, s.lists, s.counts);
    if (places) {
        const int ptune = ctx->tune.bitscan_packet_waves;
        hipLaunchKernelGGL(bitscan_headers_kernel<Jobs>, dim3(njobs), dim3(64), 0, ctx->stream, L, block, s.counts, s.cands, s.recs, s.work, s.pkcounts);
        hipLaunchKernelGGL(bitscan_blocks_kernel<Jobs>, dim3(ptune > 0 ? std::min(ptune, 1024) : packet_waves, njobs), dim3(64), 0, ctx->stream, L, block, s.recs,
                           s.work, s.pkcounts);
    }
}

// pm_scan_carry_set: one lane stores the seeded carry
__global__ void carry_set_kernel(pm_scan_carry *d_carry, pm_scan_carry v) { *d_carry = v; }

}  // namespace

extern "C" int pm_scan_carry_set(pm_ctx *ctx, pm_scan_carry *d_carry, uint64_t lfsr_state, int32_t ones, int64_t counted)
{
    PM_CTX(ctx);
    PM_ARG(d_carry && ((uintptr_t)d_carry & 7) == 0 && ones >= 0);
    pm_scan_carry v;
    memset(&v, 0, sizeof(v));
    v.lfsr_state = lfsr_state;
    v.ones = ones < 7 ? ones : 7;
    v.tail = tail_of_ones(v.ones);
    v.counted = counted;
    v.state = counted < 0 ? PM_SCAN_CARRY_LOST : ones == 0 && counted == 0 ? PM_SCAN_CARRY_START : PM_SCAN_CARRY_OK;
    hipLaunchKernelGGL(carry_set_kernel, dim3(1), dim3(1), 0, ctx->stream, d_carry, v);
    PM_HIP(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_stream_scan(pm_ctx *ctx, const pm_scan_job *h_jobs, int njobs, void *d_block, size_t block_bytes, int64_t *h_offsets, size_t *h_used)
{
    PM_CTX(ctx);
    PM_ARG(h_jobs && njobs >= 1 && njobs <= kScanJobs && d_block && ((uintptr_t)d_block & 7) == 0 && h_offsets && h_used);
    ScanJobs J;
    memset(&J, 0, sizeof(J));
    J.njobs = njobs;
    const int tune = ctx->tune.bitscan_tile_words;
    J.tile_words = tune > 0 ? std::min(tune, kLanes) : kLanes;
    const int ftune = ctx->tune.bitscan_frame_words;
    J.frame_words = ftune > 0 ? std::min(ftune, 64) : 64;
    size_t at = 0;
    int64_t tiles = 0, copies = 0, places = 0;
    bool any_carry = false;
    for (int j = 0; j < njobs; ++j) {
        const pm_scan_job &q = h_jobs[j];
        PM_ARG(q.n >= 0 && q.n <= (int64_t)1 << 29 && (q.n == 0 || (q.d_data && ((uintptr_t)q.d_data & 7) == 0)));
        PM_ARG(q.codec_kind >= -1 && q.codec_kind <= 1);
        PM_ARG(q.frames == 0 || (q.frames == 1 && q.codec_kind == 0));
        PM_ARG(q.packets == 0 || (q.packets == 1 && q.codec_kind == 1));
        PM_ARG(q.addrs == 0 || (q.addrs == 1 && q.d_addr && ((uintptr_t)q.d_addr & 7) == 0));
        J.addr[j] = q.addrs ? q.d_addr : nullptr;
        J.data[j] = q.d_data;
        J.poly[j] = q.lfsr_poly;
        J.reg0[j] = q.lfsr_state;
        if (q.d_carry) {                                    // a piece of a stream: the register comes from the carry, whose pointer takes its place
            PM_ARG(((uintptr_t)q.d_carry & 7) == 0);
            for (int i = 0; i < j; ++i) PM_ARG(h_jobs[i].d_carry != q.d_carry);
            J.reg0[j] = (uint64_t)(uintptr_t)q.d_carry;
            J.carried[j] = 1;
            any_carry = true;
        }
        J.n[j] = (int32_t)q.n;
        J.kind[j] = (int8_t)q.codec_kind;
        J.invert[j] = q.lfsr_invert != 0;
        J.tol[j] = (int8_t)std::max(-1, std::min(33, q.sync_tol));
        J.off[j] = h_offsets[j] = (int64_t)at;
        J.tile0[j] = (int32_t)tiles;
        at += PM_SCAN_HEAD + (size_t)list_bytes(q.codec_kind, q.n) + (size_t)((q.n + 7) & ~int64_t(7));
        J.ev0[j] = -1;
        if (q.frames) {
            at += (size_t)PM_SCAN_FRAME_TABLE_BYTES(q.n) + (size_t)PM_SCAN_FRAME_AREA_BYTES(q.n);
            J.ev0[j] = (int32_t)copies;
            copies += q.n / 19 + 2;
            PM_ARG(copies < INT32_MAX);                     // (ev0 is 32 bits; 64 jobs of 2^29 bytes stay below it)
        }
        J.pk0[j] = -1;
        if (q.packets) {
            at += (size_t)PM_SCAN_PACKET_TABLE_BYTES(q.n) + (size_t)PM_SCAN_PACKET_AREA_BYTES(q.n);
            J.pk0[j] = (int32_t)places;
            // (a min_dist below 0 corrects what 0 does, one above 8 nothing: the locator has eight roots at most)
            J.pkopt[j] = (uint8_t)((q.il2p_crc != 0) | (q.il2p_disable_rs != 0) << 1 | std::max(0, std::min(9, q.il2p_min_dist)) << 2);
            places += q.n / 64 + 2;
        }
        if (q.addrs) at += (size_t)PM_SCAN_ADDR_BYTES(q.n);   // behind everything else of the part
        if (q.d_carry) at += PM_SCAN_CARRY_BYTES;             // ... but the carry piece
        tiles += pm_cdiv(pm_cdiv(q.n, 8), J.tile_words);
        PM_ARG(tiles < (int64_t)1 << 30);
    }
    J.tile0[njobs] = (int32_t)tiles;
    *h_used = at;
    if (at > block_bytes) return pm_set_error(PM_ERR_CAPACITY, "pm_stream_scan: the block holds %zu bytes, the batch needs %zu", block_bytes, at);
    ScanScratch s;
    if (int rc = scan_scratch(ctx, kScanJobs, tiles, copies, places, 0, &s, false, any_carry ? kScanJobs : 0)) return rc;
    ScanJobs L = J;                                         // behind the combine launch the carries are read from its copies
    L.carry_in = s.carry_in;
    L.late = 1;
    bool any = false;
    for (int j = 0; j < njobs; ++j) any = any || ((h_jobs[j].codec_kind == 0 || h_jobs[j].packets) && h_jobs[j].n > 0);
    scan_launch(ctx, J, L, njobs, tiles, copies, places, any, static_cast<uint8_t *>(d_block), s, kFrameWaves, kPacketWaves);
    PM_HIP(hipGetLastError());
    return PM_OK;
}

// what pm_rows_scan and pm_rows_scan_pieces share: the arguments' checks and the table's fields that do not depend on the rows
static int rows_jobs_fill(pm_ctx *ctx, RowJobs &J, const pm_rowslice_rec *d_recs, const uint8_t *d_data, const uint16_t *d_steps, int64_t cap, int64_t row0, int nrows,
                          const pm_rows_scan_chain *h_chains, int nchains, const int64_t *h_counts, void *d_block, int64_t *h_offsets, size_t *h_used)
{
    using namespace pm_rows;
    PM_ARG(d_recs && d_data && d_steps && cap >= 0 && (cap & 7) == 0 && ((uintptr_t)d_data & 7) == 0 && ((uintptr_t)d_steps & 7) == 0 && row0 >= 0);
    PM_ARG(nrows >= 1 && nrows <= kMaxRows && h_chains && nchains >= 1 && nchains <= kMaxChains && h_counts);
    PM_ARG(d_block && ((uintptr_t)d_block & 7) == 0 && h_offsets && h_used);
    J.data = d_data;
    J.steps = d_steps;
    J.recs = d_recs;
    J.cap = cap;
    J.row0 = row0;
    J.nrows = nrows;
    J.nchains = nchains;
    const int tune = ctx->tune.bitscan_tile_words;
    J.tile_words = tune > 0 ? std::min(tune, kLanes) : kLanes;
    const int ftune = ctx->tune.bitscan_frame_words;
    J.frame_words = ftune > 0 ? std::min(ftune, 64) : 64;
    for (int c = 0; c < nchains; ++c) {
        const pm_rows_scan_chain &q = h_chains[c];
        PM_ARG(q.codec_kind >= -1 && q.codec_kind <= 1);
        PM_ARG(q.frames == 0 || (q.frames == 1 && q.codec_kind == 0));
        PM_ARG(q.packets == 0 || (q.packets == 1 && q.codec_kind == 1));
        PM_ARG(q.addrs == 0 || q.addrs == 1);
        J.addrs[c] = (int8_t)q.addrs;
        J.poly[c] = q.lfsr_poly;
        J.reg0[c] = q.lfsr_state;
        J.kind[c] = (int8_t)q.codec_kind;
        J.invert[c] = q.lfsr_invert != 0;
        J.tol[c] = (int8_t)std::max(-1, std::min(33, q.sync_tol));
        J.frames[c] = (int8_t)q.frames;
        J.packets[c] = (int8_t)q.packets;
        // (a min_dist below 0 corrects what 0 does, one above 8 nothing: the locator has eight roots at most)
        J.pkopt[c] = (uint8_t)((q.il2p_crc != 0) | (q.il2p_disable_rs != 0) << 1 | std::max(0, std::min(9, q.il2p_min_dist)) << 2);
    }
    return PM_OK;
}

extern "C" int pm_rows_scan(pm_ctx *ctx, const pm_rowslice_rec *d_recs, const uint8_t *d_data, const uint16_t *d_steps, int64_t cap, int64_t row0, int nrows,
                            const pm_rows_scan_chain *h_chains, int nchains, const int64_t *h_counts, void *d_block, size_t block_bytes, int64_t *h_offsets,
                            size_t *h_used)
{
    using namespace pm_rows;
    PM_CTX(ctx);
    RowJobs J;
    memset(&J, 0, sizeof(J));
    if (int rc = rows_jobs_fill(ctx, J, d_recs, d_data, d_steps, cap, row0, nrows, h_chains, nchains, h_counts, d_block, h_offsets, h_used)) return rc;
    // the host's copy of the sums, for the sizes: the device makes its own from the records
    Sums all = sums_zero();
    bool any = false, any_addrs = false;
    for (int r = 0; r < nrows; ++r) {
        const pm_rows_scan_chain &q = h_chains[(row0 + r) % nchains];
        any_addrs = any_addrs || q.addrs;
        const int64_t n = h_counts[r];
        PM_ARG(n >= 0 && n <= cap && n <= kMaxBytes);
        h_offsets[r] = all.off;
        all = sums_add(all, row_sums(q.codec_kind, q.frames, q.packets, n, J.tile_words, q.addrs));
        PM_ARG(all.tiles < (int64_t)1 << 30);
        any = any || ((q.codec_kind == 0 || q.packets) && n > 0);
    }
    *h_used = (size_t)all.off;
    if ((size_t)all.off > block_bytes) return pm_set_error(PM_ERR_CAPACITY, "pm_rows_scan: the block holds %zu bytes, the rows need %zu", block_bytes, (size_t)all.off);
    ScanScratch s;
    if (int rc = scan_scratch(ctx, (size_t)nrows, all.tiles, all.events, all.places, ((size_t)nrows + 1) * sizeof(Entry), &s, any_addrs)) return rc;
    Entry *table = reinterpret_cast<Entry *>(s.extra);
    J.table = table;
    hipLaunchKernelGGL(rows_prepare_kernel, dim3(1), dim3(kLanes), 0, ctx->stream, J, d_recs, table, all);
    scan_launch(ctx, J, J, nrows, all.tiles, all.events, all.places, any, static_cast<uint8_t *>(d_block), s, kRowFrameWaves, kRowPacketWaves);
    if (any_addrs && all.tiles)
        hipLaunchKernelGGL(rows_addrs_kernel<RowJobs>, dim3((unsigned)all.tiles), dim3(kLanes), 0, ctx->stream, J, static_cast<uint8_t *>(d_block), s.steps_before);
    PM_HIP(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_rows_carry_start(pm_ctx *ctx, pm_rows_carry *d_carries, int64_t row0, int nrows, const pm_rows_scan_chain *h_chains, int nchains)
{
    PM_CTX(ctx);
    PM_ARG(d_carries && ((uintptr_t)d_carries & 7) == 0 && row0 >= 0 && nrows >= 1 && h_chains && nchains >= 1 && nchains <= pm_rows::kMaxChains);
    ChainRegs regs;
    memset(&regs, 0, sizeof(regs));
    for (int c = 0; c < nchains; ++c) regs.reg0[c] = h_chains[c].lfsr_state;
    hipLaunchKernelGGL(rows_carry_start_kernel, dim3((unsigned)pm_cdiv(nrows, kLanes)), dim3(kLanes), 0, ctx->stream, d_carries, row0, nrows, regs, nchains);
    PM_HIP(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_rows_scan_pieces(pm_ctx *ctx, const pm_rowslice_rec *d_recs, const uint8_t *d_data, const uint16_t *d_steps, int64_t cap, int64_t row0, int nrows,
                                   const pm_rows_scan_chain *h_chains, int nchains, pm_rows_carry *d_carries, const int64_t *d_upto, int32_t final_piece,
                                   const int64_t *h_counts, void *d_block, size_t block_bytes, int64_t *h_offsets, size_t *h_used)
{
    using namespace pm_rows;
    PM_CTX(ctx);
    RowPieceJobs J;
    memset(&J, 0, sizeof(J));
    if (int rc = rows_jobs_fill(ctx, J, d_recs, d_data, d_steps, cap, row0, nrows, h_chains, nchains, h_counts, d_block, h_offsets, h_used)) return rc;
    PM_ARG(d_carries && ((uintptr_t)d_carries & 7) == 0 && ((uintptr_t)d_upto & 7) == 0);
    J.carries = d_carries;
    // the host's copy of the sums, for the sizes: the device cuts the pieces itself, from the records, d_upto and the carries
    Sums all = sums_zero();
    bool any = false, any_addrs = false;
    for (int r = 0; r < nrows; ++r) {
        const pm_rows_scan_chain &q = h_chains[(row0 + r) % nchains];
        any_addrs = any_addrs || q.addrs;
        const int64_t n = h_counts[r];
        PM_ARG(n >= 0 && n <= cap && n <= kMaxBytes);
        h_offsets[r] = all.off;
        all = sums_add(all, piece_sums(q.codec_kind, q.frames, q.packets, n, J.tile_words, q.addrs));
        PM_ARG(all.tiles < (int64_t)1 << 30);
        any = any || ((q.codec_kind == 0 || q.packets) && n > 0);
    }
    *h_used = (size_t)all.off;
    if ((size_t)all.off > block_bytes)
        return pm_set_error(PM_ERR_CAPACITY, "pm_rows_scan_pieces: the block holds %zu bytes, the pieces need %zu", block_bytes, (size_t)all.off);
    ScanScratch s;
    if (int rc = scan_scratch(ctx, (size_t)nrows, all.tiles, all.events, all.places, ((size_t)nrows + 1) * sizeof(PieceEntry), &s, any_addrs, (size_t)nrows)) return rc;
    PieceEntry *table = reinterpret_cast<PieceEntry *>(s.extra);
    J.ptable = table;
    RowPieceJobs L = J;                                     // behind the combine launch the carries are read from its copies
    L.carry_in = s.carry_in;
    L.late = 1;
    hipLaunchKernelGGL(rows_pieces_prepare_kernel, dim3(1), dim3(kLanes), 0, ctx->stream, J, d_recs, d_upto, final_piece, table, all);
    scan_launch(ctx, J, L, nrows, all.tiles, all.events, all.places, any, static_cast<uint8_t *>(d_block), s, kRowFrameWaves, kRowPacketWaves);
    if (any_addrs && all.tiles)
        hipLaunchKernelGGL(rows_addrs_kernel<RowPieceJobs>, dim3((unsigned)all.tiles), dim3(kLanes), 0, ctx->stream, L, static_cast<uint8_t *>(d_block), s.steps_before);
    PM_HIP(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_rows_packets(pm_ctx *ctx, const pm_rowslice_rec *d_recs, const uint16_t *d_steps, int64_t cap, int64_t row0, int nrows,
                               const pm_rows_scan_chain *h_chains, int nchains, const int32_t *h_sources, const int64_t *h_counts, const void *d_block,
                               const int64_t *h_offsets, void *d_out, size_t out_bytes, size_t *h_used)
{
    using namespace pm_rows;
    PM_CTX(ctx);
    PM_ARG(d_recs && d_steps && cap >= 0 && (cap & 7) == 0 && ((uintptr_t)d_steps & 7) == 0 && row0 >= 0);
    PM_ARG(nrows >= 1 && nrows <= kMaxRows && h_chains && nchains >= 1 && nchains <= kMaxChains && h_counts && h_offsets);
    PM_ARG(d_block && ((uintptr_t)d_block & 7) == 0 && d_out && ((uintptr_t)d_out & 7) == 0 && h_used);
    RowPk K;
    memset(&K, 0, sizeof(K));
    K.recs = d_recs;
    K.steps = d_steps;
    K.cap = cap;
    K.row0 = row0;
    K.nrows = nrows;
    K.nchains = nchains;
    const int tune = ctx->tune.bitscan_tile_words;
    K.tile_words = tune > 0 ? std::min(tune, kLanes) : kLanes;
    for (int c = 0; c < nchains; ++c) {
        const pm_rows_scan_chain &q = h_chains[c];
        PM_ARG(q.codec_kind >= -1 && q.codec_kind <= 1);
        PM_ARG(q.frames == 0 || (q.frames == 1 && q.codec_kind == 0));
        PM_ARG(q.packets == 0 || (q.packets == 1 && q.codec_kind == 1));
        PM_ARG(q.addrs == 0 || q.addrs == 1);
        // a chain with a codec goes this way by the table of its kind and the checkpoints
        PM_ARG(q.codec_kind < 0 || (q.addrs == 1 && (q.codec_kind == 0 ? q.frames : q.packets) == 1));
        K.kind[c] = (int8_t)q.codec_kind;
        K.frames[c] = (int8_t)q.frames;
        K.packets[c] = (int8_t)q.packets;
        K.addrs[c] = (int8_t)q.addrs;
        K.tol[c] = (int8_t)std::max(-1, std::min(33, q.sync_tol));
        K.pkopt[c] = (uint8_t)(q.il2p_crc != 0);
        K.source[c] = h_sources ? h_sources[c] : c;
    }
    // the sums as pm_rows_scan made them from the same counts: the limits of the device's own table, and what the offsets must be
    Sums all = sums_zero();
    for (int r = 0; r < nrows; ++r) {
        const pm_rows_scan_chain &q = h_chains[(row0 + r) % nchains];
        const int64_t n = h_counts[r];
        PM_ARG(n >= 0 && n <= cap && n <= kMaxBytes && h_offsets[r] == all.off);
        all = sums_add(all, row_sums(q.codec_kind, q.frames, q.packets, n, K.tile_words, q.addrs));
        PM_ARG(all.tiles < (int64_t)1 << 30);
    }
    // these launches read the block: it must be memory of the device's
    {
        hipPointerAttribute_t attr;
        memset(&attr, 0, sizeof(attr));
        const hipError_t e = hipPointerGetAttributes(&attr, d_block);
        if (e != hipSuccess) (void)hipGetLastError();
        if (e != hipSuccess || (attr.type != hipMemoryTypeDevice && attr.type != hipMemoryTypeManaged))
            return pm_set_error(PM_ERR_ARG, "pm_rows_packets: d_block is not device memory (the launches read it)");
    }
    const size_t front = (size_t)pm_rpk::kHeadBytes + (size_t)pm_rpk::kEntryBytes * (size_t)nrows;
    *h_used = front;
    if (out_bytes < front) return pm_set_error(PM_ERR_CAPACITY, "pm_rows_packets: d_out holds %zu bytes, head and entries need %zu", out_bytes, front);
    const int64_t capacity = (int64_t)((out_bytes - front) / sizeof(pm_packet));
    const size_t info_bytes = ((size_t)nrows * sizeof(RowPkInfo) + 63) & ~(size_t)63;
    if (int rc = pm_scratch_reserve(ctx, info_bytes + (size_t)(all.events + all.places) * sizeof(pm_rpk::Accepted) + 64)) return rc;
    RowPkInfo *info = static_cast<RowPkInfo *>(ctx->d_scratch);
    pm_rpk::Accepted *acc = reinterpret_cast<pm_rpk::Accepted *>(static_cast<uint8_t *>(ctx->d_scratch) + info_bytes);
    uint8_t *out = static_cast<uint8_t *>(d_out);
    pm_rows_packets_head *head = reinterpret_cast<pm_rows_packets_head *>(out);
    pm_rows_packets_entry *entries = reinterpret_cast<pm_rows_packets_entry *>(out + pm_rpk::kHeadBytes);
    hipLaunchKernelGGL(rows_packets_walk_kernel, dim3((unsigned)pm_cdiv(nrows, kLanes)), dim3(kLanes), 0, ctx->stream, K, static_cast<const uint8_t *>(d_block), entries,
                       info, acc, all);
    hipLaunchKernelGGL(rows_packets_room_kernel, dim3(1), dim3(kLanes), 0, ctx->stream, nrows, head, entries, capacity);
    hipLaunchKernelGGL(rows_packets_build_kernel, dim3(kBuildWaves), dim3(64), 0, ctx->stream, K, static_cast<const uint8_t *>(d_block), out, info, acc);
    PM_HIP(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_stream_packets(pm_ctx *ctx, const pm_scan_job *h_jobs, int njobs, const int32_t *h_sources, const void *d_block, const int64_t *h_offsets,
                                 void *d_out, size_t out_bytes, size_t *h_used)
{
    PM_CTX(ctx);
    PM_ARG(h_jobs && njobs >= 1 && njobs <= kScanJobs && d_block && ((uintptr_t)d_block & 7) == 0 && h_offsets && d_out && ((uintptr_t)d_out & 7) == 0 && h_used);
    StreamPk K;
    memset(&K, 0, sizeof(K));
    K.njobs = njobs;
    // the parts as pm_stream_scan laid them out for the same jobs: what the offsets must be
    size_t at = 0;
    int64_t places = 0;
    for (int j = 0; j < njobs; ++j) {
        const pm_scan_job &q = h_jobs[j];
        PM_ARG(q.n >= 0 && q.n <= (int64_t)1 << 29 && q.codec_kind >= -1 && q.codec_kind <= 1 && !q.d_carry);
        PM_ARG(q.frames == (q.codec_kind == 0) && q.packets == (q.codec_kind == 1) && (q.addrs == 0 || q.addrs == 1));
        // a job with a codec goes this way by the table of its kind and the stream's addresses
        PM_ARG(q.codec_kind < 0 || (q.d_addr && ((uintptr_t)q.d_addr & 7) == 0));
        PM_ARG(h_offsets[j] == (int64_t)at);
        K.off[j] = (int64_t)at;
        K.addr[j] = q.d_addr;
        K.n[j] = (int32_t)q.n;
        K.acc0[j] = (int32_t)places;
        K.source[j] = h_sources ? h_sources[j] : j;
        K.kind[j] = (int8_t)q.codec_kind;
        K.tol[j] = (int8_t)std::max(-1, std::min(33, q.sync_tol));
        K.crc[j] = q.il2p_crc != 0;
        at += (size_t)pm_rows::scan_bytes(q.codec_kind, q.frames, q.packets, q.n) + (q.addrs ? (size_t)PM_SCAN_ADDR_BYTES(q.n) : 0);
        places += q.codec_kind == 0 ? q.n / 19 + 2 : q.codec_kind == 1 ? q.n / 64 + 2 : 0;
        PM_ARG(places < INT32_MAX);
    }
    // these launches read the block: it must be memory of the device's
    {
        hipPointerAttribute_t attr;
        memset(&attr, 0, sizeof(attr));
        const hipError_t e = hipPointerGetAttributes(&attr, d_block);
        if (e != hipSuccess) (void)hipGetLastError();
        if (e != hipSuccess || (attr.type != hipMemoryTypeDevice && attr.type != hipMemoryTypeManaged))
            return pm_set_error(PM_ERR_ARG, "pm_stream_packets: d_block is not device memory (the launches read it)");
    }
    const size_t front = (size_t)pm_rpk::kStreamHeadBytes + (size_t)pm_rpk::kEntryBytes * (size_t)njobs;
    *h_used = front;
    if (out_bytes < front) return pm_set_error(PM_ERR_CAPACITY, "pm_stream_packets: d_out holds %zu bytes, head and entries need %zu", out_bytes, front);
    const int64_t capacity = (int64_t)((out_bytes - front) & ~(size_t)7);
    const size_t notes_bytes = (sizeof(StreamPkNotes) + 63) & ~(size_t)63, acc_bytes = ((size_t)places * sizeof(pm_rpk::Accepted) + 63) & ~(size_t)63;
    if (int rc = pm_scratch_reserve(ctx, notes_bytes + acc_bytes + (size_t)places * sizeof(int64_t) + 64)) return rc;
    uint8_t *base = static_cast<uint8_t *>(ctx->d_scratch), *out = static_cast<uint8_t *>(d_out);
    StreamPkNotes *notes = reinterpret_cast<StreamPkNotes *>(base);
    pm_rpk::Accepted *acc = reinterpret_cast<pm_rpk::Accepted *>(base + notes_bytes);
    int64_t *recoff = reinterpret_cast<int64_t *>(base + notes_bytes + acc_bytes);
    const int btune = ctx->tune.bitscan_packet_waves;
    hipLaunchKernelGGL(stream_packets_walk_kernel, dim3(njobs), dim3(64), 0, ctx->stream, K, static_cast<const uint8_t *>(d_block), notes, acc, recoff);
    hipLaunchKernelGGL(stream_packets_room_kernel, dim3(1), dim3(64), 0, ctx->stream, njobs, notes, reinterpret_cast<uint64_t *>(out), capacity);
    hipLaunchKernelGGL(stream_packets_build_kernel, dim3(btune > 0 ? std::min(btune, kBuildWaves) : kBuildWaves), dim3(64), 0, ctx->stream, K,
                       static_cast<const uint8_t *>(d_block), out + front, notes, acc, recoff);
    PM_HIP(hipGetLastError());
    return PM_OK;
}
