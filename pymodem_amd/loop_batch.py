"""Many recordings through carrier-loop chains at once (pm_lbatch, csrc/pm_loopbatch.hip).

A BPSK / MPSK / QPSK / AFSK-PLL chain spends its time in one sequential carrier loop (psk.py:173-189, psk.py:734-747,
psk.py:434-467, afsk_pll.py:153-165): one GPU lane steps it slower than one host core does, and nothing makes a single loop faster
(DESIGN.md 4.5).  The GPU's answer is width: a loop needs one lane, so the loops of hundreds of recordings x chains run in the time
of one.  `LoopBatch` is the object that puts them side by side: R recordings x the C chains of a group that shares its front end
(band-pass, AGC, Hilbert pair; the chains of configs/qpsk_2400.json differ in carrier_freq only) go through ONE engine run, in time
chunks, every loop of every recording in one launch per chunk.  `process_recordings_device` is chain_execute.process_chains_device
for a list of recordings: engine -> all slicers in batches -> LFSR + codec per recording.

Results are those of process_chain on every recording, bit for bit (tests/test_gpu_loopbatch.py).
"""
import ctypes
import threading

import numpy as np

from . import _native as N
from ._native import check, lib
from .data_classes import SignBits
from .device import Context, DeviceBuffer
from .modems import AFSKPLLModem, BPSKModem, MPSKModem, QPSKModem

_MODEM_ID = {BPSKModem: N.MODEM_BPSK, MPSKModem: N.MODEM_MPSK, AFSKPLLModem: N.MODEM_AFSK_PLL, QPSKModem: N.MODEM_QPSK}


def _output_taps(modem):
    return modem.output_lpf if isinstance(modem, AFSKPLLModem) else modem.rrc_taps


def group_key(modem):
    """Chains whose modems have equal keys can share one engine run: same kind, same front end, same output filter, same tables;
    what is left to differ is the loop (carrier_freq, loop filter, PI constants)."""
    if type(modem) not in _MODEM_ID:
        return None
    fe = modem.front_end_key() if hasattr(modem, "front_end_key") else (
        "qpsk", float(modem.sample_rate), modem.input_bpf.tobytes(),
        (modem.AGC.attack_rate, modem.AGC.decay_rate, modem.AGC.sustain_time, modem.AGC.target_amplitude))
    extra = modem.phase_error_table.tobytes() if isinstance(modem, MPSKModem) else b""
    return (type(modem).__name__, fe, _output_taps(modem).tobytes(), np.asarray(modem.wavetable).tobytes(), extra)


class LoopBatch:
    """One pm_lbatch engine: `recordings` recordings (at most) x the chains of `modems` per run.  `modems`: the modem objects of ONE
    recording's chains (equal group_key); their loop parameters and initial states are what every recording starts from."""

    def __init__(self, modems, recordings, ctx=None, chunk=0):
        keys = {group_key(m) for m in modems}
        if len(keys) != 1 or None in keys:
            raise ValueError("LoopBatch: the chains of a run must be carrier-loop modems that share front end, output filter and tables")
        self.ctx = ctx or Context.default()
        self.recordings, self.chains = int(recordings), len(modems)
        lead = modems[0]
        self.kind = type(lead)
        self.quadrature = isinstance(lead, (MPSKModem, QPSKModem))
        d = N.LBatchDesc()
        keep = []

        def vec(x, dtype=np.float64):
            a = np.ascontiguousarray(x, dtype=dtype)
            keep.append(a)
            return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double if dtype == np.float64 else ctypes.c_int32)), len(a)
        d.modem, d.recordings, d.chains, d.chunk = _MODEM_ID[self.kind], self.recordings, self.chains, int(chunk)
        d.input_fir, d.n_input_fir = vec(lead.input_bpf)
        if isinstance(lead, MPSKModem):
            d.hilbert, d.n_hilbert = vec(lead.hilbert_taps)
            d.hilbert_delay = lead.hilbert_delay
            d.pd_table = vec(lead.phase_error_table.reshape(-1), np.int32)[0]
        d.output_fir, d.n_output_fir = vec(_output_taps(lead))
        a = lead.AGC
        d.agc = N.AGCParams(a.attack_rate, a.decay_rate, a.sustain_time, a.sample_rate, a.target_amplitude)
        loops = (N.Loop * self.chains)()
        for c, m in enumerate(modems):
            ctypes.memmove(ctypes.byref(loops[c]), m._loop0, ctypes.sizeof(N.Loop))
        d.loops = loops
        d.wavetable = vec(lead.wavetable)[0]
        self._h = ctypes.c_void_p()
        check(lib().pm_lbatch_create(self.ctx.handle, ctypes.byref(d), ctypes.byref(self._h)))
        self._front = None

    def geometry(self, n):
        """(samples per demodulated stream, final-filter outputs per chunk, chunks) for recordings of n samples."""
        a, b, c = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        check(lib().pm_lbatch_geometry(self._h, int(n), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value

    @property
    def front(self):
        """The engine's own context (band-pass, AGC, Hilbert pair of the next chunk) as a borrowed Context, for profile_read()."""
        if self._front is None:
            f = Context.__new__(Context)
            f._h, f.device = ctypes.c_void_p(lib().pm_lbatch_front_ctx(self._h)), self.ctx.device
            f.close = lambda: None                          # the engine owns it
            self._front = f
        return self._front

    @property
    def tail(self):
        """The engine's third context (the matched filters of chunk t - 1 beside the loops of chunk t), borrowed, for profile_read()."""
        if getattr(self, "_tail", None) is None:
            self._tail = Context.borrowed(lib().pm_lbatch_tail_ctx(self._h), self.ctx.device)
        return self._tail

    @property
    def loop(self):
        """The engine's loop context when the carrier loops have compute units of their own (csrc/pm_loopbatch.hip), borrowed, for
        profile_read(); None when they run on the caller's context."""
        if getattr(self, "_loop", None) is None:
            h = lib().pm_lbatch_loop_ctx(self._h)
            self._loop = Context.borrowed(h, self.ctx.device) if h else False
        return self._loop or None

    @property
    def slicing(self):
        """The engine's slicer context (a sliced run's row slicers, beside the matched filters of the next chunk), borrowed, for profile_read()."""
        if getattr(self, "_slicing", None) is None:
            self._slicing = Context.borrowed(lib().pm_lbatch_slice_ctx(self._h), self.ctx.device)
        return self._slicing

    def _bits(self, r, nout, slot):
        stride = ((nout + 63) // 64 + 1 + 7) // 8 * 8
        streams = r * self.chains
        bits_i = self.ctx.scratch(("lbatch", id(self), slot, "i"), streams * stride, np.uint64)
        bits_q = self.ctx.scratch(("lbatch", id(self), slot, "q"), streams * stride, np.uint64) if self.quadrature else None
        return stride, bits_i, bits_q

    def reserve(self, recordings, n, slot=0):
        """Allocate the bitmap set of `slot` for `recordings` recordings of n samples now (a warm-up's job: the first run of a size
        would otherwise do it, with the allocator's wait inside the run)."""
        nout = self.geometry(n)[0]
        if nout >= 1:
            self._bits(int(recordings), nout, slot)

    def run(self, audios, slot=0):
        """audios: DeviceBuffers of int16 recordings of equal length (they may be the same buffer).  Enqueues the whole run and
        returns [[SignBits of chain 0, chain 1, ...] per recording]; the bitmaps are complete when this context's stream gets there
        (slice on it, or behind an event recorded on it).  `slot`: which of the caller's bitmap sets to write (a set stays untouched
        until the same slot is used again)."""
        r = len(audios)
        if not 1 <= r <= self.recordings:
            raise ValueError(f"LoopBatch.run: {r} recordings, the engine was made for {self.recordings}")
        n = audios[0].n
        for a in audios:
            if not isinstance(a, DeviceBuffer) or a.dtype != np.dtype(np.int16) or a.n != n:
                raise ValueError("LoopBatch.run: recordings must be int16 DeviceBuffers of equal length")
        nout = self.geometry(n)[0]
        if nout < 1:
            raise ValueError(f"input of {n} samples is shorter than the filters of the chain")
        stride, bits_i, bits_q = self._bits(r, nout, slot)
        ptrs = (ctypes.c_void_p * r)(*[a.ptr.value for a in audios])
        got = ctypes.c_int64()
        check(lib().pm_lbatch_run(self._h, ptrs, r, n, bits_i.ptr, bits_q.ptr if bits_q is not None else None, stride, ctypes.byref(got)))
        out = []
        for k in range(r):
            row = []
            for c in range(self.chains):
                s = k * self.chains + c
                row.append(SignBits(bits_i.view(s * stride, stride), bits_q.view(s * stride, stride) if bits_q is not None else None, got.value))
            out.append(row)
        return out

    def _sliced_room(self, r, nout, slicers, slot):
        # room per stream: 1.5 x the nominal byte count (a clock pulled by its crossings runs at most twice nominal; real streams stay
        # within a few percent); a row that needs more says so in its record and the caller slices that run the other way
        nominal = max(nout * sl.bits_per_symbol / (8.0 * sl.samples_per_symbol) for sl in slicers)
        cap = (int(nominal * 1.5) + 64 + 7) // 8 * 8
        rows = r * self.chains
        data = self.ctx.scratch(("lbatch", id(self), slot, "sliced-data"), rows * cap, np.uint8)
        steps = self.ctx.scratch(("lbatch", id(self), slot, "sliced-steps"), rows * cap, np.uint16)
        recs = self.ctx.scratch(("lbatch", id(self), slot, "sliced-recs"), rows * ctypes.sizeof(N.RowSliceRec), np.uint8)
        return cap, rows, data, steps, recs

    def reserve_sliced(self, recordings, n, slicers, slot=0):
        """reserve() for run_sliced(): the rows' output blocks for `recordings` recordings of n samples, now."""
        nout = self.geometry(n)[0]
        if nout >= 1:
            self._sliced_room(int(recordings), nout, slicers, slot)

    def _marks_for(self, slot, chunks):
        """the slot's marks object (pm_lbatch_marks), made for at least `chunks` chunks: it lives as long as the slot's output blocks do"""
        held = self.__dict__.setdefault("_marks", {})
        hit = held.get(slot)
        if hit is None or hit[1] < chunks:
            if hit is not None:
                check(lib().pm_lbatch_marks_destroy(hit[0]))
                del held[slot]
            h = ctypes.c_void_p()
            room = max(int(chunks), 1)
            check(lib().pm_lbatch_marks_create(self._h, room, ctypes.byref(h)))
            hit = held[slot] = (h, room)
        return hit[0]

    def run_sliced(self, audios, slicers, slot=0, marks=False, _cap=None):
        """run() with the slicers inside the engine (pm_lbatch_run_sliced): every stream is sliced chunk by chunk behind its matched
        filter by a lane of its own, no sign bitmap of a whole recording is kept and nothing is left to slice when the run ends.
        `slicers`: one slicer object per chain -- its parameters; every stream starts from the just-tuned state (slicer.py:49-56).
        -> SlicedRun (complete when this context's stream gets there).
        marks=True (pm_lbatch_run_sliced_marked): the run also leaves, behind the slicers of every chunk, a mark -- every row's count as it
        stands, the OR of the rows' flags and an event -- and the SlicedRun carries them (run.marks: RunMarks, run.chunks), so that its rows
        can be taken in pieces while it runs (RowPieces.fetch(mark=t)).  The run itself is the same run.  _cap: the rows' room in bytes in
        place of the engine's own figure (tests make a row outgrow it)."""
        r = len(audios)
        if not 1 <= r <= self.recordings:
            raise ValueError(f"LoopBatch.run_sliced: {r} recordings, the engine was made for {self.recordings}")
        if len(slicers) != self.chains:
            raise ValueError("LoopBatch.run_sliced: one slicer per chain")
        n = audios[0].n
        for a in audios:
            if not isinstance(a, DeviceBuffer) or a.dtype != np.dtype(np.int16) or a.n != n:
                raise ValueError("LoopBatch.run_sliced: recordings must be int16 DeviceBuffers of equal length")
        nout = self.geometry(n)[0]
        if nout < 1:
            raise ValueError(f"input of {n} samples is shorter than the filters of the chain")
        params = (N.SlicerParams * self.chains)(*[sl._params() for sl in slicers])
        cap, rows, data, steps, recs = self._sliced_room(r, nout, slicers, slot)
        if _cap is not None:
            if not (8 <= int(_cap) <= cap and int(_cap) % 8 == 0):
                raise ValueError("LoopBatch.run_sliced: _cap is a multiple of 8 within the rows' room")
            cap = int(_cap)
        ptrs = (ctypes.c_void_p * r)(*[a.ptr.value for a in audios])
        got = ctypes.c_int64()
        if marks:
            handle, chunks = self._marks_for(slot, self.geometry(n)[2]), ctypes.c_int64()
            check(lib().pm_lbatch_run_sliced_marked(self._h, ptrs, r, n, params, self.chains, data.ptr, steps.ptr, cap, recs.ptr, ctypes.byref(got),
                                                    handle, ctypes.byref(chunks)))
            return SlicedRun(self.ctx, data, steps, recs, cap, rows, got.value, marks=RunMarks(handle, rows, chunks.value), engine=self)
        check(lib().pm_lbatch_run_sliced(self._h, ptrs, r, n, params, self.chains, data.ptr, steps.ptr, cap, recs.ptr, ctypes.byref(got)))
        return SlicedRun(self.ctx, data, steps, recs, cap, rows, got.value)

    def close(self):
        if self._h:
            for handle, _ in self.__dict__.pop("_marks", {}).values():
                lib().pm_lbatch_marks_destroy(handle)        # (in front of the engine: waits for the marks still in flight)
            lib().pm_lbatch_destroy(self._h)                 # waits for both of the engine's streams
            self._h = ctypes.c_void_p()
            pool = self.ctx.__dict__.get("_pool", {})
            for tag in [t for t in pool if isinstance(t, tuple) and t[:2] == ("lbatch", id(self))]:
                pool.pop(tag).free()                         # the bitmap sets
            self.ctx.__dict__.get("_pool_views", {}).clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def next_mark(last, newest, chunks, k):
    """Which mark the driver of process_recordings_device(beside=k) takes next, or None: `last` the mark it took last (-1: none yet), `newest`
    the newest mark whose event has completed (pm_lbatch_marks_ready; -1: none), `chunks` the run's chunk count.  Due are the marks t with
    (t + 1) % k == 0; they are taken in order, each at most once; once the run's LAST mark has completed nothing more is due -- the rows are
    all there and go in one final piece."""
    if chunks < 1 or newest >= chunks - 1:
        return None
    t = (last + 1 + k) // k * k - 1                          # the first t > last with (t + 1) % k == 0
    return t if t < chunks else None


def piece_cut(avail, taken, final=False):
    """pm_rows_scan_pieces' rule for the next piece of rows that have `avail` bytes to give (min(upto, count, cap)) and have given `taken`:
    n = avail - taken, rounded down to a multiple of 8 unless final, never below 0; nothing behind a final piece (taken % 8 != 0)"""
    taken = np.asarray(taken, dtype=np.int64)
    n = np.asarray(avail, dtype=np.int64) - taken
    if not final:
        n = n // 8 * 8                                       # (floor: rounds down below zero too)
    return np.ascontiguousarray(np.where(taken % 8 != 0, 0, np.maximum(n, 0)), dtype=np.int64)


class RunMarks:
    """The marks of one marked run (pm_lbatch_marks_*; the engine owns the object): chunks marks of `rows` int64 each.  Every reader refuses
    a t outside [0, chunks) -- so does the library -- and none of them touches the run's records."""

    def __init__(self, handle, rows, chunks):
        self._h, self.rows, self.chunks = handle, int(rows), int(chunks)

    def ready(self):
        """the newest mark whose event has completed, -1 if none: no waiting"""
        t = ctypes.c_int64()
        check(lib().pm_lbatch_marks_ready(self._h, ctypes.byref(t)))
        return t.value

    def wait(self, t, poll_us=200):
        """host wait for mark t without spinning; its host copies may be read afterwards"""
        check(lib().pm_lbatch_marks_wait(self._h, int(t), int(poll_us)))

    def wait_on(self, t, ctx):
        """what is submitted to ctx from now on waits, on the GPU, for mark t"""
        check(lib().pm_lbatch_marks_wait_on(self._h, int(t), ctx.handle))

    def _view(self, t):
        d, h, f = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        check(lib().pm_lbatch_marks_view(self._h, int(t), ctypes.byref(d), ctypes.byref(h), ctypes.byref(f)))
        return d.value, h.value, f.value

    def d_upto(self, t, row0=0):
        """device address of mark t's int64 of row row0"""
        return self._view(t)[0] + 8 * int(row0)

    def h_upto(self, t):
        """mark t's `rows` int64 in page-locked host memory, as an array over that memory (read it behind wait(t))"""
        at = self._view(t)[1]
        return np.ctypeslib.as_array((ctypes.c_int64 * self.rows).from_address(at))

    def flags(self, t):
        """the OR of the rows' flags at mark t (read it behind wait(t))"""
        return int(ctypes.c_int32.from_address(self._view(t)[2]).value)


class SlicedRun:
    """What a sliced engine run left in device memory: per stream (row = recording * chains + chain) its data bytes, address steps and
    record.  records() and fetch() want the run complete (synchronise the context it ran on first).  A run made with marks=True carries them
    (marks: RunMarks, chunks): RowPieces.fetch(mark=t) takes its rows while it runs."""

    def __init__(self, ctx, data, steps, recs, cap, rows, nout, marks=None, engine=None):
        self.ctx, self.data, self.steps, self.recs, self.cap, self.rows, self.nout = ctx, data, steps, recs, cap, rows, nout
        self.marks, self.chunks = marks, (marks.chunks if marks is not None else None)
        self._engine = engine                                # (the marks are the engine's: it lives as long as they are read)
        self._records = None
        self.copied = 0                                      # bytes that fetch() and fetch_scanned() have brought to the host (diagnosis)
        self._copied_lock = threading.Lock()

    def records(self, copy_ctx=None):
        if self._records is None:
            self._records = self.recs.download(self.rows * ctypes.sizeof(N.RowSliceRec), ctx=copy_ctx).view(N.rowslice_dtype())
        return self._records

    def ok(self):
        """False if a row overflowed its room or took an address step beyond 16 bits: slice that run with slice_batch instead."""
        return not self.records()["flags"].any()

    def state_into(self, row, slicer):
        """The end state of the row's slicer, as slice() would have left it in the object."""
        rec, st = self.records()[row], slicer._state
        st.phase_clock, st.last_i_negative, st.last_q_negative = float(rec["clk"]), int(rec["li_neg"]), int(rec["lq_neg"])
        st.working_byte, st.working_bits, st.state_register, st.streamaddress = int(rec["wbyte"]), int(rec["wbits"]), int(rec["sreg"]), int(rec["seen"])
        slicer.phase_clock, slicer.streamaddress = st.phase_clock, st.streamaddress

    def fetch(self, row0, nrows, copy_ctx=None, tag=None):
        """-> [AddressedArray of row row0, row0 + 1, ...]: one gather launch and ONE copy to the host for the lot (on copy_ctx's stream)."""
        from .data_classes import AddressedArray
        ctx = copy_ctx or self.ctx
        recs = self.records()[row0:row0 + nrows]
        counts = np.minimum(recs["count"], self.cap)
        sizes = (2 * counts + 7) // 8 * 8 + (counts + 7) // 8 * 8
        offs = np.concatenate(([0], np.cumsum(sizes)))
        used = int(offs[-1])
        out = []
        if used:
            # (host blocks in 8 MB size classes: streams run within a few percent of their nominal counts, so the groups of a run ask
            # for the same class and the page-locked blocks go round; the worst case, 1.5 x that, would be filled and pinned for nothing)
            room = (used + (8 << 20) - 1) // (8 << 20) * (8 << 20)
            block = ctx.scratch((tag if tag is not None else ("sliced-run", id(self)), "dense"), room, np.uint8)
            check(lib().pm_rows_gather(ctx.handle, self.recs.ptr, self.data.ptr, self.steps.ptr, self.cap, row0, nrows, block.ptr, block.n))
            host = block.download(used, recycle=True, ctx=ctx, room=room)
            with self._copied_lock:
                self.copied += used
        for k in range(nrows):
            c, o = int(counts[k]), int(offs[k])
            if c == 0:
                out.append(AddressedArray(np.zeros(0, np.uint8), np.zeros(0, np.int64)))
                continue
            sw = (2 * c + 7) // 8 * 8
            out.append(AddressedArray.from_steps(host[o + sw:o + sw + c], host[o:o + 2 * c].view(np.uint16), int(recs["first_addr"][k])))
        return out

    def fetch_scanned(self, row0, nrows, chains, frames, packets, copy_ctx=None, tag=None, addrs=False):
        """fetch() with the bitstream stage on the device in front of the copy (pm_rows_scan): `chains` are the run's chains [name, modem,
        slicer, stream, codec], row k a stream of chain k % len(chains) that starts from that chain's LFSR register; frames / packets: the
        AX.25 chains' frame tables / the IL2P chains' packet tables too; addrs: every row's address checkpoints at the end of its part
        (pm_rows_scan_chain.addrs).  -> per row (address steps, first address, n, the row's scan part
        -- record, list, descrambled bytes, tables -- as views of one host block): one scan and ONE copy to the host for the lot."""
        ctx = copy_ctx or self.ctx
        recs = self.records()[row0:row0 + nrows]
        counts = np.ascontiguousarray(np.minimum(recs["count"], self.cap), dtype=np.int64)
        nchains = len(chains)
        desc = _scan_desc(chains, frames, packets, addrs)
        of = [desc[(row0 + k) % nchains] for k in range(nrows)]
        parts = [N.scan_part_bytes(d.codec_kind, d.frames, d.packets, int(c), d.addrs) for d, c in zip(of, counts)]
        used = int(sum(N.rows_scan_steps_bytes(int(c)) for c in counts) + sum(parts))
        # (the same 8 MB size classes as fetch(): the groups of a run ask for the same class and the page-locked blocks go round)
        room = (used + (8 << 20) - 1) // (8 << 20) * (8 << 20)
        block = ctx.scratch((tag if tag is not None else ("sliced-run", id(self)), "scanned"), room, np.uint8)
        offs, need = (ctypes.c_int64 * nrows)(), ctypes.c_size_t()
        check(lib().pm_rows_scan(ctx.handle, self.recs.ptr, self.data.ptr, self.steps.ptr, self.cap, row0, nrows, desc, nchains,
                                 counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), block.ptr, block.n, offs, ctypes.byref(need)))
        assert need.value == used, "pm_rows_scan and _native.scan_part_bytes size a row alike"
        host = block.download(used, recycle=True, ctx=ctx, room=room)
        with self._copied_lock:
            self.copied += used
        out = []
        for k in range(nrows):
            c, o = int(counts[k]), int(offs[k])
            sw = N.rows_scan_steps_bytes(c)
            out.append((host[o:o + 2 * c].view(np.uint16), int(recs["first_addr"][k]), c, host[o + sw:o + sw + parts[k]]))
        return out

    def fetch_packets(self, row0, nrows, chains, copy_ctx=None, tag=None, sources=None, desc=None):
        """fetch_scanned() with the codecs' work on the device as well (pm_rows_scan into a DEVICE block, pm_rows_packets behind it): the rows
        of whole recordings -- row0 and nrows multiples of len(chains) -- with frames, packets and addrs on.  sources: what goes into
        pm_packet.source_decoder per chain (None: 0, as a codec without chain ids stamps it).
        -> (entries, packet rows, handed): the call's pm_rows_packets_entry per row and its pm_packet rows as host arrays -- a FINISHED row's
        packets are rows[first:first + packets], and a recording's rows lie chain after chain -- and, for every recording with a row that is
        not FINISHED, handed[index of its first row in the call] = what fetch_scanned returns for its rows, for _host_rows_scanned.
        At most two copies to the host, head and entries, then exactly the packet rows, and one more per handed recording: its
        consecutive parts of the scan block.  desc: the chains' pm_rows_scan_chain made earlier (_scan_desc with frames, packets and addrs
        on), for a caller whose chain objects move on while the groups of a run are fetched."""
        ctx = copy_ctx or self.ctx
        nchains = len(chains)
        assert row0 % nchains == 0 and nrows % nchains == 0, "whole recordings"
        recs = self.records()[row0:row0 + nrows]
        counts = np.ascontiguousarray(np.minimum(recs["count"], self.cap), dtype=np.int64)
        desc = _scan_desc(chains, True, True, True) if desc is None else desc
        of = [desc[k % nchains] for k in range(nrows)]
        parts = [N.scan_part_bytes(d.codec_kind, d.frames, d.packets, int(c), d.addrs) for d, c in zip(of, counts)]
        sizes = [N.rows_scan_steps_bytes(int(c)) + p for c, p in zip(counts, parts)]
        used = int(sum(sizes))
        key = tag if tag is not None else ("sliced-run", id(self))
        room = (used + (8 << 20) - 1) // (8 << 20) * (8 << 20)
        block = ctx.scratch((key, "scanned"), room, np.uint8)
        offs, need = (ctypes.c_int64 * nrows)(), ctypes.c_size_t()
        h_counts = counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
        check(lib().pm_rows_scan(ctx.handle, self.recs.ptr, self.data.ptr, self.steps.ptr, self.cap, row0, nrows, desc, nchains, h_counts, block.ptr, block.n,
                                 offs, ctypes.byref(need)))
        assert need.value == used, "pm_rows_scan and _native.scan_part_bytes size a row alike"
        # (room for two packets a row and a few more: a row that finds none goes the existing way, whatever the room)
        front, capacity = N.rows_packets_bytes(nrows), 2 * nrows + 64
        out = ctx.scratch((key, "packets"), N.rows_packets_bytes(nrows, capacity), np.uint8)
        h_sources = (ctypes.c_int32 * nchains)(*([0] * nchains if sources is None else [int(v) for v in sources]))
        check(lib().pm_rows_packets(ctx.handle, self.recs.ptr, self.steps.ptr, self.cap, row0, nrows, desc, nchains, h_sources, h_counts, block.ptr, offs,
                                    out.ptr, out.n, ctypes.byref(need)))
        lead = out.download(front, ctx=ctx)
        head = lead[:N.ROWS_PACKETS_HEAD_BYTES].view(N.rows_packets_head_dtype())[0]
        entries = lead[N.ROWS_PACKETS_HEAD_BYTES:].view(N.rows_packets_entry_dtype())
        total = int(head["packets"])
        rows = out.view(front, total * N.packet_dtype().itemsize).download(ctx=ctx).view(N.packet_dtype()) if total else np.zeros(0, dtype=N.packet_dtype())
        copied = front + rows.nbytes
        handed = {}
        for k in range(0, nrows, nchains):
            if (entries["status"][k:k + nchains] == 0).all():
                continue
            lo = int(offs[k])
            host = block.view(lo, sum(sizes[k:k + nchains])).download(ctx=ctx)
            copied += host.nbytes
            mine = []
            for j in range(k, k + nchains):
                c, o = int(counts[j]), int(offs[j]) - lo
                sw = N.rows_scan_steps_bytes(c)
                mine.append((host[o:o + 2 * c].view(np.uint16), int(recs["first_addr"][j]), c, host[o + sw:o + sw + parts[j]]))
            handed[k] = mine
        with self._copied_lock:
            self.copied += copied
        return entries, rows, handed

    def pieces(self, chains, frames=False, packets=False, addrs=False):
        """The rows of this run scanned piece by piece (pm_rows_scan_pieces), a device carry per row: -> RowPieces.  `chains`, frames, packets
        and addrs as for fetch_scanned()."""
        return RowPieces(self, chains, frames, packets, addrs)


class RowPieces:
    """A sliced run's rows taken in pieces with the bitstream stage on the device: owns the rows' carries (pm_rows_carry, 64 bytes a row, started
    with pm_rows_carry_start in front of a row's first piece, on the stream that takes it) and the host's shadow of `taken` per row.  The
    pieces of a row must be fetched through one context (copy_ctx), one after the other; every piece is to be decoded (chain_execute.
    _host_rows_pieces) before the row's next one is fetched, and the rows that it names are to be seeded again (seed()).  seeds, ordinary: how
    often a carry was seeded from a codec's registers behind a bail, and how many pieces went the ordinary way."""

    def __init__(self, run, chains, frames=False, packets=False, addrs=False):
        self.run, self.chains, self.frames, self.packets, self.addrs = run, chains, bool(frames), bool(packets), bool(addrs)
        nchains = len(chains)
        self.desc = (N.RowsScanChain * nchains)()
        for d, ch in zip(self.desc, chains):
            lfsr, codec = ch[3], ch[4]
            d.lfsr_poly, d.lfsr_state, d.lfsr_invert = lfsr.polynomial, lfsr.shift_register, int(bool(lfsr.invert))
            d.codec_kind, d.sync_tol = int(codec._kind), int(codec.sync_tolerance)
            d.frames, d.packets = int(self.frames and codec._kind == 0), int(self.packets and codec._kind == 1)
            d.il2p_crc, d.il2p_disable_rs, d.il2p_min_dist = int(codec.collect_trailing_crc), int(codec.disable_rs), int(codec.min_distance)
            d.addrs = int(self.addrs)
        self.carries = run.ctx.empty(run.rows * ctypes.sizeof(N.RowsCarry), np.uint8)
        self.taken = np.zeros(run.rows, dtype=np.int64)      # the host's shadow of pm_rows_carry.taken
        self.begun = np.zeros(run.rows, dtype=bool)
        self.last_from = np.zeros(run.rows, dtype=np.int64)  # where each row's last piece began
        self.last_before = np.zeros(run.rows, dtype=np.int64)    # its addr_before
        self.at_mark = np.zeros(run.rows, dtype=bool)        # and whether it was taken at a mark (raw() then copies it directly)
        self.seeds = self.ordinary = 0
        self._lock = threading.Lock()

    def piece_bytes(self, row0, nrows, upto=None, final=False, mark=None):
        """n of the next piece of every row, by pm_rows_scan_pieces' rule, from the records and the shadow of `taken` -- or, with `mark`, from
        the mark's host copy alone (min(count, cap) as it stood at the mark: wait for the mark first), with no look at the records: the run
        may still be going, and records() would cache what it found for good"""
        taken = self.taken[row0:row0 + nrows]
        if mark is not None:
            assert upto is None, "a piece at a mark goes up to the mark"
            return piece_cut(np.minimum(self.run.marks.h_upto(mark)[row0:row0 + nrows], self.run.cap), taken, final)
        recs = self.run.records()[row0:row0 + nrows]
        avail = np.clip(recs["count"], 0, self.run.cap)
        if upto is not None:
            avail = np.minimum(avail, np.asarray(upto, dtype=np.int64))
        return piece_cut(avail, taken, final)

    def fetch(self, row0, nrows, upto=None, final=False, copy_ctx=None, tag=None, mark=None):
        """The next piece of rows row0 .. row0 + nrows - 1: up to `upto` bytes of each row (an int64 per row, None: the records' counts), cut at
        a multiple of 8 unless `final`.  -> per row (the piece's address steps, addr_before, n, the piece's scan part with its carry piece) as
        views of one host block: the upload of `upto`, one pm_rows_scan_pieces and ONE copy to the host for the lot.
        mark=t (a run made with marks=True, which may still be going): up to what every row had when mark t was made.  The fetching context
        waits for the mark on the GPU, `upto` is the mark's own device copy -- nothing is uploaded -- and the sizes come from its host copy, read
        behind a relaxed host wait; the run's records are not touched."""
        run = self.run
        ctx = copy_ctx or run.ctx
        nchains = len(self.chains)
        if mark is not None:
            if run.marks is None or upto is not None:
                raise ValueError("RowPieces.fetch: mark= wants a run made with marks=True and no upto")
            run.marks.wait_on(mark, ctx)                     # in front of everything this call enqueues, the carries' start included
            run.marks.wait(mark)
        if not self.begun[row0:row0 + nrows].all():
            check(lib().pm_rows_carry_start(ctx.handle, self.carries.ptr, row0, nrows, self.desc, nchains))
            self.begun[row0:row0 + nrows] = True
        counts = self.piece_bytes(row0, nrows, upto, final, mark)
        key = tag if tag is not None else ("sliced-run", id(run))
        d_upto = None
        if mark is not None:
            d_upto = ctypes.c_void_p(run.marks.d_upto(mark, row0))
        elif upto is not None:
            h_upto = np.ascontiguousarray(upto, dtype=np.int64)
            assert len(h_upto) == nrows
            buf = ctx.scratch((key, "upto"), nrows, np.int64)
            check(lib().pm_h2d(ctx.handle, buf.ptr, h_upto.ctypes.data_as(ctypes.c_void_p), h_upto.nbytes))
            d_upto = buf.ptr
        of = [self.desc[(row0 + k) % nchains] for k in range(nrows)]
        sizes = [N.rows_piece_part_bytes(d.codec_kind, d.frames, d.packets, int(c), d.addrs) for d, c in zip(of, counts)]
        used = int(sum(sizes))
        # (the same 8 MB size classes as fetch_scanned())
        room = (used + (8 << 20) - 1) // (8 << 20) * (8 << 20)
        block = ctx.scratch((key, "pieces"), room, np.uint8)
        offs, need = (ctypes.c_int64 * nrows)(), ctypes.c_size_t()
        check(lib().pm_rows_scan_pieces(ctx.handle, run.recs.ptr, run.data.ptr, run.steps.ptr, run.cap, row0, nrows, self.desc, nchains, self.carries.ptr,
                                        d_upto, int(bool(final)), counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                        block.ptr, block.n, offs, ctypes.byref(need)))
        assert need.value == used, "pm_rows_scan_pieces and _native.rows_piece_part_bytes size a piece alike"
        host = block.download(used, recycle=True, ctx=ctx, room=room)
        with run._copied_lock:
            run.copied += used
        self.last_from[row0:row0 + nrows] = self.taken[row0:row0 + nrows]
        self.taken[row0:row0 + nrows] += counts
        self.at_mark[row0:row0 + nrows] = mark is not None
        out = []
        for k in range(nrows):
            c, o = int(counts[k]), int(offs[k])
            sw, end = N.rows_scan_steps_bytes(c), o + sizes[k]
            before = int(host[end - 8:end].view(np.int64)[0])
            self.last_before[row0 + k] = before
            out.append((host[o:o + 2 * c].view(np.uint16), before, c, host[o + sw:end - 8]))
        return out

    def raw(self, row, copy_ctx=None, tag=None):
        """the slicer bytes of the row's last piece, for a piece that goes the ordinary way (SlicedRun.fetch brings the row).  A piece that was
        taken at a mark is copied directly -- bytes [last_from, taken) of the row and their steps, the addresses from the piece's addr_before,
        whose first step counts: the run may still be going, and SlicedRun.fetch (records, pm_rows_gather over the moving counts) is for a
        run that is complete.  On the context that fetched the piece: it has waited for the mark."""
        from .data_classes import AddressedArray
        a, b = int(self.last_from[row]), int(self.taken[row])
        if self.at_mark[row]:
            run, ctx = self.run, copy_ctx or self.run.ctx
            if b <= a:
                return AddressedArray(np.zeros(0, np.uint8), np.zeros(0, np.int64))
            data = run.data.view(row * run.cap + a, b - a).download(ctx=ctx)
            steps = run.steps.view(row * run.cap + a, b - a).download(ctx=ctx)
            return AddressedArray(np.ascontiguousarray(data), int(self.last_before[row]) + np.cumsum(steps.astype(np.int64)))
        whole = self.run.fetch(row, 1, copy_ctx, tag)[0]
        return AddressedArray(np.ascontiguousarray(whole.data[a:b]), np.ascontiguousarray(whole.address[a:b]))

    def seed(self, row, lfsr_state, ones, counted, copy_ctx=None):
        """pm_scan_carry_set on the row's carry from its codec's registers (pm_codec_scan_state) and its LFSR's, behind a piece that bailed or
        went the ordinary way: `taken` and `last_addr` stay."""
        ctx = copy_ctx or self.run.ctx
        check(lib().pm_scan_carry_set(ctx.handle, self.carries.ptr.value + row * ctypes.sizeof(N.RowsCarry), int(lfsr_state), int(ones), int(counted)))
        with self._lock:
            self.seeds += 1

    def went_ordinary(self, count):
        with self._lock:
            self.ordinary += int(count)



def _scan_desc(chains, frames, packets, addrs):
    """pm_rows_scan_chain for each of a run's chains [name, modem, slicer, stream, codec], from where their LFSR registers stand"""
    desc = (N.RowsScanChain * len(chains))()
    for d, ch in zip(desc, chains):
        lfsr, codec = ch[3], ch[4]
        d.lfsr_poly, d.lfsr_state, d.lfsr_invert = lfsr.polynomial, lfsr.shift_register, int(bool(lfsr.invert))
        d.codec_kind, d.sync_tol = int(codec._kind), int(codec.sync_tolerance)
        d.frames, d.packets = int(bool(frames) and codec._kind == 0), int(bool(packets) and codec._kind == 1)
        d.il2p_crc, d.il2p_disable_rs, d.il2p_min_dist = int(codec.collect_trailing_crc), int(codec.disable_rs), int(codec.min_distance)
        d.addrs = int(bool(addrs))
    return desc


_ENGINES = {}


def engine_for(modems, recordings, ctx=None, chunk=0):
    """The cached engine for this group of modems on this context (made for at least `recordings` recordings)."""
    ctx = ctx or Context.default()
    key = (id(ctx), group_key(modems[0]), tuple(bytes(m._loop0) for m in modems), int(chunk))
    hit = _ENGINES.get(key)
    if hit is None or hit.recordings < recordings:
        if hit is not None:
            hit.close()
        hit = _ENGINES[key] = LoopBatch(modems, recordings, ctx, chunk)
    return hit


def close_engines():
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()


def _scannable(chain_sets):
    """The row form of the scan describes a chain once for all recordings: the library's own LFSR and codec objects, every recording's the
    same and in the state they were made in (the codecs decode from the lists only from there)."""
    from .lfsr import LFSR

    def fresh(codec):                                         # (a native codec is made at its first use: none yet, nothing fed yet)
        return codec._h is None

    def what(ch):
        lfsr, codec = ch[3], ch[4]
        return (lfsr.polynomial, lfsr.shift_register, bool(lfsr.invert), codec._kind, bool(codec.collect_trailing_crc), bool(codec.disable_rs),
                int(codec.min_distance), int(codec.sync_tolerance))
    if not all(isinstance(ch[3], LFSR) and hasattr(ch[4], "_handle") and fresh(ch[4]) for cs in chain_sets for ch in cs):
        return False
    return len(chain_sets[0]) <= 64 and all(what(ch) == what(first) for cs in chain_sets for ch, first in zip(cs, chain_sets[0]))


def _fetch_groups(ctx, r, nchains):
    """how a run's rows go to the host: -> (parts, recordings per fetch, the parts' cuts, their side contexts)"""
    import os
    parts = max(1, min(int(os.environ.get("PYMODEM_AMD_LOOP_SLICE_STREAMS", "8")), r))
    per = max(1, int(os.environ.get("PYMODEM_AMD_LOOP_FETCH_ROWS", "256")) // nchains)
    return parts, per, [r * p // parts for p in range(parts + 1)], [Context.side(ctx.device, 400 + p) for p in range(parts)]


def _beside(eng, chain_sets, dev, ctx, k, rows, chain_ids, stages, slot, frames, packets, addrs, t0):
    """process_recordings_device's route with beside=k: the marked run, and this thread driving its marks where it would sleep through the run.
    -> the function that does the remainder and returns the result, or {"gave_up": t} with the run complete and the chains as they were
    at entry.  Nothing here looks at the run's records before the run is complete."""
    import time
    from .chain_execute import _host_rows_pieces, _pool
    from ._native import quick
    from .packet_meta import rows_to_packets
    r, nchains = len(chain_sets), len(chain_sets[0])
    registers = [[ch[3].shift_register for ch in cs] for cs in chain_sets]
    run = eng.run_sliced(dev, [ch[2] for ch in chain_sets[0]], slot=(slot, 0), marks=True)
    marks, chunks = run.marks, run.chunks
    parts, per, cuts, _ = _fetch_groups(ctx, r, nchains)
    # Side contexts and block tags of this slot's own, not the 400 + p of the remainders: with defer=True the remainder of the run before
    # this one (its final pieces, on another thread) lies beside this run's pieces at the marks, and a context's scan scratch and its
    # fetch block serve one call at a time.  A run's pieces, the final one included, all go through the same context.
    lane = 16 * (slot % 2) if isinstance(slot, int) else 0
    sides = [Context.side(ctx.device, 420 + lane + p) for p in range(parts)]
    tags = [("loop-beside", lane, p) for p in range(parts)]
    got_rows = [[[] for _ in range(nchains)] for _ in range(r)]
    state = {"taker": None, "early_bytes": 0}
    lock = threading.Lock()

    def take(p, t):
        # the next piece of this part's rows -- at mark t, or (None) the final one -- a group at a time: every piece is decoded, and the
        # carries that it names are seeded again, before the next piece of the same rows is fetched
        taker, n = state["taker"], 0
        for lo in range(cuts[p], cuts[p + 1], per):
            hi = min(lo + per, cuts[p + 1])
            row0, nr = lo * nchains, (hi - lo) * nchains
            got = taker.fetch(row0, nr, None, t is None, sides[p], tag=tags[p], mark=t)
            n += sum(g[2] for g in got)
            for rec in range(lo, hi):
                views, again, ordinary = _host_rows_pieces(chain_sets[rec], got[(rec - lo) * nchains:(rec - lo + 1) * nchains], chain_ids, frames, packets,
                                                           addrs, lambda j, rec=rec: taker.raw(rec * nchains + j, sides[p], tags[p]))
                for c, v in enumerate(views):
                    got_rows[rec][c].append(v)
                taker.went_ordinary(ordinary)
                for j, reg, ones, counted in again:
                    taker.seed(rec * nchains + j, reg, ones, counted, sides[p])
        if t is not None:
            with lock:
                state["early_bytes"] += n

    def take_all(t):
        if state["taker"] is None:
            state["taker"] = run.pieces(chain_sets[0], frames, packets, addrs)
        for f in [_pool().submit(take, p, t) for p in range(parts)]:
            f.result()

    def give_up(t):
        ctx.sync_relaxed()                                   # the run goes to its end: its engine and its blocks are the next run's
        for cs, regs in zip(chain_sets, registers):
            for ch, reg in zip(cs, regs):
                ch[3].shift_register = reg
                if ch[4]._h is not None:                     # never fed again: the pieces' decoder goes, the next use makes a new one
                    quick().pm_codec_destroy(ch[4]._h)
                    ch[4]._h = None
        return {"gave_up": int(t)}

    taken, last = [], -1
    while True:
        t = next_mark(last, marks.ready(), chunks, k)
        if t is None:
            break
        marks.wait(t)
        if marks.flags(t):
            return give_up(t)
        take_all(t)
        taken.append(t)
        last = t
    ctx.sync_relaxed()
    t1 = time.perf_counter()
    run.records(Context.side(ctx.device, 399))              # (now, and not before: the run is complete)
    if not run.ok():
        # (the run got to its end before the driver got to the mark that says so: every mark is there to be read now -- the first due one
        # with a flag, as if the driver had been in time, or the run's last mark where none was due any more)
        return give_up(next((t for t in range(last + 1, chunks) if (t + 1) % k == 0 and marks.flags(t)), chunks - 1))

    def rest():
        for rec in range(r):
            for c in range(nchains):
                sl = chain_sets[rec][c][2]
                sl._ctx = sl._ctx or ctx
                run.state_into(rec * nchains + c, sl)
        take_all(None)
        sliced = []
        if stages is not None:                               # (diagnosis only: the slicers' bytes as the old way brings them)
            for p in range(parts):
                for lo in range(cuts[p], cuts[p + 1], per):
                    sliced += run.fetch(lo * nchains, (min(lo + per, cuts[p + 1]) - lo) * nchains, sides[p], tag=tags[p])
        t2 = time.perf_counter()

        def joined(rec):
            # (packet rows are 1.3 KB each, gigabytes a run: a chain whose packets all came in one piece keeps that block, the others are
            # copied on the library's threads, a recording each -- new pages are touched faster by many)
            blocks = []
            for v in got_rows[rec]:
                some = [x for x in v if len(x)]
                blocks.append(some[0] if len(some) == 1 else np.concatenate(v))
            return blocks if rows else [rows_to_packets(b, ch[4].identifier) for ch, b in zip(chain_sets[rec], blocks)]
        out = list(_pool().map(joined, range(r)))
        if stages is not None:
            taker = state["taker"]
            stages["sliced"] = [sliced[rec * nchains:(rec + 1) * nchains] for rec in range(r)]
            stages["seconds"] = {"engine": t1 - t0, "slicers": t2 - t1, "host": time.perf_counter() - t2}
            stages["fused_slicers"] = True
            stages["scanned"] = True
            stages["copied_bytes"] = run.copied
            stages["beside"] = {"every": k, "chunks": chunks, "marks": taken, "seeds": taker.seeds, "ordinary": taker.ordinary,
                                "bytes_before_end": state["early_bytes"]}
        return out
    return rest


def process_recordings_device(chain_sets, audios, ctx=None, chunk=0, rows=False, chain_ids=None, stages=None, slot=0, defer=False, scan=None,
                              frames=None, packets=None, addrs=None, pieces=None, beside=None, rows_packets=None):
    """chain_sets[k] = the chains [name, modem, slicer, stream, codec] of recording k (every recording brings the same group of
    chains, as a service decoding successive recordings with one config does), audios[k] its int16 samples (host array or
    DeviceBuffer; equal lengths).  -> [[packets of chain 0, ...] per recording], identical to chain_execute.process_chain on each
    (rows=True: pm_packet rows instead of PacketMeta lists).  All carrier loops of all recordings advance together.
    defer=True: returns when the engine's run is complete, with a function that does the rest (the rows to the host, LFSR + codec) and
    returns the result -- a service calls it on another thread while this one starts the next batch's run (with the other `slot`): the
    host's work on batch k then lies beside the GPU's on batch k + 1 instead of behind it.
    scan / frames / packets (None: the context's switches pipe_scan, pipe_frames, pipe_packets, read from PM_PIPE_SCAN / FRAMES / PACKETS when
    it was made; frames and packets imply scan): the bitstream stage of the fused-slicer route runs on the device, a group of rows per
    pm_rows_scan (SlicedRun.fetch_scanned), and the codecs decode from its lists -- with frames the AX.25 chains' frames, with packets the
    IL2P chains' headers and RS blocks come from there too.  addrs (None: the context's switch pipe_addrs, PM_PIPE_ADDRS; implies scan): the
    rows bring address checkpoints and the codecs resolve an address where they need one instead of expanding every step.  Results are the
    same; stages["scanned"] says which way the decode went.
    pieces (an integer k >= 2; the fused-slicer route with the scan on and chains it can describe, ignored otherwise -- stages["pieces"] is
    then False): every group of rows is taken in k pieces through RowPieces -- up to count * p // k bytes of each row for p = 1 .. k - 1, then
    the final piece -- and each piece is decoded by the carried host route before the next piece of the same rows is fetched, as an engine
    that hands over its rows per time chunk would drive it.  Results are the same, nothing is faster; stages["pieces"] = {"pieces": k,
    "seeds": carries seeded again behind a bail, "ordinary": pieces that went the ordinary way}.
    beside (None: the context's switch pipe_beside, PM_PIPE_BESIDE, default 0; 0: off, nothing changes; an integer k >= 1; anything else
    raises; implies scan; not together with pieces): the host decodes BESIDE the engine's run instead of behind it.  The run is made with
    marks (LoopBatch.run_sliced(marks=True)) and this thread, where it would sleep through the run, takes the rows in pieces at the marks t
    with (t + 1) % k == 0 as they complete (next_mark): per group of rows RowPieces.fetch(mark=t), then the carried host route, every row's
    piece decoded before its next one is fetched.  What is left when the run ends -- the records, the slicers' end states, one final piece --
    is the remainder (with defer=True the caller's, as ever).  A mark whose flag word is set, or a run that is not ok() at its end, means
    the run is to be redone from sign bitmaps: the chains' LFSR registers go back to what they were, the native codecs that the pieces fed
    are dropped (never fed, as at entry), the rows gathered are discarded, stages["beside"] = {"gave_up": t}.  Ignored where pieces is
    ignored (stages["beside"] = False).  Results are the same; stages["beside"] = {"every": k, "chunks": the run's, "marks": [those taken],
    "seeds", "ordinary", "bytes_before_end": slicer bytes decoded from pieces in front of the final one}.
    rows_packets (None: the context's switch pipe_rows_packets, PM_PIPE_ROWS_PACKETS, default 0; implies scan, frames, packets and addrs;
    ignored where pieces is ignored; not together with pieces or beside): the packets of every row whose tables say everything about it are
    finished on the device (SlicedRun.fetch_packets: pm_rows_packets behind pm_rows_scan) and come to the host as pm_packet rows; a
    recording whose rows are all FINISHED makes no codec and no host job -- its result is views of the copied array (rows=True) or
    rows_to_packets of them, its chains' LFSR registers are set from the entries, its slicer states as ever.  The one visible difference:
    its codec objects are left NEVER FED, in the state they were made in (the other routes leave them as the decoder stands behind the
    recording).  A recording with a row that is handed over (bail, short row, a sync hit without a record, ...) is decoded the existing
    way from its parts of the scan block.  Results are the same; stages["rows_packets"] = {"rows", "finished", "handed": {reason: rows},
    "copied_bytes"} (False where ignored)."""
    from .chain_execute import _host_rows, _host_rows_pieces, _host_rows_scanned, _host_stages, _host_stages_scanned, _pool
    from .slicer import slice_batch
    ctx = ctx or Context.default()
    r = len(chain_sets)
    if r == 0:
        return (lambda: []) if defer else []
    frames = bool(ctx.tuned("pipe_frames")) if frames is None else bool(frames)
    packets = bool(ctx.tuned("pipe_packets")) if packets is None else bool(packets)
    addrs = bool(ctx.tuned("pipe_addrs")) if addrs is None else bool(addrs)
    scan = (bool(ctx.tuned("pipe_scan")) if scan is None else bool(scan)) or frames or packets or addrs
    if pieces is not None and (int(pieces) != pieces or pieces < 2):
        raise ValueError("process_recordings_device: pieces is an integer >= 2")
    if beside is None:
        beside = ctx.tuned("pipe_beside")
    if isinstance(beside, bool) or not isinstance(beside, (int, np.integer)) or beside < 0:
        raise ValueError("process_recordings_device: beside is 0 or an integer >= 1 (pipe_beside / PM_PIPE_BESIDE likewise)")
    beside = int(beside)
    if beside and pieces is not None:
        raise ValueError("process_recordings_device: beside and pieces are two ways to cut the same rows; one of them")
    scan = scan or bool(beside)
    rows_packets = bool(ctx.tuned("pipe_rows_packets")) if rows_packets is None else bool(rows_packets)
    if rows_packets and (beside or pieces is not None):
        raise ValueError("process_recordings_device: rows_packets finishes whole rows; not together with pieces or beside")
    if rows_packets:
        scan = frames = packets = addrs = True
    gave_up = None
    dev = []
    for a in audios:
        if isinstance(a, DeviceBuffer):
            dev.append(a)
        else:
            a = np.asarray(a)
            if a.dtype != np.int16:
                raise ValueError("process_recordings_device takes int16 recordings")
            dev.append(ctx.upload(a))
    nchains = len(chain_sets[0])
    # groups of chains that can share an engine, by position in the chain list (the same for every recording)
    groups = {}
    for c, ch in enumerate(chain_sets[0]):
        k = group_key(ch[1])
        if k is None:
            raise ValueError(f"chain {ch[0]!r} is not a carrier-loop chain: use chain_execute.process_chains_device")
        groups.setdefault(k, []).append(c)
    for cs in chain_sets:
        if len(cs) != nchains or any(group_key(cs[c][1]) != k for k, members in groups.items() for c in members):
            raise ValueError("every recording must bring the same group of chains")
    import os
    import time
    t0 = time.perf_counter()
    # One group of chains, every slicer just tuned and the same from recording to recording (a service's chains are made from one config
    # per recording): the slicers run INSIDE the engine, a lane per stream (pm_lbatch_run_sliced).  PYMODEM_AMD_LOOP_FUSED_SLICERS=0, or
    # anything else about the slicers: the engine leaves sign bitmaps and pm_slice_batch slices them afterwards, as before.
    from ._native import SlicerState
    fresh = bytes(SlicerState())
    if (len(groups) == 1 and os.environ.get("PYMODEM_AMD_LOOP_FUSED_SLICERS", "1") != "0"
            and all(hasattr(ch[2], "_params_bytes") and bytes(ch[2]._state) == fresh for cs in chain_sets for ch in cs)
            and all(cs[c][2]._params_bytes() == chain_sets[0][c][2]._params_bytes() for cs in chain_sets for c in range(nchains))):
        eng = engine_for([ch[1] for ch in chain_sets[0]], r, ctx, chunk)
        if beside and _scannable(chain_sets):
            done = _beside(eng, chain_sets, dev, ctx, beside, rows, chain_ids, stages, slot, frames, packets, addrs, t0)
            if not isinstance(done, dict):
                return done if defer else done()
            gave_up = done                                   # (the run is complete and everything the pieces moved is back where it was)
        run = None if gave_up else eng.run_sliced(dev, [ch[2] for ch in chain_sets[0]], slot=(slot, 0))
        if run is not None:
            ctx.sync_relaxed()
            t1 = time.perf_counter()
            run.records(Context.side(ctx.device, 399))      # (not on the context's own stream: the next run may be queued on it by now)
        if run is not None and run.ok():
            scanned = scan and _scannable(chain_sets)       # (foreign stream or codec objects, or codecs that have been used, go the old way)
            in_pieces = int(pieces) if scanned and pieces is not None else 0

            def rest():
                for rec in range(r):
                    for c in range(nchains):
                        sl = chain_sets[rec][c][2]
                        sl._ctx = sl._ctx or ctx
                        run.state_into(rec * nchains + c, sl)
                # to the host a few hundred streams at a time (one gather, one copy), several copies in flight on streams of their own, and a
                # recording whose streams are there goes to the host stage at once, beside the copies still to come
                parts = max(1, min(int(os.environ.get("PYMODEM_AMD_LOOP_SLICE_STREAMS", "8")), r))
                per = max(1, int(os.environ.get("PYMODEM_AMD_LOOP_FETCH_ROWS", "256")) // nchains)
                cuts = [r * p // parts for p in range(parts + 1)]
                sides = [Context.side(ctx.device, 400 + p) for p in range(parts)]
                early = {}
                taker = run.pieces(chain_sets[0], frames, packets, addrs) if in_pieces else None
                finish = scanned and rows_packets
                desc = _scan_desc(chain_sets[0], True, True, True) if finish else None     # (now: recording 0's registers move on with its group)
                tally = {"rows": 0, "finished": 0, "handed": {}}

                def part_finished(p, lo, hi):
                    # the packets of finished rows come as rows; a recording with a row that is handed over goes to the codecs from its parts
                    from concurrent.futures import Future
                    from .packet_meta import rows_to_packets
                    entries, prows, handed = run.fetch_packets(lo * nchains, (hi - lo) * nchains, chain_sets[0], sides[p], ("loop-sliced", p), chain_ids, desc)
                    for rec in range(lo, hi):
                        k = (rec - lo) * nchains
                        if k in handed:
                            early[rec] = (_pool().submit(_host_rows_scanned, chain_sets[rec], handed[k], chain_ids, True, True, True) if rows else
                                          _pool().submit(_host_stages_scanned, chain_sets[rec], handed[k], True, True, True))
                            continue
                        views = []
                        for c, ch in enumerate(chain_sets[rec]):
                            e = entries[k + c]
                            ch[3].shift_register = int(e["lfsr_state"])
                            views.append(prows[int(e["first"]):int(e["first"]) + int(e["packets"])])
                        early[rec] = Future()
                        early[rec].set_result(views if rows else [rows_to_packets(v, ch[4].identifier) for ch, v in zip(chain_sets[rec], views)])
                    with run._copied_lock:
                        tally["rows"] += len(entries)
                        tally["finished"] += int((entries["status"] == 0).sum())
                        for status in entries["status"][entries["status"] != 0].tolist():
                            name = N.ROWS_PACKETS_STATUS[status]
                            tally["handed"][name] = tally["handed"].get(name, 0) + 1

                def part_in_pieces(p, lo, hi):
                    # every piece of these rows is decoded, and the carries that it names are seeded again, before the next one is fetched
                    from concurrent.futures import Future
                    from .packet_meta import rows_to_packets
                    row0, nr = lo * nchains, (hi - lo) * nchains
                    counts = np.asarray(run.records()["count"][row0:row0 + nr], dtype=np.int64)
                    got_rows = {rec: [[] for _ in range(nchains)] for rec in range(lo, hi)}
                    for q in range(1, in_pieces + 1):
                        final = q == in_pieces
                        got = taker.fetch(row0, nr, None if final else counts * q // in_pieces, final, sides[p], tag=("loop-sliced", p))
                        for rec in range(lo, hi):
                            views, again, ordinary = _host_rows_pieces(chain_sets[rec], got[(rec - lo) * nchains:(rec - lo + 1) * nchains], chain_ids, frames, packets,
                                                                       addrs, lambda j, rec=rec: taker.raw(rec * nchains + j, sides[p], ("loop-sliced", p)))
                            for c, v in enumerate(views):
                                got_rows[rec][c].append(v)
                            taker.went_ordinary(ordinary)
                            for j, reg, ones, counted in again:
                                taker.seed(rec * nchains + j, reg, ones, counted, sides[p])
                    for rec in range(lo, hi):
                        blocks = [np.concatenate(v) for v in got_rows[rec]]
                        early[rec] = Future()
                        early[rec].set_result(blocks if rows else [rows_to_packets(b, ch[4].identifier) for ch, b in zip(chain_sets[rec], blocks)])

                def part(p):
                    out = []
                    for lo in range(cuts[p], cuts[p + 1], per):
                        hi = min(lo + per, cuts[p + 1])
                        if in_pieces:
                            part_in_pieces(p, lo, hi)
                            if stages is not None:          # (diagnosis only: the slicers' bytes as the old way brings them)
                                out += run.fetch(lo * nchains, (hi - lo) * nchains, sides[p], tag=("loop-sliced", p))
                            continue
                        if finish:
                            part_finished(p, lo, hi)
                            if stages is not None:          # (diagnosis only: the slicers' bytes as the old way brings them)
                                out += run.fetch(lo * nchains, (hi - lo) * nchains, sides[p], tag=("loop-sliced", p))
                            continue
                        if scanned:
                            # the bitstream stage on the device in front of the copy; a recording's rows go to the codecs at once
                            got = run.fetch_scanned(lo * nchains, (hi - lo) * nchains, chain_sets[0], frames, packets, sides[p], tag=("loop-sliced", p),
                                                    addrs=addrs)
                            for rec in range(lo, hi):
                                mine = got[(rec - lo) * nchains:(rec - lo + 1) * nchains]
                                if rows:
                                    early[rec] = _pool().submit(_host_rows_scanned, chain_sets[rec], mine, chain_ids, frames, packets, addrs)
                                else:
                                    early[rec] = _pool().submit(_host_stages_scanned, chain_sets[rec], mine, frames, packets, addrs)
                            if stages is not None:          # (diagnosis only: the slicers' bytes as the old way brings them)
                                out += run.fetch(lo * nchains, (hi - lo) * nchains, sides[p], tag=("loop-sliced", p))
                            continue
                        got = run.fetch(lo * nchains, (hi - lo) * nchains, sides[p], tag=("loop-sliced", p))
                        out += got
                        for rec in range(lo, hi):
                            if rows:
                                early[rec] = _pool().submit(_host_rows, chain_sets[rec], got[(rec - lo) * nchains:(rec - lo + 1) * nchains], chain_ids)
                    return out
                futs = [_pool().submit(part, p) for p in range(parts)]
                sliced = [x for f in futs for x in f.result()]
                t2 = time.perf_counter()
                if stages is not None:
                    stages["sliced"] = [sliced[rec * nchains:(rec + 1) * nchains] for rec in range(r)]
                    stages["seconds"] = {"engine": t1 - t0, "slicers": t2 - t1}
                    stages["fused_slicers"] = True
                    stages["scanned"] = bool(scanned)
                    stages["copied_bytes"] = run.copied     # (with the scan on: the plain fetch for stages["sliced"] counted too)
                    if pieces is not None:
                        stages["pieces"] = {"pieces": in_pieces, "seeds": taker.seeds, "ordinary": taker.ordinary} if in_pieces else False
                    if beside:
                        stages["beside"] = False                 # (chains that the row form of the scan cannot describe: ignored)
                    if rows_packets:
                        stages["rows_packets"] = dict(tally, copied_bytes=run.copied) if finish else False
                if scanned:
                    out = [early[rec].result() for rec in range(r)]
                    if stages is not None:
                        stages["seconds"]["host"] = time.perf_counter() - t2
                    return out
                if rows:
                    out = [early[rec].result() for rec in range(r)]
                    if stages is not None:
                        stages["seconds"]["host"] = time.perf_counter() - t2
                    return out
                futs = [[_pool().submit(_host_stages, ch, sl) for ch, sl in zip(chain_sets[rec], sliced[rec * nchains:(rec + 1) * nchains])] for rec in range(r)]
                return [[f.result() for f in futs[rec]] for rec in range(r)]
            return rest if defer else rest()
        t0 = time.perf_counter()                # (a row outgrew its room or its 16-bit steps: the whole run again, the other way)
    bitmaps = [[None] * nchains for _ in range(r)]
    for gi, (k, members) in enumerate(groups.items()):
        eng = engine_for([chain_sets[0][c][1] for c in members], r, ctx, chunk)
        got = eng.run(dev, slot=(0 if defer else slot, gi))    # (this way everything is over when the call returns: one bitmap set will do)
        for rec in range(r):
            for j, c in enumerate(members):
                sl = chain_sets[rec][c][2]
                sl._ctx = sl._ctx or ctx
                bitmaps[rec][c] = sl.sign_bitmaps(got[rec][j])
    ctx.sync_relaxed()                 # seconds: sleep through them instead of spinning in the slicer's first stream wait
    t1 = time.perf_counter()
    flat_slicers = [chain_sets[rec][c][2] for rec in range(r) for c in range(nchains)]
    flat_bits = [bitmaps[rec][c] for rec in range(r) for c in range(nchains)]
    if len(flat_slicers) >= 256:
        # Thousands of streams go through pm_slice_batch 64 at a time, each call a sequence of lockstep launches that ends in a wait.
        # Here the parallelism is in the streams, not inside one: long chunks (1024 words instead of 384: N (1 + m/L) lane-steps with m/L
        # a few percent instead of 0.6) and eight calls in flight on eight streams of their own (eight threads) -- qpsk_2400, 2048 x 8
        # quadrature streams: 2.4 ms per recording with two calls of short chunks in flight
        import os
        parts = max(1, min(int(os.environ.get("PYMODEM_AMD_LOOP_SLICE_STREAMS", "8")), r))
        words = int(os.environ.get("PYMODEM_AMD_LOOP_SLICE_CHUNK_WORDS", "1024"))
        cuts = [(r * p // parts) * nchains for p in range(parts + 1)]
        sides = [Context.side(ctx.device, 400 + p) for p in range(parts)]
        for sc in sides:
            if getattr(sc, "_loop_slice_words", None) != words:
                check(lib().pm_slicer_limits(sc.handle, words))
                sc._loop_slice_words = words
        # ... and the output crosses to the host in pm_slice_compact's form (exact counts, 16-bit address steps: 3 bytes per data byte
        # instead of 9 x the 1.5x capacity -- 18 GB instead of 80 for that run)
        # -- one group of 64 streams at a time, fetched before the next: the device blocks of a stream's context are the same for
        # every group (a key per group kept 80 GB of them alive beside the bitmaps)
        # ... and a recording whose streams are all through goes to the host stage at once (LFSR + codec on the library's threads), beside
        # the slicer groups still to come: the two stages of a run overlap instead of following each other (qpsk_2400: 0.56 + 0.75 ms per
        # recording one after the other)
        early = {}

        def part(p):
            out, rec = [], cuts[p] // nchains
            for lo in range(cuts[p], cuts[p + 1], 64):
                hi = min(lo + 64, cuts[p + 1])
                out += slice_batch(flat_slicers[lo:hi], flat_bits[lo:hi], sides[p], defer=True, compact=True, out_tag=("loop-slice", p))(sides[p])
                while rows and (rec + 1) * nchains - cuts[p] <= len(out):
                    at = rec * nchains - cuts[p]
                    early[rec] = _pool().submit(_host_rows, chain_sets[rec], out[at:at + nchains], chain_ids)
                    rec += 1
            return out
        futs = [_pool().submit(part, p) for p in range(parts)]
        sliced = [x for f in futs for x in f.result()]
    else:
        sliced, early = slice_batch(flat_slicers, flat_bits, ctx), {}
    t2 = time.perf_counter()
    if stages is not None:
        stages["sliced"] = [sliced[rec * nchains:(rec + 1) * nchains] for rec in range(r)]
        stages["seconds"] = {"engine": t1 - t0, "slicers": t2 - t1}
        if pieces is not None:
            stages["pieces"] = False                         # (not the fused-slicer route: ignored)
        if beside:
            stages["beside"] = gave_up if gave_up else False
        if rows_packets:
            stages["rows_packets"] = False                   # (not the fused-slicer route: ignored)
    out = []
    if rows:
        futs = [early[rec] if rec in early else _pool().submit(_host_rows, chain_sets[rec], sliced[rec * nchains:(rec + 1) * nchains], chain_ids)
                for rec in range(r)]
        out = [f.result() for f in futs]
        if stages is not None:
            stages["seconds"]["host"] = time.perf_counter() - t2
        return (lambda: out) if defer else out
    futs = [[_pool().submit(_host_stages, ch, sl) for ch, sl in zip(chain_sets[rec], sliced[rec * nchains:(rec + 1) * nchains])] for rec in range(r)]
    for rec in range(r):
        out.append([f.result() for f in futs[rec]])
    return (lambda: out) if defer else out
