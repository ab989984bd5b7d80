"""A chain that is fed audio as it arrives, with its bitstream stage on the device: ScannedChain.feed(audio) is process_chain_device for
the next piece of a stream -- demod_signs, the slicer's batch with its bytes left on the device, pm_stream_scan with the chain's carry
(pm_scan_carry: LFSR register, the last 64 descrambled bits, the decoder's ones and counted bits), one copy to the host, and the carried
host route (pm_host_job.scan_carry -> pm_codec_decode_carried), which takes a codec in any state.  The pieces' lists, frames and packets are
made for a decoder that continues the stream, so what comes out is what process_chain_device gives for the same pieces, and the chain's
LFSR register and codec stay current: the chain can go on through process_chain_device, and one that was fed that way can go on here."""
import ctypes

import numpy as np

from ._native import (SCAN_CARRY_LOST, SCAN_HEAD, HostJob, ScanCarry, ScanJob, check, lib, packet_dtype, quick, scan_carry_piece_dtype,
                      scan_list_bytes, scan_part_bytes, scan_record_dtype, SCAN_CARRY_BYTES)
from .data_classes import AddressedArray
from .device import Context

_COMPACT_HEAD = 80        # PM_COMPACT_HEAD


class ScannedChain:
    """chain: (name, modem, slicer, LFSR, codec) as chain_builder.build_chain makes it.  frames / packets / addrs: the AX.25 chain's frames,
    the IL2P chain's attempts, the address checkpoints on the device too (pm_scan_job.frames / .packets / .addrs)."""

    def __init__(self, chain, ctx=None, frames=False, packets=False, addrs=False):
        self.chain = chain
        self.ctx = ctx or Context.default()
        self.kind = chain[4]._kind
        self.frames, self.packets, self.addrs = bool(frames) and self.kind == 0, bool(packets) and self.kind == 1, bool(addrs)
        self._carry = self.ctx.empty(ctypes.sizeof(ScanCarry), np.uint8)
        self._key = self.ctx.owner_key(self)                 # the work buffers go when this object goes
        self._seeded = False
        self._fed = self._reg = None                         # the codec's fed bytes and the LFSR register behind the last scanned piece
        self.pieces = self.seeds = self.ordinary = 0

    def _codec_fed(self):
        w, j = ctypes.c_int64(), ctypes.c_int64()
        check(quick().pm_codec_walked(self.chain[4]._handle(), ctypes.byref(w), ctypes.byref(j)))
        return w.value + j.value

    def _seed(self):
        """pm_scan_carry_set from the chain as it stands; False: this piece has to go the ordinary way (an AX.25 codec that has been fed and
        stands at ones 0, counted 0 cannot be told from a just-created one by the seed, but may hold bytes of a frame)"""
        ones, counted = ctypes.c_int32(), ctypes.c_int64()
        check(quick().pm_codec_scan_state(self.chain[4]._handle(), ctypes.byref(ones), ctypes.byref(counted)))
        if self.kind == 0 and self._codec_fed() > 0 and (ones.value, counted.value) == (0, 0):
            return False
        check(lib().pm_scan_carry_set(self.ctx.handle, self._carry.ptr, int(self.chain[3].shift_register), ones.value, counted.value))
        self.seeds += 1
        return True

    def carry(self):
        """the carry as the device holds it (a copy; waits for the stream)"""
        from ._native import scan_carry_dtype
        self.ctx.sync()
        return self._carry.download().view(scan_carry_dtype())[0]

    def _slice(self, bitmap):
        """the slicer's batch for this chain alone (slicer.slice_batch: its capacity rule and its retry), bytes and addresses left on the
        device -> (jobs, block, the addresses' offset in the block)"""
        from .slicer import slice_batch
        fetch = slice_batch([self.chain[2]], [bitmap], ctx=self.ctx, defer=True, out_tag=(self._key, "scanned_slice"))
        jobs, block, _, a_off, _ = fetch.fetchers[0].device
        return jobs, block, a_off[0]

    def feed_rows(self, audio, stages=None):
        """The next piece of the stream -> the pm_packet rows it completes (a NumPy array of _native.packet_dtype)."""
        ctx, (_, modem, slicer, lfsr, codec) = self.ctx, self.chain
        signs = modem.demod_signs(audio)
        bitmap = slicer.sign_bitmaps(signs)
        if bitmap[2] == 0:
            if stages is not None:
                stages["sliced"] = stages["descrambled"] = AddressedArray(np.zeros(0, np.uint8), np.zeros(0, np.int64))
            return np.zeros(0, dtype=packet_dtype())
        jobs, block, a_off = self._slice(bitmap)
        n = int(jobs[0].count)
        scan = self._seeded and self._fed == self._codec_fed() and self._reg == int(lfsr.shift_register)
        if not scan:
            scan = self._seeded = self._seed()
        # the slicer's compact form (first address, 16-bit steps, bytes) and the scan part behind it, in one block and one copy
        compact_bytes = _COMPACT_HEAD + (2 * n + 7) // 8 * 8 + (n + 7) // 8 * 8
        part_bytes = scan_part_bytes(self.kind, self.frames, self.packets, n, self.addrs) + SCAN_CARRY_BYTES if scan else 0
        at = (compact_bytes + 255) & ~255
        dense = ctx.scratch((self._key, "scanned_out"), at + part_bytes + 8, np.uint8)
        offs, used = (ctypes.c_int64 * 1)(), ctypes.c_size_t()
        check(lib().pm_slice_compact(ctx.handle, jobs, 1, dense.ptr, at, offs, ctypes.byref(used)))
        if scan:
            sj = (ScanJob * 1)()
            sj[0].d_data, sj[0].n, sj[0].lfsr_poly, sj[0].lfsr_invert = jobs[0].d_data, n, int(lfsr.polynomial), int(bool(lfsr.invert))
            sj[0].codec_kind, sj[0].sync_tol = self.kind, int(getattr(codec, "sync_tolerance", 0))
            sj[0].frames, sj[0].packets, sj[0].addrs = int(self.frames), int(self.packets), int(self.addrs)
            if self.kind == 1:
                sj[0].il2p_crc, sj[0].il2p_disable_rs, sj[0].il2p_min_dist = int(codec.collect_trailing_crc), int(codec.disable_rs), int(codec.min_distance)
            sj[0].d_addr = jobs[0].d_addr if self.addrs else None
            sj[0].d_carry = self._carry.ptr.value
            soffs, sused = (ctypes.c_int64 * 1)(), ctypes.c_size_t()
            check(lib().pm_stream_scan(ctx.handle, sj, 1, dense.ptr.value + at, part_bytes, soffs, ctypes.byref(sused)))
            assert sused.value == part_bytes
        host = dense.download(at + part_bytes)                # (waits for the stream)
        first = int(host[0:8].view(np.int64)[0])
        steps = host[_COMPACT_HEAD:_COMPACT_HEAD + 2 * n].view(np.uint16)
        data = host[_COMPACT_HEAD + (2 * n + 7) // 8 * 8:_COMPACT_HEAD + (2 * n + 7) // 8 * 8 + n]
        full = None
        if n and host[16:_COMPACT_HEAD].any():               # a step beyond 16 bits: the addresses in full
            full = block.view(a_off, n * 8).download().view(np.int64)
        sliced = AddressedArray(data, full) if full is not None else AddressedArray.from_steps(data, steps, first)
        self.pieces += 1
        def ordinary():                                      # the host's LFSR and the codec's own search, from the slicer bytes just brought
            self.ordinary += 1
            plain = lfsr.stream_unscramble_8bit(sliced)
            if stages is not None:
                stages["sliced"], stages["descrambled"] = sliced, plain
            return codec.decode_rows(plain)
        if not scan:
            return ordinary()
        part = host[at:at + part_bytes]
        hj = (HostJob * 1)()
        j = hj[0]
        j.codec, j.h_data, j.n = codec._handle(), None, n
        if full is not None:
            j.h_addr = full.ctypes.data
        else:
            j.h_addr, j.h_addr_delta, j.addr_first = None, (steps.ctypes.data if n else None), first
        j.h_scan, j.scan_frames, j.scan_packets, j.scan_carry = part.ctypes.data, int(self.frames), int(self.packets), 1
        j.scan_addrs = int(self.addrs and full is None)
        j.lfsr_poly, j.lfsr_state, j.lfsr_invert = int(lfsr.polynomial), int(lfsr.shift_register), int(bool(lfsr.invert))
        # The device carry has moved on by this piece whatever the host makes of it: until the host route has taken the piece, the next one
        # is to be seeded again from the codec.
        self._seeded = False
        fed = self._codec_fed()
        rc = lib().pm_host_decode_batch(hj, 1, 1)
        if rc != 0:
            if self._codec_fed() == fed:                     # refused with the codec untouched: the piece is not lost, it goes the ordinary way
                return ordinary()
            check(rc)
        lfsr.shift_register = j.lfsr_state
        rec = part[:SCAN_HEAD].view(scan_record_dtype())[0]
        piece = part[part_bytes - SCAN_CARRY_BYTES:].view(scan_carry_piece_dtype())[0]
        # LOST: the carry behind a piece that bailed, or in front of this one -- the next piece is seeded from the codec's registers
        self._seeded = not (int(piece["state"]) == SCAN_CARRY_LOST or (self.kind == 0 and int(rec["bail_bit"]) >= 0))
        self._fed, self._reg = self._codec_fed(), int(lfsr.shift_register)
        if stages is not None:
            lb = scan_list_bytes(self.kind, n)
            stages["sliced"] = sliced
            stages["descrambled"] = AddressedArray(part[SCAN_HEAD + lb:SCAN_HEAD + lb + n], sliced.address)
            stages["scan_part"] = part
        return codec.fetch_into(np.empty(int(j.pending), dtype=packet_dtype()))

    def feed(self, audio, stages=None):
        """The next piece of the stream -> list[PacketMeta], as process_chain_device(chain, audio) gives it."""
        from .packet_meta import rows_to_packets
        return rows_to_packets(self.feed_rows(audio, stages), self.chain[4].identifier)
