"""The host route for rows scanned in pieces (pm_host_decode_batch with pm_host_job.scan_carry, pm_codec.cpp): parts written by
rows_pieces_model.py -- a row cut by pm_rows_scan_pieces' rule, each piece the job form's part of scan_carry_model.py behind its steps and in
front of the 40-byte tail -- go through the carried route with addr_first = the piece's addr_before, with address checkpoints and without.
What a row piece adds is its addressing: byte 0 of a later piece lies at addr_before + steps[0], and that step is not 0.  Without addrs the
steps are expanded from addr_first, which already counts step 0; with addrs A[0] must be addr_before + steps[0], which pm_codec_decode_carried
now accepts (and nothing else).  The cuts lie at every multiple of 8 around a flag, a stuffed zero, a run of seven, a closing flag's last one,
inside a frame and through an IL2P packet -- the streams are shifted byte by byte so that each mark meets the cuts at every distance.  Packet
rows, LFSR registers and pm_codec_scan_state equal pm_codec_decode on the whole stream and the oracle; pm_codec_walked stays within the
model's bound.  No GPU: the kernels are held to the job form and the same model in test_gpu_rows_pieces.py."""

import numpy as np
import pytest

import rows_pieces_model as RM
import scan_carry_model as CM
import test_host_scan_carry as H
from pymodem_amd._native import SCAN_CARRY_OK, HostJob, lib

POLY, INVERT = H.POLY, H.INVERT
CAP = 1024
IL2P = dict(tol=0, crc=True, disable_rs=False, min_dist=0)


def steps_for(n, seed):
    """a row's steps: the first 0, none of the others 0 (every later piece's first step counts), one of them 65535"""
    steps = (40 + (np.arange(CAP) * (3 + seed % 5)) % 23).astype(np.uint16)
    steps[0] = 0
    if n > 1:
        steps[1 + (seed * 37) % (n - 1)] = 65535
    return steps


def host_job(codec, steps, addr_before, n, scan, frames, packets, addrs, reg):
    jobs = (HostJob * 1)()
    j = jobs[0]
    j.codec, j.h_data, j.h_addr, j.n = codec.h, None, None, n
    j.h_addr_delta, j.addr_first = (steps.ctypes.data if n else None), addr_before
    j.h_scan, j.scan_frames, j.scan_packets, j.scan_addrs, j.scan_carry = scan.ctypes.data, frames, packets, addrs, 1
    j.lfsr_poly, j.lfsr_state, j.lfsr_invert = POLY, reg, INVERT
    return jobs


def run_row(plain, uptos, kind, frames=0, packets=0, addrs=0, opts=None, seed=0):
    """The stream as a row, taken up to each of `uptos` and then finally, every piece through the model and pm_host_decode_batch.
    -> the pieces' n"""
    opts = dict(opts or {})
    plain = np.ascontiguousarray(plain, dtype=np.uint8)
    n_all = len(plain)
    assert n_all <= CAP
    raw = np.zeros(CAP, dtype=np.uint8)
    raw[:n_all] = CM.scramble(plain, POLY)
    steps = steps_for(n_all, seed)
    first = H.FIRST + seed
    addr = first + np.cumsum(steps[:n_all].astype(np.int64))
    got, ref = H.Codec(kind, **opts), H.Codec(kind, **opts)
    pk = {k: v for k, v in opts.items() if k != "tol"} if packets else None
    carry = RM.rows_carry_start(0)
    reg, rows_got, ns = 0, [], []
    for k, upto in enumerate(list(uptos) + [None]):
        final = upto is None
        n = RM.piece_bytes(n_all, CAP, upto, carry["taken"], final)
        a = carry["taken"]
        assert final or n % 8 == 0
        part, written, after, plain_piece, addr_before = RM.model_row_piece(raw, steps, first, carry, n, POLY, INVERT, kind, opts.get("tol", 0), bool(frames), pk, bool(addrs))
        assert np.array_equal(plain_piece, plain[a:a + n]), "the register crosses the cut"
        assert addr_before == (int(addr[a - 1]) if a else first) and (a == 0 or n == 0 or steps[a] != 0)
        part = np.where(written, part, 0xA5).astype(np.uint8)     # what the device does not write is not read
        got_steps, scan, before = RM.split_piece(part, kind, frames, packets, n, addrs)
        assert before == addr_before
        scan = np.ascontiguousarray(scan)
        piece_steps = np.ascontiguousarray(got_steps)
        jobs = host_job(got, piece_steps, addr_before, n, scan, frames, packets, addrs, reg)
        walked = got.walked()
        rc = lib().pm_host_decode_batch(jobs, 1, 1)
        assert rc == 0 and jobs[0].status == 0, (k, a, n, rc)
        reg = int(jobs[0].lfsr_state)
        assert reg == after["scan"]["lfsr_state"]
        rows_got.append(got.fetch(int(jobs[0].pending)))
        if kind == 0:
            assert got.walked() - walked <= CM.walked_bound(scan, n, frames), (k, a, n)
            if after["scan"]["state"] == SCAN_CARRY_OK and after["scan"]["counted"] < 8000:
                assert got.scan_state() == (after["scan"]["ones"], after["scan"]["counted"]), ("the model's carry-out is the decoder's registers", k, a, n)
        ns.append(n)
        carry = after
    assert carry["taken"] == n_all and carry["last_addr"] == (int(addr[-1]) if n_all else 0)
    whole = ref.decode(plain, addr)
    flat = np.concatenate(rows_got)
    assert flat.tobytes() == whole.tobytes(), "pm_codec_decode on the whole stream"
    assert got.scan_state() == ref.scan_state() and reg == CM.host_lfsr(raw[:n_all], POLY, 0, INVERT)[1]
    assert H._rows(flat) == H._oracle_rows(kind, plain, addr, opts), "the oracle fed the whole stream"
    return ns, len(flat)


def cuts_around(at):
    """the multiples of 8 within 8 bytes of byte `at`"""
    return [c for c in range((at - 8) // 8 * 8, at + 9, 8) if at - 8 <= c <= at + 8]


@pytest.mark.parametrize("frames,addrs", H.MODES)
@pytest.mark.parametrize("name", sorted(H.ax25_windows()))
def test_ax25_rows_cut_at_every_multiple_of_8_around_a_mark(name, frames, addrs):
    plain, at = H.ax25_windows()[name]
    packets = seen = 0
    for shift in range(8):                                    # the mark's byte at every distance from the cuts
        stream = plain[shift:]
        for cut in cuts_around(at - shift):
            ns, found = run_row(stream, [cut + 5], 0, frames=frames, addrs=addrs, seed=shift)
            assert ns == [cut, len(stream) - cut]
            packets += found
            seen += 1
    assert seen >= 16 and packets > 0
    # three pieces with one of 8 bytes at the mark, an empty one (upto - taken < 8) in between, and one more in front of the final one
    mark = at // 8 * 8
    ns, _ = run_row(plain, [mark, mark + 7, mark + 8, mark + 8, 688 + 3], 0, frames=frames, addrs=addrs, seed=9)
    assert ns == [mark, 0, 8, 0, 688 - mark - 8, len(plain) - 688]


@pytest.mark.parametrize("packets,addrs", H.MODES)
def test_il2p_rows_cut_at_every_multiple_of_8_through_a_packet(packets, addrs):
    plain = H.il2p_stream()
    first = 40 + H.PM.SYNC_AT // 8 - 2
    last = first + 2 + 3 + 15 + 20 + 16 + 4 + 3
    seen = 0
    for shift in range(8):
        stream = plain[shift:]
        for cut in range((first - shift) // 8 * 8, last - shift + 8, 8):
            ns, found = run_row(stream, [cut], 1, packets=packets, addrs=addrs, opts=IL2P, seed=shift)
            assert found == 2 and ns == [cut, len(stream) - cut]
            seen += 1
        run_row(stream, [48, 56, 57, 96], 1, packets=packets, addrs=addrs, opts=IL2P, seed=shift)
    assert seen >= 8 * 8


@pytest.mark.parametrize("final_mod", range(8))
def test_the_final_piece_takes_what_the_cuts_held_back(final_mod):
    plain, at = H.ax25_windows()["inside_a_frame"]
    stream = plain[:688 + final_mod]
    ns, _ = run_row(stream, [at + 3, len(stream)], 0, frames=1, addrs=1, seed=final_mod)
    cut = (at + 3) // 8 * 8
    assert ns == [cut, 688 - cut, final_mod]


def test_the_refusals_stay_and_a_first_step_of_zero_means_what_it_meant():
    plain, at = H.ax25_windows()["straddle_flag_3"]
    raw = np.zeros(CAP, dtype=np.uint8)
    raw[:len(plain)] = CM.scramble(plain, POLY)
    steps = steps_for(len(plain), 1)
    first = H.FIRST
    cut = at // 8 * 8

    def pieces(codec):
        """piece 0 through the route -> (piece 1's steps, addr_before, n, scan part, register)"""
        carry = RM.rows_carry_start(0)
        part, written, carry, _, before = RM.model_row_piece(raw, steps, first, carry, cut, POLY, INVERT, 0, 0, True, None, True)
        s, scan, _ = RM.split_piece(np.where(written, part, 0xA5).astype(np.uint8), 0, 1, 0, cut, 1)
        s, scan = np.ascontiguousarray(s), np.ascontiguousarray(scan)
        jobs = host_job(codec, s, before, cut, scan, 1, 0, 1, 0)
        assert lib().pm_host_decode_batch(jobs, 1, 1) == 0
        n = len(plain) - cut
        part, written, _, _, before = RM.model_row_piece(raw, steps, first, carry, n, POLY, INVERT, 0, 0, True, None, True)
        s, scan, _ = RM.split_piece(np.where(written, part, 0xA5).astype(np.uint8), 0, 1, 0, n, 1)
        return np.ascontiguousarray(s), before, n, np.ascontiguousarray(scan), int(jobs[0].lfsr_state)

    def refused(change):
        codec = H.Codec(0)
        s, before, n, scan, reg = pieces(codec)
        assert s[0] != 0
        s, before, scan = change(s.copy(), before, scan.copy())
        fed, state = codec.fed(), codec.scan_state()
        jobs = host_job(codec, s, before, n, scan, 1, 0, 1, reg)
        rc = lib().pm_host_decode_batch(jobs, 1, 1)
        assert (codec.fed(), codec.scan_state()) == (fed, state) or rc == 0, "a refusal leaves the codec untouched"
        return rc

    tail = 32                                                  # the carry piece ends the scan part
    assert refused(lambda s, b, scan: (s, b, scan)) == 0
    assert refused(lambda s, b, scan: (s, b + int(s[0]), scan)) == -2, "addr_first is the address in front of the piece, not the piece's first"
    assert refused(lambda s, b, scan: (s, b - 1, scan)) == -2, "A[0] must be addr_before + steps[0]"

    def zero_first_step(s, b, scan):
        s[0] = 0
        return s, b, scan
    assert refused(zero_first_step) == -2, "a table that cannot belong to the stream"

    def other_ones(s, b, scan):
        scan[len(scan) - tail + 4:len(scan) - tail + 8].view(np.int32)[0] += 1
        return s, b, scan
    assert refused(other_ones) == -2, "a carry piece that disagrees with the codec"

    def other_piece(s, b, scan):
        scan[len(scan) - tail + 16:len(scan) - tail + 24].view(np.int64)[0] = 2
        return s, b, scan
    assert refused(other_piece) == -2, "a wrong piece number"
