"""What pm_stream_packets writes, restated from the definition in include/pymodem_amd.h: the dense form -- head, an entry a job, the
records job after job -- on top of the model blocks (bitscan_model, frames_model, il2p_packets_model) and of rows_packets_model's two rules
and packet fields, which restate the oracle's decoders and PacketMeta's checks (test_stream_packets_model.py holds every finished stream
to IL2PCodec.decode / AX25Codec.decode again).  What differs from the row form is all here: a packet's address is the stream's own at its
byte, whatever the steps between the addresses are; a record is the 40-byte head, `len` bytes and zeros up to a multiple of 8; the room is
counted in bytes; LEFT_OUT does not occur.
Shared by test_stream_packets_model.py, test_stream_packets_core.py and test_gpu_stream_packets.py."""
import functools

import numpy as np

import frames_model as FM
import il2p_packets_model as PM
import rows_packets_model as RP
from pymodem_amd import _native as N

FINISHED, NO_ROOM, NO_CODEC = RP.FINISHED, RP.NO_ROOM, RP.NO_CODEC


def record(packet, source):
    """the record of a packet (streamaddress, data, BytesCorrected, calculated CRC or None): the head of its pm_packet row, its bytes, zeros"""
    row = RP.packet_row(packet, source)
    length = int(row["len"][0])
    return row.tobytes()[:40] + row["data"][0, :(length + 7) // 8 * 8].tobytes()


def job(kind, plain, block=None, addr=None, tol=0, crc=True, source=0, register=0):
    """a job of a call: the stream, the model's part of the block for it, its addresses (0, 1, 2, ... when none are given)"""
    plain = np.asarray(plain, dtype=np.uint8)
    if block is None:
        block = FM.model_block_frames(plain)[0] if kind == 0 else PM.model_block_packets(plain, tol, crc=crc)[0] if kind == 1 else None
    return dict(kind=kind, plain=plain, block=block, addr=np.arange(len(plain), dtype=np.int64) if addr is None else np.asarray(addr, dtype=np.int64),
                tol=tol, crc=crc, source=source, register=register)


def job_packets(j):
    """(status, packets, corrected left over) of a job by the rule of its kind"""
    if j["kind"] < 0:
        return NO_CODEC, [], 0
    return RP.row_packets(j["kind"], j["block"], j["plain"], j["addr"], j["tol"], j["crc"])


def model_call(jobs, room, walks=None):
    """jobs: [job(...)] in call order; room: the bytes d_out has behind head and entries; walks: job_packets of every job, when the caller
    has them already.  -> (head, entries, the records' bytes) as pm_stream_packets leaves them."""
    entries = np.zeros(len(jobs), dtype=N.stream_packets_entry_dtype())
    out, packets, full = b"", 0, False
    room = room // 8 * 8
    for r, j in enumerate(jobs):
        status, pkts, left = walks[r] if walks else job_packets(j)
        recs = b"".join(record(p, j["source"]) for p in pkts) if status == FINISHED else b""
        full = full or len(out) + len(recs) > room
        if full:
            status, pkts, left, recs = NO_ROOM, [], 0, b""
        elif status != FINISHED:
            pkts, left = [], 0
        entries[r] = (j["register"], status, len(pkts), len(out), left, 0)
        out += recs
        packets += len(pkts)
    head = np.zeros(1, dtype=N.stream_packets_head_dtype())
    head["jobs"], head["handed"], head["packets"], head["bytes"] = len(jobs), int((entries["status"] != FINISHED).sum()), packets, len(out)
    return head, entries, np.frombuffer(out, dtype=np.uint8)


def records_of(raw, njobs):
    """[[(streamaddress, data, BytesCorrected)] per job] of a dense form, through the package's iterator"""
    out = [[] for _ in range(njobs)]
    for j, head, data in N.stream_packets_records(raw, njobs):
        out[j].append((int(head["streamaddress"]), bytes(data), int(head["bytes_corrected"])))
    return out


# ---- the model's streams as jobs ----------------------------------------------------------------------------------------------------------
def stepped_addresses(r, n):
    """addresses for stream r whose steps pass 16 bits now and then: nothing a checkpoint table with 16-bit steps could say"""
    steps = 1 + (np.arange(n, dtype=np.int64) * (r + 3)) % 17
    steps[(np.arange(n) % 97) == 5] = 70000 + r
    return 10 ** 10 + 1000 * r + np.cumsum(steps)


@functools.lru_cache(maxsize=None)
def il2p_jobs():
    """il2p_packets_model's 49 streams, in the order of their names: every tolerance and option they come with"""
    out = []
    for r, (name, (plain, tol, o)) in enumerate(sorted(PM.all_streams().items())):
        j = job(1, plain, PM.block_of(name)[0], stepped_addresses(r, len(plain)), tol, o["crc"], 100 + r)
        j.update(name=name, disable_rs=o["disable_rs"], min_dist=o["min_dist"])
        out.append(j)
    return out


@functools.lru_cache(maxsize=None)
def il2p_walks():
    return [job_packets(j) for j in il2p_jobs()]


AX25_NAMES = ("len18_17_at3", "shared_zero", "abort_then_flag", "frame1100", "bail_at_once", "bail_after_a_flag", "short0", "short1", "short23", "short24",
              "short25", "survive_at5", "long_no_bail", "first_closes", "first_closes_after_run", "two_flags_one_word", "random1")


@functools.lru_cache(maxsize=None)
def ax25_jobs():
    """frames_model's streams that say something about the rule: frames at both edges of the length, aborts, a frame longer than a packet
    row, bails, the short ones, a first flag that closes a frame"""
    streams = FM.all_streams()
    out = []
    for r, name in enumerate(AX25_NAMES):
        j = job(0, streams[name], None, stepped_addresses(50 + r, len(streams[name])), source=200 + r)
        j.update(name=name, disable_rs=False, min_dist=0)
        out.append(j)
    return out


@functools.lru_cache(maxsize=None)
def ax25_walks():
    return [job_packets(j) for j in ax25_jobs()]


# ---- streams for the walk launch's trips: a first flag that closes nothing, then events - 1 frames, each closed by one flag ----------------
EVENT_COUNTS = (0, 1, 63, 64, 65, 129)


def events_stream(events, seed=0):
    """descrambled bytes with exactly `events` listed events (0: no flag at all, and no bail either)"""
    import bitscan_model as M
    from pymodem_amd import siggen
    if events == 0:
        return np.random.default_rng(seed).choice(M.CALM, 100)
    bits = list(M.FLAG)
    for k in range(events - 1):
        bits += siggen.ax25_hdlc_bits(M._frame(18 + (5 * k + seed) % 23, 7000 + 131 * seed + k), pre_flags=0, post_flags=1)
    return np.concatenate([M._pack(bits + [0] * 3), np.random.default_rng(seed).choice(M.CALM, 30)])      # (24 bytes or more: not SHORT)


@functools.lru_cache(maxsize=None)
def events_jobs():
    out = []
    for r, events in enumerate(EVENT_COUNTS):
        plain = events_stream(events, r)
        j = job(0, plain, None, stepped_addresses(80 + r, len(plain)), source=300 + r)
        j.update(name=f"events{events}", disable_rs=False, min_dist=0)
        out.append(j)
    return out


@functools.lru_cache(maxsize=None)
def events_walks():
    return [job_packets(j) for j in events_jobs()]
