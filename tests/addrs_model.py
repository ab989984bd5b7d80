"""The address checkpoints of a scanned stream (pm_scan_job.addrs, pm_rows_scan_chain.addrs; csrc/pm_bitscan_addrs.h) by numpy.cumsum: the one
definition that the row form's arithmetic, the kernels and the host's look-up are held to.
    address of byte k = first + steps[1] + ... + steps[k]        (steps[0], "the first one 0", is never added)
    A[w]              = the address of byte 64 w, for w < (n + 63) / 64"""
import numpy as np

STRIDE = 64           # PM_SCAN_ADDR_STRIDE
MAX_GAP = 64 * 65535  # what 64 steps of 16 bits add at the most


def addr_bytes(n):
    """PM_SCAN_ADDR_BYTES"""
    return 8 * ((n + 63) // 64)


def addresses(first, steps):
    """every byte's address from the first one and the 16-bit steps, in 64 bits"""
    s = np.asarray(steps).astype(np.int64)
    if len(s):
        s[0] = 0
    return int(first) + np.cumsum(s, dtype=np.int64)


def checkpoints(first, steps):
    return np.ascontiguousarray(addresses(first, steps)[::STRIDE], dtype="<i8")


def checkpoints_of_addresses(addr):
    """the job form: the slicer's full addresses are there, every 64th is a checkpoint"""
    return np.ascontiguousarray(np.asarray(addr, dtype=np.int64)[::STRIDE], dtype="<i8")


def steps_of_addresses(addr):
    """pm_slice_compact's form of ascending addresses whose steps fit 16 bits"""
    a = np.asarray(addr, dtype=np.int64)
    d = np.diff(a, prepend=a[:1])
    assert len(a) == 0 or (d.min() >= 0 and d.max() <= 65535)
    return np.ascontiguousarray(d, dtype=np.uint16)


def with_checkpoints(block, first, steps):
    """a job's part (record, list, bytes, tables, areas) with the checkpoint table behind it"""
    block = np.asarray(block, dtype=np.uint8)
    assert len(block) % 8 == 0
    return np.ascontiguousarray(np.concatenate([block, checkpoints(first, steps).view(np.uint8)]))


def lookup(table, steps, k):
    """what the host resolves: A[k >> 6] plus steps (k & ~63) + 1 .. k -> (address, steps added)"""
    lo = (k & ~63) + 1
    return int(table[k >> 6]) + int(np.asarray(steps[lo:k + 1], dtype=np.int64).sum()), k & 63
