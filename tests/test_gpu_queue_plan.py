"""The executor's queue plan (pipe_queue_plan in pm_pipe.hip) and what it stands on: pm_ctx_create_prio's three priority levels, the
handover of EVERY recording from the caller's stream to a demod stream of the pipeline's own, the contexts the pipeline lists for
profiling, plan 0 as the streams from before the plan, and the executor beside a one-rank communicator that was made first."""
import contextlib
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, noise_i16

pytestmark = pytest.mark.gpu

CFG = "afsk_1200_ax25_super_opt.json"
N = 60000                                                     # samples per recording: about 29 workgroups of the fused launch
PM_ERR_ARG = -2


@contextlib.contextmanager
def queue_plan(ctx, plan):
    """pipe_queue_plan on the (shared) context for the body, what it held before afterwards."""
    before = ctx.tuned("pipe_queue_plan")
    ctx.tune(pipe_queue_plan=plan)
    try:
        yield ctx
    finally:
        ctx.tune(pipe_queue_plan=before)


def _priority_range():
    """hipDeviceGetStreamPriorityRange from the runtime the library itself has loaded -> (lowest, highest); numerically lower = higher."""
    from pymodem_amd._native import lib
    lib()
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert paths, "the library has no HIP runtime loaded"
    hip = ctypes.CDLL(sorted(paths)[0])
    lo, hi = ctypes.c_int(0), ctypes.c_int(0)
    assert hip.hipDeviceGetStreamPriorityRange(ctypes.byref(lo), ctypes.byref(hi)) == 0
    return lo.value, hi.value


def _priority(handle):
    from pymodem_amd._native import check, lib
    v = ctypes.c_int(12345)
    check(lib().pm_ctx_stream_priority(handle, ctypes.byref(v)))
    return v.value


def _recordings(count):
    """`count` recordings of N samples with different seeded contents: a packet or two in noise, each at another level."""
    from pymodem_amd import siggen
    out = []
    for k in range(count):
        sig = siggen.recording("afsk1200_ax25", 48000, packets=2, seed=100 + k, noise_sigma=500.0 + 150.0 * k, payload_len=(10, 30))[0]
        a = noise_i16(N, seed=200 + k, sigma=500.0 + 150.0 * k)
        m = min(N, len(sig))
        a[:m] = sig[:m]
        out.append(a)
    return out


@pytest.fixture(scope="module")
def seven(config_lines):
    """Seven recordings and, computed once, what process_chains_device makes of each: slicer bytes and addresses, packet rows."""
    from pymodem_amd import chain_builder as cb, chain_execute as ce
    lines = config_lines(CFG)
    recs = _recordings(7)
    want = []
    for a in recs:
        st = {}
        rows = ce.process_chains_device([cb.build_chain(48000, l) for l in lines], a, stages=st, _rows=True)
        rows = [np.array(r) for r in rows]
        for c, r in enumerate(rows):                          # (the pipeline stamps a packet with its chain's place in the config)
            r["source_decoder"] = c
        want.append(([(np.array(s.data), np.array(s.address)) for s in st["sliced"]], rows))
    assert sum(len(r) for _, rows in want for r in rows) >= 20              # (the recordings do carry packets)
    assert len({w[0][0][0].tobytes() for w in want}) == 7                   # (and differ)
    return lines, recs, want


def _same_rows(got, want):
    return np.array_equal(got, want) or (
        len(got) == len(want) and all(np.array_equal(got[f], want[f]) for f in got.dtype.names if f != "correlated_count"))


def test_three_priority_levels():
    """pm_ctx_create_prio at -1, 0 and 1: low >= normal >= high numerically, all different whenever the device reports a range; levels 2
    and -2 are refused (PM_ERR_ARG) and make nothing; every context made goes away again."""
    from pymodem_amd._native import check, lib
    L = lib()
    lo, hi = _priority_range()
    got = {}
    for level in (-1, 0, 1):
        h = ctypes.c_void_p()
        check(L.pm_ctx_create_prio(0, level, ctypes.byref(h)))
        assert h.value
        got[level] = _priority(h)
        check(L.pm_ctx_sync(h))
        assert L.pm_ctx_destroy(h) == 0
    print("priority range", lo, hi, "levels", got)
    assert got[-1] >= got[0] >= got[1]
    if lo != hi:
        assert len(set(got.values())) == 3
        assert got[-1] == lo and got[1] == hi
    else:
        assert len(set(got.values())) == 1
    for level in (2, -2):
        h = ctypes.c_void_p()
        assert L.pm_ctx_create_prio(0, level, ctypes.byref(h)) == PM_ERR_ARG
        assert not h.value                                    # refused before anything was made


@pytest.mark.parametrize("plan", [1, 0])
def test_every_recording_is_handed_over(seven, plan):
    """Slots 2, group 2: slots, counter cells and both demod streams are reused within seven recordings.  Each recording is uploaded on the
    caller's stream behind a 64 MB device-to-device copy queued there, and submitted with no synchronise in between: a demod stream that
    did not wait for the caller's stream at the submission would read the buffer before the audio is in it.  Slicer bytes, addresses and
    packets equal process_chains_device's on the same audio; afterwards the profiling contexts have counted seven fused launches."""
    import pymodem_amd
    from pymodem_amd import chain_builder as cb, chain_execute as ce
    from pymodem_amd._native import check, lib
    lines, recs, want = seven
    ctx = pymodem_amd.Context.default()
    big = 64 << 20
    src, dst = ctx.empty(big, np.uint8), ctx.empty(big, np.uint8)
    bufs = [ctx.empty(N, np.int16) for _ in recs]
    for b in bufs:                                            # stale contents: another recording's worth of zeros
        check(lib().pm_memset(ctx.handle, b.ptr, 0, N * 2))
    ctx.sync()
    with queue_plan(ctx, plan):
        pipe = ce.NativePipeline([cb.build_chain(48000, l) for l in lines], N, 48000 / 40, ctx=ctx, slots=2, slice_group=2, keep_slices=True)
    sides = pipe.side_contexts()
    watched = [ctx] + sides
    handles = [c.handle.value for c in watched]
    assert len(set(handles)) == len(handles)                  # every context once, the caller's only as the caller's
    for c in watched:
        c.profile(True)
    tickets = []
    for a, b in zip(recs, bufs):
        check(lib().pm_d2d(ctx.handle, dst.ptr, src.ptr, big))
        check(lib().pm_h2d(ctx.handle, b.ptr, a.ctypes.data_as(ctypes.c_void_p), a.nbytes))
        tickets.append(pipe.submit(b))
    for k, t in enumerate(tickets):
        w_sliced, w_rows = want[k]
        kept = [pipe.slices(t, c) for c in range(len(lines))]
        rows = pipe.rows(t)
        for c in range(len(lines)):
            assert np.array_equal(kept[c][0].data, w_sliced[c][0]), (plan, k, c)
            assert np.array_equal(kept[c][0].address, w_sliced[c][1]), (plan, k, c)
            assert _same_rows(rows[c], w_rows[c]), (plan, k, c)
        del rows, kept
    fused = 0
    for c in watched:
        fused += c.profile_read()["fir_f64"][1]
        c.profile(False)
    assert fused == 7
    own, side = _streams(pipe)
    assert set(handles[1:]) == set(side) | (set(own) - {ctx.handle.value})      # all the pipeline owns, and nothing of the caller's
    pipe.close()
    ctx.sync()
    del src, dst, bufs


def _streams(pipe):
    """(demod contexts, slicer contexts) of a default pipeline as the library names them: two of each."""
    from pymodem_amd._native import lib
    own = [lib().pm_pipe_demod_ctx(pipe._h, i) for i in range(2)]
    side = [lib().pm_pipe_side_ctx(pipe._h, i) for i in range(2)]
    assert all(own) and all(side) and not lib().pm_pipe_demod_ctx(pipe._h, 2) and not lib().pm_pipe_side_ctx(pipe._h, 2)
    assert len(set(own + side)) == 4
    return own, side


@pytest.mark.parametrize("plan", [1, 0])
def test_where_the_plan_makes_the_streams(config_lines, plan):
    """Plan 0 makes what the executor made before the plan: demod[0] IS the caller's stream, demod[1] a plain stream, the slicers at the
    highest level.  Plan 1: both demod streams the pipeline's own at the lowest level.  In every plan the slicers are strictly above."""
    import pymodem_amd
    from pymodem_amd import chain_builder as cb, chain_execute as ce
    lines = config_lines(CFG)
    ctx = pymodem_amd.Context.default()
    with queue_plan(ctx, plan):
        pipe = ce.NativePipeline([cb.build_chain(48000, l) for l in lines], N, 48000 / 40, ctx=ctx)
    assert ctx.tuned("pipe_queue_plan") == int(os.environ.get("PM_PIPE_QUEUE_PLAN", "1"))
    own, side = _streams(pipe)
    pri = {"demod": [_priority(h) for h in own], "slicer": [_priority(h) for h in side], "caller": _priority(ctx.handle)}
    print("plan", plan, pri)
    lo, hi = _priority_range()
    if plan == 0:
        assert own[0] == ctx.handle.value
        assert pri["demod"] == [pri["caller"]] * 2
    else:
        assert ctx.handle.value not in own
        assert pri["demod"] == [lo, lo]
    assert pri["slicer"] == [hi, hi]
    if lo != hi:
        assert max(pri["slicer"]) < min(pri["demod"])
    pipe.close()


CHILD = r'''
import json, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
if sys.argv[2] == "comm":
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    opts = dist.ProcessGroupNCCL.Options()
    opts.is_high_priority_stream = True
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0), pg_options=opts)
import pymodem_amd
from pymodem_amd import chain_builder as cb, chain_execute as ce
import test_gpu_queue_plan as T
with open(os.path.join(sys.argv[1], "tests", "golden", "configs", T.CFG)) as f:
    lines = [l for l in (json.loads(s) for s in f if s.strip()) if l.get("object_type") == "demod_chain"]
recs = T._recordings(3)
ctx = pymodem_amd.Context.default()
pipe = ce.NativePipeline([cb.build_chain(48000, l) for l in lines], T.N, 48000 / 40, ctx=ctx, keep_slices=True)
bufs = [ctx.upload(a) for a in recs]                          # (resident until the recordings are sliced)
tickets = [pipe.submit(b) for b in bufs]
out = {}
for k, t in enumerate(tickets):
    for c in range(len(lines)):
        sl, plain = pipe.slices(t, c)
        out[f"d{k}_{c}"], out[f"a{k}_{c}"] = np.array(sl.data), np.array(sl.address)
    for c, r in enumerate(pipe.rows(t)):
        out[f"r{k}_{c}"] = np.array(r).view(np.uint8)
pipe.close()
np.savez(sys.argv[3], **out)
if sys.argv[2] == "comm":
    dist.destroy_process_group()
print("CHILD OK", len(out))
'''


def test_beside_a_communicator(tmp_path):
    """A one-rank process group (RCCL, a high-priority stream asked for, as the benchmark does) made first in a fresh child process, then
    three recordings through the executor: what comes out equals the same three in a child without a communicator."""
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    res = {}
    for mode in ("plain", "comm"):
        env = dict(os.environ, RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29400 + os.getpid() % 500),
                   HSA_ENABLE_IPC_MODE_LEGACY="0")
        out = tmp_path / f"{mode}.npz"
        p = subprocess.run([sys.executable, str(script), ROOT, mode, str(out)], env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and "CHILD OK" in p.stdout, (mode, p.stderr[-3000:])
        res[mode] = np.load(out)
    assert sorted(res["plain"].files) == sorted(res["comm"].files) and len(res["plain"].files) == 3 * 8 * 3
    assert sum(len(res["plain"][k]) for k in res["plain"].files if k.startswith("r")) > 0
    for k in res["plain"].files:
        assert np.array_equal(res["plain"][k], res["comm"][k]), k
