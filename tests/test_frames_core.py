"""The per-word code of bitscan_frames_kernel (csrc/pm_bitscan_frames.h) without a GPU: frames_core_check.cpp steps a wave's lanes through
the kernel's trip on the host, and every frame of every stream must be the bit-serial model's (frames_model.py) at every trip length."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import frames_model as FM
from conftest import ROOT


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("frames_core")
    exe = d / "frames_core_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "pymodem_amd", "csrc"),
                           os.path.join(ROOT, "tests", "frames_core_check.cpp"), "-o", str(exe)])
    streams = FM.all_streams()
    events = 0
    with open(d / "streams.bin", "wb") as f:
        f.write(struct.pack("<i", len(streams)))
        for name in sorted(streams):
            plain = np.ascontiguousarray(streams[name])
            found = FM.frames_of(plain)
            events += len(found)
            f.write(struct.pack("<i", len(plain)) + plain.tobytes() + struct.pack("<i", len(found)))
            for P, F, frame in found:
                f.write(struct.pack("<qqi", P, F, -1 if frame is None else len(frame)) + (frame or b""))
    return str(exe), str(d / "streams.bin"), events


@pytest.mark.parametrize("words", [1, 2, 3, 7, 64])
def test_every_frame_is_the_model_s(checker, words):
    exe, path, events = checker
    run = subprocess.run([exe, path, str(words)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert run.stdout.strip().endswith(f"{events} events, 0 bad") and events >= 1258
