"""What decides pm_stream_scan's AX.25 event list (csrc/pm_bitscan_events.h) without a GPU: bitscan_core_check.cpp steps the tile
launch's lanes, the combine and the emit's lanes on the host, and the record and the list of every stream must be the bit-serial
model's (bitscan_model.py) at every tile size from 1 to 256 words.  The streams' own conditions -- which spans bail, what lies across
which tile boundary, how many events the frames launch's waves share -- are held here too, on the model."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import bitscan_model as M
import frames_model as FM
from conftest import ROOT


@pytest.fixture(scope="module")
def found():
    """name -> (events, bail_bit, last_flag) of the model, made once"""
    return {name: M.ax25_model(plain) for name, plain in FM.all_streams().items()}


@pytest.fixture(scope="module")
def checker(tmp_path_factory, found):
    if shutil.which("g++") is None:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("bitscan_core")
    exe = d / "bitscan_core_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "pymodem_amd", "csrc"),
                           os.path.join(ROOT, "tests", "bitscan_core_check.cpp"), "-o", str(exe)])
    streams = FM.all_streams()
    with open(d / "streams.bin", "wb") as f:
        f.write(struct.pack("<i", len(streams)))
        for name in sorted(streams):
            plain = np.ascontiguousarray(streams[name])
            events, bail, last_flag = found[name]
            frames = FM.frames_of(plain)
            assert [(P, F) for P, F, _ in frames] == events
            f.write(struct.pack("<i", len(plain)) + plain.tobytes() + struct.pack("<qqi", bail, last_flag, len(events)))
            for P, F, frame in frames:
                f.write(struct.pack("<IIi", P, F & 0xFFFFFFFF, int(frame is not None)))
    return str(exe), str(d / "streams.bin"), len(streams)


# 1: only the combine's carry; 2..255: lanes that scan, lanes that idle behind them and the carry; 125 / 126: the largest tile in which
# no span reaches the bail and the smallest in which one can; 256: the scan alone on every stream shorter than 2048 bytes
@pytest.mark.parametrize("tiles", [(1, 32), (33, 64), (65, 128), (129, 192), (193, 256)])
def test_record_and_list_are_the_model_s_at_every_tile_size(checker, tiles):
    exe, path, streams = checker
    run = subprocess.run([exe, path, str(tiles[0]), str(tiles[1])], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-2000:]
    runs = streams * (tiles[1] - tiles[0] + 1)
    # no lane's emit walk wanted a third event: the kernel has two places and would drop it silently
    assert run.stdout.strip().splitlines()[-1].startswith(f"{runs} runs, 0 mismatches, 0 lanes wanted a third event"), run.stdout[-3000:]
    assert run.stdout.strip().endswith("0 racing stores")


def test_every_list_fits_its_capacity(found):
    for name, plain in FM.all_streams().items():
        assert len(found[name][0]) <= len(plain) // 19 + 2, name


@pytest.mark.parametrize("S", M.SPANS)
@pytest.mark.parametrize("start", ["start", "flag"])
@pytest.mark.parametrize("kind", ["calm", "stuffed"])
def test_a_span_bails_from_8000_raw_bits_on(found, S, start, kind):
    plain = FM.all_streams()[f"span{S}_{start}_{kind}"]
    events, bail, _ = found[f"span{S}_{start}_{kind}"]
    begin = 19 if start == "flag" else 0                      # the first bit behind the two flags in front
    bits = np.unpackbits(plain)
    assert not bits[begin + S] and bits[begin + S - 6:begin + S].all() and not bits[begin + S - 7], "a flag's zero S bits behind the reset"
    stuffed = sum(bits[k - 5:k].all() and not bits[k - 6] and not bits[k] for k in range(begin + 6, begin + S - 7))
    assert stuffed == (21 if kind == "stuffed" else 0), "the counted bits are more than the margin short of the raw ones"
    in_front = [(10, -1)] if start == "flag" else []
    if S >= 8000:
        assert bail == begin + S and events == in_front, "nothing behind the bail is listed"
    else:
        assert bail == -1
        behind = [e for e in events if e[0] > begin + S]
        assert len(behind) == 1 and FM.frame_model(bits.tolist(), *behind[0]) is not None and len(FM.frame_model(bits.tolist(), *behind[0])) == 20, "the frame behind the span"
        # the flag that ends the span: the stream's first, or behind 7999 counted bits (7999 & 7 == 7) a closing one; behind 7978 it is neither
        assert len([e for e in events if e[0] == begin + S]) == (0 if (start, kind) == ("flag", "stuffed") else 1)


def test_the_late_bail_spans_a_whole_tile(found):
    events, bail, last_flag = found["late_bail"]
    assert len(FM.all_streams()["late_bail"]) >= 3 * 2048
    start = last_flag                                         # the flag in front of the span is the last one listed or not
    assert M.TILE_BITS - 64 <= start < M.TILE_BITS, "the span starts in the last word of the first tile"
    assert 2 * M.TILE_BITS <= bail < 3 * M.TILE_BITS and bail - start >= 8000, "and ends in the third"
    lens = [len(f) for _, _, f in FM.frames_of(FM.all_streams()["late_bail"]) if f is not None]
    assert 40 in lens and 25 in lens and 33 not in lens and 22 not in lens, "the frames in front are listed, those behind are not"


def test_the_straddling_pieces_lie_where_they_should(found):
    streams = FM.all_streams()
    marks = M.straddle_marks()
    assert len(marks) >= 5 and len(streams["straddle_flag"]) > 5 * 2048
    for name in ("straddle_flag", "straddle_stuffed", "straddle_run7", "straddle_bit151"):
        events, bail, _ = found[name]
        bits = np.unpackbits(streams[name])
        assert bail == -1, name
        listed = {P for P, _ in events}
        for at in marks:
            if name == "straddle_flag":                       # the zero of a flag that closes a 30-byte frame
                assert not bits[at] and bits[at - 6:at].all() and not bits[at - 7] and at in listed, at
            elif name == "straddle_stuffed":                  # a zero behind exactly five ones
                assert not bits[at] and bits[at - 5:at].all() and not bits[at - 6], at
            elif name == "straddle_run7":                     # the zero behind exactly seven ones
                assert not bits[at] and bits[at - 7:at].all() and not bits[at - 8], at
            else:                                             # the last one of the flag that closes an 18-byte frame
                assert bits[at] and not bits[at + 1] and at + 1 in listed, at
                P, F = [e for e in events if e[0] == at + 1][0]
                assert len(FM.frame_model(bits.tolist(), P, F)) == 18, at


def test_many_frames_give_a_wave_of_the_frames_launch_three(found):
    events, bail, _ = found["many_frames"]
    assert bail == -1 and len(events) >= 600                  # 256 waves share a job's events
    gaps = {P - F for P, F in events[1:]}
    assert min(gaps) >= 8 * 19 + 7 and len({g for g in gaps}) > 7, "frames of several lengths"
    two = sum(1 for (P0, _), (_, F1) in zip(events, events[1:]) if F1 - (P0 + 1) == 8)
    assert 100 < two < len(events) - 100, "one flag between some frames, two between others"


@pytest.mark.parametrize("r", range(8))
def test_the_padding_completes_nothing(found, r):
    for name, ones in (("five", 5), ("six", 6), ("seven", 7)):
        plain = FM.all_streams()[f"end{r}_{name}"]
        bits = np.unpackbits(plain)
        assert len(plain) == 8 * 4 + r + 1 and bits[-ones:].all() and not bits[-ones - 1]
        events, bail, last_flag = found[f"end{r}_{name}"]
        assert bail == -1 and last_flag < len(bits) - 8 and max(P for P, _ in events) < len(bits) - 8, "nothing at the stream's end is an event"


def test_first_flag_and_second_flag_share_a_word(found):
    events, _, last_flag = found["two_flags_one_word"]
    (P, F), = events
    assert F == -1 and (P - 7) >> 6 == (P + 8) >> 6 and last_flag == P + 9, "both flags in one 64-bit word, the first one listed"
    assert len(FM.frame_model(np.unpackbits(FM.all_streams()["two_flags_one_word"]).tolist(), P, F)) == 30
