"""The host arithmetic the certified AFSK sweeps' decision rests on (csrc/pm_afsk_sweep.h) without a GPU: afsk_sweep_core_check.cpp
evaluates the bound E, the matrix-pipe constants, the dynamic-LDS layouts of the fused kernels and the route -- which launch a sweep,
and a group of sweeps, takes -- for the headline config's two sweeps, the 8 kHz / 300 baud shape of test_one_chain_certified_signs_are_the_exact_chain_s and the edges (ml = 113 / 114, m = 2,
long correlators), and every number must be the one recorded in golden/afsk_sweep_core.json from the expressions the launchers
carried before they shared this header (its "about" says how).  A wrong E or layout fails no bitmap test: the bitmaps stay the
oracle's and only the count of uncertain samples, or the launch path, moves; the same holds for every condition of the route."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

CASE_KEYS = ("name", "m", "ml", "mb", "kb", "one", "gmax", "lpf_abs_sum", "x_bound", "tap_dev", "e_x", "S", "tapq_int", "qabs", "dlow")
GROUP_KEYS = ("planned", "aligned", "afsk_split")
ROUTE_KEYS = ("name", "m", "ml", "groups", "tones", "mb", "plan_ml", "own_list", "afsk_unfused", "afsk_lpf8", "sweep_no_tail")
DIRECT, SLIDE, FUSED64, FUSED8 = range(4)                      # pm_sweep::SweepRoute
BAND, LIST, MAXIMA = 2 * 3 * 64 * 16, (48 + 4) * 4, 32        # bytes behind the templates: band operands, workgroup list, wave maxima


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "afsk_sweep_core.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def got(tmp_path_factory, golden):
    """name -> {key: value as printed} from the checker, run once"""
    if shutil.which("g++") is None:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("afsk_sweep_core")
    exe = d / "afsk_sweep_core_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(ROOT, "pymodem_amd", "csrc"),
                           os.path.join(ROOT, "tests", "afsk_sweep_core_check.cpp"), "-o", str(exe)])
    lines = [str(len(golden["cases"]))] + [" ".join(str(c[k]) for k in CASE_KEYS) for c in golden["cases"]]
    lines += [str(len(golden["groups"]))]
    lines += [f"{g['name']} {g['kb']} {g['mb']} {len(g['sweeps'])} " + " ".join(f"{m} {ml} {one}" for m, ml, one in g["sweeps"]) + " " +
              " ".join(str(g[k]) for k in GROUP_KEYS) for g in golden["groups"]]
    lines += [str(len(golden["routes"]))] + [" ".join(str(r[k]) for k in ROUTE_KEYS) for r in golden["routes"]]
    (d / "cases.txt").write_text("\n".join(lines) + "\n")
    run = subprocess.run([str(exe), str(d / "cases.txt")], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    out = {}
    for line in run.stdout.splitlines():
        tok = line.split()
        out[tok[0]] = dict(t.split("=") for t in tok[1:])
    assert set(out) == set(golden["expected"])
    return out


def _num(s):
    return float.fromhex(s) if "x" in s else int(s)


def test_the_cases_are_the_configs_own(golden):
    """The recorded inputs are what the headline config and the one-chain test give on this machine: lengths and gains exactly, the sums
    of taps to a few units in the last place (a sum's order is numpy's)."""
    import test_gpu_certified_edges as CE
    from pymodem_amd import taps as T
    by = {c["name"]: c for c in golden["cases"]}
    sweeps = CE._sweeps(CE._lines())
    assert sorted(len(chains) for chains, *_ in sweeps) == [1, 7]
    for chains, gains, mark, unit, lpf, bpf, m in sweeps:
        c = by["headline_one" if len(chains) == 1 else "headline_seven"]
        assert (c["m"], c["ml"], c["mb"], c["one"]) == (m, len(lpf), len(bpf), int(len(chains) == 1)) and m == (40 if len(chains) == 1 else 60)
        assert c["kb"] == (3 if len(bpf) + 15 <= 192 else 4)                      # pm_bpf8_plan_create's blocks
        assert float.fromhex(c["gmax"]) == max(gains)
        assert float.fromhex(c["lpf_abs_sum"]) == pytest.approx(float(np.abs(lpf).sum()), rel=1e-14)
        assert float.fromhex(c["x_bound"]) == pytest.approx(float(np.abs(bpf).sum()) * 32768.0, rel=1e-14)
        mk, sp = T.tone_model(*mark), T.tone_model(*unit)
        assert float.fromhex(c["tap_dev"]) == pytest.approx(max(mk[2], sp[2]), rel=1e-3) and float.fromhex(c["tap_dev"]) < 1e-13
    c = by["rate8000_baud300"]
    mi = T.afsk_tone_correlators(8000.0, 300.0, 1600.0, 1800.0, 1.0, 1.0, 0.0)[0]
    assert (c["m"], c["ml"], c["one"]) == (len(mi), round(8000.0 * 2.5 / 300.0) | 1, 1) and float.fromhex(c["x_bound"]) == 4.0e4
    assert {by[k]["ml"] for k in ("ml113", "ml114")} == {113, 114} and by["m2"]["m"] == 2
    for c in golden["cases"]:
        assert 0.0 < float.fromhex(c["e_x"]) < 1e-6 * float.fromhex(c["x_bound"]), c["name"]


def test_every_number_is_the_one_the_launchers_computed(golden, got):
    """E without and with a band-pass error, for runs of 12 and of 16 and for the direct sums; the matrix-pipe constants; every number
    of both kernels' layouts: equal, bit for bit, to what sweep_signs' and afsk_group_run_fused's own expressions gave."""
    for name, want in golden["expected"].items():
        for key, value in want.items():
            if key in ("E12x_f", "E12_f0", "E12_s0"):
                continue                                          # the second copy's values: the next two tests
            assert _num(got[name][key]) == _num(value), (name, key, got[name][key], value)


def test_both_copies_of_the_bound_were_this_one(golden, got):
    for c in golden["cases"]:
        want = golden["expected"][c["name"]]
        assert _num(want["E12x_f"]) == _num(want["E12x"]) == _num(got[c["name"]]["E12x"]), c["name"]
        assert _num(got[c["name"]]["E12"]) < _num(got[c["name"]]["E12x"]) and _num(got[c["name"]]["E0"]) < _num(got[c["name"]]["E12"]) < _num(got[c["name"]]["E16"])


def test_no_band_pass_error_is_the_path_without_a_source(golden, got):
    """e_x = 0 through the widening (as afsk_group_run_fused and a sweep_signs with a source worked it out) is the E of a sweep
    without a source, bit for bit."""
    for c in golden["cases"]:
        want = golden["expected"][c["name"]]
        assert _num(want["E12_f0"]) == _num(want["E12_s0"]) == _num(want["E12"]) == _num(got[c["name"]]["E12"]), c["name"]


def _check_layout(L, prefix, m4_bytes, tail, name):
    g = lambda k: int(L[prefix + k])
    window, planes = 8 * g("xw_doubles"), g("plane_bytes")
    if g("off_planes") == 0:                                      # split kernel: the planes lie over the window
        assert 8 * g("region0") == max(window, planes), name
    else:                                                         # fused kernel: window, then planes
        assert g("off_planes") == window and 8 * g("region0") == window + planes, name
    # disjoint, in the stated order, and the total is the sum of the parts
    assert g("off_tpl") == 8 * g("region0") and g("off_band") == g("off_tpl") + m4_bytes and g("off_list") == g("off_band") + BAND, name
    assert g("off_max") == g("off_list") + LIST and g("lds") == g("off_max") + MAXIMA, name
    # ds_read_b128 of the planes and the band operands: 16-byte boundaries (off them the split kernel ran four times slower)
    assert g("off_planes") % 16 == 0 and g("off_band") % 16 == 0 and g("off_list") % 4 == 0 and g("off_max") % 4 == 0, name
    assert g("lds_ok") == int(tail <= g("region0")), name


def _tail(m, ml, mb):
    return 2 * ml + 2 * (ml + m - 1) + 2 * mb + 4 * m              # sweep_tail_entry's work space, in doubles


def test_the_layouts_hold_together(golden, got):
    for c in golden["cases"]:
        L = got[c["name"]]
        assert int(L["tail"]) == _tail(c["m"], c["ml"], c["mb"])
        assert int(L["runs"]) == -(-(2048 + c["ml"] - 1) // 12)
        _check_layout(L, "sp0_", 32 * c["m"], _tail(c["m"], c["ml"], 0), c["name"])
        _check_layout(L, "sp_", 32 * c["m"], _tail(c["m"], c["ml"], c["mb"]), c["name"])
        assert int(L["sp_plane_bytes"]) == (1 if c["one"] else 2) * 3 * 2176
    for g in golden["groups"]:
        L = got[g["name"]]
        mmax = max(m for m, _, _ in g["sweeps"])
        assert int(L["mmax"]) == mmax and int(L["xs_span"]) == max(-(-(2048 + ml - 1) // 12) * 12 + m - 1 for m, ml, _ in g["sweeps"])
        _check_layout(L, "", 32 * mmax, max(_tail(m, ml, g["mb"]) for m, ml, _ in g["sweeps"]), g["name"])
        # two audio digit planes fit where the low-pass planes come later; a plane holds what the band-pass's last tile reads
        assert int(L["plane_bytes"]) >= max(2 * int(L["aplane"]), (2 if not all(one for _, _, one in g["sweeps"]) else 1) * 3 * 2176)
        assert int(L["aplane"]) % 16 == 0 and int(L["aplane"]) >= -(-int(L["xs_span"]) // 256) * 256 + 64 * g["kb"] - 16
    # both outcomes of lds_ok and of the 64 KiB limit are among the cases
    assert {int(got[c["name"]]["sp_lds_ok"]) for c in golden["cases"]} == {0, 1}
    assert {int(got[g["name"]]["lds_ok"]) for g in golden["groups"]} == {0, 1}
    assert int(got["group_m1000"]["lds"]) > 65536 and not int(got["group_m1000"]["fuses"])


def test_the_headline_group_takes_the_fused_launch(golden, got):
    """The headline config's two sweeps behind its own band-pass qualify for the one-launch path, in either order: at most 64 KiB of LDS,
    low-passes the matrix-pipe tile is written for (the last is ml = 113), a run per lane at most.  A layout that outgrew this would
    send the headline to the split path without failing anything else."""
    by = {c["name"]: c for c in golden["cases"]}
    for name in ("group_headline", "group_headline_swapped"):
        g = [x for x in golden["groups"] if x["name"] == name][0]
        assert sorted(map(tuple, g["sweeps"])) == sorted((by[k]["m"], by[k]["ml"], by[k]["one"]) for k in ("headline_one", "headline_seven"))
        assert g["mb"] == by["headline_one"]["mb"] and g["kb"] == by["headline_one"]["kb"]
        assert int(got[name]["fuses"]) == 1 and int(got[name]["lds"]) <= 64 * 1024 and int(got[name]["lds_ok"]) == 1
    assert int(got["group_ml113"]["fuses"]) == 1 and int(got["group_ml114"]["fuses"]) == 0
    assert int(got["group_ml114"]["lds"]) <= 64 * 1024, "it is the low-pass length that refuses ml = 114, not the LDS"


def test_the_fused_binary64_kernels_lds_holds_together(golden, got):
    """afsk_slide_lpf_kernel's block: the window of x in runs of 12 with a pad slot each (later the space image), the mark image in
    the FIR's padded layout, four templates."""
    for c in golden["cases"]:
        L = got[c["name"]]
        nmag = 2048 + c["ml"] - 1
        window = int(L["runs"]) * 12 + c["m"] - 1
        image = nmag + nmag // 8
        assert int(L["fuse_image"]) % 2 == 0 and image + 2 <= int(L["fuse_image"]) <= image + 3, c["name"]
        assert int(L["fuse_region0"]) % 2 == 0 and 0 <= int(L["fuse_region0"]) - max(window + window // 12 + 2, image + 2) <= 1, c["name"]
        assert int(L["fuse_lds"]) == 8 * (int(L["fuse_region0"]) + int(L["fuse_image"]) + 4 * c["m"]), c["name"]


def test_every_route_and_both_outcomes_of_every_condition_occur(golden, got):
    """The recorded routes (test_every_number_is_the_one_the_launchers_computed compares them) cover the launchers' whole decision:
    each case below names the one condition that sends it where it goes."""
    R = {r["name"]: {k: int(v) for k, v in got[r["name"]].items()} for r in golden["routes"]}
    assert {x["route"] for x in R.values()} == {DIRECT, SLIDE, FUSED64, FUSED8}
    for key in ("one", "call_plan", "lds_ok", "ends"):
        assert {x[key] for x in R.values()} == {0, 1}, key
    where = {"direct_no_tones": DIRECT, "direct_one_group_no_tones": DIRECT, "direct_m1": DIRECT,            # no tone templates; m == 1
             "slide_lpf_1026": SLIDE, "fused64_lpf_1025": FUSED64,                                            # sweep_runs(ml) > 256 or not
             "slide_m2200": SLIDE, "fused64_m2000": FUSED64,                                                  # more than 120 KiB of LDS or not
             "slide_unfused": SLIDE, "slide_unfused_planned": SLIDE, "fused64_plain": FUSED64,                # afsk_unfused
             "fused8_call_plan": FUSED8, "fused64_call_plan_ml114": FUSED64,                                  # afsk_lpf8, and ml + 15 <= 128
             "fused64_plan_other_ml": FUSED64, "fused64_plan_other_ml_lpf8_switch": FUSED64,                  # a plan of another length
             "route_ml113": FUSED8, "route_ml114": FUSED64, "fused8_ring": FUSED8}
    for name, route in where.items():
        assert R[name]["route"] == route, name
    by = {r["name"]: r for r in golden["routes"]}
    assert by["slide_lpf_1026"]["ml"] - by["fused64_lpf_1025"]["ml"] == 1 and -(-(2048 + 1025 - 1) // 12) == 256      # a run per lane at most

    def fuse_lds(m, ml):
        nmag, window = 2048 + ml - 1, -(-(2048 + ml - 1) // 12) * 12 + m - 1
        even = lambda v: (v + 1) // 2 * 2
        return 8 * (even(max(window + window // 12 + 2, nmag + nmag // 8 + 2)) + even(nmag + nmag // 8 + 2) + 4 * m)
    assert fuse_lds(by["fused64_m2000"]["m"], 100) <= 120 * 1024 < fuse_lds(by["slide_m2200"]["m"], 100)
    # one stream: one chain AND sliding sums
    assert R["fused64_one"]["one"] and R["slide_unfused_one"]["one"] and not R["direct_one_group_no_tones"]["one"] and not R["direct_m1"]["one"]
    assert not R["fused64_plain"]["one"]
    # the call's own plan only where the matrix pipe takes the sweep and the caller brought none
    assert R["fused8_call_plan"]["call_plan"] and not R["fused64_call_plan_ml114"]["call_plan"] and not R["fused64_plan_other_ml_lpf8_switch"]["call_plan"]
    assert not R["direct_no_tones_lpf8_switch"]["call_plan"] and not R["route_headline_seven"]["call_plan"]
    # the workgroups' own exact chain: the layout's room, and sweep_no_tail
    assert R["fused8_ring"]["lds_ok"] and not R["fused8_no_tail"]["lds_ok"] and not R["route_m400"]["lds_ok"] and not R["fused8_m400_no_source"]["lds_ok"]
    for r in golden["routes"]:
        x = R[r["name"]]
        # no launch behind the sweep: the matrix pipe with the recording's own list, nothing else
        assert x["ends"] == int(x["route"] == FUSED8 and r["own_list"] == 1), r["name"]
        assert x["route"] == FUSED8 or not (x["lds_ok"] or x["call_plan"]), r["name"]
        assert x["route"] >= SLIDE or not x["one"], r["name"]


def test_a_sweeps_route_agrees_with_its_layout(golden, got):
    """lds_ok of a matrix-pipe sweep is the split kernel's layout's (with the band-pass taps of its source) unless sweep_no_tail."""
    for c in golden["cases"]:
        x = got["route_" + c["name"]]
        if int(x["route"]) == FUSED8:
            assert int(x["lds_ok"]) == int(got[c["name"]]["sp_lds_ok"]), c["name"]


def test_the_group_launch_needs_every_condition(golden, got):
    """group_fuses: the layout's verdict and nothing that asks for the launches apart -- every condition refuses at least one group
    that would otherwise take the single launch."""
    takes = {g["name"]: int(got[g["name"]]["takes"]) for g in golden["groups"]}
    for g in golden["groups"]:
        plain = g["planned"] and g["aligned"] and not g["afsk_split"] and g["kb"] in (3, 4)
        assert takes[g["name"]] == int(bool(plain) and int(got[g["name"]]["fuses"]) == 1), g["name"]
    assert takes["group_headline"] == takes["group_headline_swapped"] == takes["group_headline_kb4"] == 1
    for name in ("group_unplanned", "group_unaligned", "group_split", "group_kb5", "group_ml114", "group_m1000"):
        assert takes[name] == 0, name
    for name in ("group_unplanned", "group_unaligned", "group_split"):
        assert int(got[name]["fuses"]) == 1, name + ": it is the named condition that refuses it, not the layout"
    # the headline's sweeps, as the pipeline submits them, each take the matrix pipe and end without a launch of their own
    for name in ("route_headline_one", "route_headline_seven"):
        assert (int(got[name]["route"]), int(got[name]["lds_ok"]), int(got[name]["ends"])) == (FUSED8, 1, 1), name
