"""What tests/test_oracle_loop_edges.py and tests/test_gpu_loop_edges.py share: the fixtures tests/golden/make_loop_edges.py made from
the reference (loop_edges.npz, loop_edges_recordings.npz, loop_edges_summary.json) and the oracle's loops run over them, whole or in pieces."""
import json
import os

import numpy as np

from conftest import GOLDEN
from oracle import oracle as O

SUMMARY = json.load(open(os.path.join(GOLDEN, "loop_edges_summary.json")))
CASES = SUMMARY["cases"]
LOOPS = ("bpsk", "qpsk", "pll", "mpsk")
PARAMS = [f for f, _ in O.LoopState._fields_][:10]
STATE = [f for f, _ in O.LoopState._fields_][10:]
_NPZ = None
_CASE = {}


def fixture():
    global _NPZ
    if _NPZ is None:
        _NPZ = np.load(os.path.join(GOLDEN, "loop_edges.npz"))
    return _NPZ


def recordings():
    """The degenerate recordings and the reference's modem outputs on them (a file of its own)."""
    if "rec" not in _CASE:
        _CASE["rec"] = np.load(os.path.join(GOLDEN, "loop_edges_recordings.npz"))
    return _CASE["rec"]


def case(name):
    """{field: array} of one case (read once: every access to an .npz member decompresses it)."""
    if name not in _CASE:
        g = fixture()
        _CASE[name] = {k[len(name) + 2:]: g[k] for k in g.files if k.startswith(name + "__")}
        for a in _CASE[name].values():
            a.flags.writeable = False
    return _CASE[name]


def oracle_loop(c):
    """(LoopState, branch or None) at the case's initial state."""
    L = O.LoopState()
    for f, v in zip(PARAMS, c["params"]):
        setattr(L, f, float(v))
    for f, v in zip(STATE, c["state0"]):
        setattr(L, f, float(v))
    return L, (c["branch0"].copy() if "branch0" in c else None)


def oracle_run(kind, L, branch, x0, x1=None):
    """One call of the oracle's loop `kind` over a piece; (out0, out1 or None).  L and branch carry the state."""
    if kind == "bpsk":
        return O.costas_bpsk(L, x0), None
    if kind == "pll":
        return O.pll_afsk(L, x0), None
    if kind == "qpsk":
        return O.costas_qpsk(L, branch, x0)
    return O.mpsk_loop(L, x0, x1)


def cuts_of(name):
    """Piece boundaries every case is run with: whole, two pieces, three pieces, and the ones the generator asks for."""
    n = CASES[name]["n"]
    cuts = [[], [n // 2], [n // 3, 2 * n // 3]] + [list(s) for s in CASES[name]["splits"]]
    return [c for k, c in enumerate(cuts) if c not in cuts[:k] and all(0 < a < n for a in c)] if n > 1 else [[]]


def pieces(n, cuts):
    edges = [0] + list(cuts) + [n]
    return list(zip(edges[:-1], edges[1:]))


def oracle_case(name, cuts=()):
    """The oracle over the whole case, cut at `cuts` with the state carried: (out0, out1 or None, state[9], branch[9] or None)."""
    c = case(name)
    kind = CASES[name]["loop"]
    L, br = oracle_loop(c)
    o0, o1 = [], []
    for a, b in pieces(len(c["x0"]), cuts):
        p0, p1 = oracle_run(kind, L, br, c["x0"][a:b], c["x1"][a:b] if "x1" in c else None)
        o0.append(p0)
        o1.append(p1)
    state = np.array([getattr(L, f) for f in STATE])
    return np.concatenate(o0), (np.concatenate(o1) if o1[0] is not None else None), state, br
