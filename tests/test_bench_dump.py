"""bench.py --dump-outputs: the packet table of the timed path's last step as .npy files (host-only; the GPU run is test_gpu_chains)."""
import os

import numpy as np

import bench
from pymodem_amd._native import packet_dtype
from pymodem_amd.packet_meta import PacketTable


def make_table(chains=3, per_chain=5, seed=0):
    """Each chain decodes the same packets a few samples apart: the de-dup folds them into `per_chain` unique ones."""
    rng = np.random.default_rng(seed)
    rows = {}
    lens = rng.integers(1, 300, per_chain)
    payloads = [rng.integers(0, 256, n) for n in lens]
    for c in range(chains):
        r = np.zeros(per_chain, dtype=packet_dtype())
        r["streamaddress"] = np.arange(per_chain) * 100_000 + 10 * c + (1 << 40)
        r["len"] = lens
        r["valid_crc"] = r["valid_header"] = 1
        for k in range(per_chain):
            r["data"][k, :lens[k]] = payloads[k]
        rows[c] = r
    return PacketTable(rows, [f"chain {c}" for c in range(chains)]).correlate(1200.0), np.concatenate(payloads)


def load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_is_exact(tmp_path):
    table, payloads = make_table()
    bench.dump_outputs(table, str(tmp_path))
    got = load(tmp_path)
    assert set(got) == {"packets_header", "packets_payload", "chain_counts", "unique_rows", "unique_decoders"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    h = got["packets_header"]
    assert h.shape == (15, 1 + len(bench.HEAD_FIELDS))
    assert np.array_equal(h[:, 0], np.arange(15))
    for j, f in enumerate(bench.HEAD_FIELDS):
        assert np.array_equal(h[:, j + 1], table.heads[f].astype(np.float64)), f
    assert h[0, 1] == float(1 << 40)                                   # stream addresses past 2^32 survive
    assert np.array_equal(got["packets_payload"], np.tile(payloads, 3).astype(np.float32))
    assert np.array_equal(got["chain_counts"], [5, 5, 5])
    assert np.array_equal(got["unique_rows"], table.unique_idx)
    assert got["unique_decoders"].shape == (5, 3) and np.all(got["unique_decoders"] == 1)


def test_dump_over_the_limit_is_a_fixed_sample(tmp_path, monkeypatch):
    table, _ = make_table(chains=4, per_chain=50)
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 20_000)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(table, str(a))
    bench.dump_outputs(table, str(b))
    ga, gb = load(a), load(b)
    assert sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a)) <= 20_000 + 5 * 128      # (+ the .npy headers)
    keep = ga["packets_header"][:, 0].astype(np.int64)
    assert 0 < len(keep) < 200 and np.all(np.diff(keep) > 0)
    assert len(ga["packets_payload"]) == int(table.heads["len"][keep].sum())
    assert all(np.array_equal(ga[k], gb[k]) for k in ga)


def test_dump_of_no_result(tmp_path):
    bench.dump_outputs(None, str(tmp_path))
    got = load(tmp_path)
    assert got["packets_header"].shape == (0, 1 + len(bench.HEAD_FIELDS)) and got["packets_payload"].size == 0
