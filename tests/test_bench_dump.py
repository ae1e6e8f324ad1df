"""bench.py --dump-outputs, host side: the arrays written are the graphs of the step, exactly, in float32 (pairs, matches) and
float64 (offsets); above the size limit a fixed per-pair sample is written -- the same pairs in every graph and on every run."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _graphs():
    from regard3d_amd import api
    rng = np.random.default_rng(3)
    i, j = np.triu_indices(40, k=1)
    pairs = np.stack([i, j], 1).astype(np.uint32)
    counts = rng.integers(0, 400, len(pairs)).astype(np.uint64)
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    matches = rng.integers(0, 16384, (int(offs[-1]), 2)).astype(np.uint32)
    sub = np.arange(0, len(pairs), 3)
    f = api.Graph.from_csr(pairs[sub], np.concatenate([[0], np.cumsum(counts[sub])]).astype(np.uint64),
                           np.concatenate([matches[offs[k]:offs[k + 1]] for k in sub]))
    return {"putative": api.Graph.from_csr(pairs, offs, matches), "F": f}


def _load(d, name):
    p, o, m = (np.load(os.path.join(d, f"{name}_{w}.npy")) for w in ("pairs", "offsets", "matches"))
    assert p.dtype == np.float32 and o.dtype == np.float64 and m.dtype == np.float32
    return p.astype(np.uint32), o.astype(np.int64), m.astype(np.uint32)


def test_dump_is_the_graphs_exactly(tmp_path):
    import bench
    graphs = _graphs()
    info = bench.dump_outputs(str(tmp_path), graphs)
    assert info["pairs_fraction"] == 1.0
    assert sum(f.stat().st_size for f in tmp_path.iterdir()) == info["bytes"] <= bench.DUMP_LIMIT_BYTES
    for name, g in graphs.items():
        p, o, m = _load(str(tmp_path), name)
        assert np.array_equal(p, g.pairs) and np.array_equal(o, g.offsets.astype(np.int64)) and np.array_equal(m, g.matches)


def test_dump_above_the_limit_is_a_fixed_sample_of_pairs(tmp_path, monkeypatch):
    import bench
    graphs = _graphs()
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 200_000)
    a, b = tmp_path / "a", tmp_path / "b"
    info = bench.dump_outputs(str(a), graphs)
    bench.dump_outputs(str(b), graphs)
    assert 0 < info["pairs_fraction"] < 1.0
    assert sum(f.stat().st_size for f in a.iterdir()) == info["bytes"] <= 200_000
    kept = {}
    for name, g in graphs.items():
        p, o, m = _load(str(a), name)
        assert all(np.array_equal(x, y) for x, y in zip((p, o, m), _load(str(b), name)))       # the same sample on every run
        full = g.as_dict()
        assert 0 < len(p) < g.num_pairs
        for k, (I, J) in enumerate(p.tolist()):                                                # every sampled pair with all its matches
            assert np.array_equal(m[o[k]:o[k + 1]], full[(I, J)])
        kept[name] = set(map(tuple, p.tolist()))
    # the draw is per (I, J): a pair of the F graph is sampled exactly when it is sampled in the putative graph
    assert kept["F"] == kept["putative"] & set(map(tuple, graphs["F"].pairs.tolist()))
