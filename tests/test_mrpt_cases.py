"""CPU: every case of tests/mrpt_cases.py reaches the edge it was built for, shown on the model (oracle/mrpt.c through
oracle.mrpt_build(..).export() / knn2, and the numpy model of tests/test_gpu_ann_knn.py); the numpy model equals orc_mrpt_knn2 at
k = 2 on every case; and four wrong variants of the model each change the expected output of a named case, so the GPU comparison
(tests/test_gpu_mrpt_edges.py) would notice a kernel that is wrong in that way.  The floors are asserted on the model's own numbers
and printed (pytest -s)."""
import numpy as np
import pytest

import mrpt_cases as M


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _proj(oracle, case):
    return M.project(M.index_of(oracle, case.name)[1]["R"], case.data)


@pytest.mark.parametrize("name", M.KNN_NAMES)
def test_numpy_model_is_the_restatement_at_k2(oracle, name):
    """rows, distance bits and n_elected of orc_mrpt_knn2; the first attempt's count is the answering one's where nothing was retried"""
    c = M.knn_cases()[name]
    mi, md, ne, cls, nf = M.expected(oracle, name, 2)
    ei, ed, ene = M.index_of(oracle, name)[0].knn2(c.queries, c.votes)
    assert np.array_equal(mi, ei) and np.array_equal(_bits(md), _bits(ed)) and np.array_equal(ne, ene)
    assert np.array_equal(nf[cls == 0], ne[cls == 0]) and (nf[cls == 1] < 2).all()
    assert ((mi < 0).all(axis=1) == (cls == 2)).all()


def test_self_odd_median_rows_meet_their_split(oracle):
    for c in M.family("self_odd"):
        ix, ex = M.index_of(oracle, c.name)
        n = len(c.data)
        assert ix.depth == 6 and len(np.unique(c.data, axis=0)) == n and ex["R"].any(axis=1).all()
        proj = _proj(oracle, c)
        nodes, equal = M.routes(ex, proj, ix.n_trees, ix.depth)              # the queries ARE the rows
        odd = [cut for cut in M.cuts(ex, proj, ix.n_trees, ix.depth) if cut[3] % 2]
        for t, level, node, _, vl, _, median in odd:
            assert nodes[median, t, level] == node and equal[median, t, level]
            assert _bits(vl) == _bits(ex["splits"][t, node])
        assert len(odd) >= 6 * ix.n_trees and equal.sum() >= len(odd)
        for k in M.KS:
            mi, md, _, cls, nf = M.expected(oracle, c.name, k)
            found = cls != 2
            assert np.array_equal(mi[found, 0], np.arange(n)[found]) and (md[found, 0] == 0).all()
            if k == 1:
                assert found.all() and (cls == 0).all() and nf.min() >= 1
        print(f"{c.name}: {len(odd)} odd nodes, {int(equal.sum())} equality visits")
    c = M.knn_cases()["self_odd-n129-d8-t1v1"]                                # 129 = 65 + 64: one odd node a level
    ex = M.index_of(oracle, c.name)[1]
    assert M.routes(ex, _proj(oracle, c), 1, 6)[1].sum() == 6


def test_ties_at_cuts_are_tied(oracle):
    for c in M.family("ties_at_cuts"):
        ix, ex = M.index_of(oracle, c.name)
        cuts = M.cuts(ex, _proj(oracle, c), ix.n_trees, ix.depth)
        tied = [cut for cut in cuts if cut[4] == cut[5]]
        tied_even = [cut for cut in tied if cut[3] % 2 == 0]
        distinct = len(np.unique(_bits(ex["splits"][0])))
        assert len(tied_even) >= 4 and len(tied) > len(tied_even) and distinct < ex["splits"].shape[1]
        for t, _, node, _, vl, _, _ in tied_even:
            assert _bits(ex["splits"][t, node]) == _bits(vl)                 # (vl + vl) / 2
        # a query on a tied cut: its projection equals the split
        _, equal = M.routes(ex, M.project(ex["R"], c.queries), ix.n_trees, ix.depth)
        assert equal.sum() >= 20
        print(f"{c.name}: {len(np.unique(c.data, axis=0))} distinct rows, {len(tied)} tied cuts of {len(cuts)} ({len(tied_even)} at even nodes), "
              f"{distinct} distinct splits of {ex['splits'].shape[1]} in tree 0, {int(equal.sum())} equality visits of the queries")


def test_constant_view_is_arranged_by_row(oracle):
    (c,) = M.family("constant_view")
    ix, ex = M.index_of(oracle, c.name)
    proj = _proj(oracle, c)
    assert (proj == proj[0]).all() and (ex["leaves"] == np.arange(len(c.data))).all()
    nodes, equal = M.routes(ex, M.project(ex["R"], c.queries), ix.n_trees, ix.depth)
    assert equal[0].all() and (nodes[0] == (1 << np.arange(ix.depth)) - 1).all()          # left at every node
    for k in M.KS:
        mi, md, _, cls, nf = M.expected(oracle, c.name, k)
        assert nf[0] == ex["leaf_first"][1] == 4 and cls[0] == 0
        assert np.array_equal(mi[0], np.arange(k)) and (md[0] == 0).all()                   # equal distances: ascending rows
    print(f"constant_view: first-attempt counts {M.expected(oracle, c.name, 2)[4].tolist()}, classes {M.expected(oracle, c.name, 2)[3].tolist()}")


def test_zero_vectors_split_by_row(oracle):
    (c,) = M.family("zero_vectors")
    ix, ex = M.index_of(oracle, c.name)
    zero = ~ex["R"].any(axis=1)
    assert len(zero) == 24 and zero.sum() >= 12 and not zero.all()
    assert (c.data < 0).any(axis=0).all() and (c.data > 0).any(axis=0).all()                # x * 0 of both signs
    checked = 0
    for t in range(ix.n_trees):
        for level, level_nodes in enumerate(M.node_ranges(len(c.data), ix.depth)[:ix.depth]):
            if zero[t * ix.depth + level]:
                for lo, ln in level_nodes:
                    nl = ln - ln // 2
                    assert ex["leaves"][t, lo:lo + nl].max() < ex["leaves"][t, lo + nl:lo + ln].min()
                    checked += 1
    assert checked >= 12
    print(f"zero_vectors: {int(zero.sum())} of {len(zero)} random vectors are zero; {checked} nodes split by row index alone")


def test_even_odd_levels_hold_both(oracle):
    odd_at, even_at, even_open = set(), set(), 0
    for c in M.family("even_odd_levels"):
        ix, ex = M.index_of(oracle, c.name)
        n = len(c.data)
        sizes = np.diff(ex["leaf_first"])
        assert ix.depth == 6 and sizes.sum() == n and np.array_equal(sizes, [ln for _, ln in M.node_ranges(n, 6)[6]])
        assert set(sizes.tolist()) <= {n // 64, n // 64 + 1}
        for t, level, node, ln, vl, vr, _ in M.cuts(ex, _proj(oracle, c), ix.n_trees, ix.depth):
            (odd_at if ln % 2 else even_at).add(level)
            if ln % 2 == 0 and vl != vr:
                even_open += 1
                assert _bits(ex["splits"][t, node]) == _bits(np.float32(np.float64(np.float32(vl + vr)) / 2.0))
    assert odd_at == even_at == set(range(6)) and even_open >= 100
    print(f"even_odd_levels: odd nodes at levels {sorted(odd_at)}, even at {sorted(even_at)}; {even_open} even nodes with vl != vr")


def test_sort_seams_take_every_cap(oracle):
    caps = [1 << int(np.ceil(np.log2(len(c.data)))) for c in M.family("sort_seams")]
    assert caps == [4096, 8192, 8192, 16384, 32768]
    for c in M.family("sort_seams"):
        assert len(c.queries) == 65 and (M.expected(oracle, c.name, 2)[3] == 0).all()
    print(f"sort_seams: caps {caps}")


def test_retry_counts_hold_every_tail(oracle):
    first = {k: np.zeros(4, np.int64) for k in M.KS}
    classes = {k: np.zeros(3, np.int64) for k in M.KS}
    for c in M.family("retry_counts"):
        for k in M.KS:
            _, _, ne, cls, nf = M.expected(oracle, c.name, k)
            print(f"{c.name} k {k}: first attempt {np.bincount(nf.astype(np.int64))[:6].tolist()}, answering {np.bincount(ne.astype(np.int64))[:6].tolist()}, "
                  f"classes {np.bincount(cls, minlength=3).tolist()}, distances measured {M.n_measured(c, k, ne, nf)}")
            if c.votes == 1:
                assert (cls == 0).all() and M.n_measured(c, k, ne, nf) == int(nf.sum())     # nothing is retried
            if c.votes > 2:
                first[k] += np.bincount(np.minimum(nf, 4).astype(np.int64), minlength=5)[:4]
                classes[k] += np.bincount(cls, minlength=3)
    for k in (2, 3):                                                                        # both tails: 1, 2 and 3 elected rows at once
        assert (first[k][1:] >= 3).all(), first[k]
        assert (classes[k] >= 3).all(), classes[k]                                          # answered at once, only by the retry, dropped
    assert (M.expected(oracle, "retry_counts-v26", 2)[4] == 1).sum() >= 3                   # one row at votes = n_trees: need - 1 is tried


def test_lane_counts_hold_64_and_65(oracle):
    for c in M.family("lane_counts"):
        mi, md, ne, cls, nf = M.expected(oracle, c.name, 2)
        hist = np.bincount(nf.astype(np.int64), minlength=66)
        assert hist[64] >= 10 and hist[65] >= 10 and hist[:64].sum() == 0 and (cls == 0).all()
        twice = (_bits(md[:, 0]) == _bits(md[:, 1])) & (md[:, 0] == 0)                      # one row twice among the elected
        assert (twice & (nf == 64)).sum() >= 5 and (twice & (nf == 65)).sum() >= 5
        assert (mi[twice, 1] == mi[twice, 0] + 1).all()                                    # the lower row is first
        print(f"{c.name}: elected {{64: {hist[64]}, 65: {hist[65]}}}, {int(twice.sum())} queries with two elected rows at distance 0")


def test_wide_narrow_and_waves_shapes(oracle):
    assert [c.data.shape[1] for c in M.family("wide_narrow")] == [4, 512]
    for c in M.family("wide_narrow"):
        cls = M.expected(oracle, c.name, 2)[3]
        assert (cls != 2).sum() >= 60
    for want, (c,) in ((2, M.family("waves_2")), (1, M.family("waves_1"))):
        per_wave, waves = M.launch_shape(len(c.data), c.n_trees, c.depth, c.votes)
        assert waves == want and per_wave <= 160 * 1024 and len(c.queries) == 97
        assert (M.expected(oracle, c.name, 2)[3] != 2).sum() >= 90
        print(f"{c.name}: {len(c.data)} rows, {per_wave} B a wavefront, waves {waves}")


def test_collections_reach_their_paths(oracle):
    col = M.collections_()
    c = col["unfit_view"]
    per_wave, _ = M.launch_shape(len(c.descs[0]), c.n_trees, c.depth, c.votes)
    assert per_wave > 160 * 1024 and M.launch_shape(len(c.descs[1]), c.n_trees, c.depth, c.votes)[0] <= 160 * 1024
    counts, matches = M.expected_collection(oracle, "unfit_view")
    assert counts[0] >= 100
    print(f"unfit_view: {per_wave} B a wavefront; {int(counts[0])} matches of the scan")
    c = col["mixed_batch"]
    sizes = [len(d) for d in c.descs]
    assert sizes == [60, 128, 129, 4097, 14000] and len(c.pairs) == 20
    assert M.launch_shape(max(sizes), c.n_trees, c.depth, c.votes)[1] == 2
    assert all(M.launch_shape(n, c.n_trees, c.depth, c.votes)[1] == 4 for n in sizes[1:4])
    counts, matches = M.expected_collection(oracle, "mixed_batch")
    assert (counts >= 30).all()
    print(f"mixed_batch: waves 2 for the batch, 4 for the views below 14,000 rows; matches per pair {counts.tolist()}")
    c = col["wide_narrow_u8"]
    assert all(d.dtype == np.uint8 and d.shape == (300, 64) for d in c.descs)
    counts, _ = M.expected_collection(oracle, "wide_narrow_u8")
    assert (counts >= 30).all()


# ---- the table has teeth: four wrong variants of the model, each changes what a named case expects
def test_strict_routing_changes_self_odd(oracle):
    """`<` for `<=`: the median row of an odd node goes right and misses its own leaf"""
    for name in ("self_odd-n129-d8-t1v1", "self_odd-n257-d16-t1v1"):
        right, wrong = M.expected(oracle, name, 1), M.expected(oracle, name, 1, route_strict=True)
        assert not np.array_equal(right[0], wrong[0])
        assert (wrong[0][:, 0] != np.arange(len(right[0]))).sum() >= 6
    # three trees, votes 3: the retry with votes 2 finds most of these rows again -- the distances measured tell (n_ann_dist)
    name = "self_odd-n257-d16-t3v3"
    c = M.knn_cases()[name]
    right, wrong = M.expected(oracle, name, 1), M.expected(oracle, name, 1, route_strict=True)
    assert M.n_measured(c, 1, right[2], right[4]) != M.n_measured(c, 1, wrong[2], wrong[4])
    name = "constant_view"
    assert not np.array_equal(M.expected(oracle, name, 2)[0], M.expected(oracle, name, 2, route_strict=True)[0])


def _model_index(oracle, name, **variant):
    c = M.knn_cases()[name]
    ix, ex = M.index_of(oracle, name)
    return ex, M.model_index(ex["R"], c.data, ix.n_trees, ix.depth, **variant)


@pytest.mark.parametrize("name", ["ties_at_cuts-n300", "constant_view", "zero_vectors", "even_odd_levels-n130", "self_odd-n255-d8-t3v3"])
def test_numpy_index_is_the_restatement(oracle, name):
    ex, (splits, leaves) = _model_index(oracle, name)
    assert np.array_equal(_bits(splits), _bits(ex["splits"])) and np.array_equal(leaves, ex["leaves"])


@pytest.mark.parametrize("name", ["ties_at_cuts-n300", "constant_view", "zero_vectors"])
def test_descending_ties_change_the_leaves(oracle, name):
    ex, (_, leaves) = _model_index(oracle, name, ties_descending=True)
    assert not np.array_equal(leaves, ex["leaves"])


@pytest.mark.parametrize("name", ["even_odd_levels-n128", "even_odd_levels-n192", "sort_seams-n4096"])
def test_left_value_at_even_nodes_changes_the_splits(oracle, name):
    ex, (splits, leaves) = _model_index(oracle, name, even_split_left=True)
    assert np.array_equal(leaves, ex["leaves"]) and not np.array_equal(_bits(splits), _bits(ex["splits"]))


@pytest.mark.parametrize("name", ["lane_counts-n258", "lane_counts-n4128", "constant_view"])
def test_rerank_ties_to_the_higher_row_change_the_rows(oracle, name):
    for k in M.KS:
        right, wrong = M.expected(oracle, name, k), M.expected(oracle, name, k, rerank_high=True)
        assert not np.array_equal(right[0], wrong[0]) and np.array_equal(_bits(right[1]), _bits(wrong[1]))
