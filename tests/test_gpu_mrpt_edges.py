"""The MRPT arm (kernels_mrpt.hip, api_mrpt.cpp) on the forests and queries of tests/mrpt_cases.py (`-m gpu`): the index, r3dm_mrpt_knn2,
r3dm_mrpt_knn at k = 1 and 3, r3dm_match_pairs_mrpt -- every query of every case against the CPU model with np.array_equal, distances and
splits by their bits, and the distance counter n_ann_dist EQUAL to the model's elected rows of both attempts.  Which edge a case is for
and why it reaches it: the case module's header; that it does: tests/test_mrpt_cases.py."""
import numpy as np
import pytest

from regard3d_amd import api

import mrpt_cases as M

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _params(c):
    return api.MrptParams(c.n_trees, c.depth, c.votes, c.density, c.seed)


def _register(ctx, descs, xys=None):
    ctx.clear_images()
    for v, d in enumerate(descs):
        ctx.set_image(v, d, None if xys is None else xys[v])


@pytest.mark.parametrize("name", M.KNN_NAMES)
def test_index_equals_the_cpu_model(ctx, oracle, name):
    c = M.knn_cases()[name]
    ix, ex = M.index_of(oracle, name)
    _register(ctx, [c.data])
    g = ctx.mrpt_index(0, len(c.data), c.data.shape[1], _params(c))
    ctx.clear_images()
    assert g["depth"] == ix.depth
    assert np.array_equal(_bits(g["R"]), _bits(ex["R"]))
    assert np.array_equal(g["leaf_first"], ex["leaf_first"])
    assert np.array_equal(_bits(g["splits"]), _bits(ex["splits"]))
    assert np.array_equal(g["leaves"], ex["leaves"])


@pytest.mark.parametrize("k", M.KS)
@pytest.mark.parametrize("name", M.KNN_NAMES)
def test_neighbours_equal_the_cpu_model(ctx, oracle, name, k):
    """k = 2: r3dm_mrpt_knn2 (the 2-NN tail); k = 1, 3: r3dm_mrpt_knn (the k-list tail)"""
    c = M.knn_cases()[name]
    mi, md, ne, cls, nf = M.expected(oracle, name, k)
    gi, gd = ctx.mrpt_knn2(c.data, c.queries, _params(c)) if k == 2 else ctx.mrpt_knn(c.data, c.queries, _params(c), k)
    measured = ctx.stats().n_ann_dist
    assert np.array_equal(gi, mi)
    assert np.array_equal(_bits(gd), _bits(md))
    assert measured == M.n_measured(c, k, ne, nf)
    if c.family == "self_odd" and k == 1:                     # every row finds itself (asserted on the model in test_mrpt_cases.py)
        assert np.array_equal(gi[:, 0], np.arange(len(c.data))) and (gd[:, 0] == 0).all()


def test_rejected_lengths_still_refuse(ctx):
    rng = np.random.default_rng(1)
    for dim in (2, 6, 516):
        d = np.ascontiguousarray(rng.standard_normal((256, dim)), np.float32)
        for call in (lambda: ctx.mrpt_knn2(d, d[:4], api.MrptParams.preset()), lambda: ctx.mrpt_knn(d, d[:4], api.MrptParams.preset(), 3)):
            with pytest.raises(api.R3dmError, match=r"-> -5:"):
                call()


def _graph_equals(g, pairs, counts, matches):
    keep = counts > 0
    return (np.array_equal(g.pairs, pairs[keep]) and np.array_equal(np.diff(g.offsets.astype(np.int64)), counts[keep])
            and np.array_equal(g.matches, matches))


def _collection_params(c):
    return api.MrptParams(c.n_trees, c.depth, c.votes, -1.0, 0)


def test_u8_collection_equals_the_cpu_model(ctx, oracle):
    c = M.collections_()["wide_narrow_u8"]
    counts, matches = M.expected_collection(oracle, c.name)
    _register(ctx, c.descs, c.xys)
    g = ctx.match_pairs_mrpt(c.pairs, c.ratio, _collection_params(c))
    built = ctx.stats().n_ann_built
    ctx.clear_images()
    assert built == 3 and _graph_equals(g, c.pairs, counts, matches)


def test_unfit_view_is_scanned(ctx, oracle):
    c = M.collections_()["unfit_view"]
    counts, matches = M.expected_collection(oracle, c.name)            # the exhaustive arm's model: ratio^2 on squared distances
    _register(ctx, c.descs, c.xys)
    g = ctx.match_pairs_mrpt(c.pairs, c.ratio, _collection_params(c))
    built = ctx.stats().n_ann_built
    scan = ctx.match_pairs(c.pairs, c.ratio, True)
    ctx.clear_images()
    assert built == 0
    assert _graph_equals(g, c.pairs, counts, matches)
    assert np.array_equal(g.pairs, scan.pairs) and np.array_equal(g.offsets, scan.offsets) and np.array_equal(g.matches, scan.matches)
    for call in (lambda: ctx.mrpt_knn2(c.descs[0], c.descs[1], _collection_params(c)), lambda: ctx.mrpt_knn(c.descs[0], c.descs[1], _collection_params(c), 3)):
        with pytest.raises(api.R3dmError, match=r"-> -5:"):
            call()


def test_mixed_batch_equals_the_cpu_model(ctx, oracle):
    c = M.collections_()["mixed_batch"]
    counts, matches = M.expected_collection(oracle, c.name)
    mp = _collection_params(c)
    _register(ctx, c.descs, c.xys)
    g = ctx.match_pairs_mrpt(c.pairs, c.ratio, mp)
    built = ctx.stats().n_ann_built
    g2 = ctx.match_pairs_mrpt(c.pairs, c.ratio, mp)                      # served by the cached forests
    built2 = ctx.stats().n_ann_built
    ctx.clear_images()
    assert built == 4 and built2 == 0                                   # (the 60-row view is scanned)
    assert _graph_equals(g, c.pairs, counts, matches)
    assert _graph_equals(g2, c.pairs, counts, matches)
    fresh = api.Context(0)
    try:
        _register(fresh, c.descs, c.xys)
        g3 = fresh.match_pairs_mrpt(c.pairs, c.ratio, mp)
        assert fresh.stats().n_ann_built == 4
        assert _graph_equals(g3, c.pairs, counts, matches)
    finally:
        fresh.close()
