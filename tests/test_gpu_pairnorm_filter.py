"""The cascade of the pruning f32 2-NN kernel (l2_knn2_half_kernel<…, MODE 20>: the pair-norm filter in front of the prefix test; match mode,
128-dimensional rows, R <= 0.5) on views built for the filter's edges.  Every case compares ctx.match_pairs with
oracle.match_collection and with the same call after set_prefix_pruning(False), and reads both counters: the tiles pruned by any
test (prefix_pruning_counts) and those pruned by the filter (pair_filter_counts).

How a view is built (pairnorm_filter_cases.py): every row holds the same base in its first 96 dimensions -- every prefix distance is
0, the prefix test stops nothing -- and 16 one-sided pairs in its last 32; tile 0 and the queries are near rows, a far row lies
374,000 away of which its pair norms keep 102,400.  tests/test_pairnorm_filter_model.py shows on the CPU, with the numpy model of
the cascade, that each case holds what it is built for."""
import importlib.util
import os

import numpy as np
import pytest

import pairnorm_filter_cases as FC
import prefix_prune_cases as PC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("prefix_prune_model", os.path.join(ROOT, "tools", "prefix_prune_model.py"))
M = importlib.util.module_from_spec(_spec); _spec.loader.exec_module(M)


def _graph(g):
    return np.array(g.pairs), np.array(g.offsets), np.array(g.matches)


def _run(ctx, oracle, views, ratio=0.6):
    """match (0, 1) with pruning on and off; both equal the oracle; -> (graph, (tested, pruned), filtered, stats) with pruning on"""
    pairs = np.array([[0, 1]], np.uint32)
    counts, matches = oracle.match_collection(views, None, pairs, ratio, True)
    ctx.clear_images()
    for i, v in enumerate(views):
        ctx.set_image(i, v)
    try:
        ctx.set_prefix_pruning(True)
        g_on = ctx.match_pairs(pairs, ratio, True)
        cnt, filt = ctx.prefix_pruning_counts(), ctx.pair_filter_counts()
        stats = ctx.stats()
        ctx.set_prefix_pruning(False)
        g_off = ctx.match_pairs(pairs, ratio, True)
        assert ctx.prefix_pruning_counts() == (0, 0) and ctx.pair_filter_counts() == 0
    finally:
        ctx.set_prefix_pruning(True)
        ctx.clear_images()
    print("tested, pruned", cnt, "filtered", filt, "exact scans", stats.n_exact_fallback)
    for g in (g_on, g_off):
        assert np.array_equal(g.pairs, pairs[counts > 0]) and np.array_equal(g.matches, matches)
    for x, y in zip(_graph(g_on), _graph(g_off)):
        assert np.array_equal(x, y)
    n_waves = (views[1].shape[0] + 63) // 64
    n_tiles = (views[0].shape[0] + 31) // 32
    assert cnt[0] == n_waves * n_tiles and filt <= cnt[1] < cnt[0], (cnt, filt)
    return g_on, cnt, filt, stats


@pytest.mark.parametrize("nI", [33, 97])
@pytest.mark.parametrize("nJ", [70, 130])
def test_distance_in_the_last_dimensions(ctx, oracle, nI, nJ):
    """(a), (d) sparse rows whose distance lies in the last 32 dimensions, ragged sizes (a last tile of one row, a last query tile of a
    few): the filter prunes every tile behind tile 0 for every wave; a 96-dimension prefix alone could not (its distances are 0)"""
    a, b = FC.sparse_views(nI, nJ, seed=nI * 1000 + nJ)
    g, cnt, filt, stats = _run(ctx, oracle, [a, b])
    n = ((nJ + 63) // 64) * ((nI + 31) // 32 - 1)
    assert filt == n and cnt[1] == n, (cnt, filt)
    assert g.num_matches >= 3 and stats.n_exact_fallback == 0


def test_dense_rows(ctx, oracle):
    """(b) dense rows.  The far tiles of base_views go at the filter already (36 of a far row's pair norms lie 150 above a near
    row's); a dense row the filter cannot judge is the one of runner_up_pruned and forced_fallback, 16,200 away in 72 dimensions of
    which its pair norms keep about half: the filter lets its tile through, the prefix test prunes it, and the filter counter lies
    below the total"""
    a, b = PC.base_views(160, 130, seed=77)
    g, cnt, filt, _ = _run(ctx, oracle, [a, b])
    assert cnt[1] == 3 * 4 and g.num_matches >= 3
    a, b, q, best, second = PC.runner_up_pruned()
    g, cnt, filt, stats = _run(ctx, oracle, [a, b])
    assert cnt[1] == cnt[0] - 2 and filt == cnt[1] - 2 and stats.n_exact_fallback == 0, (cnt, filt)
    a, b, q, pruned_row, late_row = PC.forced_fallback()
    g, cnt, filt, stats = _run(ctx, oracle, [a, b])
    assert cnt[1] == 3 and filt == 1 and stats.n_exact_fallback >= 1, (cnt, filt)


def test_swapped_pairs(ctx, oracle):
    """(c) a row that is the query with the members of every pair swapped: bound 0, distance large.  Its tile goes on and finishes
    (the prefix distances of its far rows are 0), the result is the oracle's, and the filter sends nothing to the exact scan"""
    a, b, q, row = FC.swapped_pairs()
    g, cnt, filt, stats = _run(ctx, oracle, [a, b])
    assert filt == cnt[1] == cnt[0] - 2 - 1, (cnt, filt)
    assert stats.n_exact_fallback == 0
    assert not (np.array(g.matches)[:, 1] == q).any()


@pytest.mark.parametrize("kind", ["negative", "real", "large_integers", "nan"])
def test_rows_without_the_exactness_proof(ctx, oracle, kind):
    """(d) negative values, real-valued rows, integers too large for the exactness proof, and a NaN: the NaN keys object (the wave
    of the NaN query prunes nothing), every other wave prunes every tile behind tile 0"""
    a, b = FC.other_rows(kind)
    g, cnt, filt, _ = _run(ctx, oracle, [a, b])
    assert filt == cnt[1] == (2 if kind == "nan" else 3) * 3, (cnt, filt)
    assert g.num_matches >= 3


def test_match_behind_filtered_tiles(ctx, oracle):
    """(e) the matching row sits in the last tile, behind filtered ones: the query's wave runs that tile from its group 0 to the end"""
    a, b, q, row = FC.match_in_last_tile()
    g, cnt, filt, _ = _run(ctx, oracle, [a, b])
    assert (np.array(g.matches) == [row, q]).all(1).any()
    assert filt == cnt[1] == cnt[0] - 3 - 1, (cnt, filt)


def test_runner_up_filtered(ctx, oracle):
    """(e) the match is seen in tile 0 and the TRUE runner-up sits in a tile the filter then prunes"""
    a, b, q, best, second = FC.runner_up_filtered()
    g, cnt, filt, stats = _run(ctx, oracle, [a, b])
    assert (np.array(g.matches) == [best, q]).all(1).any()
    assert filt == cnt[1] == cnt[0] - 2, (cnt, filt)
    assert stats.n_exact_fallback == 0


@pytest.mark.parametrize("side,pruned", [("pruned", 4), ("kept_above", 3), ("kept_below", 3)])
def test_bound_at_the_threshold(ctx, oracle, side, pruned):
    """(f) a planted row whose pair-norm bound lies within two slacks of the threshold T its lane half holds: 1.5 slacks above (the
    filter prunes its tile), half a slack above (inside the slack: the tile goes on), 1.5 slacks below.  The row is built on the CPU
    from the model; whichever side the kernel's own rounding puts it on, the result is the oracle's"""
    a, b, q, row, T, s = FC.threshold_views(M, side)
    g, cnt, filt, stats = _run(ctx, oracle, [a, b])
    assert filt == cnt[1] == pruned, (cnt, filt)
    assert stats.n_exact_fallback == 0
