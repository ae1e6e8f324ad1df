"""The pruning build of the f32 2-NN kernel (l2_knn2_prune_kernel: match mode, 128-dimensional rows, R <= 0.5) on views built for
its edges.  Every case compares ctx.match_pairs with oracle.match_collection and with the same call after set_prefix_pruning(False),
and reads from the counters that tiles were pruned (or, where the case says so, that the kernel did not run).

How a view is built (prefix_prune_cases.py): queries and the 32 rows of dataset tile 0 are integers in [30, 70] -- about 36,000 from
each other -- so every list is warm after tile 0; a FAR row adds 150 to its first 72 dimensions (at least 1.6 million away in any
prefix the kernel may test, 9 to 12 groups of 8), so a tile of far rows is pruned by every wave.  Rows placed at chosen distances
from a chosen query make the cases."""
import numpy as np
import pytest

import prefix_prune_cases as PC

pytestmark = pytest.mark.gpu


def _graph(g):
    return np.array(g.pairs), np.array(g.offsets), np.array(g.matches)


def _run(ctx, oracle, views, ratio=0.6, expect_pruned=True):
    """match (0, 1) with pruning on and off; both equal the oracle; -> (graph, counters with pruning on, stats with pruning on)"""
    pairs = np.array([[0, 1]], np.uint32)
    counts, matches = oracle.match_collection(views, None, pairs, ratio, True)
    ctx.clear_images()
    for i, v in enumerate(views):
        ctx.set_image(i, v)
    try:
        ctx.set_prefix_pruning(True)
        g_on = ctx.match_pairs(pairs, ratio, True)
        cnt = ctx.prefix_pruning_counts()
        stats = ctx.stats()
        ctx.set_prefix_pruning(False)
        g_off = ctx.match_pairs(pairs, ratio, True)
        assert ctx.prefix_pruning_counts() == (0, 0)
    finally:
        ctx.set_prefix_pruning(True)
        ctx.clear_images()
    for g in (g_on, g_off):
        assert np.array_equal(g.pairs, pairs[counts > 0]) and np.array_equal(g.matches, matches)
    for x, y in zip(_graph(g_on), _graph(g_off)):
        assert np.array_equal(x, y)
    if expect_pruned:
        n_waves = (views[1].shape[0] + 63) // 64
        n_tiles = (views[0].shape[0] + 31) // 32
        assert cnt[0] == n_waves * n_tiles and 0 < cnt[1] < cnt[0], cnt
    return g_on, cnt, stats


@pytest.mark.parametrize("nI", [64, 96, 97, 160])
@pytest.mark.parametrize("nJ", [70, 130])
def test_tile_counts(ctx, oracle, nI, nJ):
    """(a) even and odd tile counts (the loop's two tails), a last tile of one row, a last query tile of a few rows: every tile
    behind tile 0 is pruned by every wave"""
    a, b = PC.base_views(nI, nJ, seed=nI * 1000 + nJ)
    g, cnt, _ = _run(ctx, oracle, [a, b])
    n_waves = (nJ + 63) // 64
    assert cnt[1] == n_waves * ((nI + 31) // 32 - 1), cnt
    assert g.num_matches >= 3                          # base_views plants matches in tile 0


def test_match_behind_pruned_tiles(ctx, oracle):
    """(b) the matching row sits in the last tile, behind pruned ones: the query's wave runs that tile to the end"""
    a, b, q, row = PC.match_in_last_tile()
    g, cnt, _ = _run(ctx, oracle, [a, b])
    assert (np.array(g.matches) == [row, q]).all(1).any()
    assert cnt[1] == cnt[0] - 3 - 1                    # 3 waves x tile 0, and the one wave x the last tile


def test_runner_up_pruned(ctx, oracle):
    """(c) the match is seen in tile 0 and the TRUE runner-up sits in a tile that is then pruned"""
    a, b, q, best, second = PC.runner_up_pruned()
    d = PC.distances(a, b)[:, q]
    order = np.argsort(d, kind="stable")
    assert (order[0], order[1]) == (best, second)      # the case holds what it is built for
    g, cnt, stats = _run(ctx, oracle, [a, b])
    assert (np.array(g.matches) == [best, q]).all(1).any()
    assert cnt[1] == cnt[0] - 2                        # two waves x tile 0: the runner-up's tile was pruned
    assert stats.n_exact_fallback == 0


def test_forced_fallback(ctx, oracle):
    """(d) a pruned row shares its last 32 dimensions with the query and lies just above the threshold of its time; the apparent
    match arrives later and is too far for ea < R PL: the query takes the exact scan, which finds no match"""
    a, b, q, pruned_row, late_row = PC.forced_fallback()
    d = PC.distances(a, b)[:, q]
    R = np.float32(0.6) * np.float32(0.6)
    assert d[late_row] == d.min() and not d[late_row] < R * d[pruned_row]      # the brute-force verdict: no match
    g, cnt, stats = _run(ctx, oracle, [a, b])
    assert stats.n_exact_fallback >= 1
    assert not (np.array(g.matches)[:, 1] == q).any()


@pytest.mark.parametrize("case", ["seen_tie", "seen_below", "pruned_at_threshold", "pruned_above"])
def test_ratio_boundary(ctx, oracle, case):
    """(e) R = 0.25 (ratio 0.5, exact in float): ea == R eb against ea == R eb - 1 on seen rows; a row with R d == e0 exactly (at
    the threshold: not pruned, no match) against one a unit farther (pruned, match)"""
    a, b, q, best, matched = PC.ratio_boundary(case)
    g, cnt, _ = _run(ctx, oracle, [a, b], ratio=0.5)
    assert bool((np.array(g.matches) == [best, q]).all(1).any()) == matched


@pytest.mark.parametrize("kind", ["real", "large_integers"])
def test_rows_without_the_exactness_proof(ctx, oracle, kind):
    """(f) real-valued rows, and integer rows too large for the exactness proof: the thresholds carry the slack"""
    a, b = PC.base_views(160, 130, seed=77)
    if kind == "real":
        rng = np.random.default_rng(5)
        a = (a / np.float32(16.0) + rng.random(a.shape, np.float32) * np.float32(0.01)).astype(np.float32)
        b = (b / np.float32(16.0) + rng.random(b.shape, np.float32) * np.float32(0.01)).astype(np.float32)
    else:
        a = a * np.float32(2.0); b = b * np.float32(2.0)
        assert 128.0 * float(a.max()) ** 2 >= 2.0 ** 24
    g, cnt, _ = _run(ctx, oracle, [a, b])
    assert g.num_matches >= 3


def test_switched_off(ctx, oracle):
    """(g) a ratio near 1 and the raw 2-NN run the kernel they ran before: 0 tiles tested, results the oracle's"""
    a, b = PC.base_views(160, 130, seed=78)
    _, cnt, _ = _run(ctx, oracle, [a, b], ratio=0.999, expect_pruned=False)
    assert cnt == (0, 0)
    idx, dist = ctx.knn2(a, b)
    assert ctx.prefix_pruning_counts() == (0, 0)
    oidx, odist = oracle.knn2(a, b)
    ok = odist[:, 0] != odist[:, 1]
    assert np.array_equal(idx[ok], oidx[ok]) and np.array_equal(dist, odist)
