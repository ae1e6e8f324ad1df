"""The min form of l2_knn2_half_kernel's tile tests (r3dm_set_min_tile_test, default on: the minimum of a lane's 16 keys, folded by a
v_min3_f32 tree, answers the level-1 objection and the skip of level 2; the level-2 test and the restart's prefix test likewise) against
the general form on every case of the four case tables, on planted rows at every input of the tree, on padding rows and dead lanes, and
at the edge of the rule that admits a batch (every view's max |row|^2 below 2^28).  Every case runs ctx.match_pairs with the switch on
and off: graphs, the exact-scan query count and the five counters are equal, and min_tile_test_counts says which form ran."""
import functools

import numpy as np
import pytest

import half_filter_cases as HC
import level2_skip_cases as SC
import min_tile_test_cases as MC
import pairnorm_filter_cases as FC
import test_half_filter_model as HM

pytestmark = pytest.mark.gpu

M = HM.M


def _graph(g):
    return np.array(g.pairs), np.array(g.offsets), np.array(g.matches)


def _counters(ctx):
    return (ctx.prefix_pruning_counts(), ctx.pair_filter_counts(), ctx.half_filter_counts(), ctx.level2_skip_counts(),
            int(ctx.stats().n_exact_fallback))


def _run(ctx, views, ratio, pairs=((0, 1),), min_form=None):
    """match `pairs` with the switch on and off: equal graphs, equal counters; the min form ran with the switch on iff `min_form` (None:
    iff the rule holds for the views), never with it off
    -> ((tested, pruned), filtered, by level 1, level 2 skipped, exact-scan queries)"""
    pairs = np.array(pairs, np.uint32)
    if min_form is None:
        min_form = MC.rule_holds(*views)
    ctx.clear_images()
    for i, v in enumerate(views):
        ctx.set_image(i, v)
    try:
        ctx.set_min_tile_test(True)
        g_on = ctx.match_pairs(pairs, ratio, True)
        on, forms_on = _counters(ctx), ctx.min_tile_test_counts()
        ctx.set_min_tile_test(False)
        g_off = ctx.match_pairs(pairs, ratio, True)
        off, forms_off = _counters(ctx), ctx.min_tile_test_counts()
    finally:
        ctx.set_min_tile_test(True)
        ctx.clear_images()
    print("on: (tested, pruned), filtered, by level 1, level 2 skipped, exact scan", on, "forms", forms_on, " off:", off, "forms", forms_off)
    for x, y in zip(_graph(g_on), _graph(g_off)):
        assert np.array_equal(x, y)
    assert on == off, (on, off)
    assert forms_on == ((len(pairs), 0) if min_form else (0, len(pairs))), (forms_on, min_form)
    assert forms_off == (0, len(pairs)), forms_off
    return on


def _model(a, b, R=0.36):
    m = M.model_pair_levels(a, b, 12, R, skip="lane")
    print("model:", {k: m[k] for k in ("tiles", "pruned", "filtered", "half", "skipped", "gap")})
    return m


# ---- 1. on and off agree on every case of the four tables
ALL = HM.VIEWS + SC.all_cases(M)


@pytest.mark.parametrize("name,a,b,R", ALL, ids=[v[0] for v in ALL])
def test_on_and_off_agree(ctx, name, a, b, R):
    rule = name not in ("range_views scaled_up", "range_views huge_row", "range_views nan", "other_rows nan")
    assert MC.rule_holds(a, b) == rule
    cnt = _run(ctx, [a, b], round(float(np.sqrt(R)), 6), min_form=rule)
    assert cnt[0][0] == ((b.shape[0] + 63) // 64) * ((a.shape[0] + 31) // 32)


# ---- 2. every input of the tree: the one key that decides a tile in each of the 16 registers x both lane halves x both query tiles
@functools.lru_cache(maxsize=None)
def _planted(kind):
    """(a, b, q, row) with one planted row in tile 1 (lane half 0), tile 0 near and never pruned, every other row far.  (Three tiles,
    not two: the far rows of tile 2 hold the views' largest norm, which the planted distance is calibrated against.)"""
    if kind in ("cleared", "missed"):
        return HC.half_threshold_views(M, kind)[:4]
    return SC.band_views(M, kind)


POSITIONS = [(p, nj) for nj in (0, 1) for p in range(32)]


@pytest.mark.parametrize("p,nj", POSITIONS)
@pytest.mark.parametrize("side", ["missed", "cleared"])
def test_every_input_of_the_tree(ctx, side, p, nj):
    """`missed`: the one key at or below thrH sits at row position p of tile 1 in query tile nj -- a tree that drops that input prunes
    the tile at level 1; `cleared`, the mirror: the same key a margin ABOVE thrH, no key objects, level 1 prunes the tile"""
    a, b, q, row = MC.moved(*_planted(side), p, nj)
    cnt = _run(ctx, [a, b], 0.6)
    m = _model(a, b)
    assert m["gap"] > 1.0
    assert cnt[2] == m["half"] == (4 if side == "cleared" else 3)
    assert cnt[:4] == ((m["tiles"], m["pruned"]), m["filtered"], m["half"], m["skipped"])


# ---- 3. the skip of level 2 from the same minimum
@pytest.mark.parametrize("p,nj", POSITIONS)
@pytest.mark.parametrize("side", ["below", "inside"])
def test_skip_from_the_same_minimum(ctx, side, p, nj):
    """`below`: the one key at or below thrS at position p, query tile nj -- the tile skips level 2; `inside`: the tile's minimum lies
    between thrS and thrH -- it objects and does not skip"""
    a, b, q, row = MC.moved(*_planted(side), p, nj)
    cnt = _run(ctx, [a, b], 0.6)
    m = _model(a, b)
    assert m["gap"] > 1.0 and m["unsound"] == 0
    assert cnt[3] == m["skipped"] == (1 if side == "below" else 0)
    assert not m["tile_half"][1, 0]                      # the tile objects either way
    assert cnt[:4] == ((m["tiles"], m["pruned"]), m["filtered"], m["half"], m["skipped"])


# ---- 4. padding rows (+inf keys: neither object nor skip) and dead lanes / a partial query tile
@pytest.mark.parametrize("nJ", [33, 130])
@pytest.mark.parametrize("nI", [33, 63, 97])
def test_padding_and_dead_lanes(ctx, nI, nJ):
    a, b = FC.sparse_views(nI, 130, seed=nI * 1000 + nJ)
    b = b[:nJ].copy()
    cnt = _run(ctx, [a, b], 0.6)
    m = _model(a, b)
    assert cnt[:4] == ((m["tiles"], m["pruned"]), m["filtered"], m["half"], m["skipped"])
    assert cnt[2] == ((nJ + 63) // 64) * ((nI + 31) // 32 - 1)          # every tile behind tile 0 goes at level 1, its padding rows silent


# ---- 5. the rule's edge
@pytest.mark.parametrize("where", ["dataset", "query"])
@pytest.mark.parametrize("norm,min_form", [(2.0 ** 28 - 16, True), (2.0 ** 28, False), (2.0 ** 29, False)])
def test_the_rules_edge(ctx, norm, min_form, where):
    """max |row|^2 the largest float below the bound (all of it in one dimension pair), the bound, twice the bound"""
    a, b = MC.edge_views(norm, where)
    assert MC.rule_holds(a, b) == min_form
    _run(ctx, [a, b], 0.6, min_form=min_form)


def test_one_view_over_the_bound_takes_the_whole_batch(ctx):
    a, b = FC.sparse_views(97, 130, seed=48)
    c, _ = MC.edge_views(2.0 ** 28, "dataset")
    pairs = ((0, 1), (0, 2), (1, 2))
    _run(ctx, [a, b, c], 0.6, pairs=pairs, min_form=False)
    _run(ctx, [a, b, a[::-1].copy()], 0.6, pairs=pairs, min_form=True)
