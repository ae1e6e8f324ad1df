"""The f16 level in front of the pair-norm filter (l2_knn2_half_kernel: match mode, 128-dimensional rows, R <= 0.5; set_half_filter,
default on) on the views of pairnorm_filter_cases.py, prefix_prune_cases.py and half_filter_cases.py.  Every case runs
ctx.match_pairs with the switch on and off: both equal oracle.match_collection, and the graphs, prefix_pruning_counts and
pair_filter_counts are equal between on and off -- level 1 prunes a tile only if the filter would.  half_filter_counts is what the
numpy model says where the case is built for it (tests/test_half_filter_model.py shows on the CPU that each case holds what it is
built for), and 0 with the switch off."""
import importlib.util
import os

import numpy as np
import pytest

import half_filter_cases as HC
import pairnorm_filter_cases as FC
import prefix_prune_cases as PC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("prefix_prune_model", os.path.join(ROOT, "tools", "prefix_prune_model.py"))
M = importlib.util.module_from_spec(_spec); _spec.loader.exec_module(M)


def _graph(g):
    return np.array(g.pairs), np.array(g.offsets), np.array(g.matches)


def _run(ctx, oracle, views, ratio=0.6, pruning=True):
    """match (0, 1) with the f16 level on and off; both equal the oracle and each other, counters included
    -> ((tested, pruned), filtered, by level 1) with the level on"""
    pairs = np.array([[0, 1]], np.uint32)
    counts, matches = oracle.match_collection(views, None, pairs, ratio, True)
    ctx.clear_images()
    for i, v in enumerate(views):
        ctx.set_image(i, v)
    try:
        ctx.set_prefix_pruning(pruning)
        ctx.set_half_filter(True)
        g_on = ctx.match_pairs(pairs, ratio, True)
        on = ctx.prefix_pruning_counts(), ctx.pair_filter_counts(), ctx.half_filter_counts()
        ctx.set_half_filter(False)
        g_off = ctx.match_pairs(pairs, ratio, True)
        off = ctx.prefix_pruning_counts(), ctx.pair_filter_counts(), ctx.half_filter_counts()
    finally:
        ctx.set_half_filter(True)
        ctx.set_prefix_pruning(True)
        ctx.clear_images()
    print("on: (tested, pruned), filtered, by level 1", on, " off:", off)
    for g in (g_on, g_off):
        assert np.array_equal(g.pairs, pairs[counts > 0]) and np.array_equal(g.matches, matches)
    for x, y in zip(_graph(g_on), _graph(g_off)):
        assert np.array_equal(x, y)
    assert on[:2] == off[:2] and off[2] == 0, (on, off)
    assert on[2] <= on[1] <= on[0][1] <= on[0][0], on
    return on


def _named_views():
    out = []
    for nI, nJ in ((64, 70), (97, 130), (160, 130)):
        out.append((f"base_views {nI} x {nJ}", lambda nI=nI, nJ=nJ: PC.base_views(nI, nJ, seed=nI * 1000 + nJ), 0.6))
    out.append(("match_in_last_tile", lambda: PC.match_in_last_tile()[:2], 0.6))
    out.append(("runner_up_pruned", lambda: PC.runner_up_pruned()[:2], 0.6))
    out.append(("forced_fallback", lambda: PC.forced_fallback()[:2], 0.6))
    for case in ("seen_tie", "seen_below", "pruned_at_threshold", "pruned_above"):
        out.append((f"ratio_boundary {case}", lambda case=case: PC.ratio_boundary(case)[:2], 0.5))
    out.append(("swapped_pairs", lambda: FC.swapped_pairs()[:2], 0.6))
    out.append(("sparse match_in_last_tile", lambda: FC.match_in_last_tile()[:2], 0.6))
    out.append(("runner_up_filtered", lambda: FC.runner_up_filtered()[:2], 0.6))
    for kind in ("real", "large_integers"):
        out.append((f"other_rows {kind}", lambda kind=kind: FC.other_rows(kind), 0.6))
    for side in ("kept_above", "kept_below"):
        out.append((f"threshold_views {side}", lambda side=side: FC.threshold_views(M, side)[:2], 0.6))
    return out


NAMED = _named_views()


@pytest.mark.parametrize("name,make,ratio", NAMED, ids=[v[0] for v in NAMED])
def test_on_and_off_agree(ctx, oracle, name, make, ratio):
    """every older case: the oracle's graph either way, the cascade's counters either way"""
    a, b = make()
    cnt, filt, half = _run(ctx, oracle, [a, b], ratio=ratio)
    assert cnt[0] == ((b.shape[0] + 63) // 64) * ((a.shape[0] + 31) // 32)


@pytest.mark.parametrize("nI", [33, 96, 97, 160])
@pytest.mark.parametrize("nJ", [70, 100, 130])
def test_sparse_views(ctx, oracle, nI, nJ):
    """ragged sizes (a last tile of one row, a last query tile of a few): level 1 prunes every far tile for every wave, as the model
    says and as the filter does"""
    a, b = FC.sparse_views(nI, nJ, seed=nI * 1000 + nJ)
    cnt, filt, half = _run(ctx, oracle, [a, b])
    n = ((nJ + 63) // 64) * ((nI + 31) // 32 - 1)
    assert M.model_pair_levels(a, b, 12, 0.36)["half"] == n
    assert half == filt == cnt[1] == n, (cnt, filt, half)


@pytest.mark.parametrize("side,half_pruned", [("filter_only", 3), ("cleared", 4), ("missed", 3)])
def test_bound_at_the_threshold(ctx, oracle, side, half_pruned):
    """a planted row against the thresholds: `filter_only` is threshold_views("pruned"), 1.5 slacks above thrF in the f32 bound and
    some hundred below it in the f16 bound -- the filter prunes its tile, level 1 does not; `cleared` lies 1.5 margins above thrH in
    the f16 bound (level 1 prunes), `missed` half a margin below it (level 1 lets the tile through, the filter prunes it)"""
    a, b = FC.threshold_views(M, "pruned")[:2] if side == "filter_only" else HC.half_threshold_views(M, side)[:2]
    cnt, filt, half = _run(ctx, oracle, [a, b])
    assert filt == cnt[1] == 4 and half == half_pruned, (cnt, filt, half)
    if side != "cleared":
        assert half < filt


@pytest.mark.parametrize("kind", HC.RANGE_KINDS)
def test_range(ctx, oracle, kind):
    """pair norms beyond f16's range, below its normal range, one huge row among normal ones, negative values, a NaN: the oracle's
    graph and the cascade's counters; the overflowing view gets nothing from level 1"""
    a, b = HC.range_views(kind)
    cnt, filt, half = _run(ctx, oracle, [a, b])
    model = M.model_pair_levels(a, b, 12, 0.36)
    print("model:", {k: model[k] for k in ("tiles", "pruned", "filtered", "half")})
    if kind == "scaled_up":
        assert half == 0 and filt == 3 * 3
    if kind in ("negative", "nan"):
        assert half == filt == (2 if kind == "nan" else 3) * 3


def test_without_pruning_every_counter_is_zero(ctx, oracle):
    a, b = FC.sparse_views(97, 130, seed=5)
    cnt, filt, half = _run(ctx, oracle, [a, b], pruning=False)
    assert cnt == (0, 0) and filt == 0 and half == 0


def test_the_parents_path_runs_beyond_the_switchs_reach(ctx, oracle):
    """R just above kPruneMaxR (ratio 0.71: R = 0.5041 > 0.5) and 64-dimensional rows: the plain kernel runs, no tile is tested"""
    a, b = FC.sparse_views(97, 130, seed=6)
    cnt, filt, half = _run(ctx, oracle, [a, b], ratio=0.71)
    assert cnt == (0, 0) and filt == 0 and half == 0
    rng = np.random.default_rng(8)
    b = rng.integers(0, 200, (130, 64)).astype(np.float32)
    a = rng.integers(0, 200, (97, 64)).astype(np.float32)
    a[:4] = b[:4] + np.float32(1.0)
    cnt, filt, half = _run(ctx, oracle, [a, b])
    assert cnt == (0, 0) and filt == 0 and half == 0
