"""The skip of level 2 in l2_knn2_half_kernel (a tile that objects at the f16 level and holds a finite f16 key at or below thrS = thrF - L
goes straight to the restart) on the views of level2_skip_cases.py and of the three older case files.  Every case runs ctx.match_pairs
with the f16 level on and off: both equal oracle.match_collection, the graphs, prefix_pruning_counts, pair_filter_counts and
half_filter_counts are what they are without the skip -- equal between on and off, half_filter_counts the model's -- and
level2_skip_counts is the numpy model's `skipped` where the case is built for it (tests/test_level2_skip_model.py shows on the CPU that
every key of such a case lies more than 5 from its threshold, float32 roundings below 0.1) and 0 with the level off."""
import functools

import numpy as np
import pytest

import level2_skip_cases as SC
import test_half_filter_model as HM

pytestmark = pytest.mark.gpu

M = HM.M


def _graph(g):
    return np.array(g.pairs), np.array(g.offsets), np.array(g.matches)


def _run(ctx, oracle, views, ratio):
    """match (0, 1) with the f16 level on and off; both equal the oracle and each other, the older counters included
    -> ((tested, pruned), filtered, by level 1, level 2 skipped) with the level on"""
    pairs = np.array([[0, 1]], np.uint32)
    counts, matches = oracle.match_collection(views, None, pairs, ratio, True)
    ctx.clear_images()
    for i, v in enumerate(views):
        ctx.set_image(i, v)
    try:
        ctx.set_half_filter(True)
        g_on = ctx.match_pairs(pairs, ratio, True)
        on = ctx.prefix_pruning_counts(), ctx.pair_filter_counts(), ctx.half_filter_counts(), ctx.level2_skip_counts()
        ctx.set_half_filter(False)
        g_off = ctx.match_pairs(pairs, ratio, True)
        off = ctx.prefix_pruning_counts(), ctx.pair_filter_counts(), ctx.half_filter_counts(), ctx.level2_skip_counts()
    finally:
        ctx.set_half_filter(True)
        ctx.clear_images()
    print("on: (tested, pruned), filtered, by level 1, level 2 skipped", on, " off:", off)
    for g in (g_on, g_off):
        assert np.array_equal(g.pairs, pairs[counts > 0]) and np.array_equal(g.matches, matches)
    for x, y in zip(_graph(g_on), _graph(g_off)):
        assert np.array_equal(x, y)
    assert on[:2] == off[:2] and off[2] == 0 and off[3] == 0, (on, off)
    assert on[3] <= on[0][0] - on[2] and on[2] <= on[1] <= on[0][1] <= on[0][0], on
    return on


@functools.lru_cache(maxsize=None)
def _new_cases():
    return {name: (a, b) for name, a, b, _ in SC.all_cases(M)}


NEW = [f"band_views {side}" for side in SC.BAND_SIDES] + [f"block_views {name}" for name, _ in SC.block_cases(M)] + ["lowered_views"]


@pytest.mark.parametrize("ratio", [0.6, 0.7])
@pytest.mark.parametrize("name", NEW)
def test_skip_counts_are_the_models(ctx, oracle, name, ratio):
    """the cases built for the skip, at R = 0.36 and 0.49: the oracle's graph, the counters of the kernel without the skip, and the
    model's count of tiles that went from level 1 straight to the restart"""
    a, b = _new_cases()[name]
    cnt, filt, half, skipped = _run(ctx, oracle, [a, b], ratio)
    model = M.model_pair_levels(a, b, 12, ratio * ratio, skip="lane")
    print("model:", {k: model[k] for k in ("tiles", "pruned", "filtered", "half", "skipped", "gap")})
    assert cnt == (model["tiles"], model["pruned"]) and filt == model["filtered"] and half == model["half"]
    assert skipped == model["skipped"]


OLDER = [v for v in HM.VIEWS]


@pytest.mark.parametrize("name,a,b,R", OLDER, ids=[v[0] for v in OLDER])
def test_older_cases_keep_their_counters(ctx, oracle, name, a, b, R):
    """every case of the three older files: the oracle's graph either way, the older counters equal between on and off (the skip moves
    none of them), and no skip where every key of level 1 is beyond f16's range"""
    cnt, filt, half, skipped = _run(ctx, oracle, [a, b], round(float(np.sqrt(R)), 6))
    assert cnt[0] == ((b.shape[0] + 63) // 64) * ((a.shape[0] + 31) // 32)
    if name == "range_views scaled_up":
        assert skipped == 0 and half == 0 and filt == 3 * 3
