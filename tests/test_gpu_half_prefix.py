"""The f16 prefix test of l2_knn2_half_kernel (r3dm_set_half_prefix, default on: a tile that gets to the restart first runs the restart's
96-dimension prefix test on the rows rounded to f16, thrQ = thr + marginQ, and is pruned there if no lane objects) on the views of
half_prefix_cases.py.  Every case runs ctx.match_pairs with the switch on and off: the graphs, tested / pruned / filtered / by level 1 /
skipped and the exact-scan query count are equal, the graph is the oracle's, and half_prefix_counts is the numpy model's count
(tests/test_half_prefix_rule.py shows on the CPU that every key of these cases lies further from its threshold than the float32
evaluation can move it) and (0, 0) with the switch off.  The raw 2-NN lists take no pruning kernel, so there is nothing of this test in
them: they are compared where the API returns them all the same."""
import functools

import numpy as np
import pytest

import half_prefix_cases as QC
import test_half_filter_model as HM

pytestmark = pytest.mark.gpu

M = HM.M


def _graph(g):
    return np.array(g.pairs), np.array(g.offsets), np.array(g.matches)


def _counters(ctx):
    return (ctx.prefix_pruning_counts(), ctx.pair_filter_counts(), ctx.half_filter_counts(), ctx.level2_skip_counts(),
            int(ctx.stats().n_exact_fallback))


def _run(ctx, oracle, views, ratio, pairs=((0, 1),)):
    """match `pairs` with the switch on and off: the oracle's graph both times, equal older counters
    -> (older counters, half_prefix_counts with the switch on)"""
    pairs = np.array(pairs, np.uint32)
    ctx.clear_images()
    for i, v in enumerate(views):
        ctx.set_image(i, v)
    try:
        ctx.set_half_prefix(True)
        g_on = ctx.match_pairs(pairs, ratio, True)
        on, q_on = _counters(ctx), ctx.half_prefix_counts()
        ctx.set_half_prefix(False)
        g_off = ctx.match_pairs(pairs, ratio, True)
        off, q_off = _counters(ctx), ctx.half_prefix_counts()
    finally:
        ctx.set_half_prefix(True)
        ctx.clear_images()
    print("on: (tested, pruned), filtered, by level 1, level 2 skipped, exact scan", on, "f16 prefix test (reached, pruned)", q_on, " off:", off, q_off)
    for x, y in zip(_graph(g_on), _graph(g_off)):
        assert np.array_equal(x, y)
    assert on == off, (on, off)
    assert q_off == (0, 0), q_off
    if oracle is not None:
        counts, matches = oracle.match_collection(views, None, pairs, ratio, True)
        assert np.array_equal(g_on.pairs, pairs[counts > 0]) and np.array_equal(g_on.matches, matches)
    return on, q_on


def _model(a, b, R=0.36):
    m = M.model_pair_levels(a, b, 12, R, skip="lane", prefix16=True)
    print("model:", {k: m[k] for k in ("tiles", "pruned", "filtered", "half", "skipped", "reach", "prefix_pruned", "prefix16", "between", "gap16")})
    return m


@functools.lru_cache(maxsize=None)
def _cases():
    return {name: (a, b, must) for name, a, b, _, must in QC.all_cases(M)}


NAMES = [c[0] for c in QC.all_cases(M)]


@pytest.mark.parametrize("name", NAMES)
def test_counts_are_the_models(ctx, oracle, name):
    """every case of the table at R = 0.36: on and off agree, the graph is the oracle's, and the counters -- the new one included -- are
    the model's"""
    a, b, must = _cases()[name]
    with_nan = bool(np.isnan(a).any() or np.isnan(b).any())
    on, q = _run(ctx, None if with_nan else oracle, [a, b], 0.6)
    m = _model(a, b)
    assert on[:4] == ((m["tiles"], m["pruned"]), m["filtered"], m["half"], m["skipped"])
    assert q == (m["reach"], m["prefix16"]) and (q[1] >= 1) == must


def test_raw_lists_are_untouched(ctx):
    """knn2 never takes a pruning kernel: the same lists either way, and no tile counted"""
    a, b = QC.oriented_views(97, 130, seed=73)
    try:
        out = []
        for on in (True, False):
            ctx.set_half_prefix(on)
            idx, dist = ctx.knn2(a, b)
            out.append((np.array(idx), np.array(dist)))
            assert ctx.half_prefix_counts() == (0, 0)
    finally:
        ctx.set_half_prefix(True)
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


@functools.lru_cache(maxsize=None)
def _synth_views(n_views=4, n_feat=160):
    from regard3d_amd import synth
    d, _, _ = synth.make_scene_torch(n_views, n_feat, seed=2002, device="cpu", kind="sift")
    return tuple(d[i].numpy() for i in range(n_views))


def test_small_sift_collection(ctx, oracle):
    """an integer SIFT-like collection (every value exact in f16: only the margin acts), all six pairs of four views in one batch"""
    views = list(_synth_views())
    pairs = [(i, j) for i in range(4) for j in range(i + 1, 4)]
    on, q = _run(ctx, oracle, views, 0.6, pairs=pairs)
    ms = [_model(views[i], views[j]) for i, j in pairs]
    assert all(m["unsound16"] == 0 for m in ms)
    assert on[:4] == ((sum(m["tiles"] for m in ms), sum(m["pruned"] for m in ms)), sum(m["filtered"] for m in ms),
                      sum(m["half"] for m in ms), sum(m["skipped"] for m in ms))
    assert q == (sum(m["reach"] for m in ms), sum(m["prefix16"] for m in ms))


@pytest.mark.parametrize("which", ["dataset", "query"])
def test_fewer_than_two_rows(ctx, oracle, which):
    """a view of one row.  As the dataset it has no runner-up: no tile is tested, every query takes the exact scan's verdict.  As the
    query view it is one live lane in one query tile, the second query tile of its wave dead"""
    a, b = QC.oriented_views(70, 70, seed=74)
    if which == "dataset":
        on, q = _run(ctx, oracle, [a[:1].copy(), b], 0.6)
        assert on[0] == (0, 0) and q == (0, 0)
    else:
        on, q = _run(ctx, oracle, [a, b[:1].copy()], 0.6)
        m = _model(a, b[:1].copy())
        assert on[:4] == ((m["tiles"], m["pruned"]), m["filtered"], m["half"], m["skipped"]) and q == (m["reach"], m["prefix16"])


@pytest.mark.parametrize("ratio,enters", [(0.7071, True), (0.7072, False)])
def test_at_the_cutoff(ctx, oracle, ratio, enters):
    """R = 0.49999 <= kPruneMaxR: the three levels run and the f16 test sees every tile that reaches the restart; R = 0.50013 just above:
    the plain kernel runs, the level is not entered"""
    a, b = QC.oriented_views(97, 130, seed=75)
    on, q = _run(ctx, oracle, [a, b], ratio)
    if enters:
        m = _model(a, b, R=float(np.float32(ratio)) ** 2)
        assert on[:4] == ((m["tiles"], m["pruned"]), m["filtered"], m["half"], m["skipped"]) and q == (m["reach"], m["prefix16"])
        assert q[1] >= 1
    else:
        assert on[0] == (0, 0) and q == (0, 0)
