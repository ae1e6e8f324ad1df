"""The match budget on the GPU (r3dm_set_match_budget, r3dm_budget_rows, kernels_match_budget.hip) -- bit for bit against the
restatement built from the oracle (budget_restatement.py): the device selection against the brute-force selection at every size
around the selection's chunk and the wave width, the budgeted graph of every tile format against the oracle's matcher on the
sub-arrays mapped back, the approximate arms against a second context that holds the sub-arrays, and the behaviour around it (gate,
raw lists, guided matching, filter, device mirror, cache, refusals, two contexts).  tests/test_budget_cases.py shows on the CPU that
the inputs reach their edges."""
import ctypes

import numpy as np
import pytest

import budget_cases as Cs
import budget_restatement as B
import preselect_restatement as PR
from regard3d_amd import api, synth

pytestmark = pytest.mark.gpu


@pytest.fixture()
def bctx(ctx):
    ctx.clear_images()
    yield ctx
    ctx.set_match_budget(False)
    ctx.set_preemptive_matching(False)
    ctx.set_mutual_matching(False); ctx.set_symmetric_ratio(False); ctx.set_device_graphs(False)
    for f in (ctx.set_integer_mfma, ctx.set_split_mfma, ctx.set_hamming_mfma):
        f(False)
    ctx.clear_images()


def _register(c, descs, xys, prios, binary=False):
    c.clear_images()
    for v, d in enumerate(descs):
        c.set_image(v, d, None if xys is None else xys[v], 4000, 3000, binary=binary)
        if prios is not None and prios[v] is not None:
            c.set_view_priority(v, prios[v])


def _csr(g):
    return g.pairs.copy(), g.offsets.copy(), g.matches.copy()


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _has_budget(c, v):
    return bool(c.view_info(v)[0] & api.LAYOUT_BUDGET)


def _expect_graph(got, pairs, counts, matches):
    keep = np.asarray(counts) > 0
    assert np.array_equal(got.pairs, pairs[keep]), "pair set"
    assert np.array_equal(np.diff(got.offsets.astype(np.int64)), np.asarray(counts)[keep].astype(np.int64)), "per-pair counts"
    assert got.matches.tobytes() == np.asarray(matches, np.uint32).tobytes(), "matches"


# ---------------------------------------------------------------------------------------------------- the selection
@pytest.mark.parametrize("pattern", Cs.PATTERNS)
def test_selection_against_the_brute_force(bctx, pattern):
    rng = np.random.default_rng(11)
    for k, n in enumerate(Cs.selection_sizes(api.BUDGET_SELECT_CHUNK)):
        bctx.set_image(k, rng.standard_normal((n, 4)).astype(np.float32), None, 100, 100)
        for N in Cs.selection_budgets(n):
            p = Cs.priority_pattern(pattern, n, N)
            bctx.set_view_priority(k, p)
            got = bctx.budget_rows(k, N)
            want = B.brute_force_rows(p, n, N)
            assert got.tolist() == want, (n, N, got[:8], want[:8])
            rep = bctx.budget_report()
            assert (rep["n_views_whole"], rep["n_views_budgeted"]) == ((1, 0) if n <= N else (0, 1))
            assert rep["n_rows_selected"] == (0 if n <= N else N)
        assert not _has_budget(bctx, k)                              # the primitive leaves no layout behind


def test_selection_of_a_binary_and_a_byte_view(bctx):
    rng = np.random.default_rng(12)
    n = 3 * api.BUDGET_SELECT_CHUNK + 7
    p = rng.integers(0, 5, n).astype(np.float32)
    bctx.set_image(0, rng.integers(0, 256, (n, 61), dtype=np.uint8), None, 100, 100, binary=True)
    bctx.set_image(1, rng.integers(0, 256, (n, 128), dtype=np.uint8), None, 100, 100)
    for v in (0, 1):
        bctx.set_view_priority(v, p)
        assert bctx.budget_rows(v, 300).tolist() == B.brute_force_rows(p, n, 300)


# ---------------------------------------------------------------------------------------------------- graphs against the restatement
_RESTATED = {}


def _restated(oracle, kind, N, mode, real=False):
    key = (kind, N, mode, real)
    if key not in _RESTATED:
        descs, xys, prios, binary, ratio, squared = Cs.make_views(kind, seed=1 if real else 0, real=real)
        if real:
            ratio = 0.8
        pairs = Cs.all_ordered_pairs(len(descs))
        counts, mapped, _ = B.match_collection(oracle, descs, xys, prios, pairs, N, ratio, squared, binary, mode)
        _RESTATED[key] = (descs, xys, prios, binary, ratio, squared, pairs, counts, mapped)
    return _RESTATED[key]


def _budget_graph_check(c, oracle, kind, N, mode="off", real=False):
    descs, xys, prios, binary, ratio, squared, pairs, counts, mapped = _restated(oracle, kind, N, mode, real)
    _register(c, descs, xys, prios, binary)
    c.set_mutual_matching(mode == "mutual"); c.set_symmetric_ratio(mode == "symmetric")
    c.set_match_budget(True, N)
    g = c.match_pairs(pairs, ratio, squared)
    rep = c.budget_report()
    print(f"{kind} N {N} {mode}: {g.num_matches} matches in {g.num_pairs} pairs; select {rep['ms_select']:.3f} gather {rep['ms_gather']:.3f} "
          f"remap {rep['ms_remap']:.3f} ms, wall {rep['ms_wall']:.2f} ms")
    _expect_graph(g, pairs, counts, mapped)
    n_bud = sum(len(d) > N for d in descs)
    assert (rep["n_views_budgeted"], rep["n_views_whole"], rep["n_subviews_built"]) == (n_bud, len(descs) - n_bud, n_bud)
    assert rep["n_rows_selected"] == n_bud * N and 0 < rep["n_matches_remapped"] <= g.num_matches
    for v, d in enumerate(descs):
        assert _has_budget(c, v) == (len(d) > N)
    return g


@pytest.mark.parametrize("kind", [k[0] for k in Cs.KINDS])
@pytest.mark.parametrize("N", Cs.BUDGETS)
def test_budgeted_graph_default_tiles(bctx, oracle, kind, N):
    _budget_graph_check(bctx, oracle, kind, N)


@pytest.mark.parametrize("N", Cs.BUDGETS)
def test_budgeted_graph_integer_tiles(bctx, oracle, N):
    bctx.set_integer_mfma(True)
    _budget_graph_check(bctx, oracle, "f32_128", N)
    assert bctx.stats().n_integer_mfma == 1


@pytest.mark.parametrize("N", Cs.BUDGETS)
def test_budgeted_graph_hamming_mfma(bctx, oracle, N):
    bctx.set_hamming_mfma(True)
    _budget_graph_check(bctx, oracle, "bin_61", N)
    assert bctx.stats().n_hamming_mfma == 1


@pytest.mark.parametrize("N", Cs.BUDGETS)
def test_budgeted_graph_split_planes(bctx, oracle, N):
    bctx.set_split_mfma(True)
    _budget_graph_check(bctx, oracle, "f32_144", N, real=True)
    assert bctx.stats().n_split_mfma == 1


def _votes_over_norm(c):
    c = c.astype(np.float32)
    norm = np.zeros(len(c), np.float32)
    for i in range(c.shape[1]):
        norm = (norm + c[:, i] * c[:, i]).astype(np.float32)
    norm = np.maximum(np.sqrt(norm.astype(np.float64)), 1e-12).astype(np.float32)
    return (c / norm[:, None]).astype(np.float32)


@pytest.mark.parametrize("N", (33, 65))
def test_budgeted_graph_count_tiles(bctx, oracle, N):
    """rows = integer votes x a row scale: the count tiles of r3dm_set_split_mfma are made for the sub-views"""
    rng = np.random.default_rng(21)
    n, dim = 140, 144
    cI = rng.poisson(rng.gamma(0.6, 40 / 0.6, (n, dim))).astype(np.float32) + 1.0
    cJ = np.clip(cI + rng.integers(-2, 3, (n, dim)), 0, 2047)
    dI, dJ = _votes_over_norm(cI), _votes_over_norm(cJ)
    descs = [dI, dJ, np.ascontiguousarray(dI[:33]), np.ascontiguousarray(dJ[:100])]
    shared = rng.integers(0, 5, n).astype(np.float32)
    prios = [shared[:len(d)].copy() for d in descs]
    xys = Cs.positions(descs)
    pairs = Cs.all_ordered_pairs(4)
    counts, mapped, sub = B.match_collection(oracle, descs, xys, prios, pairs, N, 0.8, True)
    assert len(mapped) and (mapped != sub).any()
    bctx.set_split_mfma(True)
    _register(bctx, descs, xys, prios)
    bctx.set_match_budget(True, N)
    _expect_graph(bctx.match_pairs(pairs, 0.8, True), pairs, counts, mapped)
    st = bctx.stats()
    assert st.n_split_mfma == 1 and st.n_counts_mfma == 1


@pytest.mark.parametrize("mode", ("mutual", "symmetric"))
@pytest.mark.parametrize("kind", ("f32_128", "f32_37", "bin_61"))
@pytest.mark.parametrize("N", Cs.BUDGETS)
def test_budgeted_graph_with_the_checks_on_top(bctx, oracle, kind, N, mode):
    _budget_graph_check(bctx, oracle, kind, N, mode)


# ---------------------------------------------------------------------------------------------------- the approximate arms
def _arm(c, arm, pairs):
    if arm == "kgraph":
        return c.match_pairs_kgraph(pairs, 0.6, api.KGraphParams.preset("default"))
    if arm == "hnsw":
        return c.match_pairs_hnsw(pairs, 0.6, api.HnswParams.preset("precise"))
    return c.match_pairs_mrpt(pairs, 0.6, api.MrptParams.preset())


@pytest.mark.parametrize("arm", ["kgraph", "hnsw", "mrpt"])
@pytest.mark.parametrize("N", (150, 100))
def test_approximate_arms_against_registered_sub_arrays(bctx, arm, N):
    """N = 150: sub-views above the arms' 128-row scan bound (indices are built on the sub-views) beside a whole view below it;
    N = 100: every sub-view falls below the bound and is scanned, though its view would have been indexed"""
    descs, xys, prios, binary, ratio, squared = Cs.make_views("f32_128", seed=3, rows=(300, 257, 200, 160, 100, 40))
    pairs = Cs.all_ordered_pairs(len(descs))
    rows, sd, sx = B.sub_views(descs, xys, prios, N)
    second = api.Context(0)
    try:
        _register(second, sd, sx, None)
        ref = _arm(second, arm, pairs)
        counts = np.zeros(len(pairs), np.int64)
        where = {(int(a), int(b)): k for k, (a, b) in enumerate(pairs)}
        for (a, b), m in zip(ref.pairs, np.diff(ref.offsets.astype(np.int64))):
            counts[where[(int(a), int(b))]] = m
        mapped = B.map_back(pairs, counts, ref.matches, rows)
        assert len(mapped) and (mapped != ref.matches).any()
    finally:
        second.close()
    _register(bctx, descs, xys, prios)
    bctx.set_match_budget(True, N)
    g = _arm(bctx, arm, pairs)
    _expect_graph(g, pairs, counts, mapped)
    assert bctx.budget_report()["n_subviews_built"] == sum(len(d) > N for d in descs)
    # the whole view's index entries still report on the whole view
    if arm == "kgraph":
        adj, deg = bctx.kgraph_index(0, len(descs[0]), 24)
        assert adj.shape[0] == len(descs[0]) and (deg > 0).all()
    g2 = _arm(bctx, arm, pairs)
    assert _same(_csr(g), _csr(g2)) and bctx.budget_report()["n_subviews_built"] == 0
    bytes_with_indices = bctx.view_info(0)[1]
    bctx.drop_indices()                                              # ... also the indices built on sub-views
    assert bctx.view_info(0)[1] < bytes_with_indices or N == 100
    assert _same(_csr(g), _csr(_arm(bctx, arm, pairs)))


# ---------------------------------------------------------------------------------------------------- behaviour
def test_gate_plus_budget(bctx, oracle):
    """the gate builds its heads from the whole views and runs first: the graph is the budgeted graph restricted to the kept pairs"""
    descs, xys, prios, binary, ratio, squared, pairs, counts, mapped = _restated(oracle, "f32_128", 33, "off")
    _register(bctx, descs, xys, prios)
    _, keep = PR.gate_collection(oracle, descs, prios, pairs, 32, 4, ratio, squared)
    assert 0 < keep.sum() < len(pairs) and (np.asarray(counts)[~keep] > 0).any()
    bctx.set_match_budget(True, 33)
    bctx.set_preemptive_matching(True, 32, 4)
    g = bctx.match_pairs(pairs, ratio, squared)
    kc, km = B.restrict_to(pairs, counts, mapped, keep)
    _expect_graph(g, pairs[keep], kc, km)
    assert bctx.preselect_report()["n_kept"] == int(keep.sum())


def test_raw_lists_guided_and_filter(bctx, oracle):
    sc = synth.make_scene(4, 768, "sift", seed=1003)
    rng = np.random.default_rng(31)
    prios = [rng.integers(0, 6, len(d)).astype(np.float32) for d in sc.descs]
    pairs = sc.exhaustive_pairs()
    xys = [np.asarray(x) for x in sc.xys]
    _register(bctx, sc.descs, xys, prios)
    Hs = np.tile(np.array([1, 0, 40.0, 0, 1, 0, 0, 0, 1]), (len(pairs), 1))
    thr = np.full(len(pairs), 250.0)
    off_knn = bctx.knn2(sc.descs[0], sc.descs[1])
    off_knn4 = bctx.knn(sc.descs[0], sc.descs[1], 4)
    off_guided = _csr(bctx.guided_match(pairs, "H", Hs, thr, 0.6))
    N = 300
    bctx.set_match_budget(True, N)
    assert _same(bctx.knn2(sc.descs[0], sc.descs[1]), off_knn) and _same(bctx.knn(sc.descs[0], sc.descs[1], 4), off_knn4)
    assert _same(_csr(bctx.guided_match(pairs, "H", Hs, thr, 0.6)), off_guided)
    assert not any(_has_budget(bctx, v) for v in range(len(sc.descs)))
    g = bctx.match_pairs(pairs, 0.6, True)
    counts, mapped, sub = B.match_collection(oracle, sc.descs, xys, prios, pairs, N, 0.6, True)
    _expect_graph(g, pairs, counts, mapped)
    assert (mapped != sub).any() and mapped.max() >= N
    # the filter reads the registered positions through the original indices
    gf = bctx.filter_F(g, 4.0, 2048, seed=5489)
    oc, om = oracle.filter_F_collection(xys, sc.widths, sc.heights, g.pairs, np.diff(g.offsets.astype(np.int64)), g.matches)
    d = gf.as_dict(); off = 0
    assert gf.num_pairs > 0
    for p, (I, J) in enumerate(g.pairs):
        exp = om[off:off + oc[p]]; off += oc[p]
        got = d.get((int(I), int(J)), np.zeros((0, 2), np.uint32))
        assert set(map(tuple, got.tolist())) == set(map(tuple, exp.tolist())), (I, J)
    # guided matching behind the budgeted putatives re-matches over all features
    assert _same(_csr(bctx.guided_match(pairs, "H", Hs, thr, 0.6)), off_guided)


def test_device_mirror(bctx, oracle):
    """the mirror is made from the remapped matches: the tracks builder reads it in place of the host arrays"""
    descs, xys, prios, binary, ratio, squared, pairs, counts, mapped = _restated(oracle, "f32_128", 64, "off")
    _register(bctx, descs, xys, prios)
    bctx.set_match_budget(True, 64)
    plain = bctx.match_pairs(pairs, ratio, squared)
    assert plain.on_device == -1
    t0 = bctx.build_tracks(plain)
    bctx.set_device_graphs(True)
    mirrored = bctx.match_pairs(pairs, ratio, squared)
    assert mirrored.on_device == 0 and _same(_csr(mirrored), _csr(plain))
    _expect_graph(mirrored, pairs, counts, mapped)
    t1 = bctx.build_tracks(mirrored)
    assert len(t0) == len(t1) > 0 and np.array_equal(t0.offsets, t1.offsets) and np.array_equal(t0.observations, t1.observations)


def test_cache(bctx, oracle):
    descs, xys, prios, binary, ratio, squared, pairs, counts, mapped = _restated(oracle, "f32_128", 64, "off")
    _register(bctx, descs, xys, prios)
    big = 9                                                          # the 300-row view
    base = bctx.view_info(big)[1]
    held0 = bctx.memory_info()[0]
    bctx.match_pairs(pairs, ratio, squared)
    assert all(v == 0 for v in bctx.budget_report().values()) and not _has_budget(bctx, big)      # the switch is off
    assert bctx.view_info(big)[1] == base and bctx.memory_info()[0] == held0
    bctx.set_match_budget(True, 64)
    g = _csr(bctx.match_pairs(pairs, ratio, squared))
    n_bud = sum(len(d) > 64 for d in descs)
    assert bctx.budget_report()["n_subviews_built"] == n_bud and _has_budget(bctx, big)
    with_sub = bctx.view_info(big)[1]
    assert with_sub >= base + 64 * 4 + 64 * 128 * 4
    assert _same(_csr(bctx.match_pairs(pairs, ratio, squared)), g) and bctx.budget_report()["n_subviews_built"] == 0
    assert bctx.budget_report()["n_views_budgeted"] == n_bud
    # another N: every sub-view is remade (the views of 65 rows become whole)
    c33, m33, _ = B.match_collection(oracle, descs, xys, prios, pairs, 65, ratio, squared)
    bctx.set_match_budget(True, 65)
    _expect_graph(bctx.match_pairs(pairs, ratio, squared), pairs, c33, m33)
    assert bctx.budget_report()["n_subviews_built"] == sum(len(d) > 65 for d in descs)
    bctx.set_match_budget(True, 64)
    assert _same(_csr(bctx.match_pairs(pairs, ratio, squared)), g)
    # a priority change: that view's sub-view alone
    prios2 = list(prios); prios2[big] = prios[big][::-1].copy()
    bctx.set_view_priority(big, prios2[big])
    assert not _has_budget(bctx, big) and bctx.view_info(big)[1] < with_sub
    c2, m2, _ = B.match_collection(oracle, descs, xys, prios2, pairs, 64, ratio, squared)
    _expect_graph(bctx.match_pairs(pairs, ratio, squared), pairs, c2, m2)
    assert bctx.budget_report()["n_subviews_built"] == 1 and _has_budget(bctx, big)
    # a replaced view: the sub-view goes with the old registration, the priority too
    descs3 = list(descs); prios3 = list(prios2); xys3 = list(xys)
    descs3[big] = np.ascontiguousarray(descs[8][:280]); xys3[big] = np.ascontiguousarray(xys[8][:280]); prios3[big] = None
    bctx.set_image(big, descs3[big], xys3[big], 4000, 3000)
    assert not _has_budget(bctx, big)
    c3, m3, _ = B.match_collection(oracle, descs3, xys3, prios3, pairs, 64, ratio, squared)
    _expect_graph(bctx.match_pairs(pairs, ratio, squared), pairs, c3, m3)
    assert bctx.budget_report()["n_subviews_built"] == 1
    # cleared: nothing of it is left, and the next collection starts over
    bctx.clear_images()
    _register(bctx, descs, xys, prios)
    assert not any(_has_budget(bctx, v) for v in range(len(descs)))
    assert _same(_csr(bctx.match_pairs(pairs, ratio, squared)), g) and bctx.budget_report()["n_subviews_built"] == n_bud
    # off again: the graph of the whole views
    bctx.set_match_budget(False, 64)
    wc, wm = B.whole_collection(oracle, descs, xys, pairs, ratio, squared)
    _expect_graph(bctx.match_pairs(pairs, ratio, squared), pairs, wc, wm)
    assert all(v == 0 for v in bctx.budget_report().values())


def test_refusals(bctx):
    L = api.load_library()
    rng = np.random.default_rng(41)
    d = rng.integers(0, 121, (40, 128)).astype(np.float32)
    bctx.set_image(0, d, None, 100, 100)
    for N in (0, 1):
        with pytest.raises(api.R3dmError, match="-> -1"):
            bctx.set_match_budget(True, N)
        with pytest.raises(api.R3dmError, match="-> -1"):
            bctx.set_match_budget(False, N)                          # also when enable is 0
        with pytest.raises(api.R3dmError, match="-> -1"):
            bctx.budget_rows(0, N)
    with pytest.raises(api.R3dmError, match="-> -1"):
        bctx.budget_rows(99, 8)                                      # an unregistered view
    assert bctx.budget_rows(0, 40).tolist() == list(range(40)) and bctx.budget_rows(0, 41).tolist() == list(range(40))
    n = ctypes.c_uint32(0)
    assert L.r3dm_set_match_budget(None, 1, 8) == -1 and L.r3dm_budget_report(None, None) == -1
    assert L.r3dm_budget_rows(None, 0, 8, None, ctypes.byref(n)) == -1 and L.r3dm_multi_set_match_budget(None, 1, 8) == -1
    assert not _has_budget(bctx, 0)


def test_multi_context_two_contexts_on_one_gpu(bctx, oracle):
    descs, xys, prios, binary, ratio, squared, pairs, counts, mapped = _restated(oracle, "f32_128", 33, "off")
    m = api.MultiContext([0, 0])
    try:
        for v, d in enumerate(descs):
            m.set_image(v, d, xys[v], 4000, 3000)
            m.set_view_priority(v, prios[v])
        m.set_match_budget(True, 33)
        g = m.match_pairs(pairs, ratio, squared)
        _expect_graph(g, pairs, counts, mapped)
        reps = [m.device_budget_report(k) for k in range(2)]
        assert all(r["n_views_budgeted"] > 0 for r in reps) and sum(r["n_matches_remapped"] for r in reps) > 0
        with pytest.raises(api.R3dmError):
            m.set_match_budget(True, 1)
        m.set_match_budget(False)
        wc, wm = B.whole_collection(oracle, descs, xys, pairs, ratio, squared)
        _expect_graph(m.match_pairs(pairs, ratio, squared), pairs, wc, wm)
    finally:
        m.close()
