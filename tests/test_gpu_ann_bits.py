"""GPU parity of the Hamming graph matcher (binary views on the KGraph arm, r3dm_set_kgraph_hamming) against the float models run on
the unpacked rows (ann_bits_cases.py; test_ann_bits_cases.py shows that those ARE the Hamming models).  Index, search, k-lists and
collections are compared bit for bit on the same index and start rows; recall bars are conditions on inputs where the model alone
clears them."""
import ctypes as C
import functools

import numpy as np
import pytest

from regard3d_amd import api

import ann_bits_cases as cases

pytestmark = pytest.mark.gpu

REFUSAL = "kgraph matching needs F32/U8 descriptors with dim % 4 == 0"
REFUSAL_INDEX = "kgraph index needs >= 2 F32/U8 rows with dim % 4 == 0"


@pytest.fixture(scope="module")
def hctx():
    """a context of this module's own with the switch on (the session's context keeps refusing binary views)"""
    c = api.Context(0)
    c.set_kgraph_hamming(True)
    yield c
    c.close()


def _same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def _csr(g):
    return g.pairs.copy(), g.offsets.copy(), g.matches.copy()


def _same_graph(g, pairs, counts, matches):
    d, exp = g.as_dict(), cases.graph_dict(pairs, counts, matches)
    assert set(d.keys()) == set(exp.keys())
    for k in exp:
        assert np.array_equal(d[k], exp[k]), f"pair {k}"


def _register_scene(c):
    descs, xys, pairs = cases.scene()
    c.clear_images()
    for i in range(len(descs)):
        c.set_image(i, descs[i], xys[i], 4000, 3000, binary=True)
    return descs, xys, pairs


@functools.lru_cache(maxsize=None)
def _scene_model(oracle_mod, R, preset, builder="exact", positions=True):
    descs, xys, pairs = cases.scene()
    xys = xys if positions else None                                     # without positions: the accepted matches before any de-duplication
    unpacked = [cases.bits(d) for d in descs]
    if builder == "exact":
        kp = api.KGraphParams.preset(preset)
        return oracle_mod.match_collection_kgraph(unpacked, xys, pairs, cases.RATIOS[R], builder="exact", K=kp.index_K, P=kp.search_P,
                                                  S=kp.search_S, seed=kp.seed, min_rows=128)
    K, L, rc, P = oracle_mod.KGRAPH_PRESETS[preset]
    return oracle_mod.match_collection_kgraph(unpacked, xys, pairs, cases.RATIOS[R], builder="nndescent", K=K, L=L, recall=rc, P=P)


# ---------------------------------------------------------------------------------------------------- 1. the index
@pytest.mark.parametrize("n,nbytes,K,kind", cases.INDEX_CASES)
def test_index_equals_the_model(hctx, oracle, n, nbytes, K, kind):
    A, _ = cases.views(kind, n, n if kind != "ties" else 200, nbytes)
    hctx.clear_images()
    hctx.set_image(5, A, binary=True)
    before = hctx.kgraph_hamming_report()
    adj, deg = hctx.kgraph_index(5, n, K)
    assert hctx.kgraph_hamming_report()["n_index_builds"] == before["n_index_builds"] + 1
    off, ids, _ = oracle.kgraph_build_exact(cases.bits(A), K=K, cap=64).csr()
    eadj, edeg = cases.csr_rows(off, ids, n)
    assert np.array_equal(deg, edeg)
    assert np.array_equal(adj, eadj)


# ---------------------------------------------------------------------------------------------------- 2. the 2-NN search
@pytest.mark.parametrize("nI,nJ,nbytes,K,P,S,kind", cases.KNN2_CASES)
def test_knn2_equals_the_models_search_on_the_same_index(hctx, oracle, nI, nJ, nbytes, K, P, S, kind):
    A, B = cases.views(kind, nI, nJ, nbytes)
    kp = api.KGraphParams(index_K=K, search_P=P, search_S=S, seed=cases.SEARCH_SEED)
    before = hctx.kgraph_hamming_report()
    idx, dist = hctx.kgraph_knn2(A, B, kp, pair=cases.SEARCH_PAIR, binary=True)
    after, st = hctx.kgraph_hamming_report(), hctx.stats()
    assert (after["n_index_builds"], after["n_search_launches"]) == (before["n_index_builds"] + 1, before["n_search_launches"] + 1)
    assert st.n_ann_dist > 0 and (st.n_ann_rows16, st.n_ann_rows8, st.n_ann_dot8) == (0, 0, 0)
    g = oracle.kgraph_build_exact(cases.bits(A), K=K, cap=64)
    oidx, odist, _ = g.knn2(cases.bits(B), P=P, S=S, seed=cases.SEARCH_SEED, I=cases.SEARCH_PAIR[0], J=cases.SEARCH_PAIR[1], min_rows=128)
    assert dist.dtype == np.float32 and np.array_equal(dist, np.rint(dist))         # integers as float32
    assert np.array_equal(dist, odist)
    assert np.array_equal(idx, oidx)


# ---------------------------------------------------------------------------------------------------- 3. k-lists
@functools.lru_cache(maxsize=None)
def _klist_case(oracle_mod, k):
    A, B = cases.views("akaze", 600, 300, 61)
    g = oracle_mod.kgraph_build_exact(cases.bits(A), K=16, cap=64)
    return cases.kgraph_restated(oracle_mod, g, cases.bits(A), cases.bits(B), k, 10, 10, cases.SEARCH_SEED, *cases.SEARCH_PAIR)


@pytest.mark.parametrize("k", [1, 3, 8])
def test_klists_equal_the_models_pool_prefix(hctx, oracle, k):
    A, B = cases.views("akaze", 600, 300, 61)
    kp = api.KGraphParams(index_K=16, search_P=10, search_S=10, seed=cases.SEARCH_SEED)
    want = _klist_case(oracle, k)
    assert _same(hctx.kgraph_knn(A, B, kp, cases.SEARCH_PAIR, k, binary=True), want)
    other = api.Context(0)
    other.set_kgraph_hamming(True)
    index = hctx.index_create(A, binary=True)
    try:
        first = index.kgraph_knn(hctx, B, kp, cases.SEARCH_PAIR, k)
        assert hctx.stats().n_ann_built == 1
        second = index.kgraph_knn(other, B, kp, cases.SEARCH_PAIR, k)         # built once, searched from another context
        assert other.stats().n_ann_built == 0 and other.kgraph_hamming_report() == {"n_index_builds": 0, "n_search_launches": 1}
        assert _same(first, want) and _same(second, want)
        with pytest.raises(api.R3dmError, match="another index_K"):
            index.kgraph_knn(hctx, B, api.KGraphParams(index_K=12, search_P=10, search_S=10, seed=cases.SEARCH_SEED), cases.SEARCH_PAIR, k)
    finally:
        index.close()
        other.close()


def test_short_pool_is_padded(hctx, oracle):
    """one start round of S = 1 expansions on a sparse index leaves pools below k: -1 / +inf behind them, as the model"""
    A, B = cases.views("rand", 400, 300, 32)
    kp = api.KGraphParams(index_K=1, search_P=2, search_S=1, seed=cases.SEARCH_SEED)
    g = oracle.kgraph_build_exact(cases.bits(A), K=1, cap=64)
    want = cases.kgraph_restated(oracle, g, cases.bits(A), cases.bits(B), 8, 2, 1, cases.SEARCH_SEED, *cases.SEARCH_PAIR)
    assert (want[0] == -1).any() and np.isinf(want[1]).any()
    assert _same(hctx.kgraph_knn(A, B, kp, cases.SEARCH_PAIR, 8, binary=True), want)


def test_pool_beyond_63_is_refused(hctx):
    A, B = cases.views("rand", 400, 300, 32)
    kp = api.KGraphParams(index_K=16, search_P=56, search_S=10, seed=5)
    idx, dist = api._knn_out(300, 8)
    launches = hctx.kgraph_hamming_report()["n_search_launches"]
    rc = hctx._L.r3dm_kgraph_knn_bits(hctx._h, api._ptr(A), 400, api._ptr(B), 300, 32, C.addressof(kp), 0, 1, 8, api._ptr(idx), api._ptr(dist))
    assert rc == -1 and hctx.kgraph_hamming_report()["n_search_launches"] == launches     # R3DM_ERR_INVALID
    hctx.kgraph_knn(A, B, kp, (0, 1), 7, binary=True)                                      # 7 + 56 = 63 is served


def test_other_row_lengths_stay_unsupported(hctx):
    rng = np.random.default_rng(2)
    A = rng.integers(0, 256, (300, 40), dtype=np.uint8)
    with pytest.raises(api.R3dmError):
        hctx.kgraph_knn2(A, A[:10], api.KGraphParams.preset("default"), binary=True)
    with pytest.raises(api.R3dmError):
        hctx.set_image(0, A, binary=True)


# ---------------------------------------------------------------------------------------------------- 4. small views
def test_small_views_are_scanned(hctx, oracle):
    A, B = cases.views("akaze", 1500, 1200, 61)
    launches = hctx.kgraph_hamming_report()["n_search_launches"]
    bi, bd = oracle.knn2(A[:120], B, binary=True)
    idx, dist = hctx.kgraph_knn2(A[:120], B, api.KGraphParams.preset("precise"), binary=True)
    assert np.array_equal(idx, bi) and np.array_equal(dist, bd.astype(np.float32))
    bi, bd = oracle.knn2(A[:40], B[:50], binary=True)                      # search_P >= n
    idx, dist = hctx.kgraph_knn2(A[:40], B[:50], api.KGraphParams(index_K=16, search_P=40, search_S=10, seed=1), binary=True)
    assert np.array_equal(idx, bi) and np.array_equal(dist, bd.astype(np.float32))
    assert hctx.kgraph_hamming_report()["n_search_launches"] == launches


# ---------------------------------------------------------------------------------------------------- 5. the collection
@pytest.mark.parametrize("preset", ["default", "precise"])
def test_collection_equals_the_model_and_recovers_the_exhaustive_matches(hctx, oracle, preset):
    R = 0.765625
    descs, xys, pairs = _register_scene(hctx)
    hctx.drop_indices()
    before = hctx.kgraph_hamming_report()
    g = hctx.match_pairs_kgraph(pairs, R, api.KGraphParams.preset(preset))
    st, after = hctx.stats(), hctx.kgraph_hamming_report()
    counts, matches, _ = _scene_model(oracle, R, preset)
    _same_graph(g, pairs, counts, matches)
    assert st.n_ann_built == 3 and st.n_ann_dist > 0                     # views 0, 1, 2 are first views of an indexed pair
    assert st.n_ann_rows8 == 0 and st.n_ann_rows16 == 0 and st.n_ann_dot8 == 0
    assert after["n_index_builds"] == before["n_index_builds"] + 3 and after["n_search_launches"] > before["n_search_launches"]
    bc, _ = oracle.match_collection(descs, xys, pairs, R, squared=False, binary=True)
    print(f"{preset}: {counts.sum()} matches, exhaustive {bc.sum()}")
    assert counts.sum() >= 0.85 * bc.sum(), (counts.sum(), bc.sum())
    if preset == "default":
        nc, _, _ = _scene_model(oracle, R, preset, "nndescent")
        print(f"NN-descent model: {nc.sum()}")
        assert counts.sum() >= 0.95 * nc.sum(), (counts.sum(), nc.sum())


# ---------------------------------------------------------------------------------------------------- 6. the switch
def test_switch_off_refuses_as_before_and_on_serves(oracle):
    descs, xys, pairs = cases.scene()
    fdescs = [cases.bits(d[:, :8]) * 3.0 for d in descs[:3]]              # three float views (64-D) beside the binary ones
    fpairs = np.array([[10, 11], [10, 12], [11, 12]], np.uint32)
    c = api.Context(0)
    index = c.index_create(descs[0], binary=True)
    kp = api.KGraphParams.preset("default")
    try:
        for i in range(len(descs)):
            c.set_image(i, descs[i], xys[i], 4000, 3000, binary=True)
        for i in range(3):
            c.set_image(10 + i, fdescs[i], xys[i], 4000, 3000)
        ref_f = _csr(c.match_pairs_kgraph(fpairs, 0.8, kp))

        def refused():
            with pytest.raises(api.R3dmError, match=REFUSAL):
                c.match_pairs_kgraph(pairs, 0.765625, kp)
            with pytest.raises(api.R3dmError, match=REFUSAL_INDEX):
                c.kgraph_index(0, len(descs[0]), 16)
            with pytest.raises(api.R3dmError, match=REFUSAL):
                index.kgraph_knn(c, descs[1], kp, (0, 1), 2)
        refused()
        assert c.kgraph_hamming_report() == {"n_index_builds": 0, "n_search_launches": 0}
        c.set_kgraph_hamming(True)
        on_b = _csr(c.match_pairs_kgraph(pairs, 0.765625, kp))
        counts, matches, _ = _scene_model(oracle, 0.765625, "default")
        assert np.array_equal(on_b[2], matches) and np.array_equal(on_b[0], pairs[counts > 0])
        c.kgraph_index(0, len(descs[0]), 16)
        index.kgraph_knn(c, descs[1], kp, (0, 1), 2)
        on_f = _csr(c.match_pairs_kgraph(fpairs, 0.8, kp))
        # a list that mixes float and binary views (and names pairs across the two kinds, which are skipped) = the two lists run alone
        cross = np.array([[0, 10], [11, 1]], np.uint32)
        mixed = _csr(c.match_pairs_kgraph(np.concatenate([fpairs, cross, pairs]), 0.765625, kp))
        alone_f = _csr(c.match_pairs_kgraph(fpairs, 0.765625, kp))
        assert np.array_equal(mixed[0], np.concatenate([on_b[0], alone_f[0]]))
        assert np.array_equal(mixed[2], np.concatenate([on_b[2], alone_f[2]]))
        c.set_kgraph_hamming(False)
        refused()
        off_f = _csr(c.match_pairs_kgraph(fpairs, 0.8, kp))
        for got in (on_f, off_f):
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, ref_f))
    finally:
        index.close()
        c.close()


# ---------------------------------------------------------------------------------------------------- 7. caching, multi-context
def test_index_cache_drop_and_multi_context(hctx, oracle):
    descs, xys, pairs = _register_scene(hctx)
    kp = api.KGraphParams.preset("default")
    a16, _ = hctx.kgraph_index(0, 1300, 16)
    a24, _ = hctx.kgraph_index(0, 1300, 24)
    assert not np.array_equal(a16, a24)
    hctx.set_image(0, descs[1], xys[1], 4000, 3000, binary=True)            # re-staging drops the cached index
    b24, _ = hctx.kgraph_index(0, 1300, 24)
    c24, _ = hctx.kgraph_index(1, 1300, 24)
    assert np.array_equal(b24, c24)
    hctx.set_image(0, descs[0], xys[0], 4000, 3000, binary=True)
    hctx.drop_indices()                                                   # (view 1 still holds the K = 24 index from above)
    g0 = hctx.match_pairs_kgraph(pairs, 0.765625, kp); built0 = hctx.stats().n_ann_built
    g1 = hctx.match_pairs_kgraph(pairs, 0.765625, kp); built1 = hctx.stats().n_ann_built
    hctx.drop_indices()
    g2 = hctx.match_pairs_kgraph(pairs, 0.765625, kp); built2 = hctx.stats().n_ann_built
    assert (built0, built1, built2) == (3, 0, 3)
    for g in (g1, g2):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(_csr(g), _csr(g0)))
    m = api.MultiContext([0])
    try:
        for i in range(len(descs)):
            m.set_image(i, descs[i], xys[i], 4000, 3000, binary=True)
        with pytest.raises(api.R3dmError):
            m.match_pairs_kgraph(pairs, 0.765625, kp)
        m.set_kgraph_hamming(True)
        gm = m.match_pairs_kgraph(pairs, 0.765625, kp)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(_csr(gm), _csr(g0)))
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------- 8. the "every arm" switches
def _hamming_matrix(A, B):
    a, b = cases.bits(A).astype(np.float64), cases.bits(B).astype(np.float64)
    return a.sum(1)[:, None] + b.sum(1)[None, :] - 2.0 * (a @ b.T)


def test_mutual_matching_on_the_hamming_graph_matcher():
    """view 1 holds 200 of its rows a second time with two bits flipped: both copies pass the ratio test on the same row of I, and the
    mutual rule keeps the nearer one only"""
    descs, xys, _ = cases.scene()
    rng = np.random.default_rng(9)
    extra = descs[1][:200].copy()
    for r in range(len(extra)):
        for b in rng.choice(486, 2, replace=False):
            extra[r, b // 8] ^= np.uint8(1 << (b % 8))
    descs = [descs[0], np.concatenate([descs[1], extra]), descs[2]]
    xys = [xys[0], np.concatenate([xys[1], xys[1][:200] + np.float32(0.5)]), xys[2]]
    pairs = np.array([[0, 1], [0, 2], [1, 2]], np.uint32)
    kp = api.KGraphParams.preset("default")
    c = api.Context(0)
    try:
        c.set_kgraph_hamming(True)
        for i in range(3):
            c.set_image(i, descs[i], xys[i], 4000, 3000, binary=True)
        off = c.match_pairs_kgraph(pairs, 0.765625, kp).as_dict()
        c.set_mutual_matching(True)
        on = c.match_pairs_kgraph(pairs, 0.765625, kp).as_dict()
        st = c.stats()
        assert st.n_mutual_dropped > 0 and st.n_mutual_checked >= sum(len(v) for v in off.values()) and set(on) == set(off)
        for (I, J), m in on.items():
            D = _hamming_matrix(descs[I], descs[J])
            for i, j in m:
                assert np.flatnonzero(D[i] == D[i].min())[0] == j, (I, J, i, j)       # j is row i's nearest row of J under (distance, row)
            assert len(np.unique(m[:, 0])) == len(m)
            assert {tuple(x) for x in m.tolist()} <= {tuple(x) for x in off[(I, J)].tolist()}
        assert sum(len(v) for v in on.values()) < sum(len(v) for v in off.values())
    finally:
        c.close()


def test_preemptive_matching_on_the_hamming_graph_matcher(oracle):
    descs, xys, pairs = cases.scene()
    rng = np.random.default_rng(8)
    c = api.Context(0)
    try:
        c.set_kgraph_hamming(True)
        _register_scene(c)
        for i in range(4):
            c.set_view_priority(i, rng.uniform(1.0, 9.0, len(descs[i])).astype(np.float32))
        kp = api.KGraphParams.preset("default")
        ungated = c.match_pairs_kgraph(pairs, 0.765625, kp).as_dict()
        live = np.array([p for p in pairs.tolist() if len(descs[p[0]]) and len(descs[p[1]])], np.uint32)
        cnt = c.preselect_pairs(live, 96, 0.765625, False)
        t = int(np.sort(cnt)[len(cnt) // 2]) + 1                          # a threshold that drops some pairs and keeps others
        assert (cnt >= t).any() and (cnt < t).any()
        c.set_preemptive_matching(True, 96, t)
        gated = c.match_pairs_kgraph(pairs, 0.765625, kp).as_dict()
        rep = c.preselect_report()
        keep = {tuple(p) for p, n in zip(live.tolist(), cnt) if n >= t}
        assert rep["n_pairs"] == len(live) and rep["n_kept"] == len(keep)
        assert set(gated) == {k for k in ungated if k in keep}
        for k in gated:
            assert np.array_equal(gated[k], ungated[k])
    finally:
        c.close()
