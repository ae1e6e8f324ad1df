"""k-NN (k <= 8) through the KGraph, HNSW and MRPT matchers (`-m gpu`): r3dm_kgraph_knn, r3dm_hnsw_knn, r3dm_hnsw_knn_on_index,
r3dm_mrpt_knn and the three r3dm_index_*_knn entries.

What each arm is compared with, rows AND distance bits:
  HNSW    the reference-built hnswlib's searchKnn(row, k) on the reference-built index (tests/golden/hnsw_ref_knn.npz, written by
          tools/make_golden_hnsw_knn.py); the library's own index through the arrays r3dm_hnsw_index exports
  KGraph  the CPU restatement's orc_kgraph_search(K = k) on the exact index and the start rows of orc_kgraph_seeds
  MRPT    a numpy model of Mrpt::query(q, k, votes) + ArrayMatcher_mrpt's retry in this file, pinned at k = 2 to orc_mrpt_knn2
The shapes are the smallest at which these kernels can still go wrong (600-row views, 128 rows = the smallest indexed view, query
counts that leave a workgroup partly empty, and one MRPT view of 12,288 rows: the smallest round size whose query launch needs more
than 64 KiB of LDS); every reference is computed once per session.
"""
import ctypes as C
import functools
import os
import threading

import numpy as np
import pytest

from regard3d_amd import api, synth
from test_oracle_hnsw import PRESETS, load_case

GOLD_KNN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hnsw_ref_knn.npz")
R3DM_ERR_INVALID = -1


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1]))


@functools.lru_cache(maxsize=None)
def _views(kind, n, seed):
    sc = synth.make_scene(2, n, kind, seed=seed)
    return np.ascontiguousarray(sc.descs[0], np.float32), np.ascontiguousarray(sc.descs[1], np.float32)


# ------------------------------------------------------------------------------------------------------------------ HNSW
def hnsw_ref_lists(scene, preset, k):
    """the reference-built library's k-list of the first 512 rows of view 1: rows stored per k, distances = a prefix of the longest
    list of the same beam (k = 8 is a beam of its own for "fast", ef 5)"""
    g = np.load(GOLD_KNN)
    p = f"{scene}_{preset}_"
    src = "k5_dist" if (preset == "fast" and k <= 5) else "k8_dist"
    return g[p + f"k{k}_idx"].astype(np.int32), np.ascontiguousarray(g[p + src][:, :k])


def test_hnsw_fixture_is_self_consistent(oracle):
    """CPU: the fixture against hnsw_ref_index.npz and against itself.  Lists ascending by (distance, row) wherever rows tie; a shorter
    list of the same beam is a prefix of a longer one except where the cut falls between two equal distances (there hnswlib's heap
    decides which row stays: the rows must still be rows of that distance in the longer list)"""
    g = np.load(GOLD_KNN)
    tied_somewhere = False
    for scene in ("sift", "liop"):
        for preset in PRESETS:
            _, _, _, idx2, dist2 = load_case(scene, preset)
            ef = oracle.HNSW_PRESETS[preset][2]
            for k in (1, 3, 5, 8):
                idx, dist = hnsw_ref_lists(scene, preset, k)
                assert idx.shape == (512, k) and dist.shape == (512, k) and (idx >= 0).all()
                assert (np.diff(dist, axis=1) >= 0).all(), (scene, preset, k)
                tie = np.diff(dist, axis=1) == 0
                assert (np.diff(idx, axis=1)[tie] > 0).all(), (scene, preset, k, "equal distances: lowest row first")
                tied_somewhere |= bool(tie.any())
                for q in range(512):
                    assert len(set(idx[q].tolist())) == k
            # prefix rule, lists of one beam: k <= ef, and the stored 2-lists of hnsw_ref_index.npz (k = 2 <= every ef)
            own = [k for k in (1, 3, 5, 8) if k <= ef]
            longest = hnsw_ref_lists(scene, preset, own[-1])
            for k, (idx, dist) in [(k, hnsw_ref_lists(scene, preset, k)) for k in own[:-1]] + [(2, (idx2[:512], dist2[:512]))]:
                assert np.array_equal(_bits(dist), _bits(longest[1][:, :k])), (scene, preset, k)
                for q in np.where((idx != longest[0][:, :k]).any(axis=1))[0]:
                    assert longest[1][q, k - 1] == longest[1][q, k], (scene, preset, k, q, "rows differ without a tie at the cut")
                    for j in np.where(idx[q] != longest[0][q, :k])[0]:
                        assert idx[q, j] in longest[0][q][longest[1][q] == dist[q, j]]
    assert tied_somewhere, "the sift scene is there for its tied distances"
    assert set(g.files) == {f"{s}_{p}_k{k}_idx" for s in ("sift", "liop") for p in PRESETS for k in (1, 3, 5, 8)} | \
        {f"{s}_{p}_k8_dist" for s in ("sift", "liop") for p in PRESETS} | {f"{s}_fast_k5_dist" for s in ("sift", "liop")}


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 3, 5, 8])
@pytest.mark.parametrize("preset", PRESETS)
@pytest.mark.parametrize("scene", ["sift", "liop"])
def test_hnsw_on_the_reference_built_index_is_hnswlibs(ctx, oracle, scene, preset, k):
    """("fast", k = 8): the beam is max(ef, k) = 8, not ef = 5 -- the case that fails if any heap size still comes from ef"""
    d0, d1, ix, _, _ = load_case(scene, preset)
    M, _, ef = oracle.HNSW_PRESETS[preset]
    got = ctx.hnsw_knn_on_index(d0, ix, M, d1[:512], ef, k)
    assert _same(got, hnsw_ref_lists(scene, preset, k))


@pytest.mark.gpu
def test_hnsw_ragged_query_count(ctx, oracle):
    """509 queries: the last workgroup of four wavefronts is partly empty"""
    d0, d1, ix, _, _ = load_case("sift", "fast")
    M, _, ef = oracle.HNSW_PRESETS["fast"]
    want = hnsw_ref_lists("sift", "fast", 8)
    got = ctx.hnsw_knn_on_index(d0, ix, M, d1[:509], ef, 8)
    assert _same(got, (want[0][:509], want[1][:509]))


@pytest.mark.gpu
@pytest.mark.parametrize("k", [3, 8])
def test_hnsw_on_the_librarys_own_index(ctx, k):
    """r3dm_hnsw_knn = r3dm_hnsw_knn_on_index fed the arrays r3dm_hnsw_index exports; 128 rows: the smallest indexed view"""
    d0, d1 = _views("sift", 128, 5)
    hp = api.HnswParams.preset("fast")
    ctx.clear_images()
    ctx.set_image(0, d0)
    ix = ctx.hnsw_index(0, 128, hp)
    ctx.clear_images()
    got = ctx.hnsw_knn(d0, d1, hp, k)
    assert (got[0][:, 0] >= 0).all()
    assert _same(got, ctx.hnsw_knn_on_index(d0, ix, hp.M, d1, hp.ef, k))


# ------------------------------------------------------------------------------------------------------------------ KGraph
KG_PRESETS = ("fast", "medium", "precise", "default")


@functools.lru_cache(maxsize=None)
def _kgraph_index(oracle_mod, kind, n, seed, K):
    d0, _ = _views(kind, n, seed)
    return oracle_mod.kgraph_build_exact(d0, K=K, cap=64)


def kgraph_restated(oracle, g, d0, q, k, P, S, seed, I, J):
    """orc_kgraph_search(K = k) of every query on the start rows of orc_kgraph_seeds: (rows [nq, k] (-1 padded), distances (+inf padded))"""
    L = oracle.lib()
    L.orc_kgraph_search.restype = C.c_uint32
    L.orc_kgraph_search.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32,
                                    C.c_void_p, C.c_void_p, C.c_void_p]
    idx = np.full((len(q), k), -1, np.int32); dist = np.full((len(q), k), np.inf, np.float32)
    ids = np.zeros(k + 1, np.uint32); ds = np.zeros(k + 1, np.float32)
    for r in range(len(q)):
        seeds = oracle.kgraph_seeds(seed, I, J, r, len(d0), P)
        row = np.ascontiguousarray(q[r])
        n = L.orc_kgraph_search(g.h, d0.ctypes.data, d0.shape[1], row.ctypes.data, k, P, S, seeds.ctypes.data, 128, ids.ctypes.data, ds.ctypes.data, None)
        idx[r, :n] = ids[:n]; dist[r, :n] = ds[:n]
    return idx, dist


@functools.lru_cache(maxsize=None)
def _kgraph_expected(oracle_mod, kind, preset, k):
    d0, d1 = _views(kind, 600, 31)
    kp = api.KGraphParams.preset(preset)
    g = _kgraph_index(oracle_mod, kind, 600, 31, kp.index_K)
    return kgraph_restated(oracle_mod, g, d0, d1, k, kp.search_P, 10, kp.seed, 3, 9)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("preset", KG_PRESETS)
@pytest.mark.parametrize("kind", ["sift", "liop"])
def test_kgraph_equals_the_restatement(ctx, oracle, kind, preset, k):
    d0, d1 = _views(kind, 600, 31)
    kp = api.KGraphParams.preset(preset)
    assert kp.search_S == 10
    assert _same(ctx.kgraph_knn(d0, d1, kp, (3, 9), k), _kgraph_expected(oracle, kind, preset, k))


@pytest.mark.parametrize("kind", ["sift", "liop"])
def test_kgraph_search_depends_on_k(oracle, kind):
    """CPU: the pool is K + P entries, so the search changes with K -- the first two columns at K = 8 are not the 2-NN lists (exact
    index with K 16, P 10, S 10)"""
    d0, d1 = _views(kind, 600, 31)
    g = _kgraph_index(oracle, kind, 600, 31, 16)
    i8, e8 = kgraph_restated(oracle, g, d0, d1, 8, 10, 10, 1998, 3, 9)
    i2, e2 = kgraph_restated(oracle, g, d0, d1, 2, 10, 10, 1998, 3, 9)
    assert ((i8[:, :2] != i2).any(axis=1)).sum() >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("k", [3, 8])
def test_kgraph_smallest_indexed_view(ctx, oracle, k):
    """128 rows, 130 queries: the last workgroup holds two queries"""
    d0, d1 = _views("sift", 130, 7)
    d0 = np.ascontiguousarray(d0[:128])
    kp = api.KGraphParams(index_K=16, search_P=10, search_S=10, seed=77)
    g = oracle.kgraph_build_exact(d0, K=16, cap=64)
    assert _same(ctx.kgraph_knn(d0, d1, kp, (0, 1), k), kgraph_restated(oracle, g, d0, d1, k, 10, 10, 77, 0, 1))


@pytest.mark.gpu
def test_kgraph_pool_of_63_is_served_and_64_refused(ctx, oracle):
    d0, d1 = _views("sift", 600, 31)
    q = d1[:64]
    kp = api.KGraphParams(index_K=16, search_P=55, search_S=10, seed=5)
    g = _kgraph_index(oracle, "sift", 600, 31, 16)
    assert _same(ctx.kgraph_knn(d0, q, kp, (0, 1), 8), kgraph_restated(oracle, g, d0, q, 8, 55, 10, 5, 0, 1))
    kp = api.KGraphParams(index_K=16, search_P=56, search_S=10, seed=5)
    idx, dist = api._knn_out(64, 8)
    rc = ctx._L.r3dm_kgraph_knn(ctx._h, api._ptr(d0), 600, api._ptr(q), 64, 128, C.addressof(kp), 0, 1, 8, api._ptr(idx), api._ptr(dist))
    assert rc == R3DM_ERR_INVALID
    assert _same(ctx.kgraph_knn(d0, q, kp, (0, 1), 7), kgraph_restated(oracle, g, d0, q, 7, 56, 10, 5, 0, 1))      # 7 + 56 = 63


# ------------------------------------------------------------------------------------------------------------------ MRPT
def _l2sq(rows, q):
    """the reference's brute-force metric in its own summation order (orc_l2sq_f32): 4-way groups, float32, no FMA"""
    acc = np.zeros(len(rows), np.float32)
    for c in range(0, rows.shape[1], 4):
        d = rows[:, c:c + 4] - q[None, c:c + 4]
        acc = acc + (((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) + d[:, 3] * d[:, 3])
    return acc


def mrpt_model(ex, d0, q, n_trees, depth, votes, k, route_strict=False, rerank_high=False):
    """Mrpt::query(q, k, votes) on the arrays of orc_mrpt_export, then ArrayMatcher_mrpt::SearchNeighbours' retry and drop rules with
    NN = k (matcher_mrpt.h:207-243).  -> rows [nq, k], sqrtf distances [nq, k], n_elected of the attempt that answered [nq],
    class [nq]: 0 = k rows elected at the first attempt, 1 = only by the retry, 2 = dropped, n_elected of the FIRST attempt [nq] (the
    rows measured for a query are those of the first attempt plus, where a retry ran -- fewer than k of them and votes > 1 -- the third
    value).
    route_strict / rerank_high: two WRONG variants (`<` for `<=` at a split; equal distances to the higher row) for the tests that show
    a case table would notice them (tests/test_mrpt_cases.py)"""
    R, splits, leaves, leaf_first = ex["R"], ex["splits"], ex["leaves"], ex["leaf_first"]
    n, dim = d0.shape
    nq = len(q)
    # projections: column after column, float32, the product rounded before the sum (mr_project)
    pq = np.zeros((nq, n_trees * depth), np.float32)
    for c in range(dim):
        pq = pq + R[None, :, c] * q[:, c, None]
    n_inner = (1 << depth) - 1
    idx = np.full((nq, k), -1, np.int32); dist = np.full((nq, k), -1.0, np.float32)
    ne_out = np.zeros(nq, np.uint32); cls = np.zeros(nq, np.int32); ne_first = np.zeros(nq, np.uint32)
    for r in range(nq):
        tally = np.zeros(n, np.int32)
        for t in range(n_trees):
            node = 0
            for d in range(depth):                                       # mrpt.c:176-180
                left = pq[r, t * depth + d] < splits[t, node] if route_strict else pq[r, t * depth + d] <= splits[t, node]
                node = 2 * node + 1 if left else 2 * node + 2
            leaf = node - n_inner
            tally[leaves[t, leaf_first[leaf]:leaf_first[leaf + 1]]] += 1
        need = votes
        elected = np.where(tally >= need)[0]
        ne_first[r] = len(elected)
        if len(elected) < k and need > 1:                                # "Try again" with votes - 1
            cls[r] = 1
            need -= 1
            elected = np.where(tally >= need)[0]
        ne_out[r] = len(elected)
        if len(elected) < k:                                             # !isValid: nothing is emitted
            cls[r] = 2
            continue
        d2 = _l2sq(d0[elected], q[r])
        o = np.lexsort((-elected if rerank_high else elected, d2))[:k]
        idx[r] = elected[o]; dist[r] = np.sqrt(d2[o])
    return idx, dist, ne_out, cls, ne_first


MRPT_VOTES = (4, 1)      # 4: the three classes below; 1: a hundred and more elected rows, several per lane of the re-rank


@functools.lru_cache(maxsize=None)
def _mrpt_views():
    """600 x 300 SIFT rows at 26 trees of depth 6 (leaves of 9 or 10 rows).  On the plain scene the number of rows with v votes grows
    about sevenfold per step of v, so no votes value leaves queries on both sides of 8 elected rows before AND after the retry; a
    tight cluster of 16 dataset rows and 24 queries beside it gives the queries that elect 8 rows at the first attempt."""
    d0, d1 = _views("sift", 600, 43)
    d0, d1 = d0.copy(), d1[:300].copy()
    rng = np.random.default_rng(7)
    d0[:16] = np.clip(d0[0][None, :] + rng.integers(-2, 3, (16, d0.shape[1])), 0, 255).astype(np.float32)
    d1[:24] = np.clip(d0[0][None, :] + rng.integers(-2, 3, (24, d0.shape[1])), 0, 255).astype(np.float32)
    return d0, d1


def _mrpt_params(votes):
    mp = api.MrptParams.preset()
    return api.MrptParams(mp.n_trees, mp.depth, votes, mp.density, mp.seed)


@functools.lru_cache(maxsize=None)
def _mrpt_index(oracle_mod):
    d0, _ = _mrpt_views()
    mp = api.MrptParams.preset()
    return oracle_mod.mrpt_build(d0, mp.n_trees, mp.depth, float(np.float32(1.0 / np.sqrt(np.float64(d0.shape[1])))), mp.seed)


@functools.lru_cache(maxsize=None)
def _mrpt_case(oracle_mod, votes, k):
    d0, d1 = _mrpt_views()
    ix = _mrpt_index(oracle_mod)
    return mrpt_model(ix.export(), d0, d1, ix.n_trees, ix.depth, votes, k)


@pytest.mark.parametrize("votes", MRPT_VOTES)
def test_mrpt_model_is_the_restatement_at_k2(oracle, votes):
    """CPU: the numpy model against orc_mrpt_knn2 -- rows, distance bits, n_elected"""
    mi, md, mne, _, _ = _mrpt_case(oracle, votes, 2)
    ei, ed, ene = _mrpt_index(oracle).knn2(_mrpt_views()[1], votes)
    assert np.array_equal(mi, ei) and np.array_equal(_bits(md), _bits(ed)) and np.array_equal(mne, ene)


def test_mrpt_scene_holds_the_three_classes(oracle):
    """CPU: at k = 8 and votes 4 some queries elect 8 rows at once, some only with votes - 1, some are dropped"""
    _, _, ne, cls, _ = _mrpt_case(oracle, 4, 8)
    assert all((cls == c).sum() >= 20 for c in (0, 1, 2)), np.bincount(cls, minlength=3)
    assert _mrpt_case(oracle, 1, 8)[2].min() > 64              # votes 1: lanes of the re-rank hold several rows each


@pytest.mark.gpu
@pytest.mark.parametrize("k", [3, 8])
@pytest.mark.parametrize("votes", MRPT_VOTES)
def test_mrpt_equals_the_model(ctx, oracle, votes, k):
    d0, d1 = _mrpt_views()
    mi, md, _, cls, _ = _mrpt_case(oracle, votes, k)
    gi, gd = ctx.mrpt_knn(d0, d1, _mrpt_params(votes), k)
    assert np.array_equal(gi, mi)
    assert np.array_equal(_bits(gd), _bits(md))
    assert ((gi == -1).all(axis=1) == (cls == 2)).all() and ((gd == -1.0).all(axis=1) == (cls == 2)).all()


# ---- MRPT above 64 KiB of LDS: the branch of the launchers' shared helper (r3dm_internal.hpp: launch_with_lds) that raises the limit
# of dynamic LDS on the kernel it launches.  The views above have 600 rows (14,976 B per wavefront at 8,192 rows: 59,904 B a workgroup),
# so nothing else in the suite takes it.  KGraph and HNSW take theirs only above 131,072 and about 107,000 rows of a view, too large for
# this suite: they are covered by sharing the helper.
MRPT_BIG_ROWS, MRPT_BIG_QUERIES, MRPT_BIG_VOTES = 12288, 97, 4       # 97 queries: the last workgroup of four wavefronts holds one


def mrpt_launch_lds(n, n_trees, depth, votes):
    """launch_mrpt_query's LDS bytes for one index view of n rows (kernels_mrpt.hip; elected_cap: api_mrpt.cpp, mrpt_elected_cap)"""
    max_leaf = n // (1 << depth) + 1
    elected_cap = min(n, n_trees * max_leaf // max(votes - 1 if votes > 1 else 1, 1)) + 64
    pool_pad = (n_trees * depth + 63) // 64 * 64
    per_wave = (pool_pad * 4 + 256 * 4 + 8 + elected_cap * 4 + (n + 3) // 4 * 4 + 15) // 16 * 16
    waves = 4
    while waves > 1 and per_wave * waves > 150 * 1024:
        waves >>= 1
    return per_wave * waves


@functools.lru_cache(maxsize=None)
def _mrpt_big_views():
    d0, d1 = _views("sift", MRPT_BIG_ROWS, 47)
    return d0, np.ascontiguousarray(d1[:MRPT_BIG_QUERIES])


@functools.lru_cache(maxsize=None)
def _mrpt_big_index(oracle_mod):
    d0, _ = _mrpt_big_views()
    mp = api.MrptParams.preset()
    assert (mp.n_trees, mp.depth) == (26, 6)
    return oracle_mod.mrpt_build(d0, mp.n_trees, mp.depth, float(np.float32(1.0 / np.sqrt(np.float64(d0.shape[1])))), mp.seed)


@functools.lru_cache(maxsize=None)
def _mrpt_big_case(oracle_mod, k):
    d0, d1 = _mrpt_big_views()
    ix = _mrpt_big_index(oracle_mod)
    lds = mrpt_launch_lds(len(d0), ix.n_trees, ix.depth, MRPT_BIG_VOTES)          # 21,040 B a wavefront, four of them: 84,160 B
    assert 64 * 1024 < lds <= 150 * 1024, lds                                     # a change of preset cannot take the case off the branch
    return mrpt_model(ix.export(), d0, d1, ix.n_trees, ix.depth, MRPT_BIG_VOTES, k)


def test_mrpt_model_is_the_restatement_at_k2_above_64k_lds(oracle):
    """CPU: the numpy model against orc_mrpt_knn2 on the 12,288-row scene -- rows, distance bits, n_elected"""
    mi, md, mne, cls, _ = _mrpt_big_case(oracle, 2)
    ei, ed, ene = _mrpt_big_index(oracle).knn2(_mrpt_big_views()[1], MRPT_BIG_VOTES)
    assert np.array_equal(mi, ei) and np.array_equal(_bits(md), _bits(ed)) and np.array_equal(mne, ene)
    assert (cls != 2).sum() >= MRPT_BIG_QUERIES // 2, "most queries are answered: the comparison is about rows, not about -1"


@pytest.mark.gpu
@pytest.mark.parametrize("k", [2, 3], ids=["knn2", "k3"])
def test_mrpt_above_64k_lds_equals_the_model(ctx, oracle, k):
    """k = 2 is the 2-NN call (mrpt_knn2: the kernel's 2-NN tail), k = 3 the k-list tail; each raises its own kernel's LDS limit"""
    d0, d1 = _mrpt_big_views()
    mi, md, _, _, _ = _mrpt_big_case(oracle, k)
    gi, gd = ctx.mrpt_knn2(d0, d1, _mrpt_params(MRPT_BIG_VOTES)) if k == 2 else ctx.mrpt_knn(d0, d1, _mrpt_params(MRPT_BIG_VOTES), k)
    assert np.array_equal(gi, mi)
    assert np.array_equal(_bits(gd), _bits(md))


# ------------------------------------------------------------------------------------------------------------------ every arm
def _arms(d0, d1):
    """name -> (k-NN call, 2-NN sibling) on one context"""
    kp, hp, mp = api.KGraphParams.preset("default"), api.HnswParams.preset("medium"), api.MrptParams.preset()
    return {
        "kgraph": (lambda c, k: c.kgraph_knn(d0, d1, kp, (3, 9), k), lambda c: c.kgraph_knn2(d0, d1, kp, (3, 9))),
        "hnsw": (lambda c, k: c.hnsw_knn(d0, d1, hp, k), lambda c: c.hnsw_knn2(d0, d1, hp)),
        "mrpt": (lambda c, k: c.mrpt_knn(d0, d1, mp, k), lambda c: c.mrpt_knn2(d0, d1, mp)),
    }


@pytest.mark.gpu
@pytest.mark.parametrize("arm", ["kgraph", "hnsw", "hnsw_on_index", "mrpt"])
def test_k2_returns_the_siblings_bits(ctx, oracle, arm):
    if arm == "hnsw_on_index":
        d0, d1, ix, _, _ = load_case("sift", "fast")
        M, _, ef = oracle.HNSW_PRESETS["fast"]
        assert _same(ctx.hnsw_knn_on_index(d0, ix, M, d1[:300], ef, 2), ctx.hnsw_knn2_on_index(d0, ix, M, d1[:300], ef))
        return
    d0, d1 = _views("sift", 400, 43)
    knn, knn2 = _arms(d0, d1)[arm]
    assert _same(knn(ctx, 2), knn2(ctx))


@pytest.mark.gpu
def test_refusals(ctx):
    """k = 0, k = 9, n_dataset < k, null outputs: R3DM_ERR_INVALID, and nothing is launched"""
    d0, d1 = _views("sift", 400, 43)
    L, h = ctx._L, ctx._h
    kp, hp, mp = api.KGraphParams.preset("default"), api.HnswParams.preset("medium"), api.MrptParams.preset()
    d0p, d1p = api._ptr(d0), api._ptr(d1)
    ix = load_case("sift", "fast")[2]
    l0 = np.ascontiguousarray(ix["links0"], np.int32); uo = np.ascontiguousarray(ix["up_off"], np.int32); ul = np.ascontiguousarray(ix["up_links"], np.int32)
    arr = api.HnswArrays(5, l0.ctypes.data, uo.ctypes.data, ul.ctypes.data, ul.shape[0], ix["enterpoint"], ix["maxlevel"])
    f0 = load_case("sift", "fast")[0]
    index = ctx.index_create(d0)
    calls = {
        "kgraph": lambda n, k, oi, od: L.r3dm_kgraph_knn(h, d0p, n, d1p, 400, 128, C.addressof(kp), 0, 1, k, oi, od),
        "hnsw": lambda n, k, oi, od: L.r3dm_hnsw_knn(h, d0p, n, d1p, 400, 128, C.addressof(hp), k, oi, od),
        "hnsw_on_index": lambda n, k, oi, od: L.r3dm_hnsw_knn_on_index(h, api._ptr(f0), n, 128, C.addressof(arr), d1p, 400, 5, k, oi, od),
        "mrpt": lambda n, k, oi, od: L.r3dm_mrpt_knn(h, d0p, n, d1p, 400, 128, C.addressof(mp), k, oi, od),
        "index_kgraph": lambda n, k, oi, od: L.r3dm_index_kgraph_knn(h, index._h, C.addressof(kp), d1p, 400, 0, 1, k, oi, od),
        "index_hnsw": lambda n, k, oi, od: L.r3dm_index_hnsw_knn(h, index._h, C.addressof(hp), d1p, 400, k, oi, od),
        "index_mrpt": lambda n, k, oi, od: L.r3dm_index_mrpt_knn(h, index._h, C.addressof(mp), d1p, 400, k, oi, od),
    }
    idx, dist = api._knn_out(400, 8)
    launches = ctx.stats().n_match_launches
    try:
        for name, call in calls.items():
            n = len(f0) if name == "hnsw_on_index" else 400
            assert call(n, 0, api._ptr(idx), api._ptr(dist)) == R3DM_ERR_INVALID, name
            assert call(n, 9, api._ptr(idx), api._ptr(dist)) == R3DM_ERR_INVALID, name
            assert call(n, 8, None, api._ptr(dist)) == R3DM_ERR_INVALID, name
            assert call(n, 8, api._ptr(idx), None) == R3DM_ERR_INVALID, name
            if not name.startswith("index_"):
                assert call(5, 6, api._ptr(idx), api._ptr(dist)) == R3DM_ERR_INVALID, name          # n_dataset < k
        small = ctx.index_create(d0[:5])
        try:
            for name in ("index_kgraph", "index_hnsw", "index_mrpt"):
                fn = getattr(L, "r3dm_" + name + "_knn")
                args = (h, small._h, C.addressof({"index_kgraph": kp, "index_hnsw": hp, "index_mrpt": mp}[name]), d1p, 400) + ((0, 1) if name == "index_kgraph" else ())
                assert fn(*args, 6, api._ptr(idx), api._ptr(dist)) == R3DM_ERR_INVALID, name
        finally:
            small.close()
        assert ctx.stats().n_match_launches == launches
        assert (idx == -1).all() and (dist == 0).all()
    finally:
        index.close()


# ------------------------------------------------------------------------------------------------------------------ Build once
@pytest.mark.gpu
def test_index_structures_are_built_once_and_searched_from_two_contexts(ctx):
    d0, d1 = _views("sift", 400, 43)
    kp, hp, mp = api.KGraphParams.preset("default"), api.HnswParams.preset("medium"), api.MrptParams.preset()
    want = {"kgraph": ctx.kgraph_knn(d0, d1, kp, (3, 9), 8), "hnsw": ctx.hnsw_knn(d0, d1, hp, 8), "mrpt": ctx.mrpt_knn(d0, d1, mp, 8)}
    search = {"kgraph": lambda c, ix: ix.kgraph_knn(c, d1, kp, (3, 9), 8), "hnsw": lambda c, ix: ix.hnsw_knn(c, d1, hp, 8),
              "mrpt": lambda c, ix: ix.mrpt_knn(c, d1, mp, 8)}
    other = api.Context(0)
    index = ctx.index_create(d0)
    try:
        for arm in ("kgraph", "hnsw", "mrpt"):
            out, err = {}, []

            def run(name, c):
                try:
                    out[name] = [search[arm](c, index) for _ in range(3)]
                except BaseException as e:      # noqa: BLE001 -- reported by the asserting thread
                    err.append((name, e))
            th = [threading.Thread(target=run, args=("a", ctx)), threading.Thread(target=run, args=("b", other))]
            for t in th:
                t.start()
            for t in th:
                t.join()
            assert not err, (arm, err)
            for name in ("a", "b"):
                for got in out[name]:
                    assert _same(got, want[arm]), (arm, name)
            # the structure is there: a search builds nothing
            got = search[arm](ctx, index)
            st = ctx.stats()
            assert _same(got, want[arm]) and st.ms_ann_build == 0.0 and st.n_ann_built == 0 and st.n_ann_dist > 0, arm
        # one index holds the three structures side by side: the first one still answers
        assert _same(search["kgraph"](other, index), want["kgraph"])
        # search parameters are free per call, build parameters are not
        kp2 = api.KGraphParams(index_K=kp.index_K, search_P=6, search_S=7, seed=9)
        assert _same(index.kgraph_knn(ctx, d1, kp2, (3, 9), 8), ctx.kgraph_knn(d0, d1, kp2, (3, 9), 8))
        assert _same(index.hnsw_knn(ctx, d1, api.HnswParams(hp.M, hp.ef_construction, 40, hp.seed), 8),
                     ctx.hnsw_knn(d0, d1, api.HnswParams(hp.M, hp.ef_construction, 40, hp.seed), 8))
        assert _same(index.mrpt_knn(ctx, d1, api.MrptParams(mp.n_trees, mp.depth, 3, mp.density, mp.seed), 8),
                     ctx.mrpt_knn(d0, d1, api.MrptParams(mp.n_trees, mp.depth, 3, mp.density, mp.seed), 8))
        with pytest.raises(api.R3dmError):
            index.kgraph_knn(ctx, d1, api.KGraphParams(index_K=kp.index_K - 4, search_P=kp.search_P, search_S=kp.search_S, seed=kp.seed), (3, 9), 8)
        with pytest.raises(api.R3dmError):
            index.hnsw_knn(other, d1, api.HnswParams(hp.M + 1, hp.ef_construction, hp.ef, hp.seed), 8)
        with pytest.raises(api.R3dmError):
            index.mrpt_knn(ctx, d1, api.MrptParams(mp.n_trees + 1, mp.depth, mp.votes, mp.density, mp.seed), 8)
        assert _same(search["hnsw"](ctx, index), want["hnsw"])           # a refused call changed nothing
    finally:
        index.close()
        other.close()


@pytest.mark.gpu
def test_first_search_builds_and_the_second_does_not(ctx):
    d0, d1 = _views("sift", 400, 43)
    index = ctx.index_create(d0)
    try:
        for search in (lambda: index.kgraph_knn(ctx, d1, None, (0, 1), 5), lambda: index.hnsw_knn(ctx, d1, None, 5), lambda: index.mrpt_knn(ctx, d1, None, 5)):
            first = search(); s1 = ctx.stats()
            second = search(); s2 = ctx.stats()
            assert s1.ms_ann_build > 0.0 and s1.n_ann_built == 1
            assert s2.ms_ann_build == 0.0 and s2.n_ann_built == 0
            assert _same(first, second)
    finally:
        index.close()


@pytest.mark.gpu
def test_small_index_is_answered_exactly(ctx):
    d0, d1 = _views("sift", 400, 43)
    index = ctx.index_create(d0[:100])
    try:
        want = ctx.index_knn(index, d1, 5)
        assert _same(index.kgraph_knn(ctx, d1, None, (0, 1), 5), want)
        assert _same(index.hnsw_knn(ctx, d1, None, 5), want)
        assert _same(index.mrpt_knn(ctx, d1, None, 5), want)
    finally:
        index.close()
