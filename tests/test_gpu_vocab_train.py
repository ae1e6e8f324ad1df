"""Vocabulary training and idf-weighted scores on the GPU (include/r3dm.h, "Trained vocabularies", "idf-weighted scores"; DESIGN.md
section 4.30): `-m gpu`.  Every case of tests/vocab_train_cases.py against the numpy restatement (tests/vocab_train_restatement.py)
with == : the trained words, the report's counters, the weights, the scores, the pairs.  Then what the contract promises around them:
the same words on every exact tile path, no dependence on what the context did before, r3dm_stats and `init` left alone, the refusals."""
import numpy as np
import pytest

import vocab_cases as VC
import vocab_restatement as R
import vocab_train_cases as TC
import vocab_train_restatement as TR
from regard3d_amd import api

pytestmark = pytest.mark.gpu
INVALID = r"-> -1:"                                  # R3DM_ERR_INVALID in an R3dmError
UNSUPPORTED = r"-> -5:"                              # R3DM_ERR_UNSUPPORTED
COUNTERS = ("n_updates", "converged", "n_moved", "n_empty", "max_members", "n_rows_assigned")


@pytest.fixture(scope="module")
def tctx():
    c = api.Context(0)
    yield c
    c.close()


def _register(c, case):
    for k, d in enumerate(case.descs):
        c.set_image(case.ids[k], d, binary=case.binary)


def _init(c, case):
    return c.vocab_from_rows(case.vocab, binary=case.binary) if case.vocab is not None else c.vocab_sample(case.ids, case.n_words)


def _train(c, case):
    init = _init(c, case)
    try:
        before = init.words()
        v = c.vocab_train(init, case.ids, case.max_iterations)
        try:
            assert np.array_equal(init.words(), before)                     # init is not modified
            assert (v.n_words, v.dim, v.dtype) == (init.n_words, init.dim, init.dtype)
            return v.words(), c.vocab_train_report(v), before
        finally:
            v.close()
    finally:
        init.close()


@pytest.mark.parametrize("name", TC.NAMES)
def test_case_equals_the_restatement(tctx, oracle, name):
    case, e = TC.case(name), TC.expected(oracle, name)
    tctx.clear_images()
    _register(tctx, case)
    words, rep, init = _train(tctx, case)
    print(name, {k: rep[k] for k in COUNTERS}, "differing elements:", int((words != e["words"]).sum()))
    assert np.array_equal(init, case.init_rows())
    assert words.dtype == e["words"].dtype and np.array_equal(words, e["words"])
    assert {k: int(rep[k]) for k in COUNTERS} == {k: int(e[k]) for k in COUNTERS}
    assert rep["ms_assign"] > 0 and rep["ms_sort"] > 0 and rep["ms_update"] > 0


def test_a_trained_vocabulary_serves_proposals(tctx, oracle):
    case, e = TC.case("liop"), TC.expected(oracle, "liop")
    tctx.clear_images()
    _register(tctx, case)
    init = _init(tctx, case)
    v = tctx.vocab_train(init, case.ids, case.max_iterations)
    init.close()
    try:
        hist = tctx.view_signatures(v, case.ids)
        assert tctx.vocab_report(v)["n_signatures_built"] == len(case.ids)  # it came without signatures
        exp = R.signatures(oracle, e["words"], case.descs)
        assert np.array_equal(hist, exp)
        pairs, scores = tctx.propose_pairs(v, case.ids, 3, with_scores=True)
        assert np.array_equal(scores, R.scores(exp)) and np.array_equal(pairs, R.propose(R.scores(exp), case.ns, case.ids, 3))
        assert np.array_equal(v.weights(), np.ones(v.n_words, np.uint32))
    finally:
        v.close()


@pytest.mark.parametrize("name,switch", [("sift", "set_integer_mfma"), ("sift_u8", "set_integer_mfma"), ("liop", "set_split_mfma"),
                                         ("akaze", "set_hamming_mfma")])
def test_every_exact_tile_path_gives_the_same_words(oracle, name, switch):
    """after one update the codebook is real-valued while the views stay integer: the path decision of every later assignment"""
    case, e = TC.case(name), TC.expected(oracle, name)
    c = api.Context(0)
    try:
        _register(c, case)
        getattr(c, switch)(True)
        words, rep, _ = _train(c, case)
        assert np.array_equal(words, e["words"])
        assert {k: int(rep[k]) for k in COUNTERS} == {k: int(e[k]) for k in COUNTERS}
    finally:
        c.close()


def test_isolation(oracle):
    """two trainings with a match call in between give the same words; r3dm_stats is what the match call left; the match graph is a
    fresh context's"""
    case, e = TC.case("multi_block"), TC.expected(oracle, "multi_block")
    allp = np.array([(a, b) for a in sorted(case.ids) for b in sorted(case.ids) if a < b], np.uint32)
    c = api.Context(0); f = api.Context(0)
    try:
        _register(c, case); _register(f, case)
        fresh = f.match_pairs(allp, 0.8, True)
        w1, r1, _ = _train(c, case)
        g = c.match_pairs(allp, 0.8, True)
        before = c.stats()
        w2, r2, _ = _train(c, case)
        after = c.stats()
        assert np.array_equal(w1, e["words"]) and np.array_equal(w2, e["words"])
        assert {k: r1[k] for k in COUNTERS} == {k: r2[k] for k in COUNTERS}
        assert all(a.tobytes() == b.tobytes() for a, b in zip((g.pairs, g.offsets, g.matches), (fresh.pairs, fresh.offsets, fresh.matches)))
        # r3dm_stats is left as the call found it (n_views_staged counts since r3dm_create: one codebook staging per assignment)
        assert all(getattr(before, k) == getattr(after, k) for k, _ in api.Stats._fields_ if k != "n_views_staged")
        assert after.n_views_staged == before.n_views_staged + len(e["history"])
    finally:
        c.close(); f.close()


@pytest.mark.parametrize("what", TC.REFUSALS)
def test_refusals(tctx, what):
    case = TC.case("sift")
    tctx.clear_images()
    _register(tctx, case)
    ids = list(case.ids)
    tctx.set_image(900, VC.case("sift_u8").descs[0])                          # another type
    tctx.set_image(901, np.ascontiguousarray(case.descs[0][:, :64]))          # another length
    tctx.set_image(902, np.zeros((0, 128), np.float32))                       # no rows
    init = tctx.vocab_sample(ids, 64)
    try:
        args = {"unknown_view": (ids + [777], 3), "duplicate_id": (ids + [ids[2]], 3), "mixed_type": (ids + [900], 3),
                "mixed_length": (ids + [901], 3), "view_unlike_vocab": ([901], 3), "max_iterations_0": (ids, 0), "no_rows": ([902], 3)}[what]
        mem = tctx.memory_info()
        with pytest.raises(api.R3dmError, match=INVALID):
            tctx.vocab_train(init, *args)                                     # no handle comes back: nothing is left behind
        assert tctx.memory_info() == mem
        v = tctx.vocab_train(init, ids + [902], 1)                            # the vocabulary still serves; an empty view is allowed
        assert tctx.vocab_train_report(v)["n_updates"] == 1
        assert tctx.vocab_train_report(init)["n_updates"] == 0                # a vocabulary that was not trained reports zeros
        v.close()
        with pytest.raises(api.R3dmError):
            init.set_weighting(2)
    finally:
        init.close()


# ---------------------------------------------------------------------------------------------------- idf-weighted scores
def _register_idf(c, case, ids=None):
    c.clear_images()
    for k, d in enumerate(case.descs):
        if ids is None or case.ids[k] in ids:
            c.set_image(case.ids[k], d)


@pytest.mark.parametrize("name", TC.IDF_NAMES)
def test_idf_case_equals_the_restatement(tctx, oracle, name):
    case, e = TC.idf_case(name), TC.idf_expected(oracle, name)
    _register_idf(tctx, case)
    v = tctx.vocab_from_rows(case.vocab)
    try:
        assert np.array_equal(v.weights(), np.ones(16, np.uint32))
        v.set_weighting(api.VOCAB_WEIGHT_IDF)
        pairs, scores = tctx.propose_pairs(v, case.ids, case.top_k, with_scores=True)
        assert np.array_equal(v.weights(), e["idf"]["q"])
        assert np.array_equal(scores, e["idf"]["scores"]) and np.array_equal(pairs, e["idf"]["pairs"])
        assert np.array_equal(tctx.view_signatures(v, case.ids), e["hist"])      # unaffected by the weighting
        assert np.array_equal(v.weights(), e["idf"]["q"])                         # ... which is the last propose call's
        # COUNTS after IDF: today's scores again
        v.set_weighting(api.VOCAB_WEIGHT_COUNTS)
        pairs, scores = tctx.propose_pairs(v, case.ids, case.top_k, with_scores=True)
        assert np.array_equal(scores, R.scores(e["hist"])) and np.array_equal(pairs, e["counts"]["pairs"])
        assert np.array_equal(v.weights(), np.ones(16, np.uint32))
    finally:
        v.close()


def test_idf_weights_follow_the_listed_views(tctx, oracle):
    case = TC.idf_case("idf_rank_differs")
    _register_idf(tctx, case)
    v = tctx.vocab_from_rows(case.vocab)
    try:
        v.set_weighting(api.VOCAB_WEIGHT_IDF)
        seen = []
        for ids in (case.ids, case.ids[:3], [case.ids[4], case.ids[0], case.ids[2]]):
            e = TC.idf_expected(oracle, "idf_rank_differs", ids)
            pairs, scores = tctx.propose_pairs(v, ids, 1, with_scores=True)
            assert np.array_equal(v.weights(), e["idf"]["q"]) and np.array_equal(scores, e["idf"]["scores"]) and np.array_equal(pairs, e["idf"]["pairs"])
            seen.append(v.weights().tobytes())
        assert len(set(seen)) == 3
    finally:
        v.close()


def test_log2_q8_through_the_weights(tctx):
    """word w is held by the first w + 1 of N views, an empty view is listed too: q[w] = log2_q8(N, w + 1) for every df of 1 .. N, at
    N = 13 and, with the list cut, at every smaller N"""
    N = 13
    vocab = VC._one_hot_vocab()
    tctx.clear_images()
    for k in range(N):
        tctx.set_image(k, VC._view_of(vocab, np.array([1 if w >= k and w < N else 0 for w in range(16)])))
    tctx.set_image(99, np.zeros((0, 16), np.float32))
    v = tctx.vocab_from_rows(vocab)
    try:
        v.set_weighting(api.VOCAB_WEIGHT_IDF)
        for n in range(2, N + 1):
            tctx.propose_pairs(v, [99] + list(range(n)), 1)
            exp = [TR.log2_q8(n, min(w + 1, n)) if w < N else 0 for w in range(16)]
            assert v.weights().tolist() == exp, n
    finally:
        v.close()


def test_idf_refuses_a_weighted_sum_of_2_to_the_32(tctx):
    """32 byte views, one word that only the big view holds (q = log2_q8(32, 1) = 1280): ceil(2^32 / 1280) of its rows make W >= 2^32,
    refused; one row fewer is served.  (The issue's 2^19 + 1 rows cannot reach the bound: q <= 5,631 gives W < 2^32 there; a view holds
    fewer than 2^22 rows, so 16 views are too few as well.  27 MB of rows.)"""
    q_big = TR.log2_q8(32, 1)
    n_big = -(-(1 << 32) // q_big)
    assert q_big == 1280 and n_big < 1 << 22 and q_big * n_big >= 1 << 32 > q_big * (n_big - 1)
    vocab = TC._keyed(8, 4, 60, np.uint8)
    tctx.clear_images()
    for k in range(31):
        tctx.set_image(k, np.ascontiguousarray(vocab[[0, 1 + k % 2]]))
    big = np.ascontiguousarray(np.repeat(vocab[3:4], n_big, axis=0))
    ids = list(range(32))
    v = tctx.vocab_from_rows(vocab)
    try:
        v.set_weighting(api.VOCAB_WEIGHT_IDF)
        tctx.set_image(31, big)
        with pytest.raises(api.R3dmError, match=UNSUPPORTED):
            tctx.propose_pairs(v, ids, 2)
        assert v.weights().tolist() == [TR.log2_q8(32, 31), TR.log2_q8(32, 16), TR.log2_q8(32, 15), q_big]
        tctx.set_image(31, big[:-1])
        assert len(tctx.propose_pairs(v, ids, 2)) > 0                        # W = 2^32 - 256
        v.set_weighting(api.VOCAB_WEIGHT_COUNTS)
        tctx.set_image(31, big)
        assert len(tctx.propose_pairs(v, ids, 2)) > 0                        # COUNTS has no such bound
    finally:
        v.close()
        tctx.clear_images()
