"""Pair proposal from bag-of-words view signatures on the GPU (include/r3dm.h, "Pair proposal"): `-m gpu`.
Every case of tests/vocab_cases.py against the numpy restatement (tests/vocab_restatement.py) with == : the sampled words, the
histograms, the scores, the pairs.  Then what the contract promises around them: the same words on every exact tile path, stale
signatures rebuilt and only those, no dependence on what the context did before, no idle cost, the refusals, and the stage."""
import os

import numpy as np
import pytest

import vocab_cases as VC
import vocab_restatement as R
from regard3d_amd import api, synth

pytestmark = pytest.mark.gpu
INVALID = r"-> -1:"                                  # R3DM_ERR_INVALID in an R3dmError


@pytest.fixture(scope="module")
def vctx():
    c = api.Context(0)
    yield c
    c.close()


def _register(c, case, only=None):
    for k, d in enumerate(case.descs):
        if only is None or k in only:
            c.set_image(case.ids[k], d, binary=case.binary)


def _vocab(c, case):
    return c.vocab_from_rows(case.vocab, binary=case.binary) if case.vocab is not None else c.vocab_sample(case.ids, case.n_words)


def _run(c, case):
    v = _vocab(c, case)
    try:
        words = v.words()
        hist = c.view_signatures(v, case.ids)
        pairs, scores = c.propose_pairs(v, case.ids, case.top_k, with_scores=True)
        return words, hist, scores, pairs, c.vocab_report(v)
    finally:
        v.close()


def _csr(g):
    return g.pairs.copy(), g.offsets.copy(), g.matches.copy()


@pytest.mark.parametrize("name", VC.NAMES)
def test_case_equals_the_restatement(vctx, oracle, name):
    case, e = VC.case(name), VC.expected(oracle, name)
    vctx.clear_images()
    _register(vctx, case)
    words, hist, scores, pairs, rep = _run(vctx, case)
    assert words.dtype == e["vocab"].dtype and np.array_equal(words, e["vocab"])
    assert np.array_equal(hist, e["hist"])
    assert np.array_equal(scores, e["scores"])
    assert np.array_equal(pairs, e["pairs"])
    # the second call of _run found every signature of the first
    assert rep["n_signatures_cached"] == len(case.descs) and rep["n_signatures_built"] == 0 and rep["n_rows_quantised"] == 0


def test_report_counts_the_first_call(vctx, oracle):
    case = VC.case("empty_view")
    vctx.clear_images()
    _register(vctx, case)
    v = _vocab(vctx, case)
    pairs = vctx.propose_pairs(v, case.ids, case.top_k)
    rep = vctx.vocab_report(v)
    v.close()
    assert np.array_equal(pairs, VC.expected(oracle, "empty_view")["pairs"])
    assert rep["n_signatures_built"] == 5 and rep["n_signatures_cached"] == 0 and rep["n_rows_quantised"] == sum(case.ns)
    assert rep["ms_quantise"] > 0 and rep["ms_histogram"] > 0 and rep["ms_score"] > 0 and rep["ms_select"] > 0


@pytest.mark.parametrize("name,switch,counter", [("sift", "set_integer_mfma", "n_integer_mfma"), ("sift_u8", "set_integer_mfma", "n_integer_mfma"),
                                                 ("liop", "set_split_mfma", "n_split_mfma"), ("akaze", "set_hamming_mfma", "n_hamming_mfma")])
def test_every_exact_tile_path_gives_the_same_words(oracle, name, switch, counter):
    case, e = VC.case(name), VC.expected(oracle, name)
    c = api.Context(0)
    try:
        _register(c, case)
        getattr(c, switch)(True)
        before = c.stats()
        v = _vocab(c, case)
        hist = c.view_signatures(v, case.ids)
        v.close()
        after = c.stats()
        assert np.array_equal(hist, e["hist"])
        # r3dm_stats is left as the call found it; that the switched path really ran shows on a match call of the same views
        # (n_views_staged counts since r3dm_create: the codebook's staging is one more, as every array a raw-list entry stages is)
        assert all(getattr(before, k) == getattr(after, k) for k, _ in api.Stats._fields_ if k != "n_views_staged")
        assert after.n_views_staged == before.n_views_staged + 1
        c.match_pairs(np.array([[case.ids[0], case.ids[1]]], np.uint32), 0.8, not case.binary)
        assert getattr(c.stats(), counter) == 1
    finally:
        c.close()


def test_stale_signatures_are_rebuilt_and_only_those(oracle):
    case = VC.case("sift")
    other = synth.make_scene(1, 80, "sift", seed=77).descs[0]
    c = api.Context(0)
    try:
        _register(c, case)
        v = c.vocab_sample(case.ids, 64)
        first = c.view_signatures(v, case.ids)
        assert c.vocab_report(v)["n_signatures_built"] == 12
        c.set_image(case.ids[3], other)                                     # view 3 re-registered with other rows
        descs = list(case.descs); descs[3] = other
        pairs, scores = c.propose_pairs(v, case.ids, 3, with_scores=True)
        rep = c.vocab_report(v)
        assert rep["n_signatures_built"] == 1 and rep["n_signatures_cached"] == 11 and rep["n_rows_quantised"] == 80
        hist = c.view_signatures(v, case.ids)
        exp = R.signatures(oracle, v.words(), descs)
        assert np.array_equal(hist, exp) and not np.array_equal(hist[3], first[3]) and np.array_equal(np.delete(hist, 3, 0), np.delete(first, 3, 0))
        s = R.scores(exp)
        assert np.array_equal(scores, s) and np.array_equal(pairs, R.propose(s, [len(d) for d in descs], case.ids, 3))
        # ... the same as a fresh context that never saw the old rows, with the same words
        f = api.Context(0)
        try:
            for k, d in enumerate(descs):
                f.set_image(case.ids[k], d)
            fv = f.vocab_from_rows(v.words())
            fp, fs = f.propose_pairs(fv, case.ids, 3, with_scores=True)
            fv.close()
        finally:
            f.close()
        assert np.array_equal(fp, pairs) and np.array_equal(fs, scores)
        # r3dm_clear_images invalidates every signature; an unregistered view is refused
        c.clear_images()
        with pytest.raises(api.R3dmError, match=INVALID):
            c.view_signatures(v, case.ids)
        for k, d in enumerate(descs):
            c.set_image(case.ids[k], d)
        assert np.array_equal(c.view_signatures(v, case.ids), exp)
        assert c.vocab_report(v)["n_signatures_built"] == 12 and c.vocab_report(v)["n_signatures_cached"] == 0
        v.close()
    finally:
        c.close()


def test_no_dependence_on_what_the_context_did_before(oracle):
    case, e = VC.case("liop"), VC.expected(oracle, "liop")
    allp = np.array([(a, b) for a in sorted(case.ids) for b in sorted(case.ids) if a < b], np.uint32)
    c = api.Context(0); f = api.Context(0)
    try:
        _register(c, case); _register(f, case)
        fresh = _csr(f.match_pairs(allp, 0.8, True))
        fresh_stats = f.stats()
        v = c.vocab_sample(case.ids, 64)
        p1, s1 = c.propose_pairs(v, case.ids, 3, with_scores=True)
        g = _csr(c.match_pairs(allp, 0.8, True))                             # an unrelated match call between two proposals
        st = c.stats()
        v2 = c.vocab_sample(case.ids, 64)                                    # a second vocabulary: its own signatures
        p2, s2 = c.propose_pairs(v2, case.ids, 3, with_scores=True)
        p3, s3 = c.propose_pairs(v, case.ids, 3, with_scores=True)
        v.close(); v2.close()
        assert all(np.array_equal(p, e["pairs"]) for p in (p1, p2, p3)) and all(np.array_equal(s, e["scores"]) for s in (s1, s2, s3))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(g, fresh))     # the match graph after a proposal: a fresh context's
        assert st.n_pairs == fresh_stats.n_pairs and st.n_queries == fresh_stats.n_queries and st.n_match_launches == fresh_stats.n_match_launches
        # the proposed pairs through the matcher: the graph of all pairs restricted to them, bit for bit
        on = c.match_pairs(p1, 0.8, True)
        rp, rn, rm = R.restrict_graph(*fresh, p1)
        assert len(rp) < len(fresh[0])
        assert np.array_equal(on.pairs, rp) and np.array_equal(np.diff(on.offsets.astype(np.int64)), rn) and np.array_equal(on.matches, rm)
        # proposal composes with preemptive matching: the gate is a per-pair test, so gated proposed pairs == gated all pairs, restricted
        c.set_preemptive_matching(True, 32, 2)
        gated_all = _csr(c.match_pairs(allp, 0.8, True))
        gated_on = c.match_pairs(p1, 0.8, True)
        assert c.preselect_report()["n_pairs"] == len(p1)                   # the gate saw the proposed pairs, no others
        gp, gn, gm = R.restrict_graph(*gated_all, p1)
        assert 0 < len(gp) and len(gated_all[0]) < len(fresh[0])            # (the gate did drop pairs that have matches)
        assert np.array_equal(gated_on.pairs, gp) and np.array_equal(np.diff(gated_on.offsets.astype(np.int64)), gn) and np.array_equal(gated_on.matches, gm)
    finally:
        c.close(); f.close()


def test_idle_cost(oracle):
    case = VC.case("sift")
    c = api.Context(0)
    try:
        _register(c, case)
        c.match_pairs(np.array([[case.ids[0], case.ids[1]]], np.uint32))
        mem = c.memory_info()
        info = [c.view_info(i)[:2] for i in case.ids]
        v = c.vocab_sample(case.ids, 64)
        w = c.vocab_from_rows(VC.case("ties").vocab)
        assert c.memory_info() == mem and [c.view_info(i)[:2] for i in case.ids] == info
        v.close(); w.close()
        assert c.memory_info() == mem and [c.view_info(i)[:2] for i in case.ids] == info
    finally:
        c.close()


@pytest.mark.parametrize("what", VC.REFUSALS)
def test_refusals(vctx, what):
    case = VC.case("sift")
    vctx.clear_images()
    _register(vctx, case)
    ids = list(case.ids)
    T = sum(case.ns)
    vctx.set_image(900, VC.case("sift_u8").descs[0])                          # another type
    vctx.set_image(901, np.ascontiguousarray(case.descs[0][:, :64]))          # another length
    if what in ("n_words_above_T", "n_words_1", "mixed_type", "mixed_length"):
        args = {"n_words_above_T": (ids, T + 1), "n_words_1": (ids, 1), "mixed_type": (ids + [900], 64), "mixed_length": (ids + [901], 64)}[what]
        with pytest.raises(api.R3dmError, match=INVALID):
            vctx.vocab_sample(*args)                                          # no handle comes back: nothing is left behind
        if what == "n_words_above_T":
            vctx.vocab_sample(ids, T).close()                                 # ... while T itself is served
        return
    if what in ("unknown_view", "duplicate_id"):
        bad = ids + [777] if what == "unknown_view" else ids + [ids[2]]
        with pytest.raises(api.R3dmError, match=INVALID):
            vctx.vocab_sample(bad, 64)
    v = vctx.vocab_sample(ids, 64)
    try:
        call = {"top_k_0": lambda: vctx.propose_pairs(v, ids, 0, cap_pairs=100),
                "unknown_view": lambda: vctx.propose_pairs(v, ids + [777], 3),
                "duplicate_id": lambda: vctx.propose_pairs(v, ids + [ids[2]], 3),
                "view_unlike_vocab": lambda: vctx.propose_pairs(v, ids + [901], 3),
                "cap_pairs_too_small": lambda: vctx.propose_pairs(v, ids, 3, cap_pairs=3 * len(ids) - 1)}[what]
        with pytest.raises(api.R3dmError, match=INVALID):
            call()
        if what == "view_unlike_vocab":
            with pytest.raises(api.R3dmError, match=INVALID):
                vctx.view_signatures(v, [900])
        rep = vctx.vocab_report(v)
        assert rep["n_signatures_built"] == 0 and rep["n_rows_quantised"] == 0      # a refused call builds nothing
        assert len(vctx.propose_pairs(v, ids, 3, cap_pairs=3 * len(ids))) > 0        # the vocabulary still serves, at the least room accepted
    finally:
        v.close()


# ---------------------------------------------------------------------------------------------------- the stage
def _read_desc(path, dim=144):
    raw = np.fromfile(path, np.uint8)
    n = int(np.frombuffer(raw[:8].tobytes(), np.uint64)[0])
    return np.frombuffer(raw[8:8 + n * dim * 4].tobytes(), np.float32).reshape(n, dim).copy()


def test_stage_flag_on_the_synthetic_photographs(oracle, tmp_path):
    """R3DM_STAGE_PAIR_PROPOSAL from pixels: the match files are those of the switch-off run restricted to the pairs propose_pairs
    returns for the same views under the stage's defaults (T / 2 words here, top_k 20)"""
    ims, K = synth.make_photo_set(4, 240, 320, seed=5, device="cpu")
    ims = [np.ascontiguousarray(im.numpy(), np.float32) for im in ims]
    views = [dict(id=3 * k + 2, width=320, height=240, basename=f"s{k}", gray=ims[k]) for k in range(4)]
    off, on = tmp_path / "off", tmp_path / "on"
    off.mkdir(); on.mkdir()
    api.compute_matches_stage([0], str(off), views, 0.001, 0.8, 9, True, False, False)
    rep = api.compute_matches_stage([0], str(on), views, 0.001, 0.8, 9, True, False, False, proposal=True)
    descs = [_read_desc(str(off / f"s{k}.desc")) for k in range(4)]
    ids = [v["id"] for v in views]
    c = api.Context(0)
    try:
        for i, d in zip(ids, descs):
            c.set_image(i, d)
        T = sum(len(d) for d in descs)
        v = c.vocab_sample(sorted(ids), min(16384, T // 2))
        keep = c.propose_pairs(v, sorted(ids), 20)
        v.close()
    finally:
        c.close()
    assert T >= 4 and len(keep) > 0 and rep.n_putative_pairs <= len(keep)
    VC.assert_files_restricted(oracle, str(off), str(on), keep)
