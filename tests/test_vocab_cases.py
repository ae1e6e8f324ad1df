"""The case table of pair proposal proven on the CPU restatement alone (no GPU): every property a case of tests/vocab_cases.py is
built for really holds in it -- otherwise the GPU test that compares the kernels with the restatement on that case shows nothing --
and the method meets its quality bar on a synthetic collection.  The GPU equals the restatement bit for bit (test_gpu_vocab.py), so
what is proven here transfers."""
import os
import re

import numpy as np
import pytest

import vocab_cases as VC
import vocab_restatement as R
from regard3d_amd import api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_are_those_of_the_header():
    h = open(os.path.join(ROOT, "include", "r3dm.h")).read()
    val = lambda name: int(re.search(r"#define\s+" + name + r"\s+(\d+)u", h).group(1))
    assert val("R3DM_VOCAB_HIST_LDS_WORDS") == VC.HIST_LDS_WORDS == api.VOCAB_HIST_LDS_WORDS
    assert val("R3DM_VOCAB_WORD_CHUNK") == VC.WORD_CHUNK == api.VOCAB_WORD_CHUNK
    assert val("R3DM_VOCAB_MAX_WORDS") == api.VOCAB_MAX_WORDS
    k = open(os.path.join(ROOT, "regard3d_amd", "csrc", "r3dm_internal.hpp")).read()
    kval = lambda name: int(re.search(r"constexpr uint32_t " + name + r" = (\d+);", k).group(1))
    assert kval("kVocabHistLdsWords") == VC.HIST_LDS_WORDS and kval("kVocabChunk") == VC.WORD_CHUNK and kval("kVocabTile") == VC.VIEW_TILE
    hpp = open(os.path.join(ROOT, "include", "r3d_compute_matches.hpp")).read()
    assert int(re.search(r"#define\s+R3DM_STAGE_PAIR_PROPOSAL\s+(\d+)u", hpp).group(1)) == api.STAGE_PAIR_PROPOSAL == 2048


def test_sample_rule():
    assert R.sample_rows([3, 0, 5], 8) == list(range(8))                        # T == n_words: every row
    assert R.sample_rows([10], 2) == [2, 7] and R.sample_rows([4, 6], 5) == [1, 3, 5, 7, 9]
    rows = R.sample_rows([1000, 24], 64)
    assert rows == sorted(set(rows)) and rows[0] == 8 and rows[-1] == 1016      # strictly ascending, centred in their strides
    with pytest.raises(AssertionError):
        R.sample_rows([3, 4], 8)


@pytest.mark.parametrize("name", VC.NAMES)
def test_case_is_well_formed(oracle, name):
    c, e = VC.case(name), VC.expected(oracle, name)
    n = len(c.descs)
    assert len(set(c.ids)) == n == len(c.ids) and c.top_k >= 1
    assert e["hist"].shape == (n, len(e["vocab"])) and e["hist"].sum(axis=1).tolist() == c.ns
    s = e["scores"]
    assert np.array_equal(s, s.T) and not s.diagonal().any()
    assert all(s[i, j] <= min(c.ns[i], c.ns[j]) for i in range(n) for j in range(n))
    p = e["pairs"]
    assert len(p) <= n * c.top_k and (p[:, 0] < p[:, 1]).all() and [tuple(x) for x in p] == sorted({tuple(x) for x in p.tolist()})
    # the case discriminates: some pair is proposed, and unless the case proposes everything some pair is left out
    live = sum(1 for x in c.ns if x)
    assert len(p) > 0 and (len(p) < live * (live - 1) // 2 or c.top_k >= live - 1)


def test_shapes_sit_on_the_edges_they_are_named_for(oracle):
    assert len(VC.case("views13").descs) == 13 and len(VC.case("views17").descs) == 17
    assert len(VC.case("views_two_tiles").descs) == VC.VIEW_TILE + 3
    assert len(VC.expected(oracle, "words67")["vocab"]) == 67 and 67 % 4 and 67 % VC.WORD_CHUNK
    assert len(VC.expected(oracle, "words_chunk_plus_1")["vocab"]) == VC.WORD_CHUNK + 1
    for name, nw in (("hist_lds_bound", VC.HIST_LDS_WORDS), ("hist_lds_bound_plus_1", VC.HIST_LDS_WORDS + 1)):
        h = VC.expected(oracle, name)["hist"]
        assert h.shape[1] == nw and h[:, nw - 1].sum() >= 5 and h[:, :64].sum() < h.sum()      # the last word counts; the words spread
    kinds = {n: VC.case(n).descs[0] for n in ("sift", "liop", "akaze", "sift_u8")}
    assert kinds["sift"].dtype == np.float32 and kinds["sift"].shape[1] == 128 and np.array_equal(kinds["sift"], np.rint(kinds["sift"]))
    assert kinds["liop"].shape[1] == 144 and not np.array_equal(kinds["liop"], np.rint(kinds["liop"]))
    assert kinds["akaze"].dtype == np.uint8 and kinds["akaze"].shape[1] == 61 and VC.case("akaze").binary
    assert kinds["sift_u8"].dtype == np.uint8 and np.array_equal(kinds["sift_u8"], kinds["sift"].astype(np.uint8))
    assert np.array_equal(VC.expected(oracle, "sift_u8")["hist"], VC.expected(oracle, "sift")["hist"])


def test_ties_go_to_the_lowest_word(oracle):
    c, e = VC.case("ties"), VC.expected(oracle, "ties")
    assert np.array_equal(c.vocab[2], c.vocab[0]) and np.array_equal(c.vocab[3], c.vocab[1])
    assert any((d == c.vocab[2]).all(axis=1).any() for d in c.descs)           # rows equal to a duplicated word exist
    assert not e["hist"][:, 2:4].any() and e["hist"][:, :2].all()               # ... and are counted under the lower index


def _picks(oracle, name, order_by=None):
    c, e = VC.case(name), VC.expected(oracle, name)
    return [c.ids[j] for j in R.rank(0, e["scores"], c.ns, c.ids, order_by)]


def test_key_cases_separate_the_key_from_its_neighbours(oracle):
    # 1. the key ranks otherwise than the raw score
    assert _picks(oracle, "key_beats_raw_score") == [1, 2, 3, 4] and _picks(oracle, "key_beats_raw_score", VC.raw_score) == [3, 4, 1, 2]
    e = VC.expected(oracle, "key_beats_raw_score")
    assert e["scores"][0, 1] == 3 and e["scores"][0, 2] == 10
    # 2. equal fractions of different denominators tie, and the lower view id comes first
    c, e = VC.case("key_equal_fractions"), VC.expected(oracle, "key_equal_fractions")
    assert (int(e["scores"][0, 1]), c.ns[1], int(e["scores"][0, 2]), c.ns[2]) == (3, 6, 2, 4)
    assert R.key(3, 10, 6) == R.key(2, 10, 4) == 1 << 31
    assert _picks(oracle, "key_equal_fractions") == [4, 5, 7, 8] and _picks(oracle, "key_equal_fractions", VC.raw_score) == [7, 8, 4, 5]
    # 3. two fractions a float32 division cannot tell apart, which the integer key can
    (s1, n1), (s2, n2) = VC.float_tie()
    c, e = VC.case("key_below_float_resolution"), VC.expected(oracle, "key_below_float_resolution")
    assert (int(e["scores"][0, 1]), c.ns[1], int(e["scores"][0, 2]), c.ns[2]) == (s1, n1, s2, n2) and c.ns[0] >= max(n1, n2)
    assert np.float32(s1) / np.float32(n1) == np.float32(s2) / np.float32(n2) and R.key(s1, c.ns[0], n1) < R.key(s2, c.ns[0], n2)
    assert _picks(oracle, "key_below_float_resolution") == [7, 8, 5, 6] and _picks(oracle, "key_below_float_resolution", VC.float_fraction) == [5, 6, 7, 8]
    # ... and each difference reaches the proposal: with top_k 1 view 0's pick is another pair
    for name, other in (("key_beats_raw_score", VC.raw_score), ("key_equal_fractions", VC.raw_score), ("key_below_float_resolution", VC.float_fraction)):
        c, e = VC.case(name), VC.expected(oracle, name)
        assert c.top_k == 1 and not np.array_equal(e["pairs"], R.propose(e["scores"], c.ns, c.ids, 1, other)), name


def test_degenerate_cases(oracle):
    c, e = VC.case("empty_view"), VC.expected(oracle, "empty_view")
    assert c.ns[2] == 0 and not e["hist"][2].any() and c.ids[2] not in e["pairs"]          # proposes nothing, proposed by nobody
    assert R.rank(2, e["scores"], c.ns, c.ids) == [] and all(2 not in R.rank(i, e["scores"], c.ns, c.ids) for i in range(5))
    c, e = VC.case("every_row_a_word"), VC.expected(oracle, "every_row_a_word")
    assert sum(c.ns) == len(e["vocab"]) == 64
    assert np.array_equal(e["hist"], np.kron(np.eye(4, dtype=np.uint32), np.ones(16, np.uint32)))   # every histogram: its own rows' indicator
    c, e = VC.case("top_k_1"), VC.expected(oracle, "top_k_1")
    assert c.top_k == 1 and 3 <= len(e["pairs"]) <= 6
    c, e = VC.case("top_k_everything"), VC.expected(oracle, "top_k_everything")
    assert c.top_k >= len(c.descs) - 1 and len(e["pairs"]) == 15


@pytest.mark.parametrize("kind", ["sift", "liopc"])
def test_quality_bar_of_the_method(oracle, kind):
    """24 overlapping views of 512 rows, 1,024 sampled words, top_k 6: every one of the 66 pairs of views less than 4 apart (the views
    that share features) is proposed, and at most 90 of the 276 pairs are.  Measured with this sample rule: 78 pairs, recall 1.0,
    for both kinds.  (akaze reaches 0.909 at these sizes and is not under the bar.)"""
    sc = synth.make_scene(24, 512, kind=kind, seed=11)
    ids = list(range(24))
    vocab = R.sample_vocab(sc.descs, 1024)
    s = R.scores(R.signatures(oracle, vocab, sc.descs))
    pairs = {tuple(p) for p in R.propose(s, [512] * 24, ids, 6).tolist()}
    must = {(i, j) for i in range(24) for j in range(i + 1, 24) if j - i < 4}
    assert len(must) == 66 and must <= pairs and len(pairs) <= 90, (len(pairs), len(must - pairs))
