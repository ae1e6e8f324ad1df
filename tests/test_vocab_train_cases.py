"""The case table of vocabulary training and idf-weighted scores proven on the CPU restatement alone (no GPU): every property a case
of tests/vocab_train_cases.py is built for really holds in it -- otherwise the GPU test that compares the kernels with the restatement
on that case shows nothing.  The GPU equals the restatement bit for bit (test_gpu_vocab_train.py), so what is proven here transfers."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import vocab_cases as VC
import vocab_restatement as R
import vocab_train_cases as TC
import vocab_train_restatement as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["r3dm_vocab_train", "r3dm_vocab_train_report", "r3dm_vocab_set_weighting", "r3dm_vocab_weights"]


# ------------------------------------------------------------------------------------------------- the interface
@pytest.mark.parametrize("lib", ["libr3dm.so", "libr3dm_dev.so"])
def test_new_symbols_are_exported_by_both_libraries(lib):
    L = C.CDLL(os.path.join(ROOT, "regard3d_amd", lib))
    for name in NEW:
        assert hasattr(L, name), (lib, name)


def test_new_symbols_are_declared_bound_and_listed():
    from regard3d_amd import api
    L = api.load_library()
    h = open(os.path.join(ROOT, "include", "r3dm.h")).read()
    for name in NEW:
        assert name in api.EXPORTS and re.search(r"\b" + name + r"\s*\(", h), name
        assert getattr(L, name).argtypes is not None, name
    assert all(hasattr(api.Context, n) for n in ("vocab_train", "vocab_train_report")) and all(hasattr(api.Vocab, n) for n in ("set_weighting", "weights"))
    assert "#define R3DM_VOCAB_WEIGHT_COUNTS 0" in h and "#define R3DM_VOCAB_WEIGHT_IDF    1" in h
    assert (api.VOCAB_WEIGHT_COUNTS, api.VOCAB_WEIGHT_IDF) == (0, 1)
    assert int(re.search(r"#define\s+R3DM_VOCAB_TRAIN_BLOCK\s+(\d+)u", h).group(1)) == TC.BLOCK
    k = open(os.path.join(ROOT, "regard3d_amd", "csrc", "r3dm_internal.hpp")).read()
    assert int(re.search(r"constexpr uint32_t kVocabTrainBlock = (\d+);", k).group(1)) == TC.BLOCK
    # the report struct: the header's fields in api.VocabTrainStats' order; null handles are refused
    body = h[h.index("R3DM_VOCAB_TRAIN_BLOCK 256u"):h.index("} r3dm_vocab_train_stats;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.strip() for grp in re.findall(r"\b(?:uint64_t|double|uint32_t)\s+([\w\s,]+);", body) for f in grp.split(",")]
    assert fields == [f for f, _ in api.VocabTrainStats._fields_]
    out = C.c_void_p()
    assert L.r3dm_vocab_train(None, None, None, 0, 1, C.byref(out)) == -1 and L.r3dm_vocab_train_report(None, None) == -1
    assert L.r3dm_vocab_set_weighting(None, 1) == -1 and L.r3dm_vocab_weights(None, None) == -1


# ------------------------------------------------------------------------------------------------- training
def test_scenes_train_for_a_while_and_stop_both_ways(oracle):
    stops = {}
    for name in TC.SCENES:
        c, e = TC.case(name), TC.expected(oracle, name)
        assert len(c.descs) == 12 and c.ns == [96] * 12 and len(e["words"]) == 64
        assert e["n_updates"] >= 3, name
        assert e["converged"] == (e["n_moved"] == 0) and e["n_rows_assigned"] == len(e["history"]) * sum(c.ns)
        assert e["converged"] or e["n_updates"] == c.max_iterations
        assert not np.array_equal(e["words"], c.init_rows())
        stops[name] = "converged" if e["converged"] else "cap"
    assert all(TC.case(n).max_iterations == 12 for n in ("sift", "sift_u8", "liop", "akaze"))
    assert "converged" in stops.values() and "cap" in stops.values(), stops
    kinds = {n: TC.case(n).descs[0] for n in TC.SCENES}
    assert kinds["msurf"].dtype == np.float32 and kinds["msurf"].shape[1] == 64 and not np.array_equal(kinds["msurf"], np.rint(kinds["msurf"]))
    assert kinds["akaze"].shape[1] == 61 and TC.case("akaze").binary and kinds["sift_u8"].dtype == np.uint8
    # byte rows are not float rows rounded at the end: the two SIFT trainings part ways
    assert not np.array_equal(TC.expected(oracle, "sift")["words"].astype(np.uint8), TC.expected(oracle, "sift_u8")["words"])
    # an integer codebook becomes real-valued with the first update
    w = TC.expected(oracle, "sift")["words"]
    assert not np.array_equal(w, np.rint(w))


def _first_assignment(oracle, c):
    rows = np.concatenate([d for d in c.descs if len(d)])
    return rows, R.words_of(oracle, c.init_rows(), rows, c.binary)


def test_block_and_view_seams(oracle):
    c = TC.case("multi_block")
    _, a = _first_assignment(oracle, c)
    cnt = np.bincount(a, minlength=5)
    assert len(c.descs) == 6 and c.ns == [400] * 6 and cnt.min() > 100 and (cnt > TC.BLOCK).sum() >= 4 and (cnt % TC.BLOCK != 0).all() and cnt.max() > 3 * TC.BLOCK
    assert TC.expected(oracle, "multi_block")["n_updates"] == 3 and not TC.expected(oracle, "multi_block")["converged"]
    c, e = TC.case("block_seam"), TC.expected(oracle, "block_seam")
    _, a = _first_assignment(oracle, c)
    assert np.bincount(a, minlength=6).tolist() == [TC.BLOCK, TC.BLOCK + 1, TC.BLOCK - 1, 40, 1, 0]
    assert e["n_empty"] == 1 and e["max_members"] == TC.BLOCK + 1 and np.array_equal(e["words"][5], c.vocab[5])
    for c in (TC.case("block_seam"), TC.case("view_seams")):
        _, a = _first_assignment(oracle, c)
        assert 33 in c.ns and 0 in c.ns[1:-1] and c.ids != sorted(c.ids)        # the 32-row tile group straddled, an empty view inside
        view = np.repeat(np.arange(len(c.ns)), c.ns)
        assert len(set(view[a == 0].tolist())) >= 3                               # a word's members in three views or more
        assert not np.array_equal(TC.expected(oracle, c.name)["words"], c.vocab)


def test_degenerate_words(oracle):
    c, e = TC.case("one_big_word"), TC.expected(oracle, "one_big_word")
    _, a = _first_assignment(oracle, c)
    assert not a.any() and e["n_empty"] == 3 and e["max_members"] == sum(c.ns) == 600 and e["converged"] and e["n_updates"] == 1
    assert np.array_equal(e["words"][1:], c.vocab[1:]) and not np.array_equal(e["words"][0], c.vocab[0])
    c, e = TC.case("duplicate_words"), TC.expected(oracle, "duplicate_words")
    _, a = _first_assignment(oracle, c)
    assert np.array_equal(c.vocab[5], c.vocab[2]) and (a == 2).any() and not (a == 5).any()
    assert e["n_empty"] == 1 and np.array_equal(e["words"][5], c.vocab[5]) and not np.array_equal(e["words"][2], c.vocab[2])
    c, e = TC.case("distance_tie"), TC.expected(oracle, "distance_tie")
    rows, a = _first_assignment(oracle, c)
    d = ((rows[:4, None, :] - c.vocab[None, :2, :]) ** 2).sum(axis=2)
    assert (d[:, 0] == d[:, 1]).all() and not np.array_equal(c.vocab[0], c.vocab[1]) and a[:4].tolist() == [0] * 4
    assert e["words"][0, 0] == np.float32(4.0 / 6.0) and e["words"][1, 0] == 2.0


def test_f32_arithmetic_separates_the_rule_from_its_neighbours(oracle):
    c, e = TC.case("f32_arithmetic"), TC.expected(oracle, "f32_arithmetic")
    rows, a = _first_assignment(oracle, c)
    assert np.bincount(a).tolist() == [2 * TC.BLOCK, 3, 2] and e["converged"] and e["n_updates"] == 1
    m = rows[a == 0]
    rule = TR.mean_f32(m)
    assert np.array_equal(rule, e["words"][0])
    assert rule[0] == 2.0 ** 21 + 0.25 and rule[1] == 2.0 ** 21               # dimension 0 above the f32 tie, dimension 1 on it (to even)
    for how in (dict(order="reversed"), dict(order="flat"), dict(acc=np.float32)):
        assert not np.array_equal(TR.mean_f32(m, **how), rule), how
    assert TR.mean_f32(m, order="flat")[0] == 2.0 ** 21 and TR.mean_f32(m, order="reversed")[1] == 2.0 ** 21 + 0.25
    # a third that another float when the division is done in float
    s = TC.float_division_differs()
    m1 = rows[a == 1]
    assert int(m1[:, 2].astype(np.float64).sum()) == s
    assert TR.mean_f32(m1)[2] == np.float32(s / 3.0) != TR.mean_f32(m1, divide=np.float32)[2]
    assert np.array_equal(e["words"][1], TR.mean_f32(m1))


def test_u8_and_bin_roundings(oracle):
    e = TC.expected(oracle, "u8_rounding")
    assert e["words"].dtype == np.uint8 and e["converged"]
    assert e["words"][0].tolist() == [2, 255, 1, 0, 7, 0, 0, 0]                 # 1.5, 254.5, 0.5 round up
    assert e["words"][1].tolist() == [1, 2, 0, 0, 0, 0, 0, 100]                 # 4/3, 5/3, 1/3
    assert e["words"][2].tolist() == [2, 1, 2, 0, 0, 0, 0, 200]                 # 6/4 up, 5/4, 7/4
    c, e = TC.case("bin_majority"), TC.expected(oracle, "bin_majority")
    assert c.binary and e["words"][0, 0] == 0b0110 and e["words"][0, 31] == 0x80 and not e["words"][0, 1:31].any()
    assert e["words"][1, 9] == 0b00111111 and not e["words"][1, :8].any() and (e["words"][1, 10:] == 0xFF).all()


def test_stop_rules(oracle):
    e = TC.expected(oracle, "max_iterations_1")
    assert e["n_updates"] == 1 and not e["converged"] and e["history"] == [1152] and e["n_moved"] == 1152
    c, e = TC.case("fixed_point"), TC.expected(oracle, "fixed_point")
    assert e["n_updates"] == 1 and e["converged"] and e["history"] == [64, 0] and np.array_equal(e["words"], c.init_rows())
    with pytest.raises(AssertionError):
        TR.train(oracle, c.init_rows(), c.descs, 0)


# ------------------------------------------------------------------------------------------------- idf
def test_log2_q8():
    assert TR.log2_q8(5, 5) == 0 and TR.log2_q8(8, 1) == 768 and TR.log2_q8(3, 2) == 149
    assert TR.log2_q8(4194240, 1) == 5631 and max(TR.log2_q8(4194240, d) for d in (1, 2, 3, 1000)) <= 5631
    for N in range(1, 301):
        for df in range(1, N + 1):
            q, x = TR.log2_q8(N, df), 256.0 * math.log2(N / df)
            assert x - 1.0 - 1e-9 < q <= x + 1e-9, (N, df)
        assert TR.log2_q8(N, N) == 0


def test_idf_cases(oracle):
    c, e = TC.idf_case("idf_rank_differs"), TC.idf_expected(oracle, "idf_rank_differs")
    q, W, s = e["idf"]["q"], [int(x) for x in e["idf"]["W"]], e["idf"]["scores"]
    assert (e["hist"][:, 0] > 0).all() and q[0] == 0 and (q[1:7] > 0).all()           # the word of every view weighs nothing
    counts_rank = [c.ids[j] for j in R.rank(0, e["counts"]["scores"], e["ns"], c.ids)]
    idf_rank = [c.ids[j] for j in R.rank(0, s, W, c.ids)]
    assert counts_rank[0] == 3 and idf_rank[0] == 2 and counts_rank != idf_rank
    assert not np.array_equal(e["counts"]["pairs"], e["idf"]["pairs"]) and [2, 9] in e["idf"]["pairs"].tolist() and [3, 9] in e["counts"]["pairs"].tolist()
    # N follows the list: the same views, fewer of them, other weights
    sub = TC.idf_expected(oracle, "idf_rank_differs", c.ids[:3])
    assert not np.array_equal(sub["idf"]["q"], q)
    c, e = TC.idf_case("idf_zero_view"), TC.idf_expected(oracle, "idf_zero_view")
    assert e["idf"]["W"][2] == 0 and e["ns"][2] > 0 and c.ids[2] not in e["idf"]["pairs"] and c.ids[2] in e["counts"]["pairs"]
    c, e = TC.idf_case("idf_key_tie"), TC.idf_expected(oracle, "idf_key_tie")
    s, W = e["idf"]["scores"], [int(x) for x in e["idf"]["W"]]
    assert R.key(s[0, 1], W[0], W[1]) == R.key(s[0, 2], W[0], W[2]) > 0 and c.ids[2] < c.ids[1]
    assert [c.ids[j] for j in R.rank(0, s, W, c.ids)][:2] == [c.ids[2], c.ids[1]]
    assert c.top_k == 1 and [4, 9] in e["idf"]["pairs"].tolist()                      # view 0's one pick is the lower id


def test_the_bound_on_W():
    """q <= 5,631, so a view of 2^19 + 1 rows cannot reach W = 2^32; a view holds fewer than 2^22 rows, so q must exceed 1,024: 32
    listed views and a word that one of them holds (q = 1,280) reach it with 3,355,444 rows"""
    assert 5631 * ((1 << 19) + 1) < 1 << 32 and TR.log2_q8(16, 1) * ((1 << 22) - 1) < 1 << 32
    q = TR.log2_q8(32, 1)
    n = -(-(1 << 32) // q)
    assert q == 1280 and n == 3355444 < 1 << 22 and q * n >= 1 << 32 > q * (n - 1)
    hist = np.zeros((2, 4), np.int64)
    hist[0, 3] = n; hist[1, 0] = 2
    assert TR.weighted_scores(hist, np.array([11, 0, 0, q], np.uint32))[1][0] >= 1 << 32
