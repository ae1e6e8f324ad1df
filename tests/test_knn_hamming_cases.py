"""Hamming k-NN on the i8 MFMA tiles (kernels_match_knn8.hip) evaluated in numpy, without a GPU (knn_hamming_cases.py):
  * the biased integer keys, read as floats, order as the integers do -- the float list code runs on them unchanged;
  * the per-lane-half lists (lexicographic top-KL of a half's rows, padding rows included), merged under (key, row), ARE the
    restatement's k-NN on every data set of tests/test_gpu_knn_hamming_tiles.py, and no padding row comes out;
  * the preconditions those data sets are trusted for hold."""
import numpy as np
import pytest

import certificate_cases as CC
import knn_hamming_cases as H
import knn_restatement as R


def test_biased_keys_order_as_floats():
    """every key popcount(a) - 2 a.q of a row of up to 512 bits lies in [-512, 512]: the float with the bits key + 0x3F800000 is a
    normal positive number and the floats ascend strictly with the keys; the padding rows' key is finite, above all of them and
    below the +inf of an empty list entry"""
    keys = np.arange(-512, 513)
    f = H.biased_key_floats(keys)
    assert np.isfinite(f).all() and (f > 0).all() and (f >= np.finfo(np.float32).tiny).all()
    assert (np.diff(f) > 0).all()
    assert f[512] == np.float32(1.0)
    for x in range(0, len(keys), 37):                                     # ... and pairwise: '<' and '==' agree with the integers
        assert np.array_equal(f[x] < f, keys[x] < keys) and np.array_equal(f[x] == f, keys[x] == keys)
    pad = np.array([H.PAD_KEY], np.uint32).view(np.float32)[0]
    assert np.isfinite(pad) and pad > f.max() and pad < np.float32(np.inf)


@pytest.mark.parametrize("name,a,b,ref", H.gpu_datasets(), ids=[d[0] for d in H.gpu_datasets()])
def test_half_lists_merge_to_the_restatement(name, a, b, ref):
    n = a.shape[0]
    for k in (1,) + H.KS:
        if k > n or (k == 1 and n != 1):
            continue
        idx, dist = H.half_lists_knn(a, b, k)
        assert np.array_equal(idx, ref[0][:, :k]) and np.array_equal(dist, ref[1][:, :k]), (name, k)
        assert (idx < n).all() and (dist < 2.0 ** 23).all(), (name, k)      # no padding row


def test_restatement_depth_is_the_restatement():
    """the cached 8-column restatement's first k columns are knn(k)"""
    a, b, ref = H.random_rows(97, 40, 61)
    for k in H.KS:
        ri, rd = R.knn(a, b, k, binary=True)
        assert np.array_equal(ri, ref[0][:, :k]) and np.array_equal(rd, ref[1][:, :k])


# ---------------------------------------------------------------------------------------------------- preconditions
def test_tile_counts_cover_one_to_nine_tiles_and_the_padding_case():
    tiles = sorted({H.n_tiles(n) for n in H.TILE_ROWS_N})
    assert tiles == [1, 2, 3, 4, 5, 8, 9]
    assert {H.n_tiles(n) % 2 for n in H.TILE_ROWS_N} == {0, 1}             # both tails of the double-stepped loop
    assert max(tiles) >= 3 * 3                                             # each of the three buffers holds a third tile
    assert any(n % CC.TILE_ROWS == 0 for n in H.TILE_ROWS_N) and any(n % CC.TILE_ROWS == 1 for n in H.TILE_ROWS_N)
    assert [n for n in H.TILE_ROWS_N if n in H.KS] == [3, 8]               # the sizes at which n = k is run
    # n = k: a lane half holds fewer than KL real rows and the padding rows enter its list
    for n in (3, 8):
        half = H.half_of_rows(n)
        assert min((half == 0).sum(), (half == 1).sum()) < H.kl_of(n)


def test_query_counts_cover_idle_waves_and_an_idle_workgroup():
    """a workgroup serves 4 waves x NJ query tiles (NJ = 2 at 8 words, 1 at 16): 1 query leaves three waves idle, 33 and 129 end inside
    a workgroup, 257 = 9 tiles starts a workgroup whose later waves have no tile"""
    assert [H.n_tiles(q) for q in H.QUERY_COUNTS] == [1, 2, 5, 9]
    for nj in (1, 2):
        per_wg = 4 * nj
        assert any(H.n_tiles(q) % per_wg != 0 for q in H.QUERY_COUNTS)
        assert any(H.n_tiles(q) > per_wg and H.n_tiles(q) % per_wg <= nj for q in H.QUERY_COUNTS)   # a trailing workgroup with one busy wave


def test_byte_lengths_cover_both_kernels_and_their_ragged_rows():
    assert [H.words_of(x) for x in H.BYTE_LENGTHS] == [8, 8, 16, 16]
    assert {x % 4 for x in H.BYTE_LENGTHS} == {0, 1}


@pytest.mark.parametrize("nbytes", (32, 61, 64))
def test_dense_ties_precondition(nbytes):
    a, b, _ = H.dense_ties(nbytes)
    assert a.shape == (289, nbytes) and b.shape == (161, nbytes)
    for k in H.KS:
        t = H.ties_across_halves(a, b, k)
        print(f"{nbytes} bytes, k = {k}: k-th and (k + 1)-th tie across the lane halves for {t} of 161 queries")
        assert t >= 20


def test_duplicated_rows_span_both_halves_of_three_tiles():
    half = H.half_of_rows(101)
    assert {(r // CC.TILE_ROWS, half[r]) for r in H.DUP_ROWS} == {(t, h) for t in (0, 1, 2) for h in (0, 1)}
    for nbytes in (32, 61, 64):
        a, b, ref = H.duplicated_rows(nbytes)
        assert ref[0][0].tolist() == list(H.DUP_ROWS[:8]) and (ref[1][0] == 0).all()


def test_all_identical_answer():
    for nbytes in (32, 61, 64):
        a, b, ref = H.all_identical(nbytes)
        assert a.shape[0] == 70 and (ref[0] == np.arange(8)[None, :]).all() and (ref[1][:3] == 0).all()


def test_tie_across_halves_layout():
    for nbytes in (32, 61, 64):
        a, b, ref, near, A, B, C = H.tie_across_halves(nbytes)
        assert A < B < C and A // 32 == B // 32 == 1 and C // 32 == 2
        assert CC._lane_half(A % 32) == 0 and CC._lane_half(B % 32) == 1 and CC._lane_half(C % 32) == 0
        assert all(CC._lane_half(r % 32) == 0 and r // 32 == 1 for r in near)
        d = R.hamming_all(a, b[:1])[0]
        assert d[near].tolist() == [1, 2, 3, 4, 5, 6, 7] and d[[A, B, C]].tolist() == [9, 9, 9]
        assert (np.delete(d, near + [A, B, C]) > 9).all()
        assert ref[0][0].tolist() == near + [A] and ref[1][0].tolist() == [1, 2, 3, 4, 5, 6, 7, 9]
        assert R.knn(a, b, 10, binary=True)[0][0, 8:].tolist() == [B, C]


# ---------------------------------------------------------------------------------------------------- the interface, without a GPU
def test_switch_and_counter_are_exported():
    """r3dm_set_knn_hamming_tiles is declared, exported and refuses a null context; n_knn_hamming_tiles is the last field of the
    statistics, in the header as in api.Stats"""
    import os
    import re
    from regard3d_amd import api
    L = api.load_library()
    assert "r3dm_set_knn_hamming_tiles" in api.EXPORTS and hasattr(L, "r3dm_set_knn_hamming_tiles")
    assert L.r3dm_set_knn_hamming_tiles(None, 1) != 0
    assert api.Stats._fields_[-1][0] == "n_knn_hamming_tiles"
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "r3dm.h")).read()
    body = hdr[:hdr.index("} r3dm_stats;")]
    body = re.sub(r"/\*.*?\*/", "", body[body.rindex("typedef struct"):], flags=re.S)
    fields = re.findall(r"\b(?:uint64_t|double|uint32_t|float)\s+(\w+)\s*;", body)
    assert fields == [f[0] for f in api.Stats._fields_]
    assert hasattr(api.Context, "set_knn_hamming_tiles")
