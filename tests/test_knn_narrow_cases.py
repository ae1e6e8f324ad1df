"""k-NN on the narrow tiles (kernels_match_knn16.hip) evaluated in numpy, without a GPU (knn_narrow_cases.py):
  * the split planes' certificate -- K-lists per lane half over emulated split-f16 keys, the split slack -- lets through only queries
    whose k nominees are the restatement's, sends (almost) nothing to the exact scan where 2-NN is easy and (almost) everything where
    the keys' rounding exceeds every gap;
  * the integer tiles' exact lists, merged, ARE the restatement's k-NN, ties and duplicated rows included;
  * the routing predicate names the path of every case of tests/test_gpu_knn_narrow.py."""
import numpy as np
import pytest

import certificate_cases as CC
import knn_narrow_cases as N
import knn_restatement as R


# ---------------------------------------------------------------------------------------------------- split certificate
@pytest.mark.parametrize("k", (3, 8))
@pytest.mark.parametrize("case,lo,hi", N.SPLIT_CASES)
def test_split_certified_answers_are_the_restatement(case, lo, hi, k):
    a, b, (ri, rd) = N.case_views(case)
    assert N.expected_path(a, b) == "split"
    answers, certified = N.split_certificate(a, b, k)
    for q in np.flatnonzero(certified):
        assert np.array_equal(answers[q][0], ri[q, :k]) and np.array_equal(answers[q][1], rd[q, :k])
    share = 1.0 - certified.mean()
    print(f"{case}, k = {k}: exact-scan share {share:.3f}")
    if lo is not None:
        assert lo <= share <= hi


# ---------------------------------------------------------------------------------------------------- integer lists
@pytest.mark.parametrize("k", (3, 8))
@pytest.mark.parametrize("nI,nJ,dim,top", [(613, 307, 128, 256), (357, 271, 256, 128)])
def test_integer_lists_are_the_restatement(nI, nJ, dim, top, k):
    a, b = N.u8_tied(nI, nJ, dim, top)
    assert N.expected_path(a, b) == "integer"
    idx, dist, left_out = N.integer_lists_knn(a, b, k)
    ri, rd = R.knn(a, b, k)
    assert np.array_equal(idx, ri) and np.array_equal(dist, rd)
    assert left_out == 0
    planted = np.delete(np.arange(nJ // 4), 5)                            # (query 5 copied row 5 before row 4 overwrote it)
    assert (rd[planted, 0] == 0).all()                                    # the planted distance-0 neighbours
    assert ri[4, :3].tolist() == [4, 5, nI - 1] and (rd[4, :3] == 0).all()      # query 4 = row 4 and its duplicates, lowest row first


def test_integer_lists_tie_of_kth_and_next_across_halves():
    """the k-th and the (k + 1)-th neighbour tie across the lane halves, a third tied row sits un-nominated in A's half: the f32 path
    must scan (its bound equals e_k); exact lists already hold near + [A] and leave no row out that ties AND has a lower index"""
    a, b, near, A, B, C = N.tie_across_halves()
    assert N.expected_path(a, b) == "integer"
    idx, dist, left_out = N.integer_lists_knn(a, b, 8)
    assert idx[0].tolist() == near + [A] and dist[0].tolist() == [1, 2, 3, 4, 5, 6, 7, 9]
    assert left_out == 0
    ri, rd = R.knn(a, b, 8)
    assert np.array_equal(idx, ri) and np.array_equal(dist, rd)
    a, b, near, A, B, C = N.tie_across_halves(with_C=False)
    idx, _, _ = N.integer_lists_knn(a, b, 8)
    assert idx[0].tolist() == near + [A] and R.knn(a, b, 9)[0][0, 8] == B


# ---------------------------------------------------------------------------------------------------- routing
def test_exact_pair_mirror():
    z = np.zeros((4, 128), np.float32)
    def v(x):
        o = z.copy(); o[0, 0] = x; return o
    assert N.exact_pair(v(255), v(255), True)
    assert N.exact_pair(v(256), v(255), True) and not N.exact_pair(v(256), v(256), True)          # 2 D mI mJ reaches 2^24
    assert not N.exact_pair(v(257), v(1), True) and N.exact_pair(v(257), v(1), False)
    assert N.exact_pair(v(-100), v(100), True) and not N.exact_pair(v(-200), v(200), True)         # D (mI + mJ)^2 < 2^24
    assert not N.exact_pair(v(0.5), v(1), True)
    z256 = np.zeros((4, 256), np.float32); a = z256.copy(); a[0, 0] = 255; b = z256.copy(); b[0, 0] = 127
    assert not N.exact_pair(a, a, True) and N.exact_pair(b, b, True)


def test_routing_of_the_gpu_cases():
    rng = np.random.default_rng(0)
    def real(n, d): return rng.standard_normal((n, d)).astype(np.float32)
    def u8(n, d, top=256): return rng.integers(0, top, (n, d)).astype(np.uint8)
    want = {37: "integer", 64: "integer", 128: "integer", 144: "f32", 256: "f32", 300: "scan"}
    for d, p in want.items():
        assert N.expected_path(u8(40, d), u8(33, d)) == p, d
        assert N.expected_path(u8(40, d).astype(np.float32), u8(33, d).astype(np.float32)) == p, d
        assert N.expected_path(real(40, d), real(33, d)) == ("scan" if d == 300 else "split"), d
    assert N.expected_path(u8(40, 256, 128), u8(33, 256, 128)) == "integer"
    assert N.expected_path(u8(40, 61), u8(33, 61), binary=True) == "hamming"
    a = u8(40, 128).astype(np.float32); b = u8(33, 128).astype(np.float32)
    b2 = b.copy(); b2[3, 7] += 0.5
    assert N.expected_path(a, b2) == "split"                              # one non-integer value in the query view only
    a2 = a.copy(); a2[1, 1] = 257.0
    assert N.expected_path(a2, b) == "f32"
    assert N.expected_path(np.zeros((5, 128), np.float32), real(4, 128)) == "f32"       # an all-zero view: no split scale
