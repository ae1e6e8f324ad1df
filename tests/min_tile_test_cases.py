"""Views for tests/test_gpu_min_tile_test.py (the min form of l2_knn2_half_kernel's tile tests: the minimum of a lane's 16 keys, one
v_min3_f32 tree per query tile, answers what 16 compares answered) and for the CPU test of the rule that admits a batch to it
(tests/test_min_tile_test_rule.py).  Built on the planted rows of half_filter_cases.py and level2_skip_cases.py.

A lane holds the keys of the 16 rows of its half of a tile, (position >> 2) & 1, in register 4 (position >> 3) + (position & 3); the
two query tiles of a wave hold queries 0 .. 31 and 32 .. 63.  `moved` puts a planted row at any position of its tile and its query
in either query tile WITHOUT changing a threshold: positions trade places inside a lane half only (a half's list depends on the set of
its rows), the two halves trade places wholesale in every tile, and two queries of one wave trade places."""
import numpy as np

import pairnorm_filter_cases as FC

NORM_BOUND = np.float32(2.0 ** 28)          # kMinTileTestNormBits (r3dm_internal.hpp): the min form serves views whose max |row|^2 lies below


def stored_norms(x):
    """|row|^2 as staging stores it: the fma chain over the dimensions in float32 (exact here where the views are small integers or
    hold one or two non-zero members; anywhere else within 128 x 2^-24 of it, which no case of these tests comes near the bound by)"""
    n = np.zeros(x.shape[0], np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(x.shape[1]):
            n = (x[:, k].astype(np.float64) * x[:, k].astype(np.float64) + n.astype(np.float64)).astype(np.float32)
    return n


def rule_holds(*views):
    """every view's max |row|^2 below 2^28, compared on the bits as unsigned integers the way ImgDev::max_norm_bits is kept (a NaN
    norm lies above every finite one)"""
    return all(int(stored_norms(v).view(np.uint32).max(initial=0)) < int(NORM_BOUND.view(np.uint32)) for v in views)


def moved(a, b, q, row, p, nj):
    """(a, b) with the row planted at `row` (its tile's lane half 0) now at position p of the same tile, and its query q (< 32) now in
    query tile nj of its wave.  -> (a, b, q, row) as moved"""
    a, b = a.copy(), b.copy()
    t, p0 = divmod(row, 32)
    assert (p0 >> 2) & 1 == 0 and q < 32 and a.shape[0] >= 32 * (t + 1)
    if (p >> 2) & 1:                                     # the halves trade places in every whole tile (a partial one holds far rows only)
        for lo in range(0, a.shape[0] - 31, 32):
            a[lo:lo + 32] = a[lo + (np.arange(32) ^ 4)]
        p0 ^= 4
    lo = 32 * t
    a[[lo + p0, lo + p]] = a[[lo + p, lo + p0]]
    if nj:
        b[[q, q + 32]] = b[[q + 32, q]]
        q += 32
    return a, b, q, lo + p


def edge_views(norm, where="dataset", nI=97, nJ=130, seed=47):
    """sparse views with one row of a far tile (dataset row 50, or query 100) replaced by a row whose energy lies in ONE dimension pair
    -- the largest pair norm a row of that size can hold -- and whose stored |row|^2 is exactly `norm`:
    2^28 - 16 (the largest float below the bound) = fl((2^14 - 2^-10)^2) + 4^2, 2^28 = (2^14)^2, 2^29 = (2^14)^2 + (2^14)^2"""
    a, b = FC.sparse_views(nI, nJ, seed)
    r = np.zeros(FC.DIM, np.float32)
    if norm == 2.0 ** 28 - 16:
        r[0], r[1] = np.nextafter(np.float32(2.0 ** 14), np.float32(0)), 4.0
    elif norm == 2.0 ** 28:
        r[0] = 2.0 ** 14
    elif norm == 2.0 ** 29:
        r[0] = r[1] = 2.0 ** 14
    else:
        raise ValueError(norm)
    if where == "dataset":
        a[50] = r
    else:
        b[100] = r
    assert float(stored_norms(r[None])[0]) == norm
    return a, b
