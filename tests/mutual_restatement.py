"""Mutual nearest-neighbour matching (r3dm_set_mutual_matching, include/r3dm.h) restated from the oracle alone, independent of the
library: the forward 2-NN table of a pair, the reverse nearest row of J for every row of I (pyoracle.knn2 with the views swapped: its tie
rule is the lowest index), the first distance of every query whose nominee does not point back set to +inf, then pyoracle.ratio_dedup
on the masked table -- +inf fails `a < R b`, so the match is gone before the (i, j) ordering and both de-duplications, and the oracle
itself stays as it is.  For the approximate arms the forward table is the arm's own CPU model (KGraphIndex.knn2 / HnswIndex.knn2 /
MrptIndex.knn2), masked the same way: the reverse direction is always the exhaustive one."""
import numpy as np


def reverse_nearest(O, dI, dJ, binary=False):
    """for every row of I the nearest row of J under (distance, row index) -> int64 [nI]"""
    dI = np.ascontiguousarray(dI); dJ = np.ascontiguousarray(dJ)
    if len(dJ) >= 2:
        return O.knn2(dJ, dI, binary=binary)[0][:, 0].astype(np.int64)
    # a view J of one row: pyoracle.knn2 refuses a dataset of fewer than two rows; every row of I has that row as its nearest
    if binary:
        d = np.array([[O.hamming(a, b) for b in dJ] for a in dI], np.int64).reshape(len(dI), len(dJ))
    else:
        d = np.array([[O.l2sq(a, b) for b in dJ] for a in dI], np.float64).reshape(len(dI), len(dJ))
    return np.argmin(d, axis=1).astype(np.int64)               # (numpy's argmin: first minimum = lowest index)


def mask_forward(idx, dist, rev):
    """the forward table with the first distance of every query whose nominee does not point back set to +inf (float32 distances)"""
    idx = np.asarray(idx); dist = np.array(dist, np.float32)
    for j in range(len(idx)):
        i = int(idx[j, 0])
        if i < 0 or rev[i] != j:
            dist[j, 0] = np.inf
    return dist


def match_table(O, idx, dist, dI, dJ, xyI, xyJ, ratio, squared, binary=False, mutual=True):
    """a forward 2-NN table -> the pair's matches [m, 2] (i_, j_)"""
    dist = np.asarray(dist).astype(np.float32)                 # Hamming distances: the ratio test runs on floats (matching.c)
    if mutual:
        dist = mask_forward(idx, dist, reverse_nearest(O, dI, dJ, binary))
    return O.ratio_dedup(idx, dist, xyI, xyJ, ratio, squared)


def match_pair(O, dI, dJ, xyI, xyJ, ratio, squared=True, binary=False, mutual=True):
    """the exhaustive matcher on one pair; a dataset of fewer than two rows has no second neighbour: no match"""
    if len(dI) < 2 or len(dJ) < 1:
        return np.zeros((0, 2), np.uint32)
    idx, dist = O.knn2(dI, dJ, binary=binary)
    return match_table(O, idx, dist, dI, dJ, xyI, xyJ, ratio, squared, binary, mutual)


def _collect(pairs, per_pair):
    counts = np.zeros(len(pairs), np.uint32); out = []
    for k, (I, J) in enumerate(pairs):
        m = per_pair(int(I), int(J))
        counts[k] = len(m); out.append(np.asarray(m, np.uint32).reshape(-1, 2))
    return counts, (np.concatenate(out) if out else np.zeros((0, 2), np.uint32))


def match_collection(O, descs, xys, pairs, ratio, squared=True, binary=False, mutual=True):
    """-> (counts [P], matches [M, 2]) in the convention of pyoracle.match_collection"""
    return _collect(pairs, lambda I, J: match_pair(O, descs[I], descs[J], None if xys is None else xys[I], None if xys is None else xys[J],
                                                   ratio, squared, binary, mutual))


def match_collection_kgraph(O, descs, xys, pairs, ratio, K, P, S, seed, min_rows=128, cap=64, mutual=True):
    """the graph matcher's CPU model (pyoracle.match_collection_kgraph, builder "exact") with the mutual rule"""
    descs = [np.ascontiguousarray(d, np.float32) for d in descs]
    index = {}

    def one(I, J):
        dI, dJ = descs[I], descs[J]
        if len(dI) < 2 or len(dJ) < 1:
            return np.zeros((0, 2), np.uint32)
        if I not in index:
            index[I] = O.kgraph_build_exact(dI, K, cap)
        idx, dist, _ = index[I].knn2(dJ, P, S, seed, I, J, min_rows)
        return match_table(O, idx, dist, dI, dJ, xys[I], xys[J], ratio, True, False, mutual)
    return _collect(pairs, one)


def match_collection_hnsw(O, descs, xys, pairs, ratio, preset="precise", min_rows=128, seed=100, mutual=True):
    """pyoracle.match_collection_hnsw (builder "batch") with the mutual rule"""
    descs = [np.ascontiguousarray(d, np.float32) for d in descs]
    M, _, ef = O.HNSW_PRESETS[preset]
    index = {}

    def one(I, J):
        dI, dJ = descs[I], descs[J]
        if len(dI) < 2 or len(dJ) < 1:
            return np.zeros((0, 2), np.uint32)
        if len(dI) < min_rows:
            idx, dist = O.knn2(dI, dJ)
        else:
            if I not in index:
                index[I] = O.hnsw_build_batch(dI, M, seed)
            idx, dist = index[I].knn2(dJ, ef)
        return match_table(O, idx, dist, dI, dJ, xys[I], xys[J], ratio, True, False, mutual)
    return _collect(pairs, one)


def match_collection_mrpt(O, descs, xys, pairs, ratio, n_trees=26, depth=6, votes=5, density=None, seed=0, min_rows=128, mutual=True):
    """pyoracle.match_collection_mrpt with the mutual rule: the arm's ratio runs on square roots, the check on squared distances --
    which row of J is nearest to a row of I does not depend on the root"""
    descs = [np.ascontiguousarray(d, np.float32) for d in descs]
    index = {}

    def one(I, J):
        dI, dJ = descs[I], descs[J]
        if len(dI) == 0 or len(dJ) == 0:
            return np.zeros((0, 2), np.uint32)
        if len(dI) < min_rows:
            return match_pair(O, dI, dJ, xys[I], xys[J], ratio, True, False, mutual)
        if I not in index:
            dens = density if density and density > 0 else float(np.float32(1.0 / np.sqrt(np.float64(dI.shape[1]))))
            index[I] = O.mrpt_build(dI, n_trees, depth, dens, seed)
        idx, dist, _ = index[I].knn2(dJ, votes)
        idx = idx.copy(); dist = dist.copy()
        dropped = idx[:, 0] < 0
        idx[dropped] = 0; dist[dropped] = (1.0, 0.0)              # (pyoracle.match_collection_mrpt: a dropped query matches nothing)
        if mutual:
            rev = reverse_nearest(O, dI, dJ)
            keep_inf = np.array([dropped[j] or rev[int(idx[j, 0])] != j for j in range(len(idx))])
            dist[keep_inf & ~dropped, 0] = np.inf
        return O.ratio_dedup(idx, dist, xys[I], xys[J], ratio, False)
    return _collect(pairs, one)


# ---------------------------------------------------------------------------------------------------- the brute-force loop
def brute_force_pair(dI, dJ, xyI, xyJ, ratio, squared=True, binary=False, mutual=True):
    """the rule of include/r3dm.h spelled out with numpy loops on integer-valued rows (every distance exact in float64): forward
    2-NN with ties to the lowest row, ratio test in float32, the mutual rule, (i, j) order, coordinate de-duplication"""
    dI = np.asarray(dI); dJ = np.asarray(dJ)
    if len(dI) < 2:
        return np.zeros((0, 2), np.uint32)

    def dist(a, b):
        if binary:
            return float(np.unpackbits(np.bitwise_xor(a, b)).sum())
        e = a.astype(np.float64) - b.astype(np.float64)
        return float((e * e).sum())
    D = np.array([[dist(a, b) for b in dJ] for a in dI])                        # [nI, nJ]
    R = np.float32(ratio) * np.float32(ratio) if squared else np.float32(ratio)
    kept = []
    for j in range(len(dJ)):
        order = sorted(range(len(dI)), key=lambda i: (D[i, j], i))
        i0, i1 = order[0], order[1]
        if not (np.float32(D[i0, j]) < R * np.float32(D[i1, j])):
            continue
        if mutual and any((D[i0, k], k) < (D[i0, j], j) for k in range(len(dJ))):
            continue
        kept.append((i0, j))
    kept.sort()
    out, seen = [], set()
    for i, j in kept:
        key = None if xyI is None or xyJ is None else (float(xyI[i][0]), float(xyI[i][1]), float(xyJ[j][0]), float(xyJ[j][1]))
        if key is not None and key in seen:
            continue
        seen.add(key) if key is not None else None
        out.append((i, j))
    return np.array(out, np.uint32).reshape(-1, 2)


# ---------------------------------------------------------------------------------------------------- inputs the tests share
def second_observations(n, dim, seed, dtype=np.float32, nbytes=None):
    """integer SIFT-like rows (0 .. 120): view J is view I lightly perturbed, and every third row of J is a SECOND observation of the
    row of I its left neighbour observes -- the many-to-one case of the issue.  -> (dI, dJ, xyI, xyJ), positions distinct"""
    rng = np.random.default_rng(seed)
    if nbytes is not None:
        dI = rng.integers(0, 256, (n, nbytes), dtype=np.uint8)
        flip = lambda r, p: r ^ np.packbits(rng.random((len(r), nbytes * 8)) < p, axis=1)
        dJ = flip(dI, 0.02)
        for j in range(2, n, 3):
            dJ[j] = flip(dI[j - 1:j], 0.04)[0]
    else:
        dI = rng.integers(0, 121, (n, dim)).astype(np.float32)
        dJ = dI + rng.integers(-2, 3, (n, dim)).astype(np.float32)
        for j in range(2, n, 3):
            dJ[j] = dI[j - 1] + rng.integers(-3, 4, dim).astype(np.float32)
        dJ = np.clip(dJ, 0, 255)
        dI = dI.astype(dtype); dJ = dJ.astype(dtype)
    xyI = np.stack([np.arange(n) * 3.0 + 1.0, np.arange(n) * 2.0 + 5.0], 1).astype(np.float32)
    xyJ = np.stack([np.arange(n) * 3.0 + 2.0, np.arange(n) * 2.0 + 7.0], 1).astype(np.float32)
    return dI, dJ, xyI, xyJ


def engineered_views(dim=64, dtype=np.float32):
    """integer-valued rows, every distance exact.  View I: rows 0 .. 5; view J: rows built against them.
      * J0, J1 at squared distances 1 and 4 from I0: both nominate I0, only J0 is mutual
      * J2, J3 identical, nearest to I1: the lower index survives
      * J4, J5 at ONE position, both nearest to I2 at distances 4 and 1: the earlier (J4) fails the check, the later must survive the
        coordinate de-duplication that would have dropped it behind J4
      * J6 nearest to I3 alone: an ordinary mutual match
    -> (dI, dJ, xyI, xyJ)"""
    w = dim // 8                                                  # (dim >= 32: six blocks of w dimensions, the last four stay free)
    base = np.zeros((6, dim), np.float32)
    for k in range(6):
        base[k, k * w:(k + 1) * w] = 100.0                        # far apart: 2 w 100^2 between any two rows
    dJ = np.stack([base[0], base[0], base[1], base[1], base[2], base[2], base[3]]).copy()
    dJ[0, dim - 4] = 1.0                                          # d(I0, J0) = 1
    dJ[1, dim - 4] = 2.0                                          # d(I0, J1) = 4
    dJ[2, dim - 3] = 3.0; dJ[3, dim - 3] = 3.0                    # identical rows, d = 9
    dJ[4, dim - 2] = 2.0                                          # d(I2, J4) = 4
    dJ[5, dim - 2] = 1.0                                          # d(I2, J5) = 1
    dJ[6, dim - 1] = 5.0
    xyI = np.array([[10, 10], [20, 20], [30, 30], [40, 40], [50, 50], [60, 60]], np.float32)
    xyJ = np.array([[11, 11], [12, 12], [21, 21], [22, 22], [31, 31], [31, 31], [41, 41]], np.float32)
    return base.astype(dtype), dJ.astype(dtype), xyI, xyJ
