"""The symmetric ratio test (r3dm_set_symmetric_ratio, include/r3dm.h) restated from the oracle alone, independent of the library: the
forward 2-NN table of a pair (pyoracle.knn2, or an approximate arm's CPU model), the REVERSE 2-NN table (pyoracle.knn2 with the views
swapped: for every row i of I its nearest row of J and the two distances d1 <= d2, ties to the lowest row), the first distance of a
query set to +inf when its nominee does not point back or when the reverse pair (d1, d2) fails the arm's ratio form, then
pyoracle.ratio_dedup on the masked table -- +inf fails `a < R b`, so the match is gone before the (i, j) ordering and both
de-duplications, and the oracle itself stays as it is.  When the nominee points back, the second entry of the reverse table IS the
smallest distance to any other row of J.  A view J of fewer than two rows has no reverse table: nothing survives.

The ratio forms (the forward test of the arm, repeated in reverse, float32 throughout):
    "squared"  d1 < (ratio * ratio) * d2          squared L2 distances: the exhaustive matcher with squared_metric, KGraph, HNSW, and
                                                  the pairs an approximate arm scans exhaustively
    "plain"    d1 < ratio * d2                    Hamming distances converted to float
    "sqrt"     sqrt(d1) < ratio * sqrt(d2)        the pairs the MRPT arm answers through its index

Every entry returns the three counters beside the matches: candidates the check looks at (accepted by the forward test), dropped
because not nearest (what the mutual rule alone removes), dropped by the reverse ratio only."""
import numpy as np

import mutual_restatement as M

MODES = ("off", "mutual", "symmetric")


def ratio_form(squared, on_roots=False):
    return "sqrt" if on_roots else ("squared" if squared else "plain")


def reverse_ratio_passes(d1, d2, ratio, form):
    """f(d1) < R * f(d2) in float32: one multiply, a strict <"""
    r = np.float32(ratio); d1 = np.float32(d1); d2 = np.float32(d2)
    if form == "squared":
        return bool(d1 < np.float32(r * r) * d2)
    if form == "plain":
        return bool(d1 < r * d2)
    if form == "sqrt":
        return bool(np.sqrt(d1) < r * np.sqrt(d2))
    raise ValueError(form)


def reverse_table(O, dI, dJ, binary=False):
    """for every row of I: (nearest row of J, d1, d2) -> (int64 [nI], float32 [nI], float32 [nI]); None when J has fewer than two rows.
    The distances are the oracle's: squared L2, or Hamming converted to float as the ratio test converts it"""
    dI = np.ascontiguousarray(dI); dJ = np.ascontiguousarray(dJ)
    if len(dJ) < 2:
        return None
    idx, dist = O.knn2(dJ, dI, binary=binary)
    dist = np.asarray(dist).astype(np.float32)
    return idx[:, 0].astype(np.int64), dist[:, 0], dist[:, 1]


def masked_tables(O, idx, dist, dI, dJ, ratio, form, binary=False):
    """the forward table's float32 distances after part 1 alone and after the whole rule -> (dist_nearest, dist_symmetric)"""
    idx = np.asarray(idx); dist = np.asarray(dist).astype(np.float32)
    rev = reverse_table(O, dI, dJ, binary)
    if rev is None:                                               # fewer than two rows of J: mutual by definition, no second neighbour
        near = M.mask_forward(idx, dist, M.reverse_nearest(O, dI, dJ, binary))
        sym = dist.copy(); sym[:, 0] = np.inf
        return near, sym
    rows, d1, d2 = rev
    near = M.mask_forward(idx, dist, rows)
    sym = near.copy()
    for j in range(len(idx)):
        i = int(idx[j, 0])
        if i >= 0 and rows[i] == j and not reverse_ratio_passes(d1[i], d2[i], ratio, form):
            sym[j, 0] = np.inf
    return near, sym


def match_table(O, idx, dist, dI, dJ, xyI, xyJ, ratio, squared, binary=False, mode="symmetric", on_roots=False):
    """a forward 2-NN table -> (the pair's matches [m, 2] (i_, j_), (checked, dropped_not_nearest, dropped_ratio)); `squared` is the
    forward test's flag (pyoracle.ratio_dedup), on_roots: the table holds square roots (MRPT) and the reverse test runs on roots"""
    dist = np.asarray(dist).astype(np.float32)
    if mode == "off":
        return O.ratio_dedup(idx, dist, xyI, xyJ, ratio, squared), (0, 0, 0)
    near, sym = masked_tables(O, idx, dist, dI, dJ, ratio, ratio_form(squared, on_roots), binary)
    n0 = len(O.ratio_dedup(idx, dist, None, None, ratio, squared))           # without positions: the accepted queries, nothing de-duplicated
    n1 = len(O.ratio_dedup(idx, near, None, None, ratio, squared))
    n2 = len(O.ratio_dedup(idx, sym, None, None, ratio, squared))
    if mode == "mutual":
        return O.ratio_dedup(idx, near, xyI, xyJ, ratio, squared), (n0, n0 - n1, 0)
    return O.ratio_dedup(idx, sym, xyI, xyJ, ratio, squared), (n0, n0 - n1, n1 - n2)


_EMPTY = (np.zeros((0, 2), np.uint32), (0, 0, 0))


def match_pair(O, dI, dJ, xyI, xyJ, ratio, squared=True, binary=False, mode="symmetric"):
    """the exhaustive matcher on one pair; a dataset of fewer than two rows has no second neighbour: no match"""
    if len(dI) < 2 or len(dJ) < 1:
        return _EMPTY
    idx, dist = O.knn2(dI, dJ, binary=binary)
    return match_table(O, idx, dist, dI, dJ, xyI, xyJ, ratio, squared, binary, mode)


def _collect(pairs, per_pair):
    counts = np.zeros(len(pairs), np.uint32); out = []; counters = np.zeros(3, np.int64)
    for k, (I, J) in enumerate(pairs):
        m, c = per_pair(int(I), int(J))
        counts[k] = len(m); out.append(np.asarray(m, np.uint32).reshape(-1, 2)); counters += np.array(c, np.int64)
    return counts, (np.concatenate(out) if out else np.zeros((0, 2), np.uint32)), tuple(int(x) for x in counters)


def _xy(xys, v):
    return None if xys is None else xys[v]


def match_collection(O, descs, xys, pairs, ratio, squared=True, binary=False, mode="symmetric"):
    """-> (counts [P], matches [M, 2], (checked, dropped_not_nearest, dropped_ratio))"""
    return _collect(pairs, lambda I, J: match_pair(O, descs[I], descs[J], _xy(xys, I), _xy(xys, J), ratio, squared, binary, mode))


def match_collection_kgraph(O, descs, xys, pairs, ratio, K, P, S, seed, min_rows=128, cap=64, mode="symmetric"):
    """the graph matcher's CPU model (forward table as mutual_restatement.match_collection_kgraph builds it) under the rule"""
    descs = [np.ascontiguousarray(d, np.float32) for d in descs]
    index = {}

    def one(I, J):
        dI, dJ = descs[I], descs[J]
        if len(dI) < 2 or len(dJ) < 1:
            return _EMPTY
        if I not in index:
            index[I] = O.kgraph_build_exact(dI, K, cap)
        idx, dist, _ = index[I].knn2(dJ, P, S, seed, I, J, min_rows)
        return match_table(O, idx, dist, dI, dJ, _xy(xys, I), _xy(xys, J), ratio, True, False, mode)
    return _collect(pairs, one)


def match_collection_hnsw(O, descs, xys, pairs, ratio, preset="precise", min_rows=128, seed=100, mode="symmetric"):
    descs = [np.ascontiguousarray(d, np.float32) for d in descs]
    Mh, _, ef = O.HNSW_PRESETS[preset]
    index = {}

    def one(I, J):
        dI, dJ = descs[I], descs[J]
        if len(dI) < 2 or len(dJ) < 1:
            return _EMPTY
        if len(dI) < min_rows:
            idx, dist = O.knn2(dI, dJ)
        else:
            if I not in index:
                index[I] = O.hnsw_build_batch(dI, Mh, seed)
            idx, dist = index[I].knn2(dJ, ef)
        return match_table(O, idx, dist, dI, dJ, _xy(xys, I), _xy(xys, J), ratio, True, False, mode)
    return _collect(pairs, one)


def match_collection_mrpt(O, descs, xys, pairs, ratio, n_trees=26, depth=6, votes=5, density=None, seed=0, min_rows=128, mode="symmetric",
                          reverse_on_roots=True):
    """the MRPT arm: views below min_rows are scanned with the squared ratio (form "squared"); the others answer through their forest,
    whose table holds float32 square roots and whose ratio runs on them un-squared -- so does the reverse test (form "sqrt": the
    float32 roots of the reverse table's squared distances).  reverse_on_roots=False is the WRONG form (the squared one) for the
    indexed pairs: the tests use it to show that their witness tells the two apart"""
    descs = [np.ascontiguousarray(d, np.float32) for d in descs]
    index = {}

    def one(I, J):
        dI, dJ = descs[I], descs[J]
        if len(dI) == 0 or len(dJ) == 0:
            return _EMPTY
        if len(dI) < min_rows:
            return match_pair(O, dI, dJ, _xy(xys, I), _xy(xys, J), ratio, True, False, mode)
        if I not in index:
            dens = density if density and density > 0 else float(np.float32(1.0 / np.sqrt(np.float64(dI.shape[1]))))
            index[I] = O.mrpt_build(dI, n_trees, depth, dens, seed)
        idx, dist, _ = index[I].knn2(dJ, votes)
        idx = idx.copy(); dist = dist.copy()
        dropped = idx[:, 0] < 0
        idx[dropped] = 0; dist[dropped] = (1.0, 0.0)              # (pyoracle.match_collection_mrpt: a dropped query matches nothing)
        if mode == "off":
            return O.ratio_dedup(idx, dist, _xy(xys, I), _xy(xys, J), ratio, False), (0, 0, 0)
        near, sym = masked_tables(O, idx, dist, dI, dJ, ratio, "sqrt" if reverse_on_roots else "squared")
        n = [len(O.ratio_dedup(idx, t, None, None, ratio, False)) for t in (dist, near, sym)]
        if mode == "mutual":
            return O.ratio_dedup(idx, near, _xy(xys, I), _xy(xys, J), ratio, False), (n[0], n[0] - n[1], 0)
        return O.ratio_dedup(idx, sym, _xy(xys, I), _xy(xys, J), ratio, False), (n[0], n[0] - n[1], n[1] - n[2])
    return _collect(pairs, one)


# ---------------------------------------------------------------------------------------------------- the brute-force loop
ITEMS_THREADS = 256          # l2_mutual_items_kernel<true>: thread t scans rows t, t + 256, ...


def brute_force_pair(dI, dJ, xyI, xyJ, ratio, squared=True, binary=False, mode="symmetric", bug=None):
    """the rule of include/r3dm.h spelled out with numpy loops on integer-valued rows (every distance exact in float64): forward 2-NN
    with ties to the lowest row, ratio test in float32, nearest, reverse ratio, (i, j) order, coordinate de-duplication.
    -> (matches, (checked, dropped_not_nearest, dropped_ratio)).
    bug: one of three wrong implementations -- "le": <= in the reverse test; "bests_only": the second minimum taken from the bests of
    ITEMS_THREADS interleaved shares of the rows, not from their 2-lists; "d2_self": d2 may be row j itself"""
    dI = np.asarray(dI); dJ = np.asarray(dJ)
    if len(dI) < 2:
        return _EMPTY

    def dist(a, b):
        if binary:
            return float(np.unpackbits(np.bitwise_xor(a, b)).sum())
        e = a.astype(np.float64) - b.astype(np.float64)
        return float((e * e).sum())
    D = np.array([[dist(a, b) for b in dJ] for a in dI])                        # [nI, nJ]
    R = np.float32(ratio) * np.float32(ratio) if squared else np.float32(ratio)
    nJ = len(dJ)
    kept = []; checked = not_nearest = by_ratio = 0
    for j in range(nJ):
        order = sorted(range(len(dI)), key=lambda i: (D[i, j], i))
        i0, i1 = order[0], order[1]
        if not (np.float32(D[i0, j]) < R * np.float32(D[i1, j])):
            continue
        if mode != "off":
            checked += 1
            if any((D[i0, k], k) < (D[i0, j], j) for k in range(nJ)):
                not_nearest += 1
                continue
        if mode == "symmetric":
            if nJ < 2:
                by_ratio += 1
                continue
            if bug == "d2_self":
                d2 = min(D[i0, k] for k in range(nJ))
            elif bug == "bests_only":
                bests = [min(D[i0, k] for k in range(t, nJ, ITEMS_THREADS)) for t in range(min(ITEMS_THREADS, nJ))]
                bests.remove(D[i0, j])
                d2 = min(bests) if bests else np.inf
            else:
                d2 = min(D[i0, k] for k in range(nJ) if k != j)
            a, b = np.float32(D[i0, j]), R * np.float32(d2)
            if not ((a <= b) if bug == "le" else (a < b)):
                by_ratio += 1
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
    return np.array(out, np.uint32).reshape(-1, 2), (checked, not_nearest, by_ratio)


# ---------------------------------------------------------------------------------------------------- inputs the tests share
BOUNDARY_RATIO = 0.5         # R = 0.25 on squared L2 distances, 0.5 on Hamming distances: both exact
BOUNDARY_ROWS_J = 300        # two 256-row shares of the rows-based kernel, ten 32-row tiles
# what the rule does with the engineered rows of boundary_views, as (i, j)
BOUNDARY_KEPT = [(1, 40), (4, 50), (5, 60)]
BOUNDARY_NOT_NEAREST = [(0, 5), (1, 3), (2, 11), (3, 276), (4, 290)]
BOUNDARY_RATIO_ONLY = [(0, 2), (2, 10), (3, 20)]


def boundary_views(dim=64, dtype=np.float32, nbytes=None):
    """integer-valued rows, every distance exact.  View I: six rows far apart; view J: BOUNDARY_ROWS_J rows, every one a filler
    (equally far from all of I: its forward ratio test fails) except the ones built against a row of I, at the distances below
    (squared L2 | Hamming, `near / far`: 4 / 16 / 17 | 8 / 16 / 17) with BOUNDARY_RATIO:
      I0: J2 near, J5 at 16      near < R x 16 is FALSE (4 < 4, 8 < 8): J2 goes by the ratio alone; d2's row is above j, in j's tile
      I1: J40 near, J3 at 17     near < R x 17 holds: J40 stays; d2's row is below j, in another tile
      I2: J10 = J11 (1 | 3)      a duplicate of row j: d2 = d1, J10 goes by the ratio alone (J11 is not nearest)
      I3: J20 near, J276 at 16   rows j and j + 256: ONE thread's share in the rows-based kernel, another tile in the tiled one; J20 goes
      I4: J50 near, J290 at 17   d2's row is above j, in another tile; J50 stays
      I5: J60 alone (9)          d2 is a filler's distance: stays
    -> (dI, dJ, xyI, xyJ), positions distinct"""
    nJ = BOUNDARY_ROWS_J
    if nbytes is not None:
        bits = nbytes * 8; w = 32                                       # blocks of 32 bits; the free bits follow block 6
        bI = np.zeros((6, bits), np.uint8); bJ = np.zeros((nJ, bits), np.uint8)
        for k in range(6):
            bI[k, k * w:(k + 1) * w] = 1
        bJ[:, 6 * w:7 * w] = 1                                          # fillers: 64 bits from every row of I
        free = 7 * w

        def put(j, i, d):
            bJ[j] = bI[i]; bJ[j, free:free + d] = 1
        near, far16, far17, dup, alone = 8, 16, 17, 3, 9
        pack = lambda b: np.packbits(b, axis=1)
    else:
        w = dim // 8
        bI = np.zeros((6, dim), np.float32); bJ = np.zeros((nJ, dim), np.float32)
        for k in range(6):
            bI[k, k * w:(k + 1) * w] = 100.0
        bJ[:, 6 * w:7 * w] = 100.0                                      # fillers: 2 w 100^2 from every row of I

        def put(j, i, d):                                               # d = a^2 + b^2 on two of the last four dimensions
            bJ[j] = bI[i]; bJ[j, dim - 4] = {1: 1, 4: 2, 9: 3, 16: 4, 17: 4}[d]; bJ[j, dim - 3] = 1.0 if d == 17 else 0.0
        near, far16, far17, dup, alone = 4, 16, 17, 1, 9
        pack = lambda b: b.astype(dtype)
    put(2, 0, near); put(5, 0, far16)
    put(40, 1, near); put(3, 1, far17)
    put(10, 2, dup); put(11, 2, dup)
    put(20, 3, near); put(276, 3, far16)
    put(50, 4, near); put(290, 4, far17)
    put(60, 5, alone)
    xyI = np.stack([np.arange(6) * 10.0 + 10.0, np.arange(6) * 10.0 + 10.0], 1).astype(np.float32)
    xyJ = np.stack([np.arange(nJ) * 3.0 + 2.0, np.arange(nJ) * 2.0 + 7.0], 1).astype(np.float32)
    return pack(bI), pack(bJ), xyI, xyJ


def ambiguous_views(n, dim, seed, dtype=np.float32, nbytes=None):
    """mutual_restatement.second_observations with the second observation brought as close as the first: every third row of J observes
    the row of I its left neighbour observes at about the same distance, so from I's side the nearer of the two is ambiguous -- with
    ratios around 0.8 a good part of the matches that pass the mutual rule fall to the reverse ratio, the rows without a second
    observer stay, the farther observers are not nearest.  -> (dI, dJ, xyI, xyJ)"""
    dI, dJ, xyI, xyJ = M.second_observations(n, dim, seed, dtype, nbytes)
    rng = np.random.default_rng(seed + 7919)
    if nbytes is not None:
        for j in range(2, n, 3):
            dJ[j] = dI[j - 1] ^ np.packbits(rng.random(nbytes * 8) < 0.02)
    else:
        for j in range(2, n, 3):
            dJ[j] = np.clip(dI[j - 1].astype(np.float32) + rng.integers(-2, 3, dim).astype(np.float32), 0, 255).astype(dtype)
    return dI, dJ, xyI, xyJ


# the MRPT witness: integer squared distances (d1, d2) and a ratio on which sqrt(d1) < r sqrt(d2) and d1 < (r r) d2 DISAGREE in float32
SQRT_WITNESS_RATIO = 0.8


def sqrt_form_witness(ratio=SQRT_WITNESS_RATIO, limit=128):
    """the smallest pair of squared distances (d2 first) whose fate differs between the two forms of the reverse test -> (d1, d2)"""
    for d2 in range(2, limit + 1):
        for d1 in range(1, d2):
            if reverse_ratio_passes(d1, d2, ratio, "sqrt") != reverse_ratio_passes(d1, d2, ratio, "squared"):
                return d1, d2
    raise AssertionError("no witness")


WITNESS_ROW = 40


def plant_sqrt_witness(dI, dJ, row=WITNESS_ROW):
    """J[row] and J[row + 1] become row `row` of I moved by one on d1 and on d2 dimensions (squared distances d1 < d2, every other row
    of J far farther): (row, row) is nearest from both sides and its reverse pair is the witness's.  I[row + 3] becomes row `row`
    moved by two on every dimension: a second row for the MRPT forest to elect beside row `row` -- at these sizes its leaves hold two
    or three rows and a query that elects fewer than two rows is dropped -- far enough for the forward test.  In place; -> (d1, d2)"""
    d1, d2 = sqrt_form_witness()
    step = np.where(dI[row] < 128, 1, -1).astype(dI.dtype)
    dJ[row] = dI[row]; dJ[row, :d1] += step[:d1]
    dJ[row + 1] = dI[row]; dJ[row + 1, :d2] += step[:d2]
    dI[row + 3] = dI[row] + 2 * step
    return d1, d2


# ---------------------------------------------------------------------------------------------------- the case tables
ROWS = (1, 2, 3, 31, 32, 33, 257)
RAGGED_RATIO = 0.8


def ragged_views(dim, dtype, seed, nbytes=None):
    """views of ROWS rows cut from two related 257-row views (ambiguous second observations, two identical rows)"""
    dI, dJ, xyI, xyJ = ambiguous_views(257, dim, seed, dtype, nbytes)
    dJ[20] = dJ[10]
    descs, xys = [], []
    for k, n in enumerate(ROWS):
        src, xy = (dI, xyI) if k % 2 == 0 else (dJ, xyJ)
        descs.append(np.ascontiguousarray(src[:n])); xys.append(np.ascontiguousarray(xy[:n]))
    return descs, xys


def all_ordered_pairs(n):
    return np.array([(i, j) for i in range(n) for j in range(n) if i != j], np.uint32)


def arm_views(n, witness=False):
    """three related views for the approximate arms; witness: the MRPT pair (0, 1) carries the sqrt-form witness at WITNESS_ROW"""
    dI, dJ, xyI, xyJ = ambiguous_views(n, 128, 70 + n)
    if witness:
        plant_sqrt_witness(dI, dJ)
    return [dI, dJ, np.ascontiguousarray(dJ[::-1])], [xyI, xyJ, np.ascontiguousarray(xyJ[::-1] + 0.25)]


ARM_RATIO = 0.8
ARM_PAIRS = np.array([[0, 1], [0, 2], [1, 2]], np.uint32)
