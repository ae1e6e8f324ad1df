"""Preemptive matching (r3dm_set_preemptive_matching, include/r3dm.h) restated from the oracle alone, independent of the library: the
head of a view (numpy's stable argsort on the negated priority IS the order priority descending, row ascending), the count of a pair
(pyoracle.match_distance_ratio on the two heads, no positions: nothing is de-duplicated), the gate of a collection.  Below it a
brute-force loop that shares no code with the first set: python's sorted on (-p, row), float64 distances on integer-valued rows."""
import numpy as np


def _clean(priority):
    return None if priority is None else np.asarray(priority, np.float32) + np.float32(0.0)      # -0.0 is stored as +0.0


def head_rows(priority, n, h):
    """rows of the head of a view of n rows for head size h, ascending -> int64 [min(h, n)]"""
    hn = min(h, n)
    if priority is None:
        return np.arange(hn, dtype=np.int64)
    p = _clean(priority)
    assert len(p) == n
    order = np.argsort(-p.astype(np.float64), kind="stable")            # ties keep ascending row index
    return np.sort(order[:hn]).astype(np.int64)


def pair_count(O, dI, dJ, pI, pJ, h, ratio, squared=True, binary=False):
    """accepted queries when the head of J is 2-NN-matched against the head of I"""
    hI = np.ascontiguousarray(np.asarray(dI)[head_rows(pI, len(dI), h)])
    hJ = np.ascontiguousarray(np.asarray(dJ)[head_rows(pJ, len(dJ), h)])
    if len(hI) < 2 or len(hJ) < 1:
        return 0
    return len(O.match_distance_ratio(hI, hJ, ratio, squared, None, None, binary))


def collection_counts(O, descs, prios, pairs, h, ratio, squared=True, binary=False):
    return np.array([pair_count(O, descs[int(I)], descs[int(J)], prios[int(I)], prios[int(J)], h, ratio, squared, binary) for I, J in pairs],
                    np.uint32).reshape(len(pairs))


def gate_collection(O, descs, prios, pairs, h, t, ratio, squared=True, binary=False):
    """-> (counts [P], keep [P] bool): the pairs a gated entry matches are pairs[keep]"""
    counts = collection_counts(O, descs, prios, pairs, h, ratio, squared, binary)
    return counts, counts >= t


def restrict_graph(pairs, offsets, matches, kept_pairs):
    """a graph (CSR arrays) restricted to the pairs listed in kept_pairs -> (pairs, per-pair counts, matches)"""
    kept = {(int(a), int(b)) for a, b in kept_pairs}
    offsets = np.asarray(offsets).astype(np.int64)
    sel = [k for k, (a, b) in enumerate(pairs) if (int(a), int(b)) in kept]
    out = [matches[offsets[k]:offsets[k + 1]] for k in sel]
    return (np.asarray(pairs)[sel].reshape(-1, 2), np.array([len(m) for m in out], np.int64),
            np.concatenate(out).reshape(-1, 2) if out else np.zeros((0, 2), np.uint32))


# ---------------------------------------------------------------------------------------------------- the brute-force loop
def brute_force_head(priority, n, h):
    if priority is None:
        return list(range(min(h, n)))
    p = [0.0 if float(x) == 0.0 else float(x) for x in priority]
    return sorted(sorted(range(n), key=lambda r: (-p[r], r))[:h])


def brute_force_count(dI, dJ, pI, pJ, h, ratio, squared=True, binary=False):
    """the rule of include/r3dm.h spelled out on integer-valued rows (every distance exact in float64): head by sorted(), 2-NN with
    ties to the lowest row, the ratio test in float32"""
    rI, rJ = brute_force_head(pI, len(dI), h), brute_force_head(pJ, len(dJ), h)
    if len(rI) < 2:
        return 0

    def dist(a, b):
        if binary:
            return float(np.unpackbits(np.bitwise_xor(a, b)).sum())
        e = a.astype(np.float64) - b.astype(np.float64)
        return float((e * e).sum())
    R = np.float32(ratio) * np.float32(ratio) if squared else np.float32(ratio)
    count = 0
    for j in rJ:
        d = sorted((dist(dI[i], dJ[j]), i) for i in rI)
        if np.float32(d[0][0]) < R * np.float32(d[1][0]):
            count += 1
    return count


# ---------------------------------------------------------------------------------------------------- inputs the tests share
def related_views(rows, dim, seed, dtype=np.float32, nbytes=None, n_unrelated=1):
    """ragged views cut from two related views of max(rows) rows (view J is view I lightly perturbed: integer SIFT-like rows 0 .. 120,
    or bit rows), alternately; the last n_unrelated views are replaced by noise.  Every view gets a priority with MANY ties (eight
    distinct values), so that the h-th and the (h + 1)-th row of a head are often equal.  -> (descs, prios)"""
    rng = np.random.default_rng(seed)
    n = max(rows)
    if nbytes is not None:
        dI = rng.integers(0, 256, (n, nbytes), dtype=np.uint8)
        dJ = dI ^ np.packbits(rng.random((n, nbytes * 8)) < 0.02, axis=1)
        noise = lambda m: rng.integers(0, 256, (m, nbytes), dtype=np.uint8)
    else:
        dI = rng.integers(0, 121, (n, dim)).astype(np.float32)
        dJ = np.clip(dI + rng.integers(-2, 3, (n, dim)).astype(np.float32), 0, 255)
        dI = dI.astype(dtype); dJ = dJ.astype(dtype)
        noise = lambda m: rng.integers(0, 121, (m, dim)).astype(dtype)
    shared = rng.integers(0, 8, n).astype(np.float32) * np.float32(0.75)       # one scale per scene point, carried to both observations
    descs, prios = [], []
    for k, m in enumerate(rows):
        unrelated = k >= len(rows) - n_unrelated
        descs.append(noise(m) if unrelated else np.ascontiguousarray((dI if k % 2 == 0 else dJ)[:m]))
        prios.append(np.ascontiguousarray(shared[:m]))
    return descs, prios
