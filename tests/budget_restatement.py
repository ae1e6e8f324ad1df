"""The match budget (r3dm_set_match_budget, include/r3dm.h) restated from the oracle alone, independent of the library: the selected
rows S of a view (numpy's stable argsort on the negated priority IS the order priority descending, row ascending; kept ascending), the
sub-arrays, the matcher of the restatements on them (symmetric_ratio_restatement: the oracle's exhaustive matcher with the mutual /
symmetric check on top), and every index mapped back through S.  Below it a brute-force selection that shares no code with the first:
python's sorted on (-p, row)."""
import numpy as np

import symmetric_ratio_restatement as SR


def _clean(priority):
    return None if priority is None else np.asarray(priority, np.float32) + np.float32(0.0)      # -0.0 is stored as +0.0


def selected_rows(priority, n, N):
    """S of a view of n rows for budget N, ascending -> int64 [min(N, n)]"""
    hn = min(N, n)
    if priority is None or hn == n:
        return np.arange(hn, dtype=np.int64)
    p = _clean(priority)
    assert len(p) == n
    order = np.argsort(-p.astype(np.float64), kind="stable")            # ties keep ascending row index
    return np.sort(order[:hn]).astype(np.int64)


def brute_force_rows(priority, n, N):
    if priority is None:
        return list(range(min(N, n)))
    p = [0.0 if float(x) == 0.0 else float(x) for x in priority]
    return sorted(sorted(range(n), key=lambda r: (-p[r], r))[:N])


def tie_straddles_cut(priority, n, N):
    """the N-th and the (N + 1)-th row under the order carry the same priority: the selection has to cut a tie class by row index"""
    if priority is None or n <= N:
        return False
    p = np.sort(_clean(priority).astype(np.float64))[::-1]
    return bool(p[N - 1] == p[N])


def sub_views(descs, xys, prios, N):
    """-> (rows per view, sub-descs, sub-xys): view v as the budget matches it"""
    rows = [selected_rows(prios[v], len(descs[v]), N) for v in range(len(descs))]
    sd = [np.ascontiguousarray(np.asarray(descs[v])[rows[v]]) for v in range(len(descs))]
    sx = None if xys is None else [None if xys[v] is None else np.ascontiguousarray(np.asarray(xys[v])[rows[v]]) for v in range(len(descs))]
    return rows, sd, sx


def map_back(pairs, counts, matches, rows):
    """matches of sub-views (per-pair counts, pair order of `pairs`) -> the same lists in the views' own row numbers"""
    out = np.asarray(matches, np.uint32).reshape(-1, 2).copy()
    off = 0
    for (I, J), c in zip(pairs, counts):
        c = int(c)
        out[off:off + c, 0] = rows[int(I)][out[off:off + c, 0]]
        out[off:off + c, 1] = rows[int(J)][out[off:off + c, 1]]
        off += c
    return out


def match_collection(O, descs, xys, prios, pairs, N, ratio, squared=True, binary=False, mode="off"):
    """the budgeted graph of the exhaustive matcher -> (counts [P], matches [M, 2] in original row numbers, sub-view matches [M, 2])"""
    rows, sd, sx = sub_views(descs, xys, prios, N)
    counts, sub, _ = SR.match_collection(O, sd, sx, pairs, ratio, squared, binary, mode)
    return counts, map_back(pairs, counts, sub, rows), sub


def whole_collection(O, descs, xys, pairs, ratio, squared=True, binary=False, mode="off"):
    counts, m, _ = SR.match_collection(O, descs, xys, pairs, ratio, squared, binary, mode)
    return counts, m


def restrict_to(pairs, counts, matches, keep):
    """(pairs, counts, matches) of a collection restricted to pairs[keep] -> (counts, matches)"""
    out, off = [], 0
    for k, c in enumerate(counts):
        c = int(c)
        if keep[k]:
            out.append(matches[off:off + c])
        off += c
    return np.asarray(counts)[keep], (np.concatenate(out).reshape(-1, 2) if out else np.zeros((0, 2), np.uint32))
