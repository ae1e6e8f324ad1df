"""Views for tests/test_gpu_prefix_pruning.py (the pruning build of the f32 2-NN kernel), and for the CPU test that runs the numpy
model of the rule on them (tests/test_prefix_prune_model.py).  128 dimensions, integer-valued float32.

Queries and the rows of dataset tile 0 are integers in [30, 70]: two of them lie about 36,000 apart (128 x twice the variance 140),
never below 20,000.  A FAR row adds 150 to its first 72 dimensions: at least 72 x 110^2 = 871,200 from every query within any prefix
of 72 to 96 dimensions.  `_at(q, steps)` is query q moved by the given steps in the first dimensions: squared distance sum(steps^2),
all of it inside the prefix."""
import numpy as np

DIM = 128
FAR_DIMS = 72


def _near(rng, n):
    return rng.integers(30, 71, (n, DIM)).astype(np.float32)


def _far(rng, n):
    a = _near(rng, n)
    a[:, :FAR_DIMS] += 150.0
    return a


def _at(q, steps):
    """q moved by `steps` in its first len(steps) dimensions, away from the nearer end of [0, 100]"""
    r = q.copy()
    s = np.asarray(steps, np.float32)
    r[:len(s)] += np.where(q[:len(s)] >= 50, -s, s)
    return r


def distances(a, b):
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    return (a64 * a64).sum(1)[:, None] - 2.0 * a64 @ b64.T + (b64 * b64).sum(1)[None, :]


def base_views(nI, nJ, seed):
    """tile 0 near (with a match, 10 away, for queries 0, 5, 65 and nJ - 1 in rows 1, 6, 9 and 20), every later tile far"""
    rng = np.random.default_rng(seed)
    b = _near(rng, nJ)
    a = np.concatenate([_near(rng, 32), _far(rng, nI - 32)])
    for row, q in ((1, 0), (6, 5), (9, 65), (20, nJ - 1)):
        a[row] = _at(b[q], [1] * 10)
    return a, b


def match_in_last_tile():
    """-> (a, b, q, row): 160 rows, 130 queries; query 70 has its match in row 140 of the last tile (far rows otherwise)"""
    a, b = base_views(160, 130, seed=21)
    a[140] = _at(b[70], [1] * 10)
    return a, b, 70, 140


def runner_up_pruned():
    """-> (a, b, q, best, second): 96 rows, 100 queries; query 7 has its match in row 3 (50 away) and its true runner-up, 16,200
    away, in row 40 of tile 1, whose other rows are far: above R x (the runner-up seen in tile 0) for R = 0.36, so the tile goes"""
    rng = np.random.default_rng(22)
    b = _near(rng, 100)
    a = np.concatenate([_near(rng, 32), _far(rng, 64)])
    a[3] = _at(b[7], [5, 5])
    a[40] = _at(b[7], [15] * 72)
    return a, b, 7, 3, 40


def forced_fallback():
    """-> (a, b, q, pruned_row, late_row): 96 rows, 100 queries; nothing in tile 0 matches query 7; row 40 of tile 1 is 16,200 away,
    all of it in the first 72 dimensions (its last 56 are the query's): above the threshold R e1 of that moment, so its tile is
    pruned; row 70 of tile 2 is 7,200 away -- below R x (the seen runner-up), above R x 16,200: the lists say match, the truth is
    none, and only the exact scan can tell"""
    rng = np.random.default_rng(23)
    b = _near(rng, 100)
    a = np.concatenate([_near(rng, 32), _far(rng, 64)])
    a[40] = _at(b[7], [15] * 72)
    a[70] = _at(b[7], [30] * 8)
    return a, b, 7, 40, 70


def ratio_boundary(case):
    """-> (a, b, q, best, matched) for R = 0.25 (ratio 0.5): 96 rows, 64 queries, query 7, best row 3, tile 2 far.
    seen_tie / seen_below: runner-up row 9 at 4,000, best at 1,000 (no match: 1000 < 0.25 x 4000 is false) / at 999 (match).
    pruned_at_threshold / pruned_above: best at 1,000, seen runner-up row 9 at 8,000, so T = max(R 8000, 1000 / R) = 4,000; row 40
    of tile 1 at exactly 4,000 (not above T: the tile runs, no match) / at 4,001 (pruned; 1000 < 0.25 x 4001: match)."""
    rng = np.random.default_rng(24)
    b = _near(rng, 64)
    a = np.concatenate([_near(rng, 32), _far(rng, 64)])
    q = b[7]
    if case in ("seen_tie", "seen_below"):
        a[3] = _at(q, [10] * 10) if case == "seen_tie" else _at(q, [10] * 9 + [9, 3, 3])
        a[9] = _at(q, [20] * 10)
        return a, b, 7, 3, case == "seen_below"
    a[3] = _at(q, [10] * 10)
    a[9] = _at(q, [20] * 20)
    a[40] = _at(q, [20] * 10) if case == "pruned_at_threshold" else _at(q, [20] * 10 + [1])
    return a, b, 7, 3, case == "pruned_above"
