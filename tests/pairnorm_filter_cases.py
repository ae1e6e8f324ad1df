"""Views for tests/test_gpu_pairnorm_filter.py (the pair-norm filter in front of the prefix test: l2_knn2_half_kernel<…, MODE 20>) and for the CPU
test that runs the numpy model of the cascade on them (tests/test_pairnorm_filter_model.py).  128 dimensions, integer-valued float32
unless a case says otherwise.

SPARSE views: every row, query or dataset, holds the same BASE in its first 96 dimensions (integers in [30, 70]), so every
96-dimension prefix distance is 0 and the prefix test alone can stop nothing.  The last 32 dimensions hold 16 pairs with ONE non-zero
member each.  A NEAR row (queries, dataset tile 0) has the even member in [30, 70]: two of them lie about 16 x 280 = 4,500 apart, and
the pair norms keep all of it (a pair (x, 0) has the norm |x|).  A FAR row has the odd member in [150, 200]: at least
16 x (150^2 + 30^2) = 374,000 from every near row, of which the pair norms keep sum (y - x)^2 >= 16 x 80^2 = 102,400 -- far above
any threshold.  `near_at(q, steps)` is near row q moved by `steps` in its first non-zero tail members: distance sum(steps^2), all of
it kept by the pair norms."""
import numpy as np

DIM = 128
TAIL = 96


def _base(rng):
    return rng.integers(30, 71, TAIL).astype(np.float32)


def _near(rng, base, n):
    a = np.zeros((n, DIM), np.float32)
    a[:, :TAIL] = base
    a[:, TAIL::2] = rng.integers(30, 71, (n, (DIM - TAIL) // 2))
    return a


def _far(rng, base, n):
    a = np.zeros((n, DIM), np.float32)
    a[:, :TAIL] = base
    a[:, TAIL + 1::2] = rng.integers(150, 201, (n, (DIM - TAIL) // 2))
    return a


def near_at(q, steps):
    """near row q with its first len(steps) non-zero tail members lowered by `steps` (members are >= 30: keep steps below that)"""
    r = q.copy()
    s = np.asarray(steps, np.float32)
    r[TAIL:TAIL + 2 * len(s):2] -= s
    assert (r >= 0).all()
    return r


def sparse_views(nI, nJ, seed):
    """tile 0 near (with a match, 8 away, for queries 0, 5, 65 and nJ - 1 in rows 1, 6, 9 and 20), every later tile far"""
    rng = np.random.default_rng(seed)
    base = _base(rng)
    b = _near(rng, base, nJ)
    a = np.concatenate([_near(rng, base, 32), _far(rng, base, nI - 32)])
    for row, q in ((1, 0), (6, 5), (9, 65), (20, nJ - 1)):
        a[row] = near_at(b[q], [1] * 8)
    return a, b


def swapped_pairs():
    """-> (a, b, q, row): 96 rows, 100 queries; row 40 of tile 1 is query 7 with the two members of every pair swapped: its pair
    norms are the query's (bound 0), its distance is large and lies in the prefix too (the base, swapped)"""
    a, b = sparse_views(96, 100, seed=31)
    r = b[7].copy().reshape(-1, 2)[:, ::-1].reshape(-1)
    a[40] = r
    return a, b, 7, 40


def match_in_last_tile():
    """-> (a, b, q, row): 160 rows, 130 queries; query 70 has its match in row 140 of the last tile (far rows otherwise)"""
    a, b = sparse_views(160, 130, seed=32)
    a[140] = near_at(b[70], [1] * 8)
    return a, b, 70, 140


def runner_up_filtered():
    """-> (a, b, q, best, second): 96 rows, 100 queries; query 7 has its match in row 3 (50 away) and its true runner-up, 1,600
    away, in row 40 of tile 1, whose other rows are far"""
    a, b = sparse_views(96, 100, seed=33)
    a[3] = near_at(b[7], [5, 5])
    a[40] = near_at(b[7], [10] * 16)
    return a, b, 7, 3, 40


def four_squares(m, top=29):
    """non-negative integers (w, x, y, z), none above `top`, with w^2 + x^2 + y^2 + z^2 == m"""
    m = int(m)
    for w in range(min(top, int(np.sqrt(m))), -1, -1):
        for x in range(min(w, int(np.sqrt(m - w * w))), -1, -1):
            rest = m - w * w - x * x
            for y in range(min(x, int(np.sqrt(rest))), -1, -1):
                z = int(round(np.sqrt(rest - y * y)))
                if z <= y and z * z == rest - y * y:
                    return w, x, y, z
    raise AssertionError(m)


def at_distance(views, q, row, distance):
    """`views` with dataset row `row` := query q moved to the squared distance `distance` (an integer), every step below 30 so that
    the members stay non-negative"""
    a, b = views[0].copy(), views[1]
    steps, rest = [], int(distance)
    while rest > 1500:
        steps += [15, 15, 15, 15]; rest -= 900
    steps += list(four_squares(rest))
    assert len(steps) <= 16
    a[row] = near_at(b[q], steps)
    return a, b


def other_rows(kind, nI=97, nJ=130, seed=41):
    """sparse views outside the exactness proof: `negative` (every odd dimension negated), `real` (scaled by 1/16, plus a little noise
    on the non-zero members), `large_integers` (doubled: 128 x 400^2 >= 2^24), `nan` (one NaN in query 70: every key of that query is NaN, its wave -- the
    second -- may prune nothing, the other waves prune as before)"""
    a, b = sparse_views(nI, nJ, seed)
    if kind == "negative":
        a[:, 1::2] *= -1.0; b[:, 1::2] *= -1.0
    elif kind == "real":
        rng = np.random.default_rng(seed + 1)
        a = (a / np.float32(16.0) + (a != 0) * rng.random(a.shape, np.float32) * np.float32(0.01)).astype(np.float32)
        b = (b / np.float32(16.0) + (b != 0) * rng.random(b.shape, np.float32) * np.float32(0.01)).astype(np.float32)
    elif kind == "large_integers":
        a = a * np.float32(2.0); b = b * np.float32(2.0)
        assert 128.0 * float(a.max()) ** 2 >= 2.0 ** 24
    elif kind == "nan":
        b[70, 100] = np.nan
    else:
        raise ValueError(kind)
    return a, b


def threshold_views(model, side, R=0.36):
    """-> (a, b, q, row, T, slack): 96 rows, 100 queries; row 40 of tile 1 (lane half 0) is query 7 at a distance -- all of it kept by
    the pair norms -- that `model` (tools/prefix_prune_model.py) places against the threshold T the half holds after tile 0 and the
    filter's slack s: `pruned` T + 1.5 s (the filter prunes its tile), `kept_above` T + 0.5 s (above T, inside the slack: the tile
    goes on), `kept_below` T - 1.5 s (the row is the query's nearest and lies below R x the half's runner-up: its tile must run)"""
    a, b = sparse_views(96, 100, seed=34)
    q, row = 7, 40
    half0 = [r for r in range(32) if ((r >> 2) & 1) == 0]
    d = np.sort(((a[half0].astype(np.float64) - b[q].astype(np.float64)) ** 2).sum(1))
    e0, e1 = d[0], d[1]
    assert e0 >= R * e1                                  # no match in sight in tile 0: T = R e1, rounded up as the kernel does
    T = float(np.float32(R)) * e1 * (1.0 + 2.0 ** -21)
    _, slack = model.pairnorm_bound(a, b)
    s = float(slack[q])
    target = {"pruned": np.ceil(T + 1.5 * s), "kept_above": np.ceil(T + 0.5 * s), "kept_below": np.floor(T - 1.5 * s)}[side]
    a, b = at_distance((a, b), q, row, target)
    return a, b, q, row, T, s
