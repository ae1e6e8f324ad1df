"""Views for tests/test_gpu_half_prefix.py (the f16 prefix test of l2_knn2_half_kernel: the restart's 96-dimension prefix test once more on
the rows rounded to f16, in front of the restart, thrQ = thr + marginQ) and for the CPU test that runs the numpy model on them
(tests/test_half_prefix_rule.py).  128 dimensions.

ORIENTED views: every row holds 64 pairs (x[2k], x[2k+1]) that are (P, 0) or (0, P), P = 40, so every row has the SAME pair norms: the
pair-norm bound of any two rows is 0, neither the f16 level nor the pair-norm filter ever prunes, and every tile behind tile 0 reaches
the restart.  Two rows lie 2 P^2 = 3,200 apart per pair they orient differently: random orientations differ in about 24 of the 48
prefix pairs (76,800 in the prefix) and in about 32 of all (102,400), a lane half's threshold after tile 0 is about 0.36 x 80,000, so
the restart's prefix test prunes every tile of random rows, and so does the f16 test: the rows are small integers, exact in f16, and
marginQ = (2^-10 + 2^-14 + 2^-15) M + 2^-6 is about 220 for M = 2 x 64 x 1,600.  Rows are planted against T and T + marginQ by moving a
query in its prefix members by integer steps (the pair norms follow, the bound stays near 0)."""
import numpy as np

DIM = 128
PREFIX = 96
P = 40.0


def oriented(rng, n):
    o = rng.integers(0, 2, (n, DIM // 2))
    x = np.zeros((n, DIM), np.float32)
    x[:, 0::2] = P * (o == 0)
    x[:, 1::2] = P * (o == 1)
    return x


def oriented_views(nI, nJ, seed):
    """random orientations; queries 0, 5, 65 and nJ - 1 (where they exist) have a match in rows 1, 6, 9 and 20 of tile 0: the query
    with one tail pair turned (3,200 away, far below 0.36 x the runner-up)"""
    rng = np.random.default_rng(seed)
    b = oriented(rng, nJ)
    a = oriented(rng, nI)
    for row, q in ((1, 0), (6, 5), (9, 65), (20, nJ - 1)):
        if q < nJ and row < nI:
            a[row] = b[q]
            a[row, DIM - 2:] = a[row, DIM - 2:][::-1]
    return a, b


def moved_in_prefix(qrow, distance):
    """query row `qrow` at the squared distance `distance` (an integer), all of it in the prefix: its non-zero prefix members lowered by
    integer steps of at most 28"""
    steps, rest = [], int(distance)
    while rest > 1500:
        steps.append(28); rest -= 784
    for w in range(min(28, int(np.sqrt(rest))), -1, -1):           # four squares, none above 28
        for x in range(min(w, int(np.sqrt(rest - w * w))), -1, -1):
            r2 = rest - w * w - x * x
            for y in range(min(x, int(np.sqrt(r2))), -1, -1):
                z = int(round(np.sqrt(r2 - y * y)))
                if z <= y and z * z == r2 - y * y:
                    steps += [w, x, y, z]
                    break
            else:
                continue
            break
        else:
            continue
        break
    assert sum(s * s for s in steps) == int(distance) and len(steps) <= PREFIX // 2
    r = qrow.copy()
    nz = np.flatnonzero(r[:PREFIX])[: len(steps)]
    r[nz] -= np.asarray(steps, np.float32)
    return r


def threshold_after_tile0(a, b, q, R):
    """T of query q's lane half 0 after tile 0 (no match in sight there: T = R e1, rounded up as the kernel does)"""
    half0 = [r for r in range(32) if ((r >> 2) & 1) == 0]
    d = np.sort(((a[half0].astype(np.float64) - b[q].astype(np.float64)) ** 2).sum(1))
    assert d[0] >= R * d[1]
    return float(np.float32(R)) * d[1] * (1.0 + 2.0 ** -21)


MARGIN_SIDES = ("between", "cleared", "below")


def margin_views(model, side, R=0.36, scale=1.0):
    """-> (a, b, q, row): 96 rows, 100 queries; row 40 of tile 1 (lane half 0) is query 7 moved in its prefix to the prefix distance
    `between`: T + 0.5 marginQ (the f16 test lets the tile through, the restart's prefix test prunes it), `cleared`: T + 1.5 marginQ (the
    f16 test prunes it), `below`: T - 0.5 marginQ (the restart finishes the tile).  scale: both views times it (a power of two keeps
    every value exact)"""
    a, b = oriented_views(96, 100, seed=71)
    q, row = 7, 40
    T = threshold_after_tile0(a, b, q, R)
    _, mq = model.prefix16_bound(a, b, 12)
    want = {"between": 0.5, "cleared": 1.5, "below": -0.5}[side]
    a[row] = moved_in_prefix(b[q], int(np.ceil(T + want * float(mq[q]))))
    s = np.float32(scale)
    return a * s, b * s, q, row


def real_views(nI, nJ, seed):
    """oriented views with full 24-bit significands: times 1 / 3 plus a little noise on the non-zero members, so every value is
    rounded on its way to f16 and the pair is not an exact one (the certificate's slack enters thr)"""
    a, b = oriented_views(nI, nJ, seed)
    rng = np.random.default_rng(seed + 1)
    third = np.float32(1.0) / np.float32(3.0)
    a = (a * third + (a != 0) * rng.random(a.shape, np.float32) * np.float32(0.01)).astype(np.float32)
    b = (b * third + (b != 0) * rng.random(b.shape, np.float32) * np.float32(0.01)).astype(np.float32)
    return a, b


def range_views(kind):
    """oriented views (97 x 130) with one row outside the table's range.  The row is QUERY 70 where the case is to leave the other waves
    their pruning: M = max|a|^2 + |q|^2 carries the dataset view's largest norm for every query, a query's own norm for itself only.
    `over_range`: prefix members of 40,000 (above 32,752) and -70,000 (above 65,504) in query 70, both NaNs in the table -- the second
    wave's f16 keys are NaNs on every tile: each goes on to the restart, whose own prefix test prunes it; the batch runs the general
    form (|row|^2 >= 2^28);  `over_range_dataset`: the same members in dataset row 40 -- M and with it marginQ are so large for every
    query that the f16 test prunes nothing, and tile 1 holds NaN keys;  `nan_row`: a NaN member in query 70: the restart's keys are NaNs
    too, the second wave finishes every tile;  `huge_row`: a member of 2^14 in the tail of query 70, |row|^2 >= 2^28: the general form,
    every value still an f16;  `tiny`: prefix members around 2^-14 in place of zeros: below it (flushed to 0), at it and just above"""
    a, b = oriented_views(97, 130, seed=72)
    if kind == "over_range":
        b[70, 0] = 40000.0; b[70, 2] = -70000.0
    elif kind == "over_range_dataset":
        a[40, 0] = 40000.0; a[40, 2] = -70000.0
    elif kind == "nan_row":
        b[70, 3] = np.nan
    elif kind == "huge_row":
        b[70, DIM - 1] = 2.0 ** 14
    elif kind == "tiny":
        z = np.flatnonzero(a[40, :PREFIX] == 0)
        a[40, z[0::2]] = 2.0 ** -15 * (1.0 + 2.0 ** -3); a[40, z[1::2]] = -(2.0 ** -14)
        z = np.flatnonzero(b[7, :PREFIX] == 0)
        b[7, z[0::2]] = 2.0 ** -14 * (1.0 - 2.0 ** -24); b[7, z[1::2]] = 2.0 ** -14 * (1.0 + 2.0 ** -10 + 2.0 ** -11)
    else:
        raise ValueError(kind)
    return a, b


RANGE_KINDS = ("over_range", "over_range_dataset", "nan_row", "huge_row", "tiny")
SHAPES = ((33, 70), (97, 130), (160, 33), (64, 100))      # a partial last tile; more than one wave and nJ no multiple of 64; a dead query tile; whole tiles


def all_cases(model):
    """(name, a, b, R, must_prune) of every view pair of this file: must_prune says whether the f16 test prunes at least one tile"""
    out = [(f"oriented_views {nI} x {nJ}", *oriented_views(nI, nJ, seed=nI * 1000 + nJ), 0.36, True) for nI, nJ in SHAPES]
    out += [(f"real_views {nI} x {nJ}", *real_views(nI, nJ, seed=nI * 1000 + nJ + 7), 0.36, True) for nI, nJ in SHAPES[:2]]
    out += [(f"margin_views {side}", *margin_views(model, side)[:2], 0.36, True) for side in MARGIN_SIDES]
    out += [("margin_views between x 2^-4", *margin_views(model, "between", scale=2.0 ** -4)[:2], 0.36, True)]
    out += [(f"range_views {kind}", *range_views(kind), 0.36, kind != "over_range_dataset") for kind in RANGE_KINDS]
    return out
