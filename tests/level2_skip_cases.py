"""Views for tests/test_gpu_level2_skip.py (the skip of level 2 in l2_knn2_half_kernel: a tile that objects at the f16 level and holds a
finite f16 key at or below thrS = thrF - L goes straight to the restart) and for the CPU test that runs the numpy model on them
(tests/test_level2_skip_model.py).  Built on the sparse views of pairnorm_filter_cases.py.  Those views keep every threshold below
L -- two near rows lie about 4,500 apart, T = R e1 is about 1,000 and L = (2^-9 + 2^-13 + 2^-15) M + 2^-8 + 2^-15 about 2,300 -- so on
them the skip never fires (which half_filter_cases' `missed` shows).  WIDE views lift a few queries (PLANT_QUERIES) by 50 in eight of their sixteen
non-zero tail members: such a query's runner-up in tile 0 lies about 24,000 away, its T is about 8,000, and the band (thrS, thrH] of some
2,300 has room on both sides for a planted row, whose distance stays within what 16 steps below 30 reach.  The eight members are a row of
the 16 x 16 Hadamard matrix, so two wide queries lie as far from each other (they differ in eight lifted members) as from tile 0, and
every other query keeps its low threshold: a row planted for one wide query lies some 24,000 from every other query, which neither
objects to its tile nor skips."""
import numpy as np

import half_filter_cases as HC
import pairnorm_filter_cases as FC

LIFT = 50.0
PLANT_QUERIES = tuple(q for q in range(7, 64, 3))[:16]      # one query per planted tile, all in wave 0, none of sparse_views' matches


def _patterns():
    """16 subsets of 8 of the 16 tail members, any two different in 8 of them: rows 1 .. 15 of the Sylvester-Hadamard matrix and
    the complement of row 1"""
    H = np.array([[1.0]])
    for _ in range(4):
        H = np.block([[H, H], [H, -H]])
    return [(H[i] > 0).astype(np.float32) for i in range(1, 16)] + [(H[1] < 0).astype(np.float32)]


_PATTERNS = _patterns()


def wide_views(nI, nJ, seed):
    """FC.sparse_views with query PLANT_QUERIES[k] lifted by LIFT in the non-zero tail members of _PATTERNS[k]"""
    a, b = FC.sparse_views(nI, nJ, seed)
    for q, pattern in zip(PLANT_QUERIES, _PATTERNS):
        b[q, FC.TAIL::2] += np.float32(LIFT) * pattern
    return a, b


def at_distance(views, q, row, distance):
    """FC.at_distance with longer steps (28 instead of 15: up to 12 x 784 + 1,500), for the distances the wide views ask for"""
    a, b = views[0].copy(), views[1]
    steps, rest = [], int(distance)
    while rest > 1500:
        steps.append(28); rest -= 784
    steps += list(FC.four_squares(rest))
    assert len(steps) <= 16
    a[row] = FC.near_at(b[q], steps)
    return a, b


def _threshold(a, b, q, R):
    """T of query q's lane half 0 after tile 0 (no match in sight there: T = R e1, rounded up as the kernel does)"""
    half0 = [r for r in range(32) if ((r >> 2) & 1) == 0]
    d = np.sort(((a[half0].astype(np.float64) - b[q].astype(np.float64)) ** 2).sum(1))
    assert d[0] >= R * d[1]
    return float(np.float32(R)) * d[1] * (1.0 + 2.0 ** -21)


def plant(model, views, q, row, want, R=0.36):
    """`views` with dataset row `row` := query q at the distance whose f16 key lies `want` x L above thrF (want < 0: below), T being the
    threshold q's lane half holds after tile 0.  The distance is searched as half_filter_cases does: the f16 bound moves by about 1
    per unit of distance, with a jitter of a few units.  -> (a, b, at): at = (kh - thrF) / L as found"""
    a0, b = views
    T = _threshold(a0, b, q, R)

    def pos(dist):
        a, _ = at_distance((a0, b), q, row, dist)
        LBH, _ = model.halfnorm_bound(a, b)
        _, slack = model.pairnorm_bound(a, b)
        L = float(np.broadcast_to(model.skip_loss(a, b, LBH, "lane"), LBH.shape)[row, q])
        return a, (LBH[row, q] - slack[q] - T) / L, L

    _, p0, L = pos(4000)
    guess = int(round(4000 + (want - p0) * L))
    best = None
    for dist in range(max(guess - 24, 1), guess + 25):
        try:
            a, p, _ = pos(dist)
        except AssertionError:
            continue
        if best is None or abs(p - want) < abs(best[1] - want):
            best = (a, p)
    a, p = best
    assert abs(p - want) < 0.02, (want, p)
    return a, b, p


BAND_SIDES = ("inside", "below", "missed")


def band_views(model, side, R=0.36):
    """-> (a, b, q, row): a planted row against the band (thrS, thrH] -- `inside`: 0.05 L above thrS (level 2 runs, does not prune: the row
    lies far below thrF), `below`: 1.5 L under thrF (the skip fires), `missed`: half_filter_cases' case, inside the band and above thrF
    (level 2 runs and prunes)"""
    if side == "missed":
        return HC.half_threshold_views(model, "missed", R)[:4]
    a, b, _ = plant(model, wide_views(96, 100, seed=34), 7, 40, {"inside": -0.95, "below": -1.5}[side], R)
    return a, b, 7, 40


def block_views(model, n_tiles, nJ, positions, last_rows=32, seed=51, R=0.36):
    """wide views of n_tiles tiles (the last one of `last_rows` rows); every tile in `positions` (none is tile 0) holds one row planted
    1.5 L under the thrF of a query of its own (PLANT_QUERIES, wave 0, lane half 0 of the tile), so it objects at level 1 and skips
    level 2 for wave 0; every other tile behind tile 0 is far"""
    nI = 32 * (n_tiles - 1) + last_rows
    a, b = wide_views(nI, nJ, seed + n_tiles)
    for k, t in enumerate(positions):
        assert 0 < t < n_tiles and (t < n_tiles - 1 or last_rows >= 1)
        row = 32 * t                                       # (row 0 of a tile: lane half 0, and there when the last tile has a single row)
        a, b, _ = plant(model, (a, b), PLANT_QUERIES[k % len(PLANT_QUERIES)], row, -1.5, R)
    return a, b


def block_cases(model):
    """(name, make) over 1, 7, 8, 9, 16 and 17 tiles (17: a last tile of one row) and 70 / 130 queries: objecting tiles at position 0 of a
    block of 8, at its last position, on both sides of a block boundary, at every position, and none beyond tile 0"""
    out = [("1 tile x 70", lambda: wide_views(32, 70, seed=52))]
    for n_tiles, nJ, positions, tag in ((7, 70, (6,), "last"), (8, 130, (7,), "last of the block"), (9, 70, (7, 8), "across the boundary"),
                                        (9, 130, (8,), "first of the second block"), (16, 70, (8, 15), "first and last of the second block"),
                                        (17, 130, (15, 16), "across the boundary into a tile of one row"),
                                        (17, 70, tuple(range(1, 17)), "every position"), (16, 130, (), "none beyond tile 0")):
        out.append((f"{n_tiles} tiles x {nJ}: {tag}",
                    lambda n_tiles=n_tiles, nJ=nJ, positions=positions: block_views(model, n_tiles, nJ, positions, last_rows=1 if n_tiles == 17 else 32)))
    return out


def lowered_views(model, R=0.36):
    """-> (a, b, q): 9 tiles, 70 queries.  Tile 2 holds a match of query q (8 away) and a second row 50 away: behind it the lane half's
    T falls from about 8,000 to R x 50.  Tile 3 holds a row planted 1.5 L under the thrF of BEFORE: it objects (and skips) under the
    thresholds tile 1 ran with, and is pruned at level 1 under those of the refresh -- a candidate of its block that drops out"""
    q = PLANT_QUERIES[0]
    a, b = wide_views(32 * 9, 70, seed=61)
    a, b, _ = plant(model, (a, b), q, 32 * 3, -1.5, R)
    a[32 * 2] = FC.near_at(b[q], [2, 2])
    a[32 * 2 + 1] = FC.near_at(b[q], [5, 5])
    return a, b, q


def all_cases(model):
    """(name, a, b, R) of every view pair of this file"""
    out = [(f"band_views {side}", *band_views(model, side)[:2], 0.36) for side in BAND_SIDES]
    out += [(f"block_views {name}", *make(), 0.36) for name, make in block_cases(model)]
    out.append(("lowered_views", *lowered_views(model)[:2], 0.36))
    return out
