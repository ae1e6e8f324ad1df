"""Views for tests/test_gpu_half_filter.py (the f16 level in front of the pair-norm filter: l2_knn2_half_kernel) and for the CPU test
that runs the numpy model of the three levels on them (tests/test_half_filter_model.py).  Built on the sparse views of
pairnorm_filter_cases.py: a near row's tail pairs are (x, 0) with x an integer in [30, 70], whose f32 pair norm is x moved one float
up and whose f16 pair norm is therefore the next f16 above x (x + 1/32 below 64, x + 1/16 from 64 on); a base pair's norm is rounded
up by up to 2^-10 of it.  Over 64 pairs the f16 bound of a near row against a near query is looser than the f32 bound by a few
hundred, against a slack of about 18 and a margin of about 13: a row the filter prunes by 1.5 slacks is far inside the f16 bound's
loss, which is what separates the levels."""
import numpy as np

import pairnorm_filter_cases as FC


def all_cases(model):
    """(name, a, b, R) of every view pair the three levels are compared on, besides those of the two older case files"""
    out = []
    for side in ("cleared", "missed"):
        out.append((f"half_threshold_views {side}", *half_threshold_views(model, side)[:2], 0.36))
    for kind in RANGE_KINDS:
        out.append((f"range_views {kind}", *range_views(kind), 0.36))
    return out


def half_threshold_views(model, side, R=0.36):
    """-> (a, b, q, row, over, margin): the views of FC.threshold_views with row 40 of tile 1 (lane half 0) := query 7 at the
    distance whose F16 bound, less the filter's slack, lies `over` above T + margin (thrH in distance units): `cleared` 1.5 margins
    above (level 1 prunes the tile), `missed` half a margin below (level 1 lets it through; the f32 bound is some hundred higher, so
    level 2 prunes it).  The distance is searched: the f16 bound moves by about 1 per unit of distance, with a jitter of a few units
    from the members the steps change"""
    a0, b = FC.sparse_views(96, 100, seed=34)
    q, row = 7, 40
    half0 = [r for r in range(32) if ((r >> 2) & 1) == 0]
    d = np.sort(((a0[half0].astype(np.float64) - b[q].astype(np.float64)) ** 2).sum(1))
    e0, e1 = d[0], d[1]
    assert e0 >= R * e1                                  # no match in sight in tile 0: T = R e1, rounded up as the kernel does
    T = float(np.float32(R)) * e1 * (1.0 + 2.0 ** -21)
    want = {"cleared": 1.5, "missed": -0.5}[side]
    best = None
    for dist in range(int(T), int(T) + 1500):
        try:
            a, _ = FC.at_distance((a0, b), q, row, dist)
        except AssertionError:
            continue
        LBH, margin = model.halfnorm_bound(a, b)
        _, slack = model.pairnorm_bound(a, b)
        over = (LBH[row, q] - slack[q] - margin[q] - T) / margin[q]
        if best is None or abs(over - want) < abs(best[0] - want):
            best = (over, a, float(margin[q]))
        if over > want + 3.0:
            break
    over, a, margin = best
    assert abs(over - want) < 0.25, (side, over)
    return a, b, q, row, over * margin, margin


RANGE_KINDS = ("scaled_up", "scaled_down", "huge_row", "negative", "nan")


def range_views(kind, nI=97, nJ=130, seed=43):
    """sparse views against f16's range: `scaled_up` (x 2^14: every non-zero pair norm lies above 65,504 and is +inf in f16 -- every
    key of level 1 is -inf or NaN, it prunes nothing), `scaled_down` (x 2^-20: the pair norms lie about 2^-14, those below are held
    at 2^-14), `huge_row` (dataset row 50 alone x 2^14 in a tile of normal rows), `negative`, `nan` (FC.other_rows)"""
    if kind in ("negative", "nan"):
        return FC.other_rows(kind, nI, nJ, seed)
    a, b = FC.sparse_views(nI, nJ, seed)
    if kind == "scaled_up":
        a = a * np.float32(2.0 ** 14); b = b * np.float32(2.0 ** 14)
    elif kind == "scaled_down":
        a = a * np.float32(2.0 ** -20); b = b * np.float32(2.0 ** -20)
    elif kind == "huge_row":
        a[50] *= np.float32(2.0 ** 14)
    else:
        raise ValueError(kind)
    return a, b
