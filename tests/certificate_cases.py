"""The case table of the certificate tests (tests/test_certificate_cases.py on the CPU, tests/test_gpu_certificate.py on the GPU).

Every float 2-NN path nominates two rows per query from keys ||a||^2 - 2 a.q accumulated in the matrix pipe's own order, re-scores
the nominees in the reference arithmetic and keeps them only if

    eb < (bound + ||q||^2) - slack,        slack = err_scale (max||a||^2 + ||q||^2) + slack_abs

(kernels_match_common.hpp, l2_finish_queries; err_scale: api_match.cpp, cert_slack_factor).  The cases here put views where the key's
rounding error is of the order of the gap between the runner-up and the third row -- norms much larger than distances -- which is
where a wrong slack, a wrong max||a||^2 or a wrong bound gives a wrong answer instead of a slow one.

A case carries a name, its family, the path it is meant for ("f32": the default tiles, "split" / "counts": set_split_mfma), the
regime it claims ("easy", "transition", "teeth", "hard": tests/test_certificate_cases.py proves the claim from the restatements
below) and a generator of (dataset, query) from a fixed seed.  Two restatements of the host's arithmetic live here as well:
emulated_keys / exact_keys and slack / certify.  They are written from the description of the arithmetic in
kernels_match_common.hpp and DESIGN.md; they are emulations of an accumulation ORDER, not of the matrix unit.
"""
import functools

import numpy as np

TILE_ROWS = 32
PATHS = ("f32", "split", "counts")
REGIMES = ("easy", "transition", "teeth", "hard")
ORDERS = ("seq", "block2", "block16", "pairwise")
U24 = np.float32(5.9604645e-08)        # 2^-24, as api_match.cpp spells it
U22 = np.float32(2.3841858e-07)        # 2^-22


# ------------------------------------------------------------------------------------------------ the host's rules, restated
def kernel_G_for(dim):
    g = (dim + 7) // 8
    return 8 if g <= 8 else 16 if g <= 16 else 18 if g <= 18 else 32 if g <= 32 else g


def has_tensor_kernel(G):
    return G in (8, 16, 18, 32)


def dpad_of(dim):
    return 8 * kernel_G_for(dim)


def counts_eligible(a):
    """r3dm_ctx.hpp counts_eligible: f32, at least one row, at most 256 dimensions"""
    return a.dtype == np.float32 and a.shape[0] > 0 and a.shape[1] <= 256


def split_k_of(max_abs):
    """the power of two that brings max|x| into [2^13, 2^14) (stage_split_kernel), clamped to +-100"""
    if not (max_abs > 0 and np.isfinite(max_abs)):
        return 0
    e = int((np.float32(max_abs).view(np.uint32) >> 23) & 0xFF) - 127
    return int(np.clip(13 - e, -100, 100))


def split_eligible(a, b):
    """api_match.cpp plan_batch: both views finite and non-zero, scales within reach of one another, not both integer-valued"""
    ma, mb = float(np.abs(a).max()), float(np.abs(b).max())
    if not (np.isfinite(ma) and np.isfinite(mb) and ma > 0 and mb > 0):
        return False
    ka, kb = split_k_of(ma), split_k_of(mb)
    both_integer = np.array_equal(a, np.rint(a)) and np.array_equal(b, np.rint(b))
    return abs(ka - kb) <= 40 and abs(ka + kb) <= 100 and not both_integer


def counts_form(rows):
    """stage_counts_kernel's test, per view: every row is integers 0..2047 times one scale within 2^-21 max|row|, and the scale is
    found from the row's smallest positive element divided by 1..64"""
    rows = np.asarray(rows, np.float32)
    if (rows < 0).any() or not np.isfinite(rows).all():
        return False
    for r in rows:
        amax = r.max()
        if amax == 0:
            continue
        amin = r[r > 0].min()
        ok = False
        for k in range(1, 65):
            s_try = np.float32(amin / np.float32(k))
            if not (amax / s_try <= np.float32(2047.5)):
                break
            q = r / s_try
            cnt = np.rint(q)
            if (np.abs(q - cnt) > 0.0625).any():
                continue
            sc = np.float32((r * cnt).sum(dtype=np.float32) / (cnt * cnt).sum(dtype=np.float32))
            if (np.abs(r - cnt * sc) <= np.float32(4.76837158203125e-07) * amax).all():
                ok = True
                break
        if not ok:
            return False
    return True


def path_eligible(path, a, b):
    if not has_tensor_kernel(kernel_G_for(a.shape[1])):
        return False
    if path == "f32":
        return True
    if not split_eligible(a, b):
        return False
    both = counts_eligible(a) and counts_eligible(b) and counts_form(a) and counts_form(b)
    return both if path == "counts" else not both


# ------------------------------------------------------------------------------------------------ the arithmetic, restated
def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def norms_f32(x):
    """||row||^2 as a sequential f32 sum of squares"""
    x = np.asarray(x, np.float32)
    acc = np.zeros(x.shape[0], np.float32)
    for k in range(x.shape[1]):
        acc = _f32(acc.astype(np.float64) + x[:, k].astype(np.float64) ** 2)
    return acc


def ref_distances(a, b):
    """[nJ, nI] squared distances in the reference's arithmetic (OpenMVG L2<float>): f32, four-way unrolled, no fused multiply-add,
    scalar tail.  tests/test_certificate_cases.py holds it to the oracle bit for bit."""
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    dim = a.shape[1]
    res = np.zeros((b.shape[0], a.shape[0]), np.float32)
    k = 0
    while k + 3 < dim:
        d = [b[:, None, k + i] - a[None, :, k + i] for i in range(4)]
        res = res + (((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + d[3] * d[3])
        k += 4
    while k < dim:
        d0 = b[:, None, k] - a[None, :, k]
        res = res + d0 * d0
        k += 1
    return res


def exact_keys(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return (a * a).sum(axis=1)[None, :] - 2.0 * (b @ a.T)


def emulated_keys(a, b, order="seq"):
    """[nJ, nI] f32 keys ||a||^2 - 2 a.q: the accumulator starts at the f32 norm and takes the products of the row with the query
    scaled by -2 (exact) in one of these orders:
      seq       one fused multiply-add per dimension
      block2    the exact sum of 2 products per step, one rounding per step (v_mfma_f32_32x32x2_f32 issues k-steps of 2)
      block16   the same in steps of 16 (the f16 instructions' k)
      pairwise  products rounded to f32, summed as a balanced tree, added to the norm last
      split16   (split planes) values scaled by the view's power of two and cut into hi + lo f16 pieces; lo.hi, hi.lo, hi.hi of
                every 16 dimensions added in that order, the lo.lo term dropped; keys returned in the views' own units
    (a fused multiply-add is modelled as the f64 sum rounded to f32: a double rounding, which differs from the true one in about
    one addition of 2^29.)"""
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    dim = a.shape[1]
    na = norms_f32(a)
    a64 = a.astype(np.float64); q64 = -2.0 * b.astype(np.float64)
    if order == "split16":
        ka, kb = split_k_of(float(np.abs(a).max())), split_k_of(float(np.abs(b).max()))
        sa, sb = a64 * 2.0 ** ka, b.astype(np.float64) * 2.0 ** kb
        ah = sa.astype(np.float16).astype(np.float64); al = (sa - ah).astype(np.float16).astype(np.float64)
        bh = sb.astype(np.float16).astype(np.float64); bl = (sb - bh).astype(np.float16).astype(np.float64)
        acc = np.broadcast_to(_f32(na.astype(np.float64) * 2.0 ** (ka + kb))[None, :], (b.shape[0], a.shape[0])).astype(np.float32)
        for k0 in range(0, dim, 16):
            s = slice(k0, min(k0 + 16, dim))
            for x, y in ((al, bh), (ah, bl), (ah, bh)):
                acc = _f32(acc.astype(np.float64) - 2.0 * (y[:, s] @ x[:, s].T))
        return _f32(acc.astype(np.float64) * 2.0 ** -(ka + kb))
    acc = np.broadcast_to(na[None, :], (b.shape[0], a.shape[0])).astype(np.float32)
    if order == "seq":
        for k in range(dim):
            acc = _f32(acc.astype(np.float64) + q64[:, k, None] * a64[None, :, k])
        return acc
    if order in ("block2", "block16"):
        step = 2 if order == "block2" else 16
        for k0 in range(0, dim, step):
            s = slice(k0, min(k0 + step, dim))
            acc = _f32(acc.astype(np.float64) + q64[:, s] @ a64[:, s].T)
        return acc
    if order == "pairwise":
        n2 = 1 << max(0, int(np.ceil(np.log2(max(dim, 1)))))
        out = np.empty((b.shape[0], a.shape[0]), np.float32)
        for j0 in range(0, b.shape[0], 64):                              # (chunks of queries: the product cube is large)
            p = np.zeros((min(64, b.shape[0] - j0), a.shape[0], n2), np.float32)
            p[:, :, :dim] = _f32(q64[j0:j0 + 64, None, :] * a64[None, :, :])
            while p.shape[2] > 1:
                p = p[:, :, 0::2] + p[:, :, 1::2]
            out[j0:j0 + 64] = p[:, :, 0] + na[None, :]
        return out
    raise ValueError(order)


def slack(path, dpad, max_norm, nb, split_k_sum=0, permille=1000):
    """the host's two err_scale formulas (api_match.cpp) times (max||a||^2 + ||q||^2), plus the absolute part of the split planes
    (Dpad 2^-9 in key units, kernels_match_16bit.hip); the count tiles have none.  permille scales err_scale alone, as the
    developer build's R3DM_CERT_SLACK_PERMILLE does.  All in f32, as the tail evaluates it."""
    if path == "f32":
        err = np.float32(4.25) * np.float32(dpad) * U24
        sabs = np.float32(0.0)
    else:
        err = (np.float32(3.0) * np.float32(dpad) + np.float32(36.0)) * U22
        sabs = np.float32(dpad) * np.float32(0.001953125) * np.float32(2.0 ** -split_k_sum) if path == "split" else np.float32(0.0)
    if permille != 1000:
        err = np.float32(err * np.float32(permille * 0.001))
    return err * (np.float32(max_norm) + np.asarray(nb, np.float32)) + sabs


def case_slack(path, a, b, permille=1000):
    """slack per query of a (dataset, query) pair on `path`"""
    ks = split_k_of(float(np.abs(a).max())) + split_k_of(float(np.abs(b).max())) if path == "split" else 0
    return slack(path, dpad_of(a.shape[1]), norms_f32(a).max(), norms_f32(b), ks, permille)


RIGHT, WRONG, UNCERTIFIED = 0, 1, 2


def _smallest(x, k):
    """[n, k] columns of the k smallest entries of every row of x, ordered by (value, column): a partition to k + 6 candidates
    and a sort among them (more than six entries equal to the k-th smallest do not occur in these views)"""
    n = x.shape[1]
    if n <= k + 6:
        return np.lexsort((np.broadcast_to(np.arange(n), x.shape), x), axis=1)[:, :k]
    cand = np.sort(np.argpartition(x, k + 5, axis=1)[:, :k + 6], axis=1)
    o = np.argsort(np.take_along_axis(x, cand, axis=1), axis=1, kind="stable")[:, :k]        # stable on ascending columns: ties -> lowest column
    return np.take_along_axis(cand, o, axis=1)


def true_top2(dist):
    """(idx [nJ,2], dist [nJ,2]) of a reference distance matrix: smallest distance first, equal distances -> lowest row"""
    order = _smallest(dist, 2)
    return order.astype(np.int32), np.take_along_axis(dist, order, axis=1)


def certify(a, b, path, order="seq", permille=1000, keys=None, dist=None, slack_of=None, second_chance=False):
    """the tail's rule on emulated keys: the two smallest keys nominate, the nominees are re-scored with the reference distance and
    ordered by (distance, row), the third key is the bound, and the pair is kept if eb < (bound + ||q||^2) - slack.  Returns per
    query RIGHT (certified and the reference's 2-NN), WRONG (certified and not) or UNCERTIFIED.
    slack_of: the slack per query in place of the host's (a planted bug: tests/test_certificate_cases.py shows which cases notice).
    second_chance: an uncertified query is certified after all if the best two (by reference distance) of the four rows that its two
    lane halves nominate -- rows (r & 3) + 8 (r >> 2) + 4 h of every tile belong to half h -- beat the smaller of the halves' third
    keys by the slack (l2_finish_queries<SPLIT>).  The count tiles stream their rows in the order of their scales, so for them
    the halves here are not the device's: an approximation of how much the second chance rescues."""
    keys = emulated_keys(a, b, order) if keys is None else keys
    dist = ref_distances(a, b) if dist is None else dist
    nI = a.shape[0]
    rank = _smallest(keys, min(3, nI))
    n0, n1 = rank[:, 0], rank[:, 1]
    bound = np.take_along_axis(keys, rank[:, 2:3], axis=1)[:, 0] if nI > 2 else np.full(len(b), np.inf, np.float32)
    rows = np.arange(len(b))
    e0, e1 = dist[rows, n0], dist[rows, n1]
    swap = (e1 < e0) | ((e1 == e0) & (n1 < n0))
    ia, ib = np.where(swap, n1, n0), np.where(swap, n0, n1)
    ea, eb = np.where(swap, e1, e0), np.where(swap, e0, e1)
    nb = norms_f32(b)
    sl = case_slack(path, a, b, permille) if slack_of is None else np.asarray(slack_of, np.float32)
    certified = eb < (bound.astype(np.float32) + nb) - sl
    if second_chance and nI >= 6:
        half = _lane_half(np.arange(nI) % TILE_ROWS)
        noms, bound4 = [], np.full(len(b), np.inf, np.float32)
        for h in (0, 1):
            kh = np.where(half[None, :] == h, keys, np.float32(np.inf))
            rh = _smallest(kh, 3)
            noms.append(rh[:, :2])
            bound4 = np.minimum(bound4, kh[rows, rh[:, 2]])
        noms = np.concatenate(noms, axis=1)                                  # [nJ, 4]
        nd = np.take_along_axis(dist, noms, axis=1)
        o4 = np.lexsort((noms, nd), axis=1)[:, :2]
        ja, jb = noms[rows, o4[:, 0]], noms[rows, o4[:, 1]]
        fa, fb = nd[rows, o4[:, 0]], nd[rows, o4[:, 1]]
        again = ~certified & (fb < (bound4 + nb) - sl)
        ia, ib = np.where(again, ja, ia), np.where(again, jb, ib)
        ea, eb = np.where(again, fa, ea), np.where(again, fb, eb)
        certified = certified | again
    tidx, tdist = true_top2(dist)
    same = (ia == tidx[:, 0]) & (ib == tidx[:, 1]) & (ea == tdist[:, 0]) & (eb == tdist[:, 1])
    return np.where(~certified, UNCERTIFIED, np.where(same, RIGHT, WRONG)).astype(np.int8)


# ------------------------------------------------------------------------------------------------ the cases
class Case:
    def __init__(self, name, family, path, regime, make, tie=False, note="", rescued=False):
        assert path in PATHS and regime in REGIMES
        self.name, self.family, self.path, self.regime, self._make, self.tie, self.note = name, family, path, regime, make, tie, note
        self.rescued = rescued        # split / count tiles: the four-nominee second chance certifies what the three-key rule cannot

    def device_band(self):
        """(lowest, highest) share of the case's queries that the device may send to the exact scan.  On the f32 tiles the tail is
        the rule that tests/test_certificate_cases.py evaluates, so the band is the regime's own (transition: exclusive ends).  The
        split and count tiles add the second chance, which only ever certifies MORE: the upper ends stay, the lower end stays for
        the hard cases that the emulated second chance does not rescue either (proved there), and falls to 0 otherwise."""
        lo, hi = {"easy": (0.0, 0.05), "transition": (0.10, 0.90), "hard": (0.95, 1.0), "teeth": (0.95, 1.0)}[self.regime]
        if self.path != "f32" and (self.regime == "transition" or self.rescued):
            lo = 0.0
        return lo, hi

    def make(self):
        """(dataset [nI, D] f32, query [nJ, D] f32), the same arrays on every call"""
        return _made(self.name)


CASES = {}          # name -> Case, in the order of the sweep of each path: its first case is the easiest, its last the hardest


@functools.lru_cache(maxsize=None)
def _made(name):
    a, b = CASES[name]._make()
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    a.setflags(write=False); b.setflags(write=False)
    return a, b


def _add(name, family, path, regime, make, **kw):
    assert name not in CASES, name
    CASES[name] = Case(name, family, path, regime, make, **kw)


def _seed(*parts):
    return np.random.default_rng([int(p) & 0x7FFFFFFF for p in parts])


# ---- common offset: c t + sigma N(0, 1), c a fixed unit-normal direction
def offset_views(dim, nI, nJ, t, sigma=1.0, seed=0, tI=None, tJ=None):
    rng = _seed(1, dim, nI, nJ, int(t * 16), seed)
    c = _seed(7, dim).normal(size=dim)                     # the direction depends on the length alone: views of one collection share it
    tI = t if tI is None else tI; tJ = t if tJ is None else tJ
    a = c[None, :] * np.asarray(tI, np.float64).reshape(-1, 1) * sigma + sigma * rng.normal(size=(nI, dim))
    b = c[None, :] * np.asarray(tJ, np.float64).reshape(-1, 1) * sigma + sigma * rng.normal(size=(nJ, dim))
    return a.astype(np.float32), b.astype(np.float32)


OFFSETS = {"f32": (0, 1, 3, 10, 20, 100, 300, 1000, 3000), "split": (0, 1, 5, 10, 15, 100, 300, 1000, 3000)}       # in units of sigma

# (dim, rows of the dataset view, queries): ragged last tiles on both sides
_SHAPES = {37: (421, 203), 64: (733, 301), 100: (1187, 257), 128: (613, 307), 144: (2091, 299), 256: (357, 271)}

# the full sweep at D = 128, both paths; the regime of every offset is what tests/test_certificate_cases.py measures under the
# sequential order (its table is in DESIGN.md 4.1) -- the split planes' slack is twelve times the f32 tiles', so their
# transition sits at smaller offsets
_REGIME_128 = {"f32": {0: "easy", 1: "easy", 3: "easy", 10: "transition", 20: "transition", 100: "hard", 300: "hard", 1000: "hard", 3000: "hard"},
               "split": {0: "easy", 1: "easy", 5: "transition", 10: "transition", 15: "transition", 100: "hard", 300: "hard", 1000: "hard", 3000: "hard"}}
for _path in ("f32", "split"):
    for _t in OFFSETS[_path]:
        _add(f"offset_{_path}_d128_t{_t}", "offset", _path, _REGIME_128[_path][_t],
             functools.partial(offset_views, 128, *_SHAPES[128], _t, 1.0 if _path == "f32" else 0.25))
# the other descriptor lengths: one offset on each side of the transition and one inside it
_REGIME_DIMS = {"f32": {0: "easy", 20: "transition", 1000: "hard"}, "split": {0: "easy", 10: "transition", 300: "hard"}}
for _path in ("f32", "split"):
    for _dim in (37, 64, 100, 144, 256):
        for _t, _reg in _REGIME_DIMS[_path].items():
            if (_path, _dim, _t) == ("f32", 256, 20):
                _t = 10                        # (at D = 256 an offset of 20 leaves 91 % uncertified: outside the label)
            _add(f"offset_{_path}_d{_dim}_t{_t}", "offset", _path, _reg, functools.partial(offset_views, _dim, *_SHAPES[_dim], _t))


# ---- mixed norms: the slack reads max||a||^2 of I and ||q||^2 of J
def _mixed_half(t, dim=128, nI=613, nJ=307):
    tI = np.where(np.arange(nI) % 2 == 0, float(t), 0.0); tJ = np.where(np.arange(nJ) % 2 == 0, float(t), 0.0)
    return offset_views(dim, nI, nJ, t, seed=11, tI=tI, tJ=tJ)


def _mixed_one_large_row(where, big=3000.0, dim=128, nI=609, nJ=307):
    """unit-variance rows and one row of very large norm: the only occupant of the last partial tile (609 = 19 x 32 + 1) or row 0"""
    tI = np.zeros(nI); tI[nI - 1 if where == "last" else 0] = big
    return offset_views(dim, nI, nJ, 0, seed=12, tI=tI)


def _mixed_sides(large_side, t, dim=128, nI=613, nJ=307):
    return offset_views(dim, nI, nJ, t, seed=13, tI=t if large_side == "dataset" else 0.0, tJ=t if large_side == "query" else 0.0)


for _path in ("f32", "split"):
    _add(f"mixed_half_{_path}_t10", "mixed", _path, "transition", functools.partial(_mixed_half, 10))
    _add(f"mixed_half_{_path}_t100", "mixed", _path, "hard", functools.partial(_mixed_half, 100))
    _add(f"mixed_large_last_{_path}", "mixed", _path, "hard", functools.partial(_mixed_one_large_row, "last"),
         note="max||a||^2 comes from the one row of the last partial tile: a slack from any other tile certifies everything")
    _add(f"mixed_large_row0_{_path}", "mixed", _path, "hard", functools.partial(_mixed_one_large_row, "row0"))
    for _t, _reg in ((300, "easy"), (3000, "hard")):
        _add(f"mixed_large_queries_{_path}_t{_t}", "mixed", _path, _reg, functools.partial(_mixed_sides, "query", float(_t)),
             note="||q||^2 alone makes the slack: with max||a||^2 only, every query would certify")
    # (rows c t + noise rank alike for every small query: the gap behind the runner-up is one number per view, and the case a step)
    for _t, _reg in ((3, "easy"), (3000, "hard")):
        _add(f"mixed_large_dataset_{_path}_t{_t}", "mixed", _path, _reg, functools.partial(_mixed_sides, "dataset", float(_t)))


# ---- gap ladder: three planted rows per query at reference distances d, d (1 + g2), d (1 + g3); g3 - g2 in octaves around slack / d
LADDER_OCTAVES = tuple(range(-8, 5))          # (g3 - g2) d = slack 2^o
PLACEMENTS = ("same_half", "opposite_halves", "different_tiles", "last_partial_tile")


def _lane_half(row):
    return (row >> 2) & 1                      # tile layout: the accumulator of lane half h holds rows (r & 3) + 8 (r >> 2) + 4 h


def ladder_rows(placement, j, n_tiles_full, n_last):
    """rows of (best, runner-up, third) for query j: the runner-up and the third as the placement says, the best in another tile"""
    if placement == "last_partial_tile":
        base = n_tiles_full * TILE_ROWS
        assert 2 * j + 1 < n_last
        assert 3 + 17 * j < base
        return 3 + 17 * j, base + 2 * j, base + 2 * j + 1
    t = 2 * j                                  # two tiles per query: [t] holds the pair (or the runner-up), [t + 1] the best (and the third)
    assert t + 1 < n_tiles_full
    if placement == "same_half":
        return (t + 1) * TILE_ROWS + 5, t * TILE_ROWS + 9, t * TILE_ROWS + 18           # rows 9 and 18: (9 >> 2) & 1 == (18 >> 2) & 1 == 0
    if placement == "opposite_halves":
        return (t + 1) * TILE_ROWS + 5, t * TILE_ROWS + 9, t * TILE_ROWS + 14           # row 14: half 1
    return (t + 1) * TILE_ROWS + 5, t * TILE_ROWS + 9, (t + 1) * TILE_ROWS + 22        # different tiles


def ladder_views(placement, path, t=30.0, dim=128, d=4.0, g2=0.5, tie=False):
    reps = 1 if placement == "last_partial_tile" else 6
    nJ = len(LADDER_OCTAVES) * reps
    n_tiles_full = 2 * nJ if placement != "last_partial_tile" else 9
    n_last = 2 * nJ + 1 if placement == "last_partial_tile" else 11
    nI = n_tiles_full * TILE_ROWS + n_last
    rng = _seed(2, PLACEMENTS.index(placement), PATHS.index(path), int(t), dim)
    c = rng.normal(size=dim)
    a = (c[None, :] * t + rng.normal(size=(nI, dim))).astype(np.float32)               # the filler: about 2 D from every query
    b = (c[None, :] * t + rng.normal(size=(nJ, dim))).astype(np.float32)
    planted = set()
    for j in range(nJ):
        planted.update(ladder_rows(placement, j, n_tiles_full, n_last))
    sl = float(np.median(slack(path, dpad_of(dim), norms_f32(a).max(), norms_f32(b),
                               split_k_of(float(np.abs(a).max())) + split_k_of(float(np.abs(b).max())))))
    for j in range(nJ):
        gap = sl * 2.0 ** LADDER_OCTAVES[j % len(LADDER_OCTAVES)]
        want = (d, d * (1 + g2), d * (1 + g2) + (0.0 if tie else gap))
        rows = ladder_rows(placement, j, n_tiles_full, n_last)
        v = rng.normal(size=dim); v /= np.linalg.norm(v)
        w = rng.normal(size=dim); w -= v * (w @ v); w /= np.linalg.norm(w)
        dirs = (v, w, -w if not tie else w)
        for r, dist, u in zip(rows, want, dirs):
            a[r] = (b[j].astype(np.float64) + np.sqrt(dist) * u).astype(np.float32)
        if tie:
            a[rows[2]] = a[rows[1]]
    if not tie:
        # from the reference's own distances: the runner-up and the third must be distinct rows at distinct f32 distances, in
        # that order -- where rounding closed a gap of the lowest octaves, push the third row away one step at a time
        for j in range(nJ):
            r1, r2, r3 = ladder_rows(placement, j, n_tiles_full, n_last)
            for _ in range(64):
                dd = ref_distances(a[[r2, r3]], b[j:j + 1])[0]
                if dd[1] > dd[0]:
                    break
                a[r3] = (b[j] + (a[r3] - b[j]) * np.float32(1.0 + 2.0 ** -18)).astype(np.float32)
    return a, b


for _path in ("f32", "split"):
    for _pl in PLACEMENTS:
        _add(f"ladder_{_pl}_{_path}", "ladder", _path, "transition", functools.partial(ladder_views, _pl, _path, 30.0 if _path == "f32" else 10.0))
    _add(f"ladder_tie_{_path}", "ladder", _path, "hard", functools.partial(ladder_views, "opposite_halves", _path, 30.0 if _path == "f32" else 10.0, tie=True),
         tie=True, rescued=_path != "f32", note="the runner-up and the third are the same vector: lowest row wins, no gap certifies")


# ---- count rows and split rows: integer votes with a common offset along a heavy-bin direction, divided by their norm as vl_liop does
def liop_like(rng, n, dim, t=0, top=40, heavy=0.02):
    """tests/test_gpu_count_tiles.py's _liop_like with t u added to the votes, u a fixed direction of a few full bins"""
    ru = np.random.default_rng(dim)                                       # the direction depends on the length alone: shared by both views
    u = np.zeros(dim); u[ru.choice(dim, dim // 8, replace=False)] = ru.integers(10, 40, dim // 8)
    c = rng.poisson(rng.gamma(0.6, top / 0.6, (n, dim))).astype(np.float32) + np.float32(t) * u.astype(np.float32)[None, :]
    big = rng.random(n) < heavy
    c[big, rng.integers(0, dim, big.sum())] += rng.integers(300, 1900, big.sum())
    c = np.minimum(c, 2047.0)
    c[c.sum(axis=1) == 0, 0] = 1.0
    norm = np.zeros(n, np.float32)
    for i in range(dim):
        norm = (norm + c[:, i] * c[:, i]).astype(np.float32)
    norm = np.maximum(np.sqrt(norm.astype(np.float64)), 1e-12).astype(np.float32)
    return (c / norm[:, None]).astype(np.float32), c


def count_views(t, top=40, variant="counts", dim=144, nI=1211, nJ=299, scale_I=1.0, scale_J=1.0):
    """votes of mean level `top` on an offset of t u: the smaller the votes beside the offset, the closer the normalised rows"""
    rng = _seed(3, int(t), dim, nI, nJ, int(top * 2))
    a, _ = liop_like(rng, nI, dim, t, top)
    b, _ = liop_like(rng, nJ, dim, t, top)
    if variant == "off_lattice":               # one row off the votes-x-scale lattice: the view keeps the split planes
        a = a.copy(); a[3] = a[3] * np.float32(1.0 + 3e-5) + np.float32(1e-4) * rng.random(dim).astype(np.float32)
    elif variant == "signed":                  # a negative element
        b = b.copy(); b[17, 5] = -b[17, 5] - np.float32(0.01)
    return a * np.float32(scale_I), b * np.float32(scale_J)              # (powers of two: exact)


# (on the device the four-nominee second chance certifies more than the emulation's rule: (40, 40) leaves 9 % to the exact scan)
_COUNT_SWEEP = (((0, 40), "easy"), ((40, 40), "transition"), ((40, 30), "transition"), ((40, 20), "transition"), ((40, 10), "hard"),
                ((50, 0.5), "hard"))      # (t, top)
for (_t, _top), _reg in _COUNT_SWEEP:
    _add(f"counts_t{_t}_top{_top}", "counts", "counts", _reg, functools.partial(count_views, _t, _top))
    for _variant in ("off_lattice", "signed"):
        _add(f"split_{_variant}_t{_t}_top{_top}", "counts", "split", _reg, functools.partial(count_views, _t, _top, _variant))
for _name, _si, _sj in (("small", 2.0 ** -20, 2.0 ** -20), ("large", 2.0 ** 14, 2.0 ** 14)):
    _add(f"counts_t40_top20_scale_{_name}", "counts", "counts", "transition", functools.partial(count_views, 40, 20, scale_I=_si, scale_J=_sj))
    _add(f"split_off_lattice_t40_top20_scale_{_name}", "counts", "split", "transition", functools.partial(count_views, 40, 20, "off_lattice", scale_I=_si, scale_J=_sj))
_add("counts_t0_top40_scale_mixed", "counts", "counts", "hard", functools.partial(count_views, 0, 40, scale_I=2.0 ** -20, scale_J=2.0 ** 14),
     note="views 34 octaves apart: every distance is ||q||^2 to f32 precision")
_add("split_signed_t0_top40_scale_mixed", "counts", "split", "hard", functools.partial(count_views, 0, 40, "signed", scale_I=2.0 ** 14, scale_J=2.0 ** -20))


# ---- teeth: views on which a slack of zero certifies wrong nominations (sized until at least 20 queries do); the last case of
# every path, and its hardest
_add("teeth_f32_d128_t300", "offset", "f32", "teeth", functools.partial(offset_views, 128, 613, 1201, 300))
_add("teeth_f32_d256_t300", "offset", "f32", "teeth", functools.partial(offset_views, 256, 613, 1201, 300))
_add("teeth_split_d128_t300", "offset", "split", "teeth", functools.partial(offset_views, 128, 613, 1201, 300))
_add("teeth_counts_t50_top0.5", "counts", "counts", "teeth", functools.partial(count_views, 50, 0.5, nJ=1201))

FAMILIES = {f: [n for n, c in CASES.items() if c.family == f] for f in ("offset", "mixed", "ladder", "counts")}


# ---- match mode: the same views as two- and three-view collections (squared metric)
RATIOS = (0.6, 0.8, 0.95, 0.999)


@functools.lru_cache(maxsize=None)
def collections():
    """name -> (views, pairs): pairs of a collection share nothing but their generator, so a third view is the dataset of one
    pair and the query of another"""
    out = {}
    for name, t in (("offset_t10", 10), ("offset_t30", 30)):
        a, b = offset_views(128, 613, 307, t)
        c, _ = offset_views(128, 421, 5, t, seed=5)
        out[name + "_2"] = ([a, b], np.array([[0, 1]], np.uint32))
        out[name + "_3"] = ([a, b, c], np.array([[0, 1], [0, 2], [1, 2]], np.uint32))
    a, b = count_views(40, 40); c, _ = count_views(40, 40, nI=517, nJ=3)
    out["counts_t40_2"] = ([a, b], np.array([[0, 1]], np.uint32))
    out["counts_t40_3"] = ([a, b, c], np.array([[0, 1], [0, 2], [1, 2]], np.uint32))
    a, b = ladder_views("opposite_halves", "f32")
    out["ladder_2"] = ([a, b], np.array([[0, 1]], np.uint32))
    return out
