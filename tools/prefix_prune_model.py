"""The prefix-pruning rule of l2_knn2_prune_kernel (kernels_match.hip) restated in numpy on the kernel's own geometry (no GPU needed):
   python tools/prefix_prune_model.py [--images 14] [--feat 8192] [--gp 9 10 11 12] [--ratio 0.6] [--pairs 13] [--kind sift]
For every pair (0, j) of a synthetic collection (synth.make_scene_torch on the CPU: the generator of bench.py's c2) and every GP:
the share of wave tiles (32 dataset rows x 64 queries) pruned after 8 GP dimensions, the MFMA work left, the queries the verdict
rule sends to the exact scan, and the WRONG VERDICTS -- queries whose verdict differs from the brute-force ratio test.  That last
number must be 0 whatever the data.

The geometry: a wave holds 64 queries (two query tiles); lane half h of a query owns the rows of a dataset tile with
((row >> 2) & 1) == h; the lists a tile's decision reads hold every earlier tile that was not pruned.  The rule (kernels_match.hip,
above the kernel; l2_finish_queries<PRUNE> has the proof): per (query, half) with e0 <= e1 the two smallest distances seen,
  T = R e1 if e0 >= R e1 else max(R e1, e0 / R), rounded up;  a tile is pruned when every prefix distance of every lane lies above its T;
  pl = the smallest T a lane pruned under.  Verdict from the merged lists (ea, eb) and PL = min of both halves' pl:
  not ea < R eb -> no match;  ea < R eb and ea < R PL -> the best seen row;  else the exact scan.
Distances are exact here (integer-valued rows: float32 sums below 2^24), as the kernel's are for such pairs.
   python tools/prefix_prune_model.py --filter pairnorm [--gp 12] ...
the cascade of l2_knn2_half_kernel<…, MODE 20>: the pair-norm filter in front of the prefix test (model_pair_cascade).
   python tools/prefix_prune_model.py --filter half [--gp 12] ...
the three levels of l2_knn2_half_kernel: the same filter on pair norms rounded up to f16 in front of the cascade (model_pair_levels);
it must prune no tile the cascade does not prune.
   python tools/prefix_prune_model.py --filter half --skip lane --prefix16 [--gp 12] ...
with the f16 prefix test in front of the restart (rows_to_half, prefix16_bound): it must prune no tile the restart's f32 prefix test keeps."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

INF = np.float32(np.inf)


def _dist(a, b):
    """[nI, nJ] squared distances in float32 (exact for integer-valued rows whose sums stay below 2^24)"""
    na = (a * a).sum(1, dtype=np.float32)[:, None]
    nb = (b * b).sum(1, dtype=np.float32)[None, :]
    return na - np.float32(2.0) * (a @ b.T) + nb


def _push(d0, i0, d1, i1, key, idx):
    """fold keys [rows, q] (rows in ascending index order) into per-query (best, runner-up) lists"""
    for r in range(key.shape[0]):
        k = key[r]
        c0 = k < d0
        c1 = k < d1
        i1[:] = np.where(c0, i0, np.where(c1, idx[r], i1)); d1[:] = np.where(c0, d0, np.where(c1, k, d1))
        i0[:] = np.where(c0, idx[r], i0); d0[:] = np.where(c0, k, d0)


def model_pair(a, b, gp, R):
    """-> dict(tiles, pruned, fallback, wrong, matches, queries) for dataset view a, query view b"""
    R = np.float32(R)
    nI, nJ = a.shape[0], b.shape[0]
    D = _dist(a, b)
    DP = _dist(a[:, :8 * gp], b[:, :8 * gp])
    n_tiles = (nI + 31) // 32
    n_waves = (nJ + 63) // 64
    half_of_row = (np.arange(32) >> 2) & 1
    # lists per (half, query)
    d0 = np.full((2, nJ), INF); d1 = np.full((2, nJ), INF)
    i0 = np.full((2, nJ), -1, np.int64); i1 = np.full((2, nJ), -1, np.int64)
    pl = np.full((2, nJ), INF)
    wave_of_q = np.arange(nJ) // 64
    tiles = pruned = 0
    for t in range(n_tiles):
        lo, hi = t * 32, min(nI, t * 32 + 32)
        rows = np.arange(lo, hi)
        with np.errstate(invalid="ignore"):
            re1 = R * d1
            T = np.where(d0 < re1, np.maximum(re1, d0 / R), re1).astype(np.float32)       # [2, nJ]; +inf while a list holds < 2 rows
            T = (T + np.abs(T) * np.float32(2.0 ** -21)).astype(np.float32)               # rounded up, as the kernel does: e0 < R (e0 / R) must hold
        obj = np.zeros((2, nJ), bool)
        for h in (0, 1):
            m = half_of_row[: hi - lo] == h
            if m.any():
                obj[h] = ~(DP[rows[m]].min(0) > T[h])
        wave_obj = np.zeros(n_waves, bool)
        np.logical_or.at(wave_obj, wave_of_q, obj[0] | obj[1])
        tiles += n_waves
        pruned += int((~wave_obj).sum())
        go = wave_obj[wave_of_q]                                                       # per query: its wave runs the suffix
        pl[:, ~go] = np.minimum(pl[:, ~go], T[:, ~go])
        if go.any():
            q = np.flatnonzero(go)
            for h in (0, 1):
                m = half_of_row[: hi - lo] == h
                if m.any():
                    e0, e1, j0, j1 = d0[h, q], d1[h, q], i0[h, q], i1[h, q]
                    _push(e0, j0, e1, j1, D[rows[m]][:, q], rows[m])
                    d0[h, q], d1[h, q], i0[h, q], i1[h, q] = e0, e1, j0, j1
    # merge the halves under (distance, row)
    cd = np.concatenate([d0, d1]); ci = np.concatenate([i0, i1]).astype(np.float64)
    ci[ci < 0] = np.inf
    order = np.lexsort((ci, cd), axis=0)
    ea = np.take_along_axis(cd, order[:1], 0)[0]; eb = np.take_along_axis(cd, order[1:2], 0)[0]
    ia = np.take_along_axis(ci, order[:1], 0)[0]
    PL = pl.min(0)
    passes = ea < R * eb
    verdict = np.where(~passes, -1, np.where(ea < R * PL, ia, -2)).astype(np.int64)    # -1 none, -2 exact scan
    # the brute-force ratio test (ties -> lowest row: argsort is stable)
    o = np.argsort(D, axis=0, kind="stable")[:2]
    t1 = np.take_along_axis(D, o[:1], 0)[0]; t2 = np.take_along_axis(D, o[1:2], 0)[0]
    truth = np.where(t1 < R * t2, o[0], -1)
    decided = verdict != -2
    return {"tiles": tiles, "pruned": pruned, "fallback": int((~decided).sum()), "wrong": int((decided & (verdict != truth)).sum()),
            "matches": int((truth >= 0).sum()), "queries": nJ}


U = 2.0 ** -24
ERR_SCALE = 4.25 * 128 * U            # cert_slack_factor (api_match.cpp) of 128-dimensional rows on the f32 tiles
KEY_SLACK = 8 * U                     # kPruneKeySlack (kernels_match_common.hpp)


def pair_norms(x):
    """[n, D] float32 -> [n, D / 2] float32, element k >= sqrt(x[2k]^2 + x[2k+1]^2): stage_pairnorm_kernel (kernels_match.hip) --
    the root in double, rounded to float32, moved one float up unless it lies above the double root by 2^-40 of it already"""
    x64 = x.astype(np.float64)
    rd = np.sqrt(x64[:, 0::2] ** 2 + x64[:, 1::2] ** 2)
    f = rd.astype(np.float32)
    up = f.astype(np.float64) < rd * (1.0 + 2.0 ** -40)
    return np.where(up, np.nextafter(f, INF), f).astype(np.float32)


def _exact_pair(a, b):
    """l2_pair_is_exact (kernels_match_common.hpp): integer-valued views whose partial sums stay below 2^24"""
    if not (np.all(a == np.rint(a)) and np.all(b == np.rint(b))):
        return False
    mI, mJ = float(np.abs(a).max(initial=0.0)), float(np.abs(b).max(initial=0.0))
    d = float(a.shape[1])
    if (a < 0).any() or (b < 0).any():
        return d * (mI + mJ) ** 2 < 2.0 ** 24
    return 2 * d * mI * mJ < 2.0 ** 24 and d * mI * mI < 2.0 ** 24 and d * mJ * mJ < 2.0 ** 24


def pairnorm_bound(a, b):
    """-> (LB [nI, nJ], slack [nJ]) in float64: LB = |a|^2 + |b|^2 - 2 sum_k sa_k sb_k <= |a - b|^2, and the slack the kernel's filter
    carries for its own float32 evaluation of it, (err_scale + kPruneKeySlack) (max|a|^2 + |b|^2)"""
    sa, sb = pair_norms(a).astype(np.float64), pair_norms(b).astype(np.float64)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    na, nb = (a64 * a64).sum(1), (b64 * b64).sum(1)
    return na[:, None] + nb[None, :] - 2.0 * sa @ sb.T, (ERR_SCALE + KEY_SLACK) * (na.max(initial=0.0) + nb)


def model_pair_cascade(a, b, gp, R, filter_only=False):
    """the cascade of l2_knn2_half_kernel<…, MODE 20>: per wave tile the pair-norm filter (8 groups), and behind it, for a tile some lane still
    needs, the prefix test of model_pair on the tile run again from its group 0.  Distances in float64 (exact for the integer-valued
    views; the reference for any other, whose prefix test then carries the certificate's slack as the kernel's does).
    -> model_pair's dict + filtered (tiles the filter pruned), work (MFMA groups run, of 16 a tile)"""
    R64 = float(np.float32(R))
    nI, nJ = a.shape[0], b.shape[0]
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    D = ((a64[:, None, :] - b64[None, :, :]) ** 2).sum(2) if nI * nJ <= 1 << 16 else \
        (a64 * a64).sum(1)[:, None] - 2.0 * a64 @ b64.T + (b64 * b64).sum(1)[None, :]
    ap, bp = a64[:, :8 * gp], b64[:, :8 * gp]
    DP = (ap * ap).sum(1)[:, None] - 2.0 * ap @ bp.T + (bp * bp).sum(1)[None, :]
    LB, slackF = pairnorm_bound(a, b)
    slackP = np.zeros(nJ) if _exact_pair(a, b) else slackF
    n_tiles = (nI + 31) // 32
    n_waves = (nJ + 63) // 64
    half_of_row = (np.arange(32) >> 2) & 1
    d0 = np.full((2, nJ), np.inf); d1 = np.full((2, nJ), np.inf)
    i0 = np.full((2, nJ), -1, np.int64); i1 = np.full((2, nJ), -1, np.int64)
    pl = np.full((2, nJ), np.inf)
    wave_of_q = np.arange(nJ) // 64
    tiles = pruned = filtered = work = 0
    for t in range(n_tiles):
        lo, hi = t * 32, min(nI, t * 32 + 32)
        rows = np.arange(lo, hi)
        with np.errstate(invalid="ignore"):
            e0, e1 = d0 + slackP, d1 + slackP                                  # the lists' distances as the kernel sees them (+ slack)
            re1 = R64 * e1
            T = np.where(e0 < re1, np.maximum(re1, e0 / R64), re1)
            T = T + np.abs(T) * 2.0 ** -21
        objF = np.zeros((2, nJ), bool); objP = np.zeros((2, nJ), bool)
        for h in (0, 1):
            m = half_of_row[: hi - lo] == h
            if m.any():
                objF[h] = ~((LB[rows[m]] - slackF[None, :]).min(0) > T[h])
                objP[h] = ~((DP[rows[m]] - slackP[None, :]).min(0) > T[h])
        wF = np.zeros(n_waves, bool); wP = np.zeros(n_waves, bool)
        np.logical_or.at(wF, wave_of_q, objF[0] | objF[1])
        np.logical_or.at(wP, wave_of_q, objP[0] | objP[1])
        if filter_only:
            wP[:] = True
        wave_on = wF & wP
        tiles += n_waves
        filtered += int((~wF).sum())
        pruned += int((~wave_on).sum())
        work += 8 * n_waves + gp * int((wF & ~wP).sum()) + 16 * int(wave_on.sum())
        go = wave_on[wave_of_q]
        pl[:, ~go] = np.minimum(pl[:, ~go], T[:, ~go])
        if go.any():
            q = np.flatnonzero(go)
            for h in (0, 1):
                m = half_of_row[: hi - lo] == h
                if m.any():
                    f0, f1, j0, j1 = d0[h, q], d1[h, q], i0[h, q], i1[h, q]
                    _push(f0, j0, f1, j1, D[rows[m]][:, q], rows[m])
                    d0[h, q], d1[h, q], i0[h, q], i1[h, q] = f0, f1, j0, j1
    cd = np.concatenate([d0, d1]); ci = np.concatenate([i0, i1]).astype(np.float64)
    ci[ci < 0] = np.inf
    order = np.lexsort((ci, cd), axis=0)
    ea = np.take_along_axis(cd, order[:1], 0)[0]; eb = np.take_along_axis(cd, order[1:2], 0)[0]
    ia = np.take_along_axis(ci, order[:1], 0)[0]
    PL = pl.min(0)
    with np.errstate(invalid="ignore"):
        passes = ea < R64 * eb
        verdict = np.where(~passes, -1, np.where(ea < R64 * PL, ia, -2)).astype(np.int64)
    o = np.argsort(D, axis=0, kind="stable")[:2]
    t1 = np.take_along_axis(D, o[:1], 0)[0]; t2 = np.take_along_axis(D, o[1:2], 0)[0]
    truth = np.where(t1 < R64 * t2, o[0], -1)
    decided = verdict != -2
    return {"tiles": tiles, "pruned": pruned, "filtered": filtered, "work": work, "fallback": int((~decided).sum()),
            "wrong": int((decided & (verdict != truth)).sum()), "matches": int((truth >= 0).sum()), "queries": nJ}


HALF_MARGIN = 400 * U                 # kHalfMarginFactor (kernels_match.hip, above l2_knn2_half_kernel)
HALF_MARGIN_ABS = 2.0 ** -35          # kHalfMarginAbs
# matrix cycles of a wave tile (32 rows x 64 queries) per level: 8 v_mfma_f32_32x32x16_f16 of 32 cycles; 64 v_mfma_f32_32x32x2_f32 of
# 64 cycles per 8 groups
CYC_HALF, CYC_GROUP = 8 * 32, 8 * 64


def pair_norms_half(x):
    """[n, D] float32 -> [n, D / 2] float64 holding f16 values >= pair_norms(x): pairnorm_to_half (kernels_match.hip) -- rounded up
    from the float32 pair norm; +inf above 65,504; 2^-14 for a non-zero value below 2^-14 (no subnormal); 0 stays 0, NaN stays NaN"""
    s = pair_norms(x)
    with np.errstate(over="ignore", invalid="ignore"):
        hn = s.astype(np.float16)                                    # to nearest (overflow -> +inf)
        up = hn.astype(np.float32) < s
        hn = np.where(up, np.nextafter(hn, np.float16(np.inf)), hn).astype(np.float16)
    h = hn.astype(np.float64)
    h = np.where(s > np.float32(65504.0), np.inf, h)
    h = np.where((s != 0) & (s < np.float32(2.0 ** -14)), 2.0 ** -14, h)
    return np.where(np.isnan(s), np.nan, h)


def halfnorm_bound(a, b):
    """-> (LBH [nI, nJ], margin [nJ]) in float64: LBH = |a|^2 + |b|^2 - 2 sum_k ha_k hb_k <= pairnorm_bound's LB (ha >= sa, hb >= sb),
    NaN or -inf where a factor is +inf; and the margin thrH carries above thrF, 400 u (max|a|^2 + |b|^2) + 2^-35"""
    ha, hb = pair_norms_half(a), pair_norms_half(b)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    na, nb = (a64 * a64).sum(1), (b64 * b64).sum(1)
    with np.errstate(invalid="ignore", over="ignore"):
        # the contraction as the matrix unit sees it: a product 0 x inf is a NaN and poisons its sum
        dot = (ha[:, None, :] * hb[None, :, :]).sum(2) if a.shape[0] * b.shape[0] <= 1 << 16 else ha @ hb.T
        return na[:, None] + nb[None, :] - 2.0 * dot, HALF_MARGIN * (na.max(initial=0.0) + nb) + HALF_MARGIN_ABS


SKIP_LOSS = 2.0 ** -9 + 2.0 ** -13 + 2.0 ** -15       # kSkipLossFactor (kernels_match.hip, above l2_knn2_half_kernel)
SKIP_LOSS_ABS = 2.0 ** -8 + 2.0 ** -15                # kSkipLossAbs


def skip_loss(a, b, LBH, form="lane"):
    """L with kf_c <= kh_c + L (the derivation above l2_knn2_half_kernel), in float64, broadcastable against LBH [nI, nJ]:
    "lane": the kernel's, (2^-9 + 2^-13 + 2^-15) (max|a|^2 + |b|^2) + 2^-8 + 2^-15 -- [1, nJ];
    "key":  the key-dependent form: 2 sum sa sb <= 2 sum ha hb = |a|^2 + |b|^2 - LBH carries the factor (1 + 2^-10)^2 - 1 instead of
            M; the cross terms of the floor and the evaluation errors stay on M -- [nI, nJ]"""
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    na, nb = (a64 * a64).sum(1), (b64 * b64).sum(1)
    M = (na.max(initial=0.0) + nb)[None, :]
    if form == "lane":
        return SKIP_LOSS * M + SKIP_LOSS_ABS
    with np.errstate(invalid="ignore"):
        dot2 = na[:, None] + nb[None, :] - LBH                        # 2 sum ha hb
        return (2.0 ** -9 + 2.0 ** -20) * dot2 + (2.0 ** -13 + 2.0 ** -15) * M + SKIP_LOSS_ABS


PREFIX_MARGIN = 2.0 ** -10 + 2.0 ** -14 + 2.0 ** -15  # kPrefixMarginFactor (kernels_match.hip, above l2_knn2_half_kernel)
PREFIX_MARGIN_ABS = 2.0 ** -6                         # kPrefixMarginAbs
CYC_PREFIX16 = 12 * 32                                # the f16 prefix test: 6 v_mfma_f32_32x32x16_f16 per query tile


def rows_to_half(x):
    """[...] float32 -> float64 holding f16 values: row_to_half (kernels_match.hip) bit for bit on the float's bits -- a NaN stays a NaN,
    |x| < 2^-14 becomes +0, |x| > 32,752 becomes a NaN, any other value loses 13 significand bits to nearest, ties to even"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    mag = u & np.uint32(0x7FFFFFFF)
    v = (mag.astype(np.int64) - (112 << 23)) & 0xFFFFFFFF
    h = (((u >> np.uint32(16)) & np.uint32(0x8000)).astype(np.int64) | ((v + 0xFFF + ((v >> 13) & 1)) >> 13)) & 0xFFFF
    h = np.where(mag < np.uint32(0x38800000), 0, h)
    h = np.where(mag > np.uint32(0x46FFE000), 0x7E00, h)
    return h.astype(np.uint16).view(np.float16).astype(np.float64)


def prefix16_bound(a, b, gp):
    """-> (DPQ [nI, nJ], marginQ [nJ]) in float64: DPQ = |a_P|^2 + |b_P|^2 - 2 sum_i A_i B_i over the first 8 gp dimensions, A and B
    the rows rounded to f16 (rows_to_half; a NaN factor poisons its sum), and the margin thrQ carries above thr,
    (2^-10 + 2^-14 + 2^-15) (max|a|^2 + |b|^2) + 2^-6"""
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    na, nb = (a64 * a64).sum(1), (b64 * b64).sum(1)
    ap, bp = a64[:, :8 * gp], b64[:, :8 * gp]
    A, B = rows_to_half(a[:, :8 * gp]), rows_to_half(b[:, :8 * gp])
    with np.errstate(invalid="ignore", over="ignore"):
        dot = (A[:, None, :] * B[None, :, :]).sum(2) if a.shape[0] * b.shape[0] <= 1 << 16 else A @ B.T
        return (ap * ap).sum(1)[:, None] + (bp * bp).sum(1)[None, :] - 2.0 * dot, PREFIX_MARGIN * (na.max(initial=0.0) + nb) + PREFIX_MARGIN_ABS


def model_pair_levels(a, b, gp, R, half=True, skip=None, prefix16=False):
    """the three levels of l2_knn2_half_kernel: per wave tile the f16 level (thrH = thrF + margin), behind it the pair-norm filter,
    behind that the tile run again with the prefix test -- model_pair_cascade with one more level in front (half=False: without it,
    the cascade itself), and with the outcome PER TILE.
    -> model_pair_cascade's dict + half (tiles level 1 pruned), cycles (matrix cycles), and [n_tiles, n_waves] bool arrays
    tile_half / tile_filtered / tile_pruned, verdict [nJ] (-1 none, -2 exact scan, else the row).
    skip = "lane" / "key" (skip_loss's forms; None: the kernel before the skip): a tile that objects at level 1 and holds a finite f16
    key at or below thrS = thrF - L goes straight to the restart.  No older output depends on it but `cycles`; it adds skipped (such
    tiles), unsound (those of them the pair-norm filter would have pruned: must be 0), tile_skip [n_tiles, n_waves] and gap: the
    smallest distance of any finite key of level 1 or 2 from the threshold it is compared with (thrH, thrF, thrS) -- where that is well
    above the float32 roundings, the kernel decides every tile as this model does.
    prefix16 = True: the f16 prefix test in front of the restart (thrQ = thr + marginQ) on every tile that gets there.  No older output
    depends on it; it adds reach (tiles that reach the restart), prefix_pruned (those the restart's f32 prefix test prunes), prefix16
    (those the f16 test prunes), unsound16 (those of them the f32 prefix test keeps: must be 0), between (tiles the f32 test prunes and the
    f16 test lets through: they lie between thr and thrQ), cycles16 (matrix cycles with the level), tile_prefix16 [n_tiles, n_waves]
    and gap16, gap's like for the f16 prefix keys against thrQ."""
    R64 = float(np.float32(R))
    nI, nJ = a.shape[0], b.shape[0]
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        D = ((a64[:, None, :] - b64[None, :, :]) ** 2).sum(2) if nI * nJ <= 1 << 16 else \
            (a64 * a64).sum(1)[:, None] - 2.0 * a64 @ b64.T + (b64 * b64).sum(1)[None, :]
        ap, bp = a64[:, :8 * gp], b64[:, :8 * gp]
        DP = (ap * ap).sum(1)[:, None] - 2.0 * ap @ bp.T + (bp * bp).sum(1)[None, :]
        LB, slackF = pairnorm_bound(a, b)
        LBH, margin = halfnorm_bound(a, b)
        loss = skip_loss(a, b, LBH, skip) if (skip and half) else None
        DPQ, marginQ = prefix16_bound(a, b, gp) if prefix16 else (None, None)
    slackP = np.zeros(nJ) if _exact_pair(a, b) else slackF
    n_tiles = (nI + 31) // 32
    n_waves = (nJ + 63) // 64
    half_of_row = (np.arange(32) >> 2) & 1
    d0 = np.full((2, nJ), np.inf); d1 = np.full((2, nJ), np.inf)
    i0 = np.full((2, nJ), -1, np.int64); i1 = np.full((2, nJ), -1, np.int64)
    pl = np.full((2, nJ), np.inf)
    wave_of_q = np.arange(nJ) // 64
    tiles = pruned = filtered = halved = work = cycles = skipped = unsound = 0
    tile_skip = np.zeros((n_tiles, n_waves), bool); gap = np.inf
    reach = prefix_pruned = n_prefix16 = unsound16 = between = cycles16 = 0
    tile_prefix16 = np.zeros((n_tiles, n_waves), bool); gap16 = np.inf
    tile_half = np.zeros((n_tiles, n_waves), bool); tile_filtered = np.zeros((n_tiles, n_waves), bool); tile_pruned = np.zeros((n_tiles, n_waves), bool)
    for t in range(n_tiles):
        lo, hi = t * 32, min(nI, t * 32 + 32)
        rows = np.arange(lo, hi)
        with np.errstate(invalid="ignore"):
            e0, e1 = d0 + slackP, d1 + slackP
            re1 = R64 * e1
            T = np.where(e0 < re1, np.maximum(re1, e0 / R64), re1)
            T = T + np.abs(T) * 2.0 ** -21
        objH = np.zeros((2, nJ), bool); objF = np.zeros((2, nJ), bool); objP = np.zeros((2, nJ), bool); far = np.zeros((2, nJ), bool)
        objQ = np.zeros((2, nJ), bool)
        with np.errstate(invalid="ignore"):
            for h in (0, 1):
                m = half_of_row[: hi - lo] == h
                if m.any():
                    # (a NaN key objects: the comparisons are written as the kernel's)
                    objH[h] = ~(LBH[rows[m]] - (slackF + margin)[None, :] > T[h][None, :]).all(0)
                    objF[h] = ~(LB[rows[m]] - slackF[None, :] > T[h][None, :]).all(0)
                    objP[h] = ~(DP[rows[m]] - slackP[None, :] > T[h][None, :]).all(0)
                    if prefix16:
                        keysQ = DPQ[rows[m]] - (slackP + marginQ)[None, :]
                        objQ[h] = ~(keysQ > T[h][None, :]).all(0)
                        g = np.abs(keysQ - T[h][None, :])
                        gap16 = min(gap16, float(g[np.isfinite(g)].min(initial=np.inf)))
                    if loss is not None:
                        # kh_c <= thrS and kh_c > -inf (false for a NaN key); thrS = -inf while the threshold is +inf
                        Lm = loss[rows[m]] if loss.shape[0] > 1 else loss
                        far[h] = ((LBH[rows[m]] - slackF[None, :] + Lm <= T[h][None, :]) & (LBH[rows[m]] > -INF) & (T[h][None, :] < INF)).any(0)
                        for keys in (LBH[rows[m]] - (slackF + margin)[None, :], LB[rows[m]] - slackF[None, :], LBH[rows[m]] - slackF[None, :] + Lm):
                            g = np.abs(keys - T[h][None, :])
                            gap = min(gap, float(g[np.isfinite(g)].min(initial=np.inf)))
        wH = np.zeros(n_waves, bool); wF = np.zeros(n_waves, bool); wP = np.zeros(n_waves, bool); wS = np.zeros(n_waves, bool)
        np.logical_or.at(wS, wave_of_q, far[0] | far[1])
        np.logical_or.at(wH, wave_of_q, objH[0] | objH[1])
        np.logical_or.at(wF, wave_of_q, objF[0] | objF[1])
        np.logical_or.at(wP, wave_of_q, objP[0] | objP[1])
        if not half:
            wH[:] = True
        wave_on = wH & wF & wP
        wS &= wH                                                       # (only a tile that objects at level 1 gets as far as the skip)
        tile_skip[t] = wS
        skipped += int(wS.sum()); unsound += int((wS & ~wF).sum())
        tile_half[t] = ~wH; tile_filtered[t] = ~(wH & wF); tile_pruned[t] = ~wave_on
        tiles += n_waves
        halved += int((~wH).sum())
        filtered += int((~(wH & wF)).sum())
        pruned += int((~wave_on).sum())
        n2, n3p, n3 = int(wH.sum()), int((wH & wF & ~wP).sum()), int(wave_on.sum())
        work += 8 * n2 + gp * n3p + 16 * n3
        cycles += (CYC_HALF * n_waves if half else 0) + CYC_GROUP * (8 * (n2 - int(wS.sum())) + gp * n3p + 16 * n3)
        if prefix16:
            wQ = np.zeros(n_waves, bool)
            np.logical_or.at(wQ, wave_of_q, objQ[0] | objQ[1])
            at_restart = wH & wF
            tile_prefix16[t] = at_restart & ~wQ
            reach += int(at_restart.sum()); prefix_pruned += n3p
            n_prefix16 += int((at_restart & ~wQ).sum()); unsound16 += int((at_restart & ~wQ & wP).sum())
            between += int((at_restart & wQ & ~wP).sum())
            cycles16 += (CYC_HALF * n_waves if half else 0) + CYC_GROUP * 8 * (n2 - int(wS.sum())) + CYC_PREFIX16 * int(at_restart.sum()) + \
                CYC_GROUP * (gp * int((at_restart & wQ & ~wP).sum()) + 16 * int((at_restart & wQ & wP).sum()))
        go = wave_on[wave_of_q]
        pl[:, ~go] = np.minimum(pl[:, ~go], T[:, ~go])
        if go.any():
            q = np.flatnonzero(go)
            for h in (0, 1):
                m = half_of_row[: hi - lo] == h
                if m.any():
                    f0, f1, j0, j1 = d0[h, q], d1[h, q], i0[h, q], i1[h, q]
                    with np.errstate(invalid="ignore"):
                        _push(f0, j0, f1, j1, D[rows[m]][:, q], rows[m])
                    d0[h, q], d1[h, q], i0[h, q], i1[h, q] = f0, f1, j0, j1
    cd = np.concatenate([d0, d1]); ci = np.concatenate([i0, i1]).astype(np.float64)
    ci[ci < 0] = np.inf
    order = np.lexsort((ci, cd), axis=0)
    ea = np.take_along_axis(cd, order[:1], 0)[0]; eb = np.take_along_axis(cd, order[1:2], 0)[0]
    ia = np.take_along_axis(ci, order[:1], 0)[0]
    PL = pl.min(0)
    with np.errstate(invalid="ignore"):
        passes = ea < R64 * eb
        verdict = np.where(~passes, -1, np.where(ea < R64 * PL, ia, -2)).astype(np.int64)
        Dt = np.where(np.isnan(D), np.inf, D)                          # (a NaN distance is below nothing: the oracle never takes it)
        o = np.argsort(Dt, axis=0, kind="stable")[:2]
        t1 = np.take_along_axis(Dt, o[:1], 0)[0]; t2 = np.take_along_axis(Dt, o[1:2], 0)[0]
        truth = np.where(t1 < R64 * t2, o[0], -1)
    decided = verdict != -2
    extra = {"reach": reach, "prefix_pruned": prefix_pruned, "prefix16": n_prefix16, "unsound16": unsound16, "between": between,
             "cycles16": cycles16, "tile_prefix16": tile_prefix16, "gap16": gap16} if prefix16 else {}
    return {**extra, "tiles": tiles, "pruned": pruned, "filtered": filtered, "half": halved, "work": work, "cycles": cycles,
            "fallback": int((~decided).sum()), "wrong": int((decided & (verdict != truth)).sum()), "matches": int((truth >= 0).sum()),
            "queries": nJ, "skipped": skipped, "unsound": unsound, "tile_skip": tile_skip, "gap": gap, "tile_half": tile_half, "tile_filtered": tile_filtered, "tile_pruned": tile_pruned, "verdict": verdict}


def run_levels(views, pairs, gp, ratio, squared=True, out=print, skip=None, prefix16=False):
    """model_pair_levels with and without the f16 level on every pair: the shares per level, the matrix cycles of both, and whether
    any tile or verdict differs between them (it must not).  prefix16 (with skip): the f16 prefix test in front of
    the restart -- a third line per pair: tiles that reach the restart, tiles its f32 prefix test prunes, tiles the f16 test prunes, tiles
    the f16 test prunes and the f32 test keeps (must be 0), the matrix cycles a tile with and without it.  skip = "lane" / "key": with the skip of level 2 in that form of L (a
    second line per pair: the share of level 1's objecting tiles that skip, the cycles with it, the unsound skips -- must be 0)"""
    R = ratio * ratio if squared else ratio
    keys = ("tiles", "pruned", "filtered", "half", "cycles", "fallback", "wrong", "matches", "queries", "skipped", "unsound")
    acc = dict.fromkeys(keys, 0); acc["cycles_cascade"] = 0; acc["differs"] = 0; acc["cycles_skip"] = 0
    keys16 = ("reach", "prefix_pruned", "prefix16", "unsound16", "between", "cycles16")
    if prefix16:
        acc.update(dict.fromkeys(keys16, 0))
    qline = lambda r: (f"reach the restart {r['reach']}  pruned there by the f32 prefix test {r['prefix_pruned']}  pruned by the f16 prefix test "
                       f"{r['prefix16']} ({r['prefix16'] / max(r['prefix_pruned'], 1):.4f} of those)  let through between thr and thrQ {r['between']}  "
                       f"pruned by the f16 test and kept by the f32 test {r['unsound16']}  "
                       f"matrix cycles a tile {r['cycles16'] / r['tiles']:.0f} (without it {r['cycles_skip'] / r['tiles']:.0f})")
    sline = lambda r: (f"level 2 skipped on {r['skipped']} of {r['tiles'] - r['half']} objecting tiles ({r['skipped'] / max(r['tiles'] - r['half'], 1):.4f}; "
                       f"level 2 still runs on {(r['tiles'] - r['half'] - r['skipped']) / r['tiles']:.4f} of all, prunes {(r['filtered'] - r['half']) / r['tiles']:.4f})  "
                       f"matrix cycles a tile {r['cycles_skip'] / r['tiles']:.0f} (without the skip {r['cycles'] / r['tiles']:.0f})  "
                       f"tiles where the skip fired and the f32 filter would have pruned {r['unsound']}")
    line = lambda r: (f"level 1 {r['half'] / r['tiles']:.4f}  filter behind it {(r['filtered'] - r['half']) / r['tiles']:.4f}  "
                      f"prefix behind that {(r['pruned'] - r['filtered']) / r['tiles']:.4f}  "
                      f"matrix cycles a tile {r['cycles'] / r['tiles']:.0f} (cascade {r['cycles_cascade'] / r['tiles']:.0f}, brute force {16 * CYC_GROUP})")
    for (i, j) in pairs:
        r = model_pair_levels(views[i], views[j], gp, R)
        r0 = model_pair_levels(views[i], views[j], gp, R, half=False)
        r["cycles_cascade"] = r0["cycles"]; r["cycles_skip"] = r["cycles"]
        if skip:
            rs = model_pair_levels(views[i], views[j], gp, R, skip=skip, prefix16=prefix16)
            if prefix16:
                r.update({k: rs[k] for k in keys16})
            assert all(np.array_equal(rs[k], r[k]) for k in ("pruned", "filtered", "half", "tile_half", "tile_filtered", "tile_pruned", "verdict"))
            r["cycles_skip"] = rs["cycles"]; r["skipped"] = rs["skipped"]; r["unsound"] = rs["unsound"]
        r["differs"] = int((r["tile_filtered"] != r0["tile_filtered"]).sum() + (r["tile_pruned"] != r0["tile_pruned"]).sum() + (r["verdict"] != r0["verdict"]).sum())
        for k in acc:
            acc[k] += r[k]
        out(f"half + pairnorm + GP {gp:2d}  pair ({i},{j})  {line(r)}  matches {r['matches']:5d}  exact scan {r['fallback']:4d}  "
            f"wrong verdicts {r['wrong']}  tiles or verdicts unlike the cascade's {r['differs']}")
        if skip:
            out(f"skip of level 2 ({skip})  pair ({i},{j})  {sline(r)}")
        if prefix16:
            out(f"f16 prefix test  pair ({i},{j})  {qline(r)}")
    if skip:
        out(f"skip of level 2 ({skip})  ALL {len(pairs)} pairs, R = {R:.4f}: {sline(acc)}")
    if prefix16:
        out(f"f16 prefix test  ALL {len(pairs)} pairs, R = {R:.4f}: {qline(acc)}")
    out(f"half + pairnorm + GP {gp:2d}  ALL {len(pairs)} pairs, {acc['queries']} queries, R = {R:.4f}: {line(acc)}  "
        f"exact scan {acc['fallback']} ({acc['fallback'] / max(acc['queries'], 1):.2e})  wrong verdicts {acc['wrong']}  "
        f"tiles or verdicts unlike the cascade's {acc['differs']}")
    return acc


def run_cascade(views, pairs, gp, ratio, squared=True, out=print):
    R = ratio * ratio if squared else ratio
    keys = ("tiles", "pruned", "filtered", "work", "fallback", "wrong", "matches", "queries")
    acc = dict.fromkeys(keys, 0)
    line = lambda r: (f"filter {r['filtered'] / r['tiles']:.4f}  prefix behind it {(r['pruned'] - r['filtered']) / r['tiles']:.4f}  "
                      f"MFMA work left {r['work'] / (16 * r['tiles']):.4f}")
    for (i, j) in pairs:
        r = model_pair_cascade(views[i], views[j], gp, R)
        for k in keys:
            acc[k] += r[k]
        out(f"pairnorm + GP {gp:2d}  pair ({i},{j})  {line(r)}  matches {r['matches']:5d}  exact scan {r['fallback']:4d}  wrong verdicts {r['wrong']}")
    out(f"pairnorm + GP {gp:2d}  ALL {len(pairs)} pairs, {acc['queries']} queries, R = {R:.4f}: {line(acc)}  "
        f"exact scan {acc['fallback']} ({acc['fallback'] / max(acc['queries'], 1):.2e})  wrong verdicts {acc['wrong']}")
    return acc


def run(views, pairs, gps, ratio, squared=True, out=print):
    R = ratio * ratio if squared else ratio
    total = {}
    for gp in gps:
        acc = {"tiles": 0, "pruned": 0, "fallback": 0, "wrong": 0, "matches": 0, "queries": 0}
        for (i, j) in pairs:
            r = model_pair(views[i], views[j], gp, R)
            for k in acc:
                acc[k] += r[k]
            out(f"GP {gp:2d}  pair ({i},{j})  pruned {r['pruned'] / r['tiles']:.4f}  work left {1 - r['pruned'] / r['tiles'] * (16 - gp) / 16:.4f}  "
                f"matches {r['matches']:5d}  exact scan {r['fallback']:4d}  wrong verdicts {r['wrong']}")
        share = acc["pruned"] / max(acc["tiles"], 1)
        out(f"GP {gp:2d}  ALL {len(pairs)} pairs, {acc['queries']} queries, R = {R:.4f}: pruned {share:.4f}  MFMA work left {1 - share * (16 - gp) / 16:.4f}  "
            f"exact scan {acc['fallback']} ({acc['fallback'] / max(acc['queries'], 1):.2e})  wrong verdicts {acc['wrong']}")
        total[gp] = acc
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=14)
    ap.add_argument("--feat", type=int, default=8192)
    ap.add_argument("--seed", type=int, default=2002)
    ap.add_argument("--kind", default="sift")
    ap.add_argument("--gp", type=int, nargs="+", default=[9, 10, 11, 12])
    ap.add_argument("--ratio", type=float, nargs="+", default=[0.6])
    ap.add_argument("--pairs", type=int, default=0, help="pairs (0, 1 .. n); default: every other view")
    ap.add_argument("--filter", choices=["none", "pairnorm", "half"], default="none",
                    help="pairnorm: the cascade, the pair-norm filter in front of GP = --gp[-1]; half: the f16 level in front of the cascade")
    ap.add_argument("--skip", choices=["none", "lane", "key"], default="none",
                    help="with --filter half: the skip of level 2 with L lane-constant (the kernel's) or key-dependent")
    ap.add_argument("--prefix16", action="store_true",
                    help="with --filter half --skip lane: the f16 prefix test in front of the restart (r3dm_set_half_prefix)")
    ap.add_argument("--summary", action="store_true", help="with --filter pairnorm: only the ALL line")
    a = ap.parse_args()
    from regard3d_amd import synth
    descs, _, _ = synth.make_scene_torch(a.images, a.feat, seed=a.seed, device="cpu", kind=a.kind)
    views = [descs[i].numpy() for i in range(a.images)]
    pairs = [(0, j) for j in range(1, (a.pairs or a.images - 1) + 1)]
    bad = 0
    for ratio in a.ratio:
        if a.filter == "half":
            acc = run_levels(views, pairs, a.gp[-1], ratio, out=(lambda s: print(s) if " ALL " in s else None) if a.summary else print,
                             skip=None if a.skip == "none" else a.skip, prefix16=a.prefix16 and a.skip != "none")
            bad += acc["wrong"] + acc["differs"] + acc["unsound"] + acc.get("unsound16", 0)
            continue
        if a.filter == "pairnorm":
            bad += run_cascade(views, pairs, a.gp[-1], ratio, out=(lambda s: print(s) if " ALL " in s else None) if a.summary else print)["wrong"]
            continue
        tot = run(views, pairs, a.gp, ratio)
        bad += sum(v["wrong"] for v in tot.values())
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
