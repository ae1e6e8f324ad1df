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
Distances are exact here (integer-valued rows: float32 sums below 2^24), as the kernel's are for such pairs."""
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
    a = ap.parse_args()
    from regard3d_amd import synth
    descs, _, _ = synth.make_scene_torch(a.images, a.feat, seed=a.seed, device="cpu", kind=a.kind)
    views = [descs[i].numpy() for i in range(a.images)]
    pairs = [(0, j) for j in range(1, (a.pairs or a.images - 1) + 1)]
    bad = 0
    for ratio in a.ratio:
        tot = run(views, pairs, a.gp, ratio)
        bad += sum(v["wrong"] for v in tot.values())
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
