"""CPU restatement of guided matching (OpenMVG's bGuided_matching = true; DESIGN.md section 2, "Guided matching").

TEST INFRASTRUCTURE ONLY, like oracle/pyoracle.py: the GPU tests compare r3dm_guided_match and the filters with the switch on against
this module.  The per-candidate arithmetic is the oracle library's own: orc_epipolar_dist_err / orc_h_asym_err decide the geometric gate,
orc_f_from_e and orc_inv3 form E's fundamental matrix, orc_l2sq_f32 / orc_l2sq_u8 / orc_hamming give the descriptor distances and
orc_acransac_F / _E / _H the models and thresholds of the filters.  numpy only narrows the candidates first: its f64 element-wise
arithmetic is the oracle's operation for operation (no contraction), and a relative margin of 1e-9 keeps every candidate the oracle
could accept; the oracle then decides each one.

Rules:
  1. only pairs the filter accepted are re-matched; an empty guided list does not enter the graph; E's overlap rule applies to the
     guided list; models and thresholds stay AC-RANSAC's.
  2. the queries are all features of I, the candidates all features of J; output (i, j) ascending in i, at most one per i.
  3. errTh = threshold_px ** 2 for every kind; a candidate passes iff err < errTh.
  4. ratio >= 0: distanceRatio over the candidates in ascending j; emit iff two candidates were seen and
     float(bd) < ratio ** 2 * float(sbd) (double arithmetic).
  5. ratio < 0: the j of smallest error, the first on ties; H then drops matches whose (xI, yI, xJ, yJ) repeat an earlier one.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
U32_MAX = 0xFFFFFFFF


def _lib():
    from oracle import pyoracle as O
    L = O.lib()
    L.orc_h_asym_err.restype = C.c_double
    L.orc_h_asym_err.argtypes = [C.c_void_p] + [C.c_double] * 4
    L.orc_f_from_e.restype = None
    L.orc_f_from_e.argtypes = [C.c_void_p] * 4
    L.orc_inv3.restype = None
    L.orc_inv3.argtypes = [C.c_void_p] * 2
    L.orc_l2sq_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.orc_l2sq_u8.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.orc_hamming.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def inv3(K) -> np.ndarray:
    K = np.ascontiguousarray(K, np.float64).reshape(9)
    out = np.zeros(9, np.float64)
    _lib().orc_inv3(_p(K), _p(out))
    return out


def f_from_e(E, KI, KJ) -> np.ndarray:
    """F = K_J^-T E K_I^-1 from the views' pinhole matrices (orc_inv3 + orc_f_from_e)"""
    E = np.ascontiguousarray(E, np.float64).reshape(9)
    out = np.zeros(9, np.float64)
    _lib().orc_f_from_e(_p(E), _p(inv3(KI)), _p(inv3(KJ)), _p(out))
    return out


def geometric_error(kind: str, M, x1, y1, x2, y2) -> float:
    """the oracle's error of one (i, j): EpipolarDistanceError (F, and E through f_from_e) or the homography's AsymmetricError"""
    M = np.ascontiguousarray(M, np.float64).reshape(9)
    L = _lib()
    if kind == "H":
        return float(L.orc_h_asym_err(_p(M), float(x1), float(y1), float(x2), float(y2)))
    return float(L.orc_epipolar_dist_err(_p(M), float(x1), float(y1), float(x2), float(y2)))


def _errors(kind, M, xyI_rows, xJ, yJ):
    """numpy form of the same errors for a block of queries (rows) against all of J, in the oracle's operation order"""
    x1 = xyI_rows[:, 0:1].astype(np.float64); y1 = xyI_rows[:, 1:2].astype(np.float64)
    with np.errstate(all="ignore"):
        if kind == "H":
            w = M[6] * x1 + M[7] * y1 + M[8]
            ex = xJ - (M[0] * x1 + M[1] * y1 + M[2]) / w
            ey = yJ - (M[3] * x1 + M[4] * y1 + M[5]) / w
            return ex * ex + ey * ey
        l0 = M[0] * x1 + M[1] * y1 + M[2]
        l1 = M[3] * x1 + M[4] * y1 + M[5]
        l2 = M[6] * x1 + M[7] * y1 + M[8]
        d = l0 * xJ + l1 * yJ + l2
        return (d * d) / (l0 * l0 + l1 * l1)


def candidates(kind, M, xyI, xyJ, errTh):
    """per query i: (ascending candidate rows j, their errors) -- err < errTh decided by the oracle's error function"""
    xyI = np.ascontiguousarray(xyI, np.float32).reshape(-1, 2); xyJ = np.ascontiguousarray(xyJ, np.float32).reshape(-1, 2)
    M = np.ascontiguousarray(M, np.float64).reshape(9)
    xJ = xyJ[:, 0].astype(np.float64)[None, :]; yJ = xyJ[:, 1].astype(np.float64)[None, :]
    out = []
    loose = errTh * (1.0 + 1e-9) + 1e-300 if np.isfinite(errTh) else errTh
    for b in range(0, xyI.shape[0], 256):
        e = _errors(kind, M, xyI[b:b + 256], xJ, yJ)
        with np.errstate(invalid="ignore"):
            maybe = (e < loose) if np.isfinite(loose) else ~np.isnan(e)
        for r in range(e.shape[0]):
            i = b + r
            js, errs = [], []
            for j in np.nonzero(maybe[r])[0]:
                err = geometric_error(kind, M, xyI[i, 0], xyI[i, 1], xyJ[j, 0], xyJ[j, 1])
                if err < errTh:
                    js.append(int(j)); errs.append(err)
            out.append((js, errs))
    return out


def candidate_count(kind: str, M, thr_px: float, xyI, xyJ, KI=None, KJ=None) -> int:
    """the number of (i, j) of one pair with err < errTh, as candidates() decides them: what r3dm_guided_report's n_candidates sums
    over the pairs of a call, in either mode.  kind, M, thr_px, KI / KJ as guided_pair takes them."""
    Fm = f_from_e(M, KI, KJ) if kind == "E" else np.ascontiguousarray(M, np.float64).reshape(9)
    errTh = float(thr_px) * float(thr_px)
    return sum(len(js) for js, _ in candidates("H" if kind == "H" else "F", Fm, xyI, xyJ, errTh))


def descriptor_distance(a: np.ndarray, b: np.ndarray, binary: bool):
    """SquaredDescriptorDistance: the oracle's squared L2 (f32 / u8 rows) or Hamming distance (binary rows)"""
    L = _lib()
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    if binary:
        return int(L.orc_hamming(_p(a), _p(b), a.size))
    if a.dtype == np.uint8:
        return float(L.orc_l2sq_u8(_p(a), _p(b), a.size))
    return float(L.orc_l2sq_f32(_p(a), _p(b), a.size))


def ratio_pick(dists, js, ratio: float, binary: bool):
    """OpenMVG's distanceRatio over the candidates in ascending j -> the chosen j or None"""
    top = U32_MAX if binary else FLT_MAX
    bd = sbd = top
    idx = None
    for d, j in zip(dists, js):
        if d < bd:
            sbd = bd; bd = d; idx = j
        elif d < sbd:
            sbd = d
    R = ratio * ratio
    if sbd != top and float(bd) < R * float(sbd):
        return idx
    return None


def coordinate_dedup(m: np.ndarray, xyI, xyJ) -> np.ndarray:
    """IndMatchDecorator: keep the first (smallest (i, j)) of every group of equal (xI, yI, xJ, yJ) (float ==)"""
    seen = []
    keep = []
    for k, (i, j) in enumerate(m.tolist()):
        key = (float(xyI[i][0]), float(xyI[i][1]), float(xyJ[j][0]), float(xyJ[j][1]))
        if any(key == s for s in seen):
            continue
        seen.append(key)
        keep.append(k)
    return m[keep]


def guided_pair(kind: str, M, thr_px: float, ratio: float, xyI, xyJ, descI=None, descJ=None, binary: bool = False, KI=None, KJ=None):
    """the guided list of one pair -> (m, 2) uint32 array of (i, j).  kind "F" / "E" / "H"; M as the filter returns it (E: the essential
    matrix, KI / KJ the views' pinhole matrices); thr_px as r3dm_pair_report.threshold_px; ratio < 0: geometry only."""
    xyI = np.ascontiguousarray(xyI, np.float32).reshape(-1, 2); xyJ = np.ascontiguousarray(xyJ, np.float32).reshape(-1, 2)
    Fm = f_from_e(M, KI, KJ) if kind == "E" else np.ascontiguousarray(M, np.float64).reshape(9)
    gk = "H" if kind == "H" else "F"
    errTh = float(thr_px) * float(thr_px)
    rows = []
    for i, (js, errs) in enumerate(candidates(gk, Fm, xyI, xyJ, errTh)):
        if ratio < 0:
            best, bj = np.finfo(np.float64).max, None
            for j, e in zip(js, errs):
                if e < errTh and e < best:
                    best, bj = e, j
            if bj is not None:
                rows.append((i, bj))
        else:
            if len(js) < 2:
                continue
            d = [descriptor_distance(descI[i], descJ[j], binary) for j in js]
            j = ratio_pick(d, js, ratio, binary)
            if j is not None:
                rows.append((i, j))
    m = np.array(rows, np.uint32).reshape(-1, 2)
    if ratio < 0 and kind == "H" and m.shape[0] > 1:
        m = coordinate_dedup(m, xyI, xyJ)
    return m


def guided_filter(kind: str, descs, xys, widths, heights, pairs, offsets, matches, ratio: float, Ks=None, binary: bool = False,
                  precision_px: float = 4.0, max_iter: int = 2048, seed: int = 5489, min_count: int = 50, min_ratio: float = 0.3):
    """a filter with the guided switch on: orc_acransac_* per putative pair, guided_pair on the accepted ones, E's overlap rule on the
    guided list, no empty entries -> (pairs, offsets, matches, models) in the graph's order"""
    from oracle import pyoracle as O
    SS = {"F": 7, "E": 5, "H": 4}[kind]
    out_p, out_m, out_o, models = [], [], [0], []
    for p, (I, J) in enumerate(np.asarray(pairs).tolist()):
        mm = np.asarray(matches[int(offsets[p]):int(offsets[p + 1])], np.uint32)
        if mm.shape[0] <= SS:
            continue
        if kind == "E" and (Ks is None or Ks[I] is None or Ks[J] is None):
            continue
        xI = xys[I][mm[:, 0]].astype(np.float64); xJ = xys[J][mm[:, 1]].astype(np.float64)
        if kind == "F":
            inl, fr = O.acransac_F(xI, xJ, int(widths[I]), int(heights[I]), int(widths[J]), int(heights[J]), precision_px, max_iter, seed, I, J)
        elif kind == "H":
            inl, fr = O.acransac_H(xI, xJ, int(widths[I]), int(heights[I]), int(widths[J]), int(heights[J]), precision_px, max_iter, seed, I, J)
        else:
            inl, fr = O.acransac_E(xI, xJ, int(widths[I]), int(heights[I]), int(widths[J]), int(heights[J]), Ks[I], Ks[J], precision_px,
                                   max_iter, seed, I, J)
        if not len(inl) > 2.5 * SS:
            continue
        M = np.array(list(fr.F), np.float64)
        g = guided_pair(kind, M, fr.threshold, ratio, xys[I], xys[J], None if descs is None else descs[I], None if descs is None else descs[J],
                        binary, None if Ks is None else Ks[I], None if Ks is None else Ks[J])
        n = g.shape[0]
        if kind == "E" and (n < min_count or np.float32(n) / np.float32(mm.shape[0]) < np.float32(min_ratio)):
            continue
        if n == 0:
            continue
        out_p.append((I, J)); out_m.append(g); out_o.append(out_o[-1] + n); models.append(M)
    return (np.array(out_p, np.uint32).reshape(-1, 2), np.array(out_o, np.uint64),
            np.concatenate(out_m).astype(np.uint32) if out_m else np.zeros((0, 2), np.uint32),
            np.array(models, np.float64).reshape(-1, 9))
