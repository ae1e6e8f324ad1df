"""An independent f64 audit of one AC-RANSAC-filtered pair, and the collection of views that all differ.

TEST INFRASTRUCTURE ONLY, plain numpy: nothing here calls the oracle or the library.  The filters are not symmetric in
their two views: I is normalised with s1 = 1/sqrt(wI hI), J with s2; logalpha0, the residual bound and the reported threshold use J's size
only; E takes pixel residuals through F = K_J^-T E K_I^-1.  `audit` re-derives what a filter reports from the PIXEL-space definitions --
deliberately not the normalised-space code path of the kernels and of oracle/acransac.c -- so that an I/J swap of a size or a K, a slot
taken for an id or a stale size shows whichever copy of the arithmetic makes it.

Residual e of every putative (s = 1/sqrt(w h)):
  F: e = (s2^2 dJ^2 + s1^2 dI^2) / 4, dJ / dI the pixel distances to the epipolar lines in J / in I under the returned pixel-space F
  H: e = s2^2 |x_J - hnormalized(H x_I)|^2
  E: e = (x_J^T F x_I)^2 / ((F x_I)_0^2 + (F x_I)_1^2), F = K_J^-T E K_I^-1 (one-sided, in pixels)
Checks (`audit` raises AuditError, an AssertionError, on the first that fails):
  1. the inliers are a prefix of the ascending order of e: max e[inliers] < min e[others], relative dead band 1e-9 (a putative inside
     the band is a badly chosen input, reported as such);
  2. threshold_px = sqrt(e_max) / s2 (F, H) or e_max itself (E), to 1e-9 relative;
  3. nfa = log10(MAXM (n - SS)) + (logalpha0 + mult log10(e_max + FLT_EPSILON)) (k - SS) + log10 C(n, k) + log10 C(k, SS) with logalpha0
     from J's D = sqrt(w^2 + h^2), A = w h: F log10(2 D / A / s2), mult 0.5; H log10(pi / A / s2^2), mult 1; E log10(2 D / A * 0.5), mult
     0.5 -- to `nfa_tolerance(n)`, the drift of the float log-combination tables that the kernel itself budgets for;
  4. e_max respects the bound precision^2 s2^2 (E: precision^2), and no k > SS under that bound has an audited NFA below the returned
     one by more than the same tolerance (near-ties inside the tables' noise are legitimate, so k itself is not compared).
"""
from __future__ import annotations

import numpy as np

FLT_EPSILON = float(np.finfo(np.float32).eps)
SS = {"F": 7, "E": 5, "H": 4}                # MINIMUM_SAMPLES
MAX_MODELS = {"F": 3, "E": 10, "H": 1}
DEAD_BAND = 1e-9
THRESHOLD_RTOL = 1e-9


class AuditError(AssertionError):
    pass


def nfa_tolerance(n: int) -> float:
    """2^-24 n (log10 C(n, n/2) + 32) + 1e-4: what n float additions of terms of that size can drift (about 0.08 at n = 2000)"""
    lf = _log10_factorials(n)
    h = n // 2
    return 2.0 ** -24 * n * (lf[n] - lf[h] - lf[n - h] + 32.0) + 1e-4


def _log10_factorials(n: int) -> np.ndarray:
    return np.concatenate([[0.0], np.cumsum(np.log10(np.arange(1, n + 1, dtype=np.float64)))])


def _hom(xy):
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    return np.c_[xy, np.ones(len(xy))]


def residuals(kind: str, model, xI, xJ, sizes, KI=None, KJ=None) -> np.ndarray:
    """e of every putative from the pixel-space definitions; sizes = (wI, hI, wJ, hJ)"""
    wI, hI, wJ, hJ = (float(v) for v in sizes)
    s1sq, s2sq = 1.0 / (wI * hI), 1.0 / (wJ * hJ)
    M = np.asarray(model, np.float64).reshape(3, 3)
    a, b = _hom(xI), _hom(xJ)
    with np.errstate(all="ignore"):
        if kind == "H":
            t = a @ M.T
            d = b[:, :2] - t[:, :2] / t[:, 2:3]
            return s2sq * np.sum(d * d, axis=1)
        if kind == "E":
            M = np.linalg.inv(np.asarray(KJ, np.float64).reshape(3, 3)).T @ M @ np.linalg.inv(np.asarray(KI, np.float64).reshape(3, 3))
        lJ = a @ M.T                            # F x_I: the epipolar line of x_I in J
        num = np.sum(b * lJ, axis=1) ** 2
        dJ2 = num / (lJ[:, 0] ** 2 + lJ[:, 1] ** 2)
        if kind == "E":
            return dJ2
        lI = b @ M                              # F^T x_J: the epipolar line of x_J in I
        dI2 = num / (lI[:, 0] ** 2 + lI[:, 1] ** 2)
        return (s2sq * dJ2 + s1sq * dI2) / 4.0


def logalpha0(kind: str, wJ, hJ) -> float:
    wJ, hJ = float(wJ), float(hJ)
    D, A = np.sqrt(wJ * wJ + hJ * hJ), wJ * hJ
    s2 = 1.0 / np.sqrt(A)
    return float(np.log10({"F": 2.0 * D / A / s2, "H": np.pi / A / (s2 * s2), "E": 2.0 * D / A * 0.5}[kind]))


def nfa_curve(kind: str, e_sorted: np.ndarray, wJ, hJ) -> np.ndarray:
    """NFA(k) for k = 0 .. n (entries k <= SS are +inf) of an ascending residual list"""
    n, ss = len(e_sorted), SS[kind]
    lf = _log10_factorials(n)
    k = np.arange(ss + 1, n + 1)
    mult = 1.0 if kind == "H" else 0.5
    with np.errstate(all="ignore"):
        la = logalpha0(kind, wJ, hJ) + mult * np.log10(e_sorted[k - 1] + FLT_EPSILON)
    v = np.log10(MAX_MODELS[kind] * float(n - ss)) + la * (k - ss) + (lf[n] - lf[k] - lf[n - k]) + (lf[k] - lf[ss] - lf[k - ss])
    return np.concatenate([np.full(ss + 1, np.inf), v])


def audit(kind: str, xI, xJ, sizes, precision_px: float, model, inliers, threshold_px: float, nfa: float, KI=None, KJ=None) -> dict:
    """-> the measured deviations {"threshold_rel", "nfa_abs", "gap_rel", "best_nfa_below", "n", "k"}; raises AuditError"""
    wI, hI, wJ, hJ = sizes
    e = residuals(kind, model, xI, xJ, sizes, KI, KJ)
    n, ss = len(e), SS[kind]
    inl = np.unique(np.asarray(inliers, np.int64))
    k = len(inl)
    if k != len(np.asarray(inliers).reshape(-1)) or k <= ss or k > n or inl[0] < 0 or inl[-1] >= n:
        raise AuditError(f"{kind}: {k} distinct inliers of {n} putatives")
    if not np.all(np.isfinite(e[inl])):
        raise AuditError(f"{kind}: an inlier has no finite residual")
    out = np.ones(n, bool); out[inl] = False
    e_max = float(e[inl].max())
    with np.errstate(invalid="ignore"):
        e_next = float(np.nanmin(np.where(np.isnan(e[out]), np.inf, e[out]))) if out.any() else np.inf
    gap = (e_next - e_max) / e_max if e_max > 0 else np.inf
    if not gap > -DEAD_BAND:
        raise AuditError(f"{kind}: the inliers are no prefix of the residual order: max inlier {e_max:.17g} >= min other {e_next:.17g}")
    if gap < DEAD_BAND:
        raise AuditError(f"{kind}: badly chosen input: a putative lies inside the dead band (gap {gap:.3g})")
    s2 = 1.0 / np.sqrt(float(wJ) * float(hJ))
    thr = e_max if kind == "E" else np.sqrt(e_max) / s2
    thr_rel = abs(float(threshold_px) - thr) / thr
    if not thr_rel <= THRESHOLD_RTOL:
        raise AuditError(f"{kind}: threshold {threshold_px:.17g} reported, {thr:.17g} audited (relative {thr_rel:.3g})")
    cap = float(precision_px) ** 2 * (1.0 if kind == "E" else s2 * s2)
    if not e_max <= cap * (1.0 + DEAD_BAND):
        raise AuditError(f"{kind}: e_max {e_max:.6g} above the bound {cap:.6g}")
    es = np.sort(np.where(np.isnan(e), np.inf, e))
    curve = nfa_curve(kind, es, wJ, hJ)
    tol = nfa_tolerance(n)
    nfa_abs = abs(float(nfa) - curve[k])
    if not nfa_abs <= tol:
        raise AuditError(f"{kind}: NFA {nfa:.9g} reported, {curve[k]:.9g} audited at k = {k} of {n} (tolerance {tol:.3g})")
    allowed = np.arange(n + 1) > ss
    allowed[1:] &= es <= cap * (1.0 - DEAD_BAND) if np.isfinite(cap) else np.isfinite(es)
    best = float(curve[allowed].min()) if allowed.any() else np.inf
    if best < float(nfa) - tol:
        raise AuditError(f"{kind}: k = {int(np.argmin(np.where(allowed, curve, np.inf)))} has NFA {best:.9g}, below the returned {nfa:.9g} "
                         f"(k = {k}) by more than {tol:.3g}")
    return dict(threshold_rel=thr_rel, nfa_abs=nfa_abs, gap_rel=gap, best_nfa_below=max(0.0, float(nfa) - best), n=n, k=k)


# ---- the collection of views that all differ -------------------------------------------------------------------------------------
SIZES = [(4000, 3000), (3000, 4000), (1920, 1080), (640, 480), (1000, 1000), (5472, 3648), (800, 1200)]
NO_K_VIEW = 4                                 # the 1000 x 1000 view has no intrinsics
N_CLOUD, N_PLANE = 3600, 2400
LONG_PAIR = 4200                              # the smallest list (> 4096) that reaches the cooperative kernel
# (view of I, view of J, putatives, share drawn from the planar patch): every ordered size relation -- larger -> smaller, smaller ->
# larger, landscape <-> portrait of equal and of different area, square -- in both id orders
PAIR_SPEC = [(0, 3, 1500, 0.4), (3, 0, 1200, 0.7), (1, 0, 1000, 0.4), (0, 1, 800, 0.7), (5, 6, 600, 0.4), (6, 5, 500, 0.7),
             (2, 6, 400, 0.4), (6, 2, 300, 0.7), (3, 5, 250, 0.4), (4, 2, 150, 0.7), (1, 4, 100, 0.4), (2, 3, 60, 0.7), (6, 3, 40, 0.7),
             (5, 2, LONG_PAIR, 0.4)]


def intrinsics(v: int) -> np.ndarray:
    """the pinhole matrix of view v: its own focal length, a principal point tens of pixels off centre; view 2 has fx != fy, view 5 a
    small skew term"""
    w, h = SIZES[v]
    f = 1.1 * min(w, h) * (1.0 + 0.04 * v)
    K = np.array([[f, 0.0, w / 2.0 + 11.0 * (v + 1)], [0.0, f, h / 2.0 - 7.0 * (v + 2)], [0.0, 0.0, 1.0]])
    if v == 2:
        K[1, 1] = 1.03 * f
    if v == 5:
        K[0, 1] = 2.5
    return K


class Collection:
    """views: per view id {"w", "h", "K" (None: no intrinsics), "xy" [n, 2] float32}; pairs [P, 2] (ids, ascending (I, J)), counts [P],
    offsets [P + 1], matches [M, 2]"""

    def __init__(self, views, pairs, counts, matches):
        self.views, self.pairs, self.counts, self.matches = views, pairs, counts, matches
        self.offsets = np.r_[0, np.cumsum(counts)].astype(np.uint64)

    def putatives(self, p: int):
        """-> (I, J, matches [m, 2], xI [m, 2] f64, xJ [m, 2] f64) of pair row p"""
        I, J = (int(v) for v in self.pairs[p])
        mm = self.matches[int(self.offsets[p]):int(self.offsets[p + 1])]
        return I, J, mm, self.views[I]["xy"][mm[:, 0]].astype(np.float64), self.views[J]["xy"][mm[:, 1]].astype(np.float64)

    def sizes(self, p: int):
        I, J = (int(v) for v in self.pairs[p])
        return self.views[I]["w"], self.views[I]["h"], self.views[J]["w"], self.views[J]["h"]

    def dense(self):
        """(xys, widths, heights, Ks) indexed by view id up to the largest, ids without a view empty, a missing K all zero: the arrays
        that the oracle's collection entries take"""
        n = max(self.views) + 1
        xys = [self.views[i]["xy"] if i in self.views else np.zeros((0, 2), np.float32) for i in range(n)]
        W = np.array([self.views[i]["w"] if i in self.views else 0 for i in range(n)], np.uint32)
        H = np.array([self.views[i]["h"] if i in self.views else 0 for i in range(n)], np.uint32)
        Ks = np.zeros((n, 3, 3))
        for i, v in self.views.items():
            if v["K"] is not None:
                Ks[i] = v["K"]
        return xys, W, H, Ks

    def subset(self, rows):
        rows = np.asarray(rows, np.int64)
        m = [self.matches[int(self.offsets[p]):int(self.offsets[p + 1])] for p in rows]
        return Collection(self.views, self.pairs[rows], self.counts[rows], np.concatenate(m) if m else np.zeros((0, 2), np.uint32))


def project(v: int, X: np.ndarray, size=None, K=None) -> np.ndarray:
    """pixel positions (f64) of the points X in the camera of view v"""
    th, ph = 0.03 * v - 0.09, 0.015 * (v % 3) - 0.015
    Ry = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(ph), -np.sin(ph)], [0, np.sin(ph), np.cos(ph)]])
    Y = X @ (Rx @ Ry).T + np.array([0.45 * v - 1.3, 0.08 * v - 0.2, 0.06 * v])
    K = intrinsics(v) if K is None else K
    p = Y @ K.T
    return p[:, :2] / p[:, 2:3]


def make_points(seed: int = 77, n_cloud: int = N_CLOUD, n_plane: int = N_PLANE) -> np.ndarray:
    """a rigid cloud followed by a planar patch, so that F, E and H all have support"""
    rng = np.random.default_rng(seed)
    cloud = np.c_[rng.uniform(-3, 3, n_cloud), rng.uniform(-3, 3, n_cloud), rng.uniform(8, 14, n_cloud)]
    px, py = rng.uniform(-3, 3, n_plane), rng.uniform(-3, 3, n_plane)
    return np.r_[cloud, np.c_[px, py, 11.0 + 0.15 * px - 0.1 * py]]


def make_collection(ids=None, seed: int = 77, spec=None, no_K=(NO_K_VIEW,), n_cloud: int = N_CLOUD, n_plane: int = N_PLANE) -> Collection:
    """The asymmetric collection: 7 views of one scene, each with its own size and K (one without), feature k of every view = point k
    + 0.4 px noise; hand-made putative lists, ~30 % of them pointing at a random other feature.  ids[v] is the view id of view v
    (default v); the pairs come out in ascending (I, J) of the ids.  spec / n_cloud / n_plane: another pair list on a smaller scene."""
    ids = list(range(len(SIZES))) if ids is None else [int(i) for i in ids]
    rng = np.random.default_rng(seed)
    X = make_points(seed + 1, n_cloud, n_plane)
    n = len(X)
    views = {}
    for v, (w, h) in enumerate(SIZES):
        xy = project(v, X) + rng.normal(0, 0.4, (n, 2))
        views[ids[v]] = dict(w=w, h=h, K=None if v in no_K else intrinsics(v), xy=xy.astype(np.float32))
    rows = []
    for a, b, m, plane in (PAIR_SPEC if spec is None else spec):
        mp = int(round(m * plane))
        ii = np.sort(np.r_[rng.permutation(n_cloud)[:m - mp], n_cloud + rng.permutation(n_plane)[:mp]])
        jj = ii.copy()
        wrong = rng.random(m) < 0.3
        jj[wrong] = rng.integers(0, n, int(wrong.sum()))
        rows.append(((ids[a], ids[b]), np.c_[ii, jj].astype(np.uint32)))
    rows.sort(key=lambda r: r[0])
    assert len({r[0] for r in rows}) == len(rows)
    return Collection(views, np.array([r[0] for r in rows], np.uint32), np.array([len(r[1]) for r in rows], np.uint32),
                      np.concatenate([r[1] for r in rows]))
