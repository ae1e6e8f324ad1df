"""Guided matching at the edges of its kernels (kernels_guided.hip): the case table of test_guided_cases.py (CPU: every case reaches
the edge it is named for, on the restatement alone) and test_gpu_guided_edges.py (GPU: r3dm_guided_match == guided_restatement).

TEST INFRASTRUCTURE ONLY.  A case is one pair of views with a caller-chosen model and threshold:

    dict(name, family, kind "F" | "H" | "E", M [9] f64, thr_px, ratio (< 0: geometry only), xyI, xyJ, descI, descJ, binary, KI, KJ,
         ratios (every mode the GPU test runs the case in), aux (what the proof reads), proof)

proof(case, cand, gate) asserts the edge on the restatement's candidate lists cand = guided_restatement.candidates(..) and on
gate = gate_model(..) with the kernel's constants; it returns the counts it measured.

gate_model restates the sweep's f32 gate from the header comment of kernels_guided.hip, operation for operation in numpy f32 (numpy
never contracts a product and a sum): the query's line or transfer in f64, its three coefficients rounded to f32, the per-tile Xmax /
Ymax of J's positions, lim, and the rule that sends a whole tile to the f64 test (exact_all).  What it returns is which (i, j) REACH the
f64 test; the kernel is right iff that set holds every (i, j) the restatement accepts.  (The NaN positions that pad a tile to a multiple
of four are no (i, j): the model has nothing to say about them; the shapes family runs J of 1 .. 5 and 4095 .. 4097 positions.)

Families: equality (err == errTh, thr 0, thr inf), slack (candidates within a few % of the threshold where the f32 rounding of the gate
is as large as the threshold), domain (tiles and queries outside the gate's argument), ties (first j, distanceRatio's updates, the
ratio test in double), shapes (query blocks and J tiles), dedup (IndMatchDecorator under H, geometry only)."""
from __future__ import annotations

import zlib

import numpy as np

import guided_restatement as G

# the kernel's constants (test_guided_cases.py holds them to the text of kernels_guided.hip and r3dm_internal.hpp)
GATE_REL = 2.0 ** -20
GATE_ABS = 1e-30
COEF_LIMIT = 1e30
POS_LIMIT = 1e7
TILE = 4096
BLOCK = 256                      # queries per workgroup

F32 = np.float32
_TINY = np.finfo(np.float32).tiny


# ---------------------------------------------------------------------------------------------------------------- the gate's model
def _lines(kind, M, xyI):
    """the query's line (F) or transfer (H) in f64, in the kernel's (= the oracle's) operation order -> a0, a1, a2, den, T(errTh)"""
    x1 = xyI[:, 0].astype(np.float64); y1 = xyI[:, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        if kind == "H":
            w = M[6] * x1 + M[7] * y1 + M[8]
            return (M[0] * x1 + M[1] * y1 + M[2]) / w, (M[3] * x1 + M[4] * y1 + M[5]) / w, np.zeros_like(x1), None
        a0 = M[0] * x1 + M[1] * y1 + M[2]
        a1 = M[3] * x1 + M[4] * y1 + M[5]
        a2 = M[6] * x1 + M[7] * y1 + M[8]
        return a0, a1, a2, a0 * a0 + a1 * a1


def gate_model(kind, M, xyI, xyJ, errTh, rel=GATE_REL, abs_=GATE_ABS, tile=TILE, ftz=False):
    """-> bool [nI, nJ]: the (i, j) the sweep hands to its f64 test.  kind "F" (E after f_from_e) or "H"; rel / abs_: kGateRel /
    kGateAbs (0, 0: the gate without its slack); tile: kGuidedTile; ftz: every f32 result below the smallest normal is flushed to
    zero (the header comment's "flushed denormals"; numpy keeps them)."""
    xyI = np.ascontiguousarray(xyI, F32).reshape(-1, 2); xyJ = np.ascontiguousarray(xyJ, F32).reshape(-1, 2)
    M = np.ascontiguousarray(M, np.float64).reshape(9)
    nI, nJ = xyI.shape[0], xyJ.shape[0]
    rel32, abs32 = F32(rel), F32(abs_)

    def z(v):
        return np.where(np.abs(v) < _TINY, F32(0), v).astype(F32) if ftz else v

    with np.errstate(all="ignore"):
        a0, a1, a2, den = _lines(kind, M, xyI)
        if kind == "H":
            T = np.full(nI, np.sqrt(np.float64(errTh)))
            ok = (np.abs(a0) < COEF_LIMIT) & (np.abs(a1) < COEF_LIMIT) & (T < COEF_LIMIT)
        else:
            T = np.sqrt(np.float64(errTh) * den)
            ok = (np.abs(a0) < COEF_LIMIT) & (np.abs(a1) < COEF_LIMIT) & (np.abs(a2) < COEF_LIMIT) & (T < COEF_LIMIT)
        f0 = z(np.where(ok, a0, 0.0).astype(F32)); f1 = z(np.where(ok, a1, 0.0).astype(F32)); f2 = z(np.where(ok, a2, 0.0).astype(F32))
        T32 = z(z(np.where(ok, T, 0.0).astype(F32)) * (F32(1) + rel32))
        out = np.zeros((nI, nJ), bool)
        for t0 in range(0, nJ, tile):
            xs = z(xyJ[t0:t0 + tile, 0]); ys = z(xyJ[t0:t0 + tile, 1])
            Xm = F32(np.fmax.reduce(np.abs(xs), initial=F32(0))); Ym = F32(np.fmax.reduce(np.abs(ys), initial=F32(0)))     # (fmax drops NaN)
            exact_all = ~(ok & bool(Xm < F32(POS_LIMIT)) & bool(Ym < F32(POS_LIMIT)))
            if kind == "H":
                limx = z(z(T32 + z(z(np.abs(f0) + Xm) * rel32)) + abs32)
                limy = z(z(T32 + z(z(np.abs(f1) + Ym) * rel32)) + abs32)
                p = (np.abs(z(xs[None, :] - f0[:, None])) <= limx[:, None]) & (np.abs(z(ys[None, :] - f1[:, None])) <= limy[:, None])
            else:
                s = z(z(z(np.abs(f0) * Xm) + z(np.abs(f1) * Ym)) + np.abs(f2))
                lim = z(z(T32 + z(s * rel32)) + abs32)
                d = z(z(z(f0[:, None] * xs[None, :]) + z(f1[:, None] * ys[None, :])) + f2[:, None])
                p = np.abs(d) <= lim[:, None]
            out[:, t0:t0 + tile] = p | exact_all[:, None]
    return out


def exact_all_tiles(kind, M, xyI, xyJ, errTh, tile=TILE):
    """-> bool [nI, n_tiles]: the (query, tile) the kernel serves without the gate"""
    xyI = np.ascontiguousarray(xyI, F32).reshape(-1, 2); xyJ = np.ascontiguousarray(xyJ, F32).reshape(-1, 2)
    # a position no finite gate would pass at errTh: only exact_all lets it through
    far = gate_model(kind, M, xyI, np.full((1, 2), np.nan, F32), errTh)[:, 0]
    out = []
    for t0 in range(0, xyJ.shape[0], tile):
        a = np.abs(xyJ[t0:t0 + tile])
        big = not (np.fmax.reduce(a[:, 0], initial=F32(0)) < F32(POS_LIMIT) and np.fmax.reduce(a[:, 1], initial=F32(0)) < F32(POS_LIMIT))
        out.append(far | big)
    return np.stack(out, axis=1) if out else np.zeros((xyI.shape[0], 0), bool)


# ---------------------------------------------------------------------------------------------------------------- helpers
def model_of(case):
    """(kind of the error function, the [9] matrix it takes): E goes through f_from_e"""
    if case["kind"] == "E":
        return "F", G.f_from_e(case["M"], case["KI"], case["KJ"])
    return case["kind"], np.ascontiguousarray(case["M"], np.float64).reshape(9)


def err_th(case) -> float:
    return float(case["thr_px"]) * float(case["thr_px"])


def candidates_of(case):
    k, M = model_of(case)
    return G.candidates(k, M, case["xyI"], case["xyJ"], err_th(case))


def candidate_mask(case, cand) -> np.ndarray:
    m = np.zeros((len(case["xyI"]), len(case["xyJ"])), bool)
    for i, (js, _) in enumerate(cand):
        m[i, js] = True
    return m


def gate_of(case, **kw):
    k, M = model_of(case)
    return gate_model(k, M, case["xyI"], case["xyJ"], err_th(case), **kw)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _default_descs(name, nI, nJ):
    """descriptor rows for a case that is about the geometry: small integers, so that every distance is exact in every arithmetic"""
    r = _rng("desc:" + name)
    return r.integers(0, 6, (nI, 8)).astype(F32), r.integers(0, 6, (nJ, 8)).astype(F32)


CASES = []


def _add(name, family, kind, M, thr_px, ratio, xyI, xyJ, proof, descI=None, descJ=None, binary=False, KI=None, KJ=None, ratios=None,
         aux=None):
    xyI = np.ascontiguousarray(xyI, F32).reshape(-1, 2); xyJ = np.ascontiguousarray(xyJ, F32).reshape(-1, 2)
    if descI is None:
        descI, descJ = _default_descs(name, len(xyI), len(xyJ))
    if ratios is None:
        ratios = (ratio, 0.8 if ratio < 0 else -1.0)
    assert len(descI) == len(xyI) and len(descJ) == len(xyJ) and not any(c["name"] == name for c in CASES), name
    CASES.append(dict(name=name, family=family, kind=kind, M=np.array(M, np.float64).reshape(9), thr_px=float(thr_px), ratio=float(ratio),
                      xyI=xyI, xyJ=xyJ, descI=np.ascontiguousarray(descI), descJ=np.ascontiguousarray(descJ), binary=binary, KI=KI, KJ=KJ,
                      ratios=tuple(float(r) for r in ratios), aux=aux or {}, proof=proof))


def skew(t):
    """F = [t]x: the line of (x, y) passes through (x, y) itself and the epipole t"""
    tx, ty, tz = t
    return np.array([0, -tz, ty, tz, 0, -tx, -ty, tx, 0], np.float64)


F_Y = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], np.float64)              # l = (0, -1, y1): err = (y1 - y2)^2, exact on integers


def _err(case, i, j):
    k, M = model_of(case)
    return G.geometric_error(k, M, case["xyI"][i, 0], case["xyI"][i, 1], case["xyJ"][j, 0], case["xyJ"][j, 1])


def _fill_far(n, r, lo=1e5, hi=2e5):
    """positions no query of the small cases comes near"""
    return r.uniform(lo, hi, (n, 2)).astype(F32)


# ---------------------------------------------------------------------------------------------------------------- equality
def _equality_views(kind):
    """40 queries on an integer lattice; per query i four planted candidates in J: err 25, 25, 16 (every third query) or 32, and 0 (every
    fourth) or 36 -- (3, 4), (5, 0) from the transfer under H; 5, -5 rows from the line under F -- and one NaN position"""
    n = 40
    xyI = np.stack([37.0 + 11.0 * np.arange(n), 100.0 * (1 + np.arange(n))], axis=1)
    rows, planted = [], []
    for i in range(n):
        x, y = xyI[i]
        if kind == "H":
            tx, ty = x + 7.0, y - 2.0
            offs = [(3, 4), (5, 0), (0, 4) if i % 3 == 0 else (4, 4), (0, 0) if i % 4 == 0 else (0, 6)]
            pts = [(tx + a, ty + b) for a, b in offs]
            errs = [a * a + b * b for a, b in offs]
        else:
            dys = [5, -5, 4 if i % 3 == 0 else 7, 0 if i % 4 == 0 else 6]
            pts = [(500.0 + 3 * k + i, y + d) for k, d in enumerate(dys)]
            errs = [d * d for d in dys]
        for p, e in zip(pts, errs):
            planted.append((i, len(rows), float(e))); rows.append(p)
    rows.append((np.nan, 50.0))
    M = np.array([1, 0, 7, 0, 1, -2, 0, 0, 1], np.float64) if kind == "H" else F_Y
    return M, xyI, np.array(rows), planted


def _proof_equality(case, cand, gate):
    mask = candidate_mask(case, cand)
    errTh = err_th(case)
    planted = case["aux"]["planted"]
    for i, j, e in planted:
        assert _err(case, i, j) == e, (i, j, e)                    # the planted errors are exact
    at = [(i, j) for i, j, e in planted if e == 25.0]
    below = [(i, j) for i, j, e in planted if e < 25.0]
    what = case["aux"]["what"]
    if what == "at":
        assert errTh == 25.0 and at and not any(mask[i, j] for i, j in at) and all(mask[i, j] for i, j in below)
        assert mask.sum() == len(below)
    elif what == "next":
        assert errTh > 25.0 and np.nextafter(case["thr_px"], 0.0) == 5.0
        assert all(mask[i, j] for i, j in at) and mask.sum() == len(at) + len(below)
    elif what == "zero":
        assert errTh == 0.0 and any(e == 0.0 for _, _, e in planted) and mask.sum() == 0
    else:
        assert np.isinf(errTh) and len(case["xyI"]) <= 200 and len(case["xyJ"]) <= 200
        k, M = model_of(case)
        e = G._errors(k, M, case["xyI"], case["xyJ"][:, 0].astype(np.float64)[None, :], case["xyJ"][:, 1].astype(np.float64)[None, :])
        assert np.array_equal(mask, np.isfinite(e)) and 0 < mask.sum() < mask.size
        assert exact_all_tiles(k, M, case["xyI"], case["xyJ"], errTh).all()          # T < 1e30 fails: no gate
    return dict(candidates=int(mask.sum()), at_threshold=len(at))


for _k in ("H", "F"):
    _M, _xI, _xJ, _pl = _equality_views(_k)
    for _what, _thr in (("at", 5.0), ("next", float(np.nextafter(5.0, np.inf))), ("zero", 0.0), ("inf", np.inf)):
        _add(f"equality_{_k}_{_what}", "equality", _k, _M, _thr, -1.0, _xI, _xJ, _proof_equality, aux=dict(planted=_pl, what=_what))


# ---------------------------------------------------------------------------------------------------------------- slack
SLACK_WINDOW = (0.97, 1.03)


def _slack_F_views(name, n, lo, hi, reach, tz, thr):
    """n queries in [lo, hi]^2, F = [t]x with t = (0.8, 0.6, tz): oblique lines towards a far epipole.  Candidate of query i: a point
    of i's line up to `reach` away along it, offset 0.97 .. 1.03 thr to either side, the f32 position chosen (among 256 draws) so
    that the f64 distance of the ROUNDED position lies in that window; J is a permutation of those."""
    r = _rng(name)
    M = skew((0.8, 0.6, tz))
    xyI = r.uniform(lo, hi, (n, 2)).astype(F32)
    a0, a1, a2, den = _lines("F", M, xyI)
    nn = np.sqrt(den)
    K = 256
    s = r.uniform(-reach, reach, (n, K)); off = r.choice([-1.0, 1.0], (n, K)) * r.uniform(*SLACK_WINDOW, (n, K)) * thr
    px = (xyI[:, 0:1].astype(np.float64) + s * (-a1 / nn)[:, None] + off * (a0 / nn)[:, None]).astype(F32).astype(np.float64)
    py = (xyI[:, 1:2].astype(np.float64) + s * (a0 / nn)[:, None] + off * (a1 / nn)[:, None]).astype(F32).astype(np.float64)
    d = a0[:, None] * px + a1[:, None] * py + a2[:, None]
    rel = np.sqrt((d * d) / den[:, None]) / thr
    good = (rel >= SLACK_WINDOW[0]) & (rel <= SLACK_WINDOW[1])
    assert good.any(axis=1).all(), name
    k = np.argmax(good, axis=1)
    pts = np.stack([px[np.arange(n), k], py[np.arange(n), k]], axis=1)
    perm = r.permutation(n)
    xyJ = np.zeros((n, 2)); xyJ[perm] = pts
    return M, xyI, xyJ.astype(F32), perm


def _proof_slack(case, cand, gate):
    """the planted candidates straddle the threshold within the window, on both sides; the coordinates are where the case says"""
    mask = candidate_mask(case, cand)
    perm = case["aux"]["perm"]
    lo, hi = case["aux"]["window"]
    errTh = err_th(case)
    rel = np.array([_err(case, i, int(perm[i])) for i in range(len(perm))]) / errTh
    assert np.all((rel >= lo * lo) & (rel <= hi * hi)), (rel.min(), rel.max())
    inside = int((rel < 1.0).sum())
    assert inside >= len(perm) // 4 and len(perm) - inside >= len(perm) // 4, inside
    assert all(mask[i, int(perm[i])] == (rel[i] < 1.0) for i in range(len(perm)))
    a = np.abs(np.concatenate([case["xyI"], case["xyJ"]]))
    assert a.min() >= case["aux"]["coords"][0] and a.max() <= case["aux"]["coords"][1], (a.min(), a.max())
    return dict(candidates=int(mask.sum()), planted_inside=inside, planted_outside=len(perm) - inside)


_M, _xI, _xJ, _perm = _slack_F_views("slack_F", 1500, 2.4e6, 3.6e6, 3e5, 1e-7, 1.0)
_add("slack_F", "slack", "F", _M, 1.0, -1.0, _xI, _xJ, _proof_slack, aux=dict(perm=_perm, window=SLACK_WINDOW, coords=(2e6, 4e6)))
# E with the views' pinhole matrices: the same lines through f_from_e (K_J^-T E K_I^-1 gives F back to within 1e-9 of a coefficient,
# which moves a distance by ~1e-9 px: the same window)
_KI = np.array([1200.0, 0, 2.5e6, 0, 1200.0, 2.5e6, 0, 0, 1]); _KJ = np.array([1500.0, 0, 2.4e6, 0, 1500.0, 2.6e6, 0, 0, 1])
_E = np.array([sum(_KJ[3 * a + r] * _M[3 * a + b] * _KI[3 * b + c] for a in range(3) for b in range(3)) for r in range(3) for c in range(3)])     # K_J^T F K_I
_add("slack_E", "slack", "E", _E, 1.0, -1.0, _xI, _xJ, _proof_slack, KI=_KI, KJ=_KJ, aux=dict(perm=_perm, window=SLACK_WINDOW, coords=(2e6, 4e6)))
_M, _xI, _xJ, _perm = _slack_F_views("slack_F_small", 1500, 2200.0, 3900.0, 140.0, 1e-4, 1e-3)
_add("slack_F_small", "slack", "F", _M, 1e-3, -1.0, _xI, _xJ, _proof_slack, aux=dict(perm=_perm, window=SLACK_WINDOW, coords=(2048.0, 4096.0)))


def _slack_H_views(name, n, thr):
    """transfers and positions in [2^21, 2^22) (f32 spacing 0.25).  Candidate of query i: one of the 17 x 17 f32 positions around the
    rounded transfer -- for i % 3 == 0 one the gate WITHOUT slack would lose (err < errTh, |x - f32(px)| > f32(thr)) if there is one,
    else (and for i % 3 == 1) one with err in [0.9, 1) errTh, for i % 3 == 2 one with err in (1, 1.1] errTh."""
    r = _rng(name)
    M = np.array([1.0003, 2e-4, 17.3, -2e-4, 0.9998, -25.7, 1e-11, -2e-11, 1.0])
    xyI = r.uniform(2.3e6, 3.7e6, (n, 2)).astype(F32)
    a0, a1, _, _ = _lines("H", M, xyI)
    f0 = a0.astype(F32); f1 = a1.astype(F32)
    assert a0.min() > 2.0 ** 21 + 4 and a0.max() < 2.0 ** 22 - 4 and a1.min() > 2.0 ** 21 + 4 and a1.max() < 2.0 ** 22 - 4
    ks = np.arange(-8, 9) * 0.25
    gx = f0.astype(np.float64)[:, None, None] + ks[None, :, None] + 0 * ks[None, None, :]
    gy = f1.astype(np.float64)[:, None, None] + 0 * ks[None, :, None] + ks[None, None, :]
    ex = gx - a0[:, None, None]; ey = gy - a1[:, None, None]
    rel = (ex * ex + ey * ey) / (thr * thr)
    T32 = F32(thr)
    lost = (rel < 1.0) & ((np.abs(gx.astype(F32) - f0[:, None, None]) > T32) | (np.abs(gy.astype(F32) - f1[:, None, None]) > T32))
    inside = (rel >= 0.9) & (rel < 1.0); outside = (rel > 1.0) & (rel <= 1.1)
    pts = np.zeros((n, 2)); n_lost = 0
    for i in range(n):
        want = [lost[i], inside[i]] if i % 3 == 0 else ([inside[i]] if i % 3 == 1 else [outside[i]])
        want += [inside[i], outside[i]]
        sel = next(w for w in want if w.any())
        n_lost += sel is lost[i]
        c = np.argwhere(sel); c = c[r.integers(len(c))]
        pts[i] = gx[i, c[0], c[1]], gy[i, c[0], c[1]]
    perm = r.permutation(n)
    xyJ = np.zeros((n, 2)); xyJ[perm] = pts
    return M, xyI, xyJ.astype(F32), perm, int(n_lost)


# thr 0.9: off the 0.25 lattice of the positions (the gate's |x - f32(px)| is a multiple of 0.25)
_M, _xI, _xJ, _perm, _nl = _slack_H_views("slack_H", 1500, 0.9)
_add("slack_H", "slack", "H", _M, 0.9, -1.0, _xI, _xJ, _proof_slack, aux=dict(perm=_perm, window=(0.9 ** 0.5, 1.1 ** 0.5), coords=(2e6, 4e6), built_lost=_nl))
# thr 1 exactly: ON the lattice.  Here a gate without slack loses nothing, whatever the positions: |x - f32(px)| is a multiple of the
# spacing u of x (u divides 1 for |x| >= 1), f32(px) is within U / 2 <= u of px (U: spacing at px, at most 2 u across a binade), and
# |x - px| < 1, so |x - f32(px)| < 1 + u and therefore <= 1 = f32(thr): the `<=` of the gate passes it.  SLACK_LOSSLESS cases assert
# that count (0) where the other slack cases assert a loss of >= 5 %.
_M, _xI, _xJ, _perm, _nl = _slack_H_views("slack_H_unit", 1500, 1.0)
assert _nl == 0
_add("slack_H_unit", "slack", "H", _M, 1.0, -1.0, _xI, _xJ, _proof_slack, aux=dict(perm=_perm, window=(0.9 ** 0.5, 1.1 ** 0.5), coords=(2e6, 4e6), built_lost=0))
SLACK_LOSSLESS = ("slack_H_unit",)


# ---------------------------------------------------------------------------------------------------------------- domain
def _plant_on_lines(M, xyI, xs):
    """the f32 position at abscissa xs[i] on query i's line (F)"""
    a0, a1, a2, _ = _lines("F", M, xyI)
    return np.stack([xs, -(a0 * xs + a2) / a1], axis=1).astype(F32)


def _domain_tiles(kind):
    """J of three tiles (4096 + 4096 + 37); only the middle one holds positions >= 1e7 and one inf.  Queries 0..99 have their
    candidate in tile 0 (one of them at its last index), 100..199 in the middle tile, 200..236 in tile 2 (all of it, first and last
    index included), 237..299 in tile 0 again."""
    r = _rng("domain_tiles_" + kind)
    nJ = 2 * TILE + 37
    xyJ = np.zeros((nJ, 2), F32)
    xyJ[:TILE] = r.uniform(0, 4000, (TILE, 2)); xyJ[2 * TILE:] = r.uniform(0, 4000, (37, 2))
    xyJ[TILE:2 * TILE, 0] = r.integers(10_000_000, 16_000_000, TILE); xyJ[TILE:2 * TILE, 1] = r.uniform(0, 4000, TILE)
    t0 = r.choice(TILE - 1, 162, replace=False)
    js = np.concatenate([t0[:99], [TILE - 1], TILE + r.choice(TILE, 100, replace=False),
                         [2 * TILE, nJ - 1], 2 * TILE + 1 + r.choice(35, 35, replace=False), t0[99:]]).astype(int)
    taken = set(js.tolist())
    inf_j = next(j for j in range(TILE + 2000, 2 * TILE) if j not in taken)
    if kind == "H":
        M = np.array([1, 0, 10, 0, 1, -6, 0, 0, 1], np.float64)
        xyI = np.floor(r.uniform(100, 3900, (300, 2)))
        xyI[100:200, 0] = r.integers(10_000_100, 15_900_000, 100)
        off = r.integers(-2, 3, (300, 2)).astype(np.float64)
        xyJ[js[:300]] = (xyI + [10, -6] + off).astype(F32)
        thr = 3.5
    else:
        M = skew((0.8, 0.6, 1e-4))
        xyI = r.uniform(100, 3900, (300, 2)).astype(F32)
        xs = r.uniform(100, 3900, 300); xs[100:200] = r.integers(10_000_100, 15_900_000, 100)
        xyJ[js[:300]] = _plant_on_lines(M, xyI, xs)
        thr = 4.0
    xyJ[inf_j] = (np.inf, 100.0)
    return M, xyI, xyJ, thr, js[:300]


def _proof_domain_tiles(case, cand, gate):
    mask = candidate_mask(case, cand)
    js = case["aux"]["js"]
    k, M = model_of(case)
    assert all(mask[i, js[i]] for i in range(300))
    per_tile = [int(mask[:, t:t + TILE].sum()) for t in range(0, mask.shape[1], TILE)]
    assert len(per_tile) == 3 and min(per_tile) >= 37
    assert mask[:, TILE - 1].any() and mask[:, 2 * TILE].any() and mask[:, -1].any()
    ex = exact_all_tiles(k, M, case["xyI"], case["xyJ"], err_th(case))
    assert not ex[:, 0].any() and ex[:, 1].all() and not ex[:, 2].any()           # gated, exact_all, gated again: both smax buffers
    assert np.isinf(case["xyJ"][TILE:2 * TILE]).sum() == 1 and np.abs(case["xyJ"][TILE:2 * TILE, 0]).min() >= POS_LIMIT
    assert gate[:, TILE:2 * TILE].all() and gate[:, :TILE].mean() < 0.1 and gate[:, 2 * TILE:].mean() < 0.5
    return dict(candidates=int(mask.sum()), per_tile=per_tile)


for _k in ("F", "H"):
    _M, _xI, _xJ, _thr, _js = _domain_tiles(_k)
    _add(f"domain_tiles_{_k}", "domain", _k, _M, _thr, -1.0, _xI, _xJ, _proof_domain_tiles, aux=dict(js=_js))


def _plain_F_views(name, nI, nJ, thr, plant=None, coords=4000.0):
    """random positions, F = [t]x with the epipole at (8000, 6000); query i (i < nJ) has a planted candidate on its line at j = plant[i]
    (default: a permutation), off the line by the f32 rounding of the position only"""
    r = _rng(name)
    M = skew((0.8, 0.6, 1e-4))
    xyI = r.uniform(0.02 * coords, coords, (nI, 2)).astype(F32)
    xyJ = r.uniform(0.02 * coords, coords, (nJ, 2)).astype(F32)
    if plant is None:
        plant = r.permutation(nJ)[:min(nI, nJ)]
    q = np.arange(len(plant))
    xyJ[plant] = _plant_on_lines(M, xyI[q], r.uniform(0.02 * coords, coords, len(q)))
    return M, xyI, xyJ, np.asarray(plant)


_SCALES = (1.0, 1e32, 1e-32, 1e-40)


def _proof_scale(case, cand, gate):
    """the scaled model's candidates are the unscaled model's; its coefficients are where the case says"""
    base = next(c for c in CASES if c["name"] == "domain_scale_1")
    assert np.array_equal(candidate_mask(case, cand), candidate_mask(base, candidates_of(base)))
    assert all(len(js) for js, _ in cand[:len(case["aux"]["plant"])])
    a0, a1, a2, den = _lines("F", case["M"], case["xyI"])
    s = case["aux"]["scale"]
    if s == 1e32:
        assert (np.maximum(np.abs(a0), np.abs(a2)) >= COEF_LIMIT).all() and gate.all()
    elif s == 1e-40:
        assert (np.abs(np.stack([a0, a1]).astype(F32)) < _TINY).all()            # (l2 = tx y - ty x is up to 4000 times larger)
    elif s == 1e-32:
        assert (np.sqrt(err_th(case) * den) < GATE_ABS).all() and (np.abs(a2.astype(F32)) > _TINY).all()
    m = candidate_mask(case, cand)
    return dict(candidates=int(m.sum()), gate_share=float(gate.mean()))


_M, _xI, _xJ, _pl = _plain_F_views("domain_scale", 300, 600, 2.0)
_dI, _dJ = _default_descs("domain_scale", 300, 600)
for _s in _SCALES:
    _add("domain_scale_%g" % _s, "domain", "F", _M * _s, 2.0, -1.0, _xI, _xJ, _proof_scale, descI=_dI, descJ=_dJ, ratios=(-1.0, 0.8),
         aux=dict(scale=_s, plant=_pl))


def _proof_w0(case, cand, gate):
    x1 = case["xyI"][:, 0].astype(np.float64); y1 = case["xyI"][:, 1].astype(np.float64)
    M = case["M"]
    w = M[6] * x1 + M[7] * y1 + M[8]
    zero = w == 0.0
    with np.errstate(all="ignore"):
        a1 = (M[3] * x1 + M[4] * y1 + M[5]) / w
    assert zero.sum() >= 8 and np.isnan(a1[zero]).any() and np.isinf(a1[zero]).any()
    assert all(len(cand[i][0]) == 0 for i in np.flatnonzero(zero))
    assert sum(len(js) for js, _ in cand) >= (~zero).sum()
    assert gate[zero].all()                                        # no gate for a transfer that is not finite
    return dict(candidates=sum(len(js) for js, _ in cand), w_zero=int(zero.sum()))


def _w0_views():
    """H = [2 0 -150; 0 1 0; 1 0 -100]: w = x - 100 is 0 for the queries at x = 100 (their transfer is inf, or 0 / 0 where y = 0 too)"""
    r = _rng("domain_w0")
    M = np.array([2, 0, -150, 0, 1, 0, 1, 0, -100], np.float64)
    xyI = np.floor(r.uniform(101, 400, (120, 2)))
    xyI[::10, 0] = 100.0
    xyI[::20, 1] = 0.0
    a0, a1, _, _ = _lines("H", M, xyI.astype(F32))
    xyJ = np.stack([a0, a1], axis=1)
    xyJ[~np.isfinite(xyJ).all(axis=1)] = (7.0, 7.0)
    return M, xyI, np.concatenate([xyJ, r.uniform(0, 400, (60, 2))])


_M, _xI, _xJ = _w0_views()
_add("domain_w0", "domain", "H", _M, 3.0, -1.0, _xI, _xJ, _proof_w0)
_add("domain_w0_inf", "domain", "H", _M, np.inf, -1.0, _xI, _xJ, _proof_w0)


def _proof_epipole(case, cand, gate):
    a0, a1, a2, den = _lines("F", case["M"], case["xyI"])
    at = np.flatnonzero(den == 0.0)
    assert len(at) == 3 and (a2[at] == 0.0).all()
    assert all(np.isnan(_err(case, int(i), 0)) for i in at) and all(len(cand[i][0]) == 0 for i in at)
    assert sum(len(js) for js, _ in cand) >= len(cand) - 3
    return dict(candidates=sum(len(js) for js, _ in cand), at_epipole=len(at))


def _epipole_views():
    """F = [e]x with e = (120, 80, 1); queries 5, 50 and 99 sit on the epipole: their line is (0, 0, 0), den = 0, err = 0 / 0"""
    r = _rng("domain_epipole")
    M = skew((120.0, 80.0, 1.0))
    xyI = np.floor(r.uniform(0, 400, (100, 2))).astype(F32)
    xyI[[5, 50, 99]] = (120.0, 80.0)
    keep = np.flatnonzero(~((xyI[:, 0] == 120) & (xyI[:, 1] == 80)))
    # a candidate on the line of every other query: the point halfway to the epipole, rounded to f32
    pts = ((xyI[keep].astype(np.float64) + [120.0, 80.0]) / 2).astype(F32)
    return M, xyI, np.concatenate([pts, r.uniform(0, 400, (50, 2)).astype(F32)])


_M, _xI, _xJ = _epipole_views()
_add("domain_epipole", "domain", "F", _M, 2.0, -1.0, _xI, _xJ, _proof_epipole)
_add("domain_epipole_inf", "domain", "F", _M, np.inf, -1.0, _xI, _xJ, _proof_epipole)


def _proof_nan(case, cand, gate):
    nI = np.isnan(case["xyI"]).any(axis=1); nJ = np.isnan(case["xyJ"]).any(axis=1)
    assert nI.sum() >= 3 and nJ.sum() >= 3
    mask = candidate_mask(case, cand)
    assert not mask[nI].any() and not mask[:, nJ].any() and mask.sum() >= 100
    assert gate[nI].all() and not gate[~nI][:, nJ].any()          # a NaN query has no gate; a NaN position fails a finite gate
    return dict(candidates=int(mask.sum()), nan_I=int(nI.sum()), nan_J=int(nJ.sum()))


for _k in ("F", "H"):
    _M, _xI, _xJ, _pl = _plain_F_views("domain_nan_" + _k, 300, 500, 2.0)
    if _k == "H":
        _M = np.array([1.01, 0.02, 5, -0.02, 0.99, -3, 1e-6, 2e-6, 1], np.float64)
        _a0, _a1, _, _ = _lines("H", _M, _xI)
        _xJ[_pl] = np.stack([_a0, _a1], axis=1)[:len(_pl)].astype(F32)
    _free = np.setdiff1d(np.arange(500), _pl)
    _xJ[_free[0]] = (np.nan, 10.0); _xJ[_free[1]] = (10.0, np.nan); _xJ[_free[2]] = (np.nan, np.nan); _xJ[_pl[7]] = (np.nan, np.nan)
    _xI[3] = (np.nan, 10.0); _xI[100] = (10.0, np.nan); _xI[299] = (np.nan, np.nan)
    _add("domain_nan_" + _k, "domain", _k, _M, 2.0, -1.0, _xI, _xJ, _proof_nan)


# ---------------------------------------------------------------------------------------------------------------- ties
def _proof_ties_geom(case, cand, gate):
    pairs = case["aux"]["pairs"]
    for i, (ja, jb) in enumerate(pairs):
        js, errs = cand[i]
        assert js == [ja, jb] and errs[0] == errs[1] and ja < jb, (i, js, errs)
    m = G.guided_pair(case["kind"], case["M"], case["thr_px"], -1.0, case["xyI"], case["xyJ"])
    assert m.tolist() == [[i, ja] for i, (ja, _) in enumerate(pairs)]
    if case["aux"]["cut"]:
        assert (TILE - 1, TILE) in pairs
    return dict(candidates=sum(len(js) for js, _ in cand), ties=len(pairs))


def _ties_geom_views(cut):
    """F_Y: query i at y = 100 i; two candidates one row above and one below (err 1 each); with `cut` the pair of query 3 sits at
    j = 4095 and 4096, on both sides of the tile cut, and that of query 4 at j = 4096 + 4095 and the last index"""
    r = _rng("ties_geom")
    n = 12
    xyI = np.stack([10.0 + np.arange(n), 100.0 * (1 + np.arange(n))], axis=1)
    nJ = 2 * TILE + 1 if cut else 64
    xyJ = _fill_far(nJ, r)
    slots = r.permutation(np.arange(10, 60))[:2 * n].reshape(n, 2); slots.sort(axis=1)
    if cut:
        slots[3] = (TILE - 1, TILE); slots[4] = (2 * TILE - 1, 2 * TILE); slots[5] = (0, 2 * TILE - 2)
    for i, (ja, jb) in enumerate(slots):
        up = 1.0 if i % 2 else -1.0
        xyJ[ja] = (500.0 + i, xyI[i, 1] + up); xyJ[jb] = (40.0 - i, xyI[i, 1] - up)
    return xyI, xyJ, [tuple(int(v) for v in s) for s in slots]


for _cut in (False, True):
    _xI, _xJ, _pairs = _ties_geom_views(_cut)
    _add("ties_geom_cut" if _cut else "ties_geom", "ties", "F", F_Y, 2.0, -1.0, _xI, _xJ, _proof_ties_geom, ratios=(-1.0,),
         aux=dict(pairs=_pairs, cut=_cut))


def ratio_flip(limit=488):
    """the first (ratio, bd, sbd), bd < sbd <= limit, whose verdict float(bd) < ratio^2 float(sbd) differs between double and f32"""
    for ratio in (0.6, 0.8, 0.7, 0.9, 0.5):
        R = ratio * ratio
        for sbd in range(2, limit + 1):
            for bd in range(1, sbd):
                if (float(bd) < R * float(sbd)) != bool(F32(bd) < F32(R) * F32(sbd)):
                    return ratio, bd, sbd
    raise AssertionError("no verdict differs")


def _squares(v, dim=8, top=255):
    """a row of `dim` non-negative integers <= top whose squares sum to v"""
    row = []
    while v:
        a = min(int(np.sqrt(v)), top)
        while (a + 1) * (a + 1) <= v and a < top:
            a += 1
        row.append(a); v -= a * a
    assert len(row) <= dim, row
    return row + [0] * (dim - len(row))


def _bits(k, nbytes=61):
    """a binary row with the k lowest bits set"""
    return np.packbits((np.arange(nbytes * 8) < k).astype(np.uint8), bitorder="little")


# per query of the tie cases: the distances of its candidates in ascending j (None: the verdict-flip pair)
_TIE_PLAN = [[], [4], [4, 25], [9, 9], [0, 0], None, [50, 4, 4], [0, 7], [16, 16, 1], [9, 1, 4], [1, 4, 9]]


def _ties_desc_views(dtype):
    ratio, bd, sbd = ratio_flip()
    plan = [p if p is not None else [sbd, bd, sbd + 60] for p in _TIE_PLAN]
    n = len(plan)
    xyI = np.stack([10.0 + np.arange(n), 100.0 * (1 + np.arange(n))], axis=1)
    rows, pos = [], []
    for i, ds in enumerate(plan):
        for c, d in enumerate(ds):
            pos.append((300.0 + 7 * c + i, xyI[i, 1] + (c % 3 - 1) * 0.5)); rows.append(d)
    pos.append((1.0, 5000.0)); rows.append(3)
    xyJ = np.array(pos)                                            # (ascending j is the plan's order within a query)
    if dtype == "bin":
        descI = np.zeros((n, 61), np.uint8); descJ = np.stack([_bits(d) for d in rows])
    else:
        descI = np.zeros((n, 8), F32 if dtype == "f32" else np.uint8)
        descJ = np.array([_squares(d) for d in rows]).astype(descI.dtype)
    return ratio, (bd, sbd), plan, xyI, xyJ, descI, descJ


def _proof_ties_desc(case, cand, gate):
    plan, (bd, sbd), ratio = case["aux"]["plan"], case["aux"]["flip"], case["ratio"]
    binary = case["binary"]
    counts = [len(js) for js, _ in cand]
    assert counts == [len(p) for p in plan] and {0, 1, 2} <= set(counts)
    for i, (js, _) in enumerate(cand):
        assert [G.descriptor_distance(case["descI"][i], case["descJ"][j], binary) for j in js] == plan[i], i
    R = ratio * ratio
    assert (float(bd) < R * float(sbd)) != bool(F32(bd) < F32(R) * F32(sbd))          # the verdict of query 5 needs the double
    flip_i = _TIE_PLAN.index(None)
    got = {r: G.guided_pair("F", case["M"], case["thr_px"], r, case["xyI"], case["xyJ"], case["descI"], case["descJ"], binary) for r in case["ratios"] if r >= 0}
    in_double = float(bd) < R * float(sbd)
    assert (flip_i in got[ratio][:, 0].tolist()) == in_double
    # duplicate rows (bd == sbd) match only above ratio 1 and then the first j; bd = sbd = 0 never; one candidate never
    assert 3 not in got[ratio][:, 0].tolist() and got[1.5][got[1.5][:, 0] == 3][0, 1] == cand[3][0][0]
    assert all(4 not in g[:, 0].tolist() and 1 not in g[:, 0].tolist() and 0 not in g[:, 0].tolist() for g in got.values())
    return dict(candidates=sum(counts), flip=(ratio, bd, sbd), verdict_in_double=in_double)


for _dt in ("f32", "u8", "bin"):
    _ratio, _flip, _plan, _xI, _xJ, _dI, _dJ = _ties_desc_views(_dt)
    _add("ties_desc_" + _dt, "ties", "F", F_Y, 1.0, _ratio, _xI, _xJ, _proof_ties_desc, descI=_dI, descJ=_dJ, binary=_dt == "bin",
         ratios=(_ratio, 1.5, -1.0), aux=dict(plan=_plan, flip=_flip))


# ---------------------------------------------------------------------------------------------------------------- shapes
N_I = (1, 255, 256, 257)
N_J = (1, 2, 3, 4, 5, 4095, 4096, 4097, 8193)


def _shape_plant(nI, nJ):
    """the j of query i's planted candidate: the last index, the first, and both sides of every tile cut come first"""
    special = [nJ - 1, 0] + [j for t in range(TILE, nJ, TILE) for j in (t - 1, t)] + [nJ - 2, 1, nJ // 2]
    seen, js = set(), []
    for j in special + list(range(2, nJ)):
        if 0 <= j < nJ and j not in seen:
            seen.add(j); js.append(j)
        if len(js) == nI:
            break
    return np.array(js)


def _proof_shapes(case, cand, gate):
    nI, nJ = len(case["xyI"]), len(case["xyJ"])
    plant = case["aux"]["plant"]
    mask = candidate_mask(case, cand)
    assert all(mask[i, j] for i, j in enumerate(plant))
    edges = [j for j in [nJ - 1, 0] + [j for t in range(TILE, nJ, TILE) for j in (t - 1, t)] if j in set(plant.tolist())]
    assert nJ - 1 in edges and all(mask[:, j].any() for j in edges)
    if nJ > TILE and nI >= 4:
        assert TILE - 1 in edges and TILE in edges
    return dict(candidates=int(mask.sum()), nI=nI, nJ=nJ, blocks=-(-nI // BLOCK), tiles=-(-nJ // TILE))


def _shape_case(nI, nJ, kind):
    name = f"shapes_{kind}_{nI}x{nJ}"
    plant = _shape_plant(nI, nJ)
    M, xyI, xyJ, _ = _plain_F_views(name, nI, nJ, 2.0, plant=plant)
    if kind == "H":
        M = np.array([0.99, 0.03, -4, -0.03, 1.02, 9, 2e-6, -1e-6, 1], np.float64)
        a0, a1, _, _ = _lines("H", M, xyI)
        xyJ[plant] = np.stack([a0, a1], axis=1)[:len(plant)].astype(F32)
    _add(name, "shapes", kind, M, 2.0, 0.8, xyI, xyJ, _proof_shapes, aux=dict(plant=plant))


for _n, _nJ in enumerate(N_J):
    _shape_case(257, _nJ, "FH"[_n % 2])
for _n, _nI in enumerate(N_I[:3]):
    _shape_case(_nI, 4097, "HF"[_n % 2])
_shape_case(1, 1, "F"); _shape_case(256, 8193, "H"); _shape_case(255, 5, "F")

# one call of many pairs: 14 views of mixed sizes -- one feature, zero features in the middle and at the end of the list, sizes on
# both sides of the query block -- and every (I, J), I < J, plus one pair whose I is the empty last view: 92 jobs, so that
# guided_job_of's search maps 25 workgroups to jobs of 0, 1, 2, 3 and 4 workgroups
MANY_SIZES = (1, 300, 0, 257, 1, 600, 256, 40, 255, 513, 3, 1000, 64, 0)


def many_pairs_case():
    """-> dict(views [(xy, desc)], pairs [P, 2], kind, models [P, 9], thrs [P], ratios): view v shows a subset of 1000 points, shifted
    by (3 v, -2 v), with their rows (small integers) up to +-1 per entry; the model of (I, J) is that translation and the thresholds
    (3 .. 7 px at 0.006 points per px^2) leave many queries two candidates or more, so both modes keep most pairs"""
    r = _rng("shapes_many_pairs")
    base = r.uniform(50, 450, (max(MANY_SIZES), 2)); rows = r.integers(0, 40, (max(MANY_SIZES), 8))
    views = []
    for v, n in enumerate(MANY_SIZES):
        pick = r.permutation(len(base))[:n]
        xy = (base[pick] + [3.0 * v, -2.0 * v] + r.normal(0, 0.5, (n, 2))).astype(F32)
        views.append((xy, (rows[pick] + r.integers(-1, 2, (n, 8))).astype(F32)))
    V = len(MANY_SIZES)
    pairs = [(i, j) for i in range(V) for j in range(i + 1, V)] + [(V - 1, 5)]
    models = [[1, 0, 3.0 * (j - i), 0, 1, -2.0 * (j - i), 0, 0, 1] for i, j in pairs]
    thrs = [3.0 + (k % 5) for k in range(len(pairs))]
    return dict(name="shapes_many_pairs", family="shapes", kind="H", views=views, pairs=np.array(pairs, np.uint32),
                models=np.array(models, np.float64), thrs=np.array(thrs), ratios=(0.8, -1.0))


# ---------------------------------------------------------------------------------------------------------------- dedup
def _dedup_views():
    """H = a translation by (5, 0), thr 1.5, geometry only.  Classes of equal positions in I (their matches share (xI, yI, xJ, yJ)):
    {0, 2} with the unmatched 1 between them; {3, 4, 6} whose best candidate is the first of two equal positions of J; {7, 8}:
    -0.0 against +0.0 in I; {9, 10} against a -0.0 in J; NaN positions in I (11, 12) and in J, which equal nothing and match nothing;
    13 alone.  Feature 5 has no candidate.  (Features of ONE class share their position and so their best candidate: in this mode an
    earlier member of a class cannot be without a match while a later one has one.  What the walk from the class's first member to i
    meets are unmatched features of other classes -- 1 inside {0, 2}, 5 inside {3, 4, 6} -- and it must step over them.)"""
    nan = np.nan
    xyI = np.array([[10, 100], [700, 900], [10, 100], [20, 200], [20, 200], [800, 900], [20, 200], [-0.0, 50], [0.0, 50],
                    [40, 0.0], [40, -0.0], [nan, 7], [nan, 7], [60, 300]], F32)
    xyJ = np.array([[15, 100.5], [16, 101], [25, 200], [25, 200], [nan, 7], [5, 50], [45, -0.0], [nan, nan], [65, 300.5], [5, 50.5]], F32)
    return xyI, xyJ


def _proof_dedup(case, cand, gate):
    m = G.guided_pair(case["kind"], case["M"], case["thr_px"], -1.0, case["xyI"], case["xyJ"])
    got = [tuple(r) for r in m.tolist()]
    if case["kind"] == "H":
        assert got == [(0, 0), (3, 2), (7, 5), (9, 6), (13, 8)], got
    else:
        assert got == [(0, 0), (2, 0), (3, 2), (4, 2), (6, 2), (7, 5), (8, 5), (9, 6), (10, 6), (13, 8)], got
    assert len(cand[1][0]) == 0 and len(cand[5][0]) == 0 and len(cand[11][0]) == 0 and len(cand[12][0]) == 0
    assert np.signbit(case["xyI"][7, 0]) and not np.signbit(case["xyI"][8, 0]) and np.signbit(case["xyJ"][6, 1])
    return dict(candidates=sum(len(js) for js, _ in cand), matches=len(got))


_xI, _xJ = _dedup_views()
_add("dedup_H", "dedup", "H", [1, 0, 5, 0, 1, 0, 0, 0, 1], 1.5, -1.0, _xI, _xJ, _proof_dedup, ratios=(-1.0,))
# the same views under F (lines y = y1: the same best candidates): every match stays
_add("dedup_F_keeps", "dedup", "F", F_Y, 1.5, -1.0, _xI, _xJ, _proof_dedup, ratios=(-1.0,))

NAMES = [c["name"] for c in CASES]
FAMILIES = ("equality", "slack", "domain", "ties", "shapes", "dedup")
