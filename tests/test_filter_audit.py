"""The CPU restatement's AC-RANSAC (oracle/acransac.c) against the pixel-space definition (filter_audit.py) on views that all differ.

Until this module every AC-RANSAC test ran on pairs of interchangeable views (one size, one K), so neither an I/J swap of a size or
a pinhole matrix nor a wrong view's size could show anywhere.  Here the oracle filters the asymmetric collection of filter_audit.py --
registered under sparse view ids, since the ids seed the sample stream -- and every result must pass the audit with the sizes and the
K of ITS two views; the same results audited with the sizes exchanged, with K_I and K_J exchanged or with the model transposed must be
rejected; and on a pair of equal views the exchanged audit passes, which is why the new scenes exist.

Measured for the oracle over the collection (14 pairs of 40 .. 4200 putatives, precision 4 px, 2048 iterations, seed 5489):
         worst |threshold - audit| / audit      worst |NFA - audit|      smallest gap last inlier -> first other
    F            1.5e-13                          7.5e-4  (n = 4200)       7.7e-3
    E            4.2e-13                          7.3e-4  (n = 4200)       1.2e-2
    H            2.0e-13                          1.05e-3 (n = 4200)       2.6e-3
against the tolerances 1e-9 (threshold, relative), filter_audit.nfa_tolerance(n) = 2^-24 n (log10 C(n, n/2) + 32) + 1e-4 (NFA: 2e-4 at
n = 40, 0.043 at n = 1500, 0.32 at n = 4200) and the dead band 1e-9 (gap).  The mutants move the NFA by tens to thousands."""
import numpy as np
import pytest

import filter_audit as A
import filter_views_cases as V

IDS = [5, 2, 11, 7, 3, 19, 8]            # view id of collection view 0 .. 6: sparse, and in no order


@pytest.fixture(scope="module")
def col():
    return A.make_collection(IDS)


@pytest.fixture(scope="module")
def results(oracle, col):
    return {kind: V.expected(oracle, col, kind) for kind in "FEH"}


def _estimated(results, kind):
    return [(p, e) for p, e in enumerate(results[kind]) if e is not None and e["n_inliers"] > 0]


def _areas_differ(col, p):
    wI, hI, wJ, hJ = col.sizes(p)
    return wI * hI != wJ * hJ


@pytest.mark.parametrize("kind", ["F", "E", "H"])
def test_the_oracle_passes_the_audit_on_views_that_differ(col, results, kind):
    worst = dict(threshold_rel=0.0, nfa_abs=0.0, gap_rel=np.inf)
    rows = _estimated(results, kind)
    for p, e in rows:
        r = V.audit_pair(col, kind, p, 4.0, e["model"], e["inliers"], e["threshold"], e["nfa"])
        assert r["k"] == e["n_inliers"]
        worst = dict(threshold_rel=max(worst["threshold_rel"], r["threshold_rel"]), nfa_abs=max(worst["nfa_abs"], r["nfa_abs"]),
                     gap_rel=min(worst["gap_rel"], r["gap_rel"]))
    print(kind, "oracle vs audit, worst over", len(rows), "pairs:", worst)
    no_K = IDS[A.NO_K_VIEW]
    if kind == "E":
        assert all((e is None) == (no_K in col.pairs[p].tolist()) for p, e in enumerate(results[kind]))
        assert len(rows) == len(col.pairs) - sum(no_K in pr.tolist() for pr in col.pairs) == 12
    else:
        assert len(rows) == len(col.pairs)
    assert any(e["kept"] and col.counts[p] == A.LONG_PAIR for p, e in rows)


@pytest.mark.parametrize("kind", ["F", "E", "H"])
def test_the_audit_rejects_exchanged_sizes(col, results, kind):
    """(wI, hI) <-> (wJ, hJ): rejected on every pair whose views differ in area (a 4000 x 3000 / 3000 x 4000 pair has s1 = s2 and one
    D / A: there the exchange changes nothing the definition can see)"""
    n = 0
    for p, e in _estimated(results, kind):
        if _areas_differ(col, p):
            with pytest.raises(A.AuditError):
                V.audit_pair(col, kind, p, 4.0, e["model"], e["inliers"], e["threshold"], e["nfa"], swap_sizes=True)
            n += 1
    assert n >= 9


def test_the_audit_rejects_exchanged_pinhole_matrices_and_transposed_models(col, results):
    rows = _estimated(results, "E")
    for p, e in rows:
        for kw in ("swap_K", "transpose"):
            with pytest.raises(A.AuditError):
                V.audit_pair(col, "E", p, 4.0, e["model"], e["inliers"], e["threshold"], e["nfa"], **{kw: True})
    for p, e in _estimated(results, "F"):
        with pytest.raises(A.AuditError):
            V.audit_pair(col, "F", p, 4.0, e["model"], e["inliers"], e["threshold"], e["nfa"], transpose=True)
    assert len(rows) >= 9


def test_equal_views_hide_every_exchange(oracle):
    """The blind spot of the scenes used so far: two 1920 x 1080 views with one K.  The audit with the sizes and the pinhole matrices
    exchanged passes, so no test on such a pair can tell I from J."""
    rng = np.random.default_rng(3)
    X = A.make_points(4)[::4]
    K = A.intrinsics(2)
    xy = [(A.project(v, X, K=K) + rng.normal(0, 0.4, (len(X), 2))).astype(np.float32) for v in (1, 4)]
    ii = np.sort(rng.permutation(len(X))[:700]); jj = ii.copy()
    wrong = rng.random(700) < 0.3
    jj[wrong] = rng.integers(0, len(X), int(wrong.sum()))
    views = {0: dict(w=1920, h=1080, K=K, xy=xy[0]), 1: dict(w=1920, h=1080, K=K, xy=xy[1])}
    col = A.Collection(views, np.array([[0, 1]], np.uint32), np.array([700], np.uint32), np.c_[ii, jj].astype(np.uint32))
    for kind in "FEH":
        e = V.expected(oracle, col, kind)[0]
        assert e["kept"]
        a = V.audit_pair(col, kind, 0, 4.0, e["model"], e["inliers"], e["threshold"], e["nfa"])
        b = V.audit_pair(col, kind, 0, 4.0, e["model"], e["inliers"], e["threshold"], e["nfa"], swap_sizes=True, swap_K=True)
        assert a == b


def test_the_audit_checks_what_it_says():
    """the audit on a hand-made homography result: exact answers pass; one inlier more or fewer, a threshold off by 1e-6 and an NFA off
    by 1 are each rejected"""
    rng = np.random.default_rng(1)
    n, k = 60, 40
    xI = rng.uniform(0, 600, (n, 2))
    d = np.r_[np.linspace(0.05, 2.0, k), np.linspace(40.0, 200.0, n - k)]
    xJ = xI + np.c_[d, np.zeros(n)] + [30.0, -20.0]
    Hm = np.array([[1, 0, 30.0], [0, 1, -20.0], [0, 0, 1]])
    sizes = (640, 480, 800, 1200)
    s2 = 1.0 / np.sqrt(800.0 * 1200.0)
    nfa = A.nfa_curve("H", np.sort(A.residuals("H", Hm, xI, xJ, sizes)), 800, 1200)
    assert int(np.argmin(nfa)) == k
    A.audit("H", xI, xJ, sizes, 4.0, Hm, np.arange(k), 2.0, nfa[k])
    assert abs(A.residuals("H", Hm, xI, xJ, sizes)[k - 1] - (2.0 * s2) ** 2) < 1e-18
    for kw in (dict(inliers=np.arange(k + 1)), dict(inliers=np.arange(k - 1)), dict(threshold_px=2.0 * (1 + 1e-6)), dict(nfa=nfa[k] + 1.0),
               dict(precision_px=1.9)):
        args = dict(inliers=np.arange(k), threshold_px=2.0, nfa=nfa[k], precision_px=4.0)
        args.update(kw)
        with pytest.raises(A.AuditError):
            A.audit("H", xI, xJ, sizes, args["precision_px"], Hm, args["inliers"], args["threshold_px"], args["nfa"])
