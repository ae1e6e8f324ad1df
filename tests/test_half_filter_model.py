"""The numpy model of the three levels of l2_knn2_half_kernel (tools/prefix_prune_model.py, model_pair_levels: the f16 level in front of
the pair-norm filter in front of the prefix test) gives the two-level model's result TILE BY TILE on every view pair of
tests/pairnorm_filter_cases.py, tests/prefix_prune_cases.py and tests/half_filter_cases.py -- the pruned set, the filtered set, the
exact-scan queries and the verdicts -- because the f16 bound, less its margin, never exceeds the f32 bound.  It also shows that each
case of tests/test_gpu_half_filter.py holds what it is built for."""
import importlib.util
import os

import numpy as np
import pytest

import half_filter_cases as HC
import pairnorm_filter_cases as FC
import prefix_prune_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("prefix_prune_model", os.path.join(ROOT, "tools", "prefix_prune_model.py"))
M = importlib.util.module_from_spec(_spec); _spec.loader.exec_module(M)

GP = 12


def _views():
    """(name, a, b, R) of every case: those of tests/test_pairnorm_filter_model.py, the NaN view, and half_filter_cases.py's own"""
    out = []
    for nI, nJ in ((64, 70), (97, 130), (160, 130)):
        out.append((f"base_views {nI} x {nJ}", *PC.base_views(nI, nJ, seed=nI * 1000 + nJ), 0.36))
    out.append(("match_in_last_tile", *PC.match_in_last_tile()[:2], 0.36))
    out.append(("runner_up_pruned", *PC.runner_up_pruned()[:2], 0.36))
    out.append(("forced_fallback", *PC.forced_fallback()[:2], 0.36))
    for case in ("seen_tie", "seen_below", "pruned_at_threshold", "pruned_above"):
        out.append((f"ratio_boundary {case}", *PC.ratio_boundary(case)[:2], 0.25))
    for nI in (33, 97):
        for nJ in (70, 130):
            out.append((f"sparse_views {nI} x {nJ}", *FC.sparse_views(nI, nJ, seed=nI * 1000 + nJ), 0.36))
    out.append(("sparse_views 160 x 130", *FC.sparse_views(160, 130, seed=30), 0.36))
    out.append(("swapped_pairs", *FC.swapped_pairs()[:2], 0.36))
    out.append(("sparse match_in_last_tile", *FC.match_in_last_tile()[:2], 0.36))
    out.append(("runner_up_filtered", *FC.runner_up_filtered()[:2], 0.36))
    for kind in ("negative", "real", "large_integers", "nan"):
        out.append((f"other_rows {kind}", *FC.other_rows(kind), 0.36))
    for side in ("pruned", "kept_above", "kept_below"):
        out.append((f"threshold_views {side}", *FC.threshold_views(M, side)[:2], 0.36))
    return out + HC.all_cases(M)


VIEWS = _views()


@pytest.mark.parametrize("name,a,b,R", VIEWS, ids=[v[0] for v in VIEWS])
def test_three_levels_give_the_two_level_result(name, a, b, R):
    """h >= s element by element; the f16 bound is at most the f32 bound wherever it is a number; and the three-level model equals the
    two-level model per tile and per query, with no wrong verdict"""
    for x in (a, b):
        s, h = M.pair_norms(x).astype(np.float64), M.pair_norms_half(x)
        ok = ~np.isnan(s)
        assert (h[ok] >= s[ok]).all() and np.isnan(h[~ok]).all()
        assert ((h == 0) == (s == 0))[ok].all() and (h[ok & (s != 0)] >= 2.0 ** -14).all()                # zero stays zero, no subnormal
        assert (h[ok] == h[ok].astype(np.float16).astype(np.float64)).all()                              # every value is an f16
    LB, _ = M.pairnorm_bound(a, b)
    LBH, margin = M.halfnorm_bound(a, b)
    num = np.isfinite(LBH) & np.isfinite(LB)
    assert (LBH[num] <= LB[num]).all() and (margin[~np.isnan(margin)] > 0).all()
    r3 = M.model_pair_levels(a, b, GP, R)
    r2 = M.model_pair_levels(a, b, GP, R, half=False)
    assert np.array_equal(r3["tile_pruned"], r2["tile_pruned"]) and np.array_equal(r3["tile_filtered"], r2["tile_filtered"])
    assert np.array_equal(r3["verdict"], r2["verdict"]) and r3["wrong"] == r2["wrong"] == 0
    assert not (r3["tile_half"] & ~r3["tile_filtered"]).any() and r2["half"] == 0
    # ... and the two-level model here is the one tests/test_pairnorm_filter_model.py tests
    if not name.startswith("range_views"):
        rc = M.model_pair_cascade(a, b, GP, R)
        for k in ("tiles", "pruned", "filtered", "work", "fallback", "wrong", "matches"):
            assert rc[k] == r2[k], (k, rc[k], r2[k])


def test_pair_norms_half_rounding():
    """the rounding rules of pairnorm_to_half, value by value"""
    x = np.zeros((8, 2), np.float32)
    x[:, 0] = [0.0, 65504.0, 65505.0, 2.0 ** -15, 2.0 ** -14, 1.0, 1.0 + 2.0 ** -10, np.nan]
    s, h = M.pair_norms(x)[:, 0], M.pair_norms_half(x)[:, 0]
    assert h[0] == 0.0
    assert h[1] == np.inf                                # (the f32 pair norm of 65,504 is one float above it: beyond the largest f16)
    assert h[2] == np.inf
    assert h[3] == 2.0 ** -14 and h[4] == 2.0 ** -14 * (1 + 2.0 ** -10)
    assert h[5] == 1.0 + 2.0 ** -10 and h[6] == 1.0 + 2.0 ** -9      # always up, never to nearest
    assert np.isnan(h[7]) and np.isnan(s[7])


def test_the_gpu_cases_hold_what_they_are_built_for():
    R = 0.36
    # the sparse views: level 1 prunes every far tile, as the filter does
    for nI in (33, 96, 97, 160):
        for nJ in (70, 100, 130):
            a, b = FC.sparse_views(nI, nJ, seed=nI * 1000 + nJ)
            r = M.model_pair_levels(a, b, GP, R)
            n = ((nJ + 63) // 64) * ((nI + 31) // 32 - 1)
            assert r["half"] == r["filtered"] == r["pruned"] == n, r
    # threshold_views("pruned"): the filter prunes the planted row's tile, level 1 does not -- the case that separates the levels
    a, b, q, row, T, s = FC.threshold_views(M, "pruned")
    LB, slack = M.pairnorm_bound(a, b)
    LBH, margin = M.halfnorm_bound(a, b)
    print("threshold_views pruned: f32 bound over T", LB[row, q] - T, "f16 bound over T", LBH[row, q] - T, "slack", slack[q], "margin", margin[q])
    assert LB[row, q] - LBH[row, q] > 5.0 * (slack[q] + margin[q])
    r = M.model_pair_levels(a, b, GP, R)
    assert r["filtered"] == r["pruned"] == 4 and r["half"] == 3, r
    # the rows planted against thrH
    for side, half in (("cleared", 4), ("missed", 3)):
        a, b, q, row, over, margin = HC.half_threshold_views(M, side)
        print("half_threshold_views", side, "f16 bound over thrH", over, "margin", margin)
        assert (over > 1.25 * margin) if side == "cleared" else (-0.75 * margin < over < -0.25 * margin)
        r = M.model_pair_levels(a, b, GP, R)
        assert r["wrong"] == 0 and r["fallback"] == 0 and r["filtered"] == r["pruned"] == 4 and r["half"] == half, (side, r)
    # the range cases
    a, b = HC.range_views("scaled_up")
    assert np.isinf(M.pair_norms_half(a)[M.pair_norms(a) != 0]).all()
    r = M.model_pair_levels(a, b, GP, R)
    assert r["half"] == 0 and r["filtered"] == r["pruned"] == 3 * 3, r
    a, b = HC.range_views("scaled_down")
    s = M.pair_norms(a)
    assert ((s != 0) & (s < 2.0 ** -14)).any() and (M.pair_norms_half(a)[s != 0] >= 2.0 ** -14).all()
    r = M.model_pair_levels(a, b, GP, R)
    assert r["half"] <= r["filtered"] == r["pruned"] == 3 * 3, r
    a, b = HC.range_views("huge_row")
    h = M.pair_norms_half(a)
    assert np.isinf(h[50]).any() and np.isfinite(h[np.arange(len(a)) != 50]).all()
    r = M.model_pair_levels(a, b, GP, R)
    assert r["wrong"] == 0 and r["half"] <= r["filtered"], r
    a, b = HC.range_views("nan")
    r = M.model_pair_levels(a, b, GP, R)
    assert r["half"] == r["filtered"] == r["pruned"] == 2 * 3, r
    a, b = HC.range_views("negative")
    r = M.model_pair_levels(a, b, GP, R)
    assert r["half"] == r["filtered"] == r["pruned"] == 3 * 3, r
