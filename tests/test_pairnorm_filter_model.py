"""The numpy model of the cascade (tools/prefix_prune_model.py, model_pair_cascade: the pair-norm filter in front of the prefix test)
never returns a wrong verdict, and its pair-norm bound, less the slack the kernel carries, never exceeds a distance: on a synthetic
scene, on every builder of tests/prefix_prune_cases.py and on the views of tests/pairnorm_filter_cases.py, where it also shows that
each case of tests/test_gpu_pairnorm_filter.py holds what it is built for."""
import importlib.util
import os

import numpy as np
import pytest

import pairnorm_filter_cases as FC
import prefix_prune_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("prefix_prune_model", os.path.join(ROOT, "tools", "prefix_prune_model.py"))
M = importlib.util.module_from_spec(_spec); _spec.loader.exec_module(M)

GP = 12


def _views():
    """(name, a, b, R) of every case"""
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
    for kind in ("negative", "real", "large_integers"):
        out.append((f"other_rows {kind}", *FC.other_rows(kind), 0.36))
    for side in ("pruned", "kept_above", "kept_below"):
        out.append((f"threshold_views {side}", *FC.threshold_views(M, side)[:2], 0.36))
    return out


VIEWS = _views()


@pytest.mark.parametrize("name,a,b,R", VIEWS, ids=[v[0] for v in VIEWS])
def test_bound_and_verdicts(name, a, b, R):
    """the reduced bound, less the slack, is at most the oracle distance of every (row, query); the cascade returns no wrong verdict,
    and prunes every tile the prefix test alone prunes on the same lists' thresholds or more"""
    LB, slack = M.pairnorm_bound(a, b)
    D = ((a.astype(np.float64)[:, None, :] - b.astype(np.float64)[None, :, :]) ** 2).sum(2)
    assert (LB - slack[None, :] <= D).all(), float((LB - slack[None, :] - D).max())
    assert (LB <= D * (1.0 + 2.0 ** -40) + 2.0 ** -40).all()          # ... and in exact arithmetic the bound needs no slack at all
    r = M.model_pair_cascade(a, b, GP, R)
    assert r["wrong"] == 0 and r["filtered"] <= r["pruned"] <= r["tiles"], r
    assert M.model_pair_cascade(a, b, GP, R, filter_only=True)["wrong"] == 0


def test_pair_norms_round_up():
    rng = np.random.default_rng(7)
    x = np.concatenate([rng.integers(0, 256, (64, 128)).astype(np.float32), rng.standard_normal((64, 128)).astype(np.float32) * np.float32(1e-3),
                        np.zeros((1, 128), np.float32)])
    s = M.pair_norms(x).astype(np.float64)
    true = np.sqrt(x.astype(np.float64)[:, 0::2] ** 2 + x.astype(np.float64)[:, 1::2] ** 2)
    assert (s >= true).all() and (s <= true * (1.0 + 2.0 ** -22)).all() and (s[-1] == 0).all()


def test_no_wrong_verdict_on_a_synthetic_scene():
    from regard3d_amd import synth
    sc = synth.make_scene(2, 1024, "sift", seed=1001)
    views = [np.asarray(d, np.float32) for d in sc.descs]
    lines = []
    acc = M.run_cascade(views, [(0, 1), (1, 0)], GP, 0.6, out=lines.append)
    print("\n".join(lines))
    plain = M.run(views, [(0, 1), (1, 0)], [GP], 0.6, out=lambda s: None)[GP]
    assert acc["wrong"] == 0 and acc["queries"] == 2048 and acc["matches"] == plain["matches"] > 100, acc
    assert acc["pruned"] >= plain["pruned"] > 0 and acc["filtered"] > 0, (acc, plain)


def test_the_gpu_cases_hold_what_they_are_built_for():
    R = 0.36
    for nI in (33, 97):
        for nJ in (70, 130):
            a, b = FC.sparse_views(nI, nJ, seed=nI * 1000 + nJ)
            r = M.model_pair_cascade(a, b, GP, R)
            n = ((nJ + 63) // 64) * ((nI + 31) // 32 - 1)
            assert r["fallback"] == 0 and r["filtered"] == r["pruned"] == n, r
            assert M.model_pair(a, b, GP, R)["pruned"] == 0            # (a) a 96-dimension prefix alone prunes nothing: its distances are 0
    # (b) dense rows: the far tiles of base_views go at the filter already (a far row's pair norms lie 150 above a near row's in 36
    # pairs); the dense rows the filter cannot judge are those of runner_up_pruned and forced_fallback, 16,200 away in 72 dimensions
    a, b = PC.base_views(160, 130, seed=77)
    r = M.model_pair_cascade(a, b, GP, R)
    assert r["filtered"] == r["pruned"] == 12, r
    a, b, q, best, second = PC.runner_up_pruned()
    r = M.model_pair_cascade(a, b, GP, R)
    assert r["fallback"] == 0 and r["pruned"] == r["tiles"] - 2 and r["filtered"] == r["pruned"] - 2, r     # tile 1: the prefix test, both waves
    a, b, q, p, late = PC.forced_fallback()
    r = M.model_pair_cascade(a, b, GP, R)
    assert r["fallback"] == 1 and r["pruned"] == 3 and r["filtered"] == 1, r
    # (c) the swapped row's bound is 0: its tile goes on for the wave of query 7 and finishes (the far rows' prefix distances are 0)
    a, b, q, row = FC.swapped_pairs()
    LB, _ = M.pairnorm_bound(a, b)
    assert abs(LB[row, q]) < 1.0 and PC.distances(a, b)[row, q] > 20000
    r = M.model_pair_cascade(a, b, GP, R)
    assert r["fallback"] == 0 and r["filtered"] == r["pruned"] == r["tiles"] - 2 - 1, r
    # (e)
    a, b, q, row = FC.match_in_last_tile()
    r = M.model_pair_cascade(a, b, GP, R)
    assert r["fallback"] == 0 and r["filtered"] == r["pruned"] == r["tiles"] - 3 - 1, r
    a, b, q, best, second = FC.runner_up_filtered()
    order = np.argsort(PC.distances(a, b)[:, q], kind="stable")
    assert (order[0], order[1]) == (best, second)
    r = M.model_pair_cascade(a, b, GP, R)
    assert r["fallback"] == 0 and r["filtered"] == r["pruned"] == r["tiles"] - 2, r
    # (d) a NaN query: its wave prunes nothing
    a, b = FC.other_rows("nan")
    r = M.model_pair_cascade(a, b, GP, R)
    assert r["filtered"] == r["pruned"] == 2 * 3, r
    # (f) the planted row against T and the slack
    for side, pruned in (("pruned", 4), ("kept_above", 3), ("kept_below", 3)):
        a, b, q, row, T, s = FC.threshold_views(M, side)
        LB, _ = M.pairnorm_bound(a, b)
        assert abs(LB[row, q] - T) < 2.0 * s and (LB[row, q] > T) == (side != "kept_below"), (side, LB[row, q], T, s)
        r = M.model_pair_cascade(a, b, GP, R)
        assert r["wrong"] == 0 and r["fallback"] == 0 and r["filtered"] == r["pruned"] == pruned, (side, r)
