"""The numpy model of the prefix-pruning rule (tools/prefix_prune_model.py) never returns a wrong verdict: on a synthetic scene, and
on the views the GPU test of the kernel is built from (tests/prefix_prune_cases.py), where it also shows that each case holds what
it is built for -- which tiles go, which query needs the exact scan."""
import importlib.util
import os

import numpy as np

import prefix_prune_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("prefix_prune_model", os.path.join(ROOT, "tools", "prefix_prune_model.py"))
M = importlib.util.module_from_spec(_spec); _spec.loader.exec_module(M)

GPS = (9, 10, 11, 12)


def test_no_wrong_verdict_on_a_synthetic_scene():
    from regard3d_amd import synth
    sc = synth.make_scene(2, 1024, "sift", seed=1001)
    lines = []
    tot = M.run([np.asarray(d, np.float32) for d in sc.descs], [(0, 1), (1, 0)], GPS, 0.6, out=lines.append)
    print("\n".join(lines))
    for gp in GPS:
        assert tot[gp]["wrong"] == 0 and tot[gp]["queries"] == 2048 and tot[gp]["matches"] > 100, (gp, tot[gp])
    assert any(tot[gp]["pruned"] > 0 for gp in GPS)


def test_the_gpu_cases_hold_what_they_are_built_for():
    gp, R = 12, 0.36                  # the product's prefix (kPrefixGroups, r3dm_internal.hpp): the counts below are for it
    for nI, nJ in ((64, 70), (97, 130), (160, 130)):
        a, b = PC.base_views(nI, nJ, seed=nI * 1000 + nJ)
        r = M.model_pair(a, b, gp, R)
        assert r["wrong"] == 0 and r["fallback"] == 0 and r["pruned"] == ((nJ + 63) // 64) * ((nI + 31) // 32 - 1), r
    a, b, q, row = PC.match_in_last_tile()
    r = M.model_pair(a, b, gp, R)
    assert r["wrong"] == 0 and r["fallback"] == 0 and r["pruned"] == r["tiles"] - 4, r
    a, b, q, best, second = PC.runner_up_pruned()
    r = M.model_pair(a, b, gp, R)
    assert r["wrong"] == 0 and r["fallback"] == 0 and r["pruned"] == r["tiles"] - 2, r
    a, b, q, p, late = PC.forced_fallback()
    r = M.model_pair(a, b, gp, R)
    assert r["wrong"] == 0 and r["fallback"] == 1 and r["pruned"] == 3, r      # tile 1 by both waves, tile 2 by the wave that does not hold query 7
    for case, pruned in (("seen_tie", 2), ("seen_below", 2), ("pruned_at_threshold", 1), ("pruned_above", 2)):
        a, b, q, best, matched = PC.ratio_boundary(case)
        r = M.model_pair(a, b, gp, 0.25)
        assert r["wrong"] == 0 and r["fallback"] == 0 and r["pruned"] == pruned, (case, r)
