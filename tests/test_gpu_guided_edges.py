"""Guided matching on the device (kernels_guided.hip) at the edges of its kernels: `-m gpu`.

Every case of guided_cases.py goes through r3dm_guided_match with the case's own model and threshold, in every mode the case names
(descriptor ratio and geometry only unless the case is about one of them), and is compared with guided_restatement.guided_pair with
==: pairs, offsets and matches, and r3dm_guided_report's n_queries, n_matches and n_candidates -- the one number that counts every
(i, j) the sweep accepted, so a candidate the f32 gate lost shows even where it would not have changed the chosen match.  That each
case reaches the edge it is named for is test_guided_cases.py's business (CPU)."""
import numpy as np
import pytest

import guided_cases as C
import guided_restatement as G

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, scope="module")
def _oracle(oracle):
    return oracle


def _register(ctx, views, binary=False, Ks=None):
    ctx.clear_images()
    for v, (xy, desc) in enumerate(views):
        ctx.set_image(v, desc, xy, 4000, 3000, binary=binary)
        if Ks is not None and Ks[v] is not None:
            ctx.set_intrinsics(v, Ks[v])


def _graph_equal(g, pairs, offsets, matches, what):
    assert np.array_equal(g.pairs, np.asarray(pairs, np.uint32).reshape(-1, 2)), what
    assert np.array_equal(g.offsets.astype(np.uint64), np.asarray(offsets, np.uint64)), what
    assert np.array_equal(g.matches, np.asarray(matches, np.uint32).reshape(-1, 2)), what


@pytest.mark.parametrize("case", C.CASES, ids=C.NAMES)
def test_case_equals_the_restatement(ctx, case):
    _register(ctx, [(case["xyI"], case["descI"]), (case["xyJ"], case["descJ"])], case["binary"], [case["KI"], case["KJ"]])
    n_cand = G.candidate_count(case["kind"], case["M"], case["thr_px"], case["xyI"], case["xyJ"], case["KI"], case["KJ"])
    for ratio in case["ratios"]:
        what = f"{case['name']} ratio {ratio}"
        want = G.guided_pair(case["kind"], case["M"], case["thr_px"], ratio, case["xyI"], case["xyJ"], case["descI"], case["descJ"],
                             case["binary"], case["KI"], case["KJ"])
        got = ctx.guided_match(np.array([[0, 1]], np.uint32), case["kind"], case["M"][None], [case["thr_px"]], ratio)
        rep = ctx.guided_report()
        print(f"\n{what}: candidates {rep['n_candidates']} (restatement {n_cand}), matches {rep['n_matches']} (restatement {len(want)})")
        assert rep["n_candidates"] == n_cand, what
        if len(want):
            _graph_equal(got, [[0, 1]], [0, len(want)], want, what)
        else:
            _graph_equal(got, np.zeros((0, 2)), [0], np.zeros((0, 2)), what)
        assert rep["n_pairs"] == 1 and rep["n_queries"] == len(case["xyI"]) and rep["n_matches"] == len(want), what


def test_scaled_models_give_the_unscaled_graph(ctx):
    """the epipolar error does not depend on F's scale: 1e32 (no gate), 1e-32 and 1e-40 (f32 denormals) give the graph of scale 1"""
    cases = [c for c in C.CASES if c["name"].startswith("domain_scale_")]
    assert len(cases) == 4
    _register(ctx, [(cases[0]["xyI"], cases[0]["descI"]), (cases[0]["xyJ"], cases[0]["descJ"])])
    out = []
    for c in cases:
        assert np.array_equal(c["xyJ"], cases[0]["xyJ"]) and np.array_equal(c["descJ"], cases[0]["descJ"])
        for ratio in (0.8, -1.0):
            g = ctx.guided_match(np.array([[0, 1]], np.uint32), "F", c["M"][None], [c["thr_px"]], ratio)
            out.append((c["name"], ratio, g.matches.copy(), ctx.guided_report()["n_candidates"]))
    for name, ratio, m, n in out[2:]:
        ref = out[0] if ratio == out[0][1] else out[1]
        assert np.array_equal(m, ref[2]) and n == ref[3] and len(m), (name, ratio)


def test_many_pairs_in_one_call(ctx):
    """92 jobs of 0 .. 4 workgroups: guided_job_of's search; views of one feature; an empty view as I (also the last job) and as J"""
    m = C.many_pairs_case()
    _register(ctx, m["views"])
    n_cand = sum(G.candidate_count("H", M, t, m["views"][I][0], m["views"][J][0]) for (I, J), M, t in zip(m["pairs"].tolist(), m["models"], m["thrs"]))
    n_queries = sum(len(m["views"][int(I)][0]) for I, _ in m["pairs"])
    for ratio in m["ratios"]:
        P, Off, Mm = [], [0], []
        for (I, J), M, t in zip(m["pairs"].tolist(), m["models"], m["thrs"]):
            w = G.guided_pair("H", M, t, ratio, m["views"][I][0], m["views"][J][0], m["views"][I][1], m["views"][J][1])
            if len(w):
                P.append((I, J)); Mm.append(w); Off.append(Off[-1] + len(w))
        got = ctx.guided_match(m["pairs"], "H", m["models"], m["thrs"], ratio)
        rep = ctx.guided_report()
        print(f"\nshapes_many_pairs ratio {ratio}: candidates {rep['n_candidates']} (restatement {n_cand}), pairs {got.num_pairs} of {len(m['pairs'])}")
        _graph_equal(got, P, Off, np.concatenate(Mm), f"ratio {ratio}")
        assert rep["n_pairs"] == len(m["pairs"]) and rep["n_queries"] == n_queries and rep["n_candidates"] == n_cand
        assert rep["n_matches"] == Off[-1]
