"""Guided matching on the GPU (kernels_guided.hip; r3dm_guided_match, r3dm_set_guided_matching): `-m gpu`.

Every graph is compared, pairs, offsets and matches, with the CPU restatement tests/guided_restatement.py, which decides each
candidate with the oracle library's own error and distance functions and takes the filters' models from orc_acransac_*."""
import os

import numpy as np
import pytest

import guided_restatement as G
from regard3d_amd import api, synth

pytestmark = pytest.mark.gpu


def _register(ctx, sc, binary=False, u8=False, K=True):
    ctx.clear_images()
    for i in range(sc.n_images):
        d = sc.descs[i].astype(np.uint8) if u8 else sc.descs[i]
        ctx.set_image(i, d, sc.xys[i], int(sc.widths[i]), int(sc.heights[i]), binary=binary)
        if K:
            ctx.set_intrinsics(i, synth.intrinsics())


def _graph_equal(g, pairs, offsets, matches):
    assert np.array_equal(g.pairs, np.asarray(pairs, np.uint32).reshape(-1, 2))
    assert np.array_equal(g.offsets.astype(np.uint64), np.asarray(offsets, np.uint64))
    assert np.array_equal(g.matches, np.asarray(matches, np.uint32).reshape(-1, 2))


def _restated(kind, sc, pairs, models, thrs, ratio, descs, binary):
    out_p, out_o, out_m = [], [0], []
    for (I, J), M, t in zip(pairs.tolist(), models, thrs):
        m = G.guided_pair(kind, M, t, ratio, sc.xys[I], sc.xys[J], descs[I], descs[J], binary, synth.intrinsics(), synth.intrinsics())
        if len(m):
            out_p.append((I, J)); out_m.append(m); out_o.append(out_o[-1] + len(m))
    return out_p, out_o, (np.concatenate(out_m) if out_m else np.zeros((0, 2), np.uint32))


def _candidate_count(kind, sc, pairs, models, thrs):
    """what r3dm_guided_report's n_candidates must be: every (i, j) with err < errTh of every pair, in either mode"""
    return sum(G.candidate_count(kind, M, t, sc.xys[I], sc.xys[J], synth.intrinsics(), synth.intrinsics())
               for (I, J), M, t in zip(np.asarray(pairs).tolist(), models, thrs))


def _accepted(ctx, g, kind):
    """the accepted pairs of one filter, their models and thresholds (r3dm_pair_report of the putative pairs)"""
    f = {"F": ctx.filter_F, "H": ctx.filter_H, "E": ctx.filter_E}[kind]
    gf, M = f(g, **{"want_" + kind: True})
    rep = ctx.filter_report()
    where = {(int(I), int(J)): k for k, (I, J) in enumerate(g.pairs)}
    thr = np.array([rep[where[(int(I), int(J))]][0] for I, J in gf.pairs], np.float64)
    return gf, M, thr


@pytest.mark.parametrize("desc", ["sift", "sift_u8", "liop", "akaze"])
def test_guided_match_equals_the_restatement(ctx, desc):
    """r3dm_guided_match with the library's own models and thresholds, F / E / H, descriptor and geometry-only mode; view sizes that
    are no multiple of 256 (the query block) or of the J tile"""
    kind = "akaze" if desc == "akaze" else ("liop" if desc == "liop" else "sift")
    sc = synth.make_scene(4, 1000, kind, seed=4141)
    binary = desc == "akaze"
    _register(ctx, sc, binary=binary, u8=desc == "sift_u8")
    descs = [d.astype(np.uint8) for d in sc.descs] if desc == "sift_u8" else sc.descs
    pairs = sc.exhaustive_pairs()
    g = ctx.match_pairs(pairs, 0.8 if binary else 0.6, not binary)
    checked = 0
    for kind_f in ("F", "E", "H"):
        gf, M, thr = _accepted(ctx, g, kind_f)
        if gf.num_pairs == 0:
            continue
        n_cand = _candidate_count(kind_f, sc, gf.pairs, M, thr)
        for ratio in ((0.8 if binary else 0.6), -1.0):
            got = ctx.guided_match(gf, kind_f, M, thr, ratio)
            _graph_equal(got, *_restated(kind_f, sc, gf.pairs, M, thr, ratio, descs, binary))
            rep = ctx.guided_report()
            assert rep["n_pairs"] == gf.num_pairs and rep["n_queries"] == sum(sc.xys[int(I)].shape[0] for I, _ in gf.pairs)
            assert rep["n_candidates"] == n_cand and rep["n_matches"] == got.num_matches and rep["ms_kernels"] > 0
            checked += 1
    assert checked >= 4
    # a homography chosen by the caller (a translation by the mean displacement, 8 px), both modes: the primitive takes any model
    d = np.array([np.mean(sc.xys[int(J)][m[:, 1]] - sc.xys[int(I)][m[:, 0]], axis=0) for (I, J), m in g.as_dict().items()])
    Hs = np.array([[1, 0, dx, 0, 1, dy, 0, 0, 1] for dx, dy in d], np.float64)
    thr = np.full(g.num_pairs, 8.0)
    n_cand = _candidate_count("H", sc, g.pairs, Hs, thr)
    for ratio in ((0.8 if binary else 0.6), -1.0):
        got = ctx.guided_match(g.pairs, "H", Hs, thr, ratio)
        _graph_equal(got, *_restated("H", sc, g.pairs, Hs, thr, ratio, descs, binary))
        assert ctx.guided_report()["n_candidates"] == n_cand


def test_full_size_pair_and_tiled_J(ctx):
    """one 8,192 x 8,192 pair (two LDS tiles of J positions) and a 9,000-feature J (three, the last one partial)"""
    for n in (8192, 9000):
        sc = synth.make_scene(2, n, "sift", seed=777 + n)
        _register(ctx, sc)
        g = ctx.match_pairs(sc.exhaustive_pairs(), 0.6, True)
        gf, M, thr = _accepted(ctx, g, "F")
        assert gf.num_pairs == 1
        n_cand = _candidate_count("F", sc, gf.pairs, M, thr)
        for ratio in (0.6, -1.0):
            got = ctx.guided_match(gf, "F", M, thr, ratio)
            _graph_equal(got, *_restated("F", sc, gf.pairs, M, thr, ratio, sc.descs, False))
            assert ctx.guided_report()["n_candidates"] == n_cand
        assert got.num_matches > 0


def _putative_csr(g):
    return g.pairs, g.offsets.astype(np.int64), g.matches


@pytest.mark.parametrize("desc", ["liop", "akaze"])
def test_filters_with_the_switch_equal_acransac_plus_restatement(ctx, desc):
    binary = desc == "akaze"
    sc = synth.make_scene(5, 700, desc, seed=5151)
    _register(ctx, sc, binary=binary)
    Ks = [synth.intrinsics()] * sc.n_images
    g = ctx.match_pairs(sc.exhaustive_pairs(), 0.8 if binary else 0.6, not binary)
    p, o, m = _putative_csr(g)
    ratios = {"F": 0.6, "E": 0.6, "H": -1.0}
    plain = {"F": ctx.filter_F(g, want_F=True), "E": ctx.filter_E(g, want_E=True), "H": ctx.filter_H(g, want_H=True)}
    ctx.set_guided_matching(True, ratios["F"], ratios["E"], ratios["H"])
    try:
        singles = {"F": ctx.filter_F(g, want_F=True), "E": ctx.filter_E(g, want_E=True), "H": ctx.filter_H(g, want_H=True)}
        feh, _, _ = ctx.filter_FEH(g, "FEH")
    finally:
        ctx.set_guided_matching(False)
    for kind in "FEH":
        rp, ro, rm, rM = G.guided_filter(kind, sc.descs, sc.xys, sc.widths, sc.heights, p, o, m, ratios[kind], Ks=Ks, binary=binary)
        gk, Mk = singles[kind]
        _graph_equal(gk, rp, ro, rm)
        _graph_equal(feh[kind], rp, ro, rm)
        # the models stay AC-RANSAC's: the plain filter's model of every pair the guided graph keeps
        g0, M0 = plain[kind]
        row = {(int(I), int(J)): k for k, (I, J) in enumerate(g0.pairs)}
        for q, (I, J) in enumerate(gk.pairs):
            assert Mk[q].tobytes() == M0[row[(int(I), int(J))]].tobytes()
    assert singles["F"][0].num_pairs > 0 and singles["E"][0].num_pairs > 0


def test_switch_on_then_off_leaves_every_filter_output_unchanged():
    sc = synth.make_scene(5, 900, "sift", seed=6161)
    outs = []
    for toggle in (False, True):
        c = api.Context(0)
        try:
            _register(c, sc)
            c.set_device_graphs(True)
            g = c.match_pairs(sc.exhaustive_pairs(), 0.6, True)
            if toggle:
                c.set_guided_matching(True)
                gg = c.filter_F(g)
                assert gg.on_device == 0 and gg.num_pairs > 0
                c.set_guided_matching(False)
            r = {}
            for kind in "FEH":
                gk, Mk = {"F": c.filter_F, "E": c.filter_E, "H": c.filter_H}[kind](g, **{"want_" + kind: True})
                r[kind] = (gk.pairs.copy(), gk.offsets.copy(), gk.matches.copy(), Mk.tobytes(), c.filter_report())
            feh, _, _ = c.filter_FEH(g, "FEH")
            r["FEH"] = [(feh[k].pairs.copy(), feh[k].offsets.copy(), feh[k].matches.copy()) for k in "FEH"]
            outs.append(r)
        finally:
            c.close()
    a, b = outs
    for kind in "FEH":
        for x, y in zip(a[kind][:3], b[kind][:3]):
            assert x.tobytes() == y.tobytes()
        assert a[kind][3] == b[kind][3] and a[kind][4] == b[kind][4]
    for x3, y3 in zip(a["FEH"], b["FEH"]):
        for x, y in zip(x3, y3):
            assert x.tobytes() == y.tobytes()


def _feat_xy(path):
    return np.loadtxt(path, dtype=np.float32).reshape(-1, 4)[:, :2].copy()


def _desc(path):
    raw = np.fromfile(path, np.uint8)
    return np.frombuffer(raw[8:].tobytes(), np.float32).reshape(-1, 144)


@pytest.mark.parametrize("devices", [[0], [0, 0]])
def test_stage_flag_files_equal_the_restatement(oracle, tmp_path, devices):
    """computeMatches with setGuidedMatching(true) (R3DM_STAGE_GUIDED_MATCHING), one device and a device list: matches.f / e / h
    byte-equal to the files the restatement's graphs give through r3dm_save_matches"""
    h, w = 240, 320
    ims, K = synth.make_photo_set(3, h, w, seed=5, device="cpu")
    ims = [np.ascontiguousarray(im.numpy(), np.float32) for im in ims]
    views = [dict(id=k, width=w, height=h, basename=f"g{k}", gray=ims[k], focal_px=K[0, 0], ppx=K[0, 2], ppy=K[1, 2]) for k in range(3)]
    d = str(tmp_path / "on"); os.makedirs(d)
    rep = api.compute_matches_stage(devices, d, views, 0.001, 0.6, 9, True, True, True, 5489, 1, 2, guided=True)
    put = api.Graph.load(os.path.join(d, "matches.putative.txt"))
    xys = [_feat_xy(os.path.join(d, f"g{k}.feat")) for k in range(3)]
    descs = [_desc(os.path.join(d, f"g{k}.desc")) for k in range(3)]
    Ks = [K] * 3
    W = np.full(3, w, np.uint32); H = np.full(3, h, np.uint32)
    p, o, m = put.pairs, put.offsets.astype(np.int64), put.matches
    for kind, ratio, name in (("F", 0.6, "f"), ("E", 0.6, "e"), ("H", -1.0, "h")):
        rp, ro, rm, _ = G.guided_filter(kind, descs, xys, W, H, p, o, m, ratio, Ks=Ks)
        exp = os.path.join(str(tmp_path), f"exp.{name}.txt")
        api.Graph.from_csr(rp, ro, rm).save(exp)
        assert open(exp, "rb").read() == open(os.path.join(d, f"matches.{name}.txt"), "rb").read(), name
    assert rep.n_F_pairs > 0
    # the flag off again on a fresh call: the plain filter files
    d2 = str(tmp_path / "off"); os.makedirs(d2)
    api.compute_matches_stage(devices, d2, views, 0.001, 0.6, 9, True, True, True, 5489, 1, 2)
    oc, om = oracle.filter_F_collection(xys, W, H, p, np.diff(o), m, 4.0, 2048, 5489)
    pf, cf, mf = oracle.load_matches(os.path.join(d2, "matches.f.txt"))
    assert np.array_equal(pf, p[oc > 0]) and np.array_equal(cf, oc[oc > 0])


def test_filters_with_the_switch_on_views_without_intrinsics(ctx):
    """E has no work items when no view has r3dm_set_intrinsics: with the switch on, r3dm_filter_FEH and r3dm_filter_E still succeed, E
    comes back empty, F and H are the guided graphs"""
    sc = synth.make_scene(4, 800, "liop", seed=7171)
    _register(ctx, sc, K=False)
    g = ctx.match_pairs(sc.exhaustive_pairs(), 0.6, True)
    p, o, m = _putative_csr(g)
    ratios = {"F": 0.6, "H": -1.0}
    ctx.set_guided_matching(True, 0.6, 0.6, -1.0)
    try:
        feh, _, _ = ctx.filter_FEH(g, "FEH")
        ge = ctx.filter_E(g)
        empty = ctx.filter_FEH(api.Graph.from_csr(np.zeros((0, 2), np.uint32), np.zeros(1, np.uint64), np.zeros((0, 2), np.uint32)), "FEH")[0]
    finally:
        ctx.set_guided_matching(False)
    assert feh["E"].num_pairs == 0 and ge.num_pairs == 0
    assert all(empty[k].num_pairs == 0 for k in "FEH")
    for kind in "FH":
        rp, ro, rm, _ = G.guided_filter(kind, sc.descs, sc.xys, sc.widths, sc.heights, p, o, m, ratios[kind])
        _graph_equal(feh[kind], rp, ro, rm)
    assert feh["F"].num_pairs > 0


def test_stage_flag_on_views_without_focal_length(tmp_path):
    """computeMatches with the guided flag on a collection without focal lengths (no intrinsics: E has nothing to estimate) succeeds;
    matches.f / .h are the restatement's, E keeps no pair"""
    h, w = 240, 320
    ims, _ = synth.make_photo_set(3, h, w, seed=5, device="cpu")
    ims = [np.ascontiguousarray(im.numpy(), np.float32) for im in ims]
    views = [dict(id=k, width=w, height=h, basename=f"n{k}", gray=ims[k]) for k in range(3)]
    d = str(tmp_path / "on"); os.makedirs(d)
    rep = api.compute_matches_stage([0], d, views, 0.001, 0.6, 9, True, True, True, 5489, 1, 2, guided=True)
    assert rep.n_E_pairs == 0 and rep.n_F_pairs > 0
    put = api.Graph.load(os.path.join(d, "matches.putative.txt"))
    xys = [_feat_xy(os.path.join(d, f"n{k}.feat")) for k in range(3)]
    descs = [_desc(os.path.join(d, f"n{k}.desc")) for k in range(3)]
    W = np.full(3, w, np.uint32); H = np.full(3, h, np.uint32)
    p, o, m = put.pairs, put.offsets.astype(np.int64), put.matches
    for kind, ratio, name in (("F", 0.6, "f"), ("H", -1.0, "h")):
        rp, ro, rm, _ = G.guided_filter(kind, descs, xys, W, H, p, o, m, ratio)
        exp = os.path.join(str(tmp_path), f"exp.{name}.txt")
        api.Graph.from_csr(rp, ro, rm).save(exp)
        assert open(exp, "rb").read() == open(os.path.join(d, f"matches.{name}.txt"), "rb").read(), name


def test_wide_threshold_runs_in_candidate_chunks(ctx, tmp_path):
    """A wide caller-chosen threshold: the descriptor mode runs its candidate lists in chunks below a budget.  The product's default
    budget (one chunk here) against the restatement; the developer build with R3DM_GUIDED_CAND_BUDGET (a test hook: the product library
    ignores the environment) forcing one chunk per few workgroups must give the same graph."""
    import subprocess, sys
    sc = synth.make_scene(3, 1000, "liop", seed=8181)
    _register(ctx, sc, K=False)
    pairs = sc.exhaustive_pairs()
    Hs = np.tile(np.array([1, 0, 40.0, 0, 1, 0, 0, 0, 1]), (len(pairs), 1))
    thr = np.full(len(pairs), 250.0)
    got = ctx.guided_match(pairs, "H", Hs, thr, 0.8)
    rep = ctx.guided_report()
    assert rep["n_desc_chunks"] == 1 and rep["candidates_per_query"] > 5
    _graph_equal(got, *_restated("H", sc, pairs, Hs, thr, 0.8, sc.descs, False))
    np.savez(str(tmp_path / "in.npz"), pairs=pairs, Hs=Hs, thr=thr, *sc.descs, **{f"xy{k}": sc.xys[k] for k in range(3)})
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (f"import sys; sys.path.insert(0, {root!r}); import numpy as np; from regard3d_amd import api; api.use_developer_library(); "
            f"z = np.load({str(tmp_path / 'in.npz')!r}); c = api.Context(0)\n"
            f"for k in range(3): c.set_image(k, z[f'arr_{{k}}'], z[f'xy{{k}}'], {int(sc.widths[0])}, {int(sc.heights[0])})\n"
            f"g = c.guided_match(z['pairs'], 'H', z['Hs'], z['thr'], 0.8); r = c.guided_report()\n"
            f"np.savez({str(tmp_path / 'out.npz')!r}, p=g.pairs, o=g.offsets, m=g.matches, chunks=r['n_desc_chunks'])")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, R3DM_GUIDED_CAND_BUDGET="3000"), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(str(tmp_path / "out.npz"))
    assert int(z["chunks"]) > 3
    _graph_equal(got, z["p"], z["o"], z["m"])
