"""The F / E / H filters, guided matching, the device list and the stage on pairs whose two views DIFFER: `-m gpu`.

Every other AC-RANSAC test registers views of one size with one pinhole matrix under the ids 0 .. N-1 in order, so an I/J swap of a size
or a K, a slot taken for an id, a stale size after re-registration or view 0's size used for everybody could not show in any of the
three copies of the arithmetic (acransac_body and the cooperative kernel in kernels_filter*.hip, kernels_guided.hip).  Here the
collection of filter_audit.py (7 views, 7 sizes, 6 pinhole matrices, one view without; 13 short pairs and one of 4200 putatives for the
cooperative kernel) is registered under sparse ids in an order that is neither the ids' nor the collection's, and every result is held
(a) against the CPU restatement pair by pair -- inlier sets, models to 1e-9 after normalisation and sign, iterations / models / inliers
of r3dm_filter_report -- and (b) against the pixel-space audit of filter_audit.py with the GPU's own model, threshold and NFA.

Deviations from the audit, measured over the collection at precision 4 px, 2048 iterations, seed 5489 (CPU: test_filter_audit.py, which
prints them; this module prints the GPU's).  On an MI355X the GPU's models, thresholds and NFAs came out bit-identical to the CPU
restatement's, so the two columns agree to every digit:
         worst |threshold - audit| / audit           worst |NFA - audit|
         oracle (CPU)     GPU                        oracle (CPU)          GPU
    F    1.5e-13          1.5e-13                    7.5e-4  (n = 4200)    7.5e-4
    E    4.2e-13          4.2e-13                    7.3e-4  (n = 4200)    7.3e-4
    H    2.0e-13          2.0e-13                    1.05e-3 (n = 4200)    1.05e-3
against the tolerances 1e-9 (threshold, relative) and filter_audit.nfa_tolerance(n) = 2^-24 n (log10 C(n, n/2) + 32) + 1e-4 (NFA: 2e-4
at n = 40, 0.043 at n = 1500, 0.32 at n = 4200), the float-table drift that the kernel's own scout budgets for.  An exchanged size
moves the NFA by tens to thousands, an exchanged K the threshold by orders of magnitude (test_filter_audit.py)."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import filter_audit as A
import filter_views_cases as V
import guided_restatement as G
from regard3d_amd import api, synth
from stage_cases import _oracle_stage

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

IDS = [5, 2, 11, 7, 3, 19, 8]              # view id of collection view 0 .. 6
ORDER = [7, 8, 5, 19, 11, 3, 2]            # registration order (ids): neither ascending nor the collection's, so slot != id != position
# a smaller scene for the guided-matching checks (their CPU restatement visits every feature of both views)
SMALL = dict(n_cloud=600, n_plane=400, spec=[(0, 3, 300, 0.4), (3, 0, 250, 0.7), (5, 6, 250, 0.4), (6, 2, 200, 0.7), (1, 0, 250, 0.4),
                                               (2, 5, 300, 0.4), (4, 1, 150, 0.4)])


def _descriptors(col, seed=9):
    """small random integer descriptors, feature k of every view a noisy copy of one row k (the filters ignore them; guided matching's
    ratio mode reads them)"""
    rng = np.random.default_rng(seed)
    n = len(next(iter(col.views.values()))["xy"])
    base = rng.integers(0, 16, (n, 16))
    return {i: np.clip(base + rng.integers(-1, 2, base.shape), 0, 15).astype(np.float32) for i in sorted(col.views)}


def _register(c, col, descs, order=ORDER):
    c.clear_images()
    for i in order:
        v = col.views[i]
        c.set_image(i, descs[i], v["xy"], v["w"], v["h"])
        if v["K"] is not None:
            c.set_intrinsics(i, v["K"])


def _graph(col):
    return api.Graph.from_csr(col.pairs, col.offsets, col.matches)


@pytest.fixture(scope="module")
def col():
    return A.make_collection(IDS)


@pytest.fixture(scope="module")
def descs(col):
    return _descriptors(col)


@pytest.fixture(scope="module")
def expected(oracle, col):
    return {kind: V.expected(oracle, col, kind) for kind in "FEH"}


def _filter(c, kind, g, precision=4.0, max_iter=2048, seed=5489, min_count=50, min_ratio=0.3):
    """-> (graph, models of its pairs, r3dm_filter_report of the putative pairs)"""
    if kind == "E":
        gk, M = c.filter_E(g, precision, max_iter, seed, min_count, min_ratio, want_E=True)
    else:
        gk, M = (c.filter_F if kind == "F" else c.filter_H)(g, precision, max_iter, seed, **{"want_" + kind: True})
    return gk, M, c.filter_report()


def _same(a, b):
    return a.pairs.tobytes() == b.pairs.tobytes() and a.offsets.tobytes() == b.offsets.tobytes() and a.matches.tobytes() == b.matches.tobytes()


def _check(col, kind, got, exp, precision=4.0, worst=None):
    """parity with the CPU restatement pair by pair, and the audit of every kept pair with the GPU's model, threshold and NFA; -> kept"""
    gk, M, rep = got
    d = gk.as_dict()
    assert len(rep) == len(col.pairs)
    q = 0
    for p, e in enumerate(exp):
        I, J, mm, _, _ = col.putatives(p)
        if e is None or not e["kept"]:
            assert (I, J) not in d, (kind, I, J)
        if e is None:
            continue
        assert tuple(rep[p][2:]) == (e["iterations"], e["models"], e["n_inliers"]), (kind, I, J, rep[p], e["iterations"], e["models"], e["n_inliers"])
        if not e["kept"]:
            continue
        assert tuple(gk.pairs[q]) == (I, J), (kind, I, J)
        rows = V.rows_of(mm, d[(I, J)])
        assert set(rows.tolist()) == set(e["inliers"].tolist()), (kind, I, J, len(rows), len(e["inliers"]))
        a = M[q] / np.linalg.norm(M[q]); b = e["model"] / np.linalg.norm(e["model"])
        assert min(np.linalg.norm(a - b), np.linalg.norm(a + b)) < 1e-9, (kind, I, J)
        r = V.audit_pair(col, kind, p, precision, M[q], rows, rep[p][0], rep[p][1])
        if worst is not None:
            worst["threshold_rel"] = max(worst.get("threshold_rel", 0.0), r["threshold_rel"])
            worst["nfa_abs"] = max(worst.get("nfa_abs", 0.0), r["nfa_abs"])
        q += 1
    assert q == gk.num_pairs
    return q


def test_filters_on_views_that_differ(ctx, oracle, col, descs, expected):
    _register(ctx, col, descs)
    g = _graph(col)
    singles = {}
    for kind in "FEH":
        singles[kind] = _filter(ctx, kind, g)
        assert ctx.stats().n_filter_coop_pairs == 1, "the long pair runs on the cooperative kernel"
        worst = {}
        kept = _check(col, kind, singles[kind], expected[kind], worst=worst)
        print(kind, "GPU vs audit, worst over", kept, "pairs:", worst)
        assert kept >= (9 if kind == "E" else 12)
        assert (IDS[5], IDS[2]) in singles[kind][0].as_dict(), "the long pair is kept"
    # E without Regard3D's overlap rule keeps the short pairs that the rule drops
    loose = V.expected(oracle, col, "E", min_count=0, min_ratio=0.0)
    assert _check(col, "E", _filter(ctx, "E", g, min_count=0, min_ratio=0.0), loose) > singles["E"][0].num_pairs
    # pairs that touch the view without intrinsics have no E entry, with or without the rule
    assert all(IDS[A.NO_K_VIEW] not in k for k in singles["E"][0].as_dict())
    assert sum(IDS[A.NO_K_VIEW] in k for k in singles["F"][0].as_dict()) == 2
    # the three side by side: the graphs of the single calls, the long pair of each on the cooperative kernel
    feh, _, _ = ctx.filter_FEH(g, "FEH")
    assert ctx.stats().n_filter_coop_pairs == 3
    for kind in "FEH":
        assert _same(feh[kind], singles[kind][0]), kind
    assert ctx.filter_report() == singles["E"][2]


def test_the_checks_notice_a_size_that_belongs_to_another_view(ctx, col, descs, expected):
    """The power of _check, on the GPU itself: the library is told view 0's size for every view (what a kernel reading slot 0 for
    everybody would compute), and then the sizes of two views exchanged; parity and audit against the true sizes must fail for F, E and H."""
    g = _graph(col)
    a, b = IDS[0], IDS[3]
    swapped = dict(col.views); swapped[a] = dict(col.views[a], w=col.views[b]["w"], h=col.views[b]["h"]); swapped[b] = dict(col.views[b], w=col.views[a]["w"], h=col.views[a]["h"])
    for views in ({i: dict(v, w=col.views[a]["w"], h=col.views[a]["h"]) for i, v in col.views.items()}, swapped):
        _register(ctx, A.Collection(views, col.pairs, col.counts, col.matches), descs)
        for kind in "FEH":
            with pytest.raises(AssertionError):
                _check(col, kind, _filter(ctx, kind, g), expected[kind])


def test_a_view_registered_again_with_another_size(ctx, oracle, col, descs):
    """Intrinsics survive a re-registration (r3dm_set_intrinsics is per view id), the size must not: view 7 (640 x 480) comes back as a
    1600 x 1200 view with new positions and no new r3dm_set_intrinsics call.  Then the collection is cleared and registered without
    that view's K: its pairs leave E."""
    _register(ctx, col, descs)
    g = _graph(col)
    before = {kind: _filter(ctx, kind, g)[0] for kind in "FEH"}
    vid = IDS[3]
    rng = np.random.default_rng(5)
    old = col.views[vid]
    X = A.make_points(77 + 1)                                                    # the collection's points (make_collection's default seed)
    xy = (A.project(3, X) + rng.normal(0, 0.4, (len(X), 2))).astype(np.float32)  # the old camera again, declared as a larger sensor
    views = dict(col.views); views[vid] = dict(w=1600, h=1200, K=old["K"], xy=xy)
    col2 = A.Collection(views, col.pairs, col.counts, col.matches)
    ctx.set_image(vid, descs[vid], xy, 1600, 1200)
    touched = 0
    for kind in "FEH":
        got = _filter(ctx, kind, g)
        _check(col2, kind, got, V.expected(oracle, col2, kind))
        touched += sum(vid in k for k in got[0].as_dict())
        assert not _same(got[0], before[kind]), kind
    assert touched >= 6
    views3 = dict(views); views3[vid] = dict(views[vid], K=None)
    col3 = A.Collection(views3, col.pairs, col.counts, col.matches)
    _register(ctx, col3, descs)
    got = _filter(ctx, "E", g)
    assert _check(col3, "E", got, V.expected(oracle, col3, "E")) >= 4
    assert all(vid not in k and IDS[A.NO_K_VIEW] not in k for k in got[0].as_dict())


def _short(col, longest=600):
    return col.subset(np.flatnonzero(col.counts <= longest))


@pytest.mark.parametrize("precision,max_iter,seed", [(0.5, 2048, 5489), (50.0, 2048, 5489), (1e7, 2048, 5489), (float("inf"), 2048, 5489),
                                                     (4.0, 1, 5489), (4.0, 9, 5489), (4.0, 10, 5489), (4.0, 11, 5489), (4.0, 64, 5489),
                                                     (4.0, 2048, 0), (4.0, 2048, 2 ** 40 + 1)])
def test_parameter_edges(ctx, oracle, col, descs, precision, max_iter, seed):
    """precision 1e7: the normalised bound exceeds the histogram's 1e6 clamp while still finite; max_iter < 10: the reserve max_iter / 10
    is 0; seeds beyond 32 bits.  (precision 4, 2048 iterations, seed 5489 is test_filters_on_views_that_differ.)"""
    sub = _short(col)
    _register(ctx, col, descs)
    g = _graph(sub)
    kept = 0
    for kind in "FEH":
        exp = V.expected(oracle, sub, kind, precision, max_iter, seed)
        kept += _check(sub, kind, _filter(ctx, kind, g, precision, max_iter, seed), exp, precision)
    assert kept >= (20 if max_iter == 2048 else 9)


def _deal(counts, W):
    """r3dm_multi_filter_*'s deal of the putative pairs: by descending length in snake order, ascending inside every context"""
    order = np.argsort(-np.asarray(counts, np.int64), kind="stable")
    idx = [[] for _ in range(W)]
    for pos, p in enumerate(order):
        rnd, off = divmod(pos, W)
        idx[W - 1 - off if rnd & 1 else off].append(int(p))
    return [sorted(i) for i in idx]


def test_device_list_equals_the_single_context(ctx, col, descs):
    _register(ctx, col, descs)
    g = _graph(col)
    one = {kind: _filter(ctx, kind, g) for kind in "FEH"}
    m = api.MultiContext([0, 0, 0])
    try:
        _register_multi(m, col, descs)
        deal = _deal(col.counts, 3)
        for kind, fn in (("F", m.filter_F), ("E", m.filter_E), ("H", m.filter_H)):
            gk, M = fn(g, **{"want_" + kind: True})
            assert _same(gk, one[kind][0]) and M.tobytes() == one[kind][1].tobytes(), kind
            rep = [None] * len(col.pairs)
            for k in range(3):
                c = m._L.r3dm_multi_ctx(m._h, k)
                n = m._L.r3dm_filter_report(c, None, 0)
                assert n == len(deal[k])
                arr = (api.PairReport * max(n, 1))()
                m._L.r3dm_filter_report(c, arr, n)
                for p, r in zip(deal[k], arr[:n]):
                    rep[p] = (r.threshold_px, r.nfa, r.iterations, r.models, r.inliers)
            assert rep == one[kind][2], kind
    finally:
        m.close()


def _register_multi(m, col, descs):
    for i in ORDER:
        v = col.views[i]
        m.set_image(i, descs[i], v["xy"], v["w"], v["h"])
        if v["K"] is not None:
            m.set_intrinsics(i, v["K"])


@pytest.fixture(scope="module")
def small():
    return A.make_collection(IDS, **SMALL)


def _graph_equal(g, pairs, offsets, matches):
    assert np.array_equal(g.pairs, np.asarray(pairs, np.uint32).reshape(-1, 2))
    assert np.array_equal(g.offsets.astype(np.uint64), np.asarray(offsets, np.uint64))
    assert np.array_equal(g.matches, np.asarray(matches, np.uint32).reshape(-1, 2))


def test_guided_match_with_each_views_own_K(ctx, small):
    """r3dm_guided_match with the filters' models and thresholds: E forms F = K_J^-T E K_I^-1 from the two views' own matrices"""
    d = _descriptors(small, 10)
    _register(ctx, small, d)
    g = _graph(small)
    xy = {i: v["xy"] for i, v in small.views.items()}
    checked = 0
    for kind in "FEH":
        gk, M, rep = _filter(ctx, kind, g)
        row = {tuple(int(x) for x in pr): p for p, pr in enumerate(small.pairs)}
        thr = np.array([rep[row[tuple(int(x) for x in pr)]][0] for pr in gk.pairs])
        assert gk.num_pairs >= 4
        for ratio in (0.6, -1.0):
            got = ctx.guided_match(gk, kind, M, thr, ratio)
            out_p, out_o, out_m = [], [0], []
            for (I, J), Mq, t in zip(gk.pairs.tolist(), M, thr):
                mm = G.guided_pair(kind, Mq, t, ratio, xy[I], xy[J], d[I], d[J], False, small.views[I]["K"], small.views[J]["K"])
                if len(mm):
                    out_p.append((I, J)); out_m.append(mm); out_o.append(out_o[-1] + len(mm))
            _graph_equal(got, out_p, out_o, np.concatenate(out_m))
            assert got.num_matches > 0
            checked += 1
    assert checked == 6


def test_guided_switch_on_views_that_differ(ctx, small):
    d = _descriptors(small, 10)
    _register(ctx, small, d)
    g = _graph(small)
    xy = {i: v["xy"] for i, v in small.views.items()}
    W = {i: v["w"] for i, v in small.views.items()}; H = {i: v["h"] for i, v in small.views.items()}
    Ks = {i: v["K"] for i, v in small.views.items()}
    ratios = {"F": 0.6, "E": 0.6, "H": -1.0}
    ctx.set_guided_matching(True, ratios["F"], ratios["E"], ratios["H"])
    try:
        got = {kind: _filter(ctx, kind, g) for kind in "FEH"}
        feh, _, _ = ctx.filter_FEH(g, "FEH")
    finally:
        ctx.set_guided_matching(False)
    for kind in "FEH":
        rp, ro, rm, rM = G.guided_filter(kind, d, xy, W, H, small.pairs, small.offsets.astype(np.int64), small.matches, ratios[kind], Ks=Ks)
        _graph_equal(got[kind][0], rp, ro, rm)
        _graph_equal(feh[kind], rp, ro, rm)
        assert len(rp) >= 3, kind


def test_developer_check_mode_on_views_that_differ(ctx, col, descs, tmp_path):
    """The developer build with R3DM_FILTER_CHECK=1 R3DM_FILTER_SCOUT=3 skips nothing and checks every model's exact count and NFA
    against what the scout promised (invariants 8 .. 10): its reciprocal intervals and slope table are built from s2 and logalpha0,
    which had only ever been checked where s1 = s2.  No invariant is violated and the outputs are the product's, byte for byte."""
    _register(ctx, col, descs)
    g = _graph(col)
    prod = {}
    for kind in "FEH":
        gk, M, rep = _filter(ctx, kind, g)
        prod[kind] = (np.array(gk.pairs), np.array(gk.offsets), np.array(gk.matches), M, np.array(rep, np.float64))
    code = textwrap.dedent(f"""
        import sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, "tests")!r})
        import numpy as np
        from regard3d_amd import api
        api.use_developer_library()
        import filter_audit as A, test_gpu_filter_views as T
        col = A.make_collection(T.IDS)
        c = api.Context(0)
        T._register(c, col, T._descriptors(col))
        g = T._graph(col)
        for kind in "FEH":
            gk, M, rep = T._filter(c, kind, g)      # raises on a violated invariant
            np.savez(sys.argv[1] + kind + ".npz", pairs=np.array(gk.pairs), offsets=np.array(gk.offsets), matches=np.array(gk.matches), models=M,
                     report=np.array(rep, np.float64))
        print("checked")
    """)
    d = str(tmp_path) + "/"
    r = subprocess.run([sys.executable, "-c", code, d], env=dict(os.environ, R3DM_FILTER_CHECK="1", R3DM_FILTER_SCOUT="3"), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "checked" in r.stdout, r.stdout[-800:] + r.stderr[-2500:]
    for kind in "FEH":
        z = np.load(d + kind + ".npz")
        for k, ref in zip(("pairs", "offsets", "matches", "models", "report"), prod[kind]):
            assert np.array_equal(z[k], ref), (kind, k)


def test_stage_on_photographs_of_two_sizes(oracle, tmp_path):
    """computeMatches from pixels over four small photographs of two sizes (two 480 x 640, two 360 x 480 cut from the same walk along
    the plane) with two focal lengths: the F / E / H files are the CPU chain's, and what the chain finds passes the audit with the size
    and the focal length that each view declares."""
    ims, K = synth.make_photo_set(4, 480, 640, seed=33, device="cpu")
    ims = [np.ascontiguousarray(im.numpy(), np.float32) for im in ims]
    for k in (1, 3):
        ims[k] = np.ascontiguousarray(ims[k][70:430, 90:570])
    views, Ks = [], []
    for k, im in enumerate(ims):
        h, w = im.shape
        f = K[0, 0] if w == 640 else 0.85 * K[0, 0]
        ppx, ppy = 0.5 * w + 3.0 * k, 0.5 * h - 2.0 * k
        views.append(dict(id=k, width=w, height=h, basename=f"p{k}", gray=im, focal_px=f, ppx=ppx, ppy=ppy))
        Ks.append(np.array([[f, 0, ppx], [0, f, ppy], [0, 0, 1.0]]))
    d = str(tmp_path)
    rep = api.compute_matches_stage([0], d, views, 0.001, 0.6, 9, True, True, True, 5489, 2, 2)
    assert rep.images_extracted == 4
    _, _, xys, pairs, counts, matches = _oracle_stage(oracle, ims, K)
    p, c, m = oracle.load_matches(os.path.join(d, "matches.putative.txt"))
    assert np.array_equal(p, pairs[counts > 0]) and np.array_equal(c, counts[counts > 0]) and np.array_equal(m, matches)
    col = A.Collection({k: dict(w=v["width"], h=v["height"], K=Ks[k], xy=xys[k]) for k, v in enumerate(views)}, p, c, m)
    kept = {}
    for kind, name in (("F", "f"), ("E", "e"), ("H", "h")):
        exp = V.expected(oracle, col, kind)
        fp, fc, fm = oracle.load_matches(os.path.join(d, f"matches.{name}.txt"))
        rows = [q for q, e in enumerate(exp) if e is not None and e["kept"]]
        assert np.array_equal(fp, p[rows]) and np.array_equal(fc, [exp[q]["n_inliers"] for q in rows]), kind
        off = 0
        for q in rows:
            e = exp[q]
            seg = fm[off:off + e["n_inliers"]]; off += e["n_inliers"]
            mm = col.putatives(q)[2]
            assert set(V.rows_of(mm, seg).tolist()) == set(e["inliers"].tolist()), (kind, q)
            V.audit_pair(col, kind, q, 4.0, e["model"], e["inliers"], e["threshold"], e["nfa"])
        kept[kind] = len(rows)
    assert (rep.n_F_pairs, rep.n_E_pairs, rep.n_H_pairs) == (kept["F"], kept["E"], kept["H"])
    assert kept["F"] >= 3 and kept["H"] >= 3 and any(col.sizes(q)[:2] != col.sizes(q)[2:] for q in range(len(p)))
