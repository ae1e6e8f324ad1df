"""The 2-NN certificate where rounding error meets the gaps (tests/certificate_cases.py; placement proved on the CPU by
tests/test_certificate_cases.py): every case through r3dm_knn2 on the path it names, one case per family through an index, the
match-mode collections through r3dm_match_pairs on both paths.

Bars: BIT-EXACT 2-NN indices and float distances against the CPU restatement of the reference (as tests/test_gpu_parity.py), graphs
equal to the oracle's and to each other, the counters of the intended kernel, and exact-scan fractions that show the sweep crosses
the certificate's transition on the device as it does in the emulation.  The last test shows that the cases have teeth: the
developer build with the slack factor scaled to zero (R3DM_CERT_SLACK_PERMILLE=0) returns wrong 2-NN on them.
"""
import os
import subprocess
import sys
import tempfile
import textwrap

import numpy as np
import pytest

import certificate_cases as CC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_RAN = {}            # name -> exact-scan fraction of the case's knn2 call


def _graph_equal(g, pairs, counts, matches):           # as tests/test_gpu_parity.py
    d = g.as_dict()
    off = 0
    exp = {}
    for p, (I, J) in enumerate(pairs):
        if counts[p]:
            exp[(int(I), int(J))] = matches[off:off + counts[p]]
        off += counts[p]
    assert set(d.keys()) == set(exp.keys())
    for k in exp:
        assert np.array_equal(d[k], exp[k]), f"pair {k}"


@pytest.fixture()
def cctx(ctx):
    yield ctx
    ctx.set_split_mfma(False)
    ctx.clear_images()


def _assert_path(s, path, name):
    want = {"f32": (0, 0), "split": (1, 0), "counts": (1, 1)}[path]
    assert (s.n_split_mfma, s.n_counts_mfma) == want and s.n_integer_mfma == 0, (name, path, s.n_split_mfma, s.n_counts_mfma)


def _run_case(ctx, oracle, name):
    case = CC.CASES[name]
    a, b = case.make()
    ctx.set_split_mfma(case.path != "f32")
    idx, dist = ctx.knn2(a, b)
    s = ctx.stats()
    _assert_path(s, case.path, name)
    frac = s.n_exact_fallback / len(b)                  # (r3dm_knn2 leaves its own count of exact-scan queries in the statistics)
    print(f"{name:44s} {case.path:6s} {case.regime:10s} exact-scan fraction {frac:.3f}")
    oidx, odist = oracle.knn2(a, b)
    assert np.array_equal(dist, odist), name
    assert np.array_equal(idx, oidx), name
    # the share of exact-scan queries lies in the band that the CPU proof gives the case (Case.device_band): a slack that is too
    # small, reads a norm of the wrong view or misses a row certifies what it must not long before any 2-NN goes wrong
    # (tests/test_certificate_cases.py::test_mixed_norm_cases_notice_a_slack_from_the_wrong_view), and one that is too large
    # sends easy queries to the exact scan
    lo, hi = case.device_band()
    if case.regime == "transition":
        assert (lo == 0.0 or lo < frac) and frac < hi, (name, frac, lo, hi)          # (exclusive ends, as on the CPU)
    else:
        assert lo <= frac <= hi, (name, frac, lo, hi)
    _RAN[name] = frac
    return frac


@pytest.mark.parametrize("name", list(CC.CASES))
def test_knn2_is_the_oracles_on_the_path_the_case_names(cctx, oracle, name):
    _run_case(cctx, oracle, name)


def test_exact_scan_fractions_cross_the_transition_on_every_path(cctx, oracle):
    """the first case of a path certifies (almost) everything, the last (almost) nothing, and at least two lie in between"""
    for path in CC.PATHS:
        names = [n for n, c in CC.CASES.items() if c.path == path]
        frac = {n: _RAN[n] if n in _RAN else _run_case(cctx, oracle, n) for n in names}
        between = [n for n in names if 0.1 < frac[n] < 0.9]
        print(path, "first", frac[names[0]], "last", frac[names[-1]], "between 0.1 and 0.9:", len(between), "largest", max(frac.values()))
        assert frac[names[0]] < 0.05, (path, names[0], frac[names[0]])
        assert frac[names[-1]] > 0.95, (path, names[-1], frac[names[-1]])
        assert len(between) >= 2, (path, between)


@pytest.mark.parametrize("name", ["offset_f32_d128_t20", "offset_split_d144_t10", "mixed_large_last_f32", "mixed_half_split_t10",
                                  "ladder_opposite_halves_f32", "ladder_last_partial_tile_split", "counts_t40_top40", "split_off_lattice_t40_top20"])
def test_index_search_is_the_oracles(cctx, oracle, name):
    """r3dm_index_create / r3dm_index_knn2: the dataset staged once (its max||a||^2 with it), two searches"""
    case = CC.CASES[name]
    a, b = case.make()
    cctx.set_split_mfma(case.path != "f32")
    ix = cctx.index_create(a)
    try:
        oidx, odist = oracle.knn2(a, b)
        for lo, hi in ((0, len(b)), (len(b) // 3, len(b) // 3 + 7)):
            idx, dist = cctx.index_knn2(ix, b[lo:hi])
            _assert_path(cctx.stats(), case.path, name)
            assert np.array_equal(dist, odist[lo:hi]) and np.array_equal(idx, oidx[lo:hi]), (name, lo, hi)
    finally:
        del ix


@pytest.mark.parametrize("name", list(CC.collections()))
def test_match_mode_graphs_are_the_oracles_on_both_paths(cctx, oracle, name):
    """r3dm_match_pairs reaches `no_match` and the tie-acceptance rule; squared metric, four ratios, f32 tiles and split / count tiles"""
    views, pairs = CC.collections()[name]
    graphs = {}
    for split in (False, True):
        cctx.clear_images()
        cctx.set_split_mfma(split)
        for i, v in enumerate(views):
            cctx.set_image(i, v)
        for ratio in CC.RATIOS:
            g = cctx.match_pairs(pairs, ratio, True)
            s = cctx.stats()
            assert (s.n_split_mfma >= 1) == split, (name, split)
            if name.startswith("counts"):
                assert (s.n_counts_mfma >= 1) == split, name
            counts, matches = oracle.match_collection(views, None, pairs, ratio, True)
            _graph_equal(g, pairs, counts, matches)
            graphs[(split, ratio)] = (np.array(g.pairs), np.array(g.offsets), np.array(g.matches))
    for ratio in CC.RATIOS:
        for x, y in zip(graphs[(False, ratio)], graphs[(True, ratio)]):
            assert np.array_equal(x, y), (name, ratio)


_CHILD = """
    import sys
    sys.path[:0] = [{root!r}, {tests!r}]
    import numpy as np
    from regard3d_amd import api
    import certificate_cases as CC
    api.use_developer_library()
    c = api.Context(0)
    out = {{}}
    for name, case in CC.CASES.items():
        if case.regime != "teeth":
            continue
        a, b = case.make()
        c.set_split_mfma(case.path != "f32")
        idx, dist = c.knn2(a, b)
        s = c.stats()
        out[name + "/idx"] = idx; out[name + "/dist"] = dist
        out[name + "/ran"] = np.array([s.n_split_mfma, s.n_counts_mfma, s.n_exact_fallback], np.int64)
    for name, (views, pairs) in CC.collections().items():
        for split in (0, 1):
            c.clear_images(); c.set_split_mfma(bool(split))
            for i, v in enumerate(views):
                c.set_image(i, v)
            for ratio in CC.RATIOS:
                g = c.match_pairs(pairs, ratio, True)
                k = "%s/%d/%g/" % (name, split, ratio)
                out[k + "pairs"] = np.array(g.pairs); out[k + "offsets"] = np.array(g.offsets); out[k + "matches"] = np.array(g.matches)
    c.close()
    np.savez(sys.argv[1], **out)
    print("ran")
"""


def test_a_slack_of_zero_gives_wrong_results_on_the_teeth_cases(oracle):
    """The developer build scales MatchParams::err_scale by R3DM_CERT_SLACK_PERMILLE / 1000 (api_match.cpp; only verdicts depend on
    it, no address does).  At 1000 every result is the oracle's; at 0 the teeth cases return wrong 2-NN on the f32 tiles and on the
    split or count tiles -- so a certificate that lost its slack would not pass this file.  One child process per setting, one
    after the other; a child that fails stops the test.
    Measured on an MI355X at 0: 140 and 172 of 1,201 queries differ on the f32 teeth cases (D = 128, 256), 170 on the split planes',
    601 on the count tiles'; none at 1000."""
    teeth = [n for n, c in CC.CASES.items() if c.regime == "teeth"]
    expect = {n: oracle.knn2(*CC.CASES[n].make()) for n in teeth}
    code = textwrap.dedent(_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests")))
    differ = {}
    with tempfile.TemporaryDirectory() as d:
        for permille in (1000, 0):
            path = os.path.join(d, f"p{permille}.npz")
            r = subprocess.run([sys.executable, "-c", code, path], env=dict(os.environ, R3DM_CERT_SLACK_PERMILLE=str(permille)),
                               capture_output=True, text=True, timeout=300)
            assert r.returncode == 0 and "ran" in r.stdout, r.stdout[-800:] + r.stderr[-2500:]
            z = np.load(path)
            differ[permille] = {}
            for n in teeth:
                ran = z[n + "/ran"]
                assert (int(ran[0]), int(ran[1])) == {"f32": (0, 0), "split": (1, 0), "counts": (1, 1)}[CC.CASES[n].path], (n, ran)
                oidx, odist = expect[n]
                differ[permille][n] = int((np.any(z[n + "/idx"] != oidx, axis=1) | np.any(z[n + "/dist"] != odist, axis=1)).sum())
                print(f"permille {permille:4d}  {n:28s} queries that differ from the oracle: {differ[permille][n]:4d} of {len(oidx)}, "
                      f"exact scan {int(ran[2])}")
            graphs_differ = 0
            for name, (views, pairs) in CC.collections().items():
                for ratio in CC.RATIOS:
                    counts, matches = oracle.match_collection(views, None, pairs, ratio, True)
                    keep = counts > 0
                    for split in (0, 1):
                        k = "%s/%d/%g/" % (name, split, ratio)
                        same = np.array_equal(z[k + "pairs"], pairs[keep]) and np.array_equal(z[k + "matches"], matches)
                        graphs_differ += not same
                        if permille == 1000:
                            assert same, (name, split, ratio)
            print(f"permille {permille:4d}  match-mode graphs that differ from the oracle: {graphs_differ}")
            if permille == 1000:
                assert not any(differ[1000].values()), differ[1000]
    assert any(v > 0 for n, v in differ[0].items() if CC.CASES[n].path == "f32"), differ[0]
    assert any(v > 0 for n, v in differ[0].items() if CC.CASES[n].path != "f32"), differ[0]
