"""CPU proof that the case table of the history tests (tests/history_cases.py) is adequate, from the oracle alone: every variant sits
on the side of the branch its case names, every make() is reproducible, and every expect() is computable.  No GPU and no code
under test: the GPU library is not loaded (the arms' presets are plain numbers in history_cases)."""
import numpy as np
import pytest

import history_cases as HC

# the branch constants, as the code states them (api_filter.cpp: R3DM_FILTER_COOP_MIN; api_match.cpp: the LDS sort's keys; kernels_akaze.hip: kAkLive;
# r3dm_ctx.hpp: the arena's reuse window; kernels_guided.hip: query block and J tile; the ANN arms' minimum)
FILTER_COOP_MIN = 4096
LDS_SORT_KEYS = 16384
CLASSIC_WAVE_BOUND = 64
AK_LIVE = 3072
GUIDED_QUERY_BLOCK, GUIDED_J_TILE = 256, 8192
TILE_ROWS = 32


def test_every_case_has_both_variants_and_reproducible_inputs():
    assert len(HC.CASES) >= 25
    for name, case in HC.CASES.items():
        assert case.branch, name
        for variant in HC.VARIANTS:
            mk = getattr(case._make, "__wrapped__", case._make)        # (past the lru_cache of filter_inputs / liop_inputs: built twice from the seed)
            a = mk(variant); b = mk(variant)
            assert a.keys() == b.keys(), (name, variant)
            for k in a:
                xa = a[k] if isinstance(a[k], (list, tuple)) else [a[k]]
                xb = b[k] if isinstance(b[k], (list, tuple)) else [b[k]]
                assert all(np.array_equal(np.asarray(p), np.asarray(q)) for p, q in zip(xa, xb)), (name, variant, k)
    for fam, members in HC.FAMILIES.items():
        assert all(m in HC.CASES for m in members), fam


@pytest.mark.parametrize("name", sorted(HC.CASES))
def test_every_expect_is_computable(oracle, name):
    case = HC.CASES[name]
    for variant in HC.VARIANTS:
        for on in ([frozenset()] + ([frozenset({"guided"})] if "guided" in case.switches else [])):
            exp = case.expect(oracle, case.make(variant), on)
            if not case.fresh:
                assert exp, (name, variant)                               # a case without a fresh-context note is restated in full
            for k, v in exp.items():
                assert isinstance(v, np.ndarray), (name, variant, k)
            if variant == "large" and not on:
                assert sum(v.size for v in exp.values()) > 0, name       # the large variant has something to compare
    # the restatement is deterministic (what the GPU tests cache per session)
    a = case.expect(oracle, case.make("small")); b = case.expect(oracle, case.make("small"))
    assert not HC.differences(a, b)


def test_knn2_variants_leave_the_small_call_inside_the_large_calls_buffers():
    for kind in ("int", "real", "u8", "bin"):
        L, S = HC.CASES["knn2_" + kind].make("large"), HC.CASES["knn2_" + kind].make("small")
        for k in ("dataset", "query"):
            assert L[k].shape[0] >= 16 * S[k].shape[0] and L[k].shape[1] == S[k].shape[1]
            assert S[k].shape[0] % TILE_ROWS != 0 and L[k].shape[0] % TILE_ROWS != 0       # padding rows in the last tile of both
    assert HC.CASES["knn2_int"].make("large")["dataset"].dtype == np.float32
    d = HC.CASES["knn2_int"].make("small")["dataset"]; assert np.array_equal(d, np.rint(d))          # integer-valued: the bf16 path applies
    d = HC.CASES["knn2_real"].make("small")["dataset"]; assert not np.array_equal(d, np.rint(d))     # real-valued: the split path applies


def test_match_variants_and_the_arena_window():
    for name in ("match_sift", "match_liop", "match_akaze"):
        L, S = HC.CASES[name].make("large"), HC.CASES[name].make("small")
        assert len(L["descs"]) > len(S["descs"]) and L["descs"][0].shape[0] >= 4 * S["descs"][0].shape[0]
        assert L["descs"][0].shape[1] == S["descs"][0].shape[1]
    for big, small in HC.SHRINK_ROWS:
        # the replacing view is smaller (DevBuf::ensure keeps the replaced view's block: bytes <= cap) by at least one whole tile, so
        # tiles of the old view stay behind the new one, and it ends inside a tile, so its last tile has padding rows
        assert 0.8 <= small / big < 1.0 and -(-small // TILE_ROWS) < -(-big // TILE_ROWS) and small % TILE_ROWS != 0


def test_long_list_variants_sit_on_both_sides_of_the_lds_sort(oracle):
    c = HC.CASES["match_long_lists"]
    nl = len(c.expect(oracle, c.make("large"))["matches"]); ns = len(c.expect(oracle, c.make("small"))["matches"])
    assert nl > LDS_SORT_KEYS > ns > 1000                                  # ONE pair each: the counts are the pair's


def test_ann_variants_sit_on_both_sides_of_the_row_minimum():
    for name in ("match_kgraph", "match_hnsw", "match_mrpt"):
        L, S = HC.CASES[name].make("large"), HC.CASES[name].make("small")
        assert all(d.shape[0] >= HC.ANN_MIN_ROWS for d in L["descs"]) and all(d.shape[0] < HC.ANN_MIN_ROWS for d in S["descs"])
    for name in ("mrpt_knn2", "hnsw_knn2"):
        L, S = HC.CASES[name].make("large"), HC.CASES[name].make("small")
        assert S["dataset"].shape[0] >= HC.ANN_MIN_ROWS and L["dataset"].shape[0] > 16 * S["dataset"].shape[0]


def test_mrpt_leaves_are_nearly_empty_only_on_the_small_dataset(oracle):
    depth = HC.MRPT_PRESET["depth"]
    L, S = HC.CASES["mrpt_knn2"].make("large"), HC.CASES["mrpt_knn2"].make("small")
    for inp in (L, S):
        assert oracle.mrpt_depth_for(inp["dataset"].shape[0], depth) == depth                 # both are served at the preset's depth
    leaves = 1 << depth
    assert S["dataset"].shape[0] / leaves < 3 < 40 < L["dataset"].shape[0] / leaves              # fewer rows per leaf than votes ask for


def test_filter_variants_sit_on_both_sides_of_the_kernel_choice():
    L, S = HC.filter_inputs("large"), HC.filter_inputs("small")
    assert len(L["pairs"]) == 1 and L["counts"][0] > FILTER_COOP_MIN       # the cooperative kernel (a pair above coop_min always is)
    assert len(S["pairs"]) >= 3 and S["counts"].max() < FILTER_COOP_MIN and S["counts"].min() > 7      # one workgroup per pair
    # guided matching: several query blocks with a partial last one and two J tiles, against a single J tile
    nL, nS = L["xys"][0].shape[0], S["xys"][0].shape[0]
    assert nL > GUIDED_J_TILE and nL % GUIDED_QUERY_BLOCK != 0 and nS < GUIDED_J_TILE


def test_filter_expectations_have_support(oracle):
    for variant in HC.VARIANTS:
        inp = HC.filter_inputs(variant)
        for kind in "FE":
            e = HC.CASES["filter_" + kind].expect(oracle, inp)
            assert len(e[kind + "_pairs"]) >= 1 and len(e[kind + "_inliers"]) > 100, (variant, kind)   # the filters keep pairs: there is output to compare
    g = HC.CASES["filter_F"].expect(oracle, HC.filter_inputs("small"), frozenset({"guided"}))
    assert len(g["F_matches"]) > 100                                       # the guided switch has lists to return
    gm = HC.CASES["guided_match"]
    for variant in HC.VARIANTS:
        e = gm.expect(oracle, gm.make(variant))
        assert len(e["geom_matches"]) > 0, variant


def test_guided_candidates_straddle_the_developer_chunk_budget():
    """the product's budget of 2^28 candidates per chunk is out of reach; under DEV_KNOBS the large variant is cut into chunks"""
    import guided_restatement as G
    budget = int(HC.DEV_KNOBS["R3DM_GUIDED_CAND_BUDGET"])
    gm = HC.CASES["guided_match"]
    total = {}
    for variant in HC.VARIANTS:
        inp = gm.make(variant)
        total[variant] = sum(len(js) for (I, J), M, t in zip(inp["pairs"].tolist(), inp["models"], inp["thr"])
                             for js, _ in G.candidates("H", M, inp["xys"][I], inp["xys"][J], float(t) * float(t)))
        assert inp["xys"][0].shape[0] ** 2 < 1 << 28                      # even every (i, j) of a pair a candidate: one chunk
    print(total)                                                          # measured: large 1997, small 48
    assert total["small"] < budget and total["large"] > 4 * budget


def _strict_maxima(ldet, thr):
    c = ldet[1:-1, 1:-1]; mx = c > np.float32(thr)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            if (dy, dx) != (1, 1):
                mx &= c > ldet[dy:dy + ldet.shape[0] - 2, dx:dx + ldet.shape[1] - 2]
    return int(mx.sum())


def test_fast_detector_variants(oracle):
    L, S = HC.fast_detector_inputs("large"), HC.fast_detector_inputs("small")
    row_pixels_small = S["images"][0].shape[1]
    for im in L["images"]:
        r = oracle.akaze_detect(im, L["thr"], dbg_level=0)
        border = int(r["info"][4]); d0 = r["ldet"]
        n0 = _strict_maxima(d0[border - 1:d0.shape[0] - border + 1, border - 1:d0.shape[1] - border + 1], L["thr"])
        assert n0 > AK_LIVE and n0 > row_pixels_small                     # level 0 alone has more candidates than live-set slots
    for im in S["images"]:
        n = len(oracle.akaze_detect(im, S["thr"])["kps"])
        assert 0 < n < 200 and im.shape != L["images"][0].shape           # a handful of candidates; planes of another stride


def test_classic_detector_variants(oracle):
    """largest kpts_aux component (tests/test_akaze_classic_components.components over the restatement's candidates): both variants
    are below the wavefront bound of 64 -- no image tried reaches it, see history_cases -- and on opposite sides of DEV_KNOBS' bound"""
    import akaze_classic_restatement as R
    import test_akaze_classic_components as CC
    bound = int(HC.DEV_KNOBS["R3DM_AC_AUX_BOUND"])
    largest = {}
    for variant in HC.VARIANTS:
        inp = HC.classic_detector_inputs(variant)
        for im in inp["images"]:
            lv, _ = R.scale_space(im)
            cands = [(i, int(r), int(c), e["Ldet"][r, c]) for i, e in enumerate(lv) for r, c in R.candidates(e["Ldet"], np.float32(inp["thr"]))]
            roots = CC.components(lv, cands)
            largest.setdefault(variant, []).append(int(np.bincount(roots[roots >= 0]).max()))
    print(largest)                                                        # measured: large [10, 10], small [3, 3]
    assert max(largest["large"]) <= CLASSIC_WAVE_BOUND                    # the product library buckets every component of both variants
    assert max(largest["small"]) <= bound < min(largest["large"])        # the developer bound hands the large variant's back
    L = HC.classic_detector_inputs("large")
    assert all(len(R.detect(im, L["thr"])["kps"]) > 64 for im in L["images"])


def test_liop_variants_with_and_without_ties(oracle):
    L, S = HC.liop_inputs("large"), HC.liop_inputs("small")
    pl = oracle.liop_extract_patches(L["image"], L["kps"], 8.0); ps = oracle.liop_extract_patches(S["image"], S["kps"], 8.0)
    assert HC.patches_with_ties(pl, 700) >= 50 and HC.patches_with_ties(ps) == 0 and len(S["kps"]) == 40
    assert len(L["kps"]) > 16 * len(S["kps"])


def test_features_variants(oracle):
    L, S = HC.features_inputs("large"), HC.features_inputs("small")
    nl = [len(oracle.akaze_detect(im, L["thr"])["kps"]) for im in L["images"]]
    ns = [len(oracle.akaze_detect(im, S["thr"])["kps"]) for im in S["images"]]
    assert min(nl) > 4 * max(ns) and min(ns) > 0
