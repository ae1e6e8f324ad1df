"""The symmetric ratio test on the GPU (r3dm_set_symmetric_ratio; the ratio kernels of kernels_match_mutual.hip) -- matches and the three
counters bit for bit against the restatement built from the oracle (symmetric_ratio_restatement.py), on every arm and tile format
that collects matches into a graph.  test_symmetric_ratio_restatement.py proves on the CPU that every case table used here holds a
match kept, one removed because not nearest and one that passes the mutual rule and falls to the reverse ratio alone.  Shapes are the
smallest at which the kernels take another path: 1 and 2 rows of J (no second neighbour / the smallest view with one), rows around the
32-row tile, a second round of 256 candidates, the four tiled lengths, a scalar tail (37), a length without a tensor kernel (260)."""
import ctypes
import os

import numpy as np
import pytest

import symmetric_ratio_restatement as S
from regard3d_amd import api, synth

pytestmark = pytest.mark.gpu

ROWS = S.ROWS


@pytest.fixture()
def sctx(ctx):
    ctx.clear_images()
    ctx.set_symmetric_ratio(True)
    yield ctx
    ctx.set_symmetric_ratio(False)
    ctx.set_mutual_matching(False)
    ctx.clear_images()


def _register(c, descs, xys, binary=False):
    c.clear_images()
    for v, d in enumerate(descs):
        c.set_image(v, d, None if xys is None else xys[v], 4000, 3000, binary=binary)


def _same_graph(g, pairs, counts, matches):
    keep = counts > 0
    assert np.array_equal(g.pairs, pairs[keep])
    assert np.array_equal(np.diff(g.offsets.astype(np.int64)), counts[keep])
    assert np.array_equal(g.matches, matches)


def _csr(g):
    return g.pairs.copy(), g.offsets.copy(), g.matches.copy()


def _check_counters(c, counters, what=""):
    st, rep = c.stats(), c.symmetric_ratio_report()
    print(f"{what}: report {rep} (expected {counters}), stats ({st.n_mutual_checked}, {st.n_mutual_dropped})")
    assert rep == counters
    assert (st.n_mutual_checked, st.n_mutual_dropped) == counters[:2]              # what the mutual switch alone would report
    return st


def _check_exhaustive(c, oracle, descs, xys, pairs, ratio, squared, binary=False):
    g = c.match_pairs(pairs, ratio, squared)
    counts, matches, counters = S.match_collection(oracle, descs, xys, pairs, ratio, squared, binary)
    _same_graph(g, pairs, counts, matches)
    st = _check_counters(c, counters, f"{len(pairs)} pairs, {len(matches)} kept")
    assert counters[2] > 0                                                           # removed by the reverse ratio only
    return st, counters


# ---------------------------------------------------------------------------------------------------- lengths x rows, default tiles
@pytest.mark.parametrize("dim,dtype", [(64, np.float32), (128, np.float32), (144, np.float32), (256, np.float32), (37, np.float32),
                                       (260, np.float32), (128, np.uint8)])
def test_rows_around_the_tile_every_length(sctx, oracle, dim, dtype):
    descs, xys = S.ragged_views(dim, dtype, 100 + dim)
    _register(sctx, descs, xys)
    _, counters = _check_exhaustive(sctx, oracle, descs, xys, S.all_ordered_pairs(len(ROWS)), S.RAGGED_RATIO, True)
    assert counters[1] > 0
    # part 3 on its own: pairs whose view J has one row lose every match, each counted as a ratio drop
    one_row = np.array([[I, 0] for I in range(1, len(ROWS))], np.uint32)
    g = sctx.match_pairs(one_row, 0.99, True)
    _, _, counters = S.match_collection(oracle, descs, xys, one_row, 0.99, True)
    assert g.num_matches == 0 and counters[0] > 0 and counters == (counters[0], 0, counters[0])
    _check_counters(sctx, counters, "one row of J")


@pytest.mark.parametrize("nbytes", [32, 61])
@pytest.mark.parametrize("mfma", [False, True])
def test_binary_rows_popcount_and_i8_tiles(sctx, oracle, nbytes, mfma):
    descs, xys = S.ragged_views(0, np.uint8, 100 + nbytes, nbytes=nbytes)
    sctx.set_hamming_mfma(mfma)
    try:
        _register(sctx, descs, xys, binary=True)
        st, counters = _check_exhaustive(sctx, oracle, descs, xys, S.all_ordered_pairs(len(ROWS)), 0.9, False, binary=True)
        assert st.n_hamming_mfma == int(mfma) and counters[1] > 0
    finally:
        sctx.set_hamming_mfma(False)


# ---------------------------------------------------------------------------------------------------- the boundary
@pytest.mark.parametrize("dim,dtype,nbytes", [(64, np.float32, None), (128, np.float32, None), (144, np.float32, None), (256, np.float32, None),
                                              (37, np.float32, None), (260, np.float32, None), (128, np.uint8, None),
                                              (0, np.uint8, 32), (0, np.uint8, 61)])
def test_boundary_rows(sctx, oracle, dim, dtype, nbytes):
    """R exact (0.25 on squared L2, 0.5 on Hamming): near-against-16 is rejected (4 < 4, 8 < 8 are false), near-against-17 accepted;
    d2's row below and above j, in j's tile and in another, in j's share of the rows-based kernel's threads (rows 20 and 276); a
    duplicate of row j gives d2 = d1"""
    dI, dJ, xyI, xyJ = S.boundary_views(dim, dtype, nbytes)
    binary = nbytes is not None
    _register(sctx, [dI, dJ], [xyI, xyJ], binary=binary)
    pairs = np.array([[0, 1]], np.uint32)
    g = sctx.match_pairs(pairs, S.BOUNDARY_RATIO, not binary)
    assert [tuple(m) for m in g.matches.tolist()] == S.BOUNDARY_KEPT
    assert np.array_equal(g.matches, S.match_pair(oracle, dI, dJ, xyI, xyJ, S.BOUNDARY_RATIO, not binary, binary)[0])
    n = len(S.BOUNDARY_KEPT) + len(S.BOUNDARY_NOT_NEAREST) + len(S.BOUNDARY_RATIO_ONLY)
    _check_counters(sctx, (n, len(S.BOUNDARY_NOT_NEAREST), len(S.BOUNDARY_RATIO_ONLY)), "boundary")
    # the mutual switch alone keeps what the reverse ratio removes
    sctx.set_symmetric_ratio(False); sctx.set_mutual_matching(True)
    g1 = sctx.match_pairs(pairs, S.BOUNDARY_RATIO, not binary)
    assert [tuple(m) for m in g1.matches.tolist()] == sorted(S.BOUNDARY_KEPT + S.BOUNDARY_RATIO_ONLY)
    assert sctx.symmetric_ratio_report() == (0, 0, 0)


# ---------------------------------------------------------------------------------------------------- more than one round, empty pairs
@pytest.mark.parametrize("integer_mfma", [False, True])
def test_second_round_of_256_candidates(sctx, oracle, integer_mfma):
    dI, dJ, xyI, xyJ = S.ambiguous_views(300, 128, 300)
    sctx.set_integer_mfma(integer_mfma)
    try:
        _register(sctx, [dI, dJ], [xyI, xyJ])
        st, counters = _check_exhaustive(sctx, oracle, [dI, dJ], [xyI, xyJ], np.array([[0, 1], [1, 0]], np.uint32), 0.9, True)
        assert st.n_integer_mfma == int(integer_mfma)
        assert counters[0] > 256 + 100 and counters[1] > 0                       # pair (0, 1) alone has 300 candidates: a second round
    finally:
        sctx.set_integer_mfma(False)


def test_batch_of_28_pairs_with_one_non_empty(sctx, oracle):
    rng = np.random.default_rng(41)
    descs = [rng.integers(0, 121, (n, 128)).astype(np.float32) for n in (40, 33, 64, 70, 35, 50)]      # unrelated views: nothing passes 0.3
    dI, dJ, _, _ = S.ambiguous_views(90, 128, 42)
    dJ[1::3] = np.clip(dJ[1::3] + np.where(np.arange(128) < 40, 3.0, 0.0), 0, 255)                      # the first observers move away: 0.3 can tell them apart
    descs += [dI, dJ]
    pairs = np.array([(i, j) for i in range(8) for j in range(i + 1, 8)], np.uint32)
    _register(sctx, descs, None)
    g = sctx.match_pairs(pairs, 0.3, True)
    counts, matches, counters = S.match_collection(oracle, descs, None, pairs, 0.3, True)
    assert len(pairs) == 28 and (counts > 0).sum() == 1 and counts[-1] > 0
    _same_graph(g, pairs, counts, matches)
    _check_counters(sctx, counters, "28 pairs")
    assert counters[1] > 0 and counters[2] > 0


# ---------------------------------------------------------------------------------------------------- tile formats
def _real_views(seed, n=257, dim=144):
    rng = np.random.default_rng(seed)
    dI = rng.standard_normal((n, dim)).astype(np.float32)
    dJ = (dI + 0.05 * rng.standard_normal((n, dim))).astype(np.float32)
    for j in range(2, n, 3):
        dJ[j] = dI[j - 1] + (0.055 * rng.standard_normal(dim)).astype(np.float32)
    dJ[20] = dJ[10]
    xy = [np.stack([np.arange(n) * 3.0 + k, np.arange(n) * 2.0 + 5.0], 1).astype(np.float32) for k in (1, 2)]
    return [dI, dJ, np.ascontiguousarray(dI[:33])], [xy[0], xy[1], np.ascontiguousarray(xy[0][:33])]


@pytest.mark.parametrize("split", [False, True])
def test_real_valued_rows_f32_tiles_and_split_planes(sctx, oracle, split):
    descs, xys = _real_views(51)
    sctx.set_split_mfma(split)
    try:
        _register(sctx, descs, xys)
        st, counters = _check_exhaustive(sctx, oracle, descs, xys, S.all_ordered_pairs(3), 0.9, True)
        assert st.n_split_mfma == int(split) and st.n_counts_mfma == 0 and counters[1] > 0
    finally:
        sctx.set_split_mfma(False)


def _votes_over_norm(c):
    """integer vote vectors divided by their norm in f32 as vl_liop.c does: the rows the count tiles are for"""
    c = c.astype(np.float32)
    norm = np.zeros(len(c), np.float32)
    for i in range(c.shape[1]):
        norm = (norm + c[:, i] * c[:, i]).astype(np.float32)
    norm = np.maximum(np.sqrt(norm.astype(np.float64)), 1e-12).astype(np.float32)
    return (c / norm[:, None]).astype(np.float32)


def test_liop_like_rows_on_the_count_tiles(sctx, oracle):
    rng = np.random.default_rng(61)
    n, dim = 257, 144
    cI = rng.poisson(rng.gamma(0.6, 40 / 0.6, (n, dim))).astype(np.float32) + 1.0
    cJ = np.clip(cI + rng.integers(-2, 3, (n, dim)), 0, 2047)
    for j in range(2, n, 3):                                                      # every third row: a second observation, as near as the first
        cJ[j] = np.clip(cI[j - 1] + rng.integers(-2, 3, dim), 0, 2047)
    cJ[20] = cJ[10]
    dI, dJ = _votes_over_norm(cI), _votes_over_norm(cJ)
    xy = [np.stack([np.arange(n) * 3.0 + k, np.arange(n) * 2.0 + 5.0], 1).astype(np.float32) for k in (1, 2)]
    descs, xys = [dI, dJ, np.ascontiguousarray(dI[:33])], [xy[0], xy[1], np.ascontiguousarray(xy[0][:33])]
    sctx.set_split_mfma(True)
    try:
        _register(sctx, descs, xys)
        st, counters = _check_exhaustive(sctx, oracle, descs, xys, S.all_ordered_pairs(3), 0.9, True)
        assert st.n_split_mfma == 1 and st.n_counts_mfma == 1 and counters[1] > 0
    finally:
        sctx.set_split_mfma(False)


# ---------------------------------------------------------------------------------------------------- the approximate arms
@pytest.mark.parametrize("n", [160, 100])          # above and below the arms' 128-row scan bound
@pytest.mark.parametrize("arm", ["kgraph", "hnsw", "mrpt"])
def test_approximate_arms(sctx, oracle, arm, n):
    descs, xys = S.arm_views(n, witness=True)
    pairs, ratio = S.ARM_PAIRS, S.ARM_RATIO
    _register(sctx, descs, xys)
    if arm == "kgraph":
        kp = api.KGraphParams.preset("default")
        g = sctx.match_pairs_kgraph(pairs, ratio, kp)
        model = lambda **kw: S.match_collection_kgraph(oracle, descs, xys, pairs, ratio, K=kp.index_K, P=kp.search_P, S=kp.search_S,
                                                       seed=kp.seed, min_rows=128, **kw)
    elif arm == "hnsw":
        g = sctx.match_pairs_hnsw(pairs, ratio, api.HnswParams.preset("precise"))
        model = lambda **kw: S.match_collection_hnsw(oracle, descs, xys, pairs, ratio, "precise", **kw)
    else:
        mp = api.MrptParams.preset()
        g = sctx.match_pairs_mrpt(pairs, ratio, mp)
        model = lambda **kw: S.match_collection_mrpt(oracle, descs, xys, pairs, ratio, mp.n_trees, mp.depth, mp.votes, None, mp.seed, **kw)
    counts, matches, counters = model()
    _same_graph(g, pairs, counts, matches)
    st = _check_counters(sctx, counters, f"{arm} n={n}")
    assert counters[1] > 0 and counters[2] > 0
    assert st.n_ann_built == (2 if n >= 128 else 0)
    if arm == "mrpt" and n >= 128:
        # the witness: a match of an indexed pair on which sqrt(d1) < r sqrt(d2) and d1 < (r r) d2 disagree -- the GPU follows the roots
        w = (S.WITNESS_ROW, S.WITNESS_ROW)
        wrong = model(reverse_on_roots=False)[1]
        in_right = w in [tuple(m) for m in matches[:counts[0]].tolist()]
        in_wrong = w in [tuple(m) for m in wrong.tolist()]
        assert in_right != in_wrong
        assert (w in [tuple(m) for m in g.matches[:int(g.offsets[1])].tolist()]) == in_right


# ---------------------------------------------------------------------------------------------------- switch discipline
def test_both_switches_in_all_four_combinations(ctx, oracle):
    descs, xys = S.ragged_views(128, np.float32, 95)
    pairs = S.all_ordered_pairs(len(ROWS))
    fresh = api.Context(0)
    try:
        _register(fresh, descs, xys)
        never = _csr(fresh.match_pairs(pairs, S.RAGGED_RATIO, True))
        never_k = _csr(fresh.match_pairs_kgraph(pairs, S.RAGGED_RATIO, api.KGraphParams.preset("default")))
    finally:
        fresh.close()
    _register(ctx, descs, xys)
    got = {}
    try:
        for mutual, symmetric in ((False, True), (True, True), (True, False), (False, False)):
            ctx.set_mutual_matching(mutual); ctx.set_symmetric_ratio(symmetric)
            got[mutual, symmetric] = _csr(ctx.match_pairs(pairs, S.RAGGED_RATIO, True)), ctx.symmetric_ratio_report(), ctx.stats()
            if (mutual, symmetric) == (False, False):
                off_k = _csr(ctx.match_pairs_kgraph(pairs, S.RAGGED_RATIO, api.KGraphParams.preset("default")))
    finally:
        ctx.set_mutual_matching(False); ctx.set_symmetric_ratio(False)
    same = lambda a, b: all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    for mode, key in (("symmetric", (False, True)), ("mutual", (True, False)), ("off", (False, False))):
        counts, matches, counters = S.match_collection(oracle, descs, xys, pairs, S.RAGGED_RATIO, True, False, mode)
        g, rep, st = got[key]
        assert np.array_equal(g[2], matches) and np.array_equal(g[0], pairs[counts > 0]), mode
        assert rep == (counters if mode == "symmetric" else (0, 0, 0)), mode        # the report reads zeros after a call with the switch off
        assert (st.n_mutual_checked, st.n_mutual_dropped) == ((0, 0) if mode == "off" else counters[:2]), mode
    # on with both equals on with the new one alone; the three results nest strictly
    assert same(got[True, True][0], got[False, True][0]) and got[True, True][1] == got[False, True][1]
    assert len(got[False, True][0][2]) < len(got[True, False][0][2]) < len(got[False, False][0][2])
    # off after on equals a context that never had it
    assert same(got[False, False][0], never) and same(off_k, never_k)
    ctx.clear_images()


def test_raw_neighbour_lists_ignore_the_switch(sctx, oracle):
    dI, dJ, _, _ = S.ambiguous_views(257, 128, 97)
    bI, bJ, _, _ = S.ambiguous_views(70, 0, 98, nbytes=61)
    sctx.set_symmetric_ratio(False)
    ref = sctx.knn2(dI, dJ), sctx.knn2(bI, bJ, binary=True), sctx.knn(dI, dJ, 2)
    sctx.set_symmetric_ratio(True)
    got = sctx.knn2(dI, dJ), sctx.knn2(bI, bJ, binary=True), sctx.knn(dI, dJ, 2)
    for (ri, rd), (gi, gd) in zip(ref, got):
        assert ri.tobytes() == gi.tobytes() and rd.tobytes() == gd.tobytes()
    oi, od = oracle.knn2(dI, dJ)
    assert np.array_equal(got[0][0], oi) and np.array_equal(got[0][1], od)
    assert (sctx.stats().n_mutual_checked, sctx.stats().n_mutual_dropped) == (0, 0)


def test_null_handles_are_refused():
    L = api.load_library()
    assert L.r3dm_set_symmetric_ratio(None, 1) != 0 and L.r3dm_multi_set_symmetric_ratio(None, 1) != 0
    assert L.r3dm_symmetric_ratio_report(None, None, None, None) != 0


# ---------------------------------------------------------------------------------------------------- multi context, stage
def test_multi_context_two_contexts_on_one_gpu(oracle):
    descs, xys = S.ragged_views(128, np.float32, 81)
    pairs = S.all_ordered_pairs(len(ROWS))
    m = api.MultiContext([0, 0])
    try:
        for v, d in enumerate(descs):
            m.set_image(v, d, xys[v], 4000, 3000)
        g0 = _csr(m.match_pairs(pairs, S.RAGGED_RATIO, True))
        m.set_symmetric_ratio(True)
        g1 = m.match_pairs(pairs, S.RAGGED_RATIO, True)
        st = [m.device_stats(k) for k in range(2)]
        rep = np.zeros(3, np.int64)
        for k in range(2):
            v = [ctypes.c_uint64(0) for _ in range(3)]
            assert m._L.r3dm_symmetric_ratio_report(m._L.r3dm_multi_ctx(m._h, k), *[ctypes.byref(x) for x in v]) == 0
            rep += [int(x.value) for x in v]
        counts, matches, counters = S.match_collection(oracle, descs, xys, pairs, S.RAGGED_RATIO, True)
        _same_graph(g1, pairs, counts, matches)
        assert tuple(int(x) for x in rep) == counters and counters[1] > 0 and counters[2] > 0
        assert (sum(s.n_mutual_checked for s in st), sum(s.n_mutual_dropped for s in st)) == counters[:2]
        assert all(s.n_pairs > 0 for s in st)                                    # both contexts took part
        m.set_symmetric_ratio(False)
        assert all(np.array_equal(a, b) for a, b in zip(g0, _csr(m.match_pairs(pairs, S.RAGGED_RATIO, True))))
    finally:
        m.close()


def test_stage_directory_entry_with_and_without_the_flag(oracle, tmp_path):
    """pre-written .feat / .desc files through r3dm_compute_matches_dir_flags: matches.putative.txt holds the reference's lists without
    R3DM_STAGE_SYMMETRIC_RATIO and the restatement's with it"""
    sc = synth.make_scene(3, 300, "liop", seed=91)
    descs = [np.ascontiguousarray(d, np.float32) for d in sc.descs]
    xys = [np.ascontiguousarray(x, np.float32) for x in sc.xys]
    descs[1] = np.concatenate([descs[1], descs[1][:40]]); xys[1] = np.concatenate([xys[1], xys[1][:40] + 0.5])
    views = []
    for i, d in enumerate(descs):
        name = f"img{i:03d}"
        assert oracle.lib().orc_save_desc(str(tmp_path / (name + ".desc")).encode(), ctypes.c_uint64(d.shape[0]),
                                          ctypes.c_size_t(d.shape[1] * 4), d.ctypes.data_as(ctypes.c_void_p)) == 0
        with open(tmp_path / (name + ".feat"), "w") as f:            # full-precision text so positions round-trip exactly
            for x, y in xys[i]:
                f.write("%.9g %.9g 1 0\n" % (x, y))
        views.append(dict(id=i, width=int(sc.widths[i]), height=int(sc.heights[i]), basename=name))
    pairs = np.array([[0, 1], [0, 2], [1, 2]], np.uint32)
    lists = {}
    for on in (False, True):
        n_put, _ = api.compute_matches_dir(0, str(tmp_path), views, api.F32, 144, 0.8, compute_F=False, symmetric_ratio=on)
        counts, matches, counters = S.match_collection(oracle, descs, xys, pairs, 0.8, True, False, "symmetric" if on else "off")
        p, c, m = oracle.load_matches(os.path.join(str(tmp_path), "matches.putative.txt"))
        assert np.array_equal(p, pairs[counts > 0]) and np.array_equal(c, counts[counts > 0]) and np.array_equal(m, matches), on
        assert n_put == int((counts > 0).sum())
        lists[on] = matches
    mutual = S.match_collection(oracle, descs, xys, pairs, 0.8, True, False, "mutual")[1]
    assert counters[2] > 0 and len(lists[False]) > len(mutual) > len(lists[True])       # the flag removed more than the mutual rule would
    # the same flag through r3dm_compute_matches_stage (r3dm_stage_create / _run / _destroy) on the same files: nothing to extract
    os.remove(os.path.join(str(tmp_path), "matches.putative.txt"))
    rep = api.compute_matches_stage([0], str(tmp_path), views, 0.001, 0.8, 9, False, False, False, symmetric_ratio=True)
    p, c, m = oracle.load_matches(os.path.join(str(tmp_path), "matches.putative.txt"))
    assert rep.images_extracted == 0 and rep.n_putative_matches == len(lists[True]) and np.array_equal(m, lists[True])
