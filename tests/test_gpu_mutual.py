"""Mutual nearest-neighbour matching on the GPU (r3dm_set_mutual_matching, kernels_match_mutual.hip) -- bit for bit against the
restatement built from the oracle (mutual_restatement.py), counters included, on every arm and tile format that collects matches into
a graph: the f32 / bf16 / split-f16 / count tiles, the popcount and the i8 Hamming matchers, the exact scan of lengths without a
tensor kernel, the KGraph / HNSW / MRPT arms, the multi context and the stage's directory entry.  Shapes are the smallest at which the
kernels take another path: rows around the 32-row tile, more than 256 accepted matches in one pair (a second round), a batch whose
pairs mostly have no accepted match, a scalar tail (37), a length without a tensor kernel (260)."""
import ctypes
import os

import numpy as np
import pytest

import mutual_restatement as R
from regard3d_amd import api, synth

pytestmark = pytest.mark.gpu

ROWS = (1, 2, 31, 32, 33, 257)


@pytest.fixture()
def mctx(ctx):
    ctx.clear_images()
    ctx.set_mutual_matching(True)
    yield ctx
    ctx.set_mutual_matching(False)
    ctx.clear_images()


def _ragged_views(dim, dtype, seed, nbytes=None):
    """views of ROWS rows cut from two related 257-row views (second observations every third row, two identical rows)"""
    dI, dJ, xyI, xyJ = R.second_observations(257, dim, seed, dtype, nbytes)
    dJ[20] = dJ[10]                                               # two identical rows of J (both inside the 31-row views)
    descs, xys = [], []
    for k, n in enumerate(ROWS):
        src, xy = (dI, xyI) if k % 2 == 0 else (dJ, xyJ)
        descs.append(np.ascontiguousarray(src[:n])); xys.append(np.ascontiguousarray(xy[:n]))
    return descs, xys


def _all_ordered_pairs(n):
    return np.array([(i, j) for i in range(n) for j in range(n) if i != j], np.uint32)


def _register(c, descs, xys, binary=False):
    c.clear_images()
    for v, d in enumerate(descs):
        c.set_image(v, d, None if xys is None else xys[v], 4000, 3000, binary=binary)


def _expect(oracle, descs, xys, pairs, ratio, squared, binary=False):
    """(counts, matches) of the restatement and the two counters: accepted matches before the check, and how many it removes"""
    c1, m1 = R.match_collection(oracle, descs, xys, pairs, ratio, squared, binary, mutual=True)
    n0 = len(R.match_collection(oracle, descs, None, pairs, ratio, squared, binary, mutual=False)[1])
    n1 = len(R.match_collection(oracle, descs, None, pairs, ratio, squared, binary, mutual=True)[1])
    return c1, m1, n0, n0 - n1


def _same_graph(g, pairs, counts, matches):
    keep = counts > 0
    assert np.array_equal(g.pairs, pairs[keep])
    assert np.array_equal(np.diff(g.offsets.astype(np.int64)), counts[keep])
    assert np.array_equal(g.matches, matches)


def _csr(g):
    return g.pairs.copy(), g.offsets.copy(), g.matches.copy()


def _check_exhaustive(c, oracle, descs, xys, pairs, ratio, squared, binary=False):
    g = c.match_pairs(pairs, ratio, squared)
    st = c.stats()
    counts, matches, checked, dropped = _expect(oracle, descs, xys, pairs, ratio, squared, binary)
    print(f"pairs {len(pairs)}: {len(matches)} matches kept, checked {st.n_mutual_checked} (expected {checked}), "
          f"dropped {st.n_mutual_dropped} (expected {dropped})")
    _same_graph(g, pairs, counts, matches)
    assert (st.n_mutual_checked, st.n_mutual_dropped) == (checked, dropped)
    return st, dropped


# ---------------------------------------------------------------------------------------------------- lengths x rows, default tiles
@pytest.mark.parametrize("dim,dtype", [(64, np.float32), (128, np.float32), (144, np.float32), (256, np.float32), (37, np.float32),
                                       (260, np.float32), (128, np.uint8)])
def test_rows_around_the_tile_every_length(mctx, oracle, dim, dtype):
    descs, xys = _ragged_views(dim, dtype, 100 + dim)
    _register(mctx, descs, xys)
    _, dropped = _check_exhaustive(mctx, oracle, descs, xys, _all_ordered_pairs(len(ROWS)), 0.9, True)
    assert dropped > 0


@pytest.mark.parametrize("nbytes", [32, 61])
@pytest.mark.parametrize("mfma", [False, True])
def test_binary_rows_popcount_and_i8_tiles(mctx, oracle, nbytes, mfma):
    descs, xys = _ragged_views(0, np.uint8, 200 + nbytes, nbytes=nbytes)
    mctx.set_hamming_mfma(mfma)
    try:
        _register(mctx, descs, xys, binary=True)
        st, dropped = _check_exhaustive(mctx, oracle, descs, xys, _all_ordered_pairs(len(ROWS)), 0.9, False, binary=True)
        assert st.n_hamming_mfma == int(mfma) and dropped > 0
    finally:
        mctx.set_hamming_mfma(False)


# ---------------------------------------------------------------------------------------------------- more than one round, empty pairs
@pytest.mark.parametrize("integer_mfma", [False, True])
def test_second_round_of_256_candidates(mctx, oracle, integer_mfma):
    dI, dJ, xyI, xyJ = R.second_observations(300, 128, 300)
    mctx.set_integer_mfma(integer_mfma)
    try:
        _register(mctx, [dI, dJ], [xyI, xyJ])
        st, dropped = _check_exhaustive(mctx, oracle, [dI, dJ], [xyI, xyJ], np.array([[0, 1], [1, 0]], np.uint32), 0.99, True)
        assert st.n_integer_mfma == int(integer_mfma)
        assert st.n_mutual_checked > 2 * 256 and dropped > 0                  # both pairs run a second round
    finally:
        mctx.set_integer_mfma(False)


def test_batch_whose_pairs_mostly_have_no_accepted_match(mctx, oracle):
    rng = np.random.default_rng(41)
    descs = [rng.integers(0, 121, (n, 128)).astype(np.float32) for n in (40, 33, 64, 70, 35, 50)]      # unrelated views: nothing passes 0.3
    dI, dJ, _, _ = R.second_observations(90, 128, 42)
    descs += [dI, dJ]
    pairs = np.array([(i, j) for i in range(8) for j in range(i + 1, 8)], np.uint32)
    _register(mctx, descs, None)
    g = mctx.match_pairs(pairs, 0.3, True)
    st = mctx.stats()
    counts, matches, checked, dropped = _expect(oracle, descs, None, pairs, 0.3, True)
    assert (counts > 0).sum() == 1 and counts[-1] > 0                           # only the last pair has accepted matches
    _same_graph(g, pairs, counts, matches)
    assert (st.n_mutual_checked, st.n_mutual_dropped) == (checked, dropped) and dropped > 0


# ---------------------------------------------------------------------------------------------------- engineered rows
@pytest.mark.parametrize("dim,dtype", [(64, np.float32), (144, np.float32), (37, np.float32), (260, np.float32), (128, np.uint8)])
def test_engineered_rows(mctx, oracle, dim, dtype):
    """distances 1 and 4 from one row of I; two identical rows of J; two rows of J at one position, the earlier of which fails the
    check -- the later must survive the coordinate de-duplication"""
    dI, dJ, xyI, xyJ = R.engineered_views(dim, dtype)
    _register(mctx, [dI, dJ], [xyI, xyJ])
    pairs = np.array([[0, 1]], np.uint32)
    g = mctx.match_pairs(pairs, 0.6, True)
    st = mctx.stats()
    assert g.matches.tolist() == [[0, 0], [1, 2], [2, 5], [3, 6]]
    assert np.array_equal(g.matches, R.match_pair(oracle, dI, dJ, xyI, xyJ, 0.6, True, False, True))
    assert (st.n_mutual_checked, st.n_mutual_dropped) == (7, 3)
    mctx.set_mutual_matching(False)
    g0 = mctx.match_pairs(pairs, 0.6, True)
    assert g0.matches.tolist() == [[0, 0], [0, 1], [1, 2], [1, 3], [2, 4], [3, 6]]
    assert (mctx.stats().n_mutual_checked, mctx.stats().n_mutual_dropped) == (0, 0)


# ---------------------------------------------------------------------------------------------------- split planes, count tiles
def _real_views(seed, n=257, dim=144):
    rng = np.random.default_rng(seed)
    dI = rng.standard_normal((n, dim)).astype(np.float32)
    dJ = (dI + 0.05 * rng.standard_normal((n, dim))).astype(np.float32)
    for j in range(2, n, 3):
        dJ[j] = dI[j - 1] + (0.08 * rng.standard_normal(dim)).astype(np.float32)
    dJ[20] = dJ[10]
    xy = [np.stack([np.arange(n) * 3.0 + k, np.arange(n) * 2.0 + 5.0], 1).astype(np.float32) for k in (1, 2)]
    return [dI, dJ, np.ascontiguousarray(dI[:33])], [xy[0], xy[1], np.ascontiguousarray(xy[0][:33])]


@pytest.mark.parametrize("split", [False, True])
def test_real_valued_rows_f32_tiles_and_split_planes(mctx, oracle, split):
    descs, xys = _real_views(51)
    mctx.set_split_mfma(split)
    try:
        _register(mctx, descs, xys)
        st, dropped = _check_exhaustive(mctx, oracle, descs, xys, _all_ordered_pairs(3), 0.9, True)
        assert st.n_split_mfma == int(split) and st.n_counts_mfma == 0 and dropped > 0
    finally:
        mctx.set_split_mfma(False)


def _votes_over_norm(c):
    """integer vote vectors divided by their norm in f32 as vl_liop.c does (float sum of squares in index order, sqrt in double,
    float division): the rows the count tiles are for"""
    c = c.astype(np.float32)
    norm = np.zeros(len(c), np.float32)
    for i in range(c.shape[1]):
        norm = (norm + c[:, i] * c[:, i]).astype(np.float32)
    norm = np.maximum(np.sqrt(norm.astype(np.float64)), 1e-12).astype(np.float32)
    return (c / norm[:, None]).astype(np.float32)


def test_liop_like_rows_on_the_count_tiles(mctx, oracle):
    rng = np.random.default_rng(61)
    n, dim = 257, 144
    cI = rng.poisson(rng.gamma(0.6, 40 / 0.6, (n, dim))).astype(np.float32) + 1.0
    cJ = np.clip(cI + rng.integers(-2, 3, (n, dim)), 0, 2047)                   # true correspondences: a few votes moved
    for j in range(2, n, 3):                                                      # every third row: a second observation of its left neighbour's row
        cJ[j] = np.clip(cI[j - 1] + rng.integers(-3, 4, dim), 0, 2047)
    cJ[20] = cJ[10]                                                               # two identical rows
    dI, dJ = _votes_over_norm(cI), _votes_over_norm(cJ)
    xy = [np.stack([np.arange(n) * 3.0 + k, np.arange(n) * 2.0 + 5.0], 1).astype(np.float32) for k in (1, 2)]
    descs, xys = [dI, dJ, np.ascontiguousarray(dI[:33])], [xy[0], xy[1], np.ascontiguousarray(xy[0][:33])]
    mctx.set_split_mfma(True)
    try:
        _register(mctx, descs, xys)
        st, dropped = _check_exhaustive(mctx, oracle, descs, xys, _all_ordered_pairs(3), 0.8, True)
        assert st.n_split_mfma == 1 and st.n_counts_mfma == 1 and dropped > 0
    finally:
        mctx.set_split_mfma(False)


# ---------------------------------------------------------------------------------------------------- the approximate arms
def _arm_views(n):
    out, xys = [], []
    for k in range(3):
        dI, dJ, xyI, xyJ = R.second_observations(n, 128, 70 + n)
        out.append(dI if k == 0 else (dJ if k == 1 else np.ascontiguousarray(dJ[::-1])))
        xys.append(xyI if k == 0 else (xyJ if k == 1 else np.ascontiguousarray(xyJ[::-1] + 0.25)))
    return out, xys


@pytest.mark.parametrize("n", [160, 100])          # above and below the arms' 128-row scan bound
@pytest.mark.parametrize("arm", ["kgraph", "hnsw", "mrpt"])
def test_approximate_arms(mctx, oracle, arm, n):
    descs, xys = _arm_views(n)
    pairs = np.array([[0, 1], [0, 2], [1, 2]], np.uint32)
    _register(mctx, descs, xys)
    nones = [None] * 3
    if arm == "kgraph":
        kp = api.KGraphParams.preset("default")
        g = mctx.match_pairs_kgraph(pairs, 0.9, kp)
        model = lambda x, mutual: R.match_collection_kgraph(oracle, descs, x, pairs, 0.9, K=kp.index_K, P=kp.search_P, S=kp.search_S,
                                                            seed=kp.seed, min_rows=128, mutual=mutual)
    elif arm == "hnsw":
        g = mctx.match_pairs_hnsw(pairs, 0.9, api.HnswParams.preset("precise"))
        model = lambda x, mutual: R.match_collection_hnsw(oracle, descs, x, pairs, 0.9, "precise", mutual=mutual)
    else:
        mp = api.MrptParams.preset()
        g = mctx.match_pairs_mrpt(pairs, 0.9, mp)
        model = lambda x, mutual: R.match_collection_mrpt(oracle, descs, x, pairs, 0.9, mp.n_trees, mp.depth, mp.votes, None, mp.seed, mutual=mutual)
    st = mctx.stats()
    counts, matches = model(xys, True)
    checked = len(model(nones, False)[1]); dropped = checked - len(model(nones, True)[1])
    print(f"{arm} n={n}: {len(matches)} kept, checked {st.n_mutual_checked} (expected {checked}), dropped {st.n_mutual_dropped} (expected {dropped})")
    _same_graph(g, pairs, counts, matches)
    assert (st.n_mutual_checked, st.n_mutual_dropped) == (checked, dropped) and dropped > 0
    assert st.n_ann_built == (2 if n >= 128 else 0)


# ---------------------------------------------------------------------------------------------------- multi context, stage
def test_multi_context_two_contexts_on_one_gpu(oracle):
    descs, xys = _ragged_views(128, np.float32, 81)
    pairs = _all_ordered_pairs(len(ROWS))
    m = api.MultiContext([0, 0])
    try:
        for v, d in enumerate(descs):
            m.set_image(v, d, xys[v], 4000, 3000)
        g0 = _csr(m.match_pairs(pairs, 0.9, True))
        m.set_mutual_matching(True)
        g1 = m.match_pairs(pairs, 0.9, True)
        st = [m.device_stats(k) for k in range(2)]
        counts, matches, checked, dropped = _expect(oracle, descs, xys, pairs, 0.9, True)
        _same_graph(g1, pairs, counts, matches)
        assert sum(s.n_mutual_checked for s in st) == checked and sum(s.n_mutual_dropped for s in st) == dropped and dropped > 0
        assert all(s.n_pairs > 0 for s in st)                                    # both contexts took part
        m.set_mutual_matching(False)
        assert all(np.array_equal(a, b) for a, b in zip(g0, _csr(m.match_pairs(pairs, 0.9, True))))
    finally:
        m.close()


def test_stage_directory_entry_with_and_without_the_flag(oracle, tmp_path):
    """pre-written .feat / .desc files through r3dm_compute_matches_dir_flags: matches.putative.txt holds the reference's lists
    without R3DM_STAGE_MUTUAL_MATCHING and the restatement's with it"""
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
    for mutual in (False, True):
        n_put, _ = api.compute_matches_dir(0, str(tmp_path), views, api.F32, 144, 0.8, compute_F=False, mutual=mutual)
        counts, matches = R.match_collection(oracle, descs, xys, pairs, 0.8, True, False, mutual=mutual)
        p, c, m = oracle.load_matches(os.path.join(str(tmp_path), "matches.putative.txt"))
        assert np.array_equal(p, pairs[counts > 0]) and np.array_equal(c, counts[counts > 0]) and np.array_equal(m, matches), mutual
        assert n_put == int((counts > 0).sum())
    off = R.match_collection(oracle, descs, xys, pairs, 0.8, True, False, mutual=False)[1]
    assert len(off) > len(matches)                                   # the flag changed the file
    # the same flag through r3dm_compute_matches_stage (r3dm_stage_create / _run / _destroy) on the same files: nothing to extract
    os.remove(os.path.join(str(tmp_path), "matches.putative.txt"))
    rep = api.compute_matches_stage([0], str(tmp_path), views, 0.001, 0.8, 9, False, False, False, mutual=True)
    p, c, m = oracle.load_matches(os.path.join(str(tmp_path), "matches.putative.txt"))
    assert rep.images_extracted == 0 and rep.n_putative_matches == len(matches) and np.array_equal(m, matches)


# ---------------------------------------------------------------------------------------------------- switch discipline
def test_switch_off_after_on_equals_a_context_that_never_had_it(ctx, oracle):
    descs, xys = _ragged_views(128, np.float32, 95)
    pairs = _all_ordered_pairs(len(ROWS))
    fresh = api.Context(0)
    try:
        _register(fresh, descs, xys)
        ref = _csr(fresh.match_pairs(pairs, 0.9, True))
        ref_k = _csr(fresh.match_pairs_kgraph(pairs, 0.9, api.KGraphParams.preset("default")))
    finally:
        fresh.close()
    _register(ctx, descs, xys)
    ctx.set_mutual_matching(True)
    try:
        on = _csr(ctx.match_pairs(pairs, 0.9, True))
        assert ctx.stats().n_mutual_dropped > 0 and len(on[2]) < len(ref[2])
    finally:
        ctx.set_mutual_matching(False)
    off = _csr(ctx.match_pairs(pairs, 0.9, True))
    st = ctx.stats()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(off, ref))
    assert (st.n_mutual_checked, st.n_mutual_dropped) == (0, 0)
    off_k = _csr(ctx.match_pairs_kgraph(pairs, 0.9, api.KGraphParams.preset("default")))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(off_k, ref_k))
    counts, matches = oracle.match_collection(descs, xys, pairs, 0.9, True)
    assert np.array_equal(off[2], matches)
    ctx.clear_images()


def test_raw_neighbour_lists_ignore_the_switch(mctx, oracle):
    dI, dJ, _, _ = R.second_observations(257, 128, 97)
    bI, bJ, _, _ = R.second_observations(70, 0, 98, nbytes=61)
    mctx.set_mutual_matching(False)
    ref = mctx.knn2(dI, dJ), mctx.knn2(bI, bJ, binary=True), mctx.knn(dI, dJ, 2)
    mctx.set_mutual_matching(True)
    got = mctx.knn2(dI, dJ), mctx.knn2(bI, bJ, binary=True), mctx.knn(dI, dJ, 2)
    for (ri, rd), (gi, gd) in zip(ref, got):
        assert ri.tobytes() == gi.tobytes() and rd.tobytes() == gd.tobytes()
    oi, od = oracle.knn2(dI, dJ)
    assert np.array_equal(got[0][0], oi) and np.array_equal(got[0][1], od)
    assert (mctx.stats().n_mutual_checked, mctx.stats().n_mutual_dropped) == (0, 0)
