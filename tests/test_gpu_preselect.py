"""Preemptive matching on the GPU (r3dm_set_preemptive_matching, r3dm_preselect_pairs, kernels_match_head.hip) -- counts bit for bit
against the restatement built from the oracle (preselect_restatement.py), and the subset property on every arm and tile format that
collects matches into a graph: the graph with the switch on is the library's own switch-off graph restricted to the restatement's
kept pairs.  Shapes are the smallest at which the kernels take another path: heads around the 32-row LDS stage and around the 64- and
128-row deals of a workgroup (h of 2 .. 256 against views of 1 .. 300 rows), a scalar tail (37), every padded length class."""
import ctypes
import os

import numpy as np
import pytest

import preselect_restatement as R
from regard3d_amd import api

pytestmark = pytest.mark.gpu

ROWS = (1, 2, 31, 32, 33, 257, 300)
HEADS = (2, 31, 32, 33, 64, 255, 256)
NO_PRIORITY = 4                                   # the 33-row view carries no priority


@pytest.fixture()
def pctx(ctx):
    ctx.clear_images()
    yield ctx
    ctx.set_preemptive_matching(False)
    for f in (ctx.set_integer_mfma, ctx.set_split_mfma, ctx.set_hamming_mfma):
        f(False)
    ctx.clear_images()


def _views(dim, dtype, seed, nbytes=None):
    """the ragged related views, the 33-row one without priority, and a 40-row view of noise at the end"""
    descs, prios = R.related_views(ROWS + (40,), dim, seed, dtype, nbytes)
    prios[NO_PRIORITY] = None
    return descs, prios


def _ordered_pairs(n):
    return np.array([(i, j) for i in range(n) for j in range(n) if i != j], np.uint32)


def _register(c, descs, prios, xys=None, binary=False):
    c.clear_images()
    for v, d in enumerate(descs):
        c.set_image(v, d, None if xys is None else xys[v], 4000, 3000, binary=binary)
        if prios[v] is not None:
            c.set_view_priority(v, prios[v])


def _xys(descs):
    return [np.stack([np.arange(len(d)) * 3.0 + k, np.arange(len(d)) * 2.0 + 5.0], 1).astype(np.float32) for k, d in enumerate(descs)]


def _csr(g):
    return g.pairs.copy(), g.offsets.copy(), g.matches.copy()


def _has_head(c, v):
    return bool(c.view_info(v)[0] & api.LAYOUT_HEAD)


# ---------------------------------------------------------------------------------------------------- counts
@pytest.mark.parametrize("dim,dtype,nbytes", [(64, np.float32, None), (128, np.float32, None), (144, np.float32, None), (256, np.float32, None),
                                              (37, np.float32, None), (128, np.uint8, None), (0, np.uint8, 32), (0, np.uint8, 61)])
def test_counts_bit_for_bit(pctx, oracle, dim, dtype, nbytes):
    binary = nbytes is not None
    descs, prios = _views(dim, dtype, 500 + dim + (nbytes or 0), nbytes)
    pairs = _ordered_pairs(len(descs))
    ratio, squared = (0.8, False) if binary else (0.6, True)
    _register(pctx, descs, prios, binary=binary)
    seen = set()
    for h in HEADS:
        got = pctx.preselect_pairs(pairs, h, ratio, squared)
        want = R.collection_counts(oracle, descs, prios, pairs, h, ratio, squared, binary)
        rep = pctx.preselect_report()
        print(f"dim {dim} nbytes {nbytes} h {h}: counts {sorted(set(want.tolist()))}, {rep['ms_kernels']:.3f} ms, heads built {rep['n_heads_built']}")
        assert np.array_equal(got, want), (h, np.flatnonzero(got != want)[:8], got[got != want][:8], want[got != want][:8])
        assert (want > 0).any() and (want == 0).any()
        assert rep["n_pairs"] == len(pairs) and rep["n_heads_built"] == len(descs) and rep["n_views_without_priority"] == 1
        seen |= set(want.tolist())
    assert max(seen) >= 200                                        # the 257- and 300-row views at h = 255 / 256: more than 128 queries count
    # the same h again: every head is cached
    pctx.preselect_pairs(pairs, HEADS[-1], ratio, squared)
    assert pctx.preselect_report()["n_heads_built"] == 0
    assert all(_has_head(pctx, v) for v in range(len(descs)))


def test_real_valued_rows_and_caller_order(pctx, oracle):
    """real-valued rows (every sum rounds): the kernel's summation is exact_l2sq's; duplicates and both orders in one call"""
    rng = np.random.default_rng(77)
    dI = rng.standard_normal((200, 144)).astype(np.float32)
    dJ = (dI + 0.05 * rng.standard_normal((200, 144))).astype(np.float32)
    t37 = [np.ascontiguousarray(dI[:150, :37]), np.ascontiguousarray(dJ[:90, :37])]
    descs = [dI, dJ, np.ascontiguousarray(dJ[::-1][:70]), rng.standard_normal((50, 144)).astype(np.float32)]
    prios = [rng.integers(0, 6, len(d)).astype(np.float32) for d in descs]
    _register(pctx, descs, prios)
    pairs = np.array([[1, 0], [0, 1], [3, 2], [1, 0], [2, 0], [0, 3], [2, 1]], np.uint32)
    for h, ratio in ((128, 0.8), (40, 0.95), (256, 0.8), (150, 0.9)):       # (J heads of 200 and 150 rows: one lane per query, no part split)
        got = pctx.preselect_pairs(pairs, h, ratio, True)
        want = R.collection_counts(oracle, descs, prios, pairs, h, ratio, True)
        print(f"h {h}: {got.tolist()}")
        assert np.array_equal(got, want) and got[0] == got[3] and (want > 0).any()
    # two lengths in one call: each class has its own launch (37 has a scalar tail)
    for v, d in enumerate(t37):
        pctx.set_image(10 + v, d, None, 4000, 3000)
    mixed = np.array([[10, 11], [0, 1], [11, 10], [0, 10]], np.uint32)           # (the last pair's views differ in length: count 0)
    got = pctx.preselect_pairs(mixed, 64, 0.8, True)
    want = [R.pair_count(oracle, t37[0], t37[1], None, None, 64, 0.8), R.pair_count(oracle, dI, dJ, prios[0], prios[1], 64, 0.8),
            R.pair_count(oracle, t37[1], t37[0], None, None, 64, 0.8), 0]
    assert got.tolist() == want and want[0] > 0
    assert pctx.preselect_report()["n_pairs"] == 3                               # the pair of two lengths is not looked at


# ---------------------------------------------------------------------------------------------------- the threshold
def test_threshold_at_the_edge(pctx, oracle):
    descs, prios = _views(128, np.float32, 601)
    xys = _xys(descs)
    _register(pctx, descs, prios, xys)
    pairs = _ordered_pairs(len(descs))
    counts = pctx.preselect_pairs(pairs, 32, 0.6, True)
    k = int(np.argmax(counts))
    assert counts[k] > 1
    c = int(counts[k]); one = pairs[k:k + 1]
    plain = _csr(pctx.match_pairs(one, 0.6, True))
    assert len(plain[2]) > 0
    pctx.set_preemptive_matching(True, 32, c)
    kept = _csr(pctx.match_pairs(one, 0.6, True))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(kept, plain)) and pctx.preselect_report()["n_kept"] == 1
    pctx.set_preemptive_matching(True, 32, c + 1)
    g = pctx.match_pairs(one, 0.6, True)
    assert g.num_pairs == 0 and g.num_matches == 0 and pctx.preselect_report()["n_kept"] == 0 and pctx.preselect_report()["n_pairs"] == 1


# ---------------------------------------------------------------------------------------------------- the subset property
def _subset_check(c, oracle, descs, prios, xys, pairs, h, t, ratio, squared, binary, match, oracle_too=False):
    c.set_preemptive_matching(False)
    off = _csr(match())
    assert c.preselect_report()["n_pairs"] == 0 and not any(_has_head(c, v) for v in range(len(descs)))
    c.set_preemptive_matching(True, h, t)
    on = match()
    rep = c.preselect_report()
    counts, keep = R.gate_collection(oracle, descs, prios, pairs, h, t, ratio, squared, binary)
    print(f"kept {int(keep.sum())} of {len(pairs)} pairs (counts {sorted(set(counts.tolist()))}); gate {rep['ms_kernels']:.3f} ms")
    assert 0 < keep.sum() < len(pairs)
    p, n, m = R.restrict_graph(off[0], off[1], off[2], pairs[keep])
    assert np.array_equal(on.pairs, p) and np.array_equal(np.diff(on.offsets.astype(np.int64)), n) and on.matches.tobytes() == m.tobytes()
    assert (rep["n_pairs"], rep["n_kept"]) == (len(pairs), int(keep.sum()))
    if oracle_too:
        oc, om = oracle.match_collection(descs, xys, pairs[keep], ratio, squared, binary=binary)
        assert np.array_equal(on.pairs, pairs[keep][oc > 0]) and np.array_equal(on.matches, om)
    c.set_preemptive_matching(False)
    return rep


@pytest.mark.parametrize("tiles", ["f32", "bf16"])
def test_subset_exhaustive_integer_rows(pctx, oracle, tiles):
    descs, prios = _views(128, np.float32, 611)
    xys = _xys(descs)
    pairs = np.array([(i, j) for i in range(len(descs)) for j in range(i + 1, len(descs))], np.uint32)
    pctx.set_integer_mfma(tiles == "bf16")
    _register(pctx, descs, prios, xys)
    _subset_check(pctx, oracle, descs, prios, xys, pairs, 32, 4, 0.6, True, False, lambda: pctx.match_pairs(pairs, 0.6, True), oracle_too=True)
    assert pctx.stats().n_integer_mfma == int(tiles == "bf16")


def _votes_over_norm(c):
    """integer vote vectors divided by their norm in f32 (float sum of squares in index order, sqrt in double, float division): the
    rows the count tiles are for"""
    c = c.astype(np.float32)
    norm = np.zeros(len(c), np.float32)
    for i in range(c.shape[1]):
        norm = (norm + c[:, i] * c[:, i]).astype(np.float32)
    norm = np.maximum(np.sqrt(norm.astype(np.float64)), 1e-12).astype(np.float32)
    return (c / norm[:, None]).astype(np.float32)


@pytest.mark.parametrize("tiles", ["split", "counts"])
def test_subset_exhaustive_real_rows(pctx, oracle, tiles):
    rng = np.random.default_rng(621)
    n, dim = 140, 144
    if tiles == "counts":
        cI = rng.poisson(rng.gamma(0.6, 40 / 0.6, (n, dim))).astype(np.float32) + 1.0
        cJ = np.clip(cI + rng.integers(-2, 3, (n, dim)), 0, 2047)
        cN = rng.poisson(rng.gamma(0.6, 40 / 0.6, (60, dim))).astype(np.float32) + 1.0
        dI, dJ, dN = _votes_over_norm(cI), _votes_over_norm(cJ), _votes_over_norm(cN)
    else:
        dI = rng.standard_normal((n, dim)).astype(np.float32)
        dJ = (dI + 0.05 * rng.standard_normal((n, dim))).astype(np.float32)
        dN = rng.standard_normal((60, dim)).astype(np.float32)
    descs = [dI, dJ, np.ascontiguousarray(dI[:33]), dN]
    shared = rng.integers(0, 5, n).astype(np.float32)
    prios = [shared, shared, shared[:33].copy(), shared[:60].copy()]
    xys = _xys(descs)
    pairs = _ordered_pairs(4)
    pctx.set_split_mfma(True)
    _register(pctx, descs, prios, xys)
    _subset_check(pctx, oracle, descs, prios, xys, pairs, 64, 4, 0.8, True, False, lambda: pctx.match_pairs(pairs, 0.8, True), oracle_too=True)
    st = pctx.stats()
    assert st.n_split_mfma == 1 and st.n_counts_mfma == int(tiles == "counts")


@pytest.mark.parametrize("mfma", [False, True])
def test_subset_binary_rows(pctx, oracle, mfma):
    descs, prios = _views(0, np.uint8, 631, nbytes=61)
    xys = _xys(descs)
    pairs = _ordered_pairs(len(descs))
    pctx.set_hamming_mfma(mfma)
    _register(pctx, descs, prios, xys, binary=True)
    _subset_check(pctx, oracle, descs, prios, xys, pairs, 33, 4, 0.8, False, True, lambda: pctx.match_pairs(pairs, 0.8, False), oracle_too=True)
    assert pctx.stats().n_hamming_mfma == int(mfma)


@pytest.mark.parametrize("arm", ["kgraph", "hnsw", "mrpt"])
def test_subset_approximate_arms(pctx, oracle, arm):
    """views above and below the arms' 128-row scan bound: the gate runs on the indexed and on the scanned pairs"""
    descs, prios = R.related_views((160, 160, 100, 160, 100), 128, 641, n_unrelated=2)
    xys = _xys(descs)
    pairs = _ordered_pairs(len(descs))
    _register(pctx, descs, prios, xys)
    if arm == "kgraph":
        match = lambda: pctx.match_pairs_kgraph(pairs, 0.6, api.KGraphParams.preset("default"))
    elif arm == "hnsw":
        match = lambda: pctx.match_pairs_hnsw(pairs, 0.6, api.HnswParams.preset("precise"))
    else:
        match = lambda: pctx.match_pairs_mrpt(pairs, 0.6, api.MrptParams.preset())
    _subset_check(pctx, oracle, descs, prios, xys, pairs, 64, 4, 0.6, True, False, match)      # (R = ratio^2 on squared distances, MRPT included)


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals(pctx):
    L = api.load_library()
    rng = np.random.default_rng(651)
    d = rng.integers(0, 121, (40, 128)).astype(np.float32)
    pctx.set_image(0, d, None, 100, 100); pctx.set_image(1, d[:30], None, 100, 100)
    pairs = np.array([[0, 1]], np.uint32)
    for h in (0, 1, 257):
        with pytest.raises(api.R3dmError, match="-> -1"):
            pctx.preselect_pairs(pairs, h, 0.6, True)
        with pytest.raises(api.R3dmError, match="-> -1"):
            pctx.set_preemptive_matching(True, h, 4)
    with pytest.raises(api.R3dmError, match="-> -1"):
        pctx.set_preemptive_matching(True, 128, 0)
    for bad in (np.full(40, np.nan, np.float32), np.r_[np.ones(39, np.float32), np.float32(-1.0)], np.r_[np.ones(39, np.float32), np.float32(np.inf)],
                np.ones(39, np.float32), np.ones(41, np.float32)):
        with pytest.raises(api.R3dmError, match="-> -1"):
            pctx.set_view_priority(0, bad)
    with pytest.raises(api.R3dmError, match="-> -1"):
        pctx.set_view_priority(99, np.ones(40, np.float32))                       # an unknown view
    with pytest.raises(api.R3dmError, match="-> -1"):
        pctx.preselect_pairs(np.array([[0, 99]], np.uint32), 32, 0.6, True)
    assert not _has_head(pctx, 0)                                                 # nothing of the refused calls was staged
    counts = np.zeros(1, np.uint32)
    assert L.r3dm_set_view_priority(None, 0, None, 0) == -1 and L.r3dm_set_preemptive_matching(None, 1, 128, 4) == -1
    assert L.r3dm_preselect_pairs(None, pairs.ctypes.data, 1, 32, ctypes.c_float(0.6), 1, counts.ctypes.data) == -1
    assert L.r3dm_preselect_report(None, None) == -1
    assert L.r3dm_multi_set_view_priority(None, 0, None, 0) == -1 and L.r3dm_multi_set_preemptive_matching(None, 1, 128, 4) == -1
    # length 260: no gate kernel -- the primitive refuses, and so does a match entry while the switch is on (and only then)
    w = rng.integers(0, 121, (40, 260)).astype(np.float32)
    pctx.set_image(2, w, None, 100, 100); pctx.set_image(3, w[:30], None, 100, 100)
    wide = np.array([[2, 3]], np.uint32)
    with pytest.raises(api.R3dmError, match="-> -5"):
        pctx.preselect_pairs(wide, 32, 0.6, True)
    assert pctx.match_pairs(wide, 0.6, True).num_pairs == 1
    pctx.set_preemptive_matching(True, 32, 1)
    with pytest.raises(api.R3dmError, match="-> -5"):
        pctx.match_pairs(wide, 0.6, True)
    assert pctx.match_pairs(pairs, 0.6, True).num_pairs == 1                      # the 128-element pair is still served


# ---------------------------------------------------------------------------------------------------- history, switch off
def test_history_independence(pctx, oracle):
    descs, prios = _views(128, np.float32, 661)
    pairs = _ordered_pairs(len(descs))

    def fresh_counts(ds, ps, h):
        f = api.Context(0)
        try:
            _register(f, ds, ps)
            return f.preselect_pairs(pairs, h, 0.6, True)
        finally:
            f.close()

    _register(pctx, descs, prios)
    base_bytes = pctx.view_info(5)[1]
    assert not _has_head(pctx, 5)
    assert np.array_equal(pctx.preselect_pairs(pairs, 64, 0.6, True), fresh_counts(descs, prios, 64))
    with_head = pctx.view_info(5)[1]
    assert _has_head(pctx, 5) and with_head >= base_bytes + 64 * 128 * 4
    assert np.array_equal(pctx.preselect_pairs(pairs, 33, 0.6, True), fresh_counts(descs, prios, 33))
    assert pctx.preselect_report()["n_heads_built"] == len(descs)                 # another h: every head is remade
    # replace a view (other rows, a new priority): its priority and head go with the old registration
    rng = np.random.default_rng(662)
    descs2 = list(descs); prios2 = list(prios)
    descs2[5] = np.ascontiguousarray(descs[6][:280]); prios2[5] = rng.integers(0, 3, 280).astype(np.float32)
    pctx.set_image(5, descs2[5], None, 4000, 3000)
    assert not _has_head(pctx, 5) and pctx.view_info(5)[1] < with_head
    unprio = list(prios2); unprio[5] = None
    assert np.array_equal(pctx.preselect_pairs(pairs, 33, 0.6, True), fresh_counts(descs2, unprio, 33))
    assert pctx.preselect_report()["n_heads_built"] == 1 and pctx.preselect_report()["n_views_without_priority"] == 2
    pctx.set_view_priority(5, prios2[5])
    assert not _has_head(pctx, 5)
    want = fresh_counts(descs2, prios2, 33)
    assert np.array_equal(pctx.preselect_pairs(pairs, 33, 0.6, True), want)
    assert np.array_equal(want, R.collection_counts(oracle, descs2, prios2, pairs, 33, 0.6, True))
    # remove a priority
    pctx.set_view_priority(6, None)
    assert not _has_head(pctx, 6)
    prios3 = list(prios2); prios3[6] = None
    assert np.array_equal(pctx.preselect_pairs(pairs, 33, 0.6, True), fresh_counts(descs2, prios3, 33))
    assert _has_head(pctx, 6)
    # clear and register again (the spare buffers are reused), then trim
    pctx.clear_images()
    _register(pctx, descs, prios)
    assert not any(_has_head(pctx, v) for v in range(len(descs)))
    assert np.array_equal(pctx.preselect_pairs(pairs, 64, 0.6, True), fresh_counts(descs, prios, 64))
    pctx.clear_images(); pctx.trim()
    _register(pctx, descs, prios)
    assert np.array_equal(pctx.preselect_pairs(pairs, 256, 0.6, True), R.collection_counts(oracle, descs, prios, pairs, 256, 0.6, True))


def test_switch_off_and_raw_lists(pctx, oracle):
    descs, prios = _views(128, np.float32, 671)
    xys = _xys(descs)
    pairs = _ordered_pairs(len(descs))
    fresh = api.Context(0)
    try:
        for v, d in enumerate(descs):
            fresh.set_image(v, d, xys[v], 4000, 3000)
        ref = _csr(fresh.match_pairs(pairs, 0.6, True))
        ref_knn = fresh.knn2(descs[5], descs[6])
    finally:
        fresh.close()
    _register(pctx, descs, prios, xys)
    pctx.set_preemptive_matching(True, 32, 4)
    on = _csr(pctx.match_pairs(pairs, 0.6, True))
    assert len(on[0]) < len(ref[0]) and pctx.preselect_report()["n_pairs"] == len(pairs)
    knn_on = pctx.knn2(descs[5], descs[6])                                        # raw lists ignore the switch
    assert all(a.tobytes() == b.tobytes() for a, b in zip(knn_on, ref_knn))
    pctx.set_preemptive_matching(False, 32, 4)
    off = _csr(pctx.match_pairs(pairs, 0.6, True))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(off, ref))
    assert all(v == 0 for v in pctx.preselect_report().values())
    # a context that never had the switch: the report is zero and no view has a head
    pctx.clear_images()
    for v, d in enumerate(descs):
        pctx.set_image(v, d, xys[v], 4000, 3000)
    pctx.match_pairs(pairs, 0.6, True)
    assert all(v == 0 for v in pctx.preselect_report().values()) and not any(_has_head(pctx, v) for v in range(len(descs)))
    oc, om = oracle.match_collection(descs, xys, pairs, 0.6, True)
    assert np.array_equal(off[2], om)


# ---------------------------------------------------------------------------------------------------- multi context, stage
def test_multi_context_two_contexts_on_one_gpu(oracle):
    descs, prios = _views(128, np.float32, 681)
    xys = _xys(descs)
    pairs = _ordered_pairs(len(descs))
    m = api.MultiContext([0, 0])
    try:
        for v, d in enumerate(descs):
            m.set_image(v, d, xys[v], 4000, 3000)
            if prios[v] is not None:
                m.set_view_priority(v, prios[v])
        off = _csr(m.match_pairs(pairs, 0.6, True))
        m.set_preemptive_matching(True, 32, 4)
        on = m.match_pairs(pairs, 0.6, True)
        reps = [m.device_preselect_report(k) for k in range(2)]
        counts, keep = R.gate_collection(oracle, descs, prios, pairs, 32, 4, 0.6, True)
        p, n, mm = R.restrict_graph(off[0], off[1], off[2], pairs[keep])
        assert np.array_equal(on.pairs, p) and np.array_equal(np.diff(on.offsets.astype(np.int64)), n) and on.matches.tobytes() == mm.tobytes()
        assert sum(r["n_pairs"] for r in reps) == len(pairs) and sum(r["n_kept"] for r in reps) == int(keep.sum())
        assert all(r["n_pairs"] > 0 for r in reps) and 0 < keep.sum() < len(pairs)     # each context gated its own shard
        with pytest.raises(api.R3dmError):
            m.set_view_priority(0, np.full(len(descs[0]), -1.0, np.float32))
        m.set_preemptive_matching(False)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(off, _csr(m.match_pairs(pairs, 0.6, True))))
    finally:
        m.close()


def test_stage_directory_entry_with_and_without_the_flag(oracle, tmp_path):
    """six small views, two of them unrelated to the rest, through r3dm_compute_matches_dir_flags: with R3DM_STAGE_PREEMPTIVE_MATCHING
    matches.putative.txt holds exactly the kept pairs' lists (the scale column of the .feat files is the priority), without it all
    non-empty pairs"""
    rows = (150, 140, 150, 135, 150, 145)
    descs, prios = R.related_views(rows, 144, 691, n_unrelated=2)
    for k in (4, 5):
        descs[k][:3] = descs[0][:3]                                  # three true correspondences with view 0: fewer than min_matches
    rng = np.random.default_rng(692)
    prios = [(p + np.float32(0.5) + rng.integers(0, 2, len(p)).astype(np.float32) * np.float32(0.125)).astype(np.float32) for p in prios]
    xys = _xys(descs)
    views = []
    for i, d in enumerate(descs):
        name = f"img{i:03d}"
        assert oracle.lib().orc_save_desc(str(tmp_path / (name + ".desc")).encode(), ctypes.c_uint64(d.shape[0]),
                                          ctypes.c_size_t(d.shape[1] * 4), d.ctypes.data_as(ctypes.c_void_p)) == 0
        with open(tmp_path / (name + ".feat"), "w") as f:            # full-precision text so positions and scales round-trip exactly
            for (x, y), s in zip(xys[i], prios[i]):
                f.write("%.9g %.9g %.9g 0\n" % (x, y, s))
        views.append(dict(id=i, width=4000, height=3000, basename=name))
    pairs = np.array([(i, j) for i in range(6) for j in range(i + 1, 6)], np.uint32)
    counts, keep = R.gate_collection(oracle, descs, prios, pairs, 128, 4, 0.8, True)
    assert 0 < keep.sum() < len(pairs)
    all_c, all_m = oracle.match_collection(descs, xys, pairs, 0.8, True)
    assert (all_c[~keep] > 0).any()                                  # the gate drops pairs that do have matches: the file must change
    for flag in (False, True):
        n_put, _ = api.compute_matches_dir(0, str(tmp_path), views, api.F32, 144, 0.8, compute_F=False, preemptive=flag)
        sel = pairs[keep] if flag else pairs
        oc, om = oracle.match_collection(descs, xys, sel, 0.8, True)
        p, c, m = oracle.load_matches(os.path.join(str(tmp_path), "matches.putative.txt"))
        assert np.array_equal(p, sel[oc > 0]) and np.array_equal(c, oc[oc > 0]) and np.array_equal(m, om), flag
        assert n_put == int((oc > 0).sum())
    # the same flag through r3dm_compute_matches_stage on the same files: nothing to extract
    os.remove(os.path.join(str(tmp_path), "matches.putative.txt"))
    rep = api.compute_matches_stage([0], str(tmp_path), views, 0.001, 0.8, 9, False, False, False, preemptive=True)
    p, c, m = oracle.load_matches(os.path.join(str(tmp_path), "matches.putative.txt"))
    assert rep.images_extracted == 0 and np.array_equal(p, sel[oc > 0]) and np.array_equal(m, om)
