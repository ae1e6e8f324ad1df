"""r3dm_knn / r3dm_index_knn on binary rows with r3dm_set_knn_hamming_tiles on: the K-list kernel of the i8 MFMA tiles
(kernels_match_knn8.hip) against the numpy restatement, indices AND distances bit for bit, and the counters of every call: one launch
on the i8 tiles, nothing scanned, none of the other paths' counters moved.  The data sets and their preconditions are
knn_hamming_cases.py's (checked without a GPU by test_knn_hamming_cases.py).  Every case switches the session context's flag off again."""
import contextlib
import threading

import numpy as np
import pytest

import knn_hamming_cases as H
import knn_restatement as R

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def tiles(ctx):
    ctx.set_knn_hamming_tiles(True)
    try:
        yield ctx
    finally:
        ctx.set_knn_hamming_tiles(False)


def _assert_counters(s, nq, on=1, what=""):
    assert s.n_knn_hamming_tiles == on, (what, s.n_knn_hamming_tiles)
    assert s.n_exact_fallback == 0, what
    assert s.n_hamming_mfma == 0, what
    assert (s.n_knn_integer_tiles, s.n_knn_split_tiles) == (0, 0), what
    assert s.n_queries == nq, what


def _assert_equal(idx, dist, ref, k, what=""):
    ri, rd = ref
    bad = np.flatnonzero((idx != ri[:, :k]).any(1) | (dist != rd[:, :k]).any(1))
    assert bad.size == 0, f"{what}: {bad.size} of {len(idx)} queries differ, first {bad[:5]}: got {idx[bad[:2]]} {dist[bad[:2]]}, want {ri[bad[:2], :k]} {rd[bad[:2], :k]}"


def _check(ctx, a, b, k, ref=None, what=""):
    """knn with the switch on equals the restatement and ran on the i8 tiles"""
    with tiles(ctx):
        idx, dist = ctx.knn(a, b, k, binary=True)
        s = ctx.stats()
    _assert_equal(idx, dist, ref if ref is not None else R.knn(a, b, k, binary=True), k, what)
    _assert_counters(s, b.shape[0], 1, what)
    return idx, dist


# ---------------------------------------------------------------------------------------------------- 1. routing
def test_routing_and_counters(ctx):
    a, b, ref = H.random_rows(300, 90, 61)
    on = _check(ctx, a, b, 3, ref, "switch on")
    # switch off: the popcount K-list kernel, the counter at 0, the same bytes
    idx, dist = ctx.knn(a, b, 3, binary=True)
    _assert_counters(ctx.stats(), 90, 0, "switch off")
    assert idx.tobytes() == on[0].tobytes() and dist.tobytes() == on[1].tobytes()
    # the other switches alone leave the counter at 0
    for setter in (ctx.set_knn_narrow_tiles, ctx.set_hamming_mfma):
        setter(True)
        try:
            idx, dist = ctx.knn(a, b, 3, binary=True)
            s = ctx.stats()
        finally:
            setter(False)
        _assert_counters(s, 90, 0, setter.__name__)
        assert idx.tobytes() == on[0].tobytes() and dist.tobytes() == on[1].tobytes()
    # k = 2 is the 2-NN path whatever the switch says
    i2, d2 = ctx.knn2(a, b, binary=True)
    with tiles(ctx):
        ik, dk = ctx.knn(a, b, 2, binary=True)
        s = ctx.stats()
    assert np.array_equal(ik, i2) and np.array_equal(dk, d2)
    assert s.n_knn_hamming_tiles == 0 and s.n_hamming_mfma == 0
    # F32 / U8 rows never consult the switch
    au = a[:, :32].copy(); bu = b[:, :32].copy()
    with tiles(ctx):
        idx, dist = ctx.knn(au, bu, 3)
        s = ctx.stats()
    ri, rd = R.knn(au, bu, 3)
    assert np.array_equal(idx, ri) and np.array_equal(dist, rd) and s.n_knn_hamming_tiles == 0


# ---------------------------------------------------------------------------------------------------- 2. tile counts
@pytest.mark.parametrize("nbytes", (32, 61))
@pytest.mark.parametrize("n", H.TILE_ROWS_N)
def test_tile_counts(ctx, n, nbytes):
    """1 .. 9 dataset tiles through the double-stepped, triple-buffered loop; n = k is the padding-row case: a lane half holds fewer
    than KL real rows, the padding rows enter its list and none may come out"""
    a, b, ref = H.random_rows(n, 40, nbytes)
    for k in H.KS:
        if k > min(n, 8):
            continue
        idx, dist = _check(ctx, a, b, k, ref, f"n = {n}, k = {k}")
        assert (idx >= 0).all() and (idx < n).all() and (dist < 2.0 ** 23).all()


@pytest.mark.parametrize("nbytes", (32, 61))
def test_one_row_dataset(ctx, nbytes):
    a, b, ref = H.random_rows(1, 40, nbytes)
    idx, dist = _check(ctx, a, b, 1, ref, "one row")
    assert (idx == 0).all()


# ---------------------------------------------------------------------------------------------------- 3. query counts
@pytest.mark.parametrize("nq", H.QUERY_COUNTS)
def test_query_counts(ctx, nq):
    a, b, ref = H.random_rows(101, nq, 61)
    for k in (3, 8):
        _check(ctx, a, b, k, ref, f"nq = {nq}, k = {k}")
    a, b = a[:, :32].copy(), b[:, :32].copy()              # the 8-word kernel: two query tiles per wave
    for k in (3, 8):
        _check(ctx, a, b, k, what=f"nq = {nq}, k = {k}, 32 bytes")


# ---------------------------------------------------------------------------------------------------- 4. byte lengths
@pytest.mark.parametrize("k", H.KS)
@pytest.mark.parametrize("nbytes", H.BYTE_LENGTHS)
def test_byte_lengths(ctx, nbytes, k):
    a, b, ref = H.random_rows(300, 90, nbytes)
    _check(ctx, a, b, k, ref, f"{nbytes} bytes")


# ---------------------------------------------------------------------------------------------------- 5. ties
@pytest.mark.parametrize("nbytes", (32, 61, 64))
def test_dense_ties(ctx, nbytes):
    a, b, ref = H.dense_ties(nbytes)
    for k in H.KS:
        assert H.ties_across_halves(a, b, k) >= 20         # the precondition, before the case is trusted
        _check(ctx, a, b, k, ref, f"dense ties, {nbytes} bytes, k = {k}")


@pytest.mark.parametrize("nbytes", (32, 61, 64))
def test_all_rows_identical(ctx, nbytes):
    a, b, ref = H.all_identical(nbytes)
    for k in H.KS:
        idx, dist = _check(ctx, a, b, k, ref, f"identical rows, k = {k}")
        assert (idx == np.arange(k)[None, :]).all() and (dist[:3] == 0).all()


@pytest.mark.parametrize("nbytes", (32, 61, 64))
def test_duplicated_rows(ctx, nbytes):
    a, b, ref = H.duplicated_rows(nbytes)
    idx, dist = _check(ctx, a, b, 8, ref, "duplicated rows")
    assert idx[0].tolist() == list(H.DUP_ROWS[:8]) and (dist[0] == 0).all()
    _check(ctx, a, b, 3, ref, "duplicated rows, k = 3")


@pytest.mark.parametrize("nbytes", (32, 61, 64))
def test_tie_of_kth_and_next_across_halves(ctx, nbytes):
    a, b, ref, near, A, B, C = H.tie_across_halves(nbytes)
    idx, dist = _check(ctx, a, b, 8, ref, "tie across halves")
    assert idx[0].tolist() == near + [A] and dist[0].tolist() == [1, 2, 3, 4, 5, 6, 7, 9]


# ---------------------------------------------------------------------------------------------------- 6. index
def test_index_knn_from_eight_threads(ctx):
    """one index, built with every switch off; eight host threads, each with a context of its own and the switch on, search it at
    once: whichever comes first stages the index's byte-per-bit tiles under the index's lock, every thread gets the restatement's
    answer on the i8 tiles, and no search re-stages the dataset (a search uploads its queries only)"""
    from regard3d_amd import api
    a, b, ref = H.random_rows(613, 307, 61)
    ix = ctx.index_create(a, binary=True)
    ctxs = [api.Context(0) for _ in range(8)]
    out = [None] * 8
    start = threading.Barrier(8)

    def work(t):
        c = ctxs[t]
        c.set_knn_hamming_tiles(True)
        before = c.stats().n_views_staged
        start.wait(timeout=60)
        res = []
        for k in (3, 8):
            idx, dist = c.index_knn(ix, b, k)
            res.append((k, idx, dist, c.stats()))
        out[t] = (res, c.stats().n_views_staged - before)

    try:
        th = [threading.Thread(target=work, args=(t,)) for t in range(8)]
        for x in th: x.start()
        for x in th: x.join()
        for t in range(8):
            assert out[t] is not None, f"thread {t} raised"
            res, staged = out[t]
            assert staged == 2                                             # two searches, two query uploads, no dataset
            for k, idx, dist, s in res:
                _assert_equal(idx, dist, ref, k, f"thread {t}, k = {k}")
                _assert_counters(s, b.shape[0], 1, f"thread {t}, k = {k}")
        # the session context, switch off, on the same index afterwards: the popcount kernel, the same answer
        idx, dist = ctx.index_knn(ix, b, 3)
        _assert_equal(idx, dist, ref, 3, "session context")
        _assert_counters(ctx.stats(), b.shape[0], 0, "session context")
    finally:
        for c in ctxs: c.close()
        ix.close()


# ---------------------------------------------------------------------------------------------------- 7. history
def test_history_independence(ctx):
    """knn(k = 3) with the switch on returns identical bytes whatever the context ran before"""
    from regard3d_amd import synth
    a, b, ref = H.random_rows(300, 90, 61)

    def run():
        idx, dist = _check(ctx, a, b, 3, ref, "history")
        return idx.tobytes(), dist.tobytes()

    first = run()
    # a 2-NN call on the i8 tiles
    ctx.set_hamming_mfma(True)
    try:
        ctx.knn2(a, b, binary=True)
        assert ctx.stats().n_hamming_mfma == 1
    finally:
        ctx.set_hamming_mfma(False)
    assert run() == first
    # a match_pairs call on a binary scene
    sc = synth.make_scene(3, 300, "akaze", seed=77)
    ctx.clear_images()
    for i in range(sc.n_images):
        ctx.set_image(i, sc.descs[i], sc.xys[i], int(sc.widths[i]), int(sc.heights[i]), binary=True)
    ctx.match_pairs(sc.exhaustive_pairs(), 0.8, False)
    assert run() == first
    ctx.clear_images()
    # a k-NN call with the switch off (the popcount K-list kernel)
    ctx.knn(a, b, 8, binary=True)
    assert ctx.stats().n_knn_hamming_tiles == 0
    assert run() == first
