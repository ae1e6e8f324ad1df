"""r3dm_knn / r3dm_index_knn (k >= 3) with r3dm_set_knn_narrow_tiles on: the K-list kernels of the bf16 tiles and the split-f16 planes
(kernels_match_knn16.hip) against the numpy restatement, indices AND distances bit for bit, and the path every call took against
the routing predicate restated in knn_narrow_cases.py.  Every case switches the session context's flag off again."""
import contextlib
import threading

import numpy as np
import pytest

import certificate_cases as CC
import knn_narrow_cases as N
import knn_restatement as R
import test_gpu_knn as T          # its shapes, data builder (one cached reference per shape) and planted-neighbour placements

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def narrow(ctx):
    ctx.set_knn_narrow_tiles(True)
    try:
        yield ctx
    finally:
        ctx.set_knn_narrow_tiles(False)


def _check(ctx, a, b, k, binary=False, ref=None, path=None, what=""):
    """knn with the switch on equals the restatement and ran where the predicate says (or where `path` says)"""
    with narrow(ctx):
        idx, dist = ctx.knn(a, b, k, binary=binary)
        s = ctx.stats()
    ri, rd = ref if ref is not None else R.knn(a, b, k, binary=binary)
    bad = np.flatnonzero((idx != ri[:, :k]).any(1) | (dist != rd[:, :k]).any(1))
    assert bad.size == 0, f"{what}: {bad.size} of {len(idx)} queries differ, first {bad[:5]}: got {idx[bad[:2]]} {dist[bad[:2]]}, want {ri[bad[:2], :k]} {rd[bad[:2], :k]}"
    want = N.expected_path(a, b, binary)
    assert path is None or path == want, (what, path, want)
    N.assert_path(s, want, b.shape[0], what)
    assert s.n_queries == b.shape[0]
    return s


# ---------------------------------------------------------------------------------------------------- 1. routing and counters
def test_routing_and_counters(ctx):
    a, b, ref = T._shape_data(128, "int_f32")
    ar, br, refr = T._shape_data(144, "real")
    rng = np.random.default_rng(3)
    ha = rng.integers(0, 256, (300, 61), dtype=np.uint8); hb = rng.integers(0, 256, (90, 61), dtype=np.uint8)
    s = _check(ctx, a, b, 3, ref=ref, path="integer")
    assert (s.n_knn_integer_tiles, s.n_knn_split_tiles, s.n_exact_fallback) == (1, 0, 0)
    s = _check(ctx, ar, br, 3, ref=refr, path="split")
    assert (s.n_knn_integer_tiles, s.n_knn_split_tiles) == (0, 1)
    s = _check(ctx, ha, hb, 3, binary=True, path="hamming")
    assert (s.n_knn_integer_tiles, s.n_knn_split_tiles) == (0, 0)
    # switch off: the f32 tiles, both counters 0, the same answers
    for x, y, r in ((a, b, ref), (ar, br, refr)):
        idx, dist = ctx.knn(x, y, 3)
        s = ctx.stats()
        assert (s.n_knn_integer_tiles, s.n_knn_split_tiles) == (0, 0)
        assert np.array_equal(idx, r[0][:, :3]) and np.array_equal(dist, r[1][:, :3])
    # k <= 2 is the 2-NN path whatever the switch says
    i2, d2 = ctx.knn2(a, b)
    with narrow(ctx):
        ik, dk = ctx.knn(a, b, 2)
        s = ctx.stats()
        i1, d1 = ctx.knn(ar, br, 1)
    assert np.array_equal(ik, i2) and np.array_equal(dk, d2)
    assert (s.n_knn_integer_tiles, s.n_knn_split_tiles) == (0, 0)
    assert np.array_equal(i1[:, 0], refr[0][:, 0]) and np.array_equal(d1[:, 0], refr[1][:, 0])


# ---------------------------------------------------------------------------------------------------- 2. shapes
_WANT = {("real", 37): "split", ("real", 64): "split", ("real", 128): "split", ("real", 144): "split", ("real", 256): "split",
         ("int", 37): "integer", ("int", 64): "integer", ("int", 128): "integer", ("int", 144): "f32", ("int", 256): "f32"}


@pytest.mark.parametrize("k", (3, 4, 5, 8))
@pytest.mark.parametrize("kind", ("real", "u8", "int_f32"))
@pytest.mark.parametrize("dim", sorted(T.SHAPES))
def test_shapes(ctx, dim, kind, k):
    a, b, ref = T._shape_data(dim, kind)
    path = "scan" if dim == 300 else _WANT[("real" if kind == "real" else "int", dim)]
    _check(ctx, a, b, k, ref=ref, path=path, what=f"D = {dim}, {kind}")


@pytest.mark.parametrize("k", (3, 4, 5, 8))
def test_shape_256_on_the_integer_tiles(ctx, k):
    """values 0 .. 127 keep 2 D mI mJ below 2^24 at D = 256: the G = 32 integer kernel, one query tile per wave"""
    nI, nJ = CC._SHAPES[256]
    a, b = N.u8_tied(nI, nJ, 256, 128)
    _check(ctx, a, b, k, path="integer")
    _check(ctx, a.astype(np.float32), b.astype(np.float32), k, path="integer")


# ---------------------------------------------------------------------------------------------------- 3. small and ragged
@pytest.mark.parametrize("k,n", [(3, 3), (3, 4), (3, 31), (3, 32), (3, 33), (8, 8), (8, 9), (8, 31), (8, 32), (8, 33)])
def test_small_datasets(ctx, k, n):
    rng = np.random.default_rng([k, n])
    a = rng.standard_normal((n, 128)).astype(np.float32); b = rng.standard_normal((40, 128)).astype(np.float32)
    _check(ctx, a, b, k, path="split")
    _check(ctx, (a * 16).round().astype(np.float32), (b * 16).round().astype(np.float32), k, path="integer")


@pytest.mark.parametrize("nq", (1, 33, 257))
def test_query_counts(ctx, nq):
    rng = np.random.default_rng(nq)
    a = rng.standard_normal((101, 128)).astype(np.float32); b = rng.standard_normal((nq, 128)).astype(np.float32)
    for k in (3, 8):
        _check(ctx, a, b, k, path="split")
        _check(ctx, (a * 16).round().astype(np.float32), (b * 16).round().astype(np.float32), k, path="integer")


def test_one_row_dataset(ctx):
    rng = np.random.default_rng(1)
    a = rng.standard_normal((1, 128)).astype(np.float32); b = rng.standard_normal((35, 128)).astype(np.float32)
    _check(ctx, a, b, 1, path="split")
    au = rng.integers(0, 256, (1, 64), dtype=np.uint8); bu = rng.integers(0, 256, (35, 64), dtype=np.uint8)
    _check(ctx, au, bu, 1, path="integer")


# ---------------------------------------------------------------------------------------------------- 4. planted neighbours
@pytest.mark.parametrize("k", (4, 8))
@pytest.mark.parametrize("name", ("one_half_of_one_tile", "alternating_halves", "one_per_tile", "last_partial_tile", "first_and_last_row"))
def test_planted_neighbours(ctx, name, k):
    """the k + 1 nearest rows of query 0 at known places and gaps (test_gpu_knn.py's placements).  A per-half list shallower than k,
    or a bound taken one key too early, loses a neighbour in the first placement."""
    rng = np.random.default_rng([k, len(name)])
    a = rng.standard_normal((T.N_PLANT, 128)).astype(np.float32)
    b = rng.standard_normal((37, 128)).astype(np.float32)
    rows = T._placement(name, k)
    for i, r in enumerate(rows):
        u = rng.standard_normal(128); u /= np.linalg.norm(u)
        a[r] = (b[0] + np.sqrt(1.0 + 0.5 * i) * u).astype(np.float32)     # squared distances 1, 1.5, 2, ...
    with narrow(ctx):
        idx, _ = ctx.knn(a, b, k)
    assert idx[0].tolist() == rows[:k]
    _check(ctx, a, b, k, path="split")
    ai = (a * 8).round().astype(np.float32); bi = (b * 8).round().astype(np.float32)      # the same rows on the integer tiles
    _check(ctx, ai, bi, k, path="integer")


# ---------------------------------------------------------------------------------------------------- 5. ties on the integer tiles
def test_ties_duplicated_rows(ctx):
    rng = np.random.default_rng(70)
    a = rng.integers(0, 256, (70, 128), dtype=np.uint8)
    a[40:48] = a[3]; a[64:70] = a[3]
    b = np.concatenate([a[3:4], rng.integers(0, 256, (20, 128), dtype=np.uint8)])
    with narrow(ctx):
        idx, dist = ctx.knn(a, b, 8)
    assert idx[0].tolist() == [3, 40, 41, 42, 43, 44, 45, 46] and (dist[0] == 0).all()
    _check(ctx, a, b, 8, path="integer")
    _check(ctx, a, b, 3, path="integer")


def test_tie_of_kth_and_next_across_halves(ctx):
    """the layout on which the f32 K-list kernel must scan (a tied row stays un-nominated: its bound equals e_k).  The integer tiles'
    lists are exact: near + [A] comes out of the merge, nothing is scanned"""
    a, b, near, A, B, C = N.tie_across_halves()
    with narrow(ctx):
        idx, dist = ctx.knn(a, b, 8)
        s = ctx.stats()
    assert idx[0].tolist() == near + [A] and dist[0].tolist() == [1, 2, 3, 4, 5, 6, 7, 9]
    assert s.n_knn_integer_tiles == 1 and s.n_exact_fallback == 0
    _check(ctx, a, b, 8, path="integer")
    idx, _ = ctx.knn(a, b, 8)                                              # (switch off: the f32 path scans this query)
    assert idx[0].tolist() == near + [A] and ctx.stats().n_exact_fallback >= 1


# ---------------------------------------------------------------------------------------------------- 6. integer eligibility edges
def _edge(name):
    rng = np.random.default_rng(len(name))
    a = rng.integers(0, 256, (203, 128)).astype(np.float32); b = rng.integers(0, 256, (77, 128)).astype(np.float32)
    b[:10] = a[:10]; a[7] = a[6]
    if name == "dataset_reaches_256":          # 2 D mI mJ = 2 x 128 x 256 x 255 < 2^24: still exact, still bf16
        a[11, 3] = 256.0
    elif name == "both_reach_256":             # 2 D mI mJ = 2^24: not exact any more
        a[11, 3] = 256.0; b[12, 5] = 256.0
    elif name == "negative_integers":          # D (mI + mJ)^2 = 128 x 200^2 < 2^24
        a = rng.integers(-100, 101, (203, 128)).astype(np.float32); b = rng.integers(-100, 101, (77, 128)).astype(np.float32)
        b[:10] = a[:10]; a[7] = a[6]
    elif name == "negative_integers_too_large":
        a = rng.integers(-200, 201, (203, 128)).astype(np.float32); b = rng.integers(-200, 201, (77, 128)).astype(np.float32)
        a[0, 0] = -200.0; b[0, 0] = 200.0
    elif name == "one_value_257":
        a[11, 3] = 257.0
    else:
        assert name == "one_non_integer_in_the_queries"
        b[20, 9] += 0.5
    return a, b


@pytest.mark.parametrize("name,path", [("dataset_reaches_256", "integer"), ("both_reach_256", "f32"), ("negative_integers", "integer"),
                                       ("negative_integers_too_large", "f32"), ("one_value_257", "f32"),
                                       ("one_non_integer_in_the_queries", "split")])
def test_integer_eligibility_edges(ctx, name, path):
    a, b = _edge(name)
    ref = R.knn(a, b, 8)
    for k in (3, 8):
        _check(ctx, a, b, k, ref=ref, path=path, what=name)


# ---------------------------------------------------------------------------------------------------- 7. split certificate under stress
@pytest.mark.parametrize("k", (3, 8))
@pytest.mark.parametrize("case,lo,hi", N.SPLIT_CASES)
def test_split_certificate_under_stress(ctx, case, lo, hi, k):
    a, b, ref = N.case_views(case)
    s = _check(ctx, a, b, k, ref=ref, path="split", what=case)
    share = s.n_exact_fallback / b.shape[0]
    print(f"{case}, k = {k}: exact-scan share {share:.3f}")
    if lo is not None:
        assert lo <= share <= hi


# ---------------------------------------------------------------------------------------------------- 8. index
@pytest.mark.parametrize("kind,dim,path", [("u8", 128, "integer"), ("real", 144, "split")])
def test_index_knn_from_eight_threads(ctx, kind, dim, path):
    """one index, built with every switch off (rows only); eight host threads, each with a context of its own and the switch on,
    search it at once: whichever comes first stages the index's bf16 tiles / split planes under the index's lock, every thread gets
    the restatement's answer on the narrow tiles, and no search re-stages the dataset (a search uploads its queries only)"""
    from regard3d_amd import api
    a, b, ref = T._shape_data(dim, kind)
    ix = ctx.index_create(a)
    ctxs = [api.Context(0) for _ in range(8)]
    out = [None] * 8
    start = threading.Barrier(8)

    def work(t):
        c = ctxs[t]
        c.set_knn_narrow_tiles(True)
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
                assert np.array_equal(idx, ref[0][:, :k]) and np.array_equal(dist, ref[1][:, :k]), (t, k)
                N.assert_path(s, path, b.shape[0], f"thread {t}, k = {k}")
        # the session context, switch off, on the same index afterwards: the f32 tiles, the same answer
        idx, dist = ctx.index_knn(ix, b, 3)
        s = ctx.stats()
        assert np.array_equal(idx, ref[0][:, :3]) and np.array_equal(dist, ref[1][:, :3])
        assert (s.n_knn_integer_tiles, s.n_knn_split_tiles) == (0, 0)
    finally:
        for c in ctxs: c.close()
        ix.close()


# ---------------------------------------------------------------------------------------------------- 9. history
def test_history_independence(ctx):
    """knn(k = 3) with the switch on returns identical bytes whatever the context ran before"""
    from regard3d_amd import synth
    a, b, ref = T._shape_data(128, "u8")
    ar, br, refr = T._shape_data(144, "real")

    def both():
        with narrow(ctx):
            ri = ctx.knn(a, b, 3); si = ctx.stats()
            rr = ctx.knn(ar, br, 3); sr = ctx.stats()
        N.assert_path(si, "integer", b.shape[0]); N.assert_path(sr, "split", br.shape[0])
        return [x.tobytes() for x in ri + rr]

    first = both()
    assert np.array_equal(np.frombuffer(first[0], np.int32).reshape(-1, 3), ref[0][:, :3])
    # a 2-NN call with the old switches on
    ctx.set_integer_mfma(True); ctx.set_split_mfma(True)
    try:
        ctx.knn2(a, b); ctx.knn2(ar, br)
    finally:
        ctx.set_integer_mfma(False); ctx.set_split_mfma(False)
    assert both() == first
    # a match_pairs call
    sc = synth.make_scene(3, 300, "sift", seed=77)
    ctx.clear_images()
    for i in range(sc.n_images):
        ctx.set_image(i, sc.descs[i], sc.xys[i], int(sc.widths[i]), int(sc.heights[i]))
    ctx.match_pairs(sc.exhaustive_pairs(), 0.6, True)
    assert both() == first
    ctx.clear_images()
    # a k-NN call on the other path (f32 K-lists, popcount lists, exact scan)
    ctx.knn(a, b, 8); ctx.knn(ar, br, 8)
    x, y, _ = T._shape_data(300, "real")
    with narrow(ctx):
        ctx.knn(x, y, 5)
    assert both() == first
    # toggling the switch
    ctx.set_knn_narrow_tiles(True); ctx.set_knn_narrow_tiles(False); ctx.set_knn_narrow_tiles(True); ctx.set_knn_narrow_tiles(False)
    assert both() == first
