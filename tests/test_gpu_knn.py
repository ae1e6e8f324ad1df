"""r3dm_knn / r3dm_index_knn (k = 1 .. 8) on the device against the numpy restatement (knn_restatement.py): indices AND distances
bit for bit, whichever way a query took -- certified by the nominator or redone by the exact scan."""
import functools
import os

import numpy as np
import pytest

import certificate_cases as CC
import knn_restatement as R

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KS = (1, 2, 3, 4, 5, 8)
# (dim, rows of the dataset, queries): the certificate cases' shapes -- ragged last tiles on both sides -- and a length without a
# tensor kernel
SHAPES = {128: CC._SHAPES[128], 144: CC._SHAPES[144], 64: CC._SHAPES[64], 256: CC._SHAPES[256], 37: CC._SHAPES[37], 300: (300, 40)}


def _check(ctx, a, b, k, binary=False, ref=None):
    idx, dist = ctx.knn(a, b, k, binary=binary)
    ri, rd = ref if ref is not None else R.knn(a, b, k, binary=binary)
    assert idx.shape == (b.shape[0], k) and dist.shape == (b.shape[0], k)
    bad = np.flatnonzero((idx != ri[:, :k]).any(1) | (dist != rd[:, :k]).any(1))
    assert bad.size == 0, f"{bad.size} of {len(idx)} queries differ, first {bad[:5]}: got {idx[bad[:2]]} {dist[bad[:2]]}, want {ri[bad[:2], :k]} {rd[bad[:2], :k]}"
    return ctx.stats()


@functools.lru_cache(maxsize=None)
def _shape_data(dim, kind):
    """(dataset, query, the restatement's 8-NN): computed once, the first k columns are the k-NN"""
    nI, nJ = SHAPES[dim]
    rng = np.random.default_rng([dim, len(kind)])
    if kind == "real":
        a = rng.standard_normal((nI, dim)).astype(np.float32); b = rng.standard_normal((nJ, dim)).astype(np.float32)
    else:                                      # integer bins: u8 rows, or the same values as f32
        a = rng.integers(0, 256, (nI, dim)).astype(np.uint8); b = rng.integers(0, 256, (nJ, dim)).astype(np.uint8)
        b[:nJ // 4] = a[:nJ // 4]                  # distance-0 neighbours
        a[5] = a[4]; a[nI - 1] = a[4]              # and exact ties
        if kind == "int_f32":
            a = a.astype(np.float32); b = b.astype(np.float32)
    ref = R.knn(a, b, 8)
    for x in (a, b) + ref:
        x.setflags(write=False)
    return a, b, ref


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("kind", ("real", "u8", "int_f32"))
@pytest.mark.parametrize("dim", sorted(SHAPES))
def test_shapes(ctx, dim, kind, k):
    a, b, ref = _shape_data(dim, kind)
    s = _check(ctx, a, b, k, ref=ref)
    assert s.n_queries == b.shape[0]
    if dim == 300:                             # no tensor kernel: every query is scanned exactly
        assert s.n_exact_fallback == b.shape[0]


# ---------------------------------------------------------------------------------------------------- edges
@pytest.mark.parametrize("k,n", [(3, 3), (3, 4), (8, 8), (8, 9), (3, 9), (8, 31), (3, 32), (8, 32), (8, 33), (3, 33)])
def test_small_datasets(ctx, k, n):
    rng = np.random.default_rng([k, n])
    a = rng.standard_normal((n, 128)).astype(np.float32); b = rng.standard_normal((40, 128)).astype(np.float32)
    _check(ctx, a, b, k)
    _check(ctx, (a * 16).round().astype(np.float32), (b * 16).round().astype(np.float32), k)


@pytest.mark.parametrize("nq", (1, 33, 257))
def test_query_counts(ctx, nq):
    rng = np.random.default_rng(nq)
    a = rng.standard_normal((101, 128)).astype(np.float32); b = rng.standard_normal((nq, 128)).astype(np.float32)
    for k in (3, 8):
        _check(ctx, a, b, k)


def test_one_row_dataset(ctx):
    rng = np.random.default_rng(1)
    a = rng.standard_normal((1, 128)).astype(np.float32); b = rng.standard_normal((35, 128)).astype(np.float32)
    _check(ctx, a, b, 1)
    au = rng.integers(0, 256, (1, 64), dtype=np.uint8); bu = rng.integers(0, 256, (35, 64), dtype=np.uint8)
    _check(ctx, au, bu, 1)
    _check(ctx, au, bu, 1, binary=True)


def test_k2_is_knn2(ctx):
    a, b, _ = _shape_data(128, "real")
    i2, d2 = ctx.knn2(a, b)
    ik, dk = ctx.knn(a, b, 2)
    assert np.array_equal(ik, i2) and np.array_equal(dk, d2)
    i1, d1 = ctx.knn(a, b, 1)
    assert np.array_equal(i1[:, 0], i2[:, 0]) and np.array_equal(d1[:, 0], d2[:, 0])


def test_bad_k_raises(ctx):
    from regard3d_amd.api import R3dmError
    a = np.zeros((5, 128), np.float32); b = np.zeros((4, 128), np.float32)
    for k in (0, 9, 6):                        # k < 1, k > R3DM_KNN_MAX, k > rows
        with pytest.raises(R3dmError):
            ctx.knn(a, b, k)


# ---------------------------------------------------------------------------------------------------- planted neighbours
N_PLANT = 3 * 32 + 11                          # three full tiles and 11 rows
_HALF0 = [r for r in range(32) if CC._lane_half(r) == 0]          # rows 0..3, 8..11, 16..19, 24..27 of a tile
_HALF1 = [r for r in range(32) if CC._lane_half(r) == 1]


def _placement(name, k):
    n = k + 1
    if name == "one_half_of_one_tile":
        return [32 + r for r in _HALF0[:n]]
    if name == "alternating_halves":
        return [32 + (_HALF0 if i % 2 == 0 else _HALF1)[i // 2] for i in range(n)]
    if name == "one_per_tile":
        return [32 * (i % 4) + 9 - (i // 4) for i in range(n)]          # tiles 0, 1, 2, 3 (the partial one), round robin
    if name == "last_partial_tile":
        return [96 + i for i in range(n)]
    assert name == "first_and_last_row"
    rows = [0] + [40 + 3 * i for i in range(n - 2)] + [50 + 3 * n]
    rows[k - 1], rows[-1] = N_PLANT - 1, rows[k - 1]                   # nearest at row 0, the k-th at the last row
    return rows


@pytest.mark.parametrize("k", (4, 8))
@pytest.mark.parametrize("name", ("one_half_of_one_tile", "alternating_halves", "one_per_tile", "last_partial_tile", "first_and_last_row"))
def test_planted_neighbours(ctx, name, k):
    """the k + 1 nearest rows of query 0 at known places and gaps.  A per-half list shallower than k, or a bound that is the k-th key
    instead of the (k + 1)-th, loses a neighbour in the first placement."""
    rng = np.random.default_rng([k, len(name)])
    a = rng.standard_normal((N_PLANT, 128)).astype(np.float32)          # ~ 256 away from any query
    b = rng.standard_normal((37, 128)).astype(np.float32)
    rows = _placement(name, k)
    assert len(set(rows)) == k + 1 and max(rows) < N_PLANT
    for i, r in enumerate(rows):
        u = rng.standard_normal(128); u /= np.linalg.norm(u)
        a[r] = (b[0] + np.sqrt(1.0 + 0.5 * i) * u).astype(np.float32)   # squared distances 1, 1.5, 2, ...
    idx, _ = ctx.knn(a, b, k)
    assert idx[0].tolist() == rows[:k]
    _check(ctx, a, b, k)
    ai = (a * 8).round().astype(np.float32); bi = (b * 8).round().astype(np.float32)      # the same on an exact pair
    _check(ctx, ai, bi, k)


# ---------------------------------------------------------------------------------------------------- ties
def test_ties_duplicated_rows(ctx):
    rng = np.random.default_rng(70)
    a = rng.integers(0, 256, (70, 128), dtype=np.uint8)
    a[40:48] = a[3]; a[64:70] = a[3]
    b = np.concatenate([a[3:4], rng.integers(0, 256, (20, 128), dtype=np.uint8)])
    idx, dist = ctx.knn(a, b, 8)
    assert idx[0].tolist() == [3, 40, 41, 42, 43, 44, 45, 46] and (dist[0] == 0).all()
    _check(ctx, a, b, 8)
    _check(ctx, a, b, 3)


def test_tie_of_kth_and_next_across_halves(ctx):
    """k = 8.  Rows at squared distances 1 .. 7 from query 0 fill a lane half's list together with row A at distance T; rows B (other
    half) and C (A's half) are at T too, A < B < C: the k-th and the (k + 1)-th neighbour tie across the halves.  Lists are k deep per
    half, so A and B alone would both be nominated and certify in index order without the exact scan; C is what leaves a tied row
    UN-nominated (the half's bound equals e_k), and the strict comparison must send the query to the exact scan."""
    rng = np.random.default_rng(8)
    a = rng.integers(100, 156, (107, 128)).astype(np.float32)
    b = rng.integers(100, 156, (9, 128)).astype(np.float32)
    near = [32 + r for r in _HALF0[:7]]                                # half 0
    A, B, C = 32 + _HALF0[7], 32 + _HALF1[7], 64 + _HALF0[0]
    assert A < B < C
    for i, r in enumerate(near):
        a[r] = b[0]; a[r, :i + 1] += 1.0                               # squared distance i + 1
    for r in (A, B, C):
        a[r] = b[0]; a[r, r % 64] += 3.0                               # T = 9
    idx, dist = ctx.knn(a, b, 8)
    s = ctx.stats()
    assert idx[0].tolist() == near + [A] and dist[0].tolist() == [1, 2, 3, 4, 5, 6, 7, 9]
    assert s.n_exact_fallback >= 1
    _check(ctx, a, b, 8)
    # without C both tied rows are nominees: the same answer, in index order
    a[C] = a[0]
    idx, _ = ctx.knn(a, b, 8)
    assert idx[0].tolist() == near + [A]
    i9, _ = R.knn(a, b, 9)
    assert i9[0, 8] == B


# ---------------------------------------------------------------------------------------------------- certificate under stress
@pytest.mark.parametrize("k", (3, 8))
@pytest.mark.parametrize("case,lo,hi", [("offset_f32_d128_t0", 0.0, 0.0), ("offset_f32_d128_t20", None, None), ("offset_f32_d128_t1000", 0.95, 1.0),
                                        ("mixed_large_last_f32", None, None), ("mixed_large_row0_f32", None, None)])
def test_certificate_under_stress(ctx, case, lo, hi, k):
    a, b = CC.CASES[case].make()
    s = _check(ctx, a, b, k)
    share = s.n_exact_fallback / b.shape[0]
    print(f"{case}, k = {k}: exact-scan share {share:.3f}")
    if lo is not None:
        assert lo <= share <= hi


# ---------------------------------------------------------------------------------------------------- Hamming
@pytest.mark.parametrize("k", (3, 8))
@pytest.mark.parametrize("nbytes", (64, 61, 32))
def test_hamming(ctx, nbytes, k):
    rng = np.random.default_rng(nbytes)
    a = rng.integers(0, 256, (1000, nbytes), dtype=np.uint8)
    b = rng.integers(0, 256, (700, nbytes), dtype=np.uint8)
    b[:100] = a[:100] ^ (rng.random((100, nbytes)) < 0.05).astype(np.uint8)
    _check(ctx, a, b, k, binary=True)


# ---------------------------------------------------------------------------------------------------- reference-built
def test_liop_fixture_3nn(ctx):
    A, B, ri, rd = R.liop_fixture(GOLD)
    idx, dist = ctx.knn(A, B, 3)
    i9, d9 = R.liop_knn9(GOLD)
    assert np.array_equal(idx, i9[:, :3]) and np.array_equal(dist, d9[:, :3])
    R.check_against_reference(idx, dist, ri, rd, d9[:, 3], 144, "device, LIOP fixture, k = 3")


def test_liop_live_reference_8nn(ctx, oracle):
    if oracle.ref_lib() is None:
        pytest.skip("oracle/_ref did not travel with this tree: the committed-fixture check (test_liop_fixture_3nn) ran")
    A, B, _, _ = R.liop_fixture(GOLD)
    li, ld = oracle.ref_knn(A, B, 9)
    idx, dist = ctx.knn(A, B, 8)
    R.check_against_reference(idx, dist, li, ld, ld[:, 8], 144, "device, LIOP live reference, k = 8")


# ---------------------------------------------------------------------------------------------------- switches, index, history
def test_switches_ignored_from_k3(ctx):
    a, b, ref = _shape_data(128, "int_f32")
    ar, br, refr = _shape_data(144, "real")
    rng = np.random.default_rng(3)
    ha = rng.integers(0, 256, (300, 61), dtype=np.uint8); hb = rng.integers(0, 256, (90, 61), dtype=np.uint8)
    plain = [ctx.knn(a, b, 3), ctx.knn(ar, br, 3), ctx.knn(ha, hb, 3, binary=True)]
    ctx.set_integer_mfma(True); ctx.set_split_mfma(True); ctx.set_hamming_mfma(True)
    try:
        for (x, y, binary), want in zip(((a, b, False), (ar, br, False), (ha, hb, True)), plain):
            got = ctx.knn(x, y, 3, binary=binary)
            s = ctx.stats()
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            assert s.n_integer_mfma == 0 and s.n_split_mfma == 0 and s.n_hamming_mfma == 0
        # the 2-NN call still takes its opt-in paths
        ctx.knn2(a, b); assert ctx.stats().n_integer_mfma == 1
        ctx.knn2(ar, br); assert ctx.stats().n_split_mfma == 1
        ctx.knn2(ha, hb, binary=True); assert ctx.stats().n_hamming_mfma == 1
    finally:
        ctx.set_integer_mfma(False); ctx.set_split_mfma(False); ctx.set_hamming_mfma(False)


def test_index_knn(ctx):
    from regard3d_amd import api
    other = api.Context(0)
    try:
        for kind, dim in (("real", 144), ("u8", 128)):
            a, b, ref = _shape_data(dim, kind)
            ix = other.index_create(a)             # created before this context's -- or any -- k-NN call on it
            for k in (3, 8):
                for c in (other, ctx):
                    idx, dist = c.index_knn(ix, b, k)
                    assert np.array_equal(idx, ref[0][:, :k]) and np.array_equal(dist, ref[1][:, :k])
                d = ctx.knn(a, b, k)
                assert np.array_equal(d[0], ref[0][:, :k]) and np.array_equal(d[1], ref[1][:, :k])
            i2, d2 = ctx.index_knn2(ix, b)
            ik, dk = ctx.index_knn(ix, b, 2)
            assert np.array_equal(ik, i2) and np.array_equal(dk, d2)
            for k in (0, 9):
                with pytest.raises(api.R3dmError):
                    ctx.index_knn(ix, b, k)
            small = ctx.index_create(a[:5])
            with pytest.raises(api.R3dmError):
                ctx.index_knn(small, b, 6)             # k > rows
            small.close(); ix.close()
    finally:
        other.close()


def test_history(ctx):
    """a match_pairs graph is the same before and after interleaved knn(k = 8) calls; a knn result is the same on a fresh context"""
    from regard3d_amd import api, synth
    sc = synth.make_scene(3, 300, "sift", seed=77)
    a, b, ref = _shape_data(144, "real")
    au, bu, refu = _shape_data(128, "u8")

    def graph():
        ctx.clear_images()
        for i in range(sc.n_images):
            ctx.set_image(i, sc.descs[i], sc.xys[i], int(sc.widths[i]), int(sc.heights[i]))
        g = ctx.match_pairs(sc.exhaustive_pairs(), 0.6, True)
        return g.pairs.copy(), g.offsets.copy(), g.matches.copy()

    g0 = graph()
    used = [ctx.knn(a, b, 8), ctx.knn(au, bu, 8)]
    g1 = graph()
    used += [ctx.knn(a, b, 8)]
    ctx.clear_images()
    assert all(np.array_equal(x, y) for x, y in zip(g0, g1))
    fresh_ctx = api.Context(0)
    try:
        fresh = [fresh_ctx.knn(a, b, 8), fresh_ctx.knn(au, bu, 8)]
    finally:
        fresh_ctx.close()
    for (ui, ud), (fi, fd) in zip(used, fresh + fresh[:1]):
        assert np.array_equal(ui, fi) and np.array_equal(ud, fd)
    assert np.array_equal(used[0][0], ref[0]) and np.array_equal(used[1][0], refu[0])
