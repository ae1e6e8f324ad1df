"""k nearest neighbours restated in numpy: what r3dm_knn / r3dm_index_knn must return, bit for bit.

Distances are float32 in the reference's order (OpenMVG L2<float>): per block of four dimensions
    result += ((d0^2 + d1^2) + d2^2) + d3^2
then a scalar tail; every operation rounds to float32, no fused multiply-add.  Hamming distances are popcounts of the xor.
Selection is the project's one order, (distance, dataset row): equal distances, lowest row first (np.lexsort).

Not a test module (no test_ prefix): imported by test_knn_restatement.py, test_gpu_knn.py and test_cpp_knn_adapter.py.
"""
import numpy as np

U = 2.0 ** -24          # unit roundoff of float32


def l2_ref_order(A, Q):
    """A [nI, D], Q [nq, D] (any real dtype; taken as float32) -> [nq, nI] float32 squared distances in the reference order"""
    A = np.asarray(A).astype(np.float32); Q = np.asarray(Q).astype(np.float32)
    nI, D = A.shape
    out = np.zeros((Q.shape[0], nI), np.float32)
    k = 0
    while k + 3 < D:
        d = [A[None, :, k + i] - Q[:, None, k + i] for i in range(4)]
        s = d[0] * d[0] + d[1] * d[1]
        s = s + d[2] * d[2]
        s = s + d[3] * d[3]
        out = out + s
        k += 4
    while k < D:
        d0 = A[None, :, k] - Q[:, None, k]
        out = out + d0 * d0
        k += 1
    return out


_POP8 = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1).astype(np.uint32)


def hamming_all(A, Q):
    """A [nI, B], Q [nq, B] uint8 rows -> [nq, nI] uint32 Hamming distances"""
    A = np.ascontiguousarray(A, np.uint8); Q = np.ascontiguousarray(Q, np.uint8)
    out = np.zeros((Q.shape[0], A.shape[0]), np.uint32)
    for b in range(A.shape[1]):
        out += _POP8[A[None, :, b] ^ Q[:, None, b]]
    return out


def knn(A, Q, k, binary=False, chunk=256):
    """-> (idx [nq, k] int32, dist [nq, k] float32): the k smallest of every query under (distance, dataset row)"""
    A = np.asarray(A); Q = np.asarray(Q)
    nq = Q.shape[0]
    assert 1 <= k <= A.shape[0]
    idx = np.zeros((nq, k), np.int32); dist = np.zeros((nq, k), np.float32)
    rows = np.arange(A.shape[0])
    for s in range(0, nq, chunk):
        d = hamming_all(A, Q[s:s + chunk]) if binary else l2_ref_order(A, Q[s:s + chunk])
        o = np.lexsort((np.broadcast_to(rows, d.shape), d), axis=1)[:, :k]
        idx[s:s + chunk] = o
        dist[s:s + chunk] = np.take_along_axis(d, o, 1).astype(np.float32)
    return idx, dist


def tol(d, dim=144):
    """|float32 sum of dim squared differences in ANY order - the exact sum| <= (dim + 2) u d (first order); two such sums differ by
    at most twice that"""
    return 2.0 * (dim + 2) * U * np.asarray(d, np.float64)


def clear_rows(dists, j, dim=144):
    """rows on which the INDEX of (zero-based) column j is determined whatever the summation order: every adjacent gap among the
    columns 0 .. j + 1 of dists exceeds TOL(d_i) + TOL(d_{i+1})"""
    r = np.asarray(dists, np.float64)
    ok = np.ones(r.shape[0], bool)
    for i in range(j + 1):
        ok &= (r[:, i + 1] - r[:, i]) > tol(r[:, i], dim) + tol(r[:, i + 1], dim)
    return ok


CAP = 0.05            # at most this share of the rows may be excluded from an index check


def check_against_reference(idx, dist, ref_idx, ref_dist, next_dist, dim, what, exact=False):
    """(idx, dist) [n, k] against a reference-built k-NN whose float32 sums ran in another order: distances within TOL on every
    column and the index of a column equal on the rows clear_rows leaves -- or, `exact` (integer rows: every order gives the same
    sums), distances identical and indices equal on the rows without an exact tie among the first k + 1.  next_dist: the
    (k + 1)-th distance.  Prints how many rows each check excludes; more than CAP of them fails."""
    k = idx.shape[1]
    rd = np.asarray(ref_dist)[:, :k].astype(np.float64)
    ri = np.asarray(ref_idx)[:, :k]
    if exact:
        assert np.array_equal(dist, np.asarray(ref_dist)[:, :k])
        d9 = np.concatenate([np.asarray(ref_dist, np.float32)[:, :k], np.asarray(next_dist, np.float32)[:, None]], 1)
        clear = ~(np.diff(d9, axis=1) == 0).any(1)
        excluded = int((~clear).sum())
        print(f"{what}: {excluded} of {len(idx)} rows hold an exact tie among the first {k + 1}")
        assert excluded <= CAP * len(idx)
        assert np.array_equal(idx[clear], ri[clear])
        return
    assert (np.abs(dist.astype(np.float64) - rd) <= tol(rd, dim)).all()
    full = np.concatenate([rd, np.asarray(next_dist, np.float64)[:, None]], 1)
    for j in range(k):
        clear = clear_rows(full, j, dim)
        excluded = int((~clear).sum())
        print(f"{what}: column {j + 1}: {excluded} of {len(idx)} rows excluded")
        assert excluded <= CAP * len(idx)
        assert np.array_equal(idx[clear, j], ri[clear, j])


_LIOP9 = {}


def liop_knn9(golden_dir):
    """the restatement's 9-NN of the LIOP fixture's first 512 queries, computed once per process: the first k columns ARE its k-NN"""
    if golden_dir not in _LIOP9:
        A, B, _, _ = liop_fixture(golden_dir)
        i9, d9 = knn(A, B, 9)
        i9.setflags(write=False); d9.setflags(write=False)
        _LIOP9[golden_dir] = (i9, d9)
    return _LIOP9[golden_dir]


def liop_fixture(golden_dir, n_query=512):
    """the LIOP fixture's rows as the matcher sees them: (dataset [8192, 144] f32, queries [n_query, 144] f32, ref_idx, ref_dist)"""
    import os
    z = np.load(os.path.join(golden_dir, "liop_match_ref.npz"))
    A = (z["hist0"].astype(np.float32) / z["norm0"][:, None]).astype(np.float32)
    B = (z["hist1"].astype(np.float32) / z["norm1"][:, None]).astype(np.float32)
    return A, B[:n_query], z["ref_idx"][:n_query], z["ref_dist"][:n_query]
