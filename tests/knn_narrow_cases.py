"""k-NN on the narrow tiles (r3dm_set_knn_narrow_tiles), restated in numpy: which path the host takes for a pair of views, what the
integer tiles' exact lists return and which queries the split planes' certificate lets through.

Not a test module (no test_ prefix): imported by test_knn_narrow_cases.py (CPU), test_gpu_knn_narrow.py and
test_cpp_knn_narrow_adapter.py.  The arithmetic it builds on is certificate_cases.py's and knn_restatement.py's.
"""
import functools

import numpy as np

import certificate_cases as CC
import knn_restatement as R

F32 = np.float32
TWO24 = F32(16777216.0)


def kl_of(k):
    """list depth of the kernel that serves k"""
    return 4 if k <= 4 else 8


# ------------------------------------------------------------------------------------------------ the host's routing, restated
def exact_pair(a, b, bf16):
    """api_match.cpp exact_pair: key + ||q||^2 is the reference distance bit for bit (integer values, every partial sum below 2^24),
    evaluated in f32 as the host does; bf16: the values also fit the bf16 tiles"""
    a = np.asarray(a, F32); b = np.asarray(b, F32)
    if not (np.array_equal(a, np.rint(a)) and np.array_equal(b, np.rint(b))):
        return False
    dpad = F32(CC.dpad_of(a.shape[1]))
    mI, mJ = F32(np.abs(a).max()), F32(np.abs(b).max())
    if (a < 0).any() or (b < 0).any():
        ok = dpad * (mI + mJ) * (mI + mJ) < TWO24
    else:
        ok = F32(2.0) * dpad * mI * mJ < TWO24 and dpad * mI * mI < TWO24 and dpad * mJ * mJ < TWO24
    return bool(ok) and (not bf16 or (mI <= 256 and mJ <= 256))


def expected_path(a, b, binary=False):
    """'integer' | 'split' | 'f32' | 'scan' | 'hamming': the kernel a knn(k >= 3) call runs on while the switch is on"""
    if binary:
        return "hamming"
    G = CC.kernel_G_for(a.shape[1])
    if not CC.has_tensor_kernel(G):
        return "scan"
    af = np.asarray(a, F32); bf = np.asarray(b, F32)
    if G != 18 and exact_pair(af, bf, True):
        return "integer"
    if CC.split_eligible(af, bf):
        return "split"
    return "f32"


def assert_path(stats, path, n_query, what=""):
    """the counters of the call say it ran on `path`; the four 2-NN opt-in counters never move on a k >= 3 call"""
    got = (stats.n_knn_integer_tiles, stats.n_knn_split_tiles)
    want = {"integer": (1, 0), "split": (0, 1)}.get(path, (0, 0))
    assert got == want, (what, path, got)
    assert (stats.n_integer_mfma, stats.n_split_mfma, stats.n_hamming_mfma, stats.n_counts_mfma) == (0, 0, 0, 0), what
    if path == "integer":
        assert stats.n_exact_fallback == 0, (what, stats.n_exact_fallback)          # exact lists: nothing to scan
    if path == "scan":
        assert stats.n_exact_fallback == n_query, what


# ------------------------------------------------------------------------------------------------ integer tiles
def integer_lists_knn(a, b, k):
    """what l2_knnk_int_kernel returns: exact keys ||a||^2 - 2 a.q, per lane half the lexicographic (key, row) top-KL, the two lists
    merged under (key, row), distance = key + ||q||^2.  -> (idx [nq, k], dist [nq, k] f32, rows left out of both lists that tie or
    beat the k-th: always 0, the lists are exact)"""
    KL = kl_of(k)
    a64 = np.asarray(a, np.float64); b64 = np.asarray(b, np.float64)
    keys = (a64 * a64).sum(1)[None, :] - 2.0 * (b64 @ a64.T)                 # exact: integers far below 2^53
    nb = (b64 * b64).sum(1)
    rows = np.arange(a64.shape[0])
    half = np.array([CC._lane_half(r % CC.TILE_ROWS) for r in rows])
    idx = np.zeros((b64.shape[0], k), np.int32); dist = np.zeros((b64.shape[0], k), F32)
    left_out = 0
    for q in range(b64.shape[0]):
        nominees = []
        for h in (0, 1):
            r = rows[half == h]
            nominees += r[np.lexsort((r, keys[q, r]))][:KL].tolist()
        nominees = np.array(nominees)
        o = nominees[np.lexsort((nominees, keys[q, nominees]))][:k]
        idx[q] = o
        dist[q] = (keys[q, o] + nb[q]).astype(F32)
        others = np.setdiff1d(rows, nominees)
        if others.size:
            kk, kr = keys[q, o[-1]], o[-1]
            left_out += int(((keys[q, others] < kk) | ((keys[q, others] == kk) & (others < kr))).sum())
    return idx, dist, left_out


def tie_across_halves(with_C=True):
    """test_gpu_knn.py's layout at k = 8: rows at squared distances 1 .. 7 fill half 0's list together with row A at T = 9; B (half 1)
    and C (half 0) are at T too, A < B < C.  -> (a, b, near, A, B, C)"""
    half0 = [r for r in range(32) if CC._lane_half(r) == 0]
    half1 = [r for r in range(32) if CC._lane_half(r) == 1]
    rng = np.random.default_rng(8)
    a = rng.integers(100, 156, (107, 128)).astype(F32)
    b = rng.integers(100, 156, (9, 128)).astype(F32)
    near = [32 + r for r in half0[:7]]
    A, B, C = 32 + half0[7], 32 + half1[7], 64 + half0[0]
    assert A < B < C
    for i, r in enumerate(near):
        a[r] = b[0]; a[r, :i + 1] += 1.0
    for r in (A, B, C):
        a[r] = b[0]; a[r, r % 64] += 3.0
    if not with_C:
        a[C] = a[0]
    return a, b, near, A, B, C


def u8_tied(nI, nJ, dim, top=256, seed=0):
    """u8 rows as test_gpu_knn.py's _shape_data builds them: distance-0 neighbours and duplicated rows"""
    rng = np.random.default_rng([dim, nI, top, seed])
    a = rng.integers(0, top, (nI, dim)).astype(np.uint8); b = rng.integers(0, top, (nJ, dim)).astype(np.uint8)
    b[:nJ // 4] = a[:nJ // 4]
    a[5] = a[4]; a[nI - 1] = a[4]
    return a, b


# ------------------------------------------------------------------------------------------------ split planes
# (case, smallest share of queries the certificate must send to the exact scan, largest): conditions, not measurements -- the caps on
# the easy cases keep a kernel from passing by scanning everything
SPLIT_CASES = (("offset_split_d128_t0", 0.0, 0.02), ("offset_split_d128_t15", None, None), ("offset_split_d128_t1000", 0.95, 1.0),
               ("offset_split_d144_t0", 0.0, 0.02), ("offset_split_d144_t300", 0.95, 1.0),
               ("mixed_large_last_split", 0.95, 1.0), ("mixed_large_row0_split", 0.95, 1.0))


def split_certificate(a, b, k):
    """what l2_knnk_split_kernel + knnk_finish decide: K-lists per lane half over the emulated split-f16 keys (bound = the smaller
    (KL + 1)-th key), nominees re-scored in the reference arithmetic, certified iff e_k < (bound + ||q||^2) - slack with the split
    planes' slack.  -> (answers [(idx, dist)] per query, certified [nq] bool)"""
    KL = kl_of(k)
    keys = CC.emulated_keys(a, b, "split16")                  # in the views' own units: key x key_inv
    dist = CC.ref_distances(a, b)
    nb = CC.norms_f32(b)
    slack = CC.case_slack("split", a, b)
    half = np.array([CC._lane_half(r % CC.TILE_ROWS) for r in range(a.shape[0])])
    answers, certified = [], np.zeros(b.shape[0], bool)
    for q in range(b.shape[0]):
        nominees, bound = [], F32(np.inf)
        for h in (0, 1):
            rows = np.flatnonzero(half == h)
            o = rows[np.argsort(keys[q, rows], kind="stable")]
            nominees += o[:KL].tolist()
            if len(o) > KL:
                bound = min(bound, keys[q, o[KL]])
        nominees = np.array(nominees)
        e = dist[q, nominees]
        o = np.lexsort((nominees, e))[:k]
        answers.append((nominees[o], e[o]))
        certified[q] = e[o][-1] < F32(F32(bound + nb[q]) - slack[q])
    return answers, certified


@functools.lru_cache(maxsize=None)
def case_views(name):
    """(dataset, query, the restatement's 8-NN) of a certificate case: made once per process, read-only"""
    a, b = CC.CASES[name].make()
    ref = R.knn(a, b, 8)
    for x in (a, b) + ref:
        x.setflags(write=False)
    return a, b, ref
