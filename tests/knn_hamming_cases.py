"""Hamming k-NN on the i8 MFMA tiles (r3dm_set_knn_hamming_tiles; kernels_match_knn8.hip), restated in numpy: the keys the tiles
compute, the per-lane-half K-lists and their merge, and the data sets of tests/test_gpu_knn_hamming_tiles.py with their preconditions.

Not a test module (no test_ prefix): imported by test_knn_hamming_cases.py (CPU) and test_gpu_knn_hamming_tiles.py.  Every data set is
made once per process and read-only; the restatement of a data set (knn_restatement.knn at k = 8, or as deep as it has rows) likewise.
"""
import functools

import numpy as np

import certificate_cases as CC
import knn_restatement as R

HAM_BIAS = 0x3F800000           # kHamBias: the bits of 1.0f
PAD_KEY = 0x7F000000            # the biased "popcount" stage_bin8_kernel gives a padding row
KS = (3, 4, 5, 8)
TILE_ROWS_N = (3, 8, 9, 31, 32, 33, 64, 65, 97, 129, 225, 257)        # 1 .. 9 tiles, odd and even tails
QUERY_COUNTS = (1, 33, 129, 257)
BYTE_LENGTHS = (29, 32, 61, 64)


def kl_of(k):
    """list depth of the kernel that serves k (dispatch_kl)"""
    return 4 if k <= 4 else 8


def words_of(nbytes):
    return (nbytes + 3) // 4


def n_tiles(n):
    return (n + CC.TILE_ROWS - 1) // CC.TILE_ROWS


def half_of_rows(n):
    return np.array([CC._lane_half(r % CC.TILE_ROWS) for r in range(n)])


def _frozen(*arrays):
    for x in arrays:
        x.setflags(write=False)
    return arrays


def _ref(a, b):
    """the restatement as deep as the tests read it: 8 columns, or every row of a smaller data set"""
    return _frozen(*R.knn(a, b, min(8, a.shape[0]), binary=True))


# ------------------------------------------------------------------------------------------------ keys and lists
def biased_key_floats(keys):
    """integer keys -> the floats whose bits are key + kHamBias (what the accumulators hold, read as the list code reads them)"""
    return (np.asarray(keys, np.int64) + HAM_BIAS).astype(np.uint32).view(np.float32)


def keys_of(a, b):
    """[nq, n_pad] int64: popcount(a) - 2 a.q of every row, PAD_KEY - kHamBias for the padding rows of the last tile"""
    bits_a = np.unpackbits(np.ascontiguousarray(a, np.uint8), axis=1).astype(np.int64)
    bits_b = np.unpackbits(np.ascontiguousarray(b, np.uint8), axis=1).astype(np.int64)
    keys = bits_a.sum(1)[None, :] - 2 * (bits_b @ bits_a.T)
    n_pad = n_tiles(a.shape[0]) * CC.TILE_ROWS
    pad = np.full((b.shape[0], n_pad - a.shape[0]), PAD_KEY - HAM_BIAS, np.int64)
    return np.concatenate([keys, pad], 1), bits_b.sum(1)


def half_lists_knn(a, b, k):
    """what hamming_knnk_mfma_kernel returns: per lane half the lexicographic (key, row) top-KL of its rows -- padding rows included,
    as the kernel sees them -- the two lists merged under (key, row), the first k, distance = key + popcount(q) as float.
    -> (idx [nq, k] int32, dist [nq, k] float32)"""
    KL = kl_of(k)
    keys, pq = keys_of(a, b)
    rows = np.arange(keys.shape[1])
    half = half_of_rows(keys.shape[1])
    idx = np.zeros((b.shape[0], k), np.int32); dist = np.zeros((b.shape[0], k), np.float32)
    for q in range(b.shape[0]):
        nominees = []
        for h in (0, 1):
            r = rows[half == h]
            nominees += r[np.lexsort((r, keys[q, r]))][:KL].tolist()
        nominees = np.array(nominees)
        o = nominees[np.lexsort((nominees, keys[q, nominees]))][:k]
        idx[q] = o
        dist[q] = (keys[q, o] + pq[q]).astype(np.float32)
    return idx, dist


# ------------------------------------------------------------------------------------------------ data sets
@functools.lru_cache(maxsize=None)
def random_rows(n, nq, nbytes):
    """(dataset [n, nbytes] u8, queries [nq, nbytes] u8, restatement): plain random rows"""
    rng = np.random.default_rng([n, nq, nbytes])
    a = rng.integers(0, 256, (n, nbytes), dtype=np.uint8); b = rng.integers(0, 256, (nq, nbytes), dtype=np.uint8)
    return _frozen(a, b) + (_ref(a, b),)


def _flip(row, bits):
    out = row.copy()
    for bit in bits:
        out[bit >> 3] ^= np.uint8(1 << (bit & 7))
    return out


@functools.lru_cache(maxsize=None)
def dense_ties(nbytes):
    """289 x 161 random rows, the first 40 queries 5 %-flipped copies of the first 40 rows, row 7 repeated in rows 200 .. 204 and 288:
    distances of random rows concentrate (sigma = sqrt(2 nbytes)), so the k-th and the (k + 1)-th neighbour of many queries tie, half of
    those ties across the lane halves"""
    rng = np.random.default_rng([2026, nbytes])
    a = rng.integers(0, 256, (289, nbytes), dtype=np.uint8); b = rng.integers(0, 256, (161, nbytes), dtype=np.uint8)
    flips = np.packbits(rng.random((40, nbytes * 8)) < 0.05, axis=1)
    b[:40] = a[:40] ^ flips
    a[200:205] = a[7]; a[288] = a[7]
    return _frozen(a, b) + (_ref(a, b),)


def ties_across_halves(a, b, k):
    """how many queries have their k-th and (k + 1)-th neighbour at one distance in DIFFERENT lane halves"""
    ri, rd = R.knn(a, b, k + 1, binary=True)
    half = half_of_rows(a.shape[0])
    return int(((rd[:, k - 1] == rd[:, k]) & (half[ri[:, k - 1]] != half[ri[:, k]])).sum())


@functools.lru_cache(maxsize=None)
def all_identical(nbytes):
    """70 copies of one row; three queries equal to it, six random ones: every query's answer is rows 0 .. k - 1"""
    rng = np.random.default_rng([70, nbytes])
    row = rng.integers(0, 256, nbytes, dtype=np.uint8)
    a = np.tile(row, (70, 1))
    b = np.concatenate([np.tile(row, (3, 1)), rng.integers(0, 256, (6, nbytes), dtype=np.uint8)])
    return _frozen(a, b) + (_ref(a, b),)


DUP_ROWS = (3, 5, 40, 44, 45, 66, 70, 75, 90, 95)          # both lane halves of tiles 0, 1 and 2


@functools.lru_cache(maxsize=None)
def duplicated_rows(nbytes):
    """random rows with row 3 copied into DUP_ROWS; query 0 is that row: its 8-NN are the first eight of DUP_ROWS at distance 0"""
    rng = np.random.default_rng([96, nbytes])
    a = rng.integers(0, 256, (101, nbytes), dtype=np.uint8)
    for r in DUP_ROWS:
        a[r] = a[3]
    b = np.concatenate([a[3:4], rng.integers(0, 256, (20, nbytes), dtype=np.uint8)])
    return _frozen(a, b) + (_ref(a, b),)


@functools.lru_cache(maxsize=None)
def tie_across_halves(nbytes):
    """knn_narrow_cases.tie_across_halves in Hamming distances, k = 8: rows at distances 1 .. 7 and row A at 9 fill the list of lane
    half 0 of tile 1; B (half 1, same tile) and C (half 0, next tile) are at 9 too, A < B < C.  -> (a, b, restatement, near, A, B, C)"""
    half0 = [r for r in range(32) if CC._lane_half(r) == 0]
    half1 = [r for r in range(32) if CC._lane_half(r) == 1]
    rng = np.random.default_rng([8, nbytes])
    a = rng.integers(0, 256, (107, nbytes), dtype=np.uint8); b = rng.integers(0, 256, (9, nbytes), dtype=np.uint8)
    near = [32 + r for r in half0[:7]]
    A, B, C = 32 + half0[7], 32 + half1[7], 64 + half0[0]
    for i, r in enumerate(near):
        a[r] = _flip(b[0], range(i + 1))
    for r in (A, B, C):
        a[r] = _flip(b[0], range(r, r + 9))                # nine bits from bit r on: three different rows at distance 9
    return _frozen(a, b) + (_ref(a, b), near, A, B, C)


def gpu_datasets():
    """(name, dataset, queries, restatement) of every data set tests/test_gpu_knn_hamming_tiles.py runs"""
    out = []
    for nbytes in (32, 61):
        for n in TILE_ROWS_N + (1,):
            out.append((f"tiles n={n} B={nbytes}",) + random_rows(n, 40, nbytes))
    for nq in QUERY_COUNTS:
        out.append((f"queries nq={nq}",) + random_rows(101, nq, 61))
    for nbytes in BYTE_LENGTHS:
        out.append((f"bytes B={nbytes}",) + random_rows(300, 90, nbytes))
    for nbytes in (32, 61, 64):
        out.append((f"dense ties B={nbytes}",) + dense_ties(nbytes))
        out.append((f"identical B={nbytes}",) + all_identical(nbytes))
        out.append((f"duplicated B={nbytes}",) + duplicated_rows(nbytes))
        out.append((f"tie across halves B={nbytes}",) + tie_across_halves(nbytes)[:3])
    out.append(("index",) + random_rows(613, 307, 61))
    return out
