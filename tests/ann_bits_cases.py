"""Inputs and CPU models of the Hamming graph matcher's tests (test_ann_bits_cases.py, test_gpu_ann_bits.py).

A Hamming distance between two packed rows equals the squared L2 distance between the rows unpacked to 0 / 1 floats, and every partial
sum of that distance is an integer below 2^24, exact in any order.  So the float models of the graph matcher -- oracle.kgraph_build_exact,
KGraphIndex.knn2, oracle.kgraph_seeds, orc_kgraph_search, oracle.match_collection_kgraph -- run on bits(rows) ARE the restatement of the
Hamming graph matcher: same (distance, id) index order, same pool semantics.  Only the ratio rule differs: the float model squares its
ratio, binary regions take theirs unsquared, so the tests use ratios that are exact f32 squares (RATIOS).
"""
import ctypes as C
import functools

import numpy as np

from regard3d_amd import synth

# GPU dist_ratio (R, unsquared) -> ratio of the float model (which squares it): R = r * r exactly in f32
RATIOS = {0.765625: 0.875, 0.5625: 0.75}

# (n, bytes, K, kind)
INDEX_CASES = [(1500, 61, 16, "akaze"), (130, 61, 2, "akaze"), (700, 64, 8, "rand"), (400, 32, 32, "rand"), (600, 32, 20, "ties"),
               (300, 29, 12, "rand")]
# (nI, nJ, bytes, K, P, S, kind); seed 77, pair (3, 9)
KNN2_CASES = [(1500, 1200, 61, 24, 10, 10, "akaze"), (1500, 700, 61, 20, 2, 10, "akaze"), (2000, 333, 64, 16, 6, 7, "rand"),
              (700, 500, 32, 8, 33, 10, "rand"), (400, 300, 32, 32, 61, 1, "rand"), (600, 200, 32, 20, 10, 10, "ties")]
SEARCH_SEED, SEARCH_PAIR = 77, (3, 9)


def bits(rows):
    """packed rows [n, bytes] uint8 -> [n, 8 bytes] float32 of 0 / 1, LSB first (the order is irrelevant to a distance)"""
    rows = np.ascontiguousarray(rows, np.uint8)
    return np.unpackbits(rows, axis=1, bitorder="little").astype(np.float32)


@functools.lru_cache(maxsize=None)
def tie_heavy():
    """600 rows of 32 bytes with four sparse bits per byte, 300 copies of row 7 and 50 of row 8: few distinct distances, hub rows whose
    incoming edges pass the adjacency cap of 64.  200 queries: rows of A with the low bit flipped in 5 % of their bytes."""
    rng = np.random.default_rng(5)
    A = (rng.integers(0, 256, (600, 32), dtype=np.uint8) & rng.integers(0, 256, (600, 32), dtype=np.uint8) & np.uint8(0x0F))
    A[100:400] = A[7]
    A[400:450] = A[8]
    B = A[rng.integers(0, 600, 200)] ^ (rng.random((200, 32)) < 0.05).astype(np.uint8)
    return np.ascontiguousarray(A), np.ascontiguousarray(B)


@functools.lru_cache(maxsize=None)
def views(kind, nI, nJ, nbytes):
    """(dataset [nI, nbytes], queries [nJ, nbytes]) uint8"""
    if kind == "ties":
        A, B = tie_heavy()
        return A[:nI], B[:nJ]
    if kind == "akaze":
        sc = synth.make_scene(2, max(nI, nJ), "akaze", seed=nI)
        return np.ascontiguousarray(sc.descs[0][:nI, :nbytes]), np.ascontiguousarray(sc.descs[1][:nJ, :nbytes])
    rng = np.random.default_rng(nI + nJ + nbytes)
    A = rng.integers(0, 256, (nI, nbytes), dtype=np.uint8)
    flips = np.packbits(rng.random((nJ, nbytes * 8)) < 0.1, axis=1, bitorder="little")
    B = A[rng.integers(0, nI, nJ)] ^ flips
    return A, np.ascontiguousarray(B)


@functools.lru_cache(maxsize=None)
def scene():
    """five MLDB-shaped views (61-byte rows): three of 1,300 rows, one of 90 (scanned, as I and as J), one empty"""
    sc = synth.make_scene(5, 1300, "akaze", seed=31)
    descs = [np.ascontiguousarray(d[:, :61]) for d in sc.descs]
    xys = list(sc.xys)
    descs[3], xys[3] = descs[3][:90], xys[3][:90]
    descs[4], xys[4] = descs[4][:0], xys[4][:0]
    return descs, xys, sc.exhaustive_pairs()


def csr_rows(off, ids, n):
    adj = np.full((n, 64), 0xFFFFFFFF, np.uint32)
    deg = np.diff(off.astype(np.int64)).astype(np.uint32)
    for i in range(n):
        adj[i, :deg[i]] = ids[off[i]:off[i + 1]]
    return adj, deg


def kgraph_restated(oracle, g, rows_f32, queries_f32, k, P, S, seed, I, J, min_rows=128):
    """orc_kgraph_search(K = k) of every query on the start rows of orc_kgraph_seeds: (rows [nq, k], -1 padded; distances, +inf padded)"""
    L = oracle.lib()
    L.orc_kgraph_search.restype = C.c_uint32
    L.orc_kgraph_search.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32,
                                    C.c_void_p, C.c_void_p, C.c_void_p]
    idx = np.full((len(queries_f32), k), -1, np.int32); dist = np.full((len(queries_f32), k), np.inf, np.float32)
    ids = np.zeros(k + 1, np.uint32); ds = np.zeros(k + 1, np.float32)
    for r in range(len(queries_f32)):
        seeds = oracle.kgraph_seeds(seed, I, J, r, len(rows_f32), P)
        row = np.ascontiguousarray(queries_f32[r])
        n = L.orc_kgraph_search(g.h, rows_f32.ctypes.data, rows_f32.shape[1], row.ctypes.data, k, P, S, seeds.ctypes.data, min_rows,
                                ids.ctypes.data, ds.ctypes.data, None)
        idx[r, :n] = ids[:n]; dist[r, :n] = ds[:n]
    return idx, dist


def graph_dict(pairs, counts, matches):
    """(counts, matches) of a model's collection call -> {(I, J): matches} of the non-empty pairs"""
    out, off = {}, 0
    for p, (I, J) in enumerate(pairs):
        if counts[p]:
            out[(int(I), int(J))] = matches[off:off + counts[p]]
        off += counts[p]
    return out
