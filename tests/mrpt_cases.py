"""Forests and queries for tests/test_gpu_mrpt_edges.py (kernels_mrpt.hip and api_mrpt.cpp against oracle/mrpt.c, every comparison
exact) and for the CPU test that shows every case reaches its edge (tests/test_mrpt_cases.py).  Pure numpy plus the oracle.

The MRPT arm is held by ONE identity -- the GPU equals the CPU model, bit for bit -- so the cases sit where the two could part:

  self_odd         integer rows 0 .. 255, n = 129 / 255 / 257, dim 8 / 16, density 0.5; the queries are ALL dataset rows.  An odd node's
                   split IS its median row's projection, so that row meets `pq <= sp` with equality and finds its own leaf only if
                   mrpt_project_kernel (R [n_pool][dim]) and the query kernel (RT [dim][n_pool]) produce the same bits and the
                   routing says `<=`.  (1 tree, depth 6, votes 1): 129 = 65 + 64 -> 33 .. -> 3 + 2 has one odd node a level; 255 and
                   257 have more.  (3, 6, 3): a row is elected only if all three trees hold it in the query's leaf.
  ties_at_cuts     rows from {0, 1}^8 (at most 256 distinct rows among 300 / 4,097): a projection takes few values, rows of equal
                   projection lie either side of a cut (vl == vr at even nodes), their sides are decided by the row index -- the
                   model's (projection, row) against the kernel's one 64-bit key; 4,097 rows also put the ties through the
                   global-memory sort passes.
  constant_view    200 copies of one row: every projection of a level is equal, the arrangement is the row index alone; the query
                   that equals the row meets equality at every node and goes left every time; its elected rows all lie at distance 0
                   (the re-rank's (distance, row) order decides everything).
  zero_vectors     dim 4 at density 0.05: most random vectors have no entry, their levels split by the row index alone; the rows are
                   real-valued with both signs, so the dense loop adds products of either sign of zero.
  even_odd_levels  n = 128, 130, 191, 192, 193 real-valued rows: over the set every level holds odd nodes (split = the median row's
                   projection) and even nodes (split = the float sum of the two rows either side of the cut, halved); leaf sizes
                   follow n - n / 2, n / 2.
  sort_seams       n = 4,096, 4,097, 8,192, 8,193, 16,385: the sort's cap = 4,096 (LDS only), 8,192, 8,192, 16,384, 32,768 -- one,
                   two and three cross-chunk merge sizes, with one padding key short of a whole half at 4,097 / 8,193 / 16,385.
  retry_counts     600 SIFT-like rows with planted groups of 1, 2 and 3 near-identical rows and queries beside them, 26 trees:
                   votes 26 (= n_trees) elects only the rows that share the query's leaf in every tree, so the first attempt elects
                   0, 1 or (seldom: some tree nearly always cuts a group) 2 rows and the tails retry with 25 -- answered only then, or
                   dropped; votes 23 lets three trees disagree, which leaves enough queries at 1, 2 AND 3 elected rows; votes 2 never
                   needs its retry on 600 rows (ties_at_cuts and even_odd_levels retry with 1); votes 1 never retries.
  lane_counts      1 tree, votes 1: the elected rows ARE the query's leaf.  258 rows at depth 2 and 4,128 rows at depth 6 have leaves
                   of exactly 65 and 64 rows (one elected row per lane of the re-rank; the first lane with two).  Half of the rows are
                   duplicates of their neighbour, queries equal dataset rows: two elected rows at distance 0, in different lanes
                   wherever 64 rows were elected; the lower row is first.
  wide_narrow      dim 4 and dim 512 (the ends of what mrpt_dim_ok admits), 256 rows; a U8 collection through match_pairs_mrpt.
  waves_2, waves_1 14,000 and 30,000 SIFT-like rows at the preset's trees and votes 2: launch_mrpt_query halves the wavefronts of a
                   workgroup to 2 and to 1; 97 queries leave the last workgroup partial.
  unfit_view       32,000 rows at 255 trees, votes 2: no wavefront's LDS holds the vote bytes and the elected list, the view is
                   scanned.
  mixed_batch      views of 60, 128, 129, 4,097 and 14,000 rows in one call: the batch takes the carve of the largest view.

All data is finite.  A non-finite row has no place here: the model sorts projections with qsort, whose result on NaN is undefined, so
such a case would have no expected output -- that is a finding about the arm, not an edge of its kernels.
"""
import collections
import functools

import numpy as np

from test_gpu_ann_knn import mrpt_launch_lds, mrpt_model

KS = (1, 2, 3)                     # 2 is r3dm_mrpt_knn2 (the 2-NN tail), 1 and 3 r3dm_mrpt_knn (the k-list tail)
N_TREES, DEPTH = 26, 6             # the reference's preset (src/R3DComputeMatches.cpp:453-455)

KnnCase = collections.namedtuple("KnnCase", "name family data queries n_trees depth votes density seed")


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def sift_like(rng, n, dim):
    """integer-valued rows 0 .. 255 with SIFT's many small and few large bins"""
    return _f32(np.minimum(np.floor(rng.gamma(0.6, 30.0, (n, dim))), 255.0))


def beside(rng, rows, step=3):
    """rows moved by integers in [-step, step], kept in 0 .. 255"""
    return _f32(np.clip(rows + rng.integers(-step, step + 1, rows.shape), 0, 255))


def density_of(case):
    """Mrpt::grow: density <= 0 means 1 / sqrt(dim), in float (api_mrpt.cpp: mrpt_density_for)"""
    return float(case.density) if case.density > 0 else float(np.float32(1.0 / np.sqrt(np.float64(case.data.shape[1]))))


def _self_odd():
    out = []
    for n in (129, 255, 257):
        for dim in (8, 16):
            for n_trees, votes in ((1, 1), (3, 3)):
                rng = np.random.default_rng(1000 + n + dim)
                data = _f32(rng.integers(0, 256, (n, dim)))
                out.append(KnnCase(f"self_odd-n{n}-d{dim}-t{n_trees}v{votes}", "self_odd", data, data, n_trees, 6, votes, 0.5, 0))
    return out


def _ties_at_cuts():
    out = []
    for n in (300, 4097):
        rng = np.random.default_rng(2000 + n)
        data = _f32(rng.integers(0, 2, (n, 8)))
        q = np.concatenate([data[:17], _f32(rng.integers(0, 2, (48, 8)))])
        out.append(KnnCase(f"ties_at_cuts-n{n}", "ties_at_cuts", data, q, 4, 6, 2, 0.5, 0))
    return out


def _constant_view():
    row = _f32([[7, 0, 3, 200, 1, 1, 0, 19]])
    q = np.concatenate([row, _f32([[7, 0, 3, 201, 1, 1, 0, 19], [0, 0, 0, 0, 0, 0, 0, 0], [255, 9, 3, 2, 100, 1, 50, 19]])])
    return [KnnCase("constant_view", "constant_view", np.repeat(row, 200, axis=0), q, 4, 6, 2, 0.5, 0)]


def _zero_vectors():
    rng = np.random.default_rng(3000)
    data = _f32(rng.standard_normal((300, 4)))
    q = np.concatenate([data[:20], _f32(data[20:65] + 0.01 * rng.standard_normal((45, 4)))])
    return [KnnCase("zero_vectors", "zero_vectors", data, q, 6, 4, 2, 0.05, 0)]


def _even_odd_levels():
    out = []
    for n in (128, 130, 191, 192, 193):
        rng = np.random.default_rng(4000 + n)
        data = _f32(rng.standard_normal((n, 8)))
        q = np.concatenate([data[:9], _f32(data[9:33] + 0.05 * rng.standard_normal((24, 8)))])
        out.append(KnnCase(f"even_odd_levels-n{n}", "even_odd_levels", data, q, 4, 6, 2, 0.5, 3))
    return out


def _sort_seams():
    out = []
    for n in (4096, 4097, 8192, 8193, 16385):
        rng = np.random.default_rng(5000 + n)
        data = _f32(rng.standard_normal((n, 8)))
        q = _f32(data[rng.choice(n, 65, replace=False)] + 0.01 * rng.standard_normal((65, 8)))
        out.append(KnnCase(f"sort_seams-n{n}", "sort_seams", data, q, 2, 6, 1, 0.5, 5))
    return out


RETRY_GROUPS = ((1, 40), (2, 40), (3, 40))        # (rows of a planted group, groups of that size): rows 0 .. 239 of the view


def _one_step_off(rng, row, m):
    """the row with m of its members moved by one"""
    r = row.copy()
    at = rng.choice(len(r), m, replace=False)
    r[at] += np.where(r[at] > 0, rng.choice([-1.0, 1.0], m), 1.0).astype(np.float32)
    return r


def _retry_counts():
    """groups of g rows that differ from one another in one member by one; query j is group j's first row with 1 .. 4 members moved by
    one -- a sparse random vector (density 1 / sqrt(128)) rarely sees such a step, so most of these queries share a leaf with their
    group in all 26 trees, some in 25, some in fewer (240 planted rows, 120 such queries); 180 more queries lie beside unplanted rows
    at +-3 and elect nothing at votes 26"""
    rng = np.random.default_rng(6000)
    data = sift_like(rng, 600, 128)
    q = []
    row = 0
    for g, count in RETRY_GROUPS:
        for j in range(count):
            for a in range(1, g):
                data[row + a] = _one_step_off(rng, data[row], 1)
            q.append(_one_step_off(rng, data[row], 1 + j % 4)[None, :])
            row += g
    q.append(beside(rng, data[row:row + 180], 3))
    q = np.concatenate(q)
    return [KnnCase(f"retry_counts-v{votes}", "retry_counts", data, q, N_TREES, DEPTH, votes, -1.0, 0) for votes in (1, 2, 23, 26)]


def _lane_counts():
    out = []
    for n, depth in ((258, 2), (4128, 6)):
        rng = np.random.default_rng(7000 + n)
        data = _f32(rng.integers(0, 256, (n, 8)))
        dup = np.arange(0, n - 1, 4)
        data[dup + 1] = data[dup]                              # rows 4i and 4i + 1 are one row twice
        picks = np.concatenate([dup[:: max(1, len(dup) // 40)][:40], dup[:25] + 2])
        out.append(KnnCase(f"lane_counts-n{n}", "lane_counts", data, _f32(data[picks]), 1, depth, 1, 0.5, 2))
    return out


def _wide_narrow():
    out = []
    for dim in (4, 512):
        rng = np.random.default_rng(8000 + dim)
        data = _f32(rng.standard_normal((256, dim)))
        q = _f32(data[rng.choice(256, 65, replace=False)] + 0.02 * rng.standard_normal((65, dim)))
        out.append(KnnCase(f"wide_narrow-d{dim}", "wide_narrow", data, q, N_TREES, DEPTH, 3, -1.0, 0))
    return out


def _waves():
    out = []
    for waves, n in ((2, 14000), (1, 30000)):
        rng = np.random.default_rng(9000 + n)
        data = sift_like(rng, n, 128)
        q = beside(rng, data[rng.choice(n, 97, replace=False)], 3)
        out.append(KnnCase(f"waves_{waves}", f"waves_{waves}", data, q, N_TREES, DEPTH, 2, -1.0, 0))
    return out


@functools.lru_cache(maxsize=None)
def knn_cases():
    """name -> KnnCase, in the order of the table above"""
    cases = (_self_odd() + _ties_at_cuts() + _constant_view() + _zero_vectors() + _even_odd_levels() + _sort_seams() + _retry_counts()
             + _lane_counts() + _wide_narrow() + _waves())
    for c in cases:
        assert np.isfinite(c.data).all() and np.isfinite(c.queries).all()
        c.data.setflags(write=False); c.queries.setflags(write=False)
    return collections.OrderedDict((c.name, c) for c in cases)


KNN_NAMES = tuple(knn_cases())


def family(name):
    return [c for c in knn_cases().values() if c.family == name]


# ------------------------------------------------------------------------------------------------------------ the model side
@functools.lru_cache(maxsize=None)
def index_of(oracle_mod, name):
    """-> (the oracle's index, its exported arrays); computed once, never written"""
    c = knn_cases()[name]
    ix = oracle_mod.mrpt_build(c.data, c.n_trees, c.depth, density_of(c), c.seed)
    ex = ix.export()
    for a in ex.values():
        a.setflags(write=False)
    return ix, ex


@functools.lru_cache(maxsize=None)
def expected(oracle_mod, name, k, route_strict=False, rerank_high=False):
    """mrpt_model on the oracle's index -> rows, sqrtf distances, n_elected (answering attempt), class, n_elected (first attempt)"""
    c = knn_cases()[name]
    ix, ex = index_of(oracle_mod, name)
    out = mrpt_model(ex, c.data, c.queries, ix.n_trees, ix.depth, c.votes, k, route_strict=route_strict, rerank_high=rerank_high)
    for a in out:
        a.setflags(write=False)
    return out


def n_measured(case, k, ne_answering, ne_first):
    """distances the query kernel evaluates: the elected rows of the first attempt plus those of the retry, where one ran"""
    retried = (ne_first < k) & (case.votes > 1)
    return int(ne_first.astype(np.int64).sum() + ne_answering.astype(np.int64)[retried].sum())


def project(R, X):
    """mr_project for every (row, random vector): column after column in float32, the product rounded before the sum -> [n, n_pool]"""
    p = np.zeros((len(X), len(R)), np.float32)
    for c in range(X.shape[1]):
        p = p + R[None, :, c] * X[:, c, None]
    return p


def node_ranges(n, depth):
    """per level the (first position, rows) of its nodes, left to right (count_leaf_sizes: n - n / 2 to the left, n / 2 to the right)"""
    levels, cur = [], [(0, n)]
    for _ in range(depth + 1):
        levels.append(cur)
        cur = [r for lo, ln in cur for r in ((lo, ln - ln // 2), (lo + ln - ln // 2, ln // 2))]
    return levels


def cuts(ex, proj, n_trees, depth):
    """every inner node of every tree -> (tree, level, node in heap order, rows, vl, vr, median row): vl / vr the largest projection
    left and the smallest right of the cut, median row = the last row of the left side in the order (projection, row).  (A node's
    range of `leaves` holds the node's rows at every later level, so the final arrangement tells the sides.)"""
    n = proj.shape[0]
    out = []
    for t in range(n_trees):
        for level, nodes in enumerate(node_ranges(n, depth)[:depth]):
            p = proj[:, t * depth + level]
            for s, (lo, ln) in enumerate(nodes):
                nl = ln - ln // 2
                left, right = ex["leaves"][t, lo:lo + nl], ex["leaves"][t, lo + nl:lo + ln]
                median = left[np.lexsort((left, p[left]))[-1]]
                out.append((t, level, (1 << level) - 1 + s, ln, p[left].max(), p[right].min(), int(median)))
    return out


def routes(ex, pq, n_trees, depth):
    """-> nodes [nq, n_trees, depth] a query visits (heap order), equal [nq, n_trees, depth]: its projection EQUALS the split there"""
    nq = len(pq)
    nodes = np.zeros((nq, n_trees, depth), np.int64); equal = np.zeros((nq, n_trees, depth), bool)
    for t in range(n_trees):
        node = np.zeros(nq, np.int64)
        for d in range(depth):
            sp = ex["splits"][t, node]
            nodes[:, t, d] = node; equal[:, t, d] = pq[:, t * depth + d] == sp
            node = 2 * node + 1 + (~(pq[:, t * depth + d] <= sp)).astype(np.int64)
    return nodes, equal


def model_index(R, X, n_trees, depth, ties_descending=False, even_split_left=False):
    """grow_subtree as oracle/mrpt.c states it, in numpy -> splits, leaves.  ties_descending / even_split_left: two WRONG variants (equal
    projections ordered by descending row; split = vl at even nodes) for the test that shows the table would notice them"""
    n = len(X)
    proj = project(R, X)
    splits = np.zeros((n_trees, (1 << depth) - 1), np.float32); leaves = np.zeros((n_trees, n), np.int32)
    for t in range(n_trees):
        idx = np.arange(n, dtype=np.int64)
        for level, nodes in enumerate(node_ranges(n, depth)[:depth]):
            p = proj[:, t * depth + level]
            for s, (lo, ln) in enumerate(nodes):
                rows = idx[lo:lo + ln]
                rows = rows[np.lexsort((-rows if ties_descending else rows, p[rows]))]
                idx[lo:lo + ln] = rows
                nl = ln - ln // 2
                vl = p[rows[nl - 1]]
                if ln % 2 or even_split_left:
                    split = vl
                else:
                    split = np.float32(np.float64(np.float32(p[rows[nl]] + vl)) / 2.0)      # mrpt.h:1072-1073: a float sum, halved in double
                splits[t, (1 << level) - 1 + s] = split
        leaves[t] = idx
    return splits, leaves


def launch_shape(n, n_trees, depth, votes):
    """launch_mrpt_query's carve for a batch whose largest index view has n rows -> (LDS bytes of one wavefront, wavefronts of a workgroup)"""
    max_leaf = n // (1 << depth) + 1
    elected_cap = min(n, n_trees * max_leaf // max(votes - 1 if votes > 1 else 1, 1)) + 64
    pool_pad = (n_trees * depth + 63) // 64 * 64
    per_wave = (pool_pad * 4 + 256 * 4 + 8 + elected_cap * 4 + (n + 3) // 4 * 4 + 15) // 16 * 16
    waves = 4
    while waves > 1 and per_wave * waves > 150 * 1024:
        waves >>= 1
    assert per_wave * waves == mrpt_launch_lds(n, n_trees, depth, votes)
    return per_wave, waves


# ------------------------------------------------------------------------------------------------------------ collections
Collection = collections.namedtuple("Collection", "name descs xys pairs n_trees depth votes ratio")


def _views_of(rng, base, sizes, step, dtype=np.float32):
    """views that see the first rows of one base set, each moved by a few integers; distinct positions"""
    descs = [np.ascontiguousarray(beside(rng, base[:n], step), dtype) for n in sizes]
    xys = [_f32(rng.permutation(4 * n)[:n, None] * np.float32([1.0, 0.5]) + np.float32([0.25, 3.0])) for n in sizes]
    return descs, xys


def _ordered_pairs(m):
    return np.array([(i, j) for i in range(m) for j in range(m) if i != j], np.uint32)


@functools.lru_cache(maxsize=None)
def collections_():
    out = collections.OrderedDict()
    rng = np.random.default_rng(10000)
    descs, xys = _views_of(rng, sift_like(rng, 300, 64), (300, 300, 300), 6, np.uint8)
    out["wide_narrow_u8"] = Collection("wide_narrow_u8", descs, xys, _ordered_pairs(3), N_TREES, DEPTH, 5, 0.8)
    rng = np.random.default_rng(10001)
    descs, xys = _views_of(rng, sift_like(rng, 32000, 32), (32000, 200), 2)
    out["unfit_view"] = Collection("unfit_view", descs, xys, np.array([(0, 1)], np.uint32), 255, 6, 2, 0.8)
    rng = np.random.default_rng(10002)
    descs, xys = _views_of(rng, sift_like(rng, 14000, 32), (60, 128, 129, 4097, 14000), 2)
    out["mixed_batch"] = Collection("mixed_batch", descs, xys, _ordered_pairs(5), N_TREES, DEPTH, 2, 0.8)
    for c in out.values():
        for a in c.descs + c.xys:
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected_collection(oracle_mod, name):
    """oracle.match_collection_mrpt with the case's parameters -> (counts per pair, matches); unfit_view: the exhaustive arm instead"""
    c = collections_()[name]
    descs = [_f32(d) for d in c.descs]
    if name == "unfit_view":
        return oracle_mod.match_collection(descs, c.xys, c.pairs, c.ratio, True)      # ratio^2 on squared distances
    return oracle_mod.match_collection_mrpt(descs, c.xys, c.pairs, c.ratio, n_trees=c.n_trees, depth=c.depth, votes=c.votes)
