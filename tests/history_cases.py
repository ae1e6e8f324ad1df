"""The case table of the history tests (tests/test_gpu_history.py, tests/test_history_cases.py).

The property under test: every public operation returns the same bytes whatever the context did before it.  A case is one public
operation with

  make(variant)         its inputs from a fixed seed ("large" / "small": opposite sides of a branch the code takes -- which branch
                        is written next to every case and proved from the oracle alone by tests/test_history_cases.py);
  run(ctx, inputs)      the call on `ctx` -> dict of arrays (data only: no timings, no history-dependent counters);
  expect(oracle, inp)   the same dict, or the part of it a CPU restatement gives bit for bit.  Keys of run() that expect() does not
                        return have no bit-comparable restatement (the case says why); their expected value is the same call on a
                        fresh context in a child process (`python tests/history_cases.py OUT.npz CASE VARIANT [SWITCH ...]`).

Switches (set_integer_mfma, set_split_mfma, set_hamming_mfma, set_device_graphs, set_guided_matching,
set_deferred_feature_files) are applied by apply_switches() before every run; a case lists the ones its operation reads.  Only
"guided" changes what is expected; the others select another path to the same bytes.
"""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from regard3d_amd import synth  # noqa: E402

SWITCHES = ("integer_mfma", "split_mfma", "hamming_mfma", "device_graphs", "guided", "deferred")
GUIDED_RATIOS = {"F": 0.6, "E": 0.6, "H": -1.0}
VARIANTS = ("large", "small")


def apply_switches(ctx, on):
    """every switch to a known state: the ones in `on` on, the others off"""
    ctx.set_integer_mfma("integer_mfma" in on)
    ctx.set_split_mfma("split_mfma" in on)
    ctx.set_hamming_mfma("hamming_mfma" in on)
    ctx.set_device_graphs("device_graphs" in on)
    ctx.set_guided_matching("guided" in on, GUIDED_RATIOS["F"], GUIDED_RATIOS["E"], GUIDED_RATIOS["H"])
    ctx.set_deferred_feature_files("deferred" in on)


class Case:
    def __init__(self, name, make, run, expect, switches=(), branch="", fresh=""):
        self.name, self._make, self._run, self._expect = name, make, run, expect
        self.switches = tuple(switches)
        self.branch = branch          # what separates "large" from "small"
        self.fresh = fresh            # why some keys are compared with a fresh context instead of a restatement ("" = none are)

    def make(self, variant):
        return _inputs(self.name, variant)

    def run(self, ctx, inputs, on=frozenset()):
        apply_switches(ctx, on)
        out = self._run(ctx, inputs, frozenset(on))
        return {k: np.ascontiguousarray(v) for k, v in out.items()}

    def expect(self, oracle, inputs, on=frozenset()):
        return {k: np.ascontiguousarray(v) for k, v in self._expect(oracle, inputs, frozenset(on)).items()}

    def expect_key(self, variant, on):
        """what the expected value depends on: only the guided switch changes results"""
        return (self.name, variant, "guided" in on and "guided" in self.switches)


CASES = {}


@functools.lru_cache(maxsize=None)
def _inputs(name, variant):
    return CASES[name]._make(variant)


def _case(name, switches=(), branch="", fresh=""):
    def deco(cls):
        CASES[name] = Case(name, cls.make, cls.run, cls.expect, switches, branch, fresh)
        return cls
    return deco


def _oracle():
    from oracle import pyoracle
    pyoracle.build()
    return pyoracle


def _graph(g):
    return dict(pairs=np.array(g.pairs), offsets=np.array(g.offsets).astype(np.uint64), matches=np.array(g.matches))


def _expected_graph(pairs, counts, matches):
    keep = counts > 0
    return dict(pairs=np.asarray(pairs, np.uint32).reshape(-1, 2)[keep],
                offsets=np.r_[0, np.cumsum(counts[keep].astype(np.int64))].astype(np.uint64),
                matches=np.asarray(matches, np.uint32).reshape(-1, 2))


def sorted_within(offsets, matches):
    """the rows of every pair in (i, j) order: the form in which an inlier SET is compared"""
    out = np.array(matches, np.uint32).reshape(-1, 2).copy()
    o = np.asarray(offsets).astype(np.int64)
    for a, b in zip(o[:-1], o[1:]):
        m = out[a:b]
        out[a:b] = m[np.lexsort((m[:, 1], m[:, 0]))]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# knn2: f32 integer-valued (integer MFMA path), f32 real-valued (split-f16 path), u8, binary (Hamming MFMA path)
# large: hundreds of 32-row tiles with a partial last tile on both sides; small: fewer rows than the large call's LAST tile offset,
# so every buffer the small call touches (rows, tiles, norms, nominations, d_nn) still holds the large call's values behind it.
# ---------------------------------------------------------------------------------------------------------------------------------
_KNN_SIZES = {"large": (2500, 2003), "small": (70, 45)}


def _knn_data(kind, variant):
    nI, nJ = _KNN_SIZES[variant]
    rng = np.random.default_rng([hash_name(kind), nI])
    if kind == "int":
        a = np.rint(np.clip(rng.gamma(0.5, 60.0, (nI, 128)), 0, 255)).astype(np.float32)
        b = np.rint(np.clip(rng.gamma(0.5, 60.0, (nJ, 128)), 0, 255)).astype(np.float32)
        k = nJ // 2
        b[:k] = np.clip(a[:k] + np.rint(rng.normal(0, 4, (k, 128))), 0, 255)
    elif kind == "real":
        a = rng.gamma(0.5, 1.0, (nI, 144)).astype(np.float32); a /= np.linalg.norm(a, axis=1, keepdims=True)
        b = rng.gamma(0.5, 1.0, (nJ, 144)).astype(np.float32); b /= np.linalg.norm(b, axis=1, keepdims=True)
        b[:20] = a[:20] + rng.normal(0, 0.01, (20, 144)).astype(np.float32)
    elif kind == "u8":
        a = rng.integers(0, 256, (nI, 128), dtype=np.uint8); b = rng.integers(0, 256, (nJ, 128), dtype=np.uint8)
        b[:nJ // 2] = a[:nJ // 2] ^ (rng.random((nJ // 2, 128)) < 0.1).astype(np.uint8)
    else:
        a = rng.integers(0, 256, (nI, 64), dtype=np.uint8); b = rng.integers(0, 256, (nJ, 64), dtype=np.uint8)
        b[:nJ // 2] = a[:nJ // 2] ^ (rng.random((nJ // 2, 64)) < 0.05).astype(np.uint8)
    return dict(dataset=a, query=b, binary=kind == "bin")


def hash_name(s):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(s))


def _knn_case(kind, switches):
    class K:
        @staticmethod
        def make(variant):
            return _knn_data(kind, variant)

        @staticmethod
        def run(ctx, inp, on):
            idx, dist = ctx.knn2(inp["dataset"], inp["query"], binary=inp["binary"])
            return dict(idx=idx, dist=dist)

        @staticmethod
        def expect(oracle, inp, on):
            idx, dist = oracle.knn2(inp["dataset"], inp["query"], binary=inp["binary"])
            return dict(idx=idx.astype(np.int32), dist=dist.astype(np.float32))
    _case("knn2_" + kind, switches, branch="rows: 2500 x 2003 (79 / 63 tiles, partial last tile) against 70 x 45 (3 / 2 tiles)")(K)


_knn_case("int", ("integer_mfma",))
_knn_case("real", ("split_mfma",))
_knn_case("u8", ("integer_mfma",))
_knn_case("bin", ("hamming_mfma",))


# ---------------------------------------------------------------------------------------------------------------------------------
# registration + the exhaustive matcher: set_image / set_images / clear_images followed by match_pairs
# ---------------------------------------------------------------------------------------------------------------------------------
_MATCH_SIZES = {"large": (4, 1500), "small": (3, 200)}
# (rows of a registered view, rows of the view that replaces it): 0.8 - 0.95 of its size.  A replaced view keeps its slot and its
# DevBufs, and DevBuf::ensure returns at once when bytes <= cap, so the smaller view lands in the same block and the old view's last
# tiles stay behind it.  (The arena's own reuse window -- a freed block taken by ANOTHER view of 0.8 - 1.0 its size -- is not
# constructed by these tests.)
SHRINK_ROWS = [(1000, 900), (2048, 1700), (640, 530)]


def _match_case(name, kind, how, switches):
    binary = kind == "akaze"
    ratio, squared = (0.8, False) if binary else (0.6, True)

    class M:
        @staticmethod
        def make(variant):
            n_img, n_feat = _MATCH_SIZES[variant]
            sc = synth.make_scene(n_img, n_feat, kind, seed=3000 + hash_name(name) + n_feat)
            return dict(descs=sc.descs, xys=sc.xys, pairs=sc.exhaustive_pairs(), w=int(sc.widths[0]), h=int(sc.heights[0]))

        @staticmethod
        def run(ctx, inp, on):
            ctx.clear_images()
            ids = list(range(len(inp["descs"])))
            if how == "set_image":
                for i in ids:
                    ctx.set_image(i, inp["descs"][i], inp["xys"][i], inp["w"], inp["h"], binary=binary)
            else:
                ctx.set_images(ids, inp["descs"], inp["xys"], inp["w"], inp["h"], binary=binary, wait=how == "set_images_wait")
            return _graph(ctx.match_pairs(inp["pairs"], ratio, squared))

        @staticmethod
        def expect(oracle, inp, on):
            counts, matches = oracle.match_collection(inp["descs"], inp["xys"], inp["pairs"], ratio, squared, binary=binary)
            return _expected_graph(inp["pairs"], counts, matches)
    _case(name, switches, branch="4 views x 1500 rows against 3 views x 200 rows: the small views fit inside one arena block of a large view")(M)


_match_case("match_sift", "sift", "set_image", ("integer_mfma", "device_graphs"))
_match_case("match_liop", "liop", "set_images_wait", ("split_mfma", "device_graphs"))
_match_case("match_akaze", "akaze", "set_images", ("hamming_mfma", "device_graphs"))


# ---------------------------------------------------------------------------------------------------------------------------------
# the ANN arms: every view of "large" has more than the 128-row minimum (an index is built and searched), every view of "small"
# fewer (the arm scans it exactly) -- oracle/kgraph.c, hnsw.c, mrpt.c model the arms bit for bit, min_rows = 128 included
# ---------------------------------------------------------------------------------------------------------------------------------
ANN_MIN_ROWS = 128
# the arms' parameter presets as plain numbers, so that the expected values need no built library (tests/test_gpu_history.py checks
# them against r3dm_kgraph_preset / r3dm_hnsw_preset / r3dm_mrpt_preset on the GPU machine)
KGRAPH_DEFAULT = dict(index_K=24, search_P=10, search_S=10, seed=1998)
HNSW_FAST = dict(M=5, ef_construction=112, ef=5, seed=100)
HNSW_MEDIUM = dict(M=15, ef_construction=112, ef=10, seed=100)
MRPT_PRESET = dict(n_trees=26, depth=6, votes=5, density=-1.0, seed=0)
_ANN_SIZES = {"large": (3, 600), "small": (3, 100)}


def _ann_inputs(name, variant):
    n_img, n_feat = _ANN_SIZES[variant]
    sc = synth.make_scene(n_img, n_feat, "sift", seed=4000 + hash_name(name) + n_feat)
    return dict(descs=[d.astype(np.float32) for d in sc.descs], xys=sc.xys, pairs=sc.exhaustive_pairs())


def _ann_register(ctx, inp):
    ctx.clear_images()
    for v, (d, xy) in enumerate(zip(inp["descs"], inp["xys"])):
        ctx.set_image(v, d, xy, 4000, 3000)


_ANN_BRANCH = "views of 600 rows (indexed) against views of 100 rows (below the 128-row minimum: scanned exactly)"


@_case("match_kgraph", ("device_graphs",), branch=_ANN_BRANCH)
class _KGraph:
    make = staticmethod(lambda variant: _ann_inputs("match_kgraph", variant))

    @staticmethod
    def run(ctx, inp, on):
        from regard3d_amd import api
        _ann_register(ctx, inp)
        return _graph(ctx.match_pairs_kgraph(inp["pairs"], 0.6, api.KGraphParams.preset("default")))

    @staticmethod
    def expect(oracle, inp, on):
        kp = KGRAPH_DEFAULT
        c, m, _ = oracle.match_collection_kgraph(inp["descs"], inp["xys"], inp["pairs"], 0.6, builder="exact", K=kp["index_K"], P=kp["search_P"],
                                                 S=kp["search_S"], seed=kp["seed"], min_rows=ANN_MIN_ROWS)
        return _expected_graph(inp["pairs"], c, m)


@_case("match_hnsw", ("device_graphs",), branch=_ANN_BRANCH)
class _Hnsw:
    make = staticmethod(lambda variant: _ann_inputs("match_hnsw", variant))

    @staticmethod
    def run(ctx, inp, on):
        from regard3d_amd import api
        _ann_register(ctx, inp)
        return _graph(ctx.match_pairs_hnsw(inp["pairs"], 0.8, api.HnswParams.preset("fast")))

    @staticmethod
    def expect(oracle, inp, on):
        c, m = oracle.match_collection_hnsw(inp["descs"], inp["xys"], inp["pairs"], 0.8, "fast")
        return _expected_graph(inp["pairs"], c, m)


@_case("match_mrpt", ("device_graphs",), branch=_ANN_BRANCH)
class _Mrpt:
    make = staticmethod(lambda variant: _ann_inputs("match_mrpt", variant))

    @staticmethod
    def run(ctx, inp, on):
        from regard3d_amd import api
        _ann_register(ctx, inp)
        return _graph(ctx.match_pairs_mrpt(inp["pairs"], 0.8, api.MrptParams.preset()))

    @staticmethod
    def expect(oracle, inp, on):
        c, m = oracle.match_collection_mrpt(inp["descs"], inp["xys"], inp["pairs"], 0.8)
        return _expected_graph(inp["pairs"], c, m)


# the two array-matcher entries refuse fewer than 128 rows, so "small" is about the smallest dataset they serve: 130 rows, two rows per
# MRPT leaf (64 leaves at the preset's depth 6) and an almost empty upper HNSW layer, against 3000 rows, 47 per leaf
_ANN_KNN_SIZES = {"large": (3000, 800), "small": (130, 37)}


def _ann_knn_inputs(name, variant):
    n, nq = _ANN_KNN_SIZES[variant]
    sc = synth.make_scene(2, n, "sift", seed=4500 + hash_name(name) + n)
    return dict(dataset=sc.descs[0].astype(np.float32), query=sc.descs[1][:nq].astype(np.float32))


@_case("mrpt_knn2", branch="3000 rows (47 per leaf) against 130 rows (2 per leaf, just above the 128-row refusal)")
class _MrptKnn:
    make = staticmethod(lambda variant: _ann_knn_inputs("mrpt_knn2", variant))

    @staticmethod
    def run(ctx, inp, on):
        from regard3d_amd import api
        idx, dist = ctx.mrpt_knn2(inp["dataset"], inp["query"], api.MrptParams.preset())
        return dict(idx=idx, dist=dist)

    @staticmethod
    def expect(oracle, inp, on):
        mp = MRPT_PRESET
        d0 = inp["dataset"]
        ix = oracle.mrpt_build(d0, mp["n_trees"], mp["depth"], float(np.float32(1.0 / np.sqrt(np.float64(d0.shape[1])))), mp["seed"])
        idx, dist, _ = ix.knn2(inp["query"], mp["votes"])
        return dict(idx=idx.astype(np.int32), dist=dist.astype(np.float32))


@_case("hnsw_knn2", branch="3000 rows (several upper layers) against 130 rows")
class _HnswKnn:
    make = staticmethod(lambda variant: _ann_knn_inputs("hnsw_knn2", variant))

    @staticmethod
    def run(ctx, inp, on):
        from regard3d_amd import api
        idx, dist = ctx.hnsw_knn2(inp["dataset"], inp["query"], api.HnswParams.preset("medium"))
        return dict(idx=idx, dist=dist)

    @staticmethod
    def expect(oracle, inp, on):
        idx, dist = oracle.hnsw_build_batch(inp["dataset"], HNSW_MEDIUM["M"]).knn2(inp["query"], HNSW_MEDIUM["ef"])
        return dict(idx=idx.astype(np.int32), dist=dist.astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------------------------
# the geometric filters.  The putative graph is the oracle's (match_collection: bit-equal to the GPU matcher's), so a filter case
# depends on no other GPU operation.
# large: ONE pair of two 9500-row views with 9025 putatives, more than R3DM_FILTER_COOP_MIN = 4096 -> the cooperative kernel (the
#        pair spread over a pool of workgroups, slice histograms, spill lists in f_coop, coop_sched); guided: 38 query blocks of 256,
#        two J tiles of 8192 positions.  (With the product's coop_min = 4096 a pair above 4096 putatives is always cooperative, so
#        the wide 512-thread one-workgroup kernel and its m_cap of 8192 are not reachable from these entries and are not covered.)
# small: six pairs of 800-row views, every one below 4096 putatives -> the 256-thread kernel, no cooperative work, one J tile.
# Restatement: AC-RANSAC's inlier SETS equal the oracle's; their order (ascending residual, ties) and the models' last bits are the
# device's own, and so are the report rows -> those keys are compared with a fresh context.  With the guided switch on the whole
# graph is restated (tests/guided_restatement.py); on the large pair that restatement would take minutes of interpreted Python
# (millions of candidate distances), so there the fresh context is the expected value.
# ---------------------------------------------------------------------------------------------------------------------------------
def _two_view_scene(rng, n, dim, frac_match):
    """n features per view; the first frac_match * n of view 1 are noisy copies of view-0 rows, seen by a second camera"""
    A = np.rint(rng.uniform(0, 255, (n, dim))).astype(np.float32)
    nm = int(frac_match * n)
    B = np.rint(rng.uniform(0, 255, (n, dim))).astype(np.float32)
    src = rng.permutation(n)[:nm]
    B[:nm] = np.clip(A[src] + np.rint(rng.normal(0, 2, (nm, dim))), 0, 255)
    X = np.c_[rng.uniform(-4, 4, n), rng.uniform(-3, 3, n), rng.uniform(8, 14, n)]
    f = 4800.0
    xyA = np.c_[f * X[:, 0] / X[:, 2] + 2000, f * X[:, 1] / X[:, 2] + 1500]
    th = 0.05
    R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
    Y = X @ R.T + np.array([0.8, 0.05, 0.1])
    xyB_all = np.c_[f * Y[:, 0] / Y[:, 2] + 2000, f * Y[:, 1] / Y[:, 2] + 1500] + rng.normal(0, 0.4, (n, 2))
    xyB = np.c_[rng.uniform(0, 4000, n), rng.uniform(0, 3000, n)]
    xyB[:nm] = xyB_all[src]
    perm = rng.permutation(n)
    return A, xyA.astype(np.float32), B[perm], xyB[perm].astype(np.float32)


@functools.lru_cache(maxsize=None)
def filter_inputs(variant):
    O = _oracle()
    if variant == "large":
        A, xyA, B, xyB = _two_view_scene(np.random.default_rng(9505), 9500, 16, 0.95)
        descs, xys = [A, B], [xyA, xyB]
        K = np.array([[4800.0, 0, 2000], [0, 4800.0, 1500], [0, 0, 1]])
    else:
        sc = synth.make_scene(4, 800, "sift", seed=5151)
        descs, xys = sc.descs, sc.xys
        K = synth.intrinsics()
    n = len(descs)
    i, j = np.triu_indices(n, k=1)
    pairs = np.stack([i, j], axis=1).astype(np.uint32)
    counts, matches = O.match_collection(descs, xys, pairs, 0.6, True)
    keep = counts > 0
    return dict(descs=descs, xys=xys, K=K, W=[4000] * n, H=[3000] * n, pairs=pairs[keep], counts=counts[keep].astype(np.uint32),
                offsets=np.r_[0, np.cumsum(counts[keep].astype(np.int64))].astype(np.uint64), matches=matches)


def _filter_register(ctx, inp):
    from regard3d_amd import api
    ctx.clear_images()
    for v, (d, xy) in enumerate(zip(inp["descs"], inp["xys"])):
        ctx.set_image(v, d, xy, 4000, 3000)
        ctx.set_intrinsics(v, inp["K"])
    return api.Graph.from_csr(inp["pairs"], inp["offsets"], inp["matches"])


def _filter_out(kind, g, models=None, report=None):
    d = {kind + "_" + k: v for k, v in _graph(g).items()}
    d[kind + "_inliers"] = sorted_within(d[kind + "_offsets"], d[kind + "_matches"])
    if models is not None:
        d[kind + "_models"] = np.asarray(models, np.float64)
    if report is not None:
        d[kind + "_report"] = np.array(report, np.float64).reshape(-1, 5)
    return d


def _filter_expect(oracle, inp, kind, on):
    if "guided" in on:
        if inp["descs"][0].shape[0] > 4000:
            return {}                                          # (see the header of this section)
        import guided_restatement as G
        p, o, m, _ = G.guided_filter(kind, inp["descs"], inp["xys"], inp["W"], inp["H"], inp["pairs"], inp["offsets"], inp["matches"],
                                     GUIDED_RATIOS[kind], Ks=[inp["K"]] * len(inp["descs"]))
        return {kind + "_pairs": p, kind + "_offsets": o, kind + "_matches": m, kind + "_inliers": sorted_within(o, m)}
    args = (inp["xys"], inp["W"], inp["H"])
    if kind == "F":
        oc, om = oracle.filter_F_collection(*args, inp["pairs"], inp["counts"], inp["matches"], 4.0, 2048, 5489)
    elif kind == "H":
        oc, om = oracle.filter_H_collection(*args, inp["pairs"], inp["counts"], inp["matches"], 4.0, 2048, 5489)
    else:
        oc, om = oracle.filter_E_collection(*args, np.stack([inp["K"]] * len(inp["descs"])), inp["pairs"], inp["counts"], inp["matches"],
                                            4.0, 2048, 5489, prune_min_count=50, prune_min_ratio=0.3)
    e = _expected_graph(inp["pairs"], oc, om)
    return {kind + "_pairs": e["pairs"], kind + "_offsets": e["offsets"], kind + "_inliers": sorted_within(e["offsets"], e["matches"])}


_FILTER_BRANCH = "one pair of 9025 putatives (above R3DM_FILTER_COOP_MIN: cooperative kernel, spill lists) against pairs below 4096 (one 256-thread workgroup each)"
_FILTER_FRESH = "inlier order, model bits and report rows have no bit-equal restatement; the guided large pair is too slow to restate"


def _filter_case(kind):
    class F:
        make = staticmethod(filter_inputs)

        @staticmethod
        def run(ctx, inp, on):
            put = _filter_register(ctx, inp)
            fn = {"F": ctx.filter_F, "E": ctx.filter_E, "H": ctx.filter_H}[kind]
            g, M = fn(put, **{"want_" + kind: True})
            return _filter_out(kind, g, M, ctx.filter_report())

        @staticmethod
        def expect(oracle, inp, on):
            return _filter_expect(oracle, inp, kind, on)
    _case("filter_" + kind, ("guided", "device_graphs"), branch=_FILTER_BRANCH, fresh=_FILTER_FRESH)(F)


for _k in "FEH":
    _filter_case(_k)


def _feh_case(which):
    class F:
        make = staticmethod(filter_inputs)

        @staticmethod
        def run(ctx, inp, on):
            put = _filter_register(ctx, inp)
            got, _, _ = ctx.filter_FEH(put, which)
            out = {}
            for k in which:
                out.update(_filter_out(k, got[k]))
            out["report"] = np.array(ctx.filter_report(), np.float64).reshape(-1, 5)
            return out

        @staticmethod
        def expect(oracle, inp, on):
            out = {}
            for k in which:
                out.update(_filter_expect(oracle, inp, k, on))
            return out
    _case("filter_" + which, ("guided", "device_graphs"), branch=_FILTER_BRANCH, fresh=_FILTER_FRESH)(F)


for _w in ("FEH", "FH", "EH"):
    _feh_case(_w)


# guided_match with the caller's models: one translation per pair (the mean displacement of its putatives), 8 px, ratio 0.6 and
# geometry only.  large: 9500 queries = 38 blocks of 256 (the last one partial), J = 9500 positions = two tiles of 8192;
# small: 800 rows, one J tile.  Restated by guided_restatement.guided_pair.
# The candidate-chunk budget (api_guided.cpp: 2^28 candidates per chunk) is out of reach at test sizes -- 9500 x 9500 pairs of
# positions are 9.0e7 -- so with the product library every guided call here is ONE chunk.  The chunked path is reached with the
# developer build's R3DM_GUIDED_CAND_BUDGET (DEV_KNOBS below): 256 lies between the 48 candidates of the small variant and the 1997
# of the large one (tests/test_history_cases.py counts them with the restatement), so large is cut into chunks and small is not.
@_case("guided_match", ("device_graphs",), branch="9500-row views (38 query blocks, 2 J tiles of 8192; several chunks under DEV_KNOBS) against 800-row views (1 J tile, 1 chunk)")
class _Guided:
    @staticmethod
    def make(variant):
        inp = dict(filter_inputs(variant))
        o = inp["offsets"].astype(np.int64)
        Hs = []
        for p, (I, J) in enumerate(inp["pairs"]):
            m = inp["matches"][o[p]:o[p + 1]]
            dx, dy = np.mean(inp["xys"][int(J)][m[:, 1]].astype(np.float64) - inp["xys"][int(I)][m[:, 0]], axis=0)
            Hs.append([1, 0, dx, 0, 1, dy, 0, 0, 1])
        inp["models"] = np.array(Hs, np.float64); inp["thr"] = np.full(len(Hs), 8.0)
        return inp

    @staticmethod
    def run(ctx, inp, on):
        _filter_register(ctx, inp)
        out = {}
        for tag, ratio in (("ratio", 0.6), ("geom", -1.0)):
            out.update({tag + "_" + k: v for k, v in _graph(ctx.guided_match(inp["pairs"], "H", inp["models"], inp["thr"], ratio)).items()})
        return out

    @staticmethod
    def expect(oracle, inp, on):
        import guided_restatement as G
        out = {}
        for tag, ratio in (("ratio", 0.6), ("geom", -1.0)):
            P, Off, Mm = [], [0], []
            for (I, J), M, t in zip(inp["pairs"].tolist(), inp["models"], inp["thr"]):
                m = G.guided_pair("H", M, t, ratio, inp["xys"][I], inp["xys"][J], inp["descs"][I], inp["descs"][J], False, inp["K"], inp["K"])
                if len(m):
                    P.append((I, J)); Mm.append(m); Off.append(Off[-1] + len(m))
            out[tag + "_pairs"] = np.array(P, np.uint32).reshape(-1, 2); out[tag + "_offsets"] = np.array(Off, np.uint64)
            out[tag + "_matches"] = np.concatenate(Mm).astype(np.uint32) if Mm else np.zeros((0, 2), np.uint32)
        return out


# the exhaustive matcher's finalisation: a pair that keeps more than the 16 384 keys of the LDS sort is sorted in global scratch
# (api_match.cpp).  large: two views of 20 000 rows (nFeatures_'s default), every row of the second a noisy copy of a row of the first
# -> one pair with more than 16 384 matches; small: the same construction at 2 000 rows -> the LDS sort.
@_case("match_long_lists", ("integer_mfma", "device_graphs"), branch="one pair keeping more than 16 384 matches (global-scratch sort) against one keeping fewer than 2 000 (LDS sort)")
class _MatchLong:
    @staticmethod
    def make(variant):
        n = 20000 if variant == "large" else 2000
        A, xyA, B, xyB = _two_view_scene(np.random.default_rng(n), n, 16, 1.0)
        return dict(descs=[A, B], xys=[xyA, xyB], pairs=np.array([[0, 1]], np.uint32))

    @staticmethod
    def run(ctx, inp, on):
        ctx.clear_images()
        for v in range(2):
            ctx.set_image(v, inp["descs"][v], inp["xys"][v], 4000, 3000)
        return _graph(ctx.match_pairs(inp["pairs"], 0.6, True))

    @staticmethod
    def expect(oracle, inp, on):
        c, m = oracle.match_collection(inp["descs"], inp["xys"], inp["pairs"], 0.6, True)
        return _expected_graph(inp["pairs"], c, m)


# ---------------------------------------------------------------------------------------------------------------------------------
# the detectors.
# Fast A-KAZE -- large: 500 x 700 white noise at threshold 1e-6: thousands of candidates per level, more than the kAkLive = 3072
#   live-set slots and more than the small image has pixels in a row, planes of 500 x 700; small: a 120 x 160 scene at 0.001
#   with a handful of candidates, planes of its own size (the plane stride follows the image).
# classic A-KAZE -- large: 480 x 640 scenes (370 / 409 candidates, largest kpts_aux component 10); small: 120 x 160 (26 / 46
#   candidates, largest component 3).  The branch of the walk is a component above the wavefront bound of 64 (handed back to the
#   one-wavefront walk).  No image tried reaches it: white and smooth noise, dense blob fields and blob grids with up to 6358
#   candidates gave a largest component of 25, because a component needs a chain of strict maxima closer than 1.5 sigma at one
#   scale.  With the product library BOTH variants therefore stay on the bucketed side (tests/test_history_cases.py asserts that,
#   so nobody reads more into them); the hand-back side is reached with the developer build's R3DM_AC_AUX_BOUND (DEV_KNOBS below):
#   a bound of 6 lies between the small variant's largest component (3) and the large one's (10).
# ---------------------------------------------------------------------------------------------------------------------------------
def scene_image(h, w, seed, n_blobs=40, noise=0.01):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = 0.5 + 0.1 * np.sin(xx / 17.0) * np.cos(yy / 23.0)
    for _ in range(n_blobs):
        mg = min(40, h // 4)
        cx, cy = rng.uniform(mg, w - mg), rng.uniform(mg, h - mg)
        s = rng.uniform(2, 12); a = rng.uniform(0.15, 0.45) * rng.choice([-1, 1])
        th = rng.uniform(0, np.pi); e = rng.uniform(1.0, 2.5)
        u = (xx - cx) * np.cos(th) + (yy - cy) * np.sin(th); v = -(xx - cx) * np.sin(th) + (yy - cy) * np.cos(th)
        img = img + a * np.exp(-(u * u / (2 * s * s * e) + v * v / (2 * s * s / e)))
    img = img + rng.normal(0, noise, img.shape)
    return np.clip(img, 0, 1).astype(np.float32)


def noise_image(h, w, seed):
    return np.clip(0.5 + np.random.default_rng(seed).normal(0, 0.2, (h, w)), 0, 1).astype(np.float32)


def fast_detector_inputs(variant):
    if variant == "large":
        return dict(images=[noise_image(500, 700, 8), noise_image(500, 700, 18)], thr=1e-6)
    return dict(images=[scene_image(120, 160, 5, n_blobs=8), scene_image(120, 160, 15, n_blobs=8)], thr=0.001)


_FAST_BRANCH = "500 x 700 noise at 1e-6 (more candidates per level than kAkLive = 3072) against a 120 x 160 scene at 0.001"


@_case("detect_akaze", branch=_FAST_BRANCH)
class _Detect:
    make = staticmethod(fast_detector_inputs)

    @staticmethod
    def run(ctx, inp, on):
        k, r = ctx.detect_akaze(inp["images"][0], inp["thr"])
        return dict(kps=k, resp=r)

    @staticmethod
    def expect(oracle, inp, on):
        ref = oracle.akaze_detect(inp["images"][0], inp["thr"])
        return dict(kps=ref["kps"], resp=ref["responses"])


@_case("detect_akaze_mldb", branch=_FAST_BRANCH)
class _DetectMldb:
    make = staticmethod(fast_detector_inputs)

    @staticmethod
    def run(ctx, inp, on):
        k, d = ctx.detect_akaze_mldb(inp["images"][0], inp["thr"])
        return dict(kps=k, desc=d)

    @staticmethod
    def expect(oracle, inp, on):
        k, d, _ = oracle.akaze_detect_mldb(inp["images"][0], inp["thr"])
        return dict(kps=k, desc=d)


@_case("detect_akaze_batch", branch=_FAST_BRANCH)
class _DetectBatch:
    make = staticmethod(fast_detector_inputs)

    @staticmethod
    def run(ctx, inp, on):
        out = {}
        for b, (k, r) in enumerate(ctx.detect_akaze_batch(inp["images"], inp["thr"])):
            out[f"kps{b}"] = k; out[f"resp{b}"] = r
        return out

    @staticmethod
    def expect(oracle, inp, on):
        out = {}
        for b, im in enumerate(inp["images"]):
            ref = oracle.akaze_detect(im, inp["thr"])
            out[f"kps{b}"] = ref["kps"]; out[f"resp{b}"] = ref["responses"]
        return out


def classic_detector_inputs(variant):
    if variant == "large":
        return dict(images=[scene_image(480, 640, 1, n_blobs=38), scene_image(480, 640, 2, n_blobs=38)], thr=0.001)
    return dict(images=[scene_image(120, 160, 5, n_blobs=8), scene_image(120, 160, 15, n_blobs=8)], thr=0.001)


_CLASSIC_BRANCH = "480 x 640 scenes (largest component 10: handed back under DEV_KNOBS' bound of 6) against 120 x 160 scenes (largest component 3: bucketed)"


@_case("detect_akaze_classic", branch=_CLASSIC_BRANCH)
class _Classic:
    make = staticmethod(classic_detector_inputs)

    @staticmethod
    def run(ctx, inp, on):
        k, r = ctx.detect_akaze_classic(inp["images"][0], inp["thr"])
        return dict(kps=k, resp=r)

    @staticmethod
    def expect(oracle, inp, on):
        import akaze_classic_restatement as R
        ref = R.detect(inp["images"][0], inp["thr"])
        return dict(kps=np.asarray(ref["kps"], np.float32).reshape(-1, 4), resp=np.asarray(ref["responses"], np.float32))


@_case("detect_akaze_classic_batch", branch=_CLASSIC_BRANCH)
class _ClassicBatch:
    make = staticmethod(classic_detector_inputs)

    @staticmethod
    def run(ctx, inp, on):
        out = {}
        for b, (k, r) in enumerate(ctx.detect_akaze_classic_batch(inp["images"], inp["thr"])):
            out[f"kps{b}"] = k; out[f"resp{b}"] = r
        return out

    @staticmethod
    def expect(oracle, inp, on):
        import akaze_classic_restatement as R
        out = {}
        for b, im in enumerate(inp["images"]):
            ref = R.detect(im, inp["thr"])
            out[f"kps{b}"] = np.asarray(ref["kps"], np.float32).reshape(-1, 4); out[f"resp{b}"] = np.asarray(ref["responses"], np.float32)
        return out


# ---------------------------------------------------------------------------------------------------------------------------------
# LIOP.  large: 1500 keypoints on a 600 x 800 image with a saturated rectangle and keypoints whose patch leaves the image -> equal
# intensities inside patches -> the exact re-sort (the tie list behind liop_cnt fills); small: 40 keypoints well inside a smooth
# 200 x 260 image whose patches hold no two equal samples -> no re-sort, the tie list keeps the large call's entries.
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def liop_inputs(variant):
    from scipy.ndimage import gaussian_filter
    if variant == "large":
        rng = np.random.default_rng(31)
        img = gaussian_filter(rng.random((600, 800)), 1.5).astype(np.float32)
        img[200:260, 300:380] = 1.0
        n = 1500
        kps = np.stack([rng.uniform(-5, 805, n), rng.uniform(-5, 605, n), rng.uniform(1.5, 12, n), rng.uniform(0, 360, n)], 1).astype(np.float32)
        kps[:50, 0] = rng.uniform(310, 370, 50); kps[:50, 1] = rng.uniform(210, 250, 50); kps[:50, 2] = 2.0
    else:
        rng = np.random.default_rng(32)
        img = gaussian_filter(rng.random((200, 260)), 1.5).astype(np.float32)
        n = 40
        kps = np.stack([rng.uniform(90, 170, 4 * n), rng.uniform(90, 110, 4 * n), rng.uniform(2.0, 6.0, 4 * n), rng.uniform(0, 360, 4 * n)], 1).astype(np.float32)
        # two of ~1257 blurred float samples coincide by chance in about one patch of ten: keep the first 40 keypoints without one
        p = _oracle().liop_extract_patches(img, kps, 8.0)
        kps = np.ascontiguousarray(kps[[k for k in range(len(kps)) if patches_with_ties(p[k:k + 1]) == 0][:n]])
    return dict(image=img, kps=kps)


def patches_with_ties(patches, min_duplicates=1):
    """how many 41 x 41 patches hold at least `min_duplicates` samples equal to another one inside the disc of radius 20 around the
    centre (1257 samples: a superset of the 669 support pixels of the descriptor, so 0 here means no tie there either, and 700 or
    more here leaves at least 112 inside the support)"""
    yy, xx = np.mgrid[0:41, 0:41]
    disc = ((yy - 20) ** 2 + (xx - 20) ** 2) <= 20 * 20
    return int(sum(int(disc.sum()) - len(np.unique(p[disc])) >= min_duplicates for p in patches))


_LIOP_BRANCH = "1500 keypoints, many patches with equal samples (exact re-sort) against 40 keypoints without a single tie"


def _liop_describe(oracle, patches):
    return oracle.ref_liop(patches) if oracle.ref_liop_lib() is not None else oracle.liop_describe(patches)


@_case("extract_liop", branch=_LIOP_BRANCH)
class _Liop:
    make = staticmethod(liop_inputs)

    @staticmethod
    def run(ctx, inp, on):
        return dict(desc=ctx.extract_liop(inp["image"], inp["kps"], 8.0))

    @staticmethod
    def expect(oracle, inp, on):
        return dict(desc=_liop_describe(oracle, oracle.liop_extract_patches(inp["image"], inp["kps"], 8.0)))


@_case("extract_liop_patches", branch=_LIOP_BRANCH)
class _LiopPatches:
    make = staticmethod(liop_inputs)

    @staticmethod
    def run(ctx, inp, on):
        d, p = ctx.extract_liop(inp["image"], inp["kps"], 8.0, want_patches=True)
        return dict(desc=d, patches=p)

    @staticmethod
    def expect(oracle, inp, on):
        p = oracle.liop_extract_patches(inp["image"], inp["kps"], 8.0)
        return dict(desc=_liop_describe(oracle, p), patches=p)


@_case("liop_describe_patches", branch=_LIOP_BRANCH, fresh="n_resorted, how many patches took the exact re-sort, is the device's own count (read from liop_cnt)")
class _LiopDescribe:
    @staticmethod
    def make(variant):
        inp = liop_inputs(variant)
        return dict(patches=_oracle().liop_extract_patches(inp["image"], inp["kps"], 8.0))

    @staticmethod
    def run(ctx, inp, on):
        d, n_resorted = ctx.liop_describe_patches(inp["patches"])
        return dict(desc=d, n_resorted=np.array([n_resorted], np.uint32))

    @staticmethod
    def expect(oracle, inp, on):
        return dict(desc=_liop_describe(oracle, inp["patches"]))


# ---------------------------------------------------------------------------------------------------------------------------------
# the features entries that write files: detector + LIOP + <name>.feat / <name>.desc.  large: 480 x 640 scenes (hundreds of features),
# small: 120 x 160 (a handful).  The .desc file is restated (count + the oracle's descriptors); the .feat file is text written with
# the host's printf, so its bytes are compared with a fresh context's.
# ---------------------------------------------------------------------------------------------------------------------------------
def features_inputs(variant):
    if variant == "large":
        return dict(images=[scene_image(480, 640, 21 + k, n_blobs=38) for k in range(3)], thr=0.001)
    return dict(images=[scene_image(120, 160, 41 + k, n_blobs=8) for k in range(3)], thr=0.001)


def _desc_file(oracle, im, thr):
    kp = oracle.akaze_detect(im, thr)["kps"]
    d = oracle.liop_describe(oracle.liop_extract_patches(im, kp, 8.0)) if len(kp) else np.zeros((0, 144), np.float32)
    return np.frombuffer(np.uint64(len(kp)).tobytes() + np.ascontiguousarray(d, np.float32).tobytes(), np.uint8)


def _read(path):
    return np.frombuffer(open(path, "rb").read(), np.uint8)


_FEAT_BRANCH = "480 x 640 scenes (hundreds of features per file) against 120 x 160 scenes (a handful)"
_FEAT_FRESH = "the .feat files are text printed by the host's printf: compared with a fresh context's bytes"


@_case("extract_features_to_files", ("deferred",), branch=_FEAT_BRANCH, fresh=_FEAT_FRESH)
class _FeatFiles:
    make = staticmethod(features_inputs)

    @staticmethod
    def run(ctx, inp, on):
        import tempfile
        with tempfile.TemporaryDirectory(prefix="r3dm_hist_") as d:
            f, s = os.path.join(d, "a.feat"), os.path.join(d, "a.desc")
            n = ctx.extract_features_to_files(inp["images"][0], f, s, inp["thr"])
            ctx.features_files_wait()
            return dict(n=np.array([n], np.uint32), feat=_read(f), desc=_read(s))

    @staticmethod
    def expect(oracle, inp, on):
        d = _desc_file(oracle, inp["images"][0], inp["thr"])
        return dict(desc=d, n=np.array([int(np.frombuffer(d[:8].tobytes(), np.uint64)[0])], np.uint32))


@_case("extract_features_batch", ("deferred",), branch=_FEAT_BRANCH, fresh=_FEAT_FRESH)
class _FeatBatch:
    make = staticmethod(features_inputs)

    @staticmethod
    def run(ctx, inp, on):
        import tempfile
        B = len(inp["images"])
        with tempfile.TemporaryDirectory(prefix="r3dm_hist_") as d:
            fs = [os.path.join(d, f"i{k}.feat") for k in range(B)]; ss = [os.path.join(d, f"i{k}.desc") for k in range(B)]
            n = ctx.extract_features_batch(inp["images"], fs, ss, inp["thr"])
            ctx.features_files_wait()
            out = dict(n=np.asarray(n, np.uint32))
            for k in range(B):
                out[f"feat{k}"] = _read(fs[k]); out[f"desc{k}"] = _read(ss[k])
            return out

    @staticmethod
    def expect(oracle, inp, on):
        out = {}
        ns = []
        for k, im in enumerate(inp["images"]):
            out[f"desc{k}"] = _desc_file(oracle, im, inp["thr"])
            ns.append(int(np.frombuffer(out[f"desc{k}"][:8].tobytes(), np.uint64)[0]))
        out["n"] = np.array(ns, np.uint32)
        return out


# developer-build knobs under which tests/test_gpu_history.py repeats large-small-large-small in a child process for the cases whose
# branch the product's constants put out of reach (see the classic detector and guided_match above)
DEV_KNOBS = {"R3DM_AC_AUX_BOUND": "6", "R3DM_GUIDED_CAND_BUDGET": "256"}
DEV_CASES = ("detect_akaze_classic", "detect_akaze_classic_batch", "guided_match", "filter_F")


# the families whose members share scratch on the context (test d of tests/test_gpu_history.py runs every ordered pair inside one)
FAMILIES = {
    "matchers (d_cnt / d_fb / d_nn)": ["match_sift", "match_long_lists", "match_kgraph", "match_hnsw", "match_mrpt"],
    "filters (coop_sched, fb[])": ["filter_F", "filter_E", "filter_H", "filter_FEH", "filter_FH", "filter_EH"],
    "LIOP (liop_cnt)": ["extract_liop", "extract_liop_patches", "liop_describe_patches"],
    "detector arms (resident planes)": ["detect_akaze", "detect_akaze_classic", "extract_liop"],
}


# ---------------------------------------------------------------------------------------------------------------------------------
# comparison and the fresh-context child
# ---------------------------------------------------------------------------------------------------------------------------------
def differences(got, exp, keys=None):
    """names of the keys of `exp` (or `keys`) whose arrays differ from `got` in shape, type or bytes"""
    bad = []
    for k in (exp.keys() if keys is None else keys):
        a, b = np.asarray(got[k]), np.asarray(exp[k])
        if a.shape != b.shape or a.dtype != b.dtype or a.tobytes() != b.tobytes():
            bad.append(k)
    return bad


def run_fresh(name, variants, on=(), developer=False):
    """the case on a context of its own, one variant after the other (this function is what the child processes run); a single
    variant gives the case's dict, several give its keys prefixed by the step number"""
    from regard3d_amd import api
    if developer:
        api.use_developer_library()
    case = CASES[name]
    ctx = api.Context(0)
    try:
        outs = [case.run(ctx, case.make(v), frozenset(on)) for v in variants]
    finally:
        ctx.close()
    if len(outs) == 1:
        return outs[0]
    return {f"{step}_{k}": v for step, out in enumerate(outs) for k, v in out.items()}


def fresh_command(out_path, name, variants, on=(), developer=False):
    variants = [variants] if isinstance(variants, str) else list(variants)
    return [sys.executable, os.path.abspath(__file__), out_path, name, ",".join(variants)] + (["--dev"] if developer else []) + sorted(on)


if __name__ == "__main__":
    out_path, name, variants = sys.argv[1:4]
    rest = sys.argv[4:]
    np.savez(out_path, **run_fresh(name, variants.split(","), [a for a in rest if a != "--dev"], developer="--dev" in rest))
