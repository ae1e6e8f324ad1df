"""The pair-list contract of the four collection matchers (r3dm_match_pairs and its _kgraph / _hnsw / _mrpt siblings) on a list that is
none of the things the other tests hand them: shuffled, with duplicates, with pairs that are skipped (two descriptor lengths, an empty
view, a binary view against float views) between the valid ones, with views above and below the 128-row index threshold, and long
enough in kinds that the sorted list is cut into three chunks (I = 0: 128-D indexed, I = 1: scanned, I = 2: 64-D indexed, I = 3: 128-D
indexed again; MRPT does not cut on the length).
  (i)   the graph equals the graph of the sorted, de-duplicated list of valid pairs, and -- pair by pair -- the graph of a call with
        that pair alone on a fresh registration: neither the list's order nor a batch's composition leaks into a pair;
  (ii)  n_pairs counts the valid unique pairs, n_ann_built the distinct indexed first views;
  (iii) the mirror rule of r3dm_set_device_graphs: a list that is all scanned or all indexed keeps its device mirror, a mixed list has
        none (Graph.on_device is the mirror's device id, -1 without one);
  (iv)  a pair that names an unregistered view is refused by all four.
"""
import numpy as np
import pytest

from regard3d_amd import api, synth

pytestmark = pytest.mark.gpu

ARMS = {
    "exhaustive": lambda c, p: c.match_pairs(p, 0.8, True),
    "kgraph": lambda c, p: c.match_pairs_kgraph(p, 0.8, api.KGraphParams.preset("default")),
    "hnsw": lambda c, p: c.match_pairs_hnsw(p, 0.8, api.HnswParams.preset("precise")),
    "mrpt": lambda c, p: c.match_pairs_mrpt(p, 0.8, api.MrptParams.preset()),
}
EMPTY, BINARY = 6, 7
VALID = [(0, 1), (0, 3), (0, 5), (1, 3), (1, 5), (2, 4), (3, 5)]          # sorted; 1 is the 60-row view: pairs (1, *) are scanned
INDEXED_FIRST = {0, 2, 3}
SKIPPED = [(0, 2), (2, 3), (4, 5), (0, EMPTY), (2, EMPTY), (EMPTY, BINARY), (0, BINARY), (2, BINARY), (5, BINARY)]
DUPLICATES = [(0, 3), (1, 5), (2, 4), (0, 3), (0, 2), (3, 5)]


def make_views():
    sc = synth.make_scene(6, 200, "sift", seed=9051)
    bn = synth.make_scene(1, 200, "akaze", seed=9052)
    d = [np.ascontiguousarray(x, np.float32) for x in sc.descs]
    out = {0: d[0], 1: d[1][:60], 2: np.ascontiguousarray(d[2][:, :64]), 3: d[3][:130], 4: np.ascontiguousarray(d[4][:, :64]), 5: d[5],
           EMPTY: np.zeros((0, 128), np.float32), BINARY: np.ascontiguousarray(bn.descs[0], np.uint8)}
    xy = {k: np.ascontiguousarray(sc.xys[k][:len(out[k])], np.float32) for k in range(6)}
    xy[EMPTY] = np.zeros((0, 2), np.float32); xy[BINARY] = np.ascontiguousarray(bn.xys[0], np.float32)
    return out, xy


@pytest.fixture(scope="module")
def views():
    return make_views()


def _register(ctx, views, ids):
    descs, xys = views
    ctx.clear_images()
    for v in ids:
        ctx.set_image(v, descs[v], xys[v], binary=(v == BINARY))


def _csr(g):
    return g.pairs.copy(), g.offsets.copy(), g.matches.copy()


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def messy_list():
    pairs = np.array(VALID + SKIPPED + DUPLICATES, np.uint32)
    return pairs[np.random.default_rng(77).permutation(len(pairs))]


@pytest.mark.parametrize("arm", list(ARMS))
def test_messy_list_equals_clean_list_and_single_pairs(ctx, views, arm):
    run = ARMS[arm]
    _register(ctx, views, range(8))
    got = _csr(run(ctx, messy_list()))
    st = ctx.stats()
    assert st.n_pairs == len(VALID)
    assert st.n_ann_built == (0 if arm == "exhaustive" else len(INDEXED_FIRST))
    _register(ctx, views, range(8))
    clean = _csr(run(ctx, np.array(VALID, np.uint32)))
    assert _same(got, clean)
    by_pair = {(int(i), int(j)): got[2][int(got[1][k]):int(got[1][k + 1])] for k, (i, j) in enumerate(got[0])}
    assert set(by_pair) <= set(VALID) and len(got[2]) > 0             # (pairs without a match never enter a graph)
    for i, j in VALID:
        _register(ctx, views, (i, j))
        one = _csr(run(ctx, np.array([(i, j)], np.uint32)))
        if (i, j) in by_pair:
            assert np.array_equal(one[0], [[i, j]]) and np.array_equal(one[2], by_pair[(i, j)]), (i, j)
        else:
            assert len(one[0]) == 0, (i, j)
    ctx.clear_images()


@pytest.mark.parametrize("arm", ["kgraph", "hnsw", "mrpt"])
def test_mirror_survives_exactly_when_one_part_is_the_whole(ctx, views, arm):
    run = ARMS[arm]
    scanned = [p for p in VALID if p[0] not in INDEXED_FIRST]
    indexed = [p for p in VALID if p[0] in INDEXED_FIRST]
    _register(ctx, views, range(8))
    ctx.set_device_graphs(True)
    try:
        dev = 0                                                       # the session context lives on device 0
        assert run(ctx, np.array(scanned, np.uint32)).on_device == dev
        assert run(ctx, np.array(indexed, np.uint32)).on_device == dev
        g = run(ctx, messy_list())
        assert g.on_device == -1 and g.num_pairs > 0
    finally:
        ctx.set_device_graphs(False)
        ctx.clear_images()


@pytest.mark.parametrize("arm", list(ARMS))
def test_unregistered_view_is_refused(ctx, views, arm):
    _register(ctx, views, range(8))
    with pytest.raises(api.R3dmError):
        ARMS[arm](ctx, np.array([(0, 3), (0, 99)], np.uint32))
    ctx.clear_images()
