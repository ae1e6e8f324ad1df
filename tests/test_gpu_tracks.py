"""r3dm_build_tracks on the GPU against the plain-Python restatement (tests/tracks_restatement.py): offsets, observations, every
counter of the statistics, the kept graph and some in_pair queries, exactly.  The graphs are built with api.Graph.from_csr and read
back from the library before they are restated, so both sides see the same pair order."""
import functools

import numpy as np
import pytest

import tracks_restatement as R

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _world(large: bool):
    return R.world_graph(**(R.LARGE_WORLD if large else R.SMALL_WORLD))


def _outputs(t, k):
    return (t.offsets, t.observations, {n: v for n, v in t.stats.as_dict().items() if not n.startswith("ms_")}, k.pairs, k.offsets, k.matches)


def check(ctx, arrays, min_length=2, queries=()):
    """tracks of the graph on the device == the restatement of the graph as the library holds it; returns the restatement"""
    from regard3d_amd import api
    g = api.Graph.from_csr(*arrays)
    P, O, M = g.pairs, g.offsets, g.matches
    t, k = ctx.build_tracks(g, min_length, want_graph=True)
    offs, obs, st, kept, in_pair = exp = R.build_tracks(P, O, M, min_length)
    assert t.offsets.dtype == np.uint64 and np.array_equal(t.offsets, offs) and len(t) == st["n_tracks"]
    assert np.array_equal(t.observations, obs)
    got = t.stats.as_dict()
    for name, value in st.items():
        assert got[name] == value, (name, got[name], value)
    assert (t.phase_ms >= 0).all() and abs(float(t.phase_ms.sum()) - got["ms_kernels"]) <= 1e-9 * max(1.0, got["ms_kernels"])
    kp, ko, km = R.kept_graph(P, O, M, kept)
    assert np.array_equal(k.pairs, kp) and np.array_equal(k.offsets, ko) and np.array_equal(k.matches, km)
    assert k.on_device == -1                                   # (the shared context never switches device graphs on)
    views = sorted({int(v) for v in P.ravel()})
    for a, b in list(queries) + [(views[0], views[-1]), (views[-1], views[0])] if len(views) > 1 else []:
        assert np.array_equal(t.in_pair(a, b), in_pair(a, b)), (a, b)
    t.close()
    return exp


@pytest.mark.parametrize("min_length", [2, 3, 4])
def test_known_answer(ctx, min_length):
    offs, obs, st, _, _ = check(ctx, R.graph_arrays(R.KNOWN), min_length, [(0, 2), (2, 0), (1, 2), (0, 77)])
    assert (st["n_nodes"], st["n_components"], st["n_conflicting"]) == (12, 4, 1)
    assert st["n_short"] == {2: 0, 3: 1, 4: 3}[min_length] and st["n_tracks"] == {2: 3, 3: 2, 4: 0}[min_length]


def test_self_pair_empty_graph_and_one_match(ctx):
    from regard3d_amd import api
    _, obs, st, _, _ = check(ctx, R.graph_arrays(R.SELF_PAIR))
    assert obs.tolist() == [[3, 1], [4, 0]] and st["n_conflicting"] == 1
    g = api.Graph.from_csr(np.zeros((0, 2), np.uint32), np.zeros(1, np.uint64), np.zeros((0, 2), np.uint32))
    t, k = ctx.build_tracks(g, 2, want_graph=True)
    assert len(t) == 0 and t.offsets.tolist() == [0] and t.observations.shape == (0, 2) and k.num_pairs == 0 and k.num_matches == 0
    assert all(v == 0 for n, v in t.stats.as_dict().items() if not n.startswith("ms_"))
    assert t.in_pair(0, 1).shape == (0, 2)
    _, obs, st, _, _ = check(ctx, R.graph_arrays([((5, 9), [(4, 2)])]))
    assert obs.tolist() == [[5, 4], [9, 2]] and st["n_tracks"] == 1
    check(ctx, R.graph_arrays([((5, 9), [(4, 2)])]), 3)
    check(ctx, R.graph_arrays([((5, 5), [(4, 4)])]))           # a loop: one node, one short component


@pytest.mark.parametrize("permuted", [False, True])
@pytest.mark.parametrize("min_length", [300, 301])
def test_chain_of_300_views(ctx, permuted, min_length):
    ids = np.random.default_rng(3).permutation(300) if permuted else np.arange(300)
    entries = [((int(ids[v]), int(ids[v + 1])), [(7, 7)]) for v in range(299)]
    offs, obs, st, kept, _ = check(ctx, R.graph_arrays(entries), min_length, [(int(ids[0]), int(ids[150]))])
    assert st["largest_component"] == 300 and st["n_components"] == 1
    assert st["n_tracks"] == (1 if min_length == 300 else 0) and st["n_short"] == (0 if min_length == 300 else 1)


def test_star_junk_beside_clean_tracks(ctx):
    entries = [((0, k), [(0, 2 * k), (0, 2 * k + 1)]) for k in range(1, 2501)]
    entries += [((1, 2), [(10000 + t, 20000 + t) for t in range(50)]), ((2, 3), [(20000 + t, 30000 + t) for t in range(50)])]
    offs, obs, st, kept, _ = check(ctx, R.graph_arrays(entries), 2, [(1, 3), (0, 1)])
    assert st["n_conflicting"] == 1 and st["largest_component"] == 5001 and st["n_tracks"] == 50 and st["n_matches_kept"] == 100
    assert np.array_equal(np.diff(offs.astype(np.int64)), np.full(50, 3))


def test_conflict_at_distance(ctx):
    closed = [((0, 1), [(1, 5)]), ((1, 2), [(5, 9)]), ((0, 2), [(2, 9)])]      # (0,1) - (1,5) - (2,9) - (0,2): two features of view 0
    _, _, st, _, _ = check(ctx, R.graph_arrays(closed))
    assert st["n_conflicting"] == 1 and st["n_tracks"] == 0
    _, obs, st, _, _ = check(ctx, R.graph_arrays(closed[:2]))
    assert st["n_conflicting"] == 0 and obs.tolist() == [[0, 1], [1, 5], [2, 9]]


def test_component_size_equal_to_the_number_of_views(ctx):
    clean = [((v, v + 1), [(3, 3)]) for v in range(4)]                            # one track that observes all 5 views
    _, _, st, _, _ = check(ctx, R.graph_arrays(clean))
    assert st["n_tracks"] == 1 and st["longest"] == 5 and st["n_conflicting"] == 0
    _, _, st, _, _ = check(ctx, R.graph_arrays(clean + [((0, 4), [(4, 3)])]))     # ... plus one node: 6 nodes in 5 views
    assert st["n_tracks"] == 0 and st["n_conflicting"] == 1 and st["largest_component"] == 6


def test_duplicates_swapped_pairs_sparse_ids_and_large_indices(ctx):
    big = 1 << 20
    A, B, Cc = 7, 1000000, 4294967294
    entries = [((A, B), [(1, 1), (1, 1), (2, 2), (big - 1, big - 3)]),            # a duplicate edge
               ((B, A), [(1, 1), (5, 2), (big - 3, big - 1)]),                    # the same views the other way round: (B,5) joins (A,2)
               ((A, B), [(2, 2), (9, 9)]),                                        # the same pair listed twice
               ((B, Cc), [(9, big + 5), (2, 0), (5, 0)]),                         # (B,2) and (B,5) meet in (Cc,0): a conflict
               ((Cc, A), [(big + 5, 9)])]
    for ml in (2, 3):
        check(ctx, R.graph_arrays(entries), ml, [(A, B), (B, A), (A, Cc), (Cc, B)])


def test_limits_and_errors(ctx):
    from regard3d_amd import api
    g = api.Graph.from_csr(*R.graph_arrays([((0, 1), [(1 << 28, 0)])]))
    with pytest.raises(api.R3dmError, match=r"-> -5"):          # R3DM_ERR_UNSUPPORTED
        ctx.build_tracks(g)
    ok = api.Graph.from_csr(*R.graph_arrays([((0, 1), [((1 << 28) - 2, 0)])]))       # s(0) + s(1) = 2^28 exactly: the limit itself
    own = api.Context(0)                                        # (a context of its own: the slot arrays of this call go back with it)
    try:
        t = own.build_tracks(ok)
        assert t.observations.tolist() == [[0, (1 << 28) - 2], [1, 0]] and t.stats.n_nodes == 2
        check(own, R.graph_arrays(R.KNOWN))                     # the per-slot arrays of that call went back to the device: the next call makes its own
    finally:
        own.close()
    for ml in (0, 1):
        with pytest.raises(api.R3dmError, match=r"-> -1"):      # R3DM_ERR_INVALID
            ctx.build_tracks(ok, ml)
    with pytest.raises(api.R3dmError):
        t.in_pair(3, 3)
    t.close()
    with pytest.raises(api.R3dmError):                          # a closed object says so
        t.offsets


@pytest.mark.parametrize("min_length", [2, 3])
@pytest.mark.parametrize("large", [False, True])
def test_random_world_graphs(ctx, large, min_length):
    offs, obs, st, kept, _ = check(ctx, _world(large), min_length, [(0, 1), (3, 9), (9, 3)])
    # the floors that keep the comparison from being vacuous, on the restatement's own numbers
    assert st["n_conflicting"] >= (500 if large else 20)
    if large:
        assert st["largest_component"] > 64 and st["n_matches"] > 100000
    assert len(set(np.diff(offs.astype(np.int64)).tolist())) >= 3
    assert 0 < st["n_matches_kept"] < st["n_matches"]
    if min_length == 3:
        assert st["n_short"] > 0


def test_mirrored_graph_uploaded_copy_and_restatement_agree():
    from regard3d_amd import api, synth
    sc = synth.make_scene(9, 1400, "sift", seed=77)
    c = api.Context(0)
    try:
        for i in range(sc.n_images):
            c.set_image(i, sc.descs[i], sc.xys[i], int(sc.widths[i]), int(sc.heights[i]))
        c.set_device_graphs(True)
        gf = c.filter_F(c.match_pairs(sc.exhaustive_pairs(), 0.8, True), 4.0, 2048, seed=5489)
        assert gf.on_device == 0 and gf.num_matches > 1000
        copy = api.Graph.from_csr(gf.pairs, gf.offsets, gf.matches)
        assert copy.on_device == -1
        t1, k1 = c.build_tracks(gf, 2, want_graph=True)
        t2, k2 = c.build_tracks(copy, 2, want_graph=True)
        assert k1.on_device == 0 and k2.on_device == 0
        offs, obs, st, kept, _ = R.build_tracks(gf.pairs, gf.offsets, gf.matches, 2)
        kp, ko, km = R.kept_graph(gf.pairs, gf.offsets, gf.matches, kept)
        assert st["n_tracks"] > 100
        for t, k in ((t1, k1), (t2, k2)):
            assert np.array_equal(t.offsets, offs) and np.array_equal(t.observations, obs)
            got = t.stats.as_dict()
            assert all(got[n] == v for n, v in st.items())
            assert np.array_equal(k.pairs, kp) and np.array_equal(k.offsets, ko) and np.array_equal(k.matches, km)
        c.set_device_graphs(False)
        t3, k3 = c.build_tracks(gf, 2, want_graph=True)         # the input's mirror is still read; the result gets none
        assert k3.on_device == -1 and np.array_equal(k3.matches, km) and np.array_equal(t3.observations, obs)
    finally:
        c.close()


def test_outputs_do_not_depend_on_history(ctx):
    from regard3d_amd import api
    A = api.Graph.from_csr(*_world(False))
    Bg = api.Graph.from_csr(*R.graph_arrays([((0, k), [(0, 2 * k), (0, 2 * k + 1)]) for k in range(1, 400)] + [((1, 2), [(5000, 5000)])]))
    runs = []
    for g in (A, Bg, A):
        runs.append(_outputs(*ctx.build_tracks(g, 3, want_graph=True)))
    fresh = api.Context(0)
    try:
        runs.append(_outputs(*fresh.build_tracks(A, 3, want_graph=True)))
    finally:
        fresh.close()
    for other in (runs[2], runs[3]):
        for x, y in zip(runs[0], other):
            if isinstance(x, dict):
                assert x == y
            else:
                assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
    assert runs[1][2]["n_conflicting"] == 1
