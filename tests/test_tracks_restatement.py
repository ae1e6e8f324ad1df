"""The plain-Python restatement of r3dm_build_tracks (tests/tracks_restatement.py) against a second, independent formulation and
against answers worked out by hand; and the new entries in the library's interface.  No GPU needed."""
import os
import re

import numpy as np
import pytest

import tracks_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACK_ENTRIES = ["r3dm_build_tracks", "r3dm_tracks_count", "r3dm_tracks_offsets", "r3dm_tracks_observations", "r3dm_tracks_report",
                 "r3dm_tracks_phase_ms", "r3dm_tracks_in_pair", "r3dm_tracks_free"]


def _same(a, b, graph, queries):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and np.array_equal(a[3], b[3])
    for x, y in queries:
        assert np.array_equal(a[4](x, y), b[4](x, y))


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("min_length", [2, 3, 5])
def test_union_find_equals_bfs_on_random_graphs(seed, min_length):
    g = R.world_graph(7, 60, 150, 0.6, 25, seed)
    _same(R.build_tracks(*g, min_length), R.tracks_by_bfs(*g, min_length), g, [(0, 1), (3, 6), (6, 3), (2, 99)])


def test_union_find_equals_bfs_with_self_pairs_duplicates_and_swapped_pairs():
    rng = np.random.default_rng(5)
    entries = []
    for I, J in [(0, 1), (1, 0), (2, 2), (0, 1), (1, 2), (2, 0), (4000000000, 1)]:
        entries.append(((I, J), [tuple(int(x) for x in rng.integers(0, 12, 2)) for _ in range(9)]))
    g = R.graph_arrays(entries)
    for ml in (2, 3):
        _same(R.build_tracks(*g, ml), R.tracks_by_bfs(*g, ml), g, [(0, 1), (1, 2), (4000000000, 0)])


def test_known_answer():
    g = R.graph_arrays(R.KNOWN)
    offs, obs, st, kept, in_pair = R.build_tracks(*g, 2)
    assert (st["n_nodes"], st["n_components"], st["n_conflicting"], st["n_short"]) == (12, 4, 1, 0)
    assert offs.tolist() == [0, 3, 6, 8]
    assert obs.tolist() == [[0, 0], [1, 0], [2, 0], [0, 2], [1, 3], [2, 2], [0, 9], [1, 9]]
    assert st["n_matches_kept"] == 6 and st["n_matches"] == 9 and st["longest"] == 3 and st["largest_component"] == 4
    kp, ko, km = R.kept_graph(*g, kept)
    assert kp.tolist() == [[0, 1], [0, 2], [1, 2]] and ko.tolist() == [0, 3, 4, 6]
    assert km.tolist() == [[0, 0], [2, 3], [9, 9], [0, 0], [0, 0], [3, 2]]
    assert in_pair(0, 2).tolist() == [[0, 0], [2, 2]]            # the second is transitive, not a match of the input
    assert in_pair(2, 0).tolist() == [[0, 0], [2, 2]]            # ... (2, 2) with the columns swapped is (2, 2)
    assert in_pair(1, 2).tolist() == [[0, 0], [3, 2]] and in_pair(2, 1).tolist() == [[0, 0], [2, 3]]
    assert in_pair(0, 77).shape == (0, 2)
    offs, obs, st, _, _ = R.build_tracks(*g, 3)
    assert obs.tolist() == [[0, 0], [1, 0], [2, 0], [0, 2], [1, 3], [2, 2]] and st["n_short"] == 1 and st["n_tracks"] == 2
    offs, obs, st, _, _ = R.build_tracks(*g, 4)
    assert offs.tolist() == [0] and len(obs) == 0 and st["n_short"] == 3 and st["n_conflicting"] == 1


def test_known_answer_conflicting_component():
    """the conflicting component of the known answer is {(0,1), (1,1), (2,5), (2,6)}: none of its nodes is observed"""
    _, obs, _, kept, _ = R.build_tracks(*R.graph_arrays(R.KNOWN), 2)
    assert not {(0, 1), (1, 1), (2, 5), (2, 6)} & set(map(tuple, obs.tolist()))
    assert kept.tolist() == [True, False, True, True, True, False, True, False, True]


def test_self_pair():
    offs, obs, st, kept, _ = R.build_tracks(*R.graph_arrays(R.SELF_PAIR), 2)
    assert obs.tolist() == [[3, 1], [4, 0]] and offs.tolist() == [0, 2]
    assert st["n_conflicting"] == 1 and st["n_components"] == 2 and kept.tolist() == [True, False, True]


def test_track_entries_are_in_the_interface():
    """the new entries are declared in include/r3dm.h, listed in api.EXPORTS and exported by the built library"""
    from regard3d_amd import api
    L = api.load_library()
    header = open(os.path.join(ROOT, "include", "r3dm.h")).read()
    for name in TRACK_ENTRIES:
        assert name in api.EXPORTS, name
        assert hasattr(L, name), f"libr3dm.so lacks {name}"
        assert re.search(r"\b" + name + r"\s*\(", header), f"include/r3dm.h does not declare {name}"
    for name in ("build_tracks",):
        assert hasattr(api.Context, name)
    assert all(hasattr(api.Tracks, n) for n in ("offsets", "observations", "stats", "in_pair", "close"))


def test_null_handles_are_refused_without_a_gpu():
    """argument checks come before any device work: they answer on a machine without a GPU too"""
    from regard3d_amd import api
    import ctypes as C
    L = api.load_library()
    out = C.c_void_p()
    assert L.r3dm_build_tracks(None, None, 2, C.byref(out), None) == -1
    n = C.c_uint64(5)
    assert L.r3dm_tracks_in_pair(None, 0, 1, None, 0, C.byref(n)) == -1 and n.value == 0
    assert L.r3dm_tracks_report(None, None) == -1 and L.r3dm_tracks_phase_ms(None, None) == -1
    assert L.r3dm_tracks_count(None) == 0 and L.r3dm_tracks_offsets(None) is None
    L.r3dm_tracks_free(None)


def test_closed_tracks_object_raises():
    from regard3d_amd import api
    t = api.Tracks(None)
    for read in (lambda: t.offsets, lambda: t.observations, lambda: t.stats, lambda: t.phase_ms, lambda: len(t), lambda: t.in_pair(0, 1)):
        with pytest.raises(api.R3dmError):
            read()
    t.close()


def _perf_tool():
    import importlib.util
    spec = importlib.util.spec_from_file_location("tracks_perf", os.path.join(ROOT, "tools", "tracks_perf.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_perf_tool_star_fits_the_slot_limit():
    """the star the tool times at its default size: one conflicting component of 100,001 nodes whose slots -- the sum over the views of
    (largest feature index + 1) -- stay within R3DM_TRACKS_MAX_SLOTS, so the library accepts it"""
    tool = _perf_tool()
    src = open(os.path.join(ROOT, "tools", "tracks_perf.py")).read()
    n_views = int(re.search(r'"--star-views", type=int, default=(\d+)', src).group(1))
    pairs, offsets, matches = tool.star_graph(n_views)
    assert 2 * n_views + 1 >= 100000 and len(matches) == 2 * n_views and int(offsets[-1]) == len(matches)
    extent = {}
    for p in range(len(pairs)):
        for m in range(int(offsets[p]), int(offsets[p + 1])):
            for v, f in ((int(pairs[p, 0]), int(matches[m, 0])), (int(pairs[p, 1]), int(matches[m, 1]))):
                extent[v] = max(extent.get(v, 0), f + 1)
    limit = int(re.search(r"#define R3DM_TRACKS_MAX_SLOTS \(1ull << (\d+)\)", open(os.path.join(ROOT, "include", "r3dm.h")).read()).group(1))
    assert sum(extent.values()) <= 1 << limit
    _, _, st, kept, _ = R.build_tracks(*tool.star_graph(300))
    assert st["n_components"] == 1 and st["n_conflicting"] == 1 and st["largest_component"] == 601 and not kept.any()


def test_perf_tool_host_baseline_equals_restatement(tmp_path):
    """the single-thread C++ union-find the tool compares the device with computes the restatement's counts, and refuses what the
    library refuses"""
    import subprocess
    import types
    tool = _perf_tool()
    src, exe = str(tmp_path / "host_tracks.cpp"), str(tmp_path / "host_tracks")
    open(src, "w").write(tool.HOST_CPP)
    subprocess.check_call(["g++", "-O2", "-std=c++17", src, "-o", exe])
    for arrays, ml in ((R.world_graph(**R.SMALL_WORLD), 2), (R.world_graph(**R.SMALL_WORLD), 3), (R.graph_arrays(R.KNOWN), 2), (tool.star_graph(500), 2)):
        g = types.SimpleNamespace(pairs=arrays[0], offsets=arrays[1], matches=arrays[2], num_pairs=len(arrays[0]), num_matches=len(arrays[2]))
        _, _, _, counts = tool.host_baseline(str(tmp_path), exe, g, ml, 1)
        st = R.build_tracks(*arrays, ml)[2]
        assert counts == {k: st[k] for k in counts}
    big = R.graph_arrays([((0, 1), [(1 << 28, 0)])])
    g = types.SimpleNamespace(pairs=big[0], offsets=big[1], matches=big[2], num_pairs=1, num_matches=1)
    with pytest.raises(subprocess.CalledProcessError):
        tool.host_baseline(str(tmp_path), exe, g, 2, 1)
