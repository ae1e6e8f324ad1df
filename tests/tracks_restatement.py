"""Feature tracks of a match graph, restated in plain Python: what r3dm_build_tracks must return (include/r3dm.h), i.e. OpenMVG's
TracksBuilder::Build + Filter + ExportToSTL + GetTracksInImages in this library's canonical order.  A union-find over a dict of
nodes; `tracks_by_bfs` is a second, independent formulation (breadth-first search over an adjacency dict, and its own filter, ordering,
counters, kept mask and in_pair: `_finish_by_sets`) the first is tested against.

A graph is (pairs [P, 2], offsets [P + 1], matches [M, 2]) as api.Graph holds it; `graph_arrays` builds that from a list of
((I, J), [(i, j), ...]) entries in the order given."""
from collections import defaultdict, deque

import numpy as np


def graph_arrays(entries):
    pairs = np.array([e[0] for e in entries], np.uint32).reshape(-1, 2)
    counts = [len(e[1]) for e in entries]
    offsets = np.r_[0, np.cumsum(counts)].astype(np.uint64)
    flat = [m for e in entries for m in e[1]]
    return pairs, offsets, np.array(flat, np.uint32).reshape(-1, 2)


def _edges(pairs, offsets, matches):
    for p in range(len(pairs)):
        I, J = int(pairs[p, 0]), int(pairs[p, 1])
        for m in range(int(offsets[p]), int(offsets[p + 1])):
            yield (I, int(matches[m, 0])), (J, int(matches[m, 1]))


def _finish(components, node_comp, pairs, offsets, matches, min_length):
    """components: lists of nodes; node_comp: node -> index into components"""
    assert min_length >= 2
    status = []                                   # per component: "conflict", "short" or "track"
    for c in components:
        views = [v for v, _ in c]
        if len(set(views)) != len(views):
            status.append("conflict")
        elif len(c) < min_length:
            status.append("short")
        else:
            status.append("track")
    tracks = sorted(sorted(c) for c, s in zip(components, status) if s == "track")      # by first observation: the smallest (view, feature)
    offs = np.r_[0, np.cumsum([len(t) for t in tracks])].astype(np.uint64)
    obs = np.array([o for t in tracks for o in t], np.uint32).reshape(-1, 2)
    kept = np.array([status[node_comp[a]] == "track" for a, _ in _edges(pairs, offsets, matches)], bool)
    stats = dict(n_matches=len(matches), n_nodes=len(node_comp), n_components=len(components),
                 n_conflicting=status.count("conflict"), n_short=status.count("short"), n_tracks=len(tracks), n_observations=len(obs),
                 n_matches_kept=int(kept.sum()), longest=max([len(t) for t in tracks], default=0),
                 largest_component=max([len(c) for c in components], default=0))

    def in_pair(a, b):
        assert a != b
        out = []
        for t in tracks:
            d = dict(t)
            if a in d and b in d:
                out.append((d[a], d[b]))
        return np.array(out, np.uint32).reshape(-1, 2)

    return offs, obs, stats, kept, in_pair


def build_tracks(pairs, offsets, matches, min_length=2):
    """(offsets, observations, stats, kept mask over the matches, in_pair(a, b)) by union-find over a dict of nodes"""
    parent = {}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in _edges(pairs, offsets, matches):
        parent.setdefault(a, a); parent.setdefault(b, b)
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra] = rb
    by_root = defaultdict(list)
    for x in parent:
        by_root[find(x)].append(x)
    components = list(by_root.values())
    node_comp = {x: k for k, c in enumerate(components) for x in c}
    return _finish(components, node_comp, pairs, offsets, matches, min_length)


def tracks_by_bfs(pairs, offsets, matches, min_length=2):
    """the same by breadth-first search over an adjacency dict"""
    adj = defaultdict(set)
    for a, b in _edges(pairs, offsets, matches):
        adj[a].add(b); adj[b].add(a)
    node_comp, components = {}, []
    for s in adj:
        if s in node_comp:
            continue
        node_comp[s] = len(components)
        comp, q = [s], deque([s])
        while q:
            for y in adj[q.popleft()]:
                if y not in node_comp:
                    node_comp[y] = len(components); comp.append(y); q.append(y)
        components.append(comp)
    return _finish_by_sets(components, pairs, offsets, matches, min_length)


def _finish_by_sets(components, pairs, offsets, matches, min_length):
    """_finish written a second time, sharing nothing with it: views counted per component, tracks keyed by their smallest node,
    kept matches by set membership"""
    tracks, n_conf, n_short = {}, 0, 0
    for comp in components:
        per_view = defaultdict(int)
        for v, _ in comp:
            per_view[v] += 1
        if max(per_view.values()) > 1:
            n_conf += 1
        elif len(comp) < min_length:
            n_short += 1
        else:
            tracks[min(comp)] = sorted(comp, key=lambda o: o[0])
    firsts = sorted(tracks)
    obs, offs, in_track = [], [0], set()
    for first in firsts:
        obs.extend(tracks[first]); offs.append(len(obs)); in_track.update(tracks[first])
    kept = np.zeros(len(matches), bool)
    for p in range(len(pairs)):
        for m in range(int(offsets[p]), int(offsets[p + 1])):
            kept[m] = (int(pairs[p, 1]), int(matches[m, 1])) in in_track
    stats = dict(n_matches=len(matches), n_nodes=sum(len(c) for c in components), n_components=len(components), n_conflicting=n_conf,
                 n_short=n_short, n_tracks=len(firsts), n_observations=len(obs), n_matches_kept=int(np.count_nonzero(kept)),
                 longest=max((len(t) for t in tracks.values()), default=0), largest_component=max((len(c) for c in components), default=0))

    def in_pair(a, b):
        out = []
        for first in firsts:
            fa = [f for v, f in tracks[first] if v == a]; fb = [f for v, f in tracks[first] if v == b]
            if fa and fb:
                out.append((fa[0], fb[0]))
        return np.array(out, np.uint32).reshape(-1, 2)

    return np.array(offs, np.uint64), np.array(obs, np.uint32).reshape(-1, 2), stats, kept, in_pair


def kept_graph(pairs, offsets, matches, kept):
    """the graph restricted to the kept matches: order unchanged, pairs left empty dropped"""
    P, O, Mm = [], [0], []
    for p in range(len(pairs)):
        sel = [m for m in range(int(offsets[p]), int(offsets[p + 1])) if kept[m]]
        if sel:
            P.append(pairs[p]); Mm.extend(matches[m] for m in sel); O.append(len(Mm))
    return (np.array(P, np.uint32).reshape(-1, 2), np.array(O, np.uint64), np.array(Mm, np.uint32).reshape(-1, 2))


# ---- the graphs of the tests ---------------------------------------------------------------------------------------------------
KNOWN = [((0, 1), [(0, 0), (1, 1), (2, 3), (9, 9)]), ((0, 2), [(0, 0), (1, 5)]), ((1, 2), [(0, 0), (1, 6), (3, 2)])]
SELF_PAIR = [((3, 3), [(1, 1), (5, 6)]), ((3, 4), [(1, 0)])]


def world_graph(V, n_features, n_points, p, w, seed, max_views=8):
    """points observed in a random subset of 2 .. max_views of the V views at distinct feature indices; an edge between two observations
    of a point with probability p; w wrong edges between random features"""
    rng = np.random.default_rng(seed)
    free = [list(rng.permutation(n_features)) for _ in range(V)]
    per_pair = defaultdict(list)
    for _ in range(n_points):
        k = int(rng.integers(2, min(V, max_views) + 1))
        views = sorted(int(v) for v in rng.choice(V, k, replace=False) if free[v])
        ob = [(v, int(free[v].pop())) for v in views]
        for x in range(len(ob)):
            for y in range(x + 1, len(ob)):
                if rng.random() < p:
                    per_pair[(ob[x][0], ob[y][0])].append((ob[x][1], ob[y][1]))
    for _ in range(w):
        a, b = sorted(int(v) for v in rng.choice(V, 2, replace=False))
        per_pair[(a, b)].append((int(rng.integers(n_features)), int(rng.integers(n_features))))
    return graph_arrays([(k, per_pair[k]) for k in sorted(per_pair)])


# parameters of the random graphs of the GPU tests (seeds picked for the floors test_gpu_tracks.py asserts)
SMALL_WORLD = dict(V=12, n_features=300, n_points=900, p=0.6, w=60, seed=5, max_views=8)
MID_WORLD = dict(V=20, n_features=700, n_points=3000, p=0.55, w=300, seed=11, max_views=10)
LARGE_WORLD = dict(V=40, n_features=2048, n_points=12000, p=0.5, w=2000, seed=7, max_views=16)
