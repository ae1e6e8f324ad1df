"""Cost of r3dm_build_tracks on BASELINE config C2's F-filtered graph -- 200 views x 8,192 SIFT-128 rows, 19,900 pairs,
ratio 0.6, F AC-RANSAC -- and on a star-shaped junk component of 100 k nodes:
    python tools/tracks_perf.py [--images N] [--feat N] [--reps R] [--star-views N] [--no-host-baseline]
One JSON line per measurement:
  mirrored   the graph as r3dm_filter_F left it with r3dm_set_device_graphs on: read where it is
  uploaded   its r3dm_graph_from_csr copy: the matches are uploaded by the call
  host       a plain single-thread C++ union-find + std::sort doing the same job on flat arrays (compiled here with g++ -O2; the time
             excludes reading the graph): the stand-in for OpenMVG's TracksBuilder, which works through a std::set of nodes, a std::map
             node -> index and a lemon union-find and can only be slower
ms_kernels is the HIP-event time of the device work, ms_wall the whole call (medians of --reps calls after one warm-up call);
ms_phases splits ms_kernels into the call's four phases (r3dm_tracks_phase_ms).  The tool does not time single kernels: for that
split run it under `rocprofv3 --kernel-trace --stats` and summarise the result with tools/rocprof_summary.py."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HOST_CPP = r"""
// tracks of a match graph on one host thread: slots by per-view bases, union-find (path halving, smaller root wins), nodes sorted by
// (root, slot), conflicts = neighbours of one view, filter, observations + kept matches.  Prints the milliseconds and the counts.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
static std::vector<uint32_t> par;
static uint32_t find(uint32_t x) { while (par[x] != x) { par[x] = par[par[x]]; x = par[x]; } return x; }
int main(int argc, char** argv)
{
    FILE* f = fopen(argv[1], "rb");
    const uint32_t min_length = (uint32_t)atoi(argv[2]);
    uint64_t P, M;
    if (!f || fread(&P, 8, 1, f) != 1 || fread(&M, 8, 1, f) != 1) return 2;
    std::vector<uint32_t> pairs(2 * P), m(2 * M); std::vector<uint64_t> off(P + 1);
    if (fread(pairs.data(), 8, P, f) != P || fread(off.data(), 8, P + 1, f) != P + 1 || fread(m.data(), 8, M, f) != M) return 2;
    fclose(f);
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint32_t> ids(pairs); std::sort(ids.begin(), ids.end()); ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    const size_t V = ids.size();
    std::vector<uint32_t> rank(2 * P);
    for (size_t k = 0; k < 2 * P; ++k) rank[k] = (uint32_t)(std::lower_bound(ids.begin(), ids.end(), pairs[k]) - ids.begin());
    std::vector<uint64_t> ext(V, 0);
    for (uint64_t p = 0; p < P; ++p) for (uint64_t q = off[p]; q < off[p + 1]; ++q) {
        ext[rank[2 * p]] = std::max<uint64_t>(ext[rank[2 * p]], (uint64_t)m[2 * q] + 1); ext[rank[2 * p + 1]] = std::max<uint64_t>(ext[rank[2 * p + 1]], (uint64_t)m[2 * q + 1] + 1); }
    std::vector<uint64_t> base(V + 1, 0);
    for (size_t v = 0; v < V; ++v) base[v + 1] = base[v] + ext[v];
    if (base[V] > (1ull << 28)) { fprintf(stderr, "more slots than R3DM_TRACKS_MAX_SLOTS: the library refuses this graph too\n"); return 3; }
    const uint32_t N = (uint32_t)base[V];
    par.resize(N); for (uint32_t i = 0; i < N; ++i) par[i] = i;
    std::vector<uint8_t> touched(N, 0);
    std::vector<uint32_t> ma(M);
    for (uint64_t p = 0; p < P; ++p) for (uint64_t q = off[p]; q < off[p + 1]; ++q) {
        uint32_t a = (uint32_t)(base[rank[2 * p]] + m[2 * q]), b = (uint32_t)(base[rank[2 * p + 1]] + m[2 * q + 1]);
        ma[q] = a; touched[a] = touched[b] = 1;
        a = find(a); b = find(b);
        if (a != b) { if (a < b) par[b] = a; else par[a] = b; }
    }
    std::vector<uint64_t> nodes;
    for (uint32_t i = 0; i < N; ++i) if (touched[i]) nodes.push_back((uint64_t)find(i) << 32 | i);
    std::sort(nodes.begin(), nodes.end());
    std::vector<uint8_t> surv(N, 0);
    std::vector<uint32_t> obs; std::vector<uint64_t> toff{0};
    uint64_t n_comp = 0, n_conf = 0, n_short = 0;
    for (size_t b = 0; b < nodes.size();) {
        size_t e = b + 1; bool conf = false;
        while (e < nodes.size() && nodes[e] >> 32 == nodes[b] >> 32) {
            const uint64_t s0 = (uint32_t)nodes[e - 1], s1 = (uint32_t)nodes[e];
            if (std::upper_bound(base.begin(), base.end(), s0) == std::upper_bound(base.begin(), base.end(), s1)) conf = true;
            ++e;
        }
        ++n_comp;
        if (conf) ++n_conf; else if (e - b < min_length) ++n_short;
        else { surv[nodes[b] >> 32] = 1; for (size_t k = b; k < e; ++k) obs.push_back((uint32_t)nodes[k]); toff.push_back(obs.size()); }
        b = e;
    }
    uint64_t kept = 0;
    for (uint64_t q = 0; q < M; ++q) kept += surv[find(ma[q])];
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    printf("%.3f %zu %llu %llu %llu %zu %zu %llu\n", ms, nodes.size(), (unsigned long long)n_comp, (unsigned long long)n_conf, (unsigned long long)n_short,
           toff.size() - 1, obs.size(), (unsigned long long)kept);
    return 0;
}
"""


PHASES = ("extents", "link_flatten_select_nodes", "sort_mark_classify_select_observations", "emit_offsets_keep")


def star_graph(n_views):
    """(pairs, offsets, matches) of one conflicting star of 2 n_views + 1 nodes: feature 0 of view 0 matched to features 0 and 1 of views
    k = 1 .. n_views.  The indices are dense on purpose: a node's slot is base[view] + feature, so the sum over the views of (largest
    feature index + 1) must stay within R3DM_TRACKS_MAX_SLOTS (2^28) -- the star of tests/test_gpu_tracks.py, features 2k and 2k + 1 of
    view k, needs n_views^2 slots and cannot be scaled to 100 k nodes."""
    k = np.arange(1, n_views + 1, dtype=np.uint32)
    pairs = np.stack([np.zeros_like(k), k], 1)
    matches = np.stack([np.zeros(2 * n_views, np.uint32), np.tile(np.array([0, 1], np.uint32), n_views)], 1)
    return pairs, np.arange(0, 2 * n_views + 1, 2, dtype=np.uint64), matches


def host_baseline(tmp, exe, g, min_length, reps):
    path = os.path.join(tmp, "graph.bin")
    with open(path, "wb") as f:
        np.array([g.num_pairs, g.num_matches], np.uint64).tofile(f)
        g.pairs.tofile(f); g.offsets.tofile(f); g.matches.tofile(f)
    runs = [subprocess.run([exe, path, str(min_length)], capture_output=True, text=True, check=True).stdout.split() for _ in range(reps)]
    ms = [float(r[0]) for r in runs]
    names = ("n_nodes", "n_components", "n_conflicting", "n_short", "n_tracks", "n_observations", "n_matches_kept")
    return float(np.median(ms)), min(ms), max(ms), dict(zip(names, map(int, runs[0][1:])))


def device_leg(c, g, min_length, reps, want_graph):
    c.build_tracks(g, min_length, want_graph=want_graph)                  # warm-up: the work buffers are made and grown
    runs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = c.build_tracks(g, min_length, want_graph=want_graph)
        wall = (time.perf_counter() - t0) * 1e3
        t = r[0] if want_graph else r
        s = t.stats.as_dict()
        runs.append((s["ms_kernels"], s["ms_wall"], wall, s, t.phase_ms))
    med = lambda k: round(float(np.median([r[k] for r in runs])), 3)
    s = runs[0][3]
    out = dict(ms_kernels=med(0), ms_wall=med(1), ms_wall_python=med(2), ms_kernels_min=round(min(r[0] for r in runs), 3),
               ms_kernels_max=round(max(r[0] for r in runs), 3))
    out["ms_phases"] = dict(zip(PHASES, np.round(np.median([r[4] for r in runs], axis=0), 3).tolist()))
    out["edges_per_s"] = round(s["n_matches"] / (out["ms_kernels"] * 1e-3)); out["nodes_per_s"] = round(s["n_nodes"] / (out["ms_kernels"] * 1e-3))
    out.update({k: v for k, v in s.items() if not k.startswith("ms_")})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--feat", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-length", type=int, default=2)
    ap.add_argument("--star-views", type=int, default=50000)
    ap.add_argument("--no-host-baseline", action="store_true")
    a = ap.parse_args()
    import torch
    from regard3d_amd import api, synth

    tmp = tempfile.mkdtemp(prefix="tracks_perf_")
    exe = None
    if not a.no_host_baseline:
        src = os.path.join(tmp, "host_tracks.cpp"); exe = os.path.join(tmp, "host_tracks")
        open(src, "w").write(HOST_CPP)
        subprocess.check_call(["g++", "-O2", "-std=c++17", src, "-o", exe])

    descs, xys, _ = synth.make_scene_torch(a.images, a.feat, seed=2002, device="cuda", kind="sift")
    torch.cuda.synchronize()
    c = api.Context(0)
    c.set_device_graphs(True)
    c.set_images(list(range(a.images)), [descs[i] for i in range(a.images)], [xys[i] for i in range(a.images)], synth.WIDTH, synth.HEIGHT, wait=True)
    pairs = np.array([(i, j) for i in range(a.images) for j in range(i + 1, a.images)], np.uint32)
    gf = c.filter_F(c.match_pairs(pairs, 0.6, True), 4.0, 2048, seed=5489)
    copy = api.Graph.from_csr(gf.pairs, gf.offsets, gf.matches)
    assert gf.on_device == 0 and copy.on_device == -1
    what = f"C2 F-filtered graph: {a.images} views x {a.feat} rows, {gf.num_pairs} pairs, {gf.num_matches} matches"
    for name, g in (("mirrored", gf), ("uploaded", copy)):
        for want_graph in (False, True):
            print(json.dumps(dict(graph=what, path=name, kept_graph=want_graph, min_length=a.min_length,
                                  **device_leg(c, g, a.min_length, a.reps, want_graph))), flush=True)
    if exe:
        med, lo, hi, counts = host_baseline(tmp, exe, copy, a.min_length, max(3, a.reps))
        print(json.dumps(dict(graph=what, path="host (one thread, g++ -O2)", min_length=a.min_length, ms=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3),
                              edges_per_s=round(gf.num_matches / (med * 1e-3)), **counts)), flush=True)

    # one conflicting star
    k = np.arange(1, a.star_views + 1)
    star = api.Graph.from_csr(*star_graph(a.star_views))
    c.set_device_graphs(False)
    what = f"star: one conflicting component of {2 * len(k) + 1} nodes, {len(k)} pairs, {2 * len(k)} matches"
    print(json.dumps(dict(graph=what, path="uploaded", kept_graph=True, min_length=2, **device_leg(c, star, 2, a.reps, True))), flush=True)
    if exe:
        med, lo, hi, counts = host_baseline(tmp, exe, star, 2, max(3, a.reps))
        print(json.dumps(dict(graph=what, path="host (one thread, g++ -O2)", min_length=2, ms=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3), **counts)), flush=True)
    c.close()


if __name__ == "__main__":
    main()
