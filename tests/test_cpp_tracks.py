"""R3DComputeMatches::buildTracks (include/r3d_compute_matches.hpp) from a small C++ host program (tests/cpp/tracks_main.cpp) on a
PairWiseMatches map read from a match file, against the plain-Python restatement."""
import os
import subprocess

import numpy as np
import pytest

import tracks_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tracks_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp_tracks") / "tracks_main")
    lib = os.path.join(ROOT, "regard3d_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fopenmp", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "tracks_main.cpp"), "-o", out,
                           "-L" + lib, "-lr3dm", "-Wl,-rpath," + lib])
    return out


def _write_map(path, pairs, offsets, matches):
    with open(path, "w") as f:
        for p in range(len(pairs)):
            b, e = int(offsets[p]), int(offsets[p + 1])
            f.write(f"{pairs[p, 0]} {pairs[p, 1]}\n{e - b}\n")
            f.writelines(f"{i} {j}\n" for i, j in matches[b:e].tolist())


def test_tracks_program_compiles_and_links(tracks_exe):
    assert subprocess.run([tracks_exe], capture_output=True).returncode == 2       # usage; the program loaded libr3dm.so


@pytest.mark.gpu
def test_build_tracks_on_a_map_against_restatement(tracks_exe, tmp_path):
    g = R.world_graph(**R.MID_WORLD)                            # (its pairs are unique and ascending: the map's order)
    offs, obs, st, kept, _ = R.build_tracks(*g, 3)
    assert st["n_conflicting"] >= 50 and st["n_short"] > 0 and st["n_tracks"] > 500
    _write_map(tmp_path / "in.txt", *g)
    r = subprocess.run([tracks_exe, str(tmp_path / "in.txt"), "3", str(tmp_path / "out")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names = ["n_nodes", "n_components", "n_conflicting", "n_short", "n_tracks", "n_observations", "n_matches_kept", "longest", "largest_component"]
    assert dict(zip(names, map(int, r.stdout.split()))) == {n: st[n] for n in names}
    assert np.array_equal(np.loadtxt(tmp_path / "out.offsets", dtype=np.uint64), offs)
    assert np.array_equal(np.loadtxt(tmp_path / "out.obs", dtype=np.uint32).reshape(-1, 2), obs)
    _write_map(tmp_path / "exp.kept", *R.kept_graph(*g, kept))
    assert open(tmp_path / "out.kept").read() == open(tmp_path / "exp.kept").read()
