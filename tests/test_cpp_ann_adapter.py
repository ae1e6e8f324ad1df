"""The three approximate matcher plugins (include/r3dm_ann_matchers.hpp): a small C++ host program (tests/cpp/ann_adapter_main.cpp)
against the C ABI's one-shot entries on the same rows."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ann_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp_ann") / "ann_adapter_main")
    lib = os.path.join(ROOT, "regard3d_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fopenmp", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "ann_adapter_main.cpp"), "-o", out,
                           "-L" + lib, "-lr3dm", "-Wl,-rpath," + lib])
    return out


def test_ann_adapter_compiles_and_links(ann_exe):
    assert subprocess.run([ann_exe], capture_output=True).returncode == 2       # usage; the program loaded libr3dm.so


@pytest.mark.gpu
def test_ann_adapters_against_the_c_abi(ann_exe, ctx, tmp_path):
    from regard3d_amd import api
    from test_gpu_ann_knn import _mrpt_views
    a, b = _mrpt_views()                                       # 600 x 300 SIFT rows; at votes 4 some queries are dropped at NN = 8
    a.tofile(tmp_path / "a.f32"); b.tofile(tmp_path / "b.f32")
    loops = 16
    r = subprocess.run([ann_exe, str(tmp_path / "a.f32"), str(len(a)), str(tmp_path / "b.f32"), str(len(b)), str(a.shape[1]), str(tmp_path / "out"), str(loops)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    hp = api.HnswParams.preset("fast")
    mp = api.MrptParams.preset()
    want = {"kgraph": lambda k: ctx.kgraph_knn(a, b, api.KGraphParams.preset("default"), (3, 9), k),
            "hnsw": lambda k: ctx.hnsw_knn(a, b, hp, k),
            "mrpt": lambda k: ctx.mrpt_knn(a, b, api.MrptParams(mp.n_trees, mp.depth, 4, mp.density, mp.seed), k)}
    for row, arm in enumerate(("kgraph", "hnsw", "mrpt")):
        refused9, refused_rows, staged_loop, same = map(int, lines[row].split())
        assert refused9 == 1 and refused_rows == 1, arm        # NN = 9 and NN > nbRows return false
        assert same == 1, arm                                  # every search of the OpenMP loop gave the first one's answer
        assert staged_loop == loops, arm                       # ... and uploaded its queries only: dataset and structure were built once
        for nn in (2, 8):
            got = np.loadtxt(str(tmp_path / f"out.{arm}.nn{nn}")).reshape(-1, 3)
            wi, wd = want[arm](nn)
            keep = np.ones(len(b), bool) if arm != "mrpt" else (wi[:, 0] >= 0)          # a dropped MRPT query contributes no entries
            assert arm != "mrpt" or nn != 8 or (0 < keep.sum() < len(b))
            assert np.array_equal(got[:, 0].astype(int), np.repeat(np.arange(len(b))[keep], nn)), (arm, nn)      # IndMatch(i_ = query row, ..)
            assert np.array_equal(got[:, 1].astype(np.int32), wi[keep].reshape(-1)), (arm, nn)
            assert np.array_equal(got[:, 2].astype(np.float32).view(np.uint32), wd[keep].reshape(-1).view(np.uint32)), (arm, nn)
    assert int(lines[3]) == 1                                  # the autotune mode is refused
