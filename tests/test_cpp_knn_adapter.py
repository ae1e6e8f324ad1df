"""The matcher-plugin slot (include/r3dm_array_matcher.hpp) asked for more than two neighbours: a small C++ host program
(tests/cpp/knn_adapter_main.cpp) against the numpy restatement."""
import os
import subprocess

import numpy as np
import pytest

import knn_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def knn_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp_knn") / "knn_adapter_main")
    lib = os.path.join(ROOT, "regard3d_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fopenmp", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "knn_adapter_main.cpp"), "-o", out,
                           "-L" + lib, "-lr3dm", "-Wl,-rpath," + lib])
    return out


def test_knn_adapter_compiles_and_links(knn_exe):
    assert subprocess.run([knn_exe], capture_output=True).returncode == 2       # usage; the program loaded libr3dm.so


@pytest.mark.gpu
def test_knn_adapter_against_restatement(knn_exe, tmp_path):
    rng = np.random.default_rng(144)
    a = rng.standard_normal((907, 144)).astype(np.float32); b = rng.standard_normal((211, 144)).astype(np.float32)
    a.tofile(tmp_path / "a.f32"); b.tofile(tmp_path / "b.f32")
    loops = 24
    r = subprocess.run([knn_exe, str(tmp_path / "a.f32"), "907", str(tmp_path / "b.f32"), "211", "144", str(tmp_path / "out"), str(loops)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    refused9, refused_rows, staged_before, staged_loop, same = map(int, r.stdout.split())
    assert refused9 == 1 and refused_rows == 1                 # NN = 9 and NN > nbRows return false
    i8, d8 = R.knn(a, b, 8)
    for nn in (3, 8):
        got = np.loadtxt(str(tmp_path / f"out.nn{nn}"))
        assert np.array_equal(got[:, 0].astype(int), np.arange(211))        # IndMatch(i_ = query row, j_ = dataset row)
        assert np.array_equal(got[:, 1::2].astype(np.int32), i8[:, :nn])
        assert np.array_equal(got[:, 2::2].astype(np.float32), d8[:, :nn])
    assert same == 1                                           # every search of the OpenMP loop gave the first one's answer
    assert staged_loop == loops                                # ... and uploaded its queries only: the dataset was staged once, by Build
