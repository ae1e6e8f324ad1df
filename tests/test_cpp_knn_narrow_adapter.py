"""The matcher-plugin slot (include/r3dm_array_matcher.hpp) asked for more than two neighbours with setKnnNarrowTiles(true): a small
C++ host program (tests/cpp/knn_narrow_adapter_main.cpp) drives ArrayMatcher_r3dm<float> and <unsigned char> against files written
from the numpy restatement's inputs."""
import os
import subprocess

import numpy as np
import pytest

import knn_narrow_cases as N
import knn_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def narrow_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp_knn_narrow") / "knn_narrow_adapter_main")
    lib = os.path.join(ROOT, "regard3d_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fopenmp", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "knn_narrow_adapter_main.cpp"), "-o", out,
                           "-L" + lib, "-lr3dm", "-Wl,-rpath," + lib])
    return out


def test_narrow_adapter_compiles_and_links(narrow_exe):
    assert subprocess.run([narrow_exe], capture_output=True).returncode == 2    # usage; the program loaded libr3dm.so and found the setter


@pytest.mark.gpu
@pytest.mark.parametrize("scalar", ("f32", "u8"))
def test_narrow_adapter_against_restatement(narrow_exe, tmp_path, scalar):
    rng = np.random.default_rng(144)
    if scalar == "f32":                        # real-valued LIOP-length rows: the split planes
        a = rng.standard_normal((907, 144)).astype(np.float32); b = rng.standard_normal((211, 144)).astype(np.float32)
        assert N.expected_path(a, b) == "split"
    else:                                      # unsigned char bins with duplicated rows: the integer tiles
        a, b = N.u8_tied(907, 211, 128)
        assert N.expected_path(a, b) == "integer"
    n, dim = a.shape
    a.tofile(tmp_path / "a.bin"); b.tofile(tmp_path / "b.bin")
    loops = 24
    r = subprocess.run([narrow_exe, scalar, str(tmp_path / "a.bin"), str(n), str(tmp_path / "b.bin"), str(len(b)), str(dim),
                        str(tmp_path / "out"), str(loops)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    staged_loop, same, off_same = map(int, r.stdout.split())
    i8, d8 = R.knn(a, b, 8)
    for nn in (3, 8):
        got = np.loadtxt(str(tmp_path / f"out.nn{nn}"))
        assert np.array_equal(got[:, 0].astype(int), np.arange(len(b)))     # IndMatch(i_ = query row, j_ = dataset row)
        assert np.array_equal(got[:, 1::2].astype(np.int32), i8[:, :nn])
        assert np.array_equal(got[:, 2::2].astype(np.float32), d8[:, :nn])
    assert same == 1                                           # every search of the OpenMP loop gave the first one's answer
    assert staged_loop == loops                                # ... and uploaded its queries only: the dataset was staged once, by Build
    assert off_same == 1                                       # the f32 K-list kernel returns the same bytes
