"""The MLDB descriptor arm through the C++ facade (include/r3d_compute_matches.hpp) from a small host program
(tests/cpp/mldb_stage_main.cpp): setRegionsType(R3DM_BIN, 61) + computeMatches from pixels, with direct registration on and off, against
the CPU restatement of the chain.  The program's compile-and-link part runs without a GPU."""
import os
import subprocess

import numpy as np
import pytest

import mldb_arm_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def stage_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp_mldb_stage") / "mldb_stage_main")
    lib = os.path.join(ROOT, "regard3d_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fopenmp", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "mldb_stage_main.cpp"), "-o", out,
                           "-L" + lib, "-lr3dm", "-Wl,-rpath," + lib])
    return out


def test_mldb_stage_program_compiles_and_links(stage_exe):
    assert subprocess.run([stage_exe], capture_output=True).returncode == 2            # usage; the program loaded libr3dm.so


@pytest.mark.gpu
def test_facade_runs_the_mldb_arm_from_pixels(stage_exe, oracle, tmp_path):
    ims = M.stage_images()
    np.stack(ims).astype(np.float32).tofile(str(tmp_path / "gray.f32"))
    kps, descs, xys, pairs, counts, matches = M.oracle_stage(oracle, ims)
    W = np.full(4, 320, np.uint32); H = np.full(4, 240, np.uint32)
    oc, _ = oracle.filter_F_collection(xys, W, H, pairs, counts, matches, 4.0, 2048, 5489)
    blobs = []
    for direct in (1, 0):
        d = tmp_path / f"direct{direct}"; d.mkdir()
        r = subprocess.run([stage_exe, str(d), "4", "320", "240", str(tmp_path / "gray.f32"), repr(M.STAGE_RATIO), str(direct)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        assert list(map(int, r.stdout.split())) == [int((counts > 0).sum()), int((oc > 0).sum()), 4, 1]
        for k in range(4):
            n, rows = M.desc_file(str(d / f"img{k:03d}.desc"))
            assert n == len(kps[k]) and np.array_equal(rows, descs[k]), k
        p, c, m = oracle.load_matches(str(d / "matches.putative.txt"))
        assert np.array_equal(p, pairs[counts > 0]) and np.array_equal(c, counts[counts > 0]) and np.array_equal(m, matches)
        blobs.append([open(str(d / name), "rb").read() for name in ("matches.putative.txt", "matches.f.txt")])
    assert blobs[0] == blobs[1]
