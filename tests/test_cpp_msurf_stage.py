"""The M-SURF-64 descriptor arm through the C++ facade (include/r3d_compute_matches.hpp) from a small host program
(tests/cpp/msurf_stage_main.cpp): setRegionsType(R3DM_F32, 64) + computeMatches from pixels, with direct registration on and off, against
the CPU restatement of the chain (tests/msurf_cases.py).  The program's compile-and-link part runs without a GPU."""
import os
import subprocess

import numpy as np
import pytest

import msurf_cases as S
from stage_cases import _check_filter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def stage_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp_msurf_stage") / "msurf_stage_main")
    lib = os.path.join(ROOT, "regard3d_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fopenmp", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "msurf_stage_main.cpp"), "-o", out,
                           "-L" + lib, "-lr3dm", "-Wl,-rpath," + lib])
    return out


def test_msurf_stage_program_compiles_and_links(stage_exe):
    assert subprocess.run([stage_exe], capture_output=True).returncode == 2            # usage; the program loaded libr3dm.so


@pytest.mark.gpu
def test_facade_runs_the_msurf_arm_from_pixels(stage_exe, oracle, tmp_path):
    ims = S.stage_images()
    np.stack(ims).astype(np.float32).tofile(str(tmp_path / "gray.f32"))
    refs, descs, xys, pairs, counts, matches = S.oracle_stage(ims)
    W = np.full(4, 320, np.uint32); H = np.full(4, 240, np.uint32)
    oc, om = oracle.filter_F_collection(xys, W, H, pairs, counts, matches, 4.0, 2048, 5489)
    blobs = []
    for direct in (1, 0):
        d = tmp_path / f"direct{direct}"; d.mkdir()
        r = subprocess.run([stage_exe, str(d), "4", "320", "240", str(tmp_path / "gray.f32"), repr(S.STAGE_RATIO), str(direct)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        assert list(map(int, r.stdout.split())) == [int((counts > 0).sum()), int((oc > 0).sum()), 4, 3]
        for k in range(4):
            n, rows = S.desc_file(str(d / f"img{k:03d}.desc"))
            assert n == len(descs[k]) and S.same_rows(rows, descs[k]), k
        p, c, m = oracle.load_matches(str(d / "matches.putative.txt"))
        assert np.array_equal(p, pairs[counts > 0]) and np.array_equal(c, counts[counts > 0]) and np.array_equal(m, matches)
        assert _check_filter(oracle, str(d / "matches.f.txt"), pairs, oc, om) >= 3
        assert not os.path.exists(str(d / "none"))
        blobs.append([open(str(d / name), "rb").read() for name in ("matches.putative.txt", "matches.f.txt")])
    assert blobs[0] == blobs[1]
