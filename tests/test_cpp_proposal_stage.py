"""Pair proposal through the C++ facade (include/r3d_compute_matches.hpp) from a small host program (tests/cpp/proposal_stage_main.cpp):
R3DComputeMatches::setPairProposal + computeMatches over a directory of feature files, against the switch-off run restricted to the
pairs r3dm_propose_pairs returns.  The program's compile-and-link part runs without a GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import vocab_cases as VC
from regard3d_amd import api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def proposal_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp_proposal_stage") / "proposal_stage_main")
    lib = os.path.join(ROOT, "regard3d_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fopenmp", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "proposal_stage_main.cpp"), "-o", out, "-L" + lib, "-lr3dm", "-Wl,-rpath," + lib])
    return out



def test_proposal_stage_program_compiles_and_links(proposal_exe):
    assert subprocess.run([proposal_exe], capture_output=True).returncode == 2         # usage; the program loaded libr3dm.so


@pytest.mark.gpu
def test_cpp_host_through_set_pair_proposal(oracle, proposal_exe, tmp_path):
    """R3DComputeMatches::setPairProposal(on, 48, 1) over a directory of feature files: with top_k 1 most pairs are left out, and the
    files are the switch-off files restricted to what propose_pairs returns"""
    sc = synth.make_scene(8, 120, "liop", seed=61)
    ids = [5, 1, 7, 3, 11, 9, 2, 4]
    dirs = {k: tmp_path / k for k in ("off", "on")}
    for d in dirs.values():
        d.mkdir()
        for k in range(8):
            name = f"img{k:03d}"
            desc = sc.descs[k]
            assert oracle.lib().orc_save_desc(str(d / (name + ".desc")).encode(), ctypes.c_uint64(desc.shape[0]), ctypes.c_size_t(144 * 4),
                                              desc.ctypes.data_as(ctypes.c_void_p)) == 0
            with open(d / (name + ".feat"), "w") as f:
                for x, y in sc.xys[k]:
                    f.write("%.9g %.9g 1 0\n" % (x, y))
    id_args = [str(i) for i in ids]
    out = {}
    for k, flag in (("off", "0"), ("on", "1")):
        r = subprocess.run([proposal_exe, str(dirs[k]), flag, "48", "1"] + id_args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        out[k] = [int(x) for x in r.stdout.split()]
    c = api.Context(0)
    try:
        for i, d in zip(ids, sc.descs):
            c.set_image(i, d)
        v = c.vocab_sample(sorted(ids), 48)
        keep = c.propose_pairs(v, sorted(ids), 1)
        v.close()
    finally:
        c.close()
    assert out["off"][2] == 28 and out["on"][2] == len(keep) and 4 <= len(keep) <= 8
    VC.assert_files_restricted(oracle, str(dirs["off"]), str(dirs["on"]), keep)
    assert out["on"][0] <= len(keep) and out["on"][0] < out["off"][0]
