"""Trained, idf-weighted pair proposal through the stage: from a small C++ host (tests/cpp/proposal_trained_stage_main.cpp:
R3DComputeMatches::setPairProposal + setPairProposalTraining + computeMatches over a directory of feature files) and through the flag
R3DM_STAGE_PROPOSAL_TRAINED of r3dm_compute_matches_dir_flags, against the switch-off run restricted to the pairs the numpy restatement
proposes from the trained, idf-weighted vocabulary.  The program's compile-and-link part runs without a GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import vocab_cases as VC
import vocab_restatement as R
import vocab_train_restatement as TR
from regard3d_amd import api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [5, 1, 7, 3, 11, 9, 2, 4]


@pytest.fixture(scope="module")
def trained_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp_proposal_trained_stage") / "proposal_trained_stage_main")
    lib = os.path.join(ROOT, "regard3d_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fopenmp", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "proposal_trained_stage_main.cpp"), "-o", out, "-L" + lib, "-lr3dm", "-Wl,-rpath," + lib])
    return out


def test_program_compiles_and_links_and_the_flag_is_the_headers(trained_exe):
    assert subprocess.run([trained_exe], capture_output=True).returncode == 2            # usage; the program loaded libr3dm.so
    hpp = open(os.path.join(ROOT, "include", "r3d_compute_matches.hpp")).read()
    assert int(re.search(r"#define\s+R3DM_STAGE_PROPOSAL_TRAINED\s+(\d+)u", hpp).group(1)) == api.STAGE_PROPOSAL_TRAINED == 16384
    assert "void setPairProposalTraining(uint32_t max_iterations, bool idf);" in hpp


def _write(oracle, d, sc):
    for k in range(len(sc.descs)):
        name = f"img{k:03d}"
        desc = sc.descs[k]
        assert oracle.lib().orc_save_desc(str(d / (name + ".desc")).encode(), ctypes.c_uint64(desc.shape[0]), ctypes.c_size_t(144 * 4),
                                          desc.ctypes.data_as(ctypes.c_void_p)) == 0
        with open(d / (name + ".feat"), "w") as f:
            for x, y in sc.xys[k]:
                f.write("%.9g %.9g 1 0\n" % (x, y))


def _restated_pairs(oracle, sc, n_words, top_k, max_iterations, idf):
    """the stage's rule: views in view-id order, a sampled vocabulary trained on them, idf-weighted scores"""
    order = np.argsort(IDS)
    ids = [IDS[k] for k in order]
    descs = [sc.descs[k] for k in order]
    words = R.sample_vocab(descs, n_words)
    if max_iterations:
        words = TR.train(oracle, words, descs, max_iterations)["words"]
    hist = R.signatures(oracle, words, descs)
    ns = [len(d) for d in descs]
    return TR.propose_idf(hist, ns, ids, top_k)["pairs"] if idf else R.propose(R.scores(hist), ns, ids, top_k)


@pytest.mark.gpu
def test_cpp_host_through_set_pair_proposal_training(oracle, trained_exe, tmp_path):
    sc = synth.make_scene(8, 120, "liop", seed=61)
    dirs = {k: tmp_path / k for k in ("off", "on", "no_proposal")}
    for d in dirs.values():
        d.mkdir()
        _write(oracle, d, sc)
    id_args = [str(i) for i in IDS]
    out = {}
    for k, args in (("off", ["0", "48", "1", "0", "0"]), ("on", ["1", "48", "1", "4", "1"]), ("no_proposal", ["0", "48", "1", "4", "1"])):
        r = subprocess.run([trained_exe, str(dirs[k])] + args + id_args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        out[k] = [int(x) for x in r.stdout.split()]
    keep = _restated_pairs(oracle, sc, 48, 1, 4, True)
    plain = _restated_pairs(oracle, sc, 48, 1, 0, False)
    assert not np.array_equal(keep, plain)                                                # training + idf propose other pairs here
    assert out["off"][2] == 28 and out["on"][2] == len(keep) and 4 <= len(keep) <= 8
    VC.assert_files_restricted(oracle, str(dirs["off"]), str(dirs["on"]), keep)
    # without setPairProposal the training switch has no effect
    assert out["no_proposal"] == out["off"]
    all_pairs = [(a, b) for a in sorted(IDS) for b in sorted(IDS) if a < b]
    VC.assert_files_restricted(oracle, str(dirs["off"]), str(dirs["no_proposal"]), all_pairs)


@pytest.mark.gpu
def test_stage_flag_through_the_directory_entry(oracle, tmp_path):
    """R3DM_STAGE_PAIR_PROPOSAL | R3DM_STAGE_PROPOSAL_TRAINED over 30 views of 40 rows: the stage's defaults are T / 2 = 600 sampled
    words, 10 updates, idf weights and top_k 20, which leave pairs out (0 < len(keep) < 435); the flag without
    R3DM_STAGE_PAIR_PROPOSAL changes nothing"""
    sc = synth.make_scene(30, 40, "liop", seed=62)
    ids = [3 * k + 1 for k in range(30)][::-1]
    views = [dict(id=ids[k], width=4000, height=3000, basename=f"img{k:03d}") for k in range(30)]
    dirs = {k: tmp_path / k for k in ("off", "on", "flag_alone")}
    for d in dirs.values():
        d.mkdir()
        _write(oracle, d, sc)
    api.compute_matches_dir(0, str(dirs["off"]), views, dim=144, dist_ratio=0.8)
    api.compute_matches_dir(0, str(dirs["on"]), views, dim=144, dist_ratio=0.8, proposal=True, proposal_trained=True)
    api.compute_matches_dir(0, str(dirs["flag_alone"]), views, dim=144, dist_ratio=0.8, proposal_trained=True)
    order = np.argsort(ids)
    sids = [ids[k] for k in order]
    descs = [sc.descs[k] for k in order]
    T = sum(len(d) for d in descs)
    words = TR.train(oracle, R.sample_vocab(descs, min(16384, T // 2)), descs, 10)["words"]
    keep = TR.propose_idf(R.signatures(oracle, words, descs), [len(d) for d in descs], sids, 20)["pairs"]
    assert 0 < len(keep) < 30 * 29 // 2
    VC.assert_files_restricted(oracle, str(dirs["off"]), str(dirs["on"]), keep)
    VC.assert_files_restricted(oracle, str(dirs["off"]), str(dirs["flag_alone"]), [(a, b) for a in sids for b in sids if a < b])
