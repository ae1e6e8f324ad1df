"""Binary rows on the graph matcher from a C++ host (tests/cpp/mldb_kgraph_main.cpp): the plugin class with a Hamming metric, and the
stage (R3DComputeMatches with setRegionsType(R3DM_BIN, 61)) on the approximate arms -- literally, and under the default policy, where
computeMatches used to return false for binary regions."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ann_bits_cases as cases
import mldb_arm_cases as M
from regard3d_amd import api

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "mldb_kgraph_main")
    lib = os.path.join(ROOT, "regard3d_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fopenmp", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "mldb_kgraph_main.cpp"), "-o", out, "-L" + lib, "-lr3dm", "-Wl,-rpath," + lib])
    return out


def _records(path):
    raw = np.fromfile(path, np.uint32).reshape(-1, 3)
    return raw[:, 0].copy(), raw[:, 1].copy(), raw[:, 2].copy().view(np.float32)


def test_plugin_class_with_a_hamming_metric(exe, tmp_path):
    A, B = cases.views("rand", 2000, 333, 64)
    A.tofile(str(tmp_path / "rows.u8")); B.tofile(str(tmp_path / "q.u8"))
    out = str(tmp_path / "out")
    r = subprocess.run([exe, "plugin", str(tmp_path / "rows.u8"), "2000", "64", str(tmp_path / "q.u8"), "333", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    kp = api.KGraphParams.preset(3)                                         # the class's default parameters, pair ids (0, 1)
    c = api.Context(0)
    c.set_kgraph_hamming(True)
    index = c.index_create(A, binary=True)
    try:
        for NN in (1, 2, 5):
            q, row, d = _records(out + f".h{NN}.bin")
            idx, dist = index.kgraph_knn(c, B, kp, (0, 1), NN)
            assert np.array_equal(q, np.repeat(np.arange(333, dtype=np.uint32), NN))
            assert np.array_equal(row, idx.reshape(-1).astype(np.uint32)) and np.array_equal(d, dist.reshape(-1))
            assert (idx >= 0).all()
    finally:
        index.close()
        c.close()
    # the default metric: the same bytes as VALUES under squared L2 (R3DM_U8), not as bits
    q, row, d = _records(out + ".l2.bin")
    assert len(q) == 2 * 333 and (row < 2000).all()
    l2 = ((A[row].astype(np.int64) - B[q].astype(np.int64)) ** 2).sum(1)
    ham = cases.bits(A[row] ^ B[q]).sum(1)
    assert np.array_equal(d, l2.astype(np.float32)) and not np.array_equal(d, ham.astype(np.float32))


@pytest.fixture(scope="module")
def stage_inputs(tmp_path_factory):
    ims = M.stage_images()
    path = str(tmp_path_factory.mktemp("stage_in") / "gray.f32")
    np.stack(ims).astype(np.float32).tofile(path)
    c = api.Context(0)
    try:
        c.set_kgraph_hamming(True)
        descs = []
        for k, im in enumerate(ims):
            kps, desc = c.detect_akaze_mldb(im, M.THR)
            c.set_image(k, desc, M.g6(kps[:, :2]), 320, 240, binary=True)
            descs.append(desc)
        i, j = np.triu_indices(len(ims), k=1)
        pairs = np.stack([i, j], axis=1).astype(np.uint32)
        graphs = {}
        for arm in (1, 2, 3):
            kp = api.KGraphParams()
            assert c._L.r3dm_ann_params_for_algorithm(arm, C.addressof(kp)) == 0
            g = c.match_pairs_kgraph(pairs, M.STAGE_RATIO, kp)
            graphs[arm] = (g.pairs.copy(), np.diff(g.offsets.astype(np.int64)), g.matches.copy())
        exhaustive = c.match_pairs(pairs, M.STAGE_RATIO, False)
        graphs["exhaustive"] = (exhaustive.pairs.copy(), np.diff(exhaustive.offsets.astype(np.int64)), exhaustive.matches.copy())
    finally:
        c.close()
    return path, graphs


def _run_stage(exe, d, gray, arm, as_requested):
    r = subprocess.run([exe, "stage", str(d), "4", "320", "240", gray, str(M.STAGE_RATIO), str(arm), str(int(as_requested))],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    n_pairs, exhaustive = map(int, r.stdout.split())
    return n_pairs, exhaustive


@pytest.mark.parametrize("arm", [1, 2, 3])
def test_stage_runs_the_literal_arms_on_the_hamming_graph_matcher(exe, oracle, stage_inputs, tmp_path, arm):
    gray, graphs = stage_inputs
    n_pairs, exhaustive = _run_stage(exe, tmp_path, gray, arm, True)
    p, c, m = oracle.load_matches(str(tmp_path / "matches.putative.txt"))
    ep, ec, em = graphs[arm]
    assert exhaustive == 0 and n_pairs == len(ep) and len(em) > 0
    assert np.array_equal(p, ep) and np.array_equal(c, ec) and np.array_equal(m, em)


def test_stage_serves_the_default_arm_for_binary_regions(exe, oracle, stage_inputs, tmp_path):
    """matchingAlgorithm 0 (the GUI's default) under the default policy: served -- it failed before -- by whichever matcher
    r3dm_exhaustive_is_faster names, and the report says which"""
    gray, graphs = stage_inputs
    n_pairs, exhaustive = _run_stage(exe, tmp_path, gray, 0, False)
    p, c, m = oracle.load_matches(str(tmp_path / "matches.putative.txt"))
    ep, ec, em = graphs["exhaustive" if exhaustive else 3]                   # (arm 0 maps to the precise preset, as arm 3)
    assert exhaustive in (0, 1) and n_pairs == len(ep)
    assert np.array_equal(p, ep) and np.array_equal(c, ec) and np.array_equal(m, em)
