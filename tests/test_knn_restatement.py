"""The k-NN restatement (knn_restatement.py) against the oracle's 2-NN, the reference-built 3-NN fixture and -- where oracle/_ref
is built -- the live reference brute force; and the two new ABI entries without a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import knn_restatement as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _two_columns(oracle, A, B, binary=False):
    i2, d2 = R.knn(A, B, 2, binary=binary)
    oi, od = oracle.knn2(A, B, binary=binary)
    assert np.array_equal(i2, oi)
    assert np.array_equal(d2, od.astype(np.float32))


def test_two_columns_liop(oracle):
    A, B, _, _ = R.liop_fixture(GOLD)
    i9, d9 = R.liop_knn9(GOLD)
    oi, od = oracle.knn2(A, B)
    assert np.array_equal(i9[:, :2], oi) and np.array_equal(d9[:, :2], od)


def test_two_columns_sift_int(oracle):
    z = np.load(os.path.join(GOLD, "knn2_sift_int.npz"))
    _two_columns(oracle, z["dataset"], z["query"])
    _two_columns(oracle, z["dataset"].astype(np.float32), z["query"].astype(np.float32))


def test_two_columns_random_f32_tail(oracle):
    rng = np.random.default_rng(37)
    _two_columns(oracle, rng.standard_normal((203, 37)).astype(np.float32), rng.standard_normal((57, 37)).astype(np.float32))


def test_two_columns_binary_61(oracle):
    rng = np.random.default_rng(61)
    a = rng.integers(0, 256, (300, 61), dtype=np.uint8); b = rng.integers(0, 256, (90, 61), dtype=np.uint8)
    b[:20] = a[:20] ^ (rng.random((20, 61)) < 0.05).astype(np.uint8)
    _two_columns(oracle, a, b, binary=True)


def test_reference_built_liop_3nn():
    _, _, ri, rd = R.liop_fixture(GOLD)
    i9, d9 = R.liop_knn9(GOLD)
    R.check_against_reference(i9[:, :3], d9[:, :3], ri, rd, d9[:, 3], 144, "LIOP fixture, k = 3")


def _ref_or_skip(oracle):
    if oracle.ref_lib() is None:
        pytest.skip("oracle/_ref/libref_hnsw.so is not built here (no reference tree): the committed-fixture check above still ran")


def test_live_reference_liop_8nn(oracle):
    _ref_or_skip(oracle)
    A, B, _, _ = R.liop_fixture(GOLD)
    li, ld = oracle.ref_knn(A, B, 9)
    i9, d9 = R.liop_knn9(GOLD)
    R.check_against_reference(i9[:, :8], d9[:, :8], li, ld, ld[:, 8], 144, "LIOP live reference, k = 8")


def test_live_reference_sift_u8_8nn(oracle):
    _ref_or_skip(oracle)
    z = np.load(os.path.join(GOLD, "knn2_c2_fullsize.npz"))
    D, Q = z["dataset"], z["query"][:512]
    li, ld = oracle.ref_knn(D.astype(np.float32), Q.astype(np.float32), 9)
    i8, d8 = R.knn(D, Q, 8)
    R.check_against_reference(i8, d8, li, ld, ld[:, 8], 128, "SIFT u8 live reference, k = 8", exact=True)


def test_abi_exports_and_null_context():
    """fails on a library without the k-NN entries"""
    from regard3d_amd import api
    L = api.load_library()
    assert "r3dm_knn" in api.EXPORTS and "r3dm_index_knn" in api.EXPORTS
    assert hasattr(L, "r3dm_knn") and hasattr(L, "r3dm_index_knn")
    a = np.zeros((8, 128), np.float32); idx = np.zeros((8, 3), np.int32); dist = np.zeros((8, 3), np.float32)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    ERR_INVALID = -1
    assert L.r3dm_knn(None, p(a), 8, p(a), 8, 128, api.F32, 3, p(idx), p(dist)) == ERR_INVALID
    assert L.r3dm_index_knn(None, None, p(a), 8, 3, p(idx), p(dist)) == ERR_INVALID
    assert api.KNN_MAX == 8
