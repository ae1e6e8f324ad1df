"""CPU: the float models of the graph matcher, run on unpacked 0 / 1 rows, are the Hamming models -- shown on the inputs the GPU tests
of the Hamming graph matcher use (ann_bits_cases.py).  These pass without the feature: they are the footing of test_gpu_ann_bits.py."""
import numpy as np
import pytest

import ann_bits_cases as cases


def test_ratios_are_exact_squares():
    for R, r in cases.RATIOS.items():
        assert np.float32(r) * np.float32(r) == np.float32(R) and float(np.float32(R)) == R and float(np.float32(r)) == r


@pytest.mark.parametrize("kind,nI,nJ,nbytes", [("akaze", 1500, 1200, 61), ("rand", 700, 500, 32), ("rand", 300, 300, 29), ("ties", 600, 200, 32)])
def test_l2_on_unpacked_rows_is_hamming(oracle, kind, nI, nJ, nbytes):
    A, B = cases.views(kind, nI, nJ, nbytes)
    bi, bd = oracle.knn2(A, B, binary=True)
    fi, fd = oracle.knn2(cases.bits(A), cases.bits(B))
    assert np.array_equal(bi, fi) and np.array_equal(bd.astype(np.float32), fd)
    if kind == "ties":
        assert (bd[:, 0] == bd[:, 1]).sum() >= 100          # ties included: both models break them by row


@pytest.mark.parametrize("R", sorted(cases.RATIOS))
def test_collection_on_unpacked_rows_is_the_hamming_collection(oracle, R):
    descs, xys, pairs = cases.scene()
    bc, bm = oracle.match_collection(descs, xys, pairs, R, squared=False, binary=True)
    fc, fm = oracle.match_collection([cases.bits(d) for d in descs], xys, pairs, cases.RATIOS[R], squared=True)
    assert np.array_equal(bc, fc) and np.array_equal(bm, fm) and bc.sum() > 500


def test_tie_heavy_set_is_tie_heavy(oracle):
    A, B = cases.tie_heavy()
    g = oracle.kgraph_build_exact(cases.bits(A), K=20, cap=64)
    off, _, dist = g.csr()
    deg = np.diff(off.astype(np.int64))
    assert len(np.unique(dist)) == 22
    assert deg.min() == 20 and deg.max() == 64           # from the forward list alone up to the adjacency cap
    _, d, _ = g.knn2(cases.bits(B), P=10, S=10, seed=cases.SEARCH_SEED, I=cases.SEARCH_PAIR[0], J=cases.SEARCH_PAIR[1], min_rows=128)
    assert (d[:, 0] == d[:, 1]).sum() >= 100             # queries whose two best are tied
