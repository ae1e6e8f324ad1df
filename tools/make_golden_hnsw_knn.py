"""Generates tests/golden/hnsw_ref_knn.npz (run in the authoring container, needs /root/reference).

Pins the k-NN tail of the HNSW plugin path (r3dm_hnsw_knn_on_index, k = 1 .. 8) with the reference-built library: for the two scenes
and three presets of tests/golden/hnsw_ref_index.npz the reference's own hnswlib::HierarchicalNSW (oracle/_ref/libref_hnsw.so:
ref_hnsw_ann_l2, the same single-thread index as ref_hnsw_export) answers searchKnn(row, k) for the first 512 rows of view 1:
    <scene>_<preset>_k<k>_idx     k = 1, 3, 5, 8: the rows, int16
    <scene>_<preset>_k8_dist      the distances of the k = 8 lists, f32 (for "fast", ef 5, that is the widened beam max(ef, k))
    <scene>_fast_k5_dist          ... and of "fast"'s k = 5 lists: the longest list of its own beam
While k <= ef the DISTANCES of a k-list are a prefix of any longer list of the same beam (the beam is popped down by distance), so only
the longest list's distances are stored.  The ROWS are not always a prefix: where the k-th and the (k + 1)-th distance are equal,
which of the two rows stays is decided by the order std::priority_queue's heap (CompareByFirst) pops them in, not by the row number
(sift scene, query 297, k = 3: rows 1121 and 1184 at distance 221221, and 1184 stays).  So the rows are stored for every k.
Before anything is written the k = 2 answer must equal the idx / dist of hnsw_ref_index.npz bit for bit: the library asked here is the
library that wrote that fixture.
"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from oracle import pyoracle as O
from test_oracle_hnsw import PRESETS, load_case

NQ = 512
out = os.path.join(ROOT, "tests", "golden", "hnsw_ref_knn.npz")
O.build()
R = O.ref_lib()
assert R is not None and hasattr(R, "ref_hnsw_ann_l2"), "oracle/_ref not built: needs /root/reference"


def ref_knn(d0, q, M, efc, ef, k):
    idx = np.zeros((len(q), k), np.int32); dist = np.zeros((len(q), k), np.float32)
    rc = R.ref_hnsw_ann_l2(d0.ctypes.data_as(C.c_void_p), len(d0), q.ctypes.data_as(C.c_void_p), len(q), d0.shape[1], M, efc, ef, k,
                           idx.ctypes.data_as(C.c_void_p), dist.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return idx, dist


KS = (1, 3, 5, 8)
data = {}
for scene in ("sift", "liop"):
    for preset in PRESETS:
        d0, d1, ix, idx2, dist2 = load_case(scene, preset)
        M, efc, ef = O.HNSW_PRESETS[preset]
        q = np.ascontiguousarray(d1[:NQ])
        i2, e2 = ref_knn(d0, q, M, efc, ef, 2)
        assert np.array_equal(i2, idx2[:NQ]) and np.array_equal(e2.view(np.uint32), dist2[:NQ].view(np.uint32)), (scene, preset, "k = 2 is not the stored fixture")
        p = f"{scene}_{preset}_"
        lists = {k: ref_knn(d0, q, M, efc, ef, k) for k in KS}
        for k, (ik, ek) in lists.items():
            assert (ik >= 0).all() and ik.max() < 32768, (scene, preset, k, "a query came back short")
            assert (np.diff(ek, axis=1) >= 0).all(), (scene, preset, k, "not ascending")
            data[p + f"k{k}_idx"] = ik.astype(np.int16)
        data[p + "k8_dist"] = lists[8][1]
        if preset == "fast":
            data[p + "k5_dist"] = lists[5][1]
        for k, (ik, ek) in lists.items():
            longest = lists[8 if (k > ef or ef >= 8) else 5]
            assert np.array_equal(ek.view(np.uint32), longest[1][:, :k].view(np.uint32)), (scene, preset, k, "distances are no prefix")
            off = np.where((ik != longest[0][:, :k]).any(axis=1))[0]
            ties = int(((np.diff(ek, axis=1) == 0).any(axis=1)).sum())
            print(scene, preset, "k", k, "queries with tied distances inside the list:", ties, "; rows that are no prefix of the longest list:", off.tolist(), flush=True)
np.savez_compressed(out, **data)
print(out, os.path.getsize(out) / 1e3, "kB")
