"""CPU: the C ABI of the Hamming graph matcher -- five new exports, declared, bound and present; the statistics structures untouched."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["r3dm_set_kgraph_hamming", "r3dm_multi_set_kgraph_hamming", "r3dm_kgraph_hamming_report", "r3dm_kgraph_knn2_bits", "r3dm_kgraph_knn_bits"]


def test_new_entries_are_declared_bound_and_exported():
    from regard3d_amd import api
    with open(os.path.join(ROOT, "include", "r3dm.h")) as f:
        declared = set(re.findall(r"\b(r3dm_[A-Za-z0-9_]+)\s*\(", f.read()))
    L = api.load_library()
    for name in NEW:
        assert name in declared, name
        assert name in api.EXPORTS, name
        assert hasattr(L, name), name


def test_new_entries_refuse_a_null_context():
    """before they touch a device: callable without a GPU"""
    from regard3d_amd import api
    L = api.load_library()
    rep = api.KGraphHammingStats()
    kp = api.KGraphParams.preset("default")
    rows = (C.c_uint8 * (256 * 64))()
    idx = (C.c_int32 * (256 * 8))(); dist = (C.c_float * (256 * 8))()
    assert L.r3dm_set_kgraph_hamming(None, 1) != 0
    assert L.r3dm_multi_set_kgraph_hamming(None, 1) != 0
    assert L.r3dm_kgraph_hamming_report(None, C.byref(rep)) != 0
    assert L.r3dm_kgraph_knn2_bits(None, rows, 256, rows, 256, 64, C.addressof(kp), 0, 1, idx, dist) != 0
    assert L.r3dm_kgraph_knn_bits(None, rows, 256, rows, 256, 64, C.addressof(kp), 0, 1, 3, idx, dist) != 0


def test_statistics_structures_are_unchanged():
    """what is new is reported through r3dm_kgraph_hamming_report, not through r3dm_stats or the stage report"""
    from regard3d_amd import api
    assert len(api.Stats._fields_) == 40 and api.Stats._fields_[-1][0] == "n_knn_hamming_tiles" and C.sizeof(api.Stats) == 320
    assert len(api.StageReport._fields_) == 27 and api.StageReport._fields_[-1][0] == "descriptor_arm"
    assert [f[0] for f in api.KGraphHammingStats._fields_] == ["n_index_builds", "n_search_launches"]
