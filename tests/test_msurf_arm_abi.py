"""The M-SURF-64 descriptor arm in the C ABI, without a GPU: the new symbols exist in the product and the developer library, the Python
ABI list names them, the headers carry the arm's two numbers, the table the existing suite pins is untouched, and a null handle (what a
host holds after a failed r3dm_create) is refused before a device is touched."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["r3dm_detect_akaze_msurf", "r3dm_detect_akaze_msurf_batch"]
R3DM_ERR_INVALID = -1


@pytest.mark.parametrize("lib", ["libr3dm.so", "libr3dm_dev.so"])
def test_new_symbols_are_exported_by_both_libraries(lib):
    L = C.CDLL(os.path.join(ROOT, "regard3d_amd", lib))
    for name in NEW:
        assert hasattr(L, name), (lib, name)


def test_python_abi_list_and_constants_name_the_arm():
    from regard3d_amd import api
    assert set(NEW) <= set(api.EXPORTS)
    assert api.DESCRIPTORS == {"LIOP": 0, "MLDB": 1}                                  # what the suite pins stays
    assert api.DESCRIPTOR_ARMS == {"LIOP": 0, "MLDB": 1, "MSURF": 3} and api.STAGE_DESCRIPTOR_MSURF == 1024
    hdr = open(os.path.join(ROOT, "include", "r3dm.h")).read() + open(os.path.join(ROOT, "include", "r3d_compute_matches.hpp")).read()
    for line in ("#define R3DM_DESCRIPTOR_MSURF 3", "#define R3DM_STAGE_DESCRIPTOR_MSURF 1024u"):
        assert line in hdr, line
    assert "#define R3DM_DESCRIPTOR_" + "MSURF 2" not in hdr
    assert [n for n, _ in api.StageReport._fields_][-1] == "descriptor_arm"
    assert api._descriptor_flag("MSURF") == 1024 and api._descriptor_flag("MLDB") == 512 and api._descriptor_flag("LIOP") == 0
    with pytest.raises(ValueError):
        api._descriptor_flag("SURF")
    for cls in (api.Context, api.MultiContext):
        assert hasattr(cls, "set_descriptor_arm")
    assert hasattr(api.Context, "detect_akaze_msurf_batch")


def test_null_handles_are_refused_without_a_gpu():
    from regard3d_amd import api
    L = api.load_library()
    for arm in (3, 2):
        assert L.r3dm_set_descriptor_arm(None, arm) == R3DM_ERR_INVALID
        assert L.r3dm_multi_set_descriptor_arm(None, arm) == R3DM_ERR_INVALID
    img = np.zeros((96, 128), np.float32)
    ip = (C.c_void_p * 1)(img.ctypes.data)
    kps = np.zeros((4, 4), np.float32); desc = np.zeros((4, 64), np.float32)
    kp_p = (C.c_void_p * 1)(kps.ctypes.data); dp_p = (C.c_void_p * 1)(desc.ctypes.data)
    n = np.full(1, 9, np.uint32)
    assert L.r3dm_detect_akaze_msurf_batch(None, 1, ip, 128, 96, 0.001, kp_p, dp_p, 4, n.ctypes.data) == R3DM_ERR_INVALID
    n1 = C.c_uint32(9)
    assert L.r3dm_detect_akaze_msurf(None, img.ctypes.data, 128, 96, 0.001, kps.ctypes.data, desc.ctypes.data, 4, C.byref(n1)) == R3DM_ERR_INVALID
    assert not desc.any() and not kps.any() and n[0] == 9 and n1.value == 9


def test_both_descriptor_stage_flags_together_are_refused_without_a_gpu():
    from regard3d_amd import api
    L = api.load_library()
    L.r3dm_compute_matches_stage.restype = C.c_int
    err = C.create_string_buffer(512)
    rep = api.StageReport()
    ids = (C.c_int * 1)(0)
    flags = api.STAGE_DESCRIPTOR_MLDB | api.STAGE_DESCRIPTOR_MSURF
    rc = L.r3dm_compute_matches_stage(ids, 1, b"/nonexistent-matches-dir", None, C.c_uint32(0), C.c_float(0.001), C.c_float(0.8), 9, 1, 0, 0, C.c_uint64(5489), 1, 1,
                                      C.c_uint32(flags), C.byref(rep), err, C.c_size_t(512))
    assert rc == R3DM_ERR_INVALID and b"R3DM_STAGE_DESCRIPTOR_MSURF" in err.value
