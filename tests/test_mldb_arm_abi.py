"""The MLDB descriptor arm in the C ABI, without a GPU: the new symbols exist in the product and the developer library, the Python ABI
list names them, and a null handle (what a host holds after a failed r3dm_create) is refused before a device is touched."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["r3dm_detect_akaze_mldb_batch", "r3dm_set_descriptor_arm", "r3dm_multi_set_descriptor_arm"]
R3DM_ERR_INVALID = -1


@pytest.mark.parametrize("lib", ["libr3dm.so", "libr3dm_dev.so"])
def test_new_symbols_are_exported_by_both_libraries(lib):
    L = C.CDLL(os.path.join(ROOT, "regard3d_amd", lib))
    for name in NEW:
        assert hasattr(L, name), (lib, name)


def test_python_abi_list_and_constants_name_the_arm():
    from regard3d_amd import api
    assert set(NEW) <= set(api.EXPORTS)
    assert api.DESCRIPTORS == {"LIOP": 0, "MLDB": 1} and api.STAGE_DESCRIPTOR_MLDB == 512
    hdr = open(os.path.join(ROOT, "include", "r3dm.h")).read() + open(os.path.join(ROOT, "include", "r3d_compute_matches.hpp")).read()
    for line in ("#define R3DM_DESCRIPTOR_LIOP 0", "#define R3DM_DESCRIPTOR_MLDB 1", "#define R3DM_STAGE_DESCRIPTOR_MLDB 512u"):
        assert line in hdr, line
    assert [n for n, _ in api.StageReport._fields_][-1] == "descriptor_arm"
    with pytest.raises(ValueError):
        api._descriptor_flag("SURF")


def test_null_handles_are_refused_without_a_gpu():
    from regard3d_amd import api
    L = api.load_library()
    for arm in (0, 1, 2, -1):
        assert L.r3dm_set_descriptor_arm(None, arm) == R3DM_ERR_INVALID
        assert L.r3dm_multi_set_descriptor_arm(None, arm) == R3DM_ERR_INVALID
    img = np.zeros((64, 64), np.float32)
    ip = (C.c_void_p * 1)(img.ctypes.data)
    kps = np.zeros((4, 4), np.float32); desc = np.zeros((4, 61), np.uint8)
    kp_p = (C.c_void_p * 1)(kps.ctypes.data); dp_p = (C.c_void_p * 1)(desc.ctypes.data)
    n = np.full(1, 9, np.uint32)
    assert L.r3dm_detect_akaze_mldb_batch(None, 1, ip, 64, 64, 0.001, kp_p, dp_p, 4, n.ctypes.data) == R3DM_ERR_INVALID
    assert not desc.any() and not kps.any()
