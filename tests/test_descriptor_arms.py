"""The one table of the descriptor arms (regard3d_amd/csrc/descriptor_arms.hpp), compiled alone by g++ and printed
by tests/cpp/descriptor_arms_test.cpp: its rows, its two lookups, and its agreement with the `#define`s of include/r3dm.h and with the
arm list of regard3d_amd/api.py -- what "one table" means across the two languages.  Needs no GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

from regard3d_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R3DM_F32, R3DM_BIN = 0, 2
ASK = ["id", "2", "id", "4", "id", "-1", "id", "0", "id", "1", "id", "3", "type", f"{R3DM_F32},128", "type", f"{R3DM_BIN},64",
       "type", f"{R3DM_F32},144", "type", f"{R3DM_BIN},61", "type", f"{R3DM_F32},64", "type", f"{R3DM_BIN},144"]


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("descriptor_arms") / "descriptor_arms_test")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + ROOT, "-o", exe, os.path.join(ROOT, "tests", "cpp", "descriptor_arms_test.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe] + ASK, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)          # 1: a lookup does not round-trip
    lines = [ln.split() for ln in r.stdout.splitlines()]
    arms = {int(f[1]): dict(name=f[2], tag=f[3], macro=f[4], dtype=int(f[5]), dim=int(f[6]), row_bytes=int(f[7]), mult=float(f[8]), level_planes=int(f[9]),
                            smax_bits=int(f[10], 16)) for f in lines if f[0] == "arm"}
    by_id = {int(f[1]): int(f[2]) for f in lines if f[0] == "by_id"}
    by_type = {(int(f[1]), int(f[2])): (None if f[3] == "none" else int(f[3])) for f in lines if f[0] == "by_type"}
    return arms, by_id, by_type


def test_the_rows(printed):
    arms, _, _ = printed
    assert sorted(arms) == [0, 1, 3]
    assert [arms[k]["row_bytes"] for k in (0, 1, 3)] == [576, 61, 256]
    assert [(arms[k]["dtype"], arms[k]["dim"]) for k in (0, 1, 3)] == [(R3DM_F32, 144), (R3DM_BIN, 61), (R3DM_F32, 64)]
    assert [arms[k]["mult"] for k in (0, 1, 3)] == [10.0, 10.0, 12.0]
    assert [arms[k]["level_planes"] for k in (0, 1, 3)] == [0, 1, 1]
    # the names the error texts are built from
    assert [(arms[k]["name"], arms[k]["tag"]) for k in (0, 1, 3)] == [("LIOP", "LIOP"), ("MLDB", "MLDB"), ("M-SURF-64", "M-SURF")]
    # ak_smax stays the float product m * sqrtf(2.0f): the level borders are rounded from it
    for k in (0, 1, 3):
        want = np.float32(arms[k]["mult"]) * np.sqrt(np.float32(2.0))
        assert arms[k]["smax_bits"] == int(np.array([want], np.float32).view(np.uint32)[0])


def test_the_lookups(printed):
    arms, by_id, by_type = printed
    assert by_id == {2: 0, 4: 0, -1: 0, 0: 1, 1: 1, 3: 1}
    assert by_type == {(R3DM_F32, 128): None, (R3DM_BIN, 64): None, (R3DM_BIN, 144): None, (R3DM_F32, 144): 0, (R3DM_BIN, 61): 1, (R3DM_F32, 64): 3}
    for k, a in arms.items():                                              # (and the program itself returns 1 when a row does not round-trip)
        assert by_type[a["dtype"], a["dim"]] == k


def test_the_table_agrees_with_the_public_header_and_with_python(printed):
    arms, _, _ = printed
    text = open(os.path.join(ROOT, "include", "r3dm.h")).read()
    defines = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define (R3DM_DESCRIPTOR_\w+) (-?\d+)\s*$", text, re.M)}
    assert defines == {a["macro"]: k for k, a in arms.items()}
    enum = dict(re.findall(r"\b(R3DM_F32|R3DM_U8|R3DM_BIN) = (\d+)", text))
    assert int(enum["R3DM_F32"]) == R3DM_F32 and int(enum["R3DM_BIN"]) == R3DM_BIN
    assert sorted(api.DESCRIPTOR_ARMS.values()) == sorted(arms)
    np_dtype = {R3DM_F32: np.float32, R3DM_BIN: np.uint8}
    for name, arm_id, flag, dtype, dim in api._ARMS:
        a = arms[arm_id]
        assert api.DESCRIPTOR_ARMS[name] == arm_id and a["macro"] == "R3DM_DESCRIPTOR_" + name
        assert np_dtype[a["dtype"]] is dtype and a["dim"] == dim and a["row_bytes"] == dim * np.dtype(dtype).itemsize
        assert api._DESCRIPTOR_STAGE_FLAGS[name] == flag == {0: 0, 1: api.STAGE_DESCRIPTOR_MLDB, 3: api.STAGE_DESCRIPTOR_MSURF}[arm_id]
    assert api.DESCRIPTORS == {"LIOP": 0, "MLDB": 1}
