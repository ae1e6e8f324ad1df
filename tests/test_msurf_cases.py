"""The tables of the M-SURF-64 arm (tests/msurf_cases.py) proved on the CPU, on the reference alone: the oracle's head and tail
(oracle/akaze.c) under the M-SURF level table, and the serial restatement tests/cpp/msurf_restatement.cpp.  The GPU halves are
tests/test_gpu_msurf_kernel.py and tests/test_gpu_msurf_arm.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import msurf_cases as S
from oracle import pyoracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The largest absolute difference between a descriptor element computed with libm's expf (the reference's) and with ak_expf (the
# kernel's), MEASURED over every case of this file (batches, stage views, kernel cases; glibc 2.35): 0.0 -- of the 241,408 exponent
# arguments of the batches one differs between the two exponentials (by 1 ulp), and no element moves.  The test asserts 4 x this.
LIBM_VS_AK_EXPF_MEASURED = 0.0


@pytest.fixture(scope="module", autouse=True)
def _oracle_built(oracle):
    return oracle


# ---- the level table
def test_the_msurf_table_is_a_prefix_with_wider_borders():
    for w, h in ((160, 120), (320, 240), (640, 480), (128, 96), (192, 160), (4000, 3000)):
        mine, mldb = S.levels(w, h), O.akaze_levels(w, h)
        assert 0 < len(mine) <= len(mldb), (w, h)
        for a, b in zip(mine, mldb):
            assert all(a[k] == b[k] for k in a if k != "border") and a["border"] > b["border"]
            assert a["border"] == int(np.float32(S.SMAX_MSURF * np.float32(a["sigma_size"])) + np.float32(0.5)) + 1
            assert a["sigma_size"] in (2, 3, 4)                                   # what the in-plane argument of the kernel counts on
    assert len(S.levels(160, 120)) == 3 < len(O.akaze_levels(160, 120)) == 5
    assert len(S.levels(320, 240)) == 7 < len(O.akaze_levels(320, 240))
    assert S.levels(64, 48) == [] and len(O.akaze_levels(64, 48)) == 0
    assert len(S.levels(128, 96)) == 1 and [e["sigma_size"] for e in S.levels(192, 160)] == [2, 3, 3, 4, 2]


@pytest.mark.parametrize("size", S.SIZES)
def test_a_build_that_keeps_the_mldb_border_fails(size):
    """on the images of the batches the M-SURF table has fewer levels and fewer keypoints than the MLDB table, and keypoints of the MLDB
    arm lie outside the M-SURF border: the arm cannot be served on the detector's other table"""
    thr, ims, ref = S.batch_refs(size)
    h, w = size
    lv = S.levels(w, h)
    assert len(lv) < len(O.akaze_levels(w, h))
    outside = 0
    for im, r in zip(ims, ref):
        kp_mldb = O.akaze_detect(im, thr)
        assert len(r["kps"]) <= len(kp_mldb["kps"])
        if len(kp_mldb["kps"]) == 0:
            continue
        assert len(r["kps"]) < len(kp_mldb["kps"])
        mine = {tuple(k) for k in r["kps"][:, :3].tolist()}
        for (x, y, _, _), level in zip(kp_mldb["kps"], kp_mldb["levels"]):
            if level >= len(lv):
                outside += 1
                continue
            e = lv[level]
            xf, yf = x / e["ratio"], y / e["ratio"]
            outside += not (e["border"] - 1 <= xf <= e["w"] - e["border"] and e["border"] - 1 <= yf <= e["h"] - e["border"])
        assert mine, "tens of keypoints under the M-SURF table too"
    assert outside >= 1


@pytest.mark.parametrize("size", S.SIZES)
def test_batches_hold_a_blank_image_and_every_remainder(size):
    thr, ims, ref = S.batch_refs(size)
    n = [len(r["kps"]) for r in ref]
    assert n[S.BLANK_INDEX] == 0 and S.BLANK_INDEX == 1
    assert sorted(k % S.KP_PER_GROUP for b, k in enumerate(n) if b != S.BLANK_INDEX) == [1, 2, 3], n
    assert min(k for b, k in enumerate(n) if b != S.BLANK_INDEX) >= 15
    for r in ref:                                                                  # every level position is where the check wants it
        for level, xf, yf, co, si, scale in r["items"]:
            e = r["levels"][int(level)]
            assert e["border"] - 1 <= xf <= e["w"] - e["border"] and e["border"] - 1 <= yf <= e["h"] - e["border"] and scale == e["sigma_size"]
            assert abs(co * co + si * si - 1.0) <= 1e-6


# ---- the rows
def test_every_restated_row_is_a_unit_vector():
    worst = 0.0
    for size in S.SIZES:
        for r in S.batch_refs(size)[2]:
            if len(r["rows"]):
                assert np.isfinite(r["rows"]).all()
                worst = max(worst, np.abs(np.linalg.norm(r["rows"].astype(np.float64), axis=1) - 1.0).max())
    for c in S.kernel_cases():
        rows = S.kernel_reference(c)
        nan = np.isnan(rows).all(axis=1)
        assert np.flatnonzero(nan).tolist() == c["nan_rows"], c["name"]           # the windows without gradient, and only those
        assert np.isfinite(rows[~nan]).all()
        if (~nan).any():
            worst = max(worst, np.abs(np.linalg.norm(rows[~nan].astype(np.float64), axis=1) - 1.0).max())
    print(f"largest | |row| - 1 | = {worst:.3e} (bound 2^-22 = {2.0 ** -22:.3e})")
    assert worst <= 2.0 ** -22


def test_exponent_arguments_stay_in_the_asserted_range():
    lo, hi = 0.0, -100.0
    for size in S.SIZES:
        for r in S.batch_refs(size)[2]:
            if len(r["rows"]):
                lo, hi = min(lo, r["arg_range"][0]), max(hi, r["arg_range"][1])
    assert -4.1 <= lo and hi <= 0.0 and lo < -3.9, (lo, hi)                       # (the restatement asserts the range per call too)


# ---- ak_expf
def _sweep():
    hi = int(np.float32(-4.1).view(np.uint32)); lo = 0x80000000                    # bit patterns of -0.0 .. -4.1, stride 2^7
    return np.arange(lo, hi + 1, 128, dtype=np.uint64).astype(np.uint32).view(np.float32)


def _case_arguments():
    return np.concatenate([r["args"].ravel() for size in S.SIZES for r in S.batch_refs(size)[2]] + [np.float32([0.0, -0.0, -4.1, -1.0])])


@pytest.mark.parametrize("which", ["cases", "sweep"])
def test_ak_expf_against_libm_and_against_the_double_exponential(which):
    """ak_expf and libm's expf are each within 0.502 ulp of exp (ak_expf: 0.5 + 2^-28 by its header; glibc documents < 0.502 for expf),
    so the two floats are the two neighbours of exp at worst: never more than 1 ulp apart.  And ak_expf is the rounded double
    exponential wherever that is not within 2^-52 relative of a rounding boundary: on every argument here."""
    x = _case_arguments() if which == "cases" else _sweep()
    assert (x >= np.float32(-4.1)).all() and (x <= 0).all() and len(x) > (200000 if which == "cases" else 8000000)
    a, b = S.expf(x, False), S.expf(x, True)
    ulp = np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
    print(f"{which}: {len(x)} arguments, {int((ulp > 0).sum())} differ between ak_expf and libm expf ({(ulp > 0).mean():.2e}), largest {int(ulp.max())} ulp")
    assert ulp.max() <= 1
    assert np.array_equal(a, np.exp(x.astype(np.float64)).astype(np.float32))


def test_descriptor_elements_of_the_two_exponentials():
    worst = 0.0
    for size in S.SIZES:
        thr, ims, ref = S.batch_refs(size)
        for im, r in zip(ims, ref):
            if len(r["rows"]):
                worst = max(worst, np.abs(S.detect(im, thr, libm=True)["rows"].astype(np.float64) - r["rows"]).max())
    for im in S.stage_images():
        a, b = S.detect(im, S.THR), S.detect(im, S.THR, libm=True)
        worst = max(worst, np.abs(a["rows"].astype(np.float64) - b["rows"]).max())
    for c in S.kernel_cases():
        a, b = S.kernel_reference(c), S.kernel_reference(c, True)
        ok = ~np.isnan(a).all(axis=1)
        assert np.array_equal(np.isnan(a), np.isnan(b))
        if ok.any():
            worst = max(worst, np.abs(a[ok].astype(np.float64) - b[ok]).max())
    print(f"largest | element(libm expf) - element(ak_expf) | = {worst:.3e} (measured {LIBM_VS_AK_EXPF_MEASURED:.3e})")
    assert worst <= 4.0 * LIBM_VS_AK_EXPF_MEASURED


# ---- the stage views
def test_stage_views_survive_the_oracle_chain_with_decided_ratios():
    ims = S.stage_images()
    refs, descs, xys, pairs, counts, matches = S.oracle_stage(ims)
    assert len(pairs) == 6 and (counts > 0).all()
    W = np.full(4, 320, np.uint32); H = np.full(4, 240, np.uint32)
    oc, om = O.filter_F_collection(xys, W, H, pairs, counts, matches, 4.0, 2048, S.STAGE_FILTER_SEED)
    assert (oc > 0).sum() >= 3
    r2 = np.float64(np.float32(S.STAGE_RATIO)) ** 2
    worst = np.inf
    for i, j in pairs:                                                             # every query's ratio decision, both nearest distances in double
        a, b = descs[i].astype(np.float64), descs[j].astype(np.float64)
        d = np.sort(((a[:, None, :] - b[None, :, :]) ** 2).sum(-1), axis=1)
        worst = min(worst, (np.abs(d[:, 0] - r2 * d[:, 1]) / d[:, 1]).min())
    print(f"smallest |d1 - r^2 d2| / d2 = {worst:.3e}")
    assert worst > 1e-5


# ---- no read leaves a plane: the stand-alone restatement under the address sanitizer
def test_border_cases_read_inside_exactly_sized_planes_under_asan():
    exe, why = S.sanitized_program()
    if exe is None:
        pytest.skip(f"-fsanitize=address,undefined does not link here: {why}")
    ran = 0
    for size in S.KERNEL_SIZES:
        for i, e in enumerate(S.levels(size[1], size[0])):
            b = e["border"]
            its = []
            for ang in ("0", "45", "90", "225", "pi"):
                co, si = S.ANGLES[ang]
                for x, y in ((b - 1, b - 1), (e["w"] - b, e["h"] - b), (b - 1, e["h"] - b), (e["w"] - b, b - 1), (b - 0.5, e["h"] - b - 0.5)):
                    its.append(f"{float(np.float32(x))!r} {float(np.float32(y))!r} {float(np.float32(co))!r} {float(np.float32(si))!r} {e['sigma_size']}")
            r = subprocess.run([exe, str(e["w"]), str(e["h"]), str(len(its))], input="\n".join(its) + "\n", capture_output=True, text=True, timeout=120)
            assert r.returncode == 0 and r.stdout.strip().endswith(f"done {len(its)}") and "ERROR" not in r.stderr, (size, i, r.stderr[-2000:])
            ran += len(its)
    assert ran == 6 * 25
    # ... and the sanitizer does see a read that leaves the plane: the same keypoint one column further out
    e = S.levels(128, 96)[0]
    r = subprocess.run([exe, str(e["w"]), str(e["h"]), "1"], input=f"{e['w'] - e['border'] + 1} {e['h'] - e['border'] + 1} -0.70710677 -0.70710677 2\n",
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "AddressSanitizer" in r.stderr


# ---- the developer build's check, without a device (in a child: the developer library is not loaded into this process)
def _in_child(fn):
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; import test_msurf_cases as M; M.{fn}()"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]


def test_dev_entries_exist_in_the_developer_build_only():
    from regard3d_amd import api
    syms = subprocess.run(["nm", "-D", api.LIB_PATH], capture_output=True, text=True).stdout
    dsyms = subprocess.run(["nm", "-D", api.DEV_LIB_PATH], capture_output=True, text=True).stdout
    assert "r3dm_dev_" not in syms
    for name in ("r3dm_dev_akaze_msurf", "r3dm_dev_akaze_msurf_check", "r3dm_dev_akaze_msurf_levels"):
        assert f" T {name}\n" in dsyms, name
    hdr = "".join(open(os.path.join(ROOT, "include", f)).read() for f in os.listdir(os.path.join(ROOT, "include")))
    assert "r3dm_dev_akaze_msurf" not in hdr


def test_the_level_table_is_the_products():
    _in_child("_level_table")


def _level_table():
    from regard3d_amd import api
    L = api.bind_dev_akaze_msurf(C.CDLL(api.DEV_LIB_PATH))
    for w, h in ((160, 120), (320, 240), (640, 480), (128, 96), (192, 160), (101, 97), (64, 48)):
        mine, theirs = S.levels(w, h), api.dev_akaze_msurf_levels(L, w, h)
        assert len(mine) == len(theirs), (w, h)
        for a, b in zip(mine, theirs):
            for k in ("w", "h", "border", "sigma_size"):
                assert a[k] == b[k], (w, h, k)
            for k in ("ratio", "esigma", "psize"):
                assert np.float32(a[k]).tobytes() == np.float32(b[k]).tobytes(), (w, h, k)


def test_check_accepts_every_case_and_refuses_each_clause():
    _in_child("_validation_checks")


def _validation_checks():
    from regard3d_amd import api
    L = api.bind_dev_akaze_msurf(C.CDLL(api.DEV_LIB_PATH))
    INVALID = -1
    for c in S.kernel_cases():
        assert api.dev_akaze_msurf_check(L, c["size"][1], c["size"][0], c["planes"], S.api_items(c)) == 0, c["name"]
    for size in S.SIZES:                                                           # the reference chain's own keypoints on its own planes
        for r in S.batch_refs(size)[2]:
            its = np.zeros(len(r["items"]), api.MSURF_ITEM)
            for j, k in enumerate(("level", "xf", "yf", "co", "si", "scale")):
                its[k] = r["items"][:, j]
            if len(its):
                assert api.dev_akaze_msurf_check(L, size[1], size[0], [p[1:3] for p in r["planes"]], its) == 0
    h, w = 160, 192
    lv = S.levels(w, h)
    planes = S.textured(lv, 3)

    def chk(items, pl=planes, ww=w, hh=h):
        its = np.zeros(len(items), api.MSURF_ITEM)
        for k, t in enumerate(items):
            its[k] = t
        return api.dev_akaze_msurf_check(L, ww, hh, pl, its)

    e0, e3, e4 = lv[0], lv[3], lv[4]
    good = (0, 96.0, 80.0, 1.0, 0.0, 2)
    assert chk([good]) == 0 and chk([]) == 0
    # non-finite plane values
    for level, q, v in ((0, 0, np.nan), (2, 1, np.inf), (4, 0, -np.inf)):
        bad = [[a.copy() for a in lev] for lev in planes]
        bad[level][q][-1, -1] = v
        assert chk([good], bad) == INVALID, (level, q, v)
    # scale other than the level's sigma_size
    assert chk([(0, 96.0, 80.0, 1.0, 0.0, 3)]) == INVALID and chk([(3, 96.0, 80.0, 1.0, 0.0, 2)]) == INVALID and chk([(1, 96.0, 80.0, 1.0, 0.0, 3)]) == 0
    assert chk([(5, 96.0, 80.0, 1.0, 0.0, 2)]) == INVALID, "a level the table does not hold"
    # a position outside [border - 1, dim - border] of the M-SURF table -- the MLDB border's positions among them
    for e, level in ((e0, 0), (e3, 3), (e4, 4)):
        b, s = e["border"], e["sigma_size"]
        cx, cy = e["w"] / 2.0, e["h"] / 2.0
        for x, y in ((b - 1, b - 1), (e["w"] - b, e["h"] - b), (b - 1, cy), (cx, e["h"] - b)):
            assert chk([(level, x, y, 1.0, 0.0, s)]) == 0, (level, x, y)
        for x, y in ((b - 1.001, cy), (cx, b - 1.001), (e["w"] - b + 0.001, cy), (cx, e["h"] - b + 0.001), (np.nan, cy), (cx, np.inf), (-cx, cy)):
            assert chk([(level, x, y, 1.0, 0.0, s)]) == INVALID, (level, x, y)
        mldb_border = int(np.float32(S.SMAX_MLDB * np.float32(s)) + np.float32(0.5)) + 1
        assert mldb_border < b
        if mldb_border < cy:
            assert chk([(level, mldb_border, cy, 1.0, 0.0, s)]) == INVALID and chk([(level, cx, e["h"] - mldb_border, 1.0, 0.0, s)]) == INVALID
    # cos / sin that are no unit vector
    for co, si in ((1.0, 1e-2), (0.999, 0.0), (0.0, 0.0), (np.nan, 0.0), (1.0 + 2e-6, 0.0)):
        assert chk([(0, 96.0, 80.0, co, si, 2)]) == INVALID, (co, si)
    assert chk([(0, 96.0, 80.0, np.float32(np.cos(1.0)), np.float32(np.sin(1.0)), 2)]) == 0
    # a bad item behind good ones; planes of another size; a size without a level
    assert chk([good] * 7 + [(0, 96.0, 80.0, 1.0, 0.0, 4)]) == INVALID
    assert chk([good], ww=320, hh=240) == INVALID and chk([good], S.textured(S.levels(128, 96), 3), 192, 160) == INVALID
    assert chk([], [], 64, 48) == INVALID, "a 48 x 64 image has no level under the M-SURF border"
    # null arrays; the entry itself refuses the same before it touches a device (null context)
    nl, dims, ptrs, n, its, keep = api.dev_msurf_args(planes, np.array([good], api.MSURF_ITEM))
    assert L.r3dm_dev_akaze_msurf_check(w, h, nl, None, C.addressof(ptrs), n, its.ctypes.data) == INVALID
    assert L.r3dm_dev_akaze_msurf_check(w, h, nl, api._ptr(dims), None, n, its.ctypes.data) == INVALID
    assert L.r3dm_dev_akaze_msurf_check(w, h, nl, api._ptr(dims), C.addressof(ptrs), n, None) == INVALID
    assert L.r3dm_dev_akaze_msurf_check(w, h, nl, api._ptr(dims), C.addressof(ptrs), (1 << 20) + 1, its.ctypes.data) == INVALID
    rows = np.full((1, 64), 7.0, np.float32)
    bad = np.array([(0, 10.0, 80.0, 1.0, 0.0, 2)], api.MSURF_ITEM)
    assert L.r3dm_dev_akaze_msurf(None, w, h, nl, api._ptr(dims), C.addressof(ptrs), 1, bad.ctypes.data, rows.ctypes.data) == INVALID
    assert L.r3dm_dev_akaze_msurf(None, w, h, nl, api._ptr(dims), C.addressof(ptrs), 1, its.ctypes.data, rows.ctypes.data) == INVALID and (rows == 7.0).all()
