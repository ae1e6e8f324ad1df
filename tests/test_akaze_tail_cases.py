"""The case table of the Fast-A-KAZE tail (tests/akaze_tail_cases.py) proved on the CPU: every case reaches the edge it is named for, on
the outputs of the reference (oracle/akaze.c: orc_akaze_tail and its orientation probes) alone; the level table the cases are built on is
the product's; r3dm_dev_akaze_tail_check (developer build, needs no device) accepts every case and refuses each clause of its contract.
The GPU half is tests/test_gpu_akaze_tail.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import akaze_tail_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = T.all_cases()
INVALID = -1


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_case_reaches_its_edge_on_the_reference(case):
    case["proof"](case, T.reference(case))


def test_every_family_of_the_issue_is_in_the_table():
    names = {c["name"] for c in CASES}
    for want in ("radius_of_the_upper_level", "equal_responses", "dead_by_lower_does_not_kill_upward", "killed_later_still_kills",
                 "unsorted_lists-descending", "unsorted_lists-shuffled", "span_edges", "span_edges-lists_of_one", "many_killer_chunks",
                 "refinement_edges", "compaction_interleaved", "key_42", "zero_gradient", "one_slice", "tied_windows", "full_slices",
                 "mldb_orientation_0", "mldb_orientation_90", "mldb_orientation_180", "mldb_orientation_270", "mldb_border_corners",
                 "mldb_constant_lt", "mldb_zero_gradient_negative_lt", "mldb_signed_zero_means"):
        assert want in names, want
    lv = T.levels()
    for i in range(len(lv) - 1):                                        # every adjacent level pair, the octave step among them
        assert {f"either_side_of_the_radius-{i}-{i + 1}-lower", f"either_side_of_the_radius-{i}-{i + 1}-upper"} <= names
    assert any(lv[i]["ratio"] != lv[i + 1]["ratio"] for i in range(len(lv) - 1))
    ns = sorted(T.reference(c)["n"] for c in CASES if c["family"] == "mldb")
    assert 1 in ns and any(n % 2 == 1 and n > 1 for n in ns) and any(n % 2 == 0 and n for n in ns), "MLDB launches of 1, an odd and an even count"
    for name, fam, cs in T.batches():                                   # every case rides in a batch of three with an empty image in the middle
        assert len(cs) == 3 and T.reference(cs[1])["n"] == 0 and sum(len(l) for l in cs[1]["lists"]) == 0
    assert {c["name"] for _, _, cs in T.batches() for c in cs} == names | {"empty"}


def test_the_160_by_120_table():
    lv = T.levels()
    assert len(lv) == 5 and lv[4]["h"] - 2 * lv[4]["border"] == 2 and lv[4]["ratio"] == 2.0, "five levels, the last with an interior of 2 rows"
    assert [e["sigma_size"] for e in lv] == [2, 3, 3, 4, 2]


# ---------------------------------------------------------------------------------------------------- the developer library, in a child
def _in_child(fn):
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; import test_akaze_tail_cases as M; M.{fn}()"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]


def _dev():
    from regard3d_amd import api
    return api, api.bind_dev_akaze_tail(C.CDLL(api.DEV_LIB_PATH))


def _check(dev, images, w=T.W, h=T.H, n_levels=None, dims=None):
    api, L = dev
    nl, d, ptrs, n_list, lists, keep = api.dev_tail_args(images)
    if dims is not None:
        d = np.ascontiguousarray(dims, np.uint32)
    return L.r3dm_dev_akaze_tail_check(w, h, len(images), nl if n_levels is None else n_levels, api._ptr(d), C.addressof(ptrs), api._ptr(n_list),
                                       api._ptr(lists))


def test_dev_entries_exist_in_the_developer_build_only():
    from regard3d_amd import api
    syms = subprocess.run(["nm", "-D", api.LIB_PATH], capture_output=True, text=True).stdout
    dsyms = subprocess.run(["nm", "-D", api.DEV_LIB_PATH], capture_output=True, text=True).stdout
    assert "r3dm_dev_" not in syms
    for name in ("r3dm_dev_akaze_tail", "r3dm_dev_akaze_tail_check", "r3dm_dev_akaze_tail_levels"):
        assert f" T {name}\n" in dsyms, name
    hdr = "".join(open(os.path.join(ROOT, "include", f)).read() for f in os.listdir(os.path.join(ROOT, "include")))
    assert "r3dm_dev_akaze_tail" not in hdr


def test_the_level_table_is_the_products():
    _in_child("_level_table")


def _level_table():
    api, L = _dev()
    for w, h in ((160, 120), (320, 240), (640, 480), (101, 97)):
        mine, theirs = T.levels(w, h), api.dev_akaze_tail_levels(L, w, h)
        assert len(mine) == len(theirs) > 0, (w, h)
        for a, b in zip(mine, theirs):
            for k in ("w", "h", "border", "sigma_size"):
                assert a[k] == b[k], (w, h, k)
            for k in ("ratio", "esigma", "psize"):
                assert np.float32(a[k]).tobytes() == np.float32(b[k]).tobytes(), (w, h, k)


def test_check_accepts_every_case_and_refuses_each_clause():
    _in_child("_validation_checks")


def _validation_checks():
    dev = _dev()
    img = lambda c: dict(planes=c["planes"], lists=c["lists"])        # noqa: E731
    for c in CASES:
        assert _check(dev, [img(c)]) == 0, c["name"]
    for name, fam, cs in T.batches():
        assert _check(dev, [img(c) for c in cs]) == 0, name
    lv = T.levels()
    base = T.finish(T.blank(1, "base", "x", None))
    good = T.blank(1, "good", "x", None); T.add(good, 0, 29, 29, 1.0); T.add(good, 4, 50, 30, 1.0); T.add(good, 0, 29, 29, 1.0); T.finish(good)
    assert _check(dev, [img(good)]) == 0, "the corners of the interiors, a repeated position"

    def with_plane(level, q, value):
        c = T.finish(T.blank(1, "bad", "x", None))
        c["planes"][level][q][-1, -1] = value
        return img(c)

    def with_entry(level, x, y, resp):
        c = T.finish(T.blank(1, "bad", "x", None))
        c["lists"][level] = np.array([[x, y, resp]], np.float32)
        return img(c)
    # a non-finite plane value or response
    for q in range(4):
        for v in (np.nan, np.inf, -np.inf):
            assert _check(dev, [with_plane(2, q, v)]) == INVALID, (q, v)
    assert _check(dev, [img(base), with_plane(4, 1, np.nan)]) == INVALID, "in a later image of the batch too"
    for v in (np.nan, np.inf, -np.inf):
        assert _check(dev, [with_entry(0, 60, 60, v)]) == INVALID
    # a position that is not column x ratio, row x ratio inside [border, dim - border)
    e0, e4 = lv[0], lv[4]
    for level, x, y in ((0, e0["border"] - 1, 60), (0, 60, e0["border"] - 1), (0, e0["w"] - e0["border"], 60), (0, 60, e0["h"] - e0["border"]),
                        (0, 60.5, 60), (0, 60, 60.25), (0, np.nan, 60), (0, -60, 60),
                        (4, 61, 60), (4, 60, 59), (4, 2 * (e4["border"] - 1), 60), (4, 60, 2 * (e4["h"] - e4["border"])), (1, e0["border"], e0["border"])):
        assert _check(dev, [with_entry(level, x, y, 1.0)]) == INVALID, (level, x, y)
    for level, x, y in ((0, e0["border"], e0["border"]), (0, e0["w"] - e0["border"] - 1, e0["h"] - e0["border"] - 1),
                        (4, 2 * e4["border"], 2 * e4["border"]), (4, 2 * (e4["w"] - e4["border"] - 1), 2 * (e4["h"] - e4["border"] - 1))):
        assert _check(dev, [with_entry(level, x, y, 1.0)]) == 0, (level, x, y)
    # plane sizes other than the table's
    dims = np.array([[e["w"], e["h"]] for e in lv], np.uint32)
    assert _check(dev, [img(base)], dims=dims) == 0
    for level, k in ((0, 0), (3, 1), (4, 0)):
        bad = dims.copy(); bad[level, k] -= 1
        assert _check(dev, [img(base)], dims=bad) == INVALID
    assert _check(dev, [img(base)], n_levels=4) == INVALID and _check(dev, [img(base)], n_levels=6) == INVALID
    assert _check(dev, [img(base)], w=320, h=240) == INVALID, "the planes of another image size"
    assert _check(dev, [img(base)], w=40, h=40) == INVALID, "an image size without a level"
    # B or list lengths beyond what the entry allocates
    assert _check(dev, [img(base)] * 64) == 0 and _check(dev, [img(base)] * 65) == INVALID
    api, L = dev
    nl, d, ptrs, n_list, lists, keep = api.dev_tail_args([img(base)])
    assert L.r3dm_dev_akaze_tail_check(T.W, T.H, 0, nl, api._ptr(d), C.addressof(ptrs), api._ptr(n_list), api._ptr(lists)) == INVALID
    long = T.finish(T.blank(1, "long", "x", None))
    long["lists"][0] = np.tile(np.array([[60, 60, 1.0]], np.float32), ((1 << 20) + 1, 1))
    assert _check(dev, [img(long)]) == INVALID
    long["lists"][0] = long["lists"][0][:1 << 20]
    assert _check(dev, [img(long)]) == 0
    # null arrays; the entry itself refuses the same before it touches a device (null context)
    assert L.r3dm_dev_akaze_tail_check(T.W, T.H, 1, nl, None, C.addressof(ptrs), api._ptr(n_list), api._ptr(lists)) == INVALID
    assert L.r3dm_dev_akaze_tail_check(T.W, T.H, 1, nl, api._ptr(d), None, api._ptr(n_list), api._ptr(lists)) == INVALID
    assert L.r3dm_dev_akaze_tail_check(T.W, T.H, 1, nl, api._ptr(d), C.addressof(ptrs), None, api._ptr(lists)) == INVALID
    one = with_entry(0, 60, 60, 1.0)
    nl, d, ptrs, n_list, lists, keep = api.dev_tail_args([one])
    assert L.r3dm_dev_akaze_tail_check(T.W, T.H, 1, nl, api._ptr(d), C.addressof(ptrs), api._ptr(n_list), None) == INVALID
    null_plane = (C.c_void_p * (nl * 4))(*[None if k == 7 else ptrs[k] for k in range(nl * 4)])
    assert L.r3dm_dev_akaze_tail_check(T.W, T.H, 1, nl, api._ptr(d), C.addressof(null_plane), api._ptr(n_list), api._ptr(lists)) == INVALID
    nl, d, ptrs, n_list, lists, keep = api.dev_tail_args([with_plane(0, 0, np.nan)])
    out = [np.zeros(64, np.uint8) for _ in range(5)]
    assert L.r3dm_dev_akaze_tail(None, T.W, T.H, 1, nl, api._ptr(d), C.addressof(ptrs), api._ptr(n_list), api._ptr(lists),
                                 *[api._ptr(o) for o in out]) == INVALID
