"""The case table of the Fast-A-KAZE head (tests/akaze_head_cases.py) proved on the CPU: every case reaches the edge it is named for, on
the outputs of the reference (oracle/akaze.c: orc_akaze_head, orc_akaze_extrema) and on the launch plan the product forms for the case's
image size (r3dm_dev_akaze_head_plan: ak_level_plan, the function the detector itself follows; needs no device); the oracle's detector is
its head followed by its tail; the level table the cases are built on is the product's; r3dm_dev_akaze_head_check and
r3dm_dev_akaze_extrema_check accept every case and refuse each clause of their contracts.  The GPU half is tests/test_gpu_akaze_head.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import akaze_head_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = T.all_cases()
INVALID = -1


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_case_reaches_its_edge_on_the_reference(case):
    case["proof"](case, T.reference(case))


def test_every_case_of_the_issue_is_in_the_table():
    names = {c["name"] for c in CASES}
    for w, h in ((163, 121), (187, 123), (160, 120), (327, 245), (60, 90), (61, 61)):
        for kind in ("noise", "scene"):
            assert {f"{kind}-{w}x{h}-1e-07", f"{kind}-{w}x{h}-0.001"} <= names
    for want in ("flat", "stripes_default_with_a_maximum", "ramp_percentile_at_the_last_bin", "isolated_pixel", "corners_and_seams",
                 "threshold_and_ties", "pruning_chains") + T.VARIANT_IMAGE_CASES:
        assert want in names, want
    assert sum(c["family"] == "seams" for c in CASES) == 6 and all(max(T.size_of(c["image"])) <= 330 for c in CASES if c["kind"] == "image")
    assert np.array_equal(T.image("stripes-162x120")[5, :6], np.float32([0.75, 0.25, 0.75, 0.75, 0.25, 0.75]))
    assert T.image("ramp-160x120")[7, 100] == np.float32(100 / 256) and np.count_nonzero(T.image("pixel-160x120") != 0.25) == 1
    # every image and every planted case rides in a batch of three with an image without a candidate in the middle
    in_batches = set()
    for name, fam, kind, thr, items in T.batches():
        assert len(items) == 3
        if kind == "image":
            assert items[1].startswith("flat") and len({T.size_of(i) for i in items}) == 1
            assert not T.head_reference(items[1], thr)["n_cand"].any()
            in_batches |= {items[0], items[2]}
        else:
            assert not T.reference(items[1])["n_cand"].any()
            in_batches |= {items[0]["name"], items[2]["name"]}
    assert in_batches >= {c["image"] for c in CASES if c["kind"] == "image" and not c["image"].startswith("flat")}
    assert in_batches >= {c["name"] for c in CASES if c["kind"] == "planes"}
    # the variants of the pruning run the planted planes, the variants of the scale space the three images
    assert {c["family"] for c in T.variant_cases()} == {"sizes", "kcontrast", "planted"}
    assert set(T.VARIANTS) == {"fed_through_lds", "fed_one_step_per_launch", "march_two_steps", "one_pass_level_head", "prune_one_wavefront", "prune_live_cap_8"}


def test_the_oracles_detector_is_its_head_then_its_tail():
    """orc_akaze_detect against orc_akaze_head + orc_akaze_tail called from here, and orc_akaze_extrema on the head's own determinant
    planes against the head's lists"""
    for name, thr in (("noise-163x121", 1e-7), ("scene-327x245", 1e-3)):
        img = T.image(name)
        head = T.head_reference(name, thr)
        tail = T.O.akaze_tail(head["levels"], head["planes"], head["lists"], want_desc=False)
        det = T.O.akaze_detect(img, thr)
        assert tail["n"] == len(det["kps"]) > 10
        for j, k in enumerate(("x", "y", "size", "angle_deg")):
            assert tail[k].tobytes() == np.ascontiguousarray(det["kps"][:, j]).tobytes(), (name, k)
        assert tail["response"].tobytes() == det["responses"].tobytes() and np.array_equal(tail["level"], det["levels"])
        for i, e in enumerate(head["levels"]):
            nc, lst = T.O.akaze_extrema(head["planes"][i][0], e["border"], e["ratio"], e["psize"], thr)
            assert nc == head["n_cand"][i] and lst.tobytes() == head["lists"][i].tobytes(), (name, i)
        dbg = T.O.akaze_detect(img, thr, dbg_level=len(head["levels"]) - 1)
        assert dbg["ldet"].tobytes() == head["planes"][-1][0].tobytes() and dbg["lt"].tobytes() == head["planes"][-1][3].tobytes()


# ---------------------------------------------------------------------------------------------------- the developer library, in a child
def _in_child(fn, env=None):
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; import test_akaze_head_cases as M; M.{fn}()"
    e = {k: v for k, v in os.environ.items() if not k.startswith("R3DM_")}
    e.update(env or {})
    r = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]


def _dev():
    from regard3d_amd import api
    return api, api.bind_dev_akaze_head(C.CDLL(api.DEV_LIB_PATH))


def test_dev_entries_exist_in_the_developer_build_only():
    from regard3d_amd import api
    syms = subprocess.run(["nm", "-D", api.LIB_PATH], capture_output=True, text=True).stdout
    dsyms = subprocess.run(["nm", "-D", api.DEV_LIB_PATH], capture_output=True, text=True).stdout
    assert "r3dm_dev_" not in syms
    for name in ("r3dm_dev_akaze_head", "r3dm_dev_akaze_head_check", "r3dm_dev_akaze_head_plan", "r3dm_dev_akaze_head_bound",
                 "r3dm_dev_akaze_extrema", "r3dm_dev_akaze_extrema_check"):
        assert f" T {name}\n" in dsyms, name
    hdr = "".join(open(os.path.join(ROOT, "include", f)).read() for f in os.listdir(os.path.join(ROOT, "include")))
    assert "r3dm_dev_akaze_head" not in hdr and "r3dm_dev_akaze_extrema" not in hdr


def test_the_level_table_is_the_products():
    _in_child("_level_table")


def _level_table():
    api, L = _dev()
    sizes = {T.size_of(c["image"]) for c in CASES if c["kind"] == "image"} | {(T.PW, T.PH), (640, 480), (101, 97)}
    for w, h in sorted(sizes):
        mine, theirs = T.levels(w, h), api.dev_akaze_tail_levels(L, w, h)
        assert len(mine) == len(theirs) > 0, (w, h)
        for a, b in zip(mine, theirs):
            for k in ("w", "h", "border", "sigma_size"):
                assert a[k] == b[k], (w, h, k)
            for k in ("ratio", "esigma", "psize"):
                assert np.float32(a[k]).tobytes() == np.float32(b[k]).tobytes(), (w, h, k)
        assert api.dev_head_bound(L, w, h) == sum(((e["w"] + 1) // 2) * ((e["h"] + 1) // 2) for e in mine)


def test_the_launch_plan_puts_the_seams_where_the_cases_say():
    _in_child("_plan_proofs")


def _plan_proofs():
    api, L = _dev()
    seen = 0
    for c in CASES:
        if c.get("plan_proof"):
            w, h = T.size_of(c["image"])
            c["plan_proof"](c, api.dev_head_plan(L, w, h, 1)); seen += 1
            if len(T.levels(w, h)) > 1:
                T.variant_plan_proof("product", api.dev_head_plan(L, w, h, 3))
    assert seen >= 30
    # the strips of the reference's time steps under the product's chunking, levels 1 to 6 of three octaves
    plan = api.dev_head_plan(L, 327, 245, 1)
    assert [vw for i, vw, rows in T.strips(plan, None) if i <= 6] == [58, 58, 56, 56, 54, 52] and {rows for _, _, rows in T.strips(plan, None)} == {16}


@pytest.mark.parametrize("variant", sorted(T.VARIANTS))
def test_a_variants_plan_shows_that_it_runs(variant):
    _in_child("_variant_plan", dict(T.VARIANTS[variant], HEAD_CASES_VARIANT=variant))


def _variant_plan():
    api, L = _dev()
    variant = os.environ["HEAD_CASES_VARIANT"]
    for c in T.variant_cases():
        if c["kind"] == "image":
            w, h = T.size_of(c["image"])
            T.variant_plan_proof(variant, api.dev_head_plan(L, w, h, 1))
    lv = T.levels(327, 245)
    if variant == "one_pass_level_head":
        assert all(2 <= e["sigma_size"] <= 4 and e["w"] >= 16 and e["h"] >= 16 for e in lv), "the head form's own conditions hold on every level"


def test_checks_accept_every_case_and_refuse_each_clause():
    _in_child("_validation_checks")


def _head_check(dev, images, w=None, h=None, B=None):
    api, L = dev
    ptrs, keep = api.dev_head_images(images)
    hh, ww = keep[0].shape
    return L.r3dm_dev_akaze_head_check(len(images) if B is None else B, C.addressof(ptrs), ww if w is None else w, hh if h is None else h)


def _extrema_check(dev, planes, w=T.PW, h=T.PH, n_levels=None, dims=None, B=None):
    api, L = dev
    nl, d, ptrs, keep = api.dev_extrema_args(planes)
    if dims is not None:
        d = np.ascontiguousarray(dims, np.uint32)
    return L.r3dm_dev_akaze_extrema_check(w, h, len(planes) if B is None else B, nl if n_levels is None else n_levels, api._ptr(d), C.addressof(ptrs))


def _validation_checks():
    dev = _dev()
    api, L = dev
    for c in CASES:
        if c["kind"] == "image":
            assert _head_check(dev, [T.image(c["image"])]) == 0, c["name"]
        else:
            assert _extrema_check(dev, [c["planes"]]) == 0, c["name"]
    for name, fam, kind, thr, items in T.batches():
        assert (_head_check(dev, [T.image(i) for i in items]) if kind == "image" else _extrema_check(dev, [i["planes"] for i in items])) == 0, name
    # ---- the head check: B outside 1 .. 8, a dimension above 4096, no evolution level, a value not finite or outside [0, 1]
    flat = T.image("flat-160x120")
    assert _head_check(dev, [flat] * 8) == 0 and _head_check(dev, [flat] * 9) == INVALID and _head_check(dev, [flat], B=0) == INVALID
    edge = np.zeros((120, 160), np.float32); edge[0, 0] = 1.0
    assert _head_check(dev, [edge]) == 0, "0 and 1 themselves are taken"
    for v in (np.nan, np.inf, -np.inf, np.nextafter(np.float32(1), np.float32(2)), -np.nextafter(np.float32(0), np.float32(1)), -1.0, 2.0):
        bad = flat.copy(); bad[-1, -1] = v
        assert _head_check(dev, [bad]) == INVALID, v
        assert _head_check(dev, [flat, flat, bad]) == INVALID, "in a later image of the batch too"
    assert _head_check(dev, [np.zeros((59, 59), np.float32)]) == INVALID and _head_check(dev, [np.zeros((61, 61), np.float32)]) == 0, "an image without a level"
    assert _head_check(dev, [np.zeros((2, 4097), np.float32)], w=4097, h=100) == INVALID and _head_check(dev, [np.zeros((2, 4097), np.float32)], w=100, h=4097) == INVALID
    assert _head_check(dev, [np.zeros((4096, 61), np.float32)]) == 0
    ptrs, keep = api.dev_head_images([flat])
    assert L.r3dm_dev_akaze_head_check(1, None, 160, 120) == INVALID
    null = (C.c_void_p * 2)(ptrs[0], None)
    assert L.r3dm_dev_akaze_head_check(2, C.addressof(null), 160, 120) == INVALID
    out = [np.zeros(4096, np.uint8) for _ in range(5)]
    bad = flat.copy(); bad[3, 3] = np.nan
    pb, kb = api.dev_head_images([bad])
    assert L.r3dm_dev_akaze_head(None, 1, C.addressof(pb), 160, 120, 0.001, *[api._ptr(o) for o in out]) == INVALID, "refused before a context is asked for"
    plan = (api.DevAkPlan * 16)()
    assert L.r3dm_dev_akaze_head_plan(160, 120, 0, C.addressof(plan)) == INVALID and L.r3dm_dev_akaze_head_plan(160, 120, 9, C.addressof(plan)) == INVALID
    assert L.r3dm_dev_akaze_head_plan(59, 59, 1, C.addressof(plan)) == INVALID and L.r3dm_dev_akaze_head_plan(4097, 100, 1, C.addressof(plan)) == INVALID
    # ---- the extrema check: what the tail's check takes for planes -- the table's dimensions, finite values
    base = T.blank_planes(1)
    assert _extrema_check(dev, [base]) == 0
    for level in (0, 4):
        for v in (np.nan, np.inf, -np.inf):
            bad = [p.copy() for p in base]; bad[level][-1, -1] = v
            assert _extrema_check(dev, [bad]) == INVALID, (level, v)
            assert _extrema_check(dev, [base, bad]) == INVALID
    big = [p.copy() for p in base]; big[0][0, 0] = np.float32(3e38); big[0][-1, -1] = np.float32(-3e38)
    assert _extrema_check(dev, [big]) == 0, "any finite value, on the rim too"
    lv = T.levels(T.PW, T.PH)
    dims = np.array([[e["w"], e["h"]] for e in lv], np.uint32)
    assert _extrema_check(dev, [base], dims=dims) == 0
    for level, k in ((0, 0), (3, 1), (4, 0)):
        bad = dims.copy(); bad[level, k] -= 1
        assert _extrema_check(dev, [base], dims=bad) == INVALID
    assert _extrema_check(dev, [base], n_levels=4) == INVALID and _extrema_check(dev, [base], n_levels=6) == INVALID
    assert _extrema_check(dev, [base], w=320, h=240) == INVALID, "the planes of another image size"
    assert _extrema_check(dev, [base], w=40, h=40) == INVALID, "an image size without a level"
    assert _extrema_check(dev, [base] * 64) == 0 and _extrema_check(dev, [base] * 65) == INVALID and _extrema_check(dev, [base], B=0) == INVALID
    nl, d, ptrs, keep = api.dev_extrema_args([base])
    assert L.r3dm_dev_akaze_extrema_check(T.PW, T.PH, 1, nl, None, C.addressof(ptrs)) == INVALID
    assert L.r3dm_dev_akaze_extrema_check(T.PW, T.PH, 1, nl, api._ptr(d), None) == INVALID
    null = (C.c_void_p * nl)(*[None if k == 2 else ptrs[k] for k in range(nl)])
    assert L.r3dm_dev_akaze_extrema_check(T.PW, T.PH, 1, nl, api._ptr(d), C.addressof(null)) == INVALID
    bad = [p.copy() for p in base]; bad[1][5, 5] = np.nan
    nl, d, ptrs, keep = api.dev_extrema_args([bad])
    assert L.r3dm_dev_akaze_extrema(None, T.PW, T.PH, 1, nl, api._ptr(d), C.addressof(ptrs), 0.001, api._ptr(out[0]), api._ptr(out[1])) == INVALID
