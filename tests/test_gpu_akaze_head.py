"""The Fast-A-KAZE head on the GPU, plane by plane, on images and determinant planes built for its edges (tests/akaze_head_cases.py;
DESIGN.md section 4.8): the developer build's r3dm_dev_akaze_head runs the PRODUCT's code -- ak_scale_space, ak_level_table,
ak_head_launches, the functions the detector calls -- on the caller's images and reads back Ldet, Lx, Ly and Lt of every level, the
k-contrast words, the candidate counts and the pruned lists; r3dm_dev_akaze_extrema runs ak_head_launches on the caller's determinant
planes.  The reference of every case is oracle/akaze.c's orc_akaze_head / orc_akaze_extrema alone, and every comparison is bit for bit,
list order included.  Every image and every set of planes also rides in a call of B = 3 with the flat image (planes without a
candidate) in the middle: the batch equals the single calls image for image.  The alternative launch forms run the same cases, one
process per form, against the same reference.

The developer library is loaded in child processes (the session's process holds the product library): one child per family of cases and
per launch form, one alive at a time, each under its own timeout.  A child that ends by a signal, at its timeout or with a HIP error
fails its test and sets _GPU_BROKEN: the module's remaining tests skip and start no further child.  There are no retries."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import akaze_head_cases as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = T.all_cases()
BATCHES = T.batches()
VARIANT_RUNS = [(v, c) for v in T.VARIANTS for c in T.variant_cases()]
PLANES = ("Ldet", "Lx", "Ly", "Lt")

_GPU_BROKEN = None                                 # the reason, once a child died, hung or reported a HIP error
_RESULTS = {}                                      # family -> {("single", case name) | ("batch", batch name): results}
_FAILED = {}                                       # family -> why its child failed (no second child for the same family)


def _family(family, tmp_path_factory, extra_env=None):
    """the results of a family's child, started on first use"""
    global _GPU_BROKEN
    if family in _RESULTS:
        return _RESULTS[family]
    if family in _FAILED:
        pytest.fail(_FAILED[family])
    if _GPU_BROKEN:
        pytest.skip(f"an earlier child of this module failed on the GPU: {_GPU_BROKEN}")
    op = str(tmp_path_factory.mktemp("head") / "out.pkl")
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; import akaze_head_cases as T; "
            f"sys.exit(T.child_main({family!r}, {op!r}))")
    env = {k: v for k, v in os.environ.items() if not k.startswith("R3DM_")}
    env.update(extra_env or {})
    try:
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    except subprocess.TimeoutExpired:
        _GPU_BROKEN = _FAILED[family] = f"the child of family {family!r} did not end within its timeout"
        pytest.fail(_GPU_BROKEN)
    res = pickle.load(open(op, "rb")) if os.path.exists(op) else {}
    if r.returncode < 0 or "__error__" in res or r.returncode != 0:
        why = res.get("__error__", r.stderr[-2000:])
        if r.returncode < 0 or "HIP" in why.upper() or "-> -3" in why:
            _GPU_BROKEN = f"family {family!r}: exit {r.returncode}: {why}"
        _FAILED[family] = f"the child of family {family!r} ended with {r.returncode}: {why}"
        pytest.fail(_FAILED[family])
    _RESULTS[family] = res
    return res


def _same(a, b, what):
    """bit for bit; a failure names what differs and the first few places (row, column of a plane)"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, "shape", a.shape, b.shape)
    if a.tobytes() != b.tobytes():
        bits = lambda v: np.ascontiguousarray(v).view(np.uint8).reshape(v.shape + (-1,)) if v.ndim else np.frombuffer(v.tobytes(), np.uint8)   # noqa: E731
        where = np.argwhere(np.any(bits(a) != bits(b), axis=-1))[:6].tolist()
        pytest.fail(f"{what}: differs at {where}: got {[a[tuple(p)].tolist() for p in where]}, reference {[b[tuple(p)].tolist() for p in where]}")


def _lists_equal(got, ref, what):
    assert got["n_cand"].tolist() == [int(n) for n in ref["n_cand"]], (what, "candidates before the pruning", got["n_cand"].tolist(), [int(n) for n in ref["n_cand"]])
    for level, (g, r) in enumerate(zip(got["lists"], ref["lists"])):
        _same(g, r, f"{what}, level {level}, pruned list (x, y, response) in list order")


def _head_equals_reference(got, ref, what):
    """k-contrast state first, then every plane level by level (a mismatch then points at the stage that made it), then counts and lists"""
    _same(got["hmax_bits"], np.float32(ref["hmax"]).view(np.uint32), f"{what}, hmax bits")
    _same(got["hist"], ref["hist"].astype(np.uint32), f"{what}, histogram")
    _same(got["inv_k2"], ref["inv_k2"], f"{what}, inv_k2[0..7]")
    assert len(got["planes"]) == len(ref["planes"])
    for level, (g, r) in enumerate(zip(got["planes"], ref["planes"])):
        for q in (3, 1, 2, 0):                                           # Lt, then what is derived from it
            _same(g[q], r[q], f"{what}, level {level}, plane {PLANES[q]}")
    _lists_equal(got, ref, what)


def _head_equals_run(a, b, what):
    for k in ("hmax_bits", "hist", "inv_k2"):
        _same(a[k], b[k], f"{what}, {k}")
    for level, (g, r) in enumerate(zip(a["planes"], b["planes"])):
        for q in range(4):
            _same(g[q], r[q], f"{what}, level {level}, plane {PLANES[q]}")
    _lists_equal(a, b, what)


def _lists_of(res):
    """(n_cand, lists) of the extrema entry as a dict"""
    return dict(n_cand=res[0], lists=res[1])


def _check_single(case, out, what):
    if case["kind"] == "image":
        _head_equals_reference(out["images"][0], T.reference(case), what)
    else:
        _lists_equal(_lists_of(out["images"][0]), T.reference(case), what)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_head_equals_the_reference(case, tmp_path_factory):
    res = _family(case["family"], tmp_path_factory)
    out = res[("single", case["name"])]
    if case.get("plan_proof"):
        case["plan_proof"](case, out["plan"])                            # the plan the entry reports it used: the seams fall where the case says
    _check_single(case, out, case["name"])


@pytest.mark.parametrize("batch", BATCHES, ids=[b[0] for b in BATCHES])
def test_batch_equals_the_single_calls(batch, tmp_path_factory):
    name, family, kind, thr, items = batch
    res = _family(family, tmp_path_factory)
    got = res[("batch", name)]["images"]
    assert len(got) == 3
    singles = {(c["image"], float(c["thr"])) if c["kind"] == "image" else c["name"]: c["name"] for c in CASES}
    for b, item in enumerate(items):
        what = f"{name}, image {b}"
        if kind == "image":
            _head_equals_reference(got[b], T.head_reference(item, thr), f"{what} ({item})")
            if (item, float(thr)) in singles:
                _head_equals_run(got[b], res[("single", singles[(item, float(thr))])]["images"][0], f"{what} ({item}) against its single call")
        else:
            _lists_equal(_lists_of(got[b]), T.reference(item), f"{what} ({item['name']})")
            if item["name"] in singles:
                _lists_equal(_lists_of(got[b]), _lists_of(res[("single", item["name"])]["images"][0]), f"{what} ({item['name']}) against its single call")


@pytest.mark.parametrize("variant,case", VARIANT_RUNS, ids=[f"{v}-{c['name']}" for v, c in VARIANT_RUNS])
def test_launch_form_equals_the_reference(variant, case, tmp_path_factory):
    res = _family(f"variant:{variant}", tmp_path_factory, T.VARIANTS[variant])
    out = res[("single", case["name"])]
    if case["kind"] == "image":
        T.variant_plan_proof(variant, out["plan"])                       # the form ran: the entry reports the plan it used
    _check_single(case, out, f"{variant}: {case['name']}")


def test_product_detector_still_equals_the_oracle():
    """the product library, in this process: r3dm_detect_akaze runs ak_scale_space (ak_level_plan's launches) and ak_head_launches, the
    functions the developer entries share with it -- the keypoints of the 163 x 121 noise image against the oracle's detector"""
    from regard3d_amd import api
    img = np.ascontiguousarray(T.image("noise-163x121"))
    ctx = api.Context(0)
    try:
        kps, resp = ctx.detect_akaze(img, 1e-7)
    finally:
        ctx.close()
    o = T.O.akaze_detect(img, 1e-7)
    assert len(o["kps"]) >= 50, "tens of keypoints on the noise image"
    _same(kps, o["kps"], "keypoints"); _same(resp, o["responses"], "responses")
