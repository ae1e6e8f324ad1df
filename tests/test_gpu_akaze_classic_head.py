"""The classic A-KAZE head on the GPU, plane by plane, on images and determinant planes built for its edges
(tests/akaze_classic_head_cases.py; DESIGN.md section 7, "The head, plane by plane"): the developer build's r3dm_dev_akaze_classic_head
runs the PRODUCT's code -- ac_scale_space and ac_find_extrema, the functions the detector calls -- on the caller's images and reads back
the k-contrast words, Lsmooth, Lflow, Lt, Lx, Ly and Ldet of every level, the per-level counts and the candidates in scan order;
r3dm_dev_akaze_classic_extrema runs ac_find_extrema on the caller's determinant planes.  The reference of every case is
tests/akaze_classic_restatement.py alone, and every comparison is bit for bit (a NaN against a NaN agrees whatever its payload and
sign: the flat image), list order included.  Every image and every set of planes also rides in a call of B = 3 with the flat image
(planes without a candidate) in the middle: the batch equals the references and the single calls image for image.

The developer library is loaded in child processes (the session's process holds the product library): one child per family of cases,
one alive at a time, each under its own timeout.  A child that ends by a signal, at its timeout or with a HIP error fails its test and
sets _GPU_BROKEN: the module's remaining tests skip and start no further child.  There are no retries."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import akaze_classic_head_cases as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = T.all_cases()
BATCHES = T.batches()

_GPU_BROKEN = None                                 # the reason, once a child died, hung or reported a HIP error
_RESULTS = {}                                      # family -> {("single", case name) | ("batch", batch name): results}
_FAILED = {}                                       # family -> why its child failed (no second child for the same family)


def _family(family, tmp_path_factory):
    """the results of a family's child, started on first use"""
    global _GPU_BROKEN
    if family in _RESULTS:
        return _RESULTS[family]
    if family in _FAILED:
        pytest.fail(_FAILED[family])
    if _GPU_BROKEN:
        pytest.skip(f"an earlier child of this module failed on the GPU: {_GPU_BROKEN}")
    op = str(tmp_path_factory.mktemp("classic_head") / "out.pkl")
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; import akaze_classic_head_cases as T; "
            f"sys.exit(T.child_main({family!r}, {op!r}))")
    env = {k: v for k, v in os.environ.items() if not k.startswith("R3DM_")}
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
    print(f"child of family {family!r}: {res['__seconds__']:.2f} s")
    _RESULTS[family] = res
    return res


def _equal(got, ref, what, planes):
    """bit for bit in pipeline order: a failure names the first stage that differs and its first few (row, column) positions"""
    m = T.first_mismatch(got, ref, planes=planes)
    if m:
        pytest.fail(f"{what}: {m[1]}")


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_head_equals_the_reference(case, tmp_path_factory):
    res = _family(case["family"], tmp_path_factory)
    out = res[("single", case["name"])]
    assert len(out) == 1
    _equal(out[0], T.reference(case), case["name"], case["kind"] == "image")


@pytest.mark.parametrize("batch", BATCHES, ids=[b[0] for b in BATCHES])
def test_batch_equals_the_references_and_the_single_calls(batch, tmp_path_factory):
    name, family, kind, thr, items = batch
    res = _family(family, tmp_path_factory)
    got = res[("batch", name)]
    assert len(got) == 3
    if kind == "image":
        singles = {(c["image"], float(c["thr"])): c["name"] for c in CASES if c["kind"] == "image"}
    else:
        singles = {c["name"]: c["name"] for c in CASES}
    for b, item in enumerate(items):
        label = item if kind == "image" else item["name"]
        what = f"{name}, image {b} ({label})"
        _equal(got[b], T.head_reference(item, thr) if kind == "image" else T.reference(item), what, kind == "image")
        key = (item, float(thr)) if kind == "image" else item["name"]
        if key in singles:
            _equal(got[b], res[("single", singles[key])][0], f"{what} against its single call", kind == "image")
    assert any(key in singles for key in ((i, float(thr)) if kind == "image" else i["name"] for i in items))
    totals = [len(g["value"]) for g in got]
    assert totals[1] == 0 and max(totals) >= totals[1], "the middle image has no candidate: the stride is another image's"


def test_product_detector_still_equals_the_restatement():
    """the product library, in this process: r3dm_detect_akaze_classic runs ac_scale_space and ac_find_extrema, the functions the
    developer entries share with it -- the keypoints of the 163 x 83 noise image at 1e-4 against R.detect"""
    from regard3d_amd import api
    img = np.ascontiguousarray(T.image("noise-163x83"))
    ctx = api.Context(0)
    try:
        kps, resp = ctx.detect_akaze_classic(img, 1e-4)
    finally:
        ctx.close()
    ref = T.R.detect(img, 1e-4)
    assert len(ref["kps"]) >= 10, "keypoints survive the descriptor border on the 163 x 83 image"
    assert kps.shape == ref["kps"].shape and kps.tobytes() == ref["kps"].tobytes() and resp.tobytes() == ref["responses"].tobytes()
