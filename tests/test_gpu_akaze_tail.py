"""The Fast-A-KAZE tail on the GPU, on planes and lists built for its edges (tests/akaze_tail_cases.py): the
developer build's r3dm_dev_akaze_tail runs the PRODUCT's code -- ak_tail_launches (list ranges, both cross-level passes, refinement +
orientation, compaction), the host's angle and item formation and ak_describe_pass, the functions the detector calls -- on the caller's
planes and lists.  The reference of every case is oracle/akaze.c's orc_akaze_tail alone, and the comparison is bit for bit: the count,
the seven record fields, theta, cos and sin, the descriptor rows, and the dead_lower / dead_upper flags of every list entry.  Every case
also rides in a call of B = 3 with an empty image in the middle: the batch equals the single calls image for image.

The developer library is loaded in child processes (the session's process holds the product library): one child per family of cases,
one alive at a time, each under its own timeout.  A child that ends by a signal, at its timeout or with a HIP error fails its test
and sets _GPU_BROKEN: the module's remaining tests skip and start no further child.  There are no retries."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import akaze_tail_cases as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = T.all_cases()
BATCHES = T.batches()
RECORD = ("x", "y", "size", "response", "max_x", "max_y", "level")
ANGLES = ("theta", "cos", "sin")

_GPU_BROKEN = None                                 # the reason, once a child died, hung or reported a HIP error
_RESULTS = {}                                      # family -> {("single", case name) | ("batch", batch name): per-image results}
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
    op = str(tmp_path_factory.mktemp(f"tail_{family}") / "out.pkl")
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; import akaze_tail_cases as T; "
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
        if r.returncode < 0 or "HIP" in why.upper() or "r3dm_dev_akaze_tail -> -3" in why:
            _GPU_BROKEN = f"family {family!r}: exit {r.returncode}: {why}"
        _FAILED[family] = f"the child of family {family!r} ended with {r.returncode}: {why}"
        pytest.fail(_FAILED[family])
    _RESULTS[family] = res
    return res


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), (what, np.flatnonzero(a.ravel() != b.ravel())[:8].tolist() if a.shape == b.shape else (a.shape, b.shape))


def _equals_reference(got, ref, what):
    for level, (g, r) in enumerate(zip(got["dead"], ref["dead"])):     # first: a mismatch here points at the pass that made it
        _same(g[:, 0], r[:, 0], (what, "dead_lower", level)); _same(g[:, 1], r[:, 1], (what, "dead_upper", level))
    assert got["n"] == ref["n"], (what, "count", got["n"], ref["n"])
    for k in RECORD:
        _same(got[k], ref[k].astype(np.uint32) if k == "level" else ref[k], (what, k))
    for k in ANGLES:
        _same(got[k], ref[k], (what, k))
    _same(got["desc"], ref["desc"], (what, "desc"))


def _equals_run(a, b, what):
    assert a["n"] == b["n"], (what, "count")
    for k in RECORD + ANGLES + ("desc",):
        _same(a[k], b[k], (what, k))
    for level, (g, r) in enumerate(zip(a["dead"], b["dead"])):
        _same(g, r, (what, "dead", level))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_tail_equals_the_reference(case, tmp_path_factory):
    res = _family(case["family"], tmp_path_factory)
    _equals_reference(res[("single", case["name"])][0], T.reference(case), case["name"])


@pytest.mark.parametrize("batch", BATCHES, ids=[b[0] for b in BATCHES])
def test_batch_equals_the_single_calls(batch, tmp_path_factory):
    name, family, cases = batch
    res = _family(family, tmp_path_factory)
    got = res[("batch", name)]
    assert len(got) == 3
    for b, c in enumerate(cases):
        _equals_reference(got[b], T.reference(c), (name, b, c["name"]))
        _equals_run(got[b], res[("single", c["name"])][0], (name, b, c["name"]))


def test_product_detector_still_equals_the_oracle():
    """the product library, in this process: r3dm_detect_akaze_mldb calls ak_tail_launches and ak_item, the functions the developer
    entry shares with it -- keypoints and descriptors of one scene of the MLDB arm's cases against the oracle's detector"""
    import mldb_arm_cases as M
    from regard3d_amd import api
    thr, ims = M.batch_images((240, 320))
    img = np.ascontiguousarray(ims[0], np.float32)
    ctx = api.Context(0)
    try:
        kps, desc = ctx.detect_akaze_mldb(img, thr)
    finally:
        ctx.close()
    okps, odesc, _ = T.O.akaze_detect_mldb(img, thr)
    assert len(okps) >= 20, "tens of keypoints, as tests/mldb_arm_cases.py builds the scene"
    _same(kps, okps, "keypoints"); _same(desc, odesc, "descriptors")
