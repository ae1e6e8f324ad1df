"""The M-SURF-64 kernel on the GPU, on planes and items built for its edges (tests/msurf_cases.py: kernel_cases):
the developer build's r3dm_dev_akaze_msurf runs the PRODUCT's kernel (ak_levels with the M-SURF border, ak_buffers, ak_level_table,
ak_describe_launch) on the caller's Lx / Ly planes and items, after r3dm_dev_akaze_msurf_check has accepted them.  The reference of every case
is the serial restatement tests/cpp/msurf_restatement.cpp in its ak_expf form, and the comparison is bit for bit, a row of a window
without gradient as "all NaN".

Cases: a keypoint at border - 1 and at dim - border at 0, 45, 90, 225 degrees on every level (sigma_size 2, 3, 4; two octaves), sample
coordinates on .5 boundaries, angles exactly 0 and pi, planes of one sign and of alternating sign, windows without gradient between
windows with, launches of 0, 1, one workgroup's worth (four keypoints) -1 / +0 / +1 and several workgroups' worth.  Plane sizes: 96 x 128 (one level)
and 160 x 192 with 80 x 96 (five levels); a 48 x 64 image has no level under the M-SURF border, the check refuses it
(tests/test_msurf_cases.py, which also holds each refusal of the check without a device).

The developer library is loaded in ONE child process (the session's process holds the product library), under its own timeout.  A child
that ends by a signal, at its timeout or with a HIP error fails its test and the module's remaining tests skip.  There are no retries."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import msurf_cases as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = S.kernel_cases()

_STATE = {}                                        # "res": {case name: rows} | "failed": why


def _results(tmp_path_factory):
    if "failed" in _STATE:
        pytest.skip(f"the child of this module failed on the GPU: {_STATE['failed']}")
    if "res" in _STATE:
        return _STATE["res"]
    op = str(tmp_path_factory.mktemp("msurf_kernel") / "out.pkl")
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; import msurf_cases as S; sys.exit(S.child_main({op!r}))")
    env = {k: v for k, v in os.environ.items() if not k.startswith("R3DM_")}
    try:
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    except subprocess.TimeoutExpired:
        _STATE["failed"] = "the child did not end within its timeout"
        pytest.fail(_STATE["failed"])
    res = pickle.load(open(op, "rb")) if os.path.exists(op) else {}
    if r.returncode != 0 or "__error__" in res:
        _STATE["failed"] = f"the child ended with {r.returncode}: {res.get('__error__', r.stderr[-2000:])}"
        pytest.fail(_STATE["failed"])
    _STATE["res"] = res
    return res


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_kernel_equals_the_restatement_bit_for_bit(case, tmp_path_factory):
    got = _results(tmp_path_factory)[case["name"]]
    ref = S.kernel_reference(case)
    assert got.shape == ref.shape == (len(case["items"]), 64)
    nan = np.isnan(got).all(axis=1)
    assert np.flatnonzero(nan).tolist() == case["nan_rows"]                        # 0 / 0 for a window without gradient, nowhere else
    assert not np.isnan(got[~nan]).any()
    diff = np.flatnonzero((got[~nan].view(np.uint32) != ref[~nan].view(np.uint32)).any(axis=1))
    assert S.same_rows(got, ref), (case["name"], "rows that differ:", diff[:8].tolist())


def test_the_cases_are_the_ones_the_kernel_can_go_wrong_on():
    names = {c["name"] for c in CASES}
    for tag in ("96x128", "160x192"):
        assert {f"border-{tag}", f"half-{tag}", f"angles-{tag}", f"one_sign-{tag}", f"alternating-{tag}", f"nan_row-{tag}", f"all_zero-{tag}"} <= names
    w = S.KP_PER_GROUP
    assert {f"count-{n}" for n in (0, 1, w - 1, w, w + 1, 4 * w + 1)} <= names
    big = next(c for c in CASES if c["name"] == "border-160x192")
    assert sorted({int(s) for s in big["items"][:, 5]}) == [2, 3, 4] and {e["ratio"] for e in big["levels"]} == {1.0, 2.0}
    for c in CASES:
        if c["name"].startswith("border-"):                                        # both ends of the accepted range, in both coordinates
            for i, e in enumerate(c["levels"]):
                it = c["items"][c["items"][:, 0] == i]
                assert it[:, 1].min() == e["border"] - 1 and it[:, 1].max() == e["w"] - e["border"]
                assert it[:, 2].min() == e["border"] - 1 and it[:, 2].max() == e["h"] - e["border"]
        if c["name"].startswith("one_sign-"):                                      # dx == mdx needs the rotated responses of one sign: angle 0 has them
            rows = S.kernel_reference(c)
            assert (rows[0::2, 0::4] == rows[0::2, 2::4]).all() and (rows[0::2, 1::4] == rows[0::2, 3::4]).all()
        if c["name"].startswith("alternating-"):
            rows = S.kernel_reference(c)
            assert (np.abs(rows[:, 0::4]) < 0.5 * rows[:, 2::4]).mean() > 0.5, "the signed sums cancel where the absolute sums do not"


def test_product_entry_still_equals_the_reference_chain(ctx):
    """the product library, in this process: r3dm_detect_akaze_msurf runs ak_describe_launch and the kernel the developer entry shares with it"""
    thr, ims, ref = S.batch_refs((120, 160))
    kps, rows = ctx.detect_akaze_msurf_batch(ims[:1], thr, single=True)[0]
    assert len(kps) >= 15 and kps.tobytes() == ref[0]["kps"].tobytes() and S.same_rows(rows, ref[0]["rows"])
