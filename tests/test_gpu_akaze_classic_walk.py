"""The classic A-KAZE kpts_aux walk on the GPU, on candidate lists built for its edges (tests/akaze_classic_walk_cases.py; DESIGN.md
section 4.17): the developer build's r3dm_dev_akaze_classic_walk runs the PRODUCT's kernels (ac_walk of api_akaze_classic.cpp, the
function the detector calls) on the caller's lists.  The reference of every case is the serial restatement alone -- R.offer over the
list, then R.upper_filter -- and the comparison is bit for bit: n_slots, x, y, size, response and class of every slot, and the kept
set, in three forms (the parallel form with bound 64, with bound 1, the one-wavefront form; some cases add a bound of their own).

The developer library is loaded in child processes (the session's process holds the product library): one child per group of cases,
one alive at a time, each under its own timeout.  A child that ends by a signal, at its timeout or with a HIP error fails its test
and sets _GPU_BROKEN: the module's remaining tests skip and start no further child."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import akaze_classic_walk_cases as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = W.all_cases()
FIELDS = ("x", "y", "size", "resp", "cls", "kept")

_GPU_BROKEN = None                                 # the reason, once a child died, hung or reported a HIP error
_RESULTS = {}                                      # group -> {(case name, form index, repeat): per-image results}
_FAILED = {}                                       # group -> why its child failed (no second child for the same group)


def _jobs(group):
    jobs = []
    for c in CASES:
        if c["group"] != group:
            continue
        for f, (parallel, bound) in enumerate(c["forms"]):
            for rep in range(c["repeats"] if parallel and bound == 64 else 1):
                jobs.append(((c["name"], f, rep), c["levels"], c["w"], c["h"], c["lists"], parallel, bound))
                if len(c["lists"]) > 1:             # the batch: every image in a call of its own too
                    for b, lst in enumerate(c["lists"]):
                        jobs.append(((c["name"], f, ("single", b)), c["levels"], c["w"], c["h"], [lst], parallel, bound))
    return jobs


def _group(group, tmp_path_factory):
    """the results of a group's child, started on first use"""
    global _GPU_BROKEN
    if group in _RESULTS:
        return _RESULTS[group]
    if group in _FAILED:
        pytest.fail(_FAILED[group])
    if _GPU_BROKEN:
        pytest.skip(f"an earlier child of this module failed on the GPU: {_GPU_BROKEN}")
    d = tmp_path_factory.mktemp(f"walk_{group}")
    jp, op = str(d / "jobs.pkl"), str(d / "out.pkl")
    pickle.dump(_jobs(group), open(jp, "wb"))
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; import akaze_classic_walk_cases as W; "
            f"sys.exit(W.child_main({jp!r}, {op!r}))")
    env = {k: v for k, v in os.environ.items() if not k.startswith("R3DM_")}
    try:
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    except subprocess.TimeoutExpired:
        _GPU_BROKEN = _FAILED[group] = f"the child of group {group!r} did not end within its timeout"
        pytest.fail(_GPU_BROKEN)
    res = pickle.load(open(op, "rb")) if os.path.exists(op) else {}
    if r.returncode < 0 or "__error__" in res or r.returncode != 0:
        why = res.get("__error__", r.stderr[-2000:])
        if r.returncode < 0 or "HIP" in why.upper() or "r3dm_dev_akaze_classic_walk -> -3" in why:
            _GPU_BROKEN = f"group {group!r}: exit {r.returncode}: {why}"
        _FAILED[group] = f"the child of group {group!r} ended with {r.returncode}: {why}"
        pytest.fail(_FAILED[group])
    _RESULTS[group] = res
    return res


def _equal(got, ref, what):
    assert len(got["x"]) == len(ref["x"]), (what, "n_slots", len(got["x"]), len(ref["x"]))
    for f in FIELDS:
        a, b = np.asarray(got[f]), np.asarray(ref[f])
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (what, f, np.flatnonzero(a != b)[:8].tolist())


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_walk_equals_the_serial_restatement(case, tmp_path_factory):
    res = _group(case["group"], tmp_path_factory)
    for f, (parallel, bound) in enumerate(case["forms"]):
        form = f"{'parallel' if parallel else 'one wavefront'}, bound {bound}"
        runs = [res[(case["name"], f, rep)] for rep in range(case["repeats"] if parallel and bound == 64 else 1)]
        for b in range(len(case["lists"])):
            ref = W.reference(case, b)
            for got in runs:
                _equal(got[b], ref, (case["name"], form, f"image {b}"))
            for got in runs[1:]:                                        # repeated runs in one process: identical bytes
                assert all(np.asarray(got[b][k]).tobytes() == np.asarray(runs[0][b][k]).tobytes() for k in FIELDS + ("hist",))
            if len(case["lists"]) > 1:                                  # the batch: every image equals its own single call
                single = res[(case["name"], f, ("single", b))][0]
                assert all(np.asarray(runs[0][b][k]).tobytes() == np.asarray(single[k]).tobytes() for k in FIELDS + ("hist",)), (form, b)


@pytest.mark.parametrize("name", ["run-64-one-random", "run-65-one-random", "mixed-sizes", "bound-3", "length-0"])
def test_component_histogram_of_the_parallel_form(name, tmp_path_factory):
    """the histogram the parallel form reports is the restated components' (bin k: sizes in [2^k, 2^(k+1))); the one-wavefront form
    reports none.  With bound 64 a component of 64 is walked by one wavefront and one of 65 is handed back: both give the slots above."""
    case = next(c for c in CASES if c["name"] == name)
    res = _group(case["group"], tmp_path_factory)
    roots = W.component_roots(case["levels"], case["lists"][0])
    sizes = np.bincount(roots[roots >= 0]) if (roots >= 0).any() else np.zeros(0, np.int64)
    want = np.bincount(np.floor(np.log2(sizes[sizes > 0])).astype(np.int64), minlength=32) if (sizes > 0).any() else np.zeros(32, np.int64)
    for f, (parallel, bound) in enumerate(case["forms"]):
        hist = res[(case["name"], f, 0)][0]["hist"]
        assert np.array_equal(hist, want if parallel else np.zeros(32)), (parallel, bound)
