"""The candidate lists of tests/akaze_classic_walk_cases.py contain what they were built for, asserted from the serial restatement alone
(R.offer / R.upper_filter); and the developer build's walk entry refuses, without a GPU, what the kernels would mis-read.  CPU only.
The GPU side is tests/test_gpu_akaze_classic_walk.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import akaze_classic_restatement as R
import akaze_classic_walk_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = W.all_cases()
INVALID = -1                                  # R3DM_ERR_INVALID (include/r3dm.h)
OPS = {"==": lambda a, b: a == b, ">=": lambda a, b: a >= b, ">": lambda a, b: a > b}


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_case_contains_what_it_was_built_for(case):
    aux, kept, outcomes, ev = W.case_events(case)
    print(case["name"], outcomes if len(outcomes) <= 64 else f"({len(outcomes)} candidates)", {k: int(v) for k, v in ev.items() if v})
    assert case["events"], "a case states the events it must contain"
    for name, (op, count) in case["events"].items():
        assert OPS[op](int(ev.get(name, 0)), count), (name, op, count, int(ev.get(name, 0)))
    if case["outcomes"] is not None:
        assert outcomes == case["outcomes"]
    # what trace() returns IS the reference: the same slots and survivors as the plain replay
    ref = W.reference(case)
    n = aux.n
    assert n == len(ref["x"]) and np.array_equal(aux.x[:n], ref["x"]) and np.array_equal(aux.resp[:n], ref["resp"])
    assert np.array_equal(np.flatnonzero(ref["kept"]), kept)
    for lst in case["lists"]:
        assert len(lst) <= 8200 and all(c[0] < len(case["levels"]) for c in lst)


def test_the_cases_cover_the_families_of_the_issue():
    names = [c["name"] for c in CASES]
    for n in (2, 63, 64, 65, 66, 130):
        for two in ("one", "two"):
            for pattern in ("increasing", "decreasing", "random"):
                assert f"run-{n}-{two}-{pattern}" in names
    for b in (1, 2, 3, 7):
        case = CASES[names.index(f"bound-{b}")]
        assert (1, b) in case["forms"]
    for n in (0, 1, 255, 256, 257, 1023, 1024, 1025, 2049):
        assert len(CASES[names.index(f"length-{n}")]["lists"][0]) == n
    batch = CASES[names.index("batch")]
    assert [len(l) for l in batch["lists"]] == [2049, 0, 1]
    assert sum(n.startswith("random-") for n in names) == 24 and sum(n.startswith("boundary-") for n in names) == 4
    assert all(set(W.FORMS) <= set(c["forms"]) for c in CASES)
    assert CASES[names.index("contention")]["repeats"] == 3
    assert {c["group"] for c in CASES} == {"families", "sizes", "edges", "lengths", "contention"}        # a handful of children


@pytest.mark.parametrize("name", ["random-3-2", "boundary-1", "chain", "border-in-cluster", "run-65-two-random", "bound-3", "moved-handback",
                                  "octave-7-8", "mixed-sizes"])
def test_component_roots_equal_the_union_find_model(name):
    """the vectorised components of the long lists against components(), the model tests/test_akaze_classic_components.py checks"""
    case = next(c for c in CASES if c["name"] == name)
    cands = case["lists"][0]
    assert np.array_equal(W.component_roots(case["levels"], cands), W.components(case["levels"], cands))


def test_bound_cases_have_components_of_exactly_the_bound_and_one_more():
    for b in (1, 2, 3, 7):
        case = next(c for c in CASES if c["name"] == f"bound-{b}")
        roots = W.components(case["levels"], case["lists"][0])
        sizes = np.bincount(roots[roots >= 0])
        assert (sizes == b).sum() >= 1 and (sizes == b + 1).sum() >= 1


# ---------------------------------------------------------------------------------------------------- the entry's validation, no GPU
def _in_child(fn):
    """the developer library is a second copy of the product library: it is loaded in a child process, never into the session's"""
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; import test_akaze_classic_walk_cases as T; T.{fn}()"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]


def _dev():
    from regard3d_amd import api
    return api, api.bind_dev_akaze_classic_walk(C.CDLL(api.DEV_LIB_PATH))


def _check(dev, levels, w, h, lists, parallel=1, bound=64, n_levels=None):
    api, L = dev
    lv, n_cand, words = api.dev_walk_args(levels, lists)
    return L.r3dm_dev_akaze_classic_walk_check(C.addressof(lv), len(levels) if n_levels is None else n_levels, w, h, len(lists),
                                               api._ptr(n_cand), api._ptr(words), parallel, bound)


def test_walk_entry_is_a_developer_build_entry_only():
    from regard3d_amd import api
    assert "r3dm_dev_akaze_classic_walk" not in api.EXPORTS
    syms = subprocess.run(["nm", "-D", os.path.join(ROOT, "regard3d_amd", "libr3dm.so")], capture_output=True, text=True).stdout
    assert "r3dm_dev_" not in syms
    dsyms = subprocess.run(["nm", "-D", api.DEV_LIB_PATH], capture_output=True, text=True).stdout
    assert "r3dm_dev_akaze_classic_walk" in dsyms
    for hdr in os.listdir(os.path.join(ROOT, "include")):
        assert "r3dm_dev_" not in open(os.path.join(ROOT, "include", hdr)).read(), hdr
    with pytest.raises(api.R3dmError):
        api.bind_dev_akaze_classic_walk(api.load_library())


def test_walk_entry_refuses_what_the_kernels_would_misread():
    """before any launch and without a device: R3DM_ERR_INVALID"""
    _in_child("_validation_checks")


def _validation_checks():
    dev = _dev()
    api, L = dev
    lv = R.levels(480, 400)[:8]
    good = [(0, 100, 100, 0.004), (0, 100, 102, 0.004), (0, 101, 50, 0.003), (4, 60, 60, 0.002)]
    assert _check(dev, lv, 480, 400, [good]) == 0
    assert _check(dev, lv, 480, 400, [good, [], good[:1]]) == 0
    assert _check(dev, lv, 480, 400, [[]]) == 0
    for case in W.all_cases()[::7]:                                   # the cases of the suite pass it
        for parallel, bound in case["forms"]:
            assert _check(dev, case["levels"], case["w"], case["h"], case["lists"], parallel, bound) == 0, case["name"]
    # the order: strict scan order (level, row, column)
    for bad in ([good[1], good[0]], [good[0], good[0]], [good[2], good[0]], [good[3], good[0]]):
        assert _check(dev, lv, 480, 400, [bad]) == INVALID
    assert _check(dev, lv, 480, 400, [good, [good[1], good[0]]]) == INVALID          # in a later image of the batch too
    # the rim and beyond (level 4 is 240 x 200)
    for c in [(0, 0, 100, .1), (0, 399, 100, .1), (0, 100, 0, .1), (0, 100, 479, .1), (0, 400, 100, .1), (4, 199, 100, .1), (4, 100, 239, .1), (4, 100, 300, .1)]:
        assert _check(dev, lv, 480, 400, [[c]]) == INVALID, c
    for c in [(0, 1, 1, .1), (0, 398, 478, .1), (4, 198, 238, .1)]:
        assert _check(dev, lv, 480, 400, [[c]]) == 0, c
    assert _check(dev, lv, 480, 400, [[(8, 50, 50, .1)]]) == INVALID                  # a level the table does not have
    for v in (float("nan"), float("inf"), -float("inf")):
        assert _check(dev, lv, 480, 400, [[(0, 100, 100, v)]]) == INVALID
    for bound in (0, 65, 1 << 31):
        assert _check(dev, lv, 480, 400, [good], 1, bound) == INVALID
    assert _check(dev, lv, 480, 400, [good], 2, 64) == INVALID
    assert _check(dev, lv, 480, 400, []) == INVALID and _check(dev, lv, 480, 400, [good], n_levels=0) == INVALID
    assert _check(dev, R.levels(1400, 1000) + lv[:1], 1400, 1000, [[]]) == INVALID          # 17 levels
    # level tables: a cell side below 3 (size 1.5 esigma < 2), a level larger than the image, ratios below 1, non-finite scales
    ok = dict(w=120, h=100, octave=0, esigma=2.0, ratio=1.0)
    assert _check(dev, [ok], 120, 100, [[]]) == 0
    for change in (dict(esigma=1.3), dict(esigma=float("nan")), dict(esigma=-2.0), dict(ratio=0.5), dict(ratio=float("inf")), dict(w=121), dict(h=101),
                   dict(w=2), dict(octave=-1), dict(octave=7, ratio=128.0), dict(ratio=2.0), dict(octave=1), dict(ratio=3.0)):
        assert _check(dev, [dict(ok, **change)], 120, 100, [[]]) == INVALID, change
    assert _check(dev, [dict(ok, ratio=2.0, w=60, h=50, octave=1)], 120, 100, [[]]) == 0
    assert _check(dev, [dict(ok, ratio=2.0, w=61, h=50, octave=1)], 120, 100, [[]]) == INVALID
    # null pointers, and a null context with everything else in order (what a host holds after a failed r3dm_create)
    lvs, n_cand, words = api.dev_walk_args(lv, [good])
    assert L.r3dm_dev_akaze_classic_walk_check(None, 8, 480, 400, 1, api._ptr(n_cand), api._ptr(words), 1, 64) == INVALID
    assert L.r3dm_dev_akaze_classic_walk_check(C.addressof(lvs), 8, 480, 400, 1, None, api._ptr(words), 1, 64) == INVALID
    assert L.r3dm_dev_akaze_classic_walk_check(C.addressof(lvs), 8, 480, 400, 1, api._ptr(n_cand), None, 1, 64) == INVALID
    n_slots = np.zeros(1, np.uint32); out = np.zeros((4, 6), np.uint32)
    assert L.r3dm_dev_akaze_classic_walk(None, C.addressof(lvs), 8, 480, 400, 1, api._ptr(n_cand), api._ptr(words), 1, 64,
                                         api._ptr(n_slots), api._ptr(out), None) == INVALID
    assert L.r3dm_dev_akaze_classic_walk(None, None, 0, 0, 0, 0, None, None, 0, 0, None, None, None) == INVALID
