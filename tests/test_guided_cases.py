"""The guided-matching edge cases (guided_cases.py) reach their edges: CPU only, on the restatement alone.

Per case: its proof (the edge it is named for, decided by the oracle's error functions through guided_restatement.candidates), and,
where the sweep's f32 gate applies,
  (a) gate_model with the kernel's constants hands every (i, j) the restatement accepts to the f64 test -- with f32 denormals kept and
      flushed; a failure here is a finding about the bound in kernels_guided.hip, not about the case;
  (b) slack family: the same gate without its slack (rel = abs = 0) loses at least 5 % of the restatement's candidates;
  (c) slack family: the gate with the kernel's constants rejects at least 90 % of all (i, j) -- the case is not served by exact_all.
The measured counts are printed (pytest -s).  One test holds the model's constants to the kernel's text."""
import os
import re

import numpy as np
import pytest

import guided_cases as C
import guided_restatement as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True, scope="module")
def _oracle(oracle):
    return oracle


@pytest.mark.parametrize("case", C.CASES, ids=C.NAMES)
def test_case_reaches_its_edge(case):
    cand = C.candidates_of(case)
    mask = C.candidate_mask(case, cand)
    gate = C.gate_of(case)
    out = case["proof"](case, cand, gate)
    n = int(mask.sum())
    k, M = C.model_of(case)
    assert n == G.candidate_count(case["kind"], case["M"], case["thr_px"], case["xyI"], case["xyJ"], case["KI"], case["KJ"])
    # (a) the kernel's gate loses nothing, whether f32 denormals are kept or flushed
    lost = int((mask & ~gate).sum())
    lost_ftz = int((mask & ~C.gate_of(case, ftz=True)).sum())
    share = 1.0 - float(gate.mean()) if gate.size else 0.0
    print(f"\n{case['name']}: candidates {n}, lost with the kernel's constants {lost} (denormals flushed: {lost_ftz}), "
          f"gate rejects {100 * share:.2f} % of {gate.size} (i, j); {out}")
    assert lost == 0 and lost_ftz == 0, (case["name"], lost, lost_ftz)
    if case["family"] == "slack":
        bare = C.gate_of(case, rel=0.0, abs_=0.0)
        lost_bare = int((mask & ~bare).sum())
        print(f"{case['name']}: lost without slack {lost_bare} of {n} ({100 * lost_bare / n:.1f} %)")
        if case["name"] in C.SLACK_LOSSLESS:
            assert lost_bare == 0                                   # (guided_cases.py: a threshold on the positions' lattice)
        else:
            assert lost_bare >= 0.05 * n, (case["name"], lost_bare, n)          # (b)
        assert share >= 0.9 and not C.exact_all_tiles(k, M, case["xyI"], case["xyJ"], C.err_th(case)).any()          # (c)


def test_every_family_and_shape_is_in_the_table():
    fam = {c["family"] for c in C.CASES}
    assert fam == set(C.FAMILIES)
    shapes = [(len(c["xyI"]), len(c["xyJ"])) for c in C.CASES if c["family"] == "shapes"]
    assert {a for a, _ in shapes} == set(C.N_I) | {257} and {b for _, b in shapes} == set(C.N_J)
    assert {c["kind"] for c in C.CASES} == {"F", "H", "E"}
    kinds = {(c["descI"].dtype.name, c["binary"]) for c in C.CASES if c["family"] == "ties" and c["ratio"] >= 0}
    assert kinds == {("float32", False), ("uint8", False), ("uint8", True)}
    assert all(c["descI"].shape[1] == 61 for c in C.CASES if c["binary"])
    assert all(len(c["xyI"]) <= 1500 for c in C.CASES)


def test_many_pairs_case_maps_blocks_to_jobs():
    """>= 70 jobs of 0 .. 4 workgroups each in one call; views of one feature; an empty view in the middle and at the end of the view
    list, as I (a job without workgroups, also as the LAST job) and as J"""
    m = C.many_pairs_case()
    sizes = [len(xy) for xy, _ in m["views"]]
    blocks = [-(-sizes[int(I)] // C.BLOCK) for I, _ in m["pairs"]]
    assert len(m["pairs"]) >= 70 and set(blocks) == {0, 1, 2, 3, 4}
    assert sizes[-1] == 0 and 0 in sizes[1:-1] and 1 in sizes
    assert blocks[-1] == 0 and blocks[0] == 1 and any(sizes[int(J)] == 0 for _, J in m["pairs"])
    key = m["pairs"][:, 0].astype(np.uint64) << np.uint64(32) | m["pairs"][:, 1].astype(np.uint64)
    assert np.all(key[1:] > key[:-1])
    total, kept = 0, {r: 0 for r in m["ratios"]}
    for (I, J), M, t in zip(m["pairs"].tolist(), m["models"], m["thrs"]):
        total += G.candidate_count("H", M, t, m["views"][I][0], m["views"][J][0])
        for r in m["ratios"]:
            kept[r] += len(G.guided_pair("H", M, t, r, m["views"][I][0], m["views"][J][0], m["views"][I][1], m["views"][J][1])) > 0
    print(f"\nshapes_many_pairs: {len(blocks)} jobs, {sum(blocks)} workgroups, {total} candidates, pairs with matches {kept}")
    assert total > 1000 and all(20 < k < len(blocks) for k in kept.values())          # both modes keep pairs and drop pairs


def test_gate_model_is_per_tile():
    """the model's Xmax / Ymax and exact_all are per tile of J: one far position changes its own tile only"""
    r = np.random.default_rng(7)
    xyI = r.uniform(0, 100, (5, 2)).astype(np.float32); xyJ = r.uniform(0, 100, (24, 2)).astype(np.float32)
    xyJ[9] = (2e7, 50)
    Hm = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], np.float64)
    g = C.gate_model("H", Hm, xyI, xyJ, 1.0, tile=8)
    assert g[:, 8:16].all() and not g[:, :8].all() and not g[:, 16:].all()
    assert C.exact_all_tiles("H", Hm, xyI, xyJ, 1.0, tile=8).tolist() == [[False, True, False]] * 5
    # without slack the gate is |x - f32(px)| <= f32(thr) exactly
    bare = C.gate_model("H", Hm, np.array([[10, 10]], np.float32), np.array([[11, 10], [11.000001, 10], [10, 9]], np.float32), 1.0, rel=0.0, abs_=0.0)
    assert bare.tolist() == [[True, False, True]]


def test_model_constants_are_the_kernels():
    """2^-20, 1e-30, 1e30, 1e7 and the tile of 4096 positions, read from the kernel's text"""
    src = open(os.path.join(ROOT, "regard3d_amd", "csrc", "kernels_guided.hip")).read()
    hdr = open(os.path.join(ROOT, "regard3d_amd", "csrc", "r3dm_internal.hpp")).read()
    rel = re.search(r"constexpr float kGateRel = ([0-9.eE+-]+)f;", src)
    ab = re.search(r"constexpr float kGateAbs = ([0-9.eE+-]+)f;", src)
    tile = re.search(r"constexpr uint32_t kGuidedTile = (\d+);", hdr)
    assert rel and ab and tile
    assert float(rel.group(1)) == C.GATE_REL == 2.0 ** -20 and np.float32(ab.group(1)) == np.float32(C.GATE_ABS)
    assert int(tile.group(1)) == C.TILE == 4096
    # the escapes: three coefficients and T below 1e30 (F), two and T (H); both tile maxima below 1e7
    assert src.count("< 1e30") == 7 and len(re.findall(r"fabs\(a[012]\) < 1e30", src)) == 5 and src.count("T < 1e30") == 2
    assert "!(gate_ok && Xm < 1e7f && Ym < 1e7f)" in src
    assert C.COEF_LIMIT == 1e30 and C.POS_LIMIT == 1e7
    # the slack terms as the model applies them
    assert "T32 = (float)T * (1.0f + kGateRel)" in src
    assert "T32 + (fabsf(f0) * Xm + fabsf(f1) * Ym + fabsf(f2)) * kGateRel + kGateAbs" in src
    assert "limx = T32 + (fabsf(f0) + Xm) * kGateRel + kGateAbs, limy = T32 + (fabsf(f1) + Ym) * kGateRel + kGateAbs" in src
    assert "dim3(256)" in src and C.BLOCK == 256
