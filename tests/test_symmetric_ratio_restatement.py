"""The symmetric-ratio restatement (symmetric_ratio_restatement.py) against a brute-force numpy loop on integer rows, the proof that
every case table of the GPU tests (test_gpu_symmetric_ratio.py) reaches its edge -- a match kept, one removed because not nearest, one
that PASSES the mutual rule and is removed by the reverse ratio only -- three wrong implementations each noticed by a named case, and
the interface without a GPU."""
import os
import re

import numpy as np
import pytest

import mutual_restatement as M
import symmetric_ratio_restatement as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pairs(m):
    return [tuple(x) for x in np.asarray(m).tolist()]


def _three_kinds(oracle, dI, dJ, ratio, squared, binary=False):
    """(kept, not nearest, ratio only) of one pair, without positions"""
    off = set(_pairs(S.match_pair(oracle, dI, dJ, None, None, ratio, squared, binary, "off")[0]))
    mut = set(_pairs(S.match_pair(oracle, dI, dJ, None, None, ratio, squared, binary, "mutual")[0]))
    sym, counters = S.match_pair(oracle, dI, dJ, None, None, ratio, squared, binary, "symmetric")
    sym = set(_pairs(sym))
    assert sym <= mut <= off
    assert counters == (len(off), len(off - mut), len(mut - sym))
    return sorted(sym), sorted(off - mut), sorted(mut - sym)


# ---------------------------------------------------------------------------------------------------- the boundary rows
BOUNDARY_CASES = [(64, np.float32, None), (128, np.float32, None), (144, np.float32, None), (256, np.float32, None), (37, np.float32, None),
                  (260, np.float32, None), (128, np.uint8, None), (0, np.uint8, 32), (0, np.uint8, 61)]


@pytest.mark.parametrize("dim,dtype,nbytes", BOUNDARY_CASES)
def test_boundary_rows_against_the_brute_force_loop(oracle, dim, dtype, nbytes):
    dI, dJ, xyI, xyJ = S.boundary_views(dim, dtype, nbytes)
    binary = nbytes is not None
    for mode in S.MODES:
        got, counters = S.match_pair(oracle, dI, dJ, xyI, xyJ, S.BOUNDARY_RATIO, not binary, binary, mode)
        exp, exp_counters = S.brute_force_pair(dI, dJ, xyI, xyJ, S.BOUNDARY_RATIO, not binary, binary, mode)
        assert _pairs(got) == _pairs(exp) and counters == exp_counters, mode
    kept, not_nearest, ratio_only = _three_kinds(oracle, dI, dJ, S.BOUNDARY_RATIO, not binary, binary)
    assert kept == S.BOUNDARY_KEPT and not_nearest == S.BOUNDARY_NOT_NEAREST and ratio_only == S.BOUNDARY_RATIO_ONLY


def test_boundary_distances(oracle):
    """4 against 16 is rejected (4 < 0.25 x 16 is false), 4 against 17 accepted; Hamming 8 against 16 rejected, 8 against 17 accepted"""
    dI, dJ, _, _ = S.boundary_views(64)
    d = lambda i, j: oracle.l2sq(dI[i], dJ[j])
    assert (d(0, 2), d(0, 5), d(1, 40), d(1, 3), d(2, 10), d(2, 11), d(3, 20), d(3, 276)) == (4, 16, 4, 17, 1, 1, 4, 16)
    assert not S.reverse_ratio_passes(4, 16, 0.5, "squared") and S.reverse_ratio_passes(4, 17, 0.5, "squared")
    bI, bJ, _, _ = S.boundary_views(nbytes=32)
    h = lambda i, j: oracle.hamming(bI[i], bJ[j])
    assert (h(0, 2), h(0, 5), h(1, 40), h(1, 3), h(2, 10), h(2, 11)) == (8, 16, 8, 17, 3, 3)
    assert not S.reverse_ratio_passes(8, 16, 0.5, "plain") and S.reverse_ratio_passes(8, 17, 0.5, "plain")
    # where d2's row lies: above / below j, in j's 32-row tile / in another, in j's share of the rows-based kernel's 256 threads
    assert 5 > 2 and 5 // 32 == 2 // 32 and 3 < 40 and 3 // 32 != 40 // 32
    assert 276 % S.ITEMS_THREADS == 20 and 276 // 32 != 20 // 32 and 290 // 32 != 50 // 32


@pytest.mark.parametrize("bug,witness", [("le", (0, 2)), ("bests_only", (3, 20)), ("d2_self", (1, 40))])
def test_three_wrong_implementations_are_each_noticed(bug, witness):
    """<= in the reverse test keeps the 4-against-16 match; a second minimum taken from per-thread bests misses row 276 behind row 20
    of the same share and keeps (3, 20); d2 allowed to be row j itself removes every match, the kept ones included"""
    for dim, nbytes in ((37, None), (64, None), (0, 32)):
        dI, dJ, xyI, xyJ = S.boundary_views(dim, np.float32, nbytes)
        binary = nbytes is not None
        right = _pairs(S.brute_force_pair(dI, dJ, xyI, xyJ, S.BOUNDARY_RATIO, not binary, binary)[0])
        wrong = _pairs(S.brute_force_pair(dI, dJ, xyI, xyJ, S.BOUNDARY_RATIO, not binary, binary, bug=bug)[0])
        assert right == S.BOUNDARY_KEPT
        assert (witness in wrong) != (witness in right), (bug, dim, nbytes)


# ---------------------------------------------------------------------------------------------------- the case tables of the GPU tests
def _collection_has_three_kinds(oracle, descs, pairs, ratio, squared, binary=False):
    c_off, _, _ = S.match_collection(oracle, descs, None, pairs, ratio, squared, binary, "off")
    c_sym, _, (checked, not_nearest, by_ratio) = S.match_collection(oracle, descs, None, pairs, ratio, squared, binary, "symmetric")
    assert checked == c_off.sum() and c_sym.sum() == checked - not_nearest - by_ratio
    assert c_sym.sum() > 0 and not_nearest > 0 and by_ratio > 0, (int(c_sym.sum()), not_nearest, by_ratio)
    return checked, not_nearest, by_ratio


@pytest.mark.parametrize("dim,dtype,nbytes", [(64, np.float32, None), (128, np.float32, None), (144, np.float32, None), (256, np.float32, None),
                                              (37, np.float32, None), (260, np.float32, None), (128, np.uint8, None),
                                              (0, np.uint8, 32), (0, np.uint8, 61)])
def test_ragged_case_tables_reach_all_three_kinds(oracle, dim, dtype, nbytes):
    descs, _ = S.ragged_views(dim, dtype, 100 + dim + (nbytes or 0), nbytes)
    binary = nbytes is not None
    pairs = S.all_ordered_pairs(len(S.ROWS))
    _collection_has_three_kinds(oracle, descs, pairs, S.RAGGED_RATIO if not binary else 0.9, not binary, binary)
    # part 3: no match of a pair whose view J has one row survives, and every accepted match of it counts as a ratio drop
    one_row = np.array([[I, 0] for I in range(1, len(S.ROWS))], np.uint32)
    c_off, _, _ = S.match_collection(oracle, descs, None, one_row, 0.99, not binary, binary, "off")
    c_sym, _, counters = S.match_collection(oracle, descs, None, one_row, 0.99, not binary, binary, "symmetric")
    assert c_off.sum() > 0 and c_sym.sum() == 0 and counters == (int(c_off.sum()), 0, int(c_off.sum()))


def test_ragged_33_rows_against_the_brute_force_loop(oracle):
    dI, dJ, xyI, xyJ = S.ambiguous_views(33, 128, 33)
    for mode in S.MODES:
        got, counters = S.match_pair(oracle, dI, dJ, xyI, xyJ, S.RAGGED_RATIO, True, False, mode)
        exp, exp_counters = S.brute_force_pair(dI, dJ, xyI, xyJ, S.RAGGED_RATIO, True, False, mode)
        assert _pairs(got) == _pairs(exp) and counters == exp_counters, mode


def test_second_round_case_has_more_than_256_candidates_per_pair(oracle):
    dI, dJ, _, _ = S.ambiguous_views(300, 128, 300)
    kept, not_nearest, ratio_only = _three_kinds(oracle, dI, dJ, 0.9, True)
    assert len(kept) + len(not_nearest) + len(ratio_only) > 256 and kept and not_nearest and ratio_only
    # (the pair the other way round has no ambiguity from its first view's side: the forward test has removed it already)
    kept, not_nearest, ratio_only = _three_kinds(oracle, dJ, dI, 0.9, True)
    assert kept and not not_nearest and not ratio_only


@pytest.mark.parametrize("n", [160, 100])
def test_arm_case_tables_reach_all_three_kinds(oracle, n):
    descs, xys = S.arm_views(n, witness=True)
    nones = [None] * 3
    for fn, kw in ((S.match_collection_kgraph, dict(K=16, P=10, S=10, seed=1998)), (S.match_collection_hnsw, {}), (S.match_collection_mrpt, {})):
        c0, m0, z = fn(oracle, descs, nones, S.ARM_PAIRS, S.ARM_RATIO, mode="off", **kw)
        c1, m1, k1 = fn(oracle, descs, nones, S.ARM_PAIRS, S.ARM_RATIO, mode="mutual", **kw)
        c2, m2, k2 = fn(oracle, descs, nones, S.ARM_PAIRS, S.ARM_RATIO, mode="symmetric", **kw)
        assert z == (0, 0, 0) and k1 == (len(m0), len(m0) - len(m1), 0) and k2 == (len(m0), len(m0) - len(m1), len(m1) - len(m2))
        assert len(m2) > 0 and k2[1] > 0 and k2[2] > 0, (fn.__name__, k2)
        # the mutual form of this restatement IS mutual_restatement's
        mm = getattr(M, fn.__name__)(oracle, descs, nones, S.ARM_PAIRS, S.ARM_RATIO, mutual=True, **kw)
        assert np.array_equal(mm[0], c1) and np.array_equal(mm[1], m1)


def test_mrpt_witness_tells_the_sqrt_form_from_the_squared_form(oracle):
    d1, d2 = S.sqrt_form_witness()
    assert S.SQRT_WITNESS_RATIO == S.ARM_RATIO                                 # the arms' case table runs at the witness's ratio
    assert S.reverse_ratio_passes(d1, d2, S.SQRT_WITNESS_RATIO, "sqrt") != S.reverse_ratio_passes(d1, d2, S.SQRT_WITNESS_RATIO, "squared")
    descs, xys = S.arm_views(160, witness=True)
    w = S.WITNESS_ROW
    assert oracle.l2sq(descs[0][w], descs[1][w]) == d1 and oracle.l2sq(descs[0][w], descs[1][w + 1]) == d2
    pair = np.array([[0, 1]], np.uint32)
    _, on_roots, _ = S.match_collection_mrpt(oracle, descs, xys, pair, S.SQRT_WITNESS_RATIO)
    _, on_squares, _ = S.match_collection_mrpt(oracle, descs, xys, pair, S.SQRT_WITNESS_RATIO, reverse_on_roots=False)
    _, mutual, _ = S.match_collection_mrpt(oracle, descs, xys, pair, S.SQRT_WITNESS_RATIO, mode="mutual")
    assert (w, w) in _pairs(mutual)                                          # the arm nominates it and it is nearest from both sides
    assert ((w, w) in _pairs(on_roots)) != ((w, w) in _pairs(on_squares))  # ... and the two forms disagree on its fate


# ---------------------------------------------------------------------------------------------------- the restatement's own consistency
def test_off_and_mutual_modes_are_the_oracle_and_the_mutual_restatement(oracle):
    dI, dJ, xyI, xyJ = S.ambiguous_views(257, 128, 11)
    pairs = np.array([[0, 1], [1, 0]], np.uint32)
    c, m, _ = S.match_collection(oracle, [dI, dJ], [xyI, xyJ], pairs, 0.8, True, False, "off")
    oc, om = oracle.match_collection([dI, dJ], [xyI, xyJ], pairs, 0.8, True)
    assert np.array_equal(c, oc) and np.array_equal(m, om)
    c, m, _ = S.match_collection(oracle, [dI, dJ], [xyI, xyJ], pairs, 0.8, True, False, "mutual")
    mc, mm = M.match_collection(oracle, [dI, dJ], [xyI, xyJ], pairs, 0.8, True, False, mutual=True)
    assert np.array_equal(c, mc) and np.array_equal(m, mm)


def test_survivors_are_what_the_swapped_matcher_returns(oracle):
    """the rule's own definition: (i, j) survives iff the forward matcher on (I, J) AND the forward matcher on (J, I) return it
    (without positions: no coordinate de-duplication on either side)"""
    dI, dJ, _, _ = S.ambiguous_views(100, 128, 5)
    fwd = set(_pairs(S.match_pair(oracle, dI, dJ, None, None, 0.8, True, False, "off")[0]))
    swapped = set((i, j) for j, i in _pairs(S.match_pair(oracle, dJ, dI, None, None, 0.8, True, False, "off")[0]))
    sym = set(_pairs(S.match_pair(oracle, dI, dJ, None, None, 0.8, True, False, "symmetric")[0]))
    assert sym == fwd & swapped and 0 < len(sym) < len(fwd)


# ---------------------------------------------------------------------------------------------------- the interface, without a GPU
def test_switch_report_and_flag_are_declared_and_exported():
    import ctypes as C
    from regard3d_amd import api
    L = api.load_library()
    for name in ("r3dm_set_symmetric_ratio", "r3dm_multi_set_symmetric_ratio", "r3dm_symmetric_ratio_report"):
        assert name in api.EXPORTS and hasattr(L, name), name
    assert L.r3dm_set_symmetric_ratio(None, 1) != 0 and L.r3dm_multi_set_symmetric_ratio(None, 1) != 0      # null handles are refused
    z = C.c_uint64(7)
    assert L.r3dm_symmetric_ratio_report(None, C.byref(z), None, None) != 0 and z.value == 7
    for cls in (api.Context, api.MultiContext):
        assert hasattr(cls, "set_symmetric_ratio")
    assert hasattr(api.Context, "symmetric_ratio_report")
    hdr = open(os.path.join(ROOT, "include", "r3dm.h")).read()
    assert "There is no reverse ratio test" not in hdr
    for decl in ("int r3dm_set_symmetric_ratio(r3dm_ctx* ctx, int enable);", "int r3dm_multi_set_symmetric_ratio(r3dm_multi* m, int enable);",
                 "int r3dm_symmetric_ratio_report(const r3dm_ctx* ctx, uint64_t* checked, uint64_t* dropped_not_nearest, uint64_t* dropped_ratio);"):
        assert decl in hdr, decl
    # r3dm_stats keeps its layout: the third counter comes through the report entry
    assert [f[0] for f in api.Stats._fields_ if "mutual" in f[0]] == ["n_mutual_checked", "n_mutual_dropped"]
    facade = open(os.path.join(ROOT, "include", "r3d_compute_matches.hpp")).read()
    assert "void setSymmetricRatio(bool on);" in facade
    flags = dict((n, int(v)) for n, v in re.findall(r"#define (R3DM_STAGE_\w+)\s+(\d+)u", facade))
    assert flags["R3DM_STAGE_SYMMETRIC_RATIO"] == api.STAGE_SYMMETRIC_RATIO == 4096
    assert sorted(flags.values()) == sorted(set(flags.values()))                                            # a free bit
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "There is no reverse ratio test" not in design
