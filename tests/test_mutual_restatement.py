"""The mutual-matching restatement (mutual_restatement.py) against a brute-force numpy loop on engineered integer rows, the three
consequences of the rule (include/r3dm.h: r3dm_set_mutual_matching), its interplay with the coordinate de-duplication, and the
interface without a GPU."""
import os
import re

import numpy as np
import pytest

import mutual_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pairs(m):
    return [tuple(x) for x in np.asarray(m).tolist()]


# ---------------------------------------------------------------------------------------------------- engineered rows
@pytest.mark.parametrize("dim,dtype", [(64, np.float32), (37, np.float32), (128, np.uint8), (260, np.float32)])
def test_engineered_cases_against_the_brute_force_loop(oracle, dim, dtype):
    dI, dJ, xyI, xyJ = R.engineered_views(dim, dtype)
    for mutual in (False, True):
        got = R.match_pair(oracle, dI, dJ, xyI, xyJ, 0.6, True, False, mutual)
        assert _pairs(got) == _pairs(R.brute_force_pair(dI, dJ, xyI, xyJ, 0.6, True, False, mutual)), mutual
    off = _pairs(R.match_pair(oracle, dI, dJ, xyI, xyJ, 0.6, True, False, False))
    on = _pairs(R.match_pair(oracle, dI, dJ, xyI, xyJ, 0.6, True, False, True))
    # switch off: both observers of I0, both identical rows, and of the two rows at one position only the earlier (J4)
    assert off == [(0, 0), (0, 1), (1, 2), (1, 3), (2, 4), (3, 6)]
    # switch on: J0 (distance 1 beats 4), J2 (lower of two identical rows), J5 (J4 failed the check BEFORE the de-duplication could
    # drop J5 behind it), J6
    assert on == [(0, 0), (1, 2), (2, 5), (3, 6)]


def test_distances_one_and_four(oracle):
    dI, dJ, xyI, xyJ = R.engineered_views(64)
    assert oracle.l2sq(dI[0], dJ[0]) == 1.0 and oracle.l2sq(dI[0], dJ[1]) == 4.0
    rev = R.reverse_nearest(oracle, dI, dJ)
    assert rev[:4].tolist() == [0, 2, 5, 6]


@pytest.mark.parametrize("n,nbytes", [(33, 32), (70, 61)])
def test_binary_rows_against_the_brute_force_loop(oracle, n, nbytes):
    dI, dJ, xyI, xyJ = R.second_observations(n, 0, 7 + n, nbytes=nbytes)
    dJ[5] = dJ[4]                                                    # two identical rows of J
    for mutual in (False, True):
        got = R.match_pair(oracle, dI, dJ, xyI, xyJ, 0.8, False, True, mutual)
        assert _pairs(got) == _pairs(R.brute_force_pair(dI, dJ, xyI, xyJ, 0.8, False, True, mutual)), mutual


# ---------------------------------------------------------------------------------------------------- the consequences of the rule
@pytest.mark.parametrize("n", [33, 257, 300])
def test_consequences_on_second_observations(oracle, n):
    dI, dJ, xyI, xyJ = R.second_observations(n, 128, n)
    off = R.match_pair(oracle, dI, dJ, xyI, xyJ, 0.99, True, False, False)
    on = R.match_pair(oracle, dI, dJ, xyI, xyJ, 0.99, True, False, True)
    assert len(off) > len(on) > 0
    # the forward list matches rows of I more than once (what the switch is for) ...
    assert len(np.unique(off[:, 0])) < len(off)
    # ... a row of I appears at most once per pair under the rule, and the result is a subset of the switch-off result (no repeated
    # positions in these views: the coordinate de-duplication drops nothing)
    assert len(np.unique(on[:, 0])) == len(on)
    assert set(_pairs(on)) <= set(_pairs(off))
    # every survivor is its row's nearest row of J
    rev = R.reverse_nearest(oracle, dI, dJ)
    assert all(rev[i] == j for i, j in _pairs(on))
    if n == 33:
        assert _pairs(on) == _pairs(R.brute_force_pair(dI, dJ, xyI, xyJ, 0.99, True, False, True))


def test_one_row_of_J_is_always_mutual(oracle):
    dI, dJ, xyI, xyJ = R.second_observations(40, 64, 3)
    for binary, a, b in ((False, dI, dJ[7:8]), (True, *R.second_observations(40, 0, 4, nbytes=32)[:2])):
        b = b[7:8] if binary else b
        off = R.match_pair(oracle, a, b, None, None, 0.9, not binary, binary, False)
        on = R.match_pair(oracle, a, b, None, None, 0.9, not binary, binary, True)
        assert len(off) == 1 and _pairs(on) == _pairs(off)


def test_of_two_identical_rows_the_lower_index_survives(oracle):
    dI, dJ, xyI, xyJ = R.second_observations(50, 128, 5)
    dJ[31] = dJ[12]                                                  # a later copy of a row that matches
    off = _pairs(R.match_pair(oracle, dI, dJ, xyI, xyJ, 0.99, True, False, False))
    on = _pairs(R.match_pair(oracle, dI, dJ, xyI, xyJ, 0.99, True, False, True))
    i = [i for i, j in off if j == 12]
    assert i and (i[0], 31) in off                                   # both copies nominate the same row of I
    assert (i[0], 12) in on and (i[0], 31) not in on


def test_dedup_interaction_later_of_two_equal_positions_survives(oracle):
    """two rows of J at one position, both nearest to I2: switch off, the coordinate de-duplication keeps the earlier (J4); switch on,
    J4 fails the check first, so the later (J5) must survive"""
    dI, dJ, xyI, xyJ = R.engineered_views(64)
    off = _pairs(R.match_pair(oracle, dI, dJ, xyI, xyJ, 0.6, True, False, False))
    on = _pairs(R.match_pair(oracle, dI, dJ, xyI, xyJ, 0.6, True, False, True))
    assert (2, 4) in off and (2, 5) not in off
    assert (2, 5) in on and (2, 4) not in on
    # without positions nothing is de-duplicated: the switch-on result is then a subset of the switch-off result
    off0 = _pairs(R.match_pair(oracle, dI, dJ, None, None, 0.6, True, False, False))
    on0 = _pairs(R.match_pair(oracle, dI, dJ, None, None, 0.6, True, False, True))
    assert set(on0) <= set(off0) and on0 == on


def test_switch_off_restatement_is_the_oracle(oracle):
    dI, dJ, xyI, xyJ = R.second_observations(257, 128, 11)
    pairs = np.array([[0, 1], [1, 0]], np.uint32)
    c, m = R.match_collection(oracle, [dI, dJ], [xyI, xyJ], pairs, 0.8, True, False, mutual=False)
    oc, om = oracle.match_collection([dI, dJ], [xyI, xyJ], pairs, 0.8, True)
    assert np.array_equal(c, oc) and np.array_equal(m, om)


def test_approximate_arms_switch_off_is_their_cpu_model(oracle):
    views = [R.second_observations(160, 128, 20 + k)[k % 2] for k in range(3)]
    xys = [np.stack([np.arange(160) * 2.0 + k, np.arange(160) * 3.0], 1).astype(np.float32) for k in range(3)]
    pairs = np.array([[0, 1], [0, 2], [1, 2]], np.uint32)
    c, m = R.match_collection_kgraph(oracle, views, xys, pairs, 0.8, K=16, P=10, S=10, seed=1998, mutual=False)
    oc, om, _ = oracle.match_collection_kgraph(views, xys, pairs, 0.8, builder="exact", K=16, P=10, S=10, seed=1998, min_rows=128)
    assert np.array_equal(c, oc) and np.array_equal(m, om)
    c, m = R.match_collection_hnsw(oracle, views, xys, pairs, 0.8, "precise", mutual=False)
    oc, om = oracle.match_collection_hnsw(views, xys, pairs, 0.8, "precise")
    assert np.array_equal(c, oc) and np.array_equal(m, om)
    c, m = R.match_collection_mrpt(oracle, views, xys, pairs, 0.8, mutual=False)
    oc, om = oracle.match_collection_mrpt(views, xys, pairs, 0.8)
    assert np.array_equal(c, oc) and np.array_equal(m, om)
    # ... and switched on each arm's result is a subset of it, a row of I at most once per pair
    for fn, kw in ((R.match_collection_kgraph, dict(K=16, P=10, S=10, seed=1998)), (R.match_collection_hnsw, {}), (R.match_collection_mrpt, {})):
        c0, m0 = fn(oracle, views, xys, pairs, 0.8, mutual=False, **kw)
        c1, m1 = fn(oracle, views, xys, pairs, 0.8, mutual=True, **kw)
        o0 = np.r_[0, np.cumsum(c0)]; o1 = np.r_[0, np.cumsum(c1)]
        for p in range(len(pairs)):
            a, b = m0[o0[p]:o0[p + 1]], m1[o1[p]:o1[p + 1]]
            assert set(_pairs(b)) <= set(_pairs(a)) and len(np.unique(b[:, 0])) == len(b)


# ---------------------------------------------------------------------------------------------------- the interface, without a GPU
def test_switch_counters_and_flag_are_declared_and_exported():
    import ctypes as C
    from regard3d_amd import api
    L = api.load_library()
    for name in ("r3dm_set_mutual_matching", "r3dm_multi_set_mutual_matching", "r3dm_compute_matches_dir_flags"):
        assert name in api.EXPORTS and hasattr(L, name), name
    assert L.r3dm_set_mutual_matching(None, 1) != 0 and L.r3dm_multi_set_mutual_matching(None, 1) != 0      # null handles are refused
    names = [f[0] for f in api.Stats._fields_]
    assert "n_mutual_checked" in names and "n_mutual_dropped" in names
    hdr = open(os.path.join(ROOT, "include", "r3dm.h")).read()
    body = hdr[:hdr.index("} r3dm_stats;")]
    body = re.sub(r"/\*.*?\*/", "", body[body.rindex("typedef struct"):], flags=re.S)
    assert re.findall(r"\b(?:uint64_t|double|uint32_t|float)\s+(\w+)\s*;", body) == names
    assert C.sizeof(api.Stats) == 8 * len(names)
    assert hasattr(api.Context, "set_mutual_matching") and hasattr(api.MultiContext, "set_mutual_matching")
    facade = open(os.path.join(ROOT, "include", "r3d_compute_matches.hpp")).read()
    assert "void setMutualMatching(bool on);" in facade
    flags = dict((n, int(v)) for n, v in re.findall(r"#define (R3DM_STAGE_\w+)\s+(\d+)u", facade))
    assert flags["R3DM_STAGE_MUTUAL_MATCHING"] == api.STAGE_MUTUAL_MATCHING == 128
    assert sorted(flags.values()) == sorted(set(flags.values()))                                            # a free bit
