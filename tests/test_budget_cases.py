"""The inputs of tests/test_gpu_budget.py reach the edges they are built for -- shown on the restatement alone (budget_restatement.py,
the oracle), without a GPU.  These are conditions on the inputs, not measurements: a case that misses one would let a wrong
implementation pass (a selection that is a prefix needs no remap; a graph that equals the full graph restricted to S needs no
sub-view; a cut that falls between two classes needs no tie rule)."""
import numpy as np
import pytest

import budget_cases as Cs
import budget_restatement as B
from regard3d_amd import api


@pytest.mark.parametrize("kind", [k[0] for k in Cs.KINDS])
@pytest.mark.parametrize("N", Cs.BUDGETS)
def test_matching_cases_reach_their_edges(oracle, kind, N):
    descs, xys, prios, binary, ratio, squared = Cs.make_views(kind)
    pairs = Cs.all_ordered_pairs(len(descs))
    modes = ("off", "mutual", "symmetric") if kind in ("f32_128", "bin_61", "f32_37") else ("off",)
    for mode in modes:
        c = Cs.conditions(oracle, descs, xys, prios, pairs, N, ratio, squared, binary, mode)
        print(kind, N, mode, c)
        assert c["budgeted_and_whole"] and c["non_empty_and_remapped"] and c["not_the_restriction"] and c["tie_straddles"], (mode, c)


def test_real_valued_case_reaches_its_edges(oracle):
    descs, xys, prios, binary, ratio, squared = Cs.make_views("f32_144", seed=1, real=True)
    pairs = Cs.all_ordered_pairs(len(descs))
    for N in Cs.BUDGETS:
        c = Cs.conditions(oracle, descs, xys, prios, pairs, N, 0.8, True, False)
        assert c["budgeted_and_whole"] and c["non_empty_and_remapped"] and c["not_the_restriction"] and c["tie_straddles"], (N, c)


def test_the_planted_rows_do_what_they_are_for(oracle):
    """N = 2: the long views select exactly the two planted rows, and the query that observes row 9 is refused on the whole views
    (its second observation, row 12, is as near) and accepted on the sub-views"""
    descs, xys, prios, binary, ratio, squared = Cs.make_views("f32_128")
    for v, d in enumerate(descs[:-1]):
        if len(d) > Cs.DUP:
            assert B.selected_rows(prios[v], len(d), 2).tolist() == list(Cs.TOP)
    assert B.selected_rows(prios[2], 4, 2).tolist() == [0, 1] and B.tie_straddles_cut(prios[2], 4, 2)
    pair = np.array([[8, 9]], np.uint32)                                 # the 257- and the 300-row view
    _, mapped, sub = B.match_collection(oracle, descs, xys, prios, pair, 2, ratio, squared)
    _, whole = B.whole_collection(oracle, descs, xys, pair, ratio, squared)
    top9 = (Cs.TOP[1], Cs.TOP[1])
    assert top9 in set(map(tuple, mapped.tolist())) and top9 not in set(map(tuple, whole.tolist()))
    assert sub.tolist() == [[0, 0], [1, 1]] and mapped.tolist() == [[5, 5], [9, 9]]


@pytest.mark.parametrize("pattern", Cs.PATTERNS)
def test_selection_patterns_against_the_brute_force(pattern):
    chunk = api.BUDGET_SELECT_CHUNK
    straddles = 0
    for n in Cs.selection_sizes(chunk):
        for N in Cs.selection_budgets(n):
            p = Cs.priority_pattern(pattern, n, N)
            got = B.selected_rows(p, n, N)
            assert got.tolist() == B.brute_force_rows(p, n, N) and len(got) == min(n, N)
            assert np.all(np.diff(got) > 0)
            straddles += B.tie_straddles_cut(p, n, N)
            if pattern == "three_values" and 3 <= N < n:
                assert B.tie_straddles_cut(p, n, N) and 2.0 in p[got] and (p[got] >= 2.0).all() and (np.delete(p, got) <= 2.0).all()
    assert pattern in ("increasing", "none") or straddles > 0


def test_selection_sizes_straddle_the_chunk():
    chunk = api.BUDGET_SELECT_CHUNK
    sizes = Cs.selection_sizes(chunk)
    assert chunk - 1 in sizes and chunk in sizes and chunk + 1 in sizes and max(sizes) > 3 * chunk and max(sizes) % chunk != 0
    # subnormal keys and -0.0: the order of the bit patterns is the order of the values once -0.0 is +0.0
    p = Cs.priority_pattern("subnormals", 3 * chunk + 7, 64)
    assert (p == 0).any() and (np.signbit(p)).any() and ((p > 0) & (p < np.finfo(np.float32).tiny)).any()
    q = p + np.float32(0.0)
    assert np.array_equal(np.argsort(-q.view(np.uint32).astype(np.int64), kind="stable"), np.argsort(-q.astype(np.float64), kind="stable"))
    b = Cs.priority_pattern("lowest_bit", 300, 64).view(np.uint32)
    assert set((b - b.min()).tolist()) == {0, 1}
