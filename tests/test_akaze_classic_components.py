"""The classic arm's kpts_aux rule by connected components, restated in numpy with the restatement's own
offer() / upper_filter() (tests/akaze_classic_restatement.py) and checked against the serial walk.  CPU only.

Decomposition: drop the candidates that fail the descriptor-border test, link every candidate p of level l to every EARLIER candidate q
of level l - 1 or l that passes the rule's float predicate against q's converted position, walk each connected component on its own
(a fresh kpts_aux list per component, members in scan order), then number the slots of all components by their openers' scan order.
The slots (position, size, response, class, octave) and the upper-level filter's survivors must equal the serial walk's."""
import numpy as np
import pytest

import akaze_classic_restatement as R
from akaze_classic_walk_cases import _is_out, _random_list, _scan_order, _size, by_components, components, serial   # (the generators moved there)

f32 = np.float32


def _same(a, b):
    assert a.n == b.n
    n = a.n
    for f in ("x", "y", "size", "resp", "cls", "octave"):
        assert np.array_equal(getattr(a, f)[:n], getattr(b, f)[:n]), f
    assert np.array_equal(R.upper_filter(a), R.upper_filter(b))


@pytest.mark.parametrize("seed", range(8))
@pytest.mark.parametrize("n_levels", [2, 3, 4])
def test_components_equal_the_serial_walk_on_random_lists(seed, n_levels):
    rng = np.random.default_rng(100 * seed + n_levels)
    levels = R.levels(480, 400)[:8]               # two octaves: level 4 onwards has ratio 2
    first = int(rng.integers(0, len(levels) - n_levels + 1))
    lv = levels[first:first + n_levels]
    cands = _random_list(rng, lv, n_levels, n_clusters=10, per_cluster=14, spread=float(rng.uniform(1.0, 4.0)))
    ser = serial(lv, cands)
    got, roots = by_components(lv, cands)
    assert ser.n > 10 and np.bincount(roots[roots >= 0]).max() > 4          # clusters: components of several candidates
    _same(got, ser)


@pytest.mark.parametrize("seed", range(4))
def test_components_at_exact_boundary_distances(seed):
    """sizes of exactly 3 (esigma 2, size^2 = 9): integer offsets (3, 0) and (0, 3) sit ON the boundary (<= holds), (2, 3) just beyond"""
    rng = np.random.default_rng(seed)
    lv = [dict(w=120, h=100, octave=0, esigma=f32(2.0), ratio=f32(1.0)) for _ in range(3)]
    assert _size(lv[0]) * _size(lv[0]) == f32(9.0)
    cands = {}
    for i in range(3):
        for _ in range(10):
            x0, y0 = int(rng.integers(32, 88)), int(rng.integers(32, 68))
            for dx, dy in [(0, 0), (3, 0), (0, 3), (6, 0), (2, 3), (-3, 0), (3, 3)]:
                cands[(i, y0 + dy, x0 + dx)] = float(rng.uniform(0.001, 0.01))
    cands = _scan_order([(i, r, c, v) for (i, r, c), v in cands.items()])
    ser = serial(lv, cands)
    got, _ = by_components(lv, cands)
    _same(got, ser)


def test_a_chain_of_replacements_across_levels():
    """every level replaces the slot the previous level wrote (class l - 1 is visible to level l), so one slot walks through all four
    levels; a weaker candidate at the start of level 2 is rejected by the slot of class 1 before the chain reaches it"""
    lv = [dict(w=200, h=200, octave=0, esigma=e, ratio=f32(1.0)) for e in R.levels(200, 200)[0:4] for e in [e["esigma"]]]
    cands = [(0, 100, 100, 0.002), (0, 100, 140, 0.002),
             (1, 100, 101, 0.003),
             (2, 100, 100, 0.001), (2, 101, 102, 0.004),
             (3, 101, 103, 0.005), (3, 102, 140, 0.003)]
    ser = serial(lv, cands)
    got, roots = by_components(lv, cands)
    _same(got, ser)
    assert ser.n == 3 and ser.cls[0] == 3 and ser.resp[0] == f32(0.005)        # the chain's slot ends with the level-3 candidate
    assert ser.cls[2] == 3 and roots[6] != roots[1]                            # level 3 does not see the class-0 slot at column 140
    assert len(set(roots[[0, 2, 3, 4, 5]].tolist())) == 1                       # one component across the four levels


def test_an_out_of_bounds_candidate_inside_a_cluster():
    """the border test drops a candidate before linking: the strong candidate at column 25 (reach 28.28 at level 0) never opens or
    replaces a slot, and it must not join the two halves of the cluster either"""
    lv = R.levels(240, 180)[0:2]
    cands = _scan_order([(0, 60, 31, 0.002), (0, 60, 33, 0.002), (1, 60, 27, 0.009), (1, 60, 29, 0.001), (0, 62, 30, 0.003),
                         (0, 60, 25, 0.02), (1, 61, 25, 0.03), (1, 61, 33, 0.004)])
    assert _is_out(lv[0], 60, 25) and _is_out(lv[1], 61, 25) and not _is_out(lv[0], 60, 31)
    ser = serial(lv, cands)
    got, roots = by_components(lv, cands)
    _same(got, ser)
    assert all(roots[k] == -1 for k, c in enumerate(cands) if c[2] == 25)
    assert not np.any(np.isin(ser.resp[:ser.n], [f32(0.02), f32(0.03)]))
