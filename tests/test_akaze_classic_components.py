"""The classic arm's kpts_aux rule by connected components, restated in numpy with the restatement's own
offer() / upper_filter() (tests/akaze_classic_restatement.py) and checked against the serial walk.  CPU only.

Decomposition: drop the candidates that fail the descriptor-border test, link every candidate p of level l to every EARLIER candidate q
of level l - 1 or l that passes the rule's float predicate against q's converted position, walk each connected component on its own
(a fresh kpts_aux list per component, members in scan order), then number the slots of all components by their openers' scan order.
The slots (position, size, response, class, octave) and the upper-level filter's survivors must equal the serial walk's."""
import numpy as np
import pytest

import akaze_classic_restatement as R

f32 = np.float32


def _size(lv):
    return f32(lv["esigma"] * R.DFAC)


def _is_out(lv, row, col):
    size, ratio = _size(lv), f32(lv["ratio"])
    r = f32(R.SMAX * f32(R.fround(f32(size / ratio))))
    px, py = f32(col), f32(row)
    return (R.fround(f32(px - r)) - 1 < 0 or R.fround(f32(px + r)) + 1 >= lv["w"] or
            R.fround(f32(py - r)) - 1 < 0 or R.fround(f32(py + r)) + 1 >= lv["h"])


def _conv(v, lv):
    ratio = f32(lv["ratio"])
    return f32(float(f32(f32(v) * ratio)) + 0.5 * (float(ratio) - 1.0))


def serial(levels, cands):
    """cands: (level, row, col, value) in scan order -> the AuxList of the serial rule"""
    aux = R.AuxList(max(1, len(cands)))
    for (i, row, col, v) in cands:
        lv = levels[i]
        R.offer(aux, lv, i, row, col, f32(v), lv["h"], lv["w"])
    return aux


def components(levels, cands):
    """union-find over the edges of the rule; returns the root of every candidate (-1: dropped by the border test)"""
    n = len(cands)
    par = np.array([-1 if _is_out(levels[c[0]], c[1], c[2]) else k for k, c in enumerate(cands)])

    def find(x):
        while par[x] != x:
            par[x] = par[par[x]]
            x = par[x]
        return x

    for p in range(n):
        if par[p] < 0:
            continue
        l, row, col, _ = cands[p]
        size = _size(levels[l]); ratio = f32(levels[l]["ratio"])
        sx, sy = f32(f32(col) * ratio), f32(f32(row) * ratio)
        for q in range(p):
            m = cands[q][0]
            if par[q] < 0 or m not in (l - 1, l):
                continue
            tx, ty = f32(sx - _conv(cands[q][2], levels[m])), f32(sy - _conv(cands[q][1], levels[m]))
            if f32(tx * tx + ty * ty) <= f32(size * size):
                a, b = find(p), find(q)
                if a != b:
                    par[max(a, b)] = min(a, b)
    return np.array([find(k) if par[k] >= 0 else -1 for k in range(n)])


def by_components(levels, cands):
    """each component walked on its own, slots numbered by opener rank -> an AuxList laid out as the serial one"""
    roots = components(levels, cands)
    opened = []                                   # (opener index, component aux, slot in it)
    for r in sorted(set(roots[roots >= 0].tolist())):
        members = [k for k in range(len(cands)) if roots[k] == r]
        aux = R.AuxList(len(members))
        for k in members:
            i, row, col, v = cands[k]
            before = aux.n
            R.offer(aux, levels[i], i, row, col, f32(v), levels[i]["h"], levels[i]["w"])
            if aux.n > before:
                opened.append((k, aux, before))
    out = R.AuxList(max(1, len(cands)))
    for s, (_, aux, q) in enumerate(sorted(opened, key=lambda t: t[0])):
        out.put(s, aux.x[q], aux.y[q], aux.size[q], aux.resp[q], aux.cls[q], aux.octave[q])
    out.n = len(opened)
    return out, roots


def _same(a, b):
    assert a.n == b.n
    n = a.n
    for f in ("x", "y", "size", "resp", "cls", "octave"):
        assert np.array_equal(getattr(a, f)[:n], getattr(b, f)[:n]), f
    assert np.array_equal(R.upper_filter(a), R.upper_filter(b))


def _scan_order(cands):
    return sorted(cands, key=lambda c: (c[0], c[1], c[2]))


def _random_list(rng, levels, n_levels, n_clusters, per_cluster, spread):
    cands = {}
    for i in range(n_levels):
        lv = levels[i]
        for _ in range(n_clusters):
            cx, cy = rng.uniform(0.1 * lv["w"], 0.9 * lv["w"]), rng.uniform(0.1 * lv["h"], 0.9 * lv["h"])      # (some near the border: out)
            for _ in range(per_cluster):
                col = int(np.clip(round(cx + rng.normal(0, spread)), 1, lv["w"] - 2))
                row = int(np.clip(round(cy + rng.normal(0, spread)), 1, lv["h"] - 2))
                cands[(i, row, col)] = float(rng.choice([rng.uniform(0.001, 0.01), 0.005]))    # ties among the responses too
    return _scan_order([(i, r, c, v) for (i, r, c), v in cands.items()])


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
