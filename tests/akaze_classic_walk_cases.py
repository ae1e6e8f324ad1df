"""Candidate lists built for the edges of the classic A-KAZE kpts_aux walk.  NOT a test module: the generators
shared by tests/test_akaze_classic_walk_cases.py (CPU: every case contains what it was built for, asserted from the restatement alone),
tests/test_gpu_akaze_classic_walk.py (GPU: the developer build's r3dm_dev_akaze_classic_walk runs the product's kernels on the lists)
and tests/test_akaze_classic_components.py (the numpy model of the decomposition).

The reference of every case is the serial restatement alone: R.offer over the list in scan order, then R.upper_filter
(tests/akaze_classic_restatement.py).  trace() replays the list through R.offer and names what happened -- it restates the rule's hit
test only to NAME events (a tie, a distance exactly on the boundary, a slot that changed its cell); the slots it returns are R.offer's.

A candidate is (level, row, col, value); a list is in scan order (level, row, col).  A case is a dict:
  name, group   group = the child process of the GPU module the case runs in
  levels        level table (dicts with w, h, octave, esigma, ratio), at most 16 levels
  w, h          the image
  lists         one candidate list per image (B = len(lists); all but the batch case have one)
  forms         (parallel, bound) pairs the GPU test runs; every case has FORMS, some add a bound of their own
  events        {event name: ("==" | ">=" | ">", count)} over trace() of lists[0] (see trace and EVENTS below)
  outcomes      optional: one letter per candidate of lists[0] -- O opened a slot, R replaced one, r rejected by the first hit,
                x dropped by the descriptor-border test
  repeats       how often the GPU test runs the parallel form in one process (contention case: 3, identical bytes asked)

Why the later-slot variants of the upper-level filter sit on a hand-made table and on levels 7 / 8 only: inside one octave the filter's
distance is the walk's.  A class k + 1 slot j within size_k of a class k slot i < j would have been written last by a level k + 1
candidate within size_k < size_(k+1) of slot i, and slot i -- earlier in the list, class k since level k -- would have been that
candidate's first hit.  So "later and within reach" needs the walk's distance (candidate position WITHOUT the half-pixel offset of its
octave) and the filter's (with it) to disagree: levels 3 / 4 cannot (shift 0.71 < size_4 - size_3), levels 7 / 8 can (converted
offsets (-7, -3): 58 <= size_7^2 = 65.2, unconverted (-8.5, -4.5): 92.5 > size_8^2 = 92.16).  A distance of exactly size_k needs an
integer size^2: the hand-made table."""
from collections import Counter

import numpy as np

import akaze_classic_restatement as R

f32 = np.float32
FORMS = ((1, 64), (1, 1), (0, 64))           # the parallel form, everything above one candidate handed back, the one-wavefront form


# ---------------------------------------------------------------------------------------------------- the rule's pieces, restated
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


def component_roots(levels, cands):
    """components() for long lists: the same edges, the predicate evaluated over all earlier candidates at once (float32 numpy, operation
    for operation), the components by scipy.  Root = the component's smallest index, -1 = dropped by the border test."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    n = len(cands)
    if n == 0:
        return np.zeros(0, np.int64)
    lvl = np.array([c[0] for c in cands]); row = np.array([c[1] for c in cands], np.float32); col = np.array([c[2] for c in cands], np.float32)
    out = np.array([_is_out(levels[c[0]], c[1], c[2]) for c in cands])
    ratio = np.array([f32(levels[l]["ratio"]) for l in lvl], np.float32)
    sx, sy = col * ratio, row * ratio
    off = 0.5 * (ratio.astype(np.float64) - 1.0)
    cx, cy = (sx.astype(np.float64) + off).astype(np.float32), (sy.astype(np.float64) + off).astype(np.float32)
    s2 = np.array([f32(_size(levels[l]) * _size(levels[l])) for l in lvl], np.float32)
    ei, ej = [], []
    for p in range(1, n):
        if out[p]:
            continue
        tx, ty = sx[p] - cx[:p], sy[p] - cy[:p]
        m = (~out[:p]) & ((lvl[:p] == lvl[p]) | (lvl[:p] == lvl[p] - 1)) & (tx * tx + ty * ty <= s2[p])
        q = np.flatnonzero(m)
        ei.extend([p] * len(q)); ej.extend(q.tolist())
    _, lab = connected_components(coo_matrix((np.ones(len(ei)), (ei, ej)), shape=(n, n)), directed=False)
    first = np.full(lab.max() + 1, n)
    np.minimum.at(first, lab, np.arange(n))
    roots = first[lab]
    roots[out] = -1
    return roots


# ---------------------------------------------------------------------------------------------------- what happened, named
EVENTS = """
open / replace / reject / out      outcome of a candidate (out = dropped by the border test, with or without a hit before it)
tie_reject                         rejected by a first hit of EQUAL response;  tie_cross: that slot was of class l - 1
ulp_replace                        replaced a slot whose response is one float below the candidate's;  ulp_cross: class l - 1
boundary_hit                       the first hit lay at a distance of exactly size^2;  boundary_cross: that slot had another ratio
cross_hit                          the first hit was a slot of class l - 1;  ratio_hit: ... of a level with another ratio
moved_cell                         a replacement carried the slot into another cell of the level's grid (side floor(size) + 1)
stale_open                         opened a slot although a position an eligible slot LEFT during this level lies within size
moved_hit                          first hit = a slot whose opening position does not lie within size (only where it moved to does)
cell_multiple                      a slot was written at an x or y that is an exact multiple of the level's cell side
first_hit_not_nearest              more than one eligible slot within size; the first in list order was not the nearest
up_drop / up_tie / up_boundary     pairs (i, later j of class + 1 within size_i): j stronger / equal / j stronger at exactly size_i^2
up_earlier                         kept slots i with an EARLIER j of class + 1 within size_i and stronger
slots / kept / n                   totals;  comp_max, comp_over64, lone: component sizes (component_roots)
"""


def trace(levels, cands, want_components=True):
    """-> (aux, kept, outcomes string, Counter of EVENTS, opener index per slot, roots)"""
    aux = R.AuxList(max(1, len(cands)))
    ev, outc, opener = Counter(), [], []
    left = {}                                     # slot -> [(x, y, level during which the slot left it)]
    born = {}                                     # slot -> its opening position
    for k, (i, row, col, v) in enumerate(cands):
        lv = levels[i]
        size, ratio = _size(lv), f32(lv["ratio"])
        s2 = f32(size * size)
        G = int(size) + 1
        sx, sy = f32(f32(col) * ratio), f32(f32(row) * ratio)
        n, q = aux.n, -1
        if n:
            tx, ty = sx - aux.x[:n], sy - aux.y[:n]
            dist = tx * tx + ty * ty
            elig = (aux.cls[:n] == i) | (aux.cls[:n] == i - 1)
            hit = elig & (dist <= s2)
            if hit.any():
                q = int(np.argmax(hit))
                if hit.sum() > 1 and dist[q] > dist[hit].min():
                    ev["first_hit_not_nearest"] += 1
        old = (aux.x[q], aux.y[q], aux.resp[q], int(aux.cls[q])) if q >= 0 else None
        R.offer(aux, lv, i, row, col, f32(v), lv["h"], lv["w"])
        if q >= 0:
            cross = old[3] == i - 1
            ev["cross_hit"] += cross
            ev["ratio_hit"] += cross and f32(levels[i - 1]["ratio"]) != ratio
            if dist[q] == s2:
                ev["boundary_hit"] += 1
                ev["boundary_cross"] += cross and f32(levels[i - 1]["ratio"]) != ratio
            bx, by = born[q]
            if not (sx - bx) * (sx - bx) + (sy - by) * (sy - by) <= s2:
                ev["moved_hit"] += 1
        if aux.n > n:
            o = "O"; opener.append(k); born[aux.n - 1] = (aux.x[aux.n - 1], aux.y[aux.n - 1])
            for s, lst in left.items():
                if (aux.cls[s] == i or aux.cls[s] == i - 1) and any(lev == i and (sx - x) * (sx - x) + (sy - y) * (sy - y) <= s2 for x, y, lev in lst):
                    ev["stale_open"] += 1
                    break
        elif q >= 0 and (aux.resp[q] != old[2] or aux.x[q] != old[0] or aux.y[q] != old[1] or aux.cls[q] != old[3]):
            o = "R"
            ev["ulp_replace"] += f32(v) == np.nextafter(old[2], f32(np.inf))
            ev["ulp_cross"] += f32(v) == np.nextafter(old[2], f32(np.inf)) and old[3] == i - 1
            left.setdefault(q, []).append((old[0], old[1], i))
            if (int(old[0]) // G, int(old[1]) // G) != (int(aux.x[q]) // G, int(aux.y[q]) // G):
                ev["moved_cell"] += 1
        elif q >= 0 and not f32(v) > old[2]:
            o = "r"
            ev["tie_reject"] += f32(v) == old[2]
            ev["tie_cross"] += f32(v) == old[2] and old[3] == i - 1
        else:
            o = "x"
        if o in "OR":
            s = q if o == "R" else aux.n - 1
            ev["cell_multiple"] += float(aux.x[s]) % G == 0 or float(aux.y[s]) % G == 0
        ev[{"O": "open", "R": "replace", "r": "reject", "x": "out"}[o]] += 1
        outc.append(o)
    kept = R.upper_filter(aux)
    ks = set(kept.tolist())
    n = aux.n
    for a in range(n):
        tx, ty = aux.x[a] - aux.x[:n], aux.y[a] - aux.y[:n]
        dist = tx * tx + ty * ty
        p2 = f32(aux.size[a] * aux.size[a])
        near = (aux.cls[:n] == aux.cls[a] + 1) & (dist <= p2)
        later = np.arange(n) > a
        ev["up_drop"] += int((near & later & (aux.resp[a] < aux.resp[:n])).sum())
        ev["up_tie"] += int((near & later & (aux.resp[a] == aux.resp[:n])).sum())
        ev["up_boundary"] += int((near & later & (aux.resp[a] < aux.resp[:n]) & (dist == p2)).sum())
        ev["up_earlier"] += int(a in ks and (near & ~later & (aux.resp[a] < aux.resp[:n])).any())
    ev["slots"], ev["kept"], ev["n"] = n, len(kept), len(cands)
    roots = None
    if want_components:
        roots = component_roots(levels, cands)
        sizes = np.bincount(roots[roots >= 0]) if (roots >= 0).any() else np.zeros(1, np.int64)
        sizes = sizes[sizes > 0]
        ev["comp_max"] = int(sizes.max()) if len(sizes) else 0
        ev["comp_over64"] = int((sizes > 64).sum())
        ev["lone"] = int((sizes == 1).sum())
    return aux, kept, "".join(outc), ev, opener, roots


_REF = {}


def reference(case, image=0):
    """the serial restatement of one image of a case, computed once: dict of x, y, size, resp (float32), cls (uint32), kept (bool)"""
    key = (case["name"], image)
    if key not in _REF:
        aux = serial(case["levels"], case["lists"][image])
        n = aux.n
        kept = np.zeros(n, bool)
        kept[R.upper_filter(aux)] = True
        _REF[key] = dict(x=aux.x[:n].copy(), y=aux.y[:n].copy(), size=aux.size[:n].copy(), resp=aux.resp[:n].copy(),
                         cls=aux.cls[:n].astype(np.uint32), kept=kept)
    return _REF[key]


# ---------------------------------------------------------------------------------------------------- tables
def _prod8():
    return R.levels(480, 400)[:8]                 # two octaves: level 4 onwards has ratio 2


def _prod12():
    return R.levels(480, 400)                     # three octaves (the fourth would be 60 x 50): ratios 1, 2, 4, offsets 0, 0.5, 1.5


def _hand(specs, w, h):
    """hand-made table: specs = (esigma, ratio) per level; the level is the image divided by its ratio"""
    return [dict(w=int(w // r), h=int(h // r), octave=int(np.log2(r)), esigma=f32(e), ratio=f32(r)) for e, r in specs]


def _case(name, group, levels, w, h, cands, events, outcomes=None, forms=FORMS, lists=None, repeats=1):
    lists = [_scan_order(cands)] if lists is None else lists
    for l in lists:
        assert l == _scan_order(l) and len({c[:3] for c in l}) == len(l), name
    return dict(name=name, group=group, levels=levels, w=w, h=h, lists=lists, events=events, outcomes=outcomes, forms=tuple(forms), repeats=repeats)


def _up(x):
    return float(np.nextafter(f32(x), f32(np.inf)))


# ---------------------------------------------------------------------------------------------------- the cases
def _existing_families():
    out = []
    for n_levels in (2, 3, 4):
        for seed in range(8):
            rng = np.random.default_rng(100 * seed + n_levels)
            levels = _prod8()
            first = int(rng.integers(0, len(levels) - n_levels + 1))
            lv = levels[first:first + n_levels]
            cands = _random_list(rng, lv, n_levels, n_clusters=10, per_cluster=14, spread=float(rng.uniform(1.0, 4.0)))
            out.append(_case(f"random-{n_levels}-{seed}", "families", lv, 480, 400, cands,
                             dict(slots=(">=", 11), comp_max=(">=", 5), tie_reject=(">=", 1), replace=(">=", 1), moved_cell=(">=", 1))))
    for seed in range(4):
        rng = np.random.default_rng(seed)
        lv = _hand([(2.0, 1)] * 3, 120, 100)
        cands = {}
        for i in range(3):
            for _ in range(10):
                x0, y0 = int(rng.integers(32, 88)), int(rng.integers(32, 68))
                for dx, dy in [(0, 0), (3, 0), (0, 3), (6, 0), (2, 3), (-3, 0), (3, 3)]:
                    cands[(i, y0 + dy, x0 + dx)] = float(rng.uniform(0.001, 0.01))
        out.append(_case(f"boundary-{seed}", "families", lv, 120, 100, [(i, r, c, v) for (i, r, c), v in cands.items()],
                         dict(boundary_hit=(">=", 4), open=(">=", 4), out=(">=", 20))))
    lv = [dict(w=200, h=200, octave=0, esigma=e["esigma"], ratio=f32(1.0)) for e in R.levels(200, 200)[0:4]]
    out.append(_case("chain", "families", lv, 200, 200,
                     [(0, 100, 100, 0.002), (0, 100, 140, 0.002), (1, 100, 101, 0.003), (2, 100, 100, 0.001), (2, 101, 102, 0.004),
                      (3, 101, 103, 0.005), (3, 102, 140, 0.003)],
                     dict(slots=("==", 3), replace=("==", 3), cross_hit=("==", 4), reject=("==", 1)), outcomes="OORrRRO"))
    lv = R.levels(240, 180)[0:2]
    out.append(_case("border-in-cluster", "families", lv, 240, 180,
                     [(0, 60, 31, 0.002), (0, 60, 33, 0.002), (1, 60, 27, 0.009), (1, 60, 29, 0.001), (0, 62, 30, 0.003),
                      (0, 60, 25, 0.02), (1, 61, 25, 0.03), (1, 61, 33, 0.004)], dict(out=("==", 4), slots=("==", 1)), outcomes="xOrRxrxx"))
    return out


def _run(level, row, col0, n, step=2):
    return [(level, row, col0 + step * k) for k in range(n)]


def _values(pattern, n, rng):
    if pattern == "increasing":
        return [0.001 + 0.00001 * k for k in range(n)]
    if pattern == "decreasing":
        return [0.009 - 0.00001 * k for k in range(n)]
    return [float(rng.choice([rng.uniform(0.001, 0.01), 0.005, 0.004])) for _ in range(n)]


def _connected_run(n, two_levels, row=100, col0=60, l0=0):
    """n candidates at a spacing of 2 (below every size): one row of level l0, or split over a row of level l0 and the next row of
    level l0 + 1 (every level l0 + 1 candidate lies 1 from a level-l0 one)"""
    if not two_levels:
        return _run(l0, row, col0, n)
    n0 = (n + 1) // 2
    return _run(l0, row, col0, n0) + _run(l0 + 1, row + 1, col0, n - n0)


def _component_sizes():
    out = []
    lv = _prod8()
    for n in (2, 63, 64, 65, 66, 130):
        for two in (False, True):
            for pattern in ("increasing", "decreasing", "random"):
                rng = np.random.default_rng(n * 7 + two)
                pos = _connected_run(n, two)
                cands = [p + (v,) for p, v in zip(pos, _values(pattern, n, rng))]
                ev = dict(comp_max=("==", n), n=("==", n), out=("==", 0))
                if pattern == "increasing" and not two:
                    ev.update(slots=("==", 1), replace=("==", n - 1))               # one slot walks the whole run
                if pattern == "increasing" and two:                                  # a second slot walks level 1 until it meets the first
                    ev.update(slots=("==", 2 if n > 2 else 1), replace=("==", n - 2 if n > 2 else 1), cross_hit=(">=", 1))
                if pattern == "decreasing" and not two:
                    ev.update(slots=("==", (n + 1) // 2), reject=("==", n // 2))      # every second candidate opens a slot
                if pattern == "decreasing" and two:
                    ev.update(open=("==", ((n + 1) // 2 + 1) // 2), reject=("==", n - ((n + 1) // 2 + 1) // 2), cross_hit=("==", n // 2))
                if pattern == "random" and n > 2:
                    ev.update(tie_reject=(">=", 1), replace=(">=", 1))
                out.append(_case(f"run-{n}-{'two' if two else 'one'}-{pattern}", "sizes", lv, 480, 400, cands, ev))
    # components of exactly bound and bound + 1 candidates, walked with that bound: runs apart from each other, random responses with ties
    for bound in (1, 2, 3, 7):
        rng = np.random.default_rng(900 + bound)
        cands = []
        for k, n in enumerate([bound, bound + 1, bound, bound + 1, 2 * bound + 3, 1, bound + 1]):
            pos = _connected_run(n, two_levels=(k % 2 == 1 and n > 1), row=60 + 20 * k, col0=60 + 10 * k, l0=k % 3)
            cands += [p + (v,) for p, v in zip(pos, _values("random", n, rng))]
        out.append(_case(f"bound-{bound}", "sizes", lv, 480, 400, cands,
                         {"comp_max": ("==", 2 * bound + 3), f"comp_size_{bound}": (">=", 2), f"comp_size_{bound + 1}": (">=", 2)},
                         forms=FORMS + ((1, bound),)))
    return out


def _mixed():
    """lone candidates, small components and two components above the bound in one list: the FIRST opener in scan order belongs to a big
    component, the LAST to a small one (the opener scan numbers the slots of all three paths)"""
    lv = _prod8()
    rng = np.random.default_rng(77)
    cands = []
    for row, col0, n, level in [(50, 40, 70, 0), (70, 60, 1, 0), (70, 100, 1, 0), (70, 140, 1, 0), (90, 50, 5, 0), (90, 200, 17, 0),
                                (120, 44, 66, 0), (150, 60, 3, 0), (60, 70, 1, 1), (80, 50, 9, 1), (130, 60, 3, 1)]:
        pos = _run(level, row, col0, n)
        cands += [p + (v,) for p, v in zip(pos, _values("decreasing" if n <= 3 else "random", n, rng))]
    return [_case("mixed-sizes", "edges", lv, 480, 400, cands,
                  dict(comp_over64=("==", 2), lone=("==", 4), first_opener_comp=(">=", 65), last_opener_comp_small=("==", 1), comp_max=("==", 70)))]


def _moved():
    """a replacement carries a slot into the neighbouring cell (hand-made table: size 3, cells of side 4).  a opens at x = 47 (cell 11),
    b (stronger, 2 away) moves the slot to x = 49 (cell 12); c lies within 3 of the OLD position only and must open a slot; d lies
    within 3 of the NEW position only and must hit, and so does e, exactly 3 from the new position in cell 13: the old cell is not
    among e's 3 x 3 cells, so only the entry the replacement added finds the slot.  Alone (a small component) and with a tail of 70
    linked candidates (handed back)."""
    lv = _hand([(2.0, 1)] * 2, 480, 400)
    core = [(0, 60, 47, 0.002), (0, 60, 49, 0.003), (0, 60, 52, 0.001), (0, 61, 45, 0.001), (0, 61, 51, 0.001)]      # a b e c d
    tail = [(0, 63, 51 + 2 * k, 0.0009 - 0.000001 * k) for k in range(70)]             # (63, 51) lies 2 from d: one component
    ev = dict(moved_cell=(">=", 1), stale_open=("==", 1), moved_hit=("==", 2), boundary_hit=(">=", 1))
    return [_case("moved-small", "edges", lv, 480, 400, core, dict(ev, comp_max=("==", 5), slots=("==", 2)), outcomes="ORrOr"),
            _case("moved-handback", "edges", lv, 480, 400, core + tail, dict(ev, comp_max=("==", 75), comp_over64=("==", 1)))]


def _equal():
    """equal responses keep the earlier slot, inside a level and from class l - 1; one float more replaces it"""
    lv = _prod8()
    v = 0.004
    cands = [(0, 100, 100, v), (0, 100, 102, v), (1, 100, 101, v),                     # O r | r (class 0 slot, equal)
             (0, 120, 100, v), (0, 120, 102, _up(v)), (1, 120, 103, _up(_up(v))),      # O R | R (class 0 slot, one float more)
             (1, 140, 100, v), (1, 140, 102, v), (1, 141, 101, _up(v)), (1, 141, 103, v)]   # O r R r (the last: one float LESS than the slot)
    return [_case("equal-responses", "edges", lv, 480, 400, cands,
                  dict(tie_reject=("==", 3), tie_cross=("==", 1), reject=("==", 4), ulp_replace=("==", 3), ulp_cross=("==", 1), slots=("==", 3)),
                  outcomes="OrOR" + "rR" + "OrRr")]


def _octaves():
    """levels 3 / 4 and 7 / 8 of the product table: a level-l candidate at column c stands at c * ratio WITHOUT the offset, a slot at
    c * ratio + offset, so the rule is not symmetric -- each list has a pair the converted positions put inside and a pair they put
    outside where the other reading (offset on both, or on neither) decides the opposite way"""
    lv = _prod12()
    v = 0.004
    # level 3 slot (ratio 1) at (x, y); level 4 candidate (row r, col c) -> (2c - x, 2r - y) against size_4^2 = 23.04
    a = [(3, 100, 200, v), (4, 51, 102, v / 2),           # (4, 2): 20 hit (with the offset on the candidate too: 26.5, a miss) -> r
         (3, 100, 260, v), (4, 48, 128, v / 2),           # (-4, -4): 32 miss either way (control) -> O
         (3, 100, 320, v), (4, 49, 158, v / 2),           # (-4, -2): 20 hit -> r
         (3, 140, 200, v), (4, 68, 98, v / 2)]            # (-4, -4): 32 miss (control) -> O
    # level 5 slots (ratio 2, offset 0.5) against level 5 candidates: (2 dc - 0.5, 2 dr - 0.5), size_5^2 = 32.6
    a += [(5, 60, 60, v), (5, 60, 63, v / 2),             # (5.5, -0.5): 30.5 hit (symmetric reading: 36, a miss) -> r
          (5, 80, 63, v), (5, 83, 63, v / 2)]             # (-0.5, 5.5): 30.5 hit -> r
    c34 = _case("octave-3-4", "edges", lv, 480, 400, a, dict(ratio_hit=("==", 2), reject=("==", 4), open=("==", 8)), outcomes="OOOO" + "OrrO" + "OrOr")
    # level 7 slot (ratio 2) at 2c' + 0.5; level 8 candidate at 4c: size_8^2 = 92.16.  Level 8 slots at 4c + 1.5: (4 dc - 1.5, 4 dr - 1.5)
    b = [(7, 80, 80, v), (8, 40, 42, v / 2),              # (168 - 160.5, 160 - 160.5) = (7.5, -0.5): 56.5 hit -> r
         (7, 80, 120, v), (8, 39, 58, v / 2),             # (232 - 240.5, 156 - 160.5) = (-8.5, -4.5): 92.5 miss (converted: (-7, -3): 58) -> O
         (7, 120, 80, v), (8, 59, 38, v / 2),             # (152 - 160.5, 236 - 240.5) = (-8.5, -4.5) -> O
         (8, 50, 70, v), (8, 51, 72, v / 2),              # (6.5, 2.5): 48.5 hit -> r
         (8, 60, 72, v), (8, 61, 70, v / 2)]              # (-9.5, 2.5): 96.5 miss (symmetric reading: 80, a hit) -> O
    c78 = _case("octave-7-8", "edges", lv, 480, 400, b, dict(ratio_hit=("==", 1), reject=("==", 2), open=("==", 8)), outcomes="OOO" + "OrOrOOO")
    # hand-made: esigma 2 on both sides of a ratio change, size^2 = 9: pairs exactly on the boundary and one step beyond it
    hl = _hand([(2.0, 1), (2.0, 2)], 240, 200)
    c = [(0, 60, 61, v), (1, 30, 32, v / 2),              # (64 - 61, 60 - 60) = (3, 0): 9, ON the boundary -> r
         (0, 61, 81, v), (1, 32, 42, v / 2),              # (84 - 81, 64 - 61) = (3, 3): 18 -> O
         (0, 64, 101, v), (1, 32, 52, v / 2),             # (104 - 101, 64 - 64) = (3, 0) ... rows: 2 * 32 = 64 -> (3, 0): 9 -> r
         (0, 67, 121, v), (1, 35, 60, v / 2),             # (120 - 121, 70 - 67) = (-1, 3): 10, one step beyond -> O
         (0, 70, 140, v), (1, 35, 72, v / 2),             # (144 - 140, 70 - 70) = (4, 0): 16, one step beyond -> O
         (0, 73, 160, v), (1, 38, 80, v / 2)]             # (160 - 160, 76 - 73) = (0, 3): 9, ON the boundary -> r
    ch = _case("octave-hand-boundary", "edges", hl, 240, 200, c, dict(boundary_cross=("==", 3), reject=("==", 3), open=("==", 9)), outcomes="OOOOOO" + "rOrOOr")
    return [c34, c78, ch]


def _admitted(lv):
    """the innermost rows and columns the border test admits: (rmin, rmax, cmin, cmax)"""
    mid_r, mid_c = lv["h"] // 2, lv["w"] // 2
    cols = [c for c in range(1, lv["w"] - 1) if not _is_out(lv, mid_r, c)]
    rows = [r for r in range(1, lv["h"] - 1) if not _is_out(lv, r, mid_c)]
    return rows[0], rows[-1], cols[0], cols[-1]


def _cells():
    out = []
    # slots on exact multiples of the cell side (hand-made: size 3, G = 4): a lattice around the multiples of 4, distances of exactly 3
    lv = _hand([(2.0, 1)] * 2, 480, 400)
    rng = np.random.default_rng(5)
    cands = {}
    for i in range(2):
        for r in (96, 99, 100, 103, 104, 107, 108):
            for c in (96, 99, 100, 103, 104, 107, 108, 112, 115):
                cands[(i, r + i, c)] = float(rng.choice([0.002, 0.003, 0.004, rng.uniform(0.001, 0.01)]))
    out.append(_case("cell-multiples", "edges", lv, 480, 400, [(i, r, c, v) for (i, r, c), v in cands.items()],
                     dict(cell_multiple=(">=", 20), boundary_hit=(">=", 8), moved_cell=(">=", 3), first_hit_not_nearest=(">=", 1))))
    # the innermost admitted positions on all four sides, with a neighbour each (2 inwards: linked) and the position one step outside
    lv = _prod8()
    cands, n_out = [], 0
    for i, e in enumerate(lv):
        rmin, rmax, cmin, cmax = _admitted(e)
        for r, c, dr, dc in [(rmin, cmin, -1, -1), (rmin, cmax, -1, 1), (rmax, cmin, 1, -1), (rmax, cmax, 1, 1)]:
            cands += [(i, r, c, 0.003), (i, r - 2 * dr // abs(dr) * 0, c - 2 * dc, 0.004), (i, r + dr, c, 0.009), (i, r, c + dc, 0.009)]
            n_out += 2
    out.append(_case("border-innermost", "edges", lv, 480, 400, cands, dict(out=("==", n_out), slots=(">=", 4 * len(lv) // 2), replace=(">=", 8))))
    # the outermost cells a slot can reach: a level whose descriptor reach is 0 (size / ratio < 0.5: esigma 2, ratio 8) admits every
    # position of the level but its rim; the last column and row stand at image - 12.5
    lv = _hand([(2.0, 8)] * 2, 480, 400)
    cands = []
    for i in range(2):
        for r in (1, 2, 47, 48):
            for c in (1, 2, 57, 58):
                cands.append((i, r, c, 0.002 + 0.0001 * ((r * 7 + c * 3 + i) % 5)))
    out.append(_case("last-cells", "edges", lv, 480, 400, cands, dict(out=("==", 0), slots=("==", 32), max_cell_x=("==", 467 // 4), max_cell_y=("==", 387 // 4))))
    return out


def _upper():
    v, s = 0.002, 0.003
    out = []
    # hand-made: size_0 = 6 and size_1 = 3 (ratio 1), so a level-1 candidate 5 or 6 from a class-0 slot does not see it in the walk
    # (25, 36 > 9) and opens a LATER slot of class 1 inside the class-0 slot's size
    hl = _hand([(4.0, 1), (2.0, 1)], 480, 400)
    out.append(_case("upper-hand-later-stronger", "edges", hl, 480, 400, [(0, 100, 100, v), (1, 100, 105, s)],
                     dict(up_drop=("==", 1), slots=("==", 2), kept=("==", 1)), outcomes="OO"))
    out.append(_case("upper-hand-later-equal", "edges", hl, 480, 400, [(0, 100, 100, v), (1, 100, 105, v)],
                     dict(up_tie=("==", 1), up_drop=("==", 0), slots=("==", 2), kept=("==", 2)), outcomes="OO"))
    out.append(_case("upper-hand-exact-distance", "edges", hl, 480, 400, [(0, 100, 100, v), (1, 100, 106, s), (0, 140, 100, v), (1, 140, 107, s)],
                     dict(up_boundary=("==", 1), up_drop=("==", 1), slots=("==", 4), kept=("==", 3)), outcomes="OOOO"))
    # the class-1 slot stands EARLIER: slot 0 opened at level 0, slot 1 opened at level 0 (8 away), then a level-1 candidate exactly 3
    # from slot 0 replaces it -- slot 0 is now class 1, 5 from slot 1 and stronger, but not later: slot 1 stays
    out.append(_case("upper-hand-earlier", "edges", hl, 480, 400, [(0, 100, 200, v), (0, 100, 208, v), (1, 100, 203, s)],
                     dict(up_earlier=("==", 1), up_drop=("==", 0), boundary_hit=("==", 1), slots=("==", 2), kept=("==", 2)), outcomes="OOR"))
    # the product table.  Inside an octave only the earlier variant exists (module docstring); levels 0 / 1:
    pl = _prod8()
    out.append(_case("upper-product-earlier", "edges", pl, 480, 400, [(0, 100, 100, v), (0, 100, 104, v), (1, 100, 102, s)],
                     dict(up_earlier=("==", 1), up_drop=("==", 0), slots=("==", 2), kept=("==", 2)), outcomes="OOR"))
    # levels 7 / 8: the level-8 candidate stands (-8.5, -4.5) from the class-7 slot in the walk (92.5 > 92.16: a new, later slot) and
    # (-7, -3) from it once converted (58 <= 65.2: inside the class-7 slot's size)
    p12 = _prod12()
    out.append(_case("upper-product-later-stronger", "edges", p12, 480, 400, [(7, 82, 84, v), (8, 40, 40, s)],
                     dict(up_drop=("==", 1), slots=("==", 2), kept=("==", 1)), outcomes="OO"))
    out.append(_case("upper-product-later-equal", "edges", p12, 480, 400, [(7, 82, 84, v), (8, 40, 40, v)],
                     dict(up_tie=("==", 1), up_drop=("==", 0), slots=("==", 2), kept=("==", 2)), outcomes="OO"))
    # several of each in one list, in both tables' cell grids: the filter's buckets hold more than one slot per cell
    cands = []
    for k in range(12):
        cands += [(0, 100 + 20 * (k // 4), 100 + 40 * (k % 4), v), (1, 100 + 20 * (k // 4), 105 + 40 * (k % 4) + (k % 3 == 2), s if k % 2 else v)]
    out.append(_case("upper-hand-many", "edges", hl, 480, 400, cands, dict(up_drop=("==", 6), up_tie=("==", 6), up_boundary=("==", 2), slots=("==", 24), kept=("==", 18))))
    return out


def _sized_list(n, seed):
    rng = np.random.default_rng(seed)
    lv = _prod8()
    if n < 2:
        return [(0, 100, 100, 0.004)][:n]
    big = _random_list(rng, lv, 3, n_clusters=max(2, n // 12), per_cluster=14, spread=2.5)
    assert len(big) >= n - 1
    pick = sorted(rng.choice(len(big), n - 1, replace=False).tolist())
    return [big[k] for k in pick] + [(3, 200, 240, 0.004)]          # the last candidate of the list stands alone: it opens the last slot


def _lengths():
    out = []
    lv = _prod8()
    for n in (0, 1, 255, 256, 257, 1023, 1024, 1025, 2049):
        ev = dict(n=("==", n))
        if n > 1:
            ev.update(open=(">=", n // 8), replace=(">=", n // 64), reject=(">=", n // 8))
        if n > 1024:
            ev.update(openers_after_1024=(">=", 1), openers_before_1024=(">=", 1), last_is_opener=("==", 1))   # the opener scan carries into its second chunk
        out.append(_case(f"length-{n}", "lengths", lv, 480, 400, _sized_list(n, 40 + n), ev))
    out.append(_case("batch", "lengths", lv, 480, 400, None, dict(n=("==", 2049)), lists=[_sized_list(2049, 7), [], [(1, 100, 100, 0.004)]]))
    return out


def _contention():
    """about 8,000 candidates in clusters tight enough that the unions of many 256-candidate workgroups meet in the same components"""
    rng = np.random.default_rng(11)
    lv = _prod8()
    cands = _random_list(rng, lv, 4, n_clusters=13, per_cluster=190, spread=6.0)
    return [_case("contention", "contention", lv, 480, 400, cands,
                  dict(n=(">=", 7000), comp_over64=(">=", 10), comp_max=(">", 256), blocks_in_one_component=(">=", 3)), repeats=3)]


_ALL = None


def all_cases():
    global _ALL
    if _ALL is None:
        _ALL = _existing_families() + _component_sizes() + _mixed() + _moved() + _equal() + _octaves() + _cells() + _upper() + _lengths() + _contention()
        assert len({c["name"] for c in _ALL}) == len(_ALL)
    return _ALL


def case_events(case):
    """trace() of lists[0] with the events that need the case's own structure added"""
    cands = case["lists"][0]
    aux, kept, outcomes, ev, opener, roots = trace(case["levels"], cands)
    sizes = np.bincount(roots[roots >= 0]) if len(cands) and (roots >= 0).any() else np.zeros(1, np.int64)
    for s, cnt in Counter(sizes[sizes > 0].tolist()).items():
        ev[f"comp_size_{s}"] = cnt
    if opener:
        ev["first_opener_comp"] = int(sizes[roots[opener[0]]])
        ev["last_opener_comp_small"] = int(2 <= sizes[roots[opener[-1]]] <= 64)
        ev["openers_after_1024"] = sum(k >= 1024 for k in opener)
        ev["openers_before_1024"] = sum(k < 1024 for k in opener)
        ev["last_is_opener"] = int(opener[-1] == len(cands) - 1)
    if aux.n:
        G = int(_size(case["levels"][0])) + 1
        ev["max_cell_x"], ev["max_cell_y"] = int(aux.x[:aux.n].max()) // G, int(aux.y[:aux.n].max()) // G
    if len(cands) and (roots >= 0).any():
        idx = np.arange(len(cands))
        span = max(len(set((idx[roots == r] // 256).tolist())) for r in np.flatnonzero(sizes > 64))if (sizes > 64).any() else 0
        ev["blocks_in_one_component"] = span
    return aux, kept, outcomes, ev


# ---------------------------------------------------------------------------------------------------- the GPU child
def child_main(job_path, out_path):
    """runs in a child process of the GPU test (the session's process holds the product library): loads the developer library, runs
    every job -- (key, levels, w, h, lists, parallel, bound) -- through r3dm_dev_akaze_classic_walk and pickles {key: per-image results}.
    Stops at the first error: the file then holds {"__error__": text} beside the results so far."""
    import pickle
    from regard3d_amd import api
    api.use_developer_library()
    jobs = pickle.load(open(job_path, "rb"))
    res = {}
    try:
        ctx = api.Context(0)
        for key, levels, w, h, lists, parallel, bound in jobs:
            res[key] = ctx.dev_akaze_classic_walk(levels, w, h, lists, bool(parallel), bound)
        ctx.close()
    except Exception as e:                        # (reported to the parent, which decides; nothing more runs on the GPU here)
        res["__error__"] = f"{type(e).__name__}: {e}"
    pickle.dump(res, open(out_path, "wb"))
    return 3 if "__error__" in res else 0
