"""The inputs of the match-budget tests (tests/test_gpu_budget.py), built so that each reaches the edges the feature has, and the
conditions that say so (tests/test_budget_cases.py proves them on the restatement alone, without a GPU).

A matching case is a set of ragged views cut from two related views (view J is view I lightly perturbed), the last one noise, with
one priority per scene point -- shared points rank alike across views -- in eight tied classes, and:
    rows TOP (5 and 9) carry the two highest priorities of all: at N = 2 every view long enough selects exactly them, so the budgeted
        graph is not empty and S is not a prefix;
    row DUP (12) of every I-side view is a near copy of row 9 (one element or bit changed) with priority 0: on the whole views the
        ratio test refuses the query that observes row 9 (its runner-up is as near as its nearest), on the sub-views the runner-up
        lies outside S and the query is accepted -- the budgeted graph is NOT the full graph restricted to S;
    rows 0 .. 3 carry the priorities (c, c, c, b), b < c: in the 4-row view the tie class of c straddles the cut at N = 2;
    every seventh row shares its position with the row before it (the coordinate de-duplication has something to do)."""
import numpy as np

import budget_restatement as B

ROWS = (1, 2, 4, 31, 33, 64, 65, 66, 257, 300, 40)      # the last view is noise
BUDGETS = (2, 33, 64, 65)
TOP, DUP = (5, 9), 12
# (name, dim, dtype, bytes per binary row, ratio, squared metric)
KINDS = [("f32_64", 64, np.float32, None, 0.6, True), ("f32_128", 128, np.float32, None, 0.6, True), ("f32_144", 144, np.float32, None, 0.6, True),
         ("f32_37", 37, np.float32, None, 0.6, True), ("u8_128", 128, np.uint8, None, 0.6, True),
         ("bin_32", 0, np.uint8, 32, 0.8, False), ("bin_61", 0, np.uint8, 61, 0.8, False)]


def positions(descs):
    out = []
    for k, d in enumerate(descs):
        r = np.arange(len(d))
        r = np.where(r % 7 == 6, r - 1, r)                            # every seventh row sits on the row before it
        out.append(np.stack([r * 3.0 + k, r * 2.0 + 5.0], 1).astype(np.float32))
    return out


def make_views(kind, seed=0, rows=ROWS, real=False):
    """-> (descs, xys, prios, binary, ratio, squared)"""
    name, dim, dtype, nbytes, ratio, squared = next(k for k in KINDS if k[0] == kind)
    rng = np.random.default_rng(7000 + seed + sum(map(ord, name)))
    n = max(rows)
    binary = nbytes is not None
    if binary:
        dI = rng.integers(0, 256, (n, nbytes), dtype=np.uint8)
        flip = lambda a: a ^ np.packbits(rng.random((len(a), nbytes * 8)) < 0.02, axis=1)
        dI[DUP] = dI[TOP[1]]; dI[DUP, 0] ^= np.uint8(1)               # one bit away
        dJ = flip(dI)
        noise = lambda m: rng.integers(0, 256, (m, nbytes), dtype=np.uint8)
    elif real:
        dI = rng.standard_normal((n, dim)).astype(np.float32)
        jitter = lambda a: (a + 0.05 * rng.standard_normal(a.shape)).astype(np.float32)
        dI[DUP] = dI[TOP[1]]; dI[DUP, 0] += np.float32(0.01)
        dJ = jitter(dI)
        noise = lambda m: rng.standard_normal((m, dim)).astype(np.float32)
    else:
        dI = rng.integers(0, 121, (n, dim)).astype(np.float32)
        jitter = lambda a: np.clip(a + rng.integers(-2, 3, a.shape).astype(np.float32), 0, 255)
        dI[DUP] = dI[TOP[1]]; dI[DUP, 0] += np.float32(1.0)           # one step away on one element
        dJ = jitter(dI)
        dI = dI.astype(dtype); dJ = dJ.astype(dtype)
        noise = lambda m: rng.integers(0, 121, (m, dim)).astype(dtype)
    shared = rng.integers(0, 8, n).astype(np.float32) * np.float32(0.75)
    shared[:4] = np.float32([3.75, 3.75, 3.75, 1.5])
    shared[TOP[0]] = np.float32(9.0); shared[TOP[1]] = np.float32(8.25)
    shared[DUP] = np.float32(0.0)
    descs, prios = [], []
    for k, m in enumerate(rows):
        unrelated = k == len(rows) - 1
        descs.append(noise(m) if unrelated else np.ascontiguousarray((dI if k % 2 == 0 else dJ)[:m]))
        prios.append(np.ascontiguousarray(shared[:m]))
    return descs, positions(descs), prios, binary, ratio, squared


def all_ordered_pairs(n):
    return np.array([(i, j) for i in range(n) for j in range(n) if i != j], np.uint32)


def conditions(O, descs, xys, prios, pairs, N, ratio, squared, binary, mode="off"):
    """the four conditions of a matching case on the restatement alone -> dict of bools (+ the figures behind them)"""
    ns = [len(d) for d in descs]
    rows = [B.selected_rows(prios[v], ns[v], N) for v in range(len(descs))]
    counts, mapped, sub = B.match_collection(O, descs, xys, prios, pairs, N, ratio, squared, binary, mode)
    wc, wm = B.whole_collection(O, descs, xys, pairs, ratio, squared, binary, mode)
    # 3: a query of some pair matched differently on the sub-views than on the whole views
    differs, off_b, off_w = 0, 0, 0
    for k, (I, J) in enumerate(pairs):
        b = {(int(i), int(j)) for i, j in mapped[off_b:off_b + int(counts[k])]}
        w = {(int(i), int(j)) for i, j in wm[off_w:off_w + int(wc[k])]}
        off_b += int(counts[k]); off_w += int(wc[k])
        SI, SJ = set(rows[int(I)].tolist()), set(rows[int(J)].tolist())
        w_in = {(i, j) for i, j in w if i in SI and j in SJ}
        differs += len(b ^ w_in)
    return dict(budgeted_and_whole=any(n > N for n in ns) and any(0 < n <= N for n in ns),
                non_empty_and_remapped=len(mapped) > 0 and bool((mapped != sub).any()),
                not_the_restriction=differs > 0,
                tie_straddles=any(B.tie_straddles_cut(prios[v], ns[v], N) for v in range(len(descs))),
                n_matches=int(len(mapped)), n_differ=int(differs))


# ---------------------------------------------------------------------------------------------------- the selection cases
def selection_sizes(chunk):
    return (1, 2, 63, 64, 65, chunk - 1, chunk, chunk + 1, 3 * chunk + 7)


def selection_budgets(n):
    return sorted({N for N in (2, 63, 64, 65, n - 1, n, n + 1) if N >= 2})


PATTERNS = ("increasing", "equal", "three_values", "lowest_bit", "subnormals", "none")


def priority_pattern(pattern, n, N, seed=0):
    """one priority per row (None: the view has no priority)"""
    rng = np.random.default_rng(9000 + seed + n * 31 + N)
    if pattern == "none":
        return None
    if pattern == "increasing":
        return (np.arange(n, dtype=np.float32) * np.float32(0.5)).astype(np.float32)
    if pattern == "equal":
        return np.full(n, 2.5, np.float32)
    if pattern == "three_values":
        # the cut inside the middle class: fewer than min(N, n) rows above it, more than that with it
        hn = min(N, n)
        top = hn // 3
        mid = min(n - top, max(hn - top + 1, (n - top) // 2))
        p = np.r_[np.full(top, 3.0, np.float32), np.full(mid, 2.0, np.float32), np.full(n - top - mid, 1.0, np.float32)]
        return rng.permutation(p).astype(np.float32)
    if pattern == "lowest_bit":
        base = np.float32(1.5).view(np.uint32)
        return (base + rng.integers(0, 2, n).astype(np.uint32)).view(np.float32)
    if pattern == "subnormals":
        bits = rng.integers(0, 4, n).astype(np.uint32)                   # +0.0 and the three smallest subnormals ...
        p = bits.view(np.float32).copy()
        p[rng.random(n) < 0.2] = np.float32(-0.0)                        # ... and -0.0, stored as +0.0
        return p
    raise ValueError(pattern)
