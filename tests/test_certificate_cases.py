"""CPU proof that the case table of the certificate tests (tests/certificate_cases.py) sits where it claims to, from the oracle and
the restatements alone -- no GPU and no code under test.

  bound     |emulated key + ||q||^2 - oracle distance| <= slack on the ten smallest keys of every query, for every case under the
            sequential order and for a third of them (ALL_ORDERS: every family, path, padded length and scale) under every order:
            the derivation behind MatchParams::err_scale (api_match.cpp; DESIGN.md 4.1 "Certification") against data
  regime    under the sequential order, "easy" cases leave at most 5 % of their queries uncertified, "hard" (and "teeth") cases at
            least 95 %, "transition" cases lie strictly between 10 % and 90 % with at least two per path, and a slack of zero
            certifies at least 20 wrong nominations in every "teeth" case
  data      finite values, at least two dataset rows, and the path a case names is the one the host's rules give it

`pytest -s` prints the regime table and the largest error / slack per path and padded length (recorded in DESIGN.md 4.1).
"""
import collections

import numpy as np
import pytest

import certificate_cases as CC

_MEASURED = {}

# the bound is checked under the sequential order on every case, and under every order (exact k-steps of 2 and 16, the pairwise tree,
# the hi/lo f16 planes) on these: every family, path, padded length and view scale, and the cases of the largest norms
ALL_ORDERS = frozenset(
    [f"offset_{p}_d128_t{t}" for p in ("f32", "split") for t in (0, 3000)] +
    [f"offset_f32_d{d}_t{t}" for d, t in ((37, 20), (64, 1000), (100, 20), (144, 20), (256, 1000))] +
    [f"offset_split_d{d}_t{t}" for d, t in ((37, 300), (64, 10), (100, 10), (144, 300), (256, 10))] +
    ["mixed_half_f32_t100", "mixed_large_last_f32", "mixed_large_row0_split", "mixed_large_queries_f32_t3000", "mixed_large_dataset_f32_t3000",
     "mixed_large_queries_split_t3000", "mixed_large_dataset_split_t3000", "ladder_last_partial_tile_f32", "ladder_last_partial_tile_split",
     "counts_t0_top40", "counts_t40_top20", "counts_t40_top20_scale_small", "counts_t40_top20_scale_large", "counts_t0_top40_scale_mixed",
     "split_off_lattice_t40_top20_scale_small", "split_off_lattice_t40_top20_scale_large", "split_signed_t0_top40_scale_mixed", "split_signed_t40_top20"])


def _measure(name):
    """keys in every order, reference distances and the verdicts under the sequential order -- once per case and session"""
    if name not in _MEASURED:
        case = CC.CASES[name]
        a, b = case.make()
        dist = CC.ref_distances(a, b)
        orders = ("seq",)
        if name in ALL_ORDERS:
            orders = CC.ORDERS + (("split16",) if case.path != "f32" else ())
        keys = {o: CC.emulated_keys(a, b, o) for o in orders}
        nb = CC.norms_f32(b)
        sl = CC.case_slack(case.path, a, b)
        worst = {}
        for o, k in keys.items():
            top = CC._smallest(k, 10)
            err = np.abs(np.take_along_axis(k, top, 1).astype(np.float64) + nb[:, None].astype(np.float64) - np.take_along_axis(dist, top, 1))
            worst[o] = float((err / sl[:, None].astype(np.float64)).max())
        v = CC.certify(a, b, case.path, keys=keys["seq"], dist=dist)
        v0 = CC.certify(a, b, case.path, keys=keys["seq"], dist=dist, permille=0)
        v2 = CC.certify(a, b, case.path, keys=keys["seq"], dist=dist, second_chance=True) if case.path != "f32" else v
        _MEASURED[name] = dict(worst=worst, uncertified=float(np.mean(v == CC.UNCERTIFIED)), wrong=int((v == CC.WRONG).sum()),
                               wrong_at_zero=int((v0 == CC.WRONG).sum()), queries=len(b),
                               uncertified_after_second_chance=float(np.mean(v2 == CC.UNCERTIFIED)), wrong_after_second_chance=int((v2 == CC.WRONG).sum()))
    return _MEASURED[name]


def test_case_table_covers_what_it_names():
    assert len(CC.CASES) >= 80
    assert ALL_ORDERS <= set(CC.CASES)
    for path in CC.PATHS:
        names = [n for n, c in CC.CASES.items() if c.path == path]
        assert CC.CASES[names[0]].regime == "easy" and CC.CASES[names[-1]].regime == "teeth", path       # the GPU test reads first and last
    dims = {c.make()[0].shape[1] for c in CC.CASES.values() if c.family == "offset"}
    assert dims >= {37, 64, 100, 128, 144, 256}
    assert all(len(ts) >= 8 and ts[0] == 0 and ts[-1] == 3000 for ts in CC.OFFSETS.values())
    for fam, members in CC.FAMILIES.items():
        assert members, fam
    assert sum(c.tie for c in CC.CASES.values()) >= 2
    for name, case in CC.CASES.items():
        a, b = case.make()
        mk = case._make
        a2, b2 = mk()
        assert np.array_equal(a, a2) and np.array_equal(b, b2), name                  # reproducible from the seed
        assert a.shape[0] % CC.TILE_ROWS != 0 and b.shape[0] % CC.TILE_ROWS != 0, name  # ragged last tiles on both sides


def test_reference_distance_restatement_is_the_oracles(oracle):
    """ref_distances is what every placement below is built from: bit for bit the oracle's 2-NN, scalar tail included"""
    for name in ("offset_f32_d37_t20", "offset_f32_d128_t20", "offset_split_d100_t10", "counts_t40_top40", "ladder_tie_f32"):
        a, b = CC.CASES[name].make()
        idx, dist = CC.true_top2(CC.ref_distances(a, b))
        oi, od = oracle.knn2(a, b)
        assert np.array_equal(dist, od) and np.array_equal(idx, oi), name


@pytest.mark.parametrize("name", list(CC.CASES))
def test_conditions_on_the_data(name):
    case = CC.CASES[name]
    a, b = case.make()
    assert np.isfinite(a).all() and np.isfinite(b).all()
    assert a.shape[0] >= 2 and b.shape[0] >= 1 and a.shape[1] == b.shape[1]
    assert a.dtype == np.float32 and b.dtype == np.float32
    assert CC.path_eligible(case.path, a, b)
    if case.path != "f32":
        assert not CC.path_eligible("counts" if case.path == "split" else "split", a, b)     # and for no other opt-in path


@pytest.mark.parametrize("name", [n for n, c in CC.CASES.items() if c.family == "ladder"])
def test_ladder_rows_sit_where_the_placement_says(name):
    """from the reference's distances: the three planted rows are the three nearest, in order; the runner-up and the third are
    distinct rows at distinct f32 distances (equal ones in the tie cases) in the lane halves and tiles the placement names"""
    case = CC.CASES[name]
    a, b = case.make()
    dist = CC.ref_distances(a, b)
    order = np.lexsort((np.broadcast_to(np.arange(a.shape[0]), dist.shape), dist), axis=1)[:, :3]
    placement = next(p for p in CC.PLACEMENTS if p in name) if not case.tie else "opposite_halves"
    n_full = a.shape[0] // CC.TILE_ROWS
    gaps = []
    for j in range(len(b)):
        r1, r2, r3 = CC.ladder_rows(placement, j, n_full, a.shape[0] - n_full * CC.TILE_ROWS)
        assert tuple(order[j]) == (r1, r2, r3), (name, j)
        d1, d2, d3 = dist[j, r1], dist[j, r2], dist[j, r3]
        assert d1 < d2 and ((d2 == d3) if case.tie else (d2 < d3)), (name, j)
        gaps.append(float(d3) - float(d2))
        t2, t3, h2, h3 = r2 // CC.TILE_ROWS, r3 // CC.TILE_ROWS, CC._lane_half(r2 % CC.TILE_ROWS), CC._lane_half(r3 % CC.TILE_ROWS)
        if placement == "same_half":
            assert t2 == t3 and h2 == h3
        elif placement == "opposite_halves":
            assert t2 == t3 and h2 != h3
        elif placement == "different_tiles":
            assert t2 != t3
        else:
            assert t2 == t3 == n_full and a.shape[0] % CC.TILE_ROWS != 0
    if not case.tie:
        sl = float(np.median(CC.case_slack(case.path, a, b)))
        assert min(gaps) < sl / 64 and max(gaps) > 8 * sl                       # the ladder runs from far below the slack to far above it


@pytest.mark.parametrize("name", list(CC.CASES))
def test_key_error_stays_within_the_slack(name):
    m = _measure(name)
    print(name, {o: round(w, 4) for o, w in m["worst"].items()})
    for order, w in m["worst"].items():
        assert w <= 1.0, (name, order, w)
    assert m["wrong"] == 0, name              # with the full slack no emulated nomination is certified wrongly


@pytest.mark.parametrize("name", list(CC.CASES))
def test_case_meets_its_regime(name):
    case, m = CC.CASES[name], _measure(name)
    u = m["uncertified"]
    print(f"{name:44s} {case.path:6s} {case.regime:10s} uncertified {u:.3f}  certified wrongly at zero slack {m['wrong_at_zero']} of {m['queries']}")
    if case.regime == "easy":
        assert u <= 0.05
    elif case.regime == "transition":
        assert 0.10 < u < 0.90
    else:
        assert u >= 0.95
    if case.regime == "teeth":
        assert m["wrong_at_zero"] >= 20
    # what the device's band (Case.device_band, asserted per case by tests/test_gpu_certificate.py) rests on for the paths with the
    # four-nominee second chance: it certifies nothing wrongly, only ever certifies more, and leaves the hard cases hard unless
    # the case says it rescues them
    if case.path != "f32":
        u2 = m["uncertified_after_second_chance"]
        print(f"{'':44s} after the second chance {u2:.3f}")
        assert m["wrong_after_second_chance"] == 0 and u2 <= u
        if case.regime in ("hard", "teeth"):
            assert (u2 <= 0.05) if case.rescued else (u2 >= 0.95)
    lo, hi = case.device_band()
    assert lo <= (u if case.path == "f32" else m["uncertified_after_second_chance"]) <= hi


def _planted(name, bug):
    """share of uncertified queries of a case under the host's slack and under a slack with one planted bug"""
    case = CC.CASES[name]
    a, b = case.make()
    na, nb = CC.norms_f32(a), CC.norms_f32(b)
    ks = CC.split_k_of(float(np.abs(a).max())) + CC.split_k_of(float(np.abs(b).max())) if case.path == "split" else 0
    max_norm, q_norm = {"max_norm_of_the_query_view": (nb.max(), nb),
                        "query_norm_dropped": (na.max(), np.zeros_like(nb)),
                        "last_partial_tile_skipped": (na[:len(na) // CC.TILE_ROWS * CC.TILE_ROWS].max(), nb),
                        "row_0_skipped": (na[1:].max(), nb)}[bug]
    keys, dist = CC.emulated_keys(a, b, "seq"), CC.ref_distances(a, b)
    sc = case.path != "f32"
    good = CC.certify(a, b, case.path, keys=keys, dist=dist, second_chance=sc)
    bad = CC.certify(a, b, case.path, keys=keys, dist=dist, second_chance=sc, slack_of=CC.slack(case.path, CC.dpad_of(a.shape[1]), max_norm, q_norm, ks))
    return float(np.mean(good == CC.UNCERTIFIED)), float(np.mean(bad == CC.UNCERTIFIED)), int((bad == CC.WRONG).sum())


@pytest.mark.parametrize("path", ["f32", "split"])
@pytest.mark.parametrize("stem,bug", [("mixed_large_dataset_%s_t3000", "max_norm_of_the_query_view"), ("mixed_large_queries_%s_t3000", "query_norm_dropped"),
                                      ("mixed_large_last_%s", "last_partial_tile_skipped"), ("mixed_large_row0_%s", "row_0_skipped")])
def test_mixed_norm_cases_notice_a_slack_from_the_wrong_view(path, stem, bug):
    """What the mixed-norm family is for.  A slack that reads max||a||^2 of the wrong view, drops ||q||^2, or misses the one large row
    gives no wrong 2-NN on these views (the gaps are wide) -- it certifies queries that the right slack sends to the exact scan:
    the share of uncertified queries falls from the case's band (hard: at least 95 %) to at most 5 %.  The GPU test asserts every
    case's share against its band, so each of these bugs fails it."""
    good, bad, wrong = _planted(stem % path, bug)
    print(stem % path, bug, "uncertified", good, "->", bad, "certified wrongly", wrong)
    lo, hi = CC.CASES[stem % path].device_band()
    assert lo <= good <= hi and lo >= 0.95
    assert bad <= 0.05


def test_every_path_has_its_transition_and_the_bound_its_margin():
    between = collections.Counter()
    worst = collections.defaultdict(float)
    for name, case in CC.CASES.items():
        m = _measure(name)
        if 0.10 < m["uncertified"] < 0.90:
            between[case.path] += 1
        key = (case.path, CC.dpad_of(case.make()[0].shape[1]))
        worst[key] = max(worst[key], max(m["worst"].values()))
    for path in CC.PATHS:
        assert between[path] >= 2, (path, dict(between))
    print("largest |key + ||q||^2 - distance| / slack over all cases and orders, per (path, padded length):")
    for key in sorted(worst):
        print(f"  {key[0]:6s} Dpad {key[1]:3d}  {worst[key]:.4f}")
    assert max(worst.values()) <= 1.0


def test_match_collections_reach_no_match_and_matches(oracle):
    """the match-mode collections have queries on both sides of the looser ratios (under the squared metric the strict ones reach
    `no_match` alone): some match, most do not"""
    for name, (views, pairs) in CC.collections().items():
        assert all(np.isfinite(v).all() and v.shape[0] >= 2 for v in views), name
        got = [int(oracle.match_collection(views, None, pairs, r, True)[0].sum()) for r in CC.RATIOS]
        print(name, dict(zip(CC.RATIOS, got)))
        assert got == sorted(got) and got[-1] > got[0], name
        assert got[0] < sum(views[j].shape[0] for _, j in pairs.tolist()), name
