"""The f16 prefix test of l2_knn2_half_kernel (r3dm_set_half_prefix) in numpy, on the CPU: the rounding of its table value by value, the
worst cases of the bound marginQ is derived from (kernels_match.hip above the kernel), and the model (tools/prefix_prune_model.py,
model_pair_levels with prefix16) on every view pair of tests/half_prefix_cases.py -- each case reaches the edge it is built for, and
the f16 test never prunes a tile the restart's own prefix test keeps."""
import numpy as np
import pytest

import half_prefix_cases as QC
import test_half_filter_model as HM

M = HM.M
GP = 12
U = 2.0 ** -24


def test_rows_to_half_value_by_value():
    f32 = lambda v: np.array(v, np.float32)
    x = f32([0.0, -0.0, 1.0, -1.0, np.nan, np.inf, -np.inf,
             2.0 ** -14, -(2.0 ** -14), 2.0 ** -14 * (1 - 2.0 ** -24), 2.0 ** -15, 1e-30, 2.0 ** -14 * (1 + 2.0 ** -11), 2.0 ** -14 * (1 + 2.0 ** -11 + 2.0 ** -23),
             32752.0, -32752.0, 32752.002, 32768.0, 40000.0, 65504.0, 65505.0, -70000.0,
             1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -23, 1 + 2.0 ** -11 - 2.0 ** -23, 2.0 ** 14, 2.0 ** 14 * (1 + 2.0 ** -17)])
    h = M.rows_to_half(x)
    want = [0.0, 0.0, 1.0, -1.0, np.nan, np.nan, np.nan,
            2.0 ** -14, -(2.0 ** -14), 0.0, 0.0, 0.0, 2.0 ** -14, 2.0 ** -14 * (1 + 2.0 ** -10),                # the flush below 2^-14; a tie goes to even
            32752.0, -32752.0, np.nan, np.nan, np.nan, np.nan, np.nan, np.nan,                                  # the cut: everything above 32,752 is a NaN
            1.0, 1 + 2.0 ** -9, 1 + 2.0 ** -10, 1.0, 2.0 ** 14, 2.0 ** 14]                                      # ties to even, to nearest on either side
    assert np.array_equal(h, np.array(want), equal_nan=True), (h, want)
    assert not np.signbit(h[1])                                       # a flushed value is +0
    # every value it keeps is numpy's round-to-nearest-even f16, no subnormal among them, and -2 x it is a finite f16
    rng = np.random.default_rng(5)
    y = (rng.standard_normal(200000) * np.exp2(rng.integers(-20, 16, 200000))).astype(np.float32)
    hy = M.rows_to_half(y)
    kept = (np.abs(y) >= np.float32(2.0 ** -14)) & (np.abs(y) <= np.float32(32752.0))
    assert np.array_equal(hy[kept], y[kept].astype(np.float16).astype(np.float64))
    assert (np.abs(hy[kept]) >= 2.0 ** -14).all() and np.isfinite((hy[kept] * -2.0).astype(np.float16)).all()
    assert (hy[np.abs(y) < np.float32(2.0 ** -14)] == 0).all() and np.isnan(hy[np.abs(y) > np.float32(32752.0)]).all()
    assert (np.abs(hy[kept] - y[kept].astype(np.float64)) <= 2.0 ** -11 * np.abs(y[kept].astype(np.float64))).all()


def _rounding_loss(a, q):
    """D = 2 sum |a_i q_i - A_i Q_i| over the prefix, S = |a_P|^2 + |q_P|^2, in float64 (exact for these operands)"""
    a64, q64 = a.astype(np.float64), q.astype(np.float64)
    A, Q = M.rows_to_half(a), M.rows_to_half(q)
    return 2.0 * np.abs(a64 * q64 - A * Q).sum(), (a64 * a64).sum() + (q64 * q64).sum()


WORST = {
    # every prefix element at a rounding midpoint of f16, the signs aligned: each product loses (1 + 2^-11)^2 - 1 of itself
    "midpoints": (np.full(96, 1 + 2.0 ** -11, np.float32) * np.float32(32.0), np.full(96, 1 + 2.0 ** -11, np.float32) * np.float32(32.0)),
    "midpoints, odd significands": (np.full(96, 1 + 3 * 2.0 ** -11, np.float32) * np.float32(-8.0), np.full(96, 1 + 3 * 2.0 ** -11, np.float32) * np.float32(-8.0)),
    # all of a row's weight in one element at 2^14
    "one element at 2^14": (np.eye(1, 96, 0, np.float32)[0] * np.float32(2.0 ** 14), np.eye(1, 96, 0, np.float32)[0] * np.float32(2.0 ** 14)),
    # every element of one row just below 2^-14 (flushed) against the largest kept values; and the mirror
    "flushed against the cut": (np.full(96, 2.0 ** -14 * (1 - 2.0 ** -24), np.float32), np.full(96, 32752.0, np.float32)),
    "the cut against flushed": (np.full(96, -32752.0, np.float32), np.full(96, 2.0 ** -14 * (1 - 2.0 ** -24), np.float32)),
    "flushed against flushed": (np.full(96, 2.0 ** -14 * (1 - 2.0 ** -24), np.float32), np.full(96, 2.0 ** -14 * (1 - 2.0 ** -24), np.float32)),
    "flushed against unit rows": (np.full(96, 2.0 ** -14 * (1 - 2.0 ** -24), np.float32), np.full(96, 96 ** -0.5, np.float32)),
    "just above 2^-14 at midpoints": (np.full(96, 2.0 ** -14 * (1 + 2.0 ** -11), np.float32), np.full(96, 2.0 ** -14 * (1 + 3 * 2.0 ** -11), np.float32)),
}


@pytest.mark.parametrize("name", list(WORST))
def test_worst_cases_of_the_bound(name):
    """the derivation's two steps hold on the worst operands: D <= (2^-10 + 2^-22 + 2^-15) S + 3 x 2^-8, and marginQ covers D and both
    evaluation errors, 771 u (1 + 2^-16) M, with M >= S / (1 + 2^-16)"""
    a, q = WORST[name]
    D, S = _rounding_loss(a, q)
    print(name, "D", D, "S", S, "D / S", D / S)
    assert D <= (2.0 ** -10 + 2.0 ** -22 + 2.0 ** -15) * S + 3 * 2.0 ** -8
    Mn = S / (1 + 2.0 ** -16)                                          # the smallest M the stored norms allow for this S
    assert M.PREFIX_MARGIN * Mn + M.PREFIX_MARGIN_ABS >= D + 771 * U * (1 + 2.0 ** -16) * Mn * (1 + 2.0 ** -16)
    if name == "midpoints":
        assert D > 0.999 * 2.0 ** -10 * S                             # the bound's leading term is reached
    if name == "flushed against the cut":
        assert D > 0.99 * 2 * 96 * 2.0 ** -14 * 32752.0                # ... and the flush's


CASES = QC.all_cases(M)


@pytest.mark.parametrize("name,a,b,R,must_prune", CASES, ids=[c[0] for c in CASES])
def test_the_cases_reach_their_edge(name, a, b, R, must_prune):
    r = M.model_pair_levels(a, b, GP, R, skip="lane", prefix16=True)
    r0 = M.model_pair_levels(a, b, GP, R, skip="lane")
    print(name, {k: r[k] for k in ("tiles", "pruned", "filtered", "half", "skipped", "reach", "prefix_pruned", "prefix16", "between", "unsound16", "gap16")})
    # the level changes no older output
    for k in ("tiles", "pruned", "filtered", "half", "skipped", "fallback", "wrong"):
        assert r[k] == r0[k], k
    assert np.array_equal(r["tile_pruned"], r0["tile_pruned"]) and np.array_equal(r["verdict"], r0["verdict"]) and r["wrong"] == 0
    # no tile is pruned by the f16 test and kept by the f32 test
    assert r["unsound16"] == 0 and r["prefix16"] <= r["prefix_pruned"] <= r["reach"]
    assert (r["prefix16"] >= 1) == must_prune
    # every f16 prefix key lies further from thrQ than the float32 evaluation can move it (eQ < 2^-15 M; 2^-13 M here), so the kernel
    # decides every tile as this model does
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    Mx = np.nanmax((a64 * a64).sum(1)) + np.nanmin((b64 * b64).sum(1))
    assert r["gap16"] > 2.0 ** -13 * Mx, (r["gap16"], Mx)
    if name.startswith("margin_views between"):
        assert r["between"] == 1 and not r["tile_prefix16"][1, 0] and r["tile_pruned"][1, 0]
    if name == "margin_views cleared":
        assert r["between"] == 0 and r["tile_prefix16"][1, 0]
    if name == "margin_views below":
        assert not r["tile_pruned"][1, 0]
    if name in ("range_views over_range", "range_views nan_row", "range_views huge_row"):
        assert not r["tile_prefix16"][:, 1].any() and r["tile_prefix16"][1:, 0].all() and r["tile_prefix16"][1:, 2].all()
