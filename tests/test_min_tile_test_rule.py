"""The rule that admits a batch to the min form of l2_knn2_half_kernel's tile tests (every view's max |row|^2 below 2^28), in numpy
with the model's own f16 rounding (tools/prefix_prune_model.py): at the derivation's worst cases every f16 pair norm stays below
32,752, every -2 h is finite in f16 and every level-1 key is finite or +inf; and on every tile of the case tables the verdicts of the
general form, any(!(k > thrH)) and any(k <= thrS and k > -inf), are those of the min form, !(min k > thrH) and min k <= thrS, at every
threshold that could tell them apart -- where the rule holds.  Where it does not (NaN data, f16 overflow) the forms can differ
(`huge_row` shows it), which is why such batches keep the general form."""
import numpy as np
import pytest

import level2_skip_cases as SC
import min_tile_test_cases as MC
import test_half_filter_model as HM

M = HM.M
INF = np.inf


def _level1_keys(a, b, pad_to=None):
    """the model's level-1 keys kh = |a|^2 - 2 sum_k ha_k hb_k, [rows, nJ] in float64 from float32 norms and f16 pair norms; rows
    beyond a.shape[0] up to pad_to are padding rows: norm +inf, pair norms 0"""
    na = MC.stored_norms(a).astype(np.float64)
    ha, hb = M.pair_norms_half(a), M.pair_norms_half(b)
    if pad_to is not None and pad_to > a.shape[0]:
        na = np.concatenate([na, np.full(pad_to - a.shape[0], INF)])
        ha = np.concatenate([ha, np.zeros((pad_to - a.shape[0], ha.shape[1]))])
    with np.errstate(invalid="ignore", over="ignore"):
        m2hb = (-2.0 * hb).astype(np.float16).astype(np.float64)          # the query fragments: -2 h rounded to f16 (exact, or -inf)
        return na[:, None] + (ha[:, None, :] * m2hb[None, :, :]).sum(2)


def _worst_cases():
    big = np.nextafter(np.float32(2.0 ** 14), np.float32(0))
    one = np.zeros((3, 128), np.float32)
    one[0, 0], one[0, 1] = big, 4.0                       # |row|^2 = 2^28 - 16, all of it in one pair
    one[1, 126] = big                                     # ... in the last pair, one member
    one[2, 0] = one[2, 1] = np.float32(11585.0)           # ... in one pair, both members: 2 x 11585^2 = 2^28 - 1,006
    even = np.empty((2, 128), np.float32)
    even[0] = 1448.0                                      # 128 x 1448^2 = 2^28 - 57,344: spread evenly
    even[1] = 1448.14                                     # ... and 5,400 below the bound, no integers
    return {"one pair": one, "spread evenly": even}


@pytest.mark.parametrize("name", ["one pair", "spread evenly"])
@pytest.mark.parametrize("nI", [3, 33])
def test_worst_cases_keep_every_key_finite_or_plus_inf(name, nI):
    rows = _worst_cases()[name]
    a = np.concatenate([rows, np.zeros((nI - len(rows), 128), np.float32)]) if nI > len(rows) else rows
    norms = MC.stored_norms(a)
    print(name, "max |row|^2", float(norms.max()), "of", float(MC.NORM_BOUND))
    assert MC.rule_holds(a) and float(norms.max()) > 0.99 * 2.0 ** 28
    h = M.pair_norms_half(a)
    print("largest f16 pair norm", h.max())
    assert (h < 32752.0).all()
    with np.errstate(over="ignore"):
        assert np.isfinite((-2.0 * h).astype(np.float16)).all()
    # against itself, against the other worst case, and with padding rows up to the tile
    for b in _worst_cases().values():
        k = _level1_keys(a, b, pad_to=(a.shape[0] + 31) // 32 * 32)
        assert not np.isnan(k).any() and (k > -INF).all()
        assert np.isposinf(k[a.shape[0]:]).all() and np.isfinite(k[: a.shape[0]]).all()


def _forms(K, T):
    """K [16, nJ]: the keys of one lane half per query; T [n, nJ]: thresholds per query -> [n, nJ] bool arrays: (general objection, min
    objection, general skip, min skip)"""
    with np.errstate(invalid="ignore"):
        m = np.fmin.reduce(K, 0)                          # v_min3_f32: the operand that is no NaN
        return ((~(K[:, None, :] > T[None, :, :])).any(0), ~(m[None, :] > T),
                ((K[:, None, :] <= T[None, :, :]) & (K[:, None, :] > -INF)).any(0), m[None, :] <= T)


def _lanes(a, b):
    """the key sets [16, nJ] of every (tile, lane half) of the pair: padding rows included"""
    nt = (a.shape[0] + 31) // 32
    k = _level1_keys(a, b, pad_to=32 * nt)
    half = (np.arange(32) >> 2) & 1
    for t in range(nt):
        for h in (0, 1):
            yield k[32 * t + np.flatnonzero(half == h)]


ALL = HM.VIEWS + SC.all_cases(M)


@pytest.mark.parametrize("name,a,b,R", ALL, ids=[v[0] for v in ALL])
def test_min_form_gives_the_general_forms_verdicts(name, a, b, R):
    """at the thresholds that could tell the forms apart: each key itself, the floats next to it, +-inf and NaN"""
    ok = MC.rule_holds(a, b)
    print(name, "rule holds:", ok)
    assert ok == (name not in ("range_views scaled_up", "range_views huge_row", "range_views nan", "other_rows nan"))
    differ = 0
    for K in _lanes(a, b):
        if ok:
            assert not np.isnan(K).any() and (K > -INF).all()
        with np.errstate(invalid="ignore"):
            fin = np.where(np.isfinite(K), K, 0.0)
            T = np.concatenate([fin, np.nextafter(fin, INF), np.nextafter(fin, -INF),
                                np.full((1, K.shape[1]), INF), np.full((1, K.shape[1]), -INF), np.full((1, K.shape[1]), np.nan)])
        gH, mH, gS, mS = _forms(K, T)
        if ok:
            assert np.array_equal(gH, mH) and np.array_equal(gS, mS)
        else:
            differ += int((gH != mH).sum() + (gS != mS).sum())
    if not ok:
        # (a NaN QUERY makes every key of its lanes a NaN, which both forms treat alike; one row beyond f16's range among rows within it
        #  gives a lane -inf or NaN keys beside finite ones, and there the forms part)
        print("lanes x thresholds on which the forms differ:", differ)
        assert differ > 0 or name != "range_views huge_row"
