"""The skip of level 2 in the numpy model of l2_knn2_half_kernel (tools/prefix_prune_model.py, model_pair_levels(skip=...)) on every view
pair of tests/pairnorm_filter_cases.py, tests/prefix_prune_cases.py, tests/half_filter_cases.py and tests/level2_skip_cases.py: the bound
kf - kh <= L holds on the stored tables, no tile exists where the skip fires and the pair-norm filter prunes, a key that is -inf or NaN
never fires it, and nothing else of the model moves.  It also shows that each case of tests/test_gpu_level2_skip.py holds what it is
built for."""
import numpy as np
import pytest

import half_filter_cases as HC
import level2_skip_cases as SC
import test_half_filter_model as HM

M = HM.M
GP = 12

VIEWS = HM.VIEWS + SC.all_cases(M)


@pytest.mark.parametrize("name,a,b,R", VIEWS, ids=[v[0] for v in VIEWS])
def test_the_skip_is_sound_and_changes_nothing_else(name, a, b, R):
    LB, _ = M.pairnorm_bound(a, b)
    LBH, _ = M.halfnorm_bound(a, b)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    Mn = ((a64 * a64).sum(1).max(initial=0.0) + (b64 * b64).sum(1))[None, :]
    num = np.isfinite(LBH) & np.isfinite(LB)
    for form in ("lane", "key"):
        L = np.broadcast_to(M.skip_loss(a, b, LBH, form), LBH.shape)
        # the rounding loss alone stays below L less the 387 u M + 2^-36 that L keeps for the evaluation errors of the two computed keys
        room = L - (387.0 * M.U * Mn + 2.0 ** -36)
        assert ((LB - LBH)[num] <= room[num]).all(), form
        r0 = M.model_pair_levels(a, b, GP, R)
        r = M.model_pair_levels(a, b, GP, R, skip=form)
        assert r["unsound"] == 0 and not (r["tile_skip"] & r["tile_filtered"]).any()
        assert r["skipped"] == int(r["tile_skip"].sum()) <= r["tiles"] - r["half"]
        for k in ("tiles", "pruned", "filtered", "half", "work", "fallback", "wrong", "matches"):
            assert r[k] == r0[k], (form, k)
        for k in ("tile_half", "tile_filtered", "tile_pruned", "verdict"):
            assert np.array_equal(r[k], r0[k]), (form, k)
        assert r["cycles"] == r0["cycles"] - 8 * M.CYC_GROUP * r["skipped"] and r0["skipped"] == 0
        assert not r["tile_skip"][0].any()                 # tile 0 runs under thresholds of +inf: it never skips


def test_keys_beyond_f16s_range_never_fire():
    """scaled_up: every key of level 1 is -inf or NaN, level 2 prunes every far tile and the skip fires nowhere; huge_row, nan: a tile
    skips only on the strength of a finite key"""
    a, b = HC.range_views("scaled_up")
    LBH, _ = M.halfnorm_bound(a, b)
    assert not np.isfinite(LBH).any()
    r = M.model_pair_levels(a, b, GP, 0.36, skip="lane")
    assert r["skipped"] == 0 and r["half"] == 0 and r["filtered"] == 3 * 3
    for kind in ("huge_row", "nan"):
        a, b = HC.range_views(kind)
        LBH, _ = M.halfnorm_bound(a, b)
        assert (~np.isfinite(LBH)).any()
        r = M.model_pair_levels(a, b, GP, 0.36, skip="lane")
        fin = np.where(np.isfinite(LBH), LBH, np.inf)      # the same views with the keys beyond the range taken out of the skip's sight
        assert r["unsound"] == 0
        for t, w in zip(*np.nonzero(r["tile_skip"])):
            assert np.isfinite(fin[32 * t:32 * t + 32, 64 * w:64 * w + 64]).any()


def test_the_gpu_cases_hold_what_they_are_built_for():
    R = 0.36
    # the planted row against the band: where its f16 key lies, and what becomes of its tile (tile 1, wave 0)
    for side, at, skipped, by_level_2 in (("inside", (-1.0, -0.9), 0, 0), ("below", (-1.55, -1.45), 1, 0), ("missed", (0.0, 0.02), 0, 1)):
        a, b, q, row = SC.band_views(M, side)
        LBH, margin = M.halfnorm_bound(a, b)
        _, slack = M.pairnorm_bound(a, b)
        L = float(np.broadcast_to(M.skip_loss(a, b, LBH, "lane"), LBH.shape)[row, q])
        r = M.model_pair_levels(a, b, GP, R, skip="lane")
        # T of the lane half after tile 0, read back from where the model puts thrH for the planted key
        half0 = [k for k in range(32) if ((k >> 2) & 1) == 0]
        d = np.sort(((a[half0].astype(np.float64) - b[q].astype(np.float64)) ** 2).sum(1))
        T = float(np.float32(R)) * d[1] * (1.0 + 2.0 ** -21)
        pos = (LBH[row, q] - slack[q] - T) / L
        print("band_views", side, "(kh - thrF) / L", pos, "L", L, "margin", margin[q], "gap", r["gap"])
        assert at[0] < pos < at[1] and 0 < margin[q] < 0.02 * L
        assert r["skipped"] == skipped and bool(r["tile_skip"][1, 0]) == bool(skipped)
        assert not r["tile_half"][1, 0] and r["filtered"] - r["half"] == by_level_2
        assert r["gap"] > 5.0 and r["wrong"] == 0
    # the block positions: every planted tile skips for wave 0 and for no other wave; every other tile behind tile 0 is pruned by level 1
    for name, make in SC.block_cases(M):
        a, b = make()
        r = M.model_pair_levels(a, b, GP, R, skip="lane")
        n_tiles, n_waves = r["tile_skip"].shape
        planted = sorted(set(int(t) for t in np.nonzero((a[:, SC.FC.TAIL::2] != 0).any(1) & (np.arange(len(a)) >= 32))[0] // 32))
        print(name, "planted tiles", planted, "gap", r["gap"])
        assert sorted(np.nonzero(r["tile_skip"][:, 0])[0].tolist()) == planted and not r["tile_skip"][:, 1:].any()
        assert r["skipped"] == len(planted) and r["half"] == r["filtered"] == (n_tiles - 1) * n_waves - len(planted)
        assert r["gap"] > 5.0 and r["wrong"] == 0
        assert M.model_pair_levels(a, b, GP, 0.49, skip="lane")["gap"] > 5.0
    # the match that lowers the thresholds: tile 2 skips and finishes, tile 3 -- which would have skipped under the thresholds of before --
    # is pruned by level 1 under those of the refresh
    a, b, q = SC.lowered_views(M)
    r = M.model_pair_levels(a, b, GP, R, skip="lane")
    assert r["tile_skip"][2, 0] and not r["tile_pruned"][2, 0] and r["tile_half"][3, 0] and r["skipped"] == 1 and r["gap"] > 5.0
    a2 = a.copy(); a2[64] = a[70]; a2[65] = a[71]          # without the match (far rows in its place) tile 3 skips
    r2 = M.model_pair_levels(a2, b, GP, R, skip="lane")
    assert r2["tile_skip"][3, 0] and r2["skipped"] == 1
