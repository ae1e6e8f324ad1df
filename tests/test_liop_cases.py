"""The inputs of tests/test_gpu_liop_edges.py (liop_cases.py) checked without a GPU:
  * the restatement (oracle/liop.c) equals the committed output of the reference's own vl_liop.c (tests/golden/liop_edge_ref.npz) on
    every patch family, and the live reference build where it exists;
  * the preconditions the families are trusted for hold, and the number of patches the device has to re-sort is what the GPU test
    compares n_resorted with;
  * the extraction families stay under their cap of constant patches, inside the fixed-point range, and never see the marker beyond
    column (row) 32,768."""
import numpy as np
import pytest

import liop_cases as L

GOLDEN, N_RESORTED, golden_desc = L.GOLDEN, L.N_RESORTED, L.golden_desc
FAMILIES = list(L.PATCH_FAMILIES)


def _rows(a, b):
    return np.flatnonzero((a.view(np.uint32) != b.view(np.uint32)).any(1))


def test_support_is_the_formula():
    """dx^2 + dy^2 <= (long)(14.6^2) = 213 around (20, 20), the patch's corner pixel (0, 0) skipped as the reference skips it: 673
    pixels in scan order, 112 ranks per ordinal bin"""
    pix, sx, sy = L.geometry()
    y, x = np.mgrid[0:41, 0:41]
    inside = ((x - 20) ** 2 + (y - 20) ** 2 <= int(14.6 * 14.6))
    assert np.array_equal(pix, np.flatnonzero(inside.ravel()))
    assert L.n_support() == 673 and L.bin_area() == 112 and L.bin_edges() == [111, 223, 335, 447, 559]
    assert sx.shape == (673, 4) and sy.shape == (673, 4)
    assert all(e % 16 == 15 for e in L.bin_edges())            # a bin edge is an edge between two lanes of the 16-keys-per-lane sort


@pytest.mark.parametrize("name", FAMILIES)
def test_restatement_equals_the_reference(oracle, name):
    z = np.load(GOLDEN)
    P = L.patches_of(name)
    assert L.crc(P) == int(z[name + "_crc"]), f"{name}: the regenerated patches are not the ones the golden was made from"
    assert np.isfinite(P).all()
    want = golden_desc(z, name)
    got = oracle.liop_describe(P)
    bad = _rows(got, want)
    assert bad.size == 0, f"{name}: restatement differs from the reference-built golden in {bad.size} patches, first {bad[:5]}"
    dv, norm = L.normalise(oracle.liop_votes(P))
    assert _rows(dv, want).size == 0 and np.array_equal(norm, z[name + "_norm"]), name
    if oracle.ref_liop_lib() is not None:
        bad = _rows(oracle.ref_liop(P), want)
        assert bad.size == 0, f"{name}: the live reference build differs from the golden in {bad.size} patches, first {bad[:5]}"


@pytest.mark.parametrize("name", FAMILIES)
def test_resorted_count_and_range(name):
    P = L.patches_of(name)
    assert L.n_resorted(P) == N_RESORTED[name]
    v = L.support_values(P)
    with np.errstate(over="ignore"):
        rng = v.max(1) - v.min(1)
    if name == "range_inf":
        assert len(P) <= 16 and np.isposinf(rng).all()
        z = np.load(GOLDEN)
        assert not z[name + "_hist"].any() and (z[name + "_norm"] == np.float32(1e-12)).all()
    elif name == "flat_support":
        z = np.load(GOLDEN)
        assert (rng == 0).all() and not L.patch_constant(P).any()
        assert z[name + "_hist"].any(1).all()                   # one intensity in the support, and a descriptor that is not zero
    else:
        assert np.isfinite(rng).all() and (rng > 0).all()       # no constant support in any other patch family


def test_pair_ties_preconditions():
    P, ranks = L.pair_ties()
    N = L.n_support()
    assert ranks[:N - 1].tolist() == list(range(N - 1))
    v = np.sort(L.support_values(P), 1)
    for p, r in zip(v, ranks):                                  # exactly one tie, at sorted ranks (r, r + 1)
        assert np.array_equal(np.flatnonzero(np.diff(p) == 0), [r])
    sens = L.order_sensitive(P)
    # a single tied pair changes the descriptor only across a bin edge ...
    assert set(ranks[sens].tolist()) <= set(L.bin_edges())
    # ... and every edge has extras that tell the scan-position order from the reference's
    for e in L.bin_edges():
        extra = ranks[N - 1:] == e
        assert extra.sum() >= 8 and sens[N - 1:][extra].sum() >= 1, e


@pytest.mark.parametrize("hot", (True, False))
def test_one_pixel_families(hot):
    P = L.one_hot() if hot else L.one_cold()
    v = L.support_values(P)
    assert len(P) == L.n_support()
    other = v.argmax(1) if hot else v.argmin(1)
    assert np.array_equal(other, np.arange(L.n_support()))     # one patch per support pixel
    assert (np.sort(v, 1)[:, 1:-1] == np.float32(0.5)).all()


def test_value_families():
    assert len(L.two_level()) == 34 and all(np.unique(p).size == 2 for p in L.two_level())
    neg = L.negative()
    assert (neg < 0).any(axis=(1, 2)).all() and (neg > 0).any(axis=(1, 2)).all()
    q = neg[16:]
    assert (q == np.rint(q / 500) * 500).all() and (np.signbit(q) & (q == 0)).any()      # quantised, with a -0.0 among the zeros
    sz = L.signed_zero()
    for p in sz:
        zero = p[p == 0]
        assert np.signbit(zero).any() and (~np.signbit(zero)).any() and (p != 0).sum() == 6
    dn = L.denormal().view(np.uint32)
    assert dn.max() == 49 and dn.min() == 0
    ir = L.support_values(L.int_range51())
    assert (ir.min(1) == 0).all() and (ir.max(1) == 51).all() and (ir == np.rint(ir)).all()
    assert np.float32(5.0 / 255) * np.float32(51) == np.float32(1.0)                       # thr lands on an integer step
    u8 = L.u8_blur()
    assert (u8 == np.rint(u8)).all() and u8.min() == 0 and u8.max() == 255
    assert (L.neighbour_tie_share(L.neighbour_ties()) > 0).all()
    assert (L.neighbour_tie_share(L.smooth()) == 0).all()                                  # the control takes the lookup table only


@pytest.mark.parametrize("name,img,kps", L.extraction_families(), ids=[f[0] for f in L.extraction_families()])
def test_extraction_family(oracle, name, img, kps):
    h, w = img.shape
    assert len(kps) <= 256 and np.isfinite(kps).all()
    assert L.fixed_point_bound(kps) < 2.0 ** 31
    assert set(np.unique(kps[:, 2]).tolist()) <= set(L.SIZES.tolist()) and set(np.unique(kps[:, 3]).tolist()) <= set(L.ANGLES.tolist())
    P = oracle.liop_extract_patches(img, kps, 8.0)
    const = L.is_constant(P)
    assert const.sum() * 2 <= len(kps), f"{name}: {const.sum()} of {len(kps)} patches are constant"
    if max(h, w) > L.SHORT_MAX:
        assert L.beyond_short_range(h, w) >= 10                # identity-scale keypoints centred ON marker columns (rows) ...
        assert P.max() <= 1.0 + 1e-5                           # ... and the marker (1e6) is never read: the coordinates saturate
        assert (img == L.MARKER).sum() == (max(h, w) - (L.SHORT_MAX + 2)) * 6
    else:
        # the pure translation: the image's own pixels, blurred
        assert np.array_equal(kps[-1], np.array([20, 20, 41 / 8, -90], np.float32))


def test_grid_stride_arrangement(oracle):
    idx = L.stride_index()
    assert len(idx) == L.GRID_CAP + L.GRID_EXTRA and idx.min() == 0 and idx.max() == L.KINDS * L.PER_KIND - 1
    kind = idx // L.PER_KIND
    pairs = set(zip(kind[:L.GRID_EXTRA].tolist(), kind[L.GRID_CAP:].tolist()))
    assert len(pairs) == L.KINDS ** 2                           # a group's first and second item: all 16 ordered pairs of kinds
    assert np.unique(idx).size == L.KINDS * L.PER_KIND
    # the unique patches are what their kinds say
    P = L.stride_patches()
    const = L.is_constant(P).reshape(L.KINDS, L.PER_KIND); tie = (L.has_tie(P) & ~L.is_constant(P)).reshape(L.KINDS, L.PER_KIND)
    assert const[0].all() and L.patch_constant(P[:L.PER_KIND]).all() and not const[1:].any()
    assert tie[1].all() and tie[2].all() and not tie[3].any()
    assert np.unique(P.reshape(len(P), -1), axis=0).shape[0] == len(P)
    # ... and the unique keypoints' patches: constant | leaving the image | inside with ties | inside
    img, kps = L.stride_keypoints()
    assert L.fixed_point_bound(kps) < 2.0 ** 31
    Q = oracle.liop_extract_patches(img, kps, 8.0)
    const = L.is_constant(Q).reshape(L.KINDS, L.PER_KIND)
    assert const[0].all() and not const[1:].any()
    assert L.has_tie(Q).reshape(L.KINDS, L.PER_KIND)[2].all()
