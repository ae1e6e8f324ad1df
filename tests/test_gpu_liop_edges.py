"""LIOP on the device (kernels_liop.hip) where the kernels can go wrong, bit for bit: ties at every rank of the support, the exact
sort's worst case, negative / signed-zero / denormal / threshold-edge intensities against the output of the reference's own vl_liop.c
(tests/golden/liop_edge_ref.npz); the warp's border logic on images smaller than a patch and wider than 32,768 columns against the
restatement; and the grid-stride loops of the three launches, where one workgroup describes a second patch.  The inputs and their
preconditions are liop_cases.py's (checked without a GPU by test_liop_cases.py)."""
import numpy as np
import pytest

import liop_cases as L

pytestmark = pytest.mark.gpu
FAMILIES = list(L.PATCH_FAMILIES)
GOLDEN, N_RESORTED, golden_desc = L.GOLDEN, L.N_RESORTED, L.golden_desc


def _assert_rows(got, want, what):
    got = np.ascontiguousarray(got); want = np.ascontiguousarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if np.array_equal(got.view(np.uint32), want.view(np.uint32)):
        return
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).reshape(len(got), -1).any(1))
    assert bad.size == 0, f"{what}: {bad.size} of {len(got)} rows differ, first {bad[:8].tolist()}"


def _describe(oracle, patches):
    return oracle.ref_liop(patches) if oracle.ref_liop_lib() is not None else oracle.liop_describe(patches)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


# ---------------------------------------------------------------------------------------------------- 1. patch families
@pytest.mark.parametrize("name", FAMILIES)
def test_patch_family(ctx, golden, name):
    """descriptors equal the reference's, and exactly the patches with a tie in their support took the exact re-sort -- for pair_ties
    that is the tie detection at every one of the 672 rank positions, the 41 that straddle two lanes of the sort included"""
    P = L.patches_of(name)
    d, n_resorted = ctx.liop_describe_patches(P)
    assert not np.isnan(d).any(), name
    _assert_rows(d, golden_desc(golden, name), name)
    assert n_resorted == N_RESORTED[name], (name, n_resorted, N_RESORTED[name])


def test_pair_ties_one_at_a_time(ctx):
    """n_resorted of the whole family cannot say WHICH tie was missed: one call per rank"""
    P, ranks = L.pair_ties()
    missed = [int(ranks[i]) for i in range(L.n_support() - 1) if ctx.liop_describe_patches(P[i:i + 1])[1] != 1]
    assert not missed, f"ties at ranks {missed} were not detected"


# ---------------------------------------------------------------------------------------------------- 2. extraction families
@pytest.mark.parametrize("name,img,kps", L.extraction_families(), ids=[f[0] for f in L.extraction_families()])
def test_extraction_family(ctx, oracle, name, img, kps):
    """patches equal the restatement's, descriptors are those patches' -- through the patches-out pair of kernels and fused"""
    want_p = oracle.liop_extract_patches(img, kps, 8.0)
    want_d = _describe(oracle, want_p)
    d, p = ctx.extract_liop(img, kps, 8.0, want_patches=True)
    _assert_rows(p, want_p, f"{name}: patches")
    _assert_rows(d, want_d, f"{name}: descriptors of the patches")
    _assert_rows(ctx.extract_liop(img, kps, 8.0), want_d, f"{name}: fused descriptors")


# ---------------------------------------------------------------------------------------------------- 3. grid stride
def test_grid_stride_patches(ctx, oracle):
    """65,536 + 4,096 patches from 64: the groups 0 .. 4,095 of liop_kernel<false> describe a second patch, every kind after every kind"""
    import torch
    uniq = L.stride_patches()
    idx = L.stride_index()
    want = _describe(oracle, uniq)
    resorted = (L.has_tie(uniq) & ~L.patch_constant(uniq))
    big = torch.from_numpy(np.array(uniq)).cuda()[torch.from_numpy(idx).cuda()].contiguous()
    torch.cuda.synchronize()
    d, n_resorted = ctx.liop_describe_patches(big)
    del big
    bad = np.flatnonzero((d.view(np.uint32) != want.view(np.uint32)[idx]).any(1))
    assert bad.size == 0, f"{bad.size} of {len(idx)} patches differ, first {bad[:8].tolist()} (kinds {[L.STRIDE_PATCH_KINDS[k] for k in (idx[bad[:8]] // L.PER_KIND)]})"
    assert n_resorted == int(resorted[idx].sum())


@pytest.mark.parametrize("want_patches", (True, False), ids=("patches_out", "fused"))
def test_grid_stride_keypoints(ctx, oracle, want_patches):
    """69,632 keypoints from 64 on one 128 x 128 image: the stride loop of liop_extract_patches_kernel (four waves a group, 16,384
    groups) + liop_kernel<false>, and of the fused liop_kernel<true>"""
    img, uniq = L.stride_keypoints()
    idx = L.stride_index()
    want_p = oracle.liop_extract_patches(img, uniq, 8.0)
    want_d = _describe(oracle, want_p)
    kps = np.ascontiguousarray(uniq[idx])
    if want_patches:
        d, p = ctx.extract_liop(img, kps, 8.0, want_patches=True)
        for s in range(0, len(idx), 8192):                      # (in slices: the expected patches are never held as one 470 MB array)
            e = min(s + 8192, len(idx))
            if not np.array_equal(p[s:e].view(np.uint32), want_p.view(np.uint32)[idx[s:e]]):
                bad = s + np.flatnonzero((p[s:e].view(np.uint32) != want_p.view(np.uint32)[idx[s:e]]).reshape(e - s, -1).any(1))
                raise AssertionError(f"patches differ, first {bad[:8].tolist()} (kinds {[L.STRIDE_KEYPOINT_KINDS[k] for k in (idx[bad[:8]] // L.PER_KIND)]})")
    else:
        d = ctx.extract_liop(img, kps, 8.0)
    bad = np.flatnonzero((d.view(np.uint32) != want_d.view(np.uint32)[idx]).any(1))
    assert bad.size == 0, f"{bad.size} of {len(idx)} descriptors differ, first {bad[:8].tolist()} (kinds {[L.STRIDE_KEYPOINT_KINDS[k] for k in (idx[bad[:8]] // L.PER_KIND)]})"
