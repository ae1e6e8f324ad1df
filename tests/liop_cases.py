"""LIOP (kernels_liop.hip) where the kernels can go wrong: the deterministic inputs of tests/test_gpu_liop_edges.py, their
preconditions, and the numpy side of the checks (support values, the scan-position order of equal intensities, neighbour samples,
the normalisation).  No GPU and no torch in here.

Not a test module (no test_ prefix): imported by test_liop_cases.py (CPU), test_gpu_liop_edges.py and tools/make_golden_liop_edges.py.
Every family is made once per process and read-only.  The patches are regenerated from seeds with integer and exactly rounded
float64 arithmetic only (no libm, no BLAS: the same bits on every machine); tests/golden/liop_edge_ref.npz holds what the
reference's own vl_liop.c makes of them, and a CRC of every family's patches so that a drifted generator is named as such.

The support (its pixel list and its size N = 673 for the 41 x 41 patch) comes from the oracle's orc_liop_geometry, which restates
vl_liopdesc_new; the ordinal bins hold N // 6 = 112 ranks, so their edges are the ranks 112 k - 1 | 112 k -- also edges between
lanes of the kernel's register sort (16 keys per lane).

What each family is for.  "Mutant" = a one-character change to a scratch copy of oracle/liop.c (run once on the CPU, not committed);
the figures are the patches of the family whose descriptor the mutant changes / the patches of the family.  A family with no
mutant is there for a branch that only the device has.

  family           n    `>=` in the   `< 0` in the   scan order   -0.0 ordered   denormal inputs   device-only branch
                        weight test   quick sort     for ties     below +0.0     flushed to 0
  pair_ties       712        0             43            23            0              0           tie detection at every rank, lane edges
  one_hot         673        0            673           672            0              0           the wave-parallel quick sort, N depths
  one_cold        673        0            673           672            0              0           the same, the odd pixel sorted first
  two_level        34        0             33            33            0              0
  negative         32        0             16            16           16              0           the ~u branch of float_order_bits
  signed_zero      16        0             16            16           16              0
  denormal         16       16             16            16            0             16
  int_range51      16       16             16            16            0              0
  u8_blur          16        1             16            16            0              0
  smooth           16        0              0             0            0              0           control: the six-comparison table alone
  smooth_q64       16        0             16            16            0              0
  neighbour_ties   16        0             16            16            0              0           liop_ref_qsort4 instead of the table
  range_inf         8        0              0             0            0              0           thr = +inf: all zero, no NaN
  flat_support     16       16             16            16            0              0           the constant-patch short cut (see below)

  (the -0.0 column orders -0.0f below +0.0f by handing the restatement -denormal_min in its place; the `< 0` mutant also reaches the
  4-element sort of the neighbour samples, which share the routine.)

  flat_support is the family this work added after the device failed: the kernel sent a patch to the all-zero descriptor when its
  support held one intensity, but the reference still counts votes there (thr = 0, samples reach past the support).  Every
  extraction family holds such patches (keypoints near a corner of the image).

  extraction families (image shape x keypoints): the four-corner `inside` test and the clamp-free warp, the guarded taps of images
  smaller than a patch or narrower than a tap pair, the short-range saturation of coordinates beyond 32,767
  grid stride (69,632 items from 64): what a workgroup does BETWEEN two patches -- hist re-zeroed, the `continue` of a constant
  patch, the exact sort's arrays over perm, qcnt, the wave sync before the next patch's tables
"""
import functools
import os
import zlib

import numpy as np

SIDE = 41
SIZES = np.array([1e-3, 0.5, 41 / 8, 82 / 8, 40, 2000], np.float32)
ANGLES = np.array([0, 90, 180, 270, -90, 359.999, 720.5, -1e-3, 33.3], np.float32)
IMAGE_SHAPES = ((1, 1), (1, 50), (50, 1), (2, 2), (40, 40), (41, 41), (42, 42), (43, 43), (6, 32800), (32800, 6))       # (h, w)
# the smallest exponent of _border_coord at which at most 45 % of an image's patches are constant in the restatement
INWARD_BIAS = {s: 2 if s[0] * s[1] <= 50 else 1 for s in IMAGE_SHAPES}
MARKER = np.float32(1e6)          # the value of every column (row) from 32,769 on in the two long images
SHORT_MAX = 32767                 # saturate_cast<short>: the last column the warp can name; its right-hand tap is column 32,768
GRID_CAP = 65536                  # launch_liop* : one-wave groups; launch_liop_extract: 16,384 groups of four waves
GRID_EXTRA = 4096
KINDS = 4
PER_KIND = 16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "liop_edge_ref.npz")
# per patch family: the patches that are not constant and hold at least one tie in the support (np.unique of the support values + 0.0,
# asserted by test_liop_cases.py) -- what the device reports as n_resorted
N_RESORTED = dict(pair_ties=712, one_hot=673, one_cold=673, two_level=34, negative=16, signed_zero=16, denormal=16, int_range51=16,
                  u8_blur=16, smooth=0, smooth_q64=16, neighbour_ties=16, range_inf=0, flat_support=16)


def _oracle():
    from oracle import pyoracle
    pyoracle.build()
    return pyoracle


def _frozen(*arrays):
    for x in arrays:
        x.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ------------------------------------------------------------------------------------------------ the support and the numpy side
@functools.lru_cache(maxsize=None)
def geometry():
    """(pix [N]: offsets x + y * 41 of the support in scan order, sx [N, 4], sy [N, 4]: neighbour sample positions) -- the oracle's
    restatement of vl_liopdesc_new, which api_liop.cpp's liop_prepare repeats"""
    return _frozen(*_oracle().liop_geometry(SIDE))


def n_support():
    return int(geometry()[0].shape[0])


def bin_area():
    return n_support() // 6


def support_values(P):
    """[n, N] the support intensities in scan order, -0.0f as +0.0f (one intensity to the reference's `a - b <= 0`)"""
    P = np.asarray(P, np.float32)
    return P.reshape(P.shape[0], -1)[:, geometry()[0]] + np.float32(0.0)


def is_constant(P):
    """[n] bool: the support holds one intensity"""
    v = support_values(P)
    return v.min(1) == v.max(1)


def patch_constant(P):
    """[n] bool: one value in all 41 x 41 pixels -- the kernel's short cut to the all-zero descriptor.  (A constant SUPPORT does not make
    the descriptor zero: thr = 0 then, and the samples of the outer support pixels reach past the support.)"""
    P = np.asarray(P, np.float32).reshape(len(P), -1)
    return P.min(1) == P.max(1)


def has_tie(P):
    v = support_values(P)
    return np.array([np.unique(r).size < r.size for r in v])


def n_resorted(P):
    """how many patches are not constant over all their pixels and have at least one tie in the support: the device's n_resorted"""
    return int((has_tie(P) & ~patch_constant(P)).sum())


def scan_order(P):
    """[n, N] int32: the support ranked by (intensity, scan position) -- the order the kernel's bitonic sort leaves, and the order a
    missed tie would keep"""
    v = support_values(P)
    pos = np.arange(v.shape[1])
    return np.stack([np.lexsort((pos, r)) for r in v]).astype(np.int32)


def neighbour_samples(P):
    """[n, N, 4] float32: the four bilinear samples of every support pixel exactly as vl_liopdesc_process takes them (double
    arithmetic, taps outside the patch read as 0, the result stored to a float)"""
    _, sx, sy = geometry()
    P = np.asarray(P, np.float32)
    ring = np.zeros((P.shape[0], SIDE + 2, SIDE + 2), np.float64)
    ring[:, 1:-1, 1:-1] = P
    ix = np.floor(sx).astype(np.int64); iy = np.floor(sy).astype(np.int64)
    assert ix.min() >= -1 and iy.min() >= -1 and ix.max() <= SIDE - 1 and iy.max() <= SIDE - 1
    wx = sx - ix; wy = sy - iy
    a = ring[:, iy + 1, ix + 1]; b = ring[:, iy + 1, ix + 2]; c = ring[:, iy + 2, ix + 1]; d = ring[:, iy + 2, ix + 2]
    return ((1.0 - wy) * (a + (b - a) * wx) + wy * (c + (d - c) * wx)).astype(np.float32)


def neighbour_tie_share(P):
    """[n] the share of support pixels with two or more equal neighbour samples (they take the 4-element quick sort)"""
    nv = neighbour_samples(P)
    tie = np.zeros(nv.shape[:2], bool)
    for i in range(4):
        for j in range(i + 1, 4):
            tie |= nv[..., i] == nv[..., j]
    return tie.mean(1)


def normalise(votes):
    """votes [n, 144] (integers) -> (desc float32, norm float32): vl_liop.c's float running sum in index order, VL_MAX(sqrt, 1e-12)
    stored to a float, one float division per bin"""
    v = np.asarray(votes).astype(np.float32)
    s = np.zeros(v.shape[0], np.float32)
    for i in range(v.shape[1]):
        s = (s + v[:, i] * v[:, i]).astype(np.float32)
    norm = np.maximum(np.sqrt(s.astype(np.float64)), 1e-12).astype(np.float32)
    return (v / norm[:, None]).astype(np.float32), norm


def desc_from(hist, norm):
    return (np.asarray(hist).astype(np.float32) / np.asarray(norm, np.float32)[:, None]).astype(np.float32)


def golden_desc(z, name):
    """the descriptors of a family from the loaded fixture: u16 votes / f32 norm, one IEEE division per bin"""
    return desc_from(z[name + "_hist"], z[name + "_norm"])


def crc(P):
    return zlib.crc32(np.ascontiguousarray(P, np.float32).tobytes())


# ------------------------------------------------------------------------------------------------ patch families
def _blur(a, passes):
    """`passes` rounds of the binomial taps (1 4 6 4 1) / 16 along both axes, reflected borders, float64, fixed operation order"""
    a = np.asarray(a, np.float64)
    for _ in range(passes):
        for axis in (a.ndim - 1, a.ndim - 2):
            pad = [(0, 0)] * a.ndim; pad[axis] = (2, 2)
            p = np.pad(a, pad, mode="reflect")
            sl = [np.take(p, np.arange(k, k + a.shape[axis]), axis=axis) for k in range(5)]
            a = (((sl[0] + sl[4]) + 4.0 * (sl[1] + sl[3])) + 6.0 * sl[2]) / 16.0
    return a


def _distinct(rng, n):
    """n strictly increasing float32 in (0, 1]: multiples of 2^-20, exact"""
    return (np.cumsum(rng.integers(1, 1000, n)).astype(np.float64) / 2.0 ** 20).astype(np.float32)


def _pair_tie_patch(rng, r):
    N = n_support()
    v = _distinct(rng, N - 1)
    s = np.insert(v, r + 1, v[r])                               # sorted ranks r and r + 1 hold one value, every other value once
    p = (rng.integers(0, 1 << 20, SIDE * SIDE).astype(np.float64) / 2.0 ** 20).astype(np.float32)
    p[geometry()[0][rng.permutation(N)]] = s
    return p.reshape(SIDE, SIDE)


def bin_edges():
    """the ranks r = 112 k - 1, k = 1..5: a tie at (r, r + 1) straddles two ordinal bins"""
    return [bin_area() * k - 1 for k in range(1, 6)]


EXTRA_PER_EDGE = 8


@functools.lru_cache(maxsize=None)
def pair_ties():
    """(patches, r): one patch for every rank r = 0 .. N - 2 whose only tie is the pair at sorted ranks (r, r + 1), then EXTRA_PER_EDGE
    more for each bin edge"""
    N = n_support()
    ranks = list(range(N - 1)) + [r for r in bin_edges() for _ in range(EXTRA_PER_EDGE)]
    P = np.stack([_pair_tie_patch(np.random.default_rng([1, r, j]), r) for j, r in enumerate(ranks)])
    return _frozen(P, np.array(ranks))


def order_sensitive(P):
    """[n] bool: the descriptor under scan-position order of equal intensities differs from the descriptor under the reference's order"""
    O = _oracle()
    return (O.liop_votes(P, scan_order(P)) != O.liop_votes(P)).any(1)


def _one_pixel(base, other):
    pix = geometry()[0]
    P = np.full((len(pix), SIDE * SIDE), base, np.float32)
    P[np.arange(len(pix)), pix] = other
    return P.reshape(-1, SIDE, SIDE)


@functools.lru_cache(maxsize=None)
def one_hot():
    """0.5 everywhere, one support pixel at 1: the exact sort's worst case (N recursion depths of one long segment each).  Not thinned:
    the 673 patches sort side by side, a wavefront each"""
    return _frozen(_one_pixel(0.5, 1.0))


@functools.lru_cache(maxsize=None)
def one_cold():
    return _frozen(_one_pixel(0.5, 0.0))


@functools.lru_cache(maxsize=None)
def two_level():
    """32 step edges (integer normals round the square |a|, |b| <= 4, five offsets), a checkerboard and a single row"""
    y, x = np.mgrid[0:SIDE, 0:SIDE] - SIDE // 2
    ring = [(4, t) for t in range(-4, 4)] + [(-t, 4) for t in range(-4, 4)] + [(-4, -t) for t in range(-4, 4)] + [(t, -4) for t in range(-4, 4)]
    P = [(a * x + b * y > 3 * (k % 5 - 2)) for k, (a, b) in enumerate(ring)]
    P.append(((x + y) & 1) == 1)
    P.append(y == 0)
    return _frozen(np.stack(P).astype(np.float32))


@functools.lru_cache(maxsize=None)
def negative():
    """16 patches of standard_normal * 1e3 and the same rounded to multiples of 500 (ties on both sides of 0, -0.0 among them)"""
    g = (np.random.default_rng([2]).standard_normal((16, SIDE, SIDE)) * 1e3).astype(np.float32)
    q = (np.rint(g.astype(np.float64) / 500.0) * 500.0).astype(np.float32)
    return _frozen(np.concatenate([g, q]))


@functools.lru_cache(maxsize=None)
def signed_zero():
    """+0.0f and -0.0f at random, six support pixels at +-1 .. +-3"""
    rng = np.random.default_rng([3])
    P = np.where(rng.integers(0, 2, (16, SIDE * SIDE)) == 1, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    pix = geometry()[0]
    for p in P:
        at = pix[rng.permutation(len(pix))[:6]]
        p[at] = (rng.integers(1, 4, 6) * (2 * rng.integers(0, 2, 6) - 1)).astype(np.float32)
    return _frozen(P.reshape(-1, SIDE, SIDE))


@functools.lru_cache(maxsize=None)
def denormal():
    """0 .. 49 times the smallest f32 denormal"""
    k = np.random.default_rng([4]).integers(0, 50, (16, SIDE, SIDE)).astype(np.uint32)
    return _frozen(k.view(np.float32))


@functools.lru_cache(maxsize=None)
def int_range51():
    """integers 0 .. 51, both extremes inside the support: thr = (float)(5 / 255) * 51 = 1.0f, and the on-axis samples are integers"""
    rng = np.random.default_rng([5])
    P = rng.integers(0, 52, (16, SIDE * SIDE)).astype(np.float32)
    pix = geometry()[0]
    for p in P:
        lo, hi = pix[rng.permutation(len(pix))[:2]]
        p[lo] = 0.0; p[hi] = 51.0
    return _frozen(P.reshape(-1, SIDE, SIDE))


@functools.lru_cache(maxsize=None)
def u8_blur():
    """a blurred 0 .. 255 image stretched to the full range and rounded: what a photograph's pixels look like"""
    b = _blur(np.random.default_rng([6]).integers(0, 256, (16, SIDE, SIDE)), 2)
    lo = b.min(axis=(1, 2), keepdims=True); hi = b.max(axis=(1, 2), keepdims=True)
    return _frozen(np.rint((b - lo) / (hi - lo) * 255.0).astype(np.float32))


@functools.lru_cache(maxsize=None)
def smooth():
    rng = np.random.default_rng([7])
    return _frozen(np.stack([_blur(rng.random((SIDE, SIDE)), passes) for passes in (1, 2, 4, 6) for _ in range(4)]).astype(np.float32))


@functools.lru_cache(maxsize=None)
def smooth_q64():
    return _frozen((np.rint(smooth().astype(np.float64) * 64.0) / 64.0).astype(np.float32))


@functools.lru_cache(maxsize=None)
def neighbour_ties():
    """plateaus: blocks of 7, 10, 14 and 21 pixels at six levels, so that two or more of the four neighbour samples (8.5 pixels
    apart) are equal"""
    rng = np.random.default_rng([8])
    y, x = np.mgrid[0:SIDE, 0:SIDE]
    P = []
    for b in (7, 10, 14, 21):
        for _ in range(4):
            m = -(-SIDE // b)
            lv = rng.integers(0, 6, (m, m))
            lv[0, 0] = 0; lv[m - 1, m - 1] = 5                                   # never one level alone
            P.append(lv[y // b, x // b])
    return _frozen(np.stack(P).astype(np.float32))


@functools.lru_cache(maxsize=None)
def range_inf():
    """finite pixels whose max - min overflows to +inf (the one family where it does): thr = +inf, every weight 0, the descriptor all
    zero -- and no NaN"""
    rng = np.random.default_rng([9])
    P = ((rng.random((8, SIDE * SIDE)) * 2.0 - 1.0) * 3e38).astype(np.float32)
    pix = geometry()[0]
    for p in P:
        lo, hi = pix[rng.permutation(len(pix))[:2]]
        p[lo] = -3.2e38; p[hi] = 3.2e38
    return _frozen(P.reshape(-1, SIDE, SIDE))


@functools.lru_cache(maxsize=None)
def flat_support():
    """one intensity in the whole support, other values outside it: thr = 0, and the samples that reach past the support (radius 14.6
    + 6) vote -- the descriptor is NOT zero.  Eight with random pixels outside the support, eight with a blob at one corner only (what a
    keypoint at the corner of an image gives)"""
    rng = np.random.default_rng([12])
    P = rng.integers(0, 256, (16, SIDE * SIDE)).astype(np.float32)
    P[8:] = 0.0
    P = P.reshape(-1, SIDE, SIDE)
    for j in range(8, 16):
        P[j, :7, :7] = rng.integers(1, 256, (7, 7)).astype(np.float32)
    P.reshape(16, -1)[:, geometry()[0]] = (np.arange(16) % 8 * 32).astype(np.float32)[:, None]
    return _frozen(P)


PATCH_FAMILIES = dict(pair_ties=lambda: pair_ties()[0], one_hot=one_hot, one_cold=one_cold, two_level=two_level, negative=negative,
                      signed_zero=signed_zero, denormal=denormal, int_range51=int_range51, u8_blur=u8_blur, smooth=smooth,
                      smooth_q64=smooth_q64, neighbour_ties=neighbour_ties, range_inf=range_inf,
                      flat_support=flat_support)


def patches_of(name):
    return PATCH_FAMILIES[name]()


# ------------------------------------------------------------------------------------------------ extraction families
_SIZE_CDF = np.cumsum([0.04, 0.18, 0.32, 0.28, 0.14, 0.04])


def _draw(rng, n):
    size = SIZES[np.minimum(np.searchsorted(_SIZE_CDF, rng.random(n)), len(SIZES) - 1)]
    angle = ANGLES[rng.integers(0, len(ANGLES), n)]
    return size, angle


def _border_coord(rng, n, length, bias):
    """coordinates from 30 px outside the image to 30 px inside it (or to its middle), measured from either border: the depth
    (negative = outside) is deepest - (deepest + 30) u^bias -- biased inward, which is what keeps the constant patches of every image
    under the cap"""
    deepest = min(30.0, (length - 1) / 2.0)
    d = deepest - (deepest + 30.0) * rng.random(n) ** bias
    return np.where(rng.integers(0, 2, n) == 1, d, (length - 1) - d)


def _keypoints(rng, h, w, n, bias):
    size, angle = _draw(rng, n)
    return np.stack([_border_coord(rng, n, w, bias), _border_coord(rng, n, h, bias), size, angle], 1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def extraction_family(h, w, bias=None):
    """(image [h, w] float32 gray / 255, keypoints [n, 4] (x, y, size, angle in degrees)), n <= 256"""
    rng = np.random.default_rng([10, h, w])
    bias = INWARD_BIAS[(h, w)] if bias is None else bias
    img = (rng.integers(1, 256, (h, w)).astype(np.float32) * np.float32(1.0 / 255.0)).astype(np.float32)
    long_axis = 1 if w > SHORT_MAX else 0 if h > SHORT_MAX else None
    if long_axis is None:
        kps = _keypoints(rng, h, w, 200, bias)
        # every size at every angle at the image's centre, and the pure translation: size 41 / 8 at angle -90 is the identity map
        # shifted by (x - 20, y - 20)
        grid = np.array([[(w - 1) / 2, (h - 1) / 2, s, a] for s in SIZES[1:5] for a in ANGLES], np.float32)
        kps = np.concatenate([kps, grid, np.array([[20, 20, 41 / 8, -90]], np.float32)])
    else:
        if long_axis == 1:
            img[:, SHORT_MAX + 2:] = MARKER
        else:
            img[SHORT_MAX + 2:, :] = MARKER
        n = 100
        size, angle = _draw(rng, n)
        along = 32768.0 + np.rint((rng.random(n) * 120.0 - 60.0) * 4.0) / 4.0                 # quarter pixels: exact in float32
        across = rng.random(n) * 12.0 - 3.0
        near = np.stack([along, across, size, angle] if long_axis == 1 else [across, along, size, angle], 1)
        ends = _keypoints(rng, h, w, 100, bias)
        shifts = np.array([[32768.0 + d, 2.5, 41 / 8, -90] for d in (-41, -21, -20, -19, 0, 1, 20, 22)], np.float32)
        if long_axis == 0:
            shifts = shifts[:, [1, 0, 2, 3]]
        kps = np.concatenate([near, ends, shifts]).astype(np.float32)
    assert len(kps) <= 256
    return _frozen(img, kps)


def extraction_families():
    return [(f"{h}x{w}",) + tuple(extraction_family(h, w)) for h, w in IMAGE_SHAPES]


def fixed_point_bound(kps, kp_size_factor=8.0):
    """max |M * 1024| over the keypoints' inverse maps and the patch's 41 steps: the reference's (int)lrint needs it below 2^31"""
    k = np.asarray(kps, np.float64)
    scale = k[:, 2] / SIDE * kp_size_factor
    reach = np.abs(k[:, :2]).max(1) + 2 * (SIDE - 1) * scale * 2
    return float((reach * 1024).max())


def beyond_short_range(h, w):
    """how many keypoints of a long image are identity maps (size 41 / 8: one patch pixel = one image pixel) centred at a marker column
    (row): without the saturation of the coordinates their patch would hold the marker"""
    _, kps = extraction_family(h, w)
    along = kps[:, 0] if w > SHORT_MAX else kps[:, 1]
    return int(((kps[:, 2] == np.float32(41 / 8)) & (along >= SHORT_MAX + 2)).sum())


# ------------------------------------------------------------------------------------------------ grid stride
def stride_index():
    """[69,632] indices into a unique set of KINDS x PER_KIND items, kind-major: item i < 65,536 is of kind i % 4, item 65,536 + t of
    kind (t // 4) % 4 -- a group that describes items i and i + 65,536 (i < 4,096) meets all 16 ordered pairs of kinds"""
    i = np.arange(GRID_CAP); t = np.arange(GRID_EXTRA)
    first = (i % KINDS) * PER_KIND + (i // KINDS) % PER_KIND
    second = ((t // KINDS) % KINDS) * PER_KIND + (t // (KINDS * KINDS)) % PER_KIND
    return np.concatenate([first, second])


STRIDE_PATCH_KINDS = ("constant", "one_hot", "pair_tie", "smooth")


@functools.lru_cache(maxsize=None)
def stride_patches():
    """[64, 41, 41]: 16 constant patches, 16 of one_hot, 16 of pair_ties' bin-edge extras, the 16 of smooth"""
    const = np.stack([np.full((SIDE, SIDE), v, np.float32) for v in np.arange(PER_KIND) * 0.125 - 1.0])
    hot = one_hot()[:: n_support() // PER_KIND][:PER_KIND]
    tie = pair_ties()[0][n_support() - 1:][:: 2][:PER_KIND]
    return _frozen(np.concatenate([const, hot, tie, smooth()]))


STRIDE_KEYPOINT_KINDS = ("constant", "border", "plateau", "inside")


@functools.lru_cache(maxsize=None)
def stride_keypoints():
    """(image [128, 128] with a saturated rectangle, keypoints [64, 4]): 16 constant patches (far outside the image, or of tiny size),
    16 that leave the image (guarded warp, zeros -> ties), 16 inside over the rectangle's edge (clamp-free warp, ties), 16 inside on
    the smooth part (clamp-free warp)"""
    rng = np.random.default_rng([11])
    a = rng.integers(0, 256, (128, 128)).astype(np.float64)
    for _ in range(2):                                                             # (1 2 1) / 4 along both axes, wrapped: exact
        a = (np.roll(a, 1, 0) + 2.0 * a + np.roll(a, -1, 0)) / 4.0
        a = (np.roll(a, 1, 1) + 2.0 * a + np.roll(a, -1, 1)) / 4.0
    img = (a / 255.0).astype(np.float32)
    img[40:80, 50:100] = 1.0
    far = [[-500 - 40 * j, -500 + 90 * j, 5 + j, 45 * j] for j in range(8)]
    tiny = [[30 + 9 * j, 100 - 8 * j, 1e-6, 40 * j] for j in range(8)]
    border = [[(0, 127, 5, 120)[j % 4] + j, (3, 60, 125, 10)[j % 4] + 2 * j, (41 / 8, 82 / 8, 6.0, 7.5)[j // 4], 23 * j] for j in range(16)]
    plateau = [[50 + 3 * j, 38 + j % 5, (41 / 8, 3.0, 4.5, 6.0)[j % 4], 17 * j] for j in range(16)]
    inside = [[30 + 2 * j, 100 - j, (41 / 8, 2.0, 3.5, 4.0)[j % 4], -29 * j] for j in range(16)]
    return _frozen(img, np.array(far + tiny + border + plateau + inside, np.float32))
