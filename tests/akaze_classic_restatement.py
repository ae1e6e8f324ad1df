"""CPU restatement of the classic A-KAZE detector: Regard3D's "AKAZE" arm ("The classic AKAZE arm").

TEST INFRASTRUCTURE ONLY, like oracle/pyoracle.py: tests/test_gpu_akaze_classic.py compares r3dm_detect_akaze_classic with this module
bit for bit.  Regard3D calls cv::AKAZE::create(DESCRIPTOR_MLDB, 0, 3, threshold, 4, 4, DIFF_PM_G2) and detect()
(src/Regard3DFeatures.cpp:578-589).  OpenCV is absent, so the arm is defined as libAKAZE, the classic code the reference tree links
(src/thirdparty/akaze/lib/): AKAZE.cpp, nldiffusion_functions.cpp and fed.cpp with the AKAZEConfig.h defaults (4 octaves x 4
sublevels, PM_G2, soffset 1.6, derivative_factor 1.5, kcontrast percentile 0.7 over 300 bins, min_dthreshold 1e-5).

Where libAKAZE runs the OpenCV primitive that oracle/akaze.c already restates, this module calls the oracle: GaussianBlur with
BORDER_REPLICATE (oracle.akaze_gaussian), Scharr (oracle.akaze_scharr) and resize INTER_AREA (oracle.akaze_halfsample).  The
multiscale derivative is sepFilter2D with the same tap structure as oracle.akaze_scaled_deriv, but libAKAZE's kernels are normalised
by the scale (compute_derivative_kernels: norm = 1 / (2 scale (w + 2)), Fast-AKAZE's V2 kernels drop the scale), so it is restated
here with those taps.  Everything else is libAKAZE's arithmetic, written out below; numpy float32 element-wise arithmetic is the
reference's float arithmetic operation for operation (no contraction), and the host libm is called through ctypes (powf) or math
(cos, sqrt) exactly where libAKAZE calls it.

Orientation: libAKAZE's Feature_Detection leaves angle = 0; OpenCV 4's detect() assigns one.  The arm computes
Compute_Main_Orientation (AKAZE.cpp:563-625) on the level's Lx / Ly as the multiscale derivative pass leaves them, converts the
radians to degrees in double and wraps 360 to 0: angle in [0, 360), no + 90 (Regard3D adds 90 to the Fast arm only).

>>> PARITY WITH OPENCV UNPINNED: OpenCV 4's extrema search is a reworked parallel form that cannot be built or checked here. <<<
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

f32 = np.float32
SOFFSET, DFAC = f32(1.6), f32(1.5)
OMAX, NSUB = 4, 4
MIN_DTHRESHOLD = f32(0.00001)
SMAX = f32(10.0 * float(np.sqrt(f32(2.0))))          # smax = 10.0 * sqrtf(2.0f), MLDB
NBINS, KPERC = 300, f32(0.7)

_libm = C.CDLL("libm.so.6")
_libm.powf.restype = C.c_float
_libm.powf.argtypes = [C.c_float, C.c_float]

GAUSS25 = np.array([
    [0.02546481, 0.02350698, 0.01849125, 0.01239505, 0.00708017, 0.00344629, 0.00142946],
    [0.02350698, 0.02169968, 0.01706957, 0.01144208, 0.00653582, 0.00318132, 0.00131956],
    [0.01849125, 0.01706957, 0.01342740, 0.00900066, 0.00514126, 0.00250252, 0.00103800],
    [0.01239505, 0.01144208, 0.00900066, 0.00603332, 0.00344629, 0.00167749, 0.00069579],
    [0.00708017, 0.00653582, 0.00514126, 0.00344629, 0.00196855, 0.00095820, 0.00039744],
    [0.00344629, 0.00318132, 0.00250252, 0.00167749, 0.00095820, 0.00046640, 0.00019346],
    [0.00142946, 0.00131956, 0.00103800, 0.00069579, 0.00039744, 0.00019346, 0.00008024]], np.float32)


def _oracle():
    from oracle import pyoracle
    return pyoracle


def fround(v) -> int:
    """fRound (AKAZE.h:200): (int)(flt + 0.5f), truncation toward zero"""
    return int(f32(v) + f32(0.5))


# ---------------------------------------------------------------------------------------------------- evolution table
def levels(w: int, h: int):
    """Allocate_Memory_Evolution (AKAZE.cpp:51-99): a list of dicts (w, h, octave, sublevel, esigma, etime, ratio, sigma_size).
    An octave i > 0 whose level is < 80 wide or < 40 high ends the table; octave 0 always exists."""
    lv = []
    for i in range(OMAX):
        rf = 1.0 / 2.0 ** i                                   # rfactor = 1.0 / pow(2.0f, i) (double)
        lh, lw = int(h * rf), int(w * rf)
        if (lw < 80 or lh < 40) and i != 0:
            break
        for j in range(NSUB):
            esigma = f32(SOFFSET * f32(_libm.powf(2.0, float(f32(f32(j) / f32(NSUB) + f32(i))))))
            ratio = f32(2.0 ** i)
            lv.append(dict(w=lw, h=lh, octave=i, sublevel=j, esigma=esigma, etime=f32(0.5 * float(f32(esigma * esigma))),
                           ratio=ratio, sigma_size=fround(f32(f32(esigma * DFAC) / ratio))))
    return lv


def _is_prime(n: int) -> bool:
    if n <= 1:
        return False
    if n in (2, 3, 5, 7):
        return True
    if n % 2 == 0 or n % 3 == 0 or n % 5 == 0 or n % 7 == 0:
        return False
    upper = int(math.sqrt(n + 1.0))
    d = 11
    while d <= upper:
        if n % d == 0:
            return False
        d += 2
    return True


def fed_tau(T) -> list:
    """fed_tau_by_process_time(T, 1, 0.25, reordering = true) (fed.cpp): n and scale in double, cos of the host libm in double.
    (libAKAZE reorders even n == 1, reading tauh[-1]; the evolution of these defaults never has n == 1, where this returns tauh.)"""
    t = f32(T)
    tau_max = f32(0.25)
    n = int(math.ceil(math.sqrt(3.0 * float(t) / float(tau_max) + 0.25) - 0.5 - float(f32(1.0e-8))) + 0.5)
    if n <= 0:
        return []
    scale = f32(3.0 * float(t) / float(f32(tau_max * f32(n * (n + 1)))))
    c = f32(f32(1.0) / f32(f32(4.0) * f32(n) + f32(2.0)))
    d = f32(f32(scale * tau_max) / f32(2.0))
    tauh = []
    for k in range(n):
        hh = f32(math.cos(math.pi * float(f32(f32(2.0) * f32(k) + f32(1.0))) * float(c)))
        tauh.append(f32(d / f32(hh * hh)))
    if n == 1:
        return tauh
    kappa, prime = n // 2, n + 1
    while not _is_prime(prime):
        prime += 1
    tau = [f32(0)] * n
    k = l = 0
    while l < n:
        while True:
            index = ((k + 1) * kappa) % prime - 1
            if index >= n:
                k += 1
            else:
                break
        tau[l] = tauh[index]
        k += 1
        l += 1
    return tau


# ---------------------------------------------------------------------------------------------------- scale space
def modulus_histogram(modg: np.ndarray):
    """the histogram of compute_k_percentile (nldiffusion_functions.cpp:166-186) over gradient moduli: (hmax, hist [300] float64,
    the counted points).  A zero modulus is not counted; nbin = floor(nbins * (modg / hmax)) with nbins itself (modg == hmax) folded
    into the last bin; a FLOAT histogram (a float count stops at 2^24)"""
    hmax = f32(max(f32(0.0), modg.max())) if modg.size else f32(0.0)
    nz = modg[modg != 0.0]
    hist = np.zeros(NBINS, np.float64)
    if nz.size:
        nbin = np.floor(f32(NBINS) * (nz / hmax)).astype(np.int64)
        nbin[nbin == NBINS] = NBINS - 1
        hist = np.minimum(np.bincount(nbin, minlength=NBINS).astype(np.float64), 2.0 ** 24)
    return hmax, hist, nz.size


def kcontrast_parts(img: np.ndarray):
    """compute_k_percentile(img, 0.7, 1.0, 300, 0, 0) (nldiffusion_functions.cpp:126-199): the INPUT image, sigma 1, Scharr, the
    histogram above, 0.03 if the percentile is not reached -> (hmax, hist [300] float64, k)"""
    O = _oracle()
    lx, ly = O.akaze_scharr(O.akaze_gaussian(img, 1.0))
    lx, ly = lx[1:-1, 1:-1], ly[1:-1, 1:-1]
    hmax, hist, n = modulus_histogram(np.sqrt(lx * lx + ly * ly))
    npoints = f32(min(n, 2 ** 24))
    nthreshold = int(f32(npoints * KPERC))
    nelements, k = 0, 0
    while nelements < nthreshold and k < NBINS:
        nelements = int(f32(f32(nelements) + f32(hist[k])))
        k += 1
    if nelements < nthreshold:
        return hmax, hist, f32(0.03)
    return hmax, hist, f32(hmax * f32(f32(k) / f32(NBINS)))


def kcontrast(img: np.ndarray) -> np.float32:
    return kcontrast_parts(img)[2]


def nld_step(L: np.ndarray, c: np.ndarray, stepsize) -> np.ndarray:
    """nld_step_scalar (nldiffusion_functions.cpp:208-331): Lstep = 0.5f * stepsize * (xpos - xneg + ypos - yneg) with the
    reference's own border forms; returns L + Lstep (the whole Lstep is formed before L is updated)"""
    h, w = L.shape
    hs = f32(f32(0.5) * f32(stepsize))
    Dx = (c[:, :-1] + c[:, 1:]) * (L[:, 1:] - L[:, :-1])     # flux between x and x + 1: xpos(x) = Dx[x], xneg(x) = Dx[x - 1]
    Dy = (c[:-1] + c[1:]) * (L[1:] - L[:-1])                  # flux between y and y + 1: ypos(y) = Dy[y], yneg(y) = Dy[y - 1]
    Dyl = (c[-1] + c[-2]) * (L[-2] - L[-1])                   # the last row's "ypos" looks up
    S = np.empty_like(L)
    S[1:-1, 1:-1] = ((Dx[1:-1, 1:] - Dx[1:-1, :-1]) + Dy[1:, 1:-1]) - Dy[:-1, 1:-1]
    S[0, 1:-1] = (Dx[0, 1:] - Dx[0, :-1]) + Dy[0, 1:-1]
    S[0, 0] = Dx[0, 0] + Dy[0, 0]
    S[0, -1] = (-Dx[0, -1]) + Dy[0, -1]
    S[-1, 1:-1] = (Dx[-1, 1:] - Dx[-1, :-1]) + Dyl[1:-1]
    S[-1, 0] = Dx[-1, 0] + Dyl[0]
    S[-1, -1] = (-Dx[-1, -1]) + Dyl[-1]
    S[1:-1, 0] = (Dx[1:-1, 0] + Dy[1:, 0]) - Dy[:-1, 0]
    S[1:-1, -1] = ((-Dx[1:-1, -1]) + Dy[1:, -1]) - Dy[:-1, -1]
    return L + hs * S


def _refl101(p: np.ndarray, n: int) -> np.ndarray:
    p = p.copy()
    if n == 1:
        return np.zeros_like(p)
    while True:
        lo, hi = p < 0, p >= n
        if not (lo.any() or hi.any()):
            return p
        p[lo] = -p[lo]
        p[hi] = 2 * n - 2 - p[hi]


def deriv_taps(s: int):
    """compute_derivative_kernels (nldiffusion_functions.cpp:346-383), scale >= 2: w = 10 / 3 in float, norm = 1 / (2 scale (w + 2))
    in double, the centre tap w * norm in float"""
    wq = f32(10.0 / 3.0)
    norm = f32(1.0 / (2.0 * s * (float(wq) + 2.0)))
    return norm, f32(wq * norm)


def scaled_deriv(src: np.ndarray, s: int, dx: bool) -> np.ndarray:
    """compute_scharr_derivatives(src, dst, dx, !dx, s) = sepFilter2D, BORDER_REFLECT_101: the tap structure of
    oracle.akaze_scaled_deriv with libAKAZE's scale-normalised taps"""
    h, w = src.shape
    norm, kc = deriv_taps(s)
    xs = np.arange(w)
    a, b = src[:, _refl101(xs - s, w)], src[:, _refl101(xs + s, w)]
    if dx:
        t = (-a) + b
    elif s == 2:
        t = src * kc + (a + b) * norm
    else:
        t = (norm * a + kc * src) + norm * b
    ys = np.arange(h)
    u, d = t[_refl101(ys - s, h)], t[_refl101(ys + s, h)]
    return (kc * t + norm * (d + u)) if dx else (d - u)


def scale_space(img: np.ndarray):
    """Create_Nonlinear_Scale_Space (AKAZE.cpp:102-170) and Compute_Multiscale_Derivatives / Compute_Determinant_Hessian_Response
    (:188-248): per level a dict with Ldet, Lx, Ly (the scaled derivatives), Lsmooth (what they are taken from), Lflow (the
    conductivity, None at level 0) and Lt (as the level's FED steps leave it) added to the table entry"""
    O = _oracle()
    img = np.ascontiguousarray(img, np.float32)
    h, w = img.shape
    lv = levels(w, h)
    with np.errstate(divide="ignore", invalid="ignore"):      # a flat image: k = 0, libAKAZE's conductivity is then NaN too
        return _scale_space(O, img, lv)


def _scale_space(O, img, lv):
    k = kcontrast(img)
    Lt = O.akaze_gaussian(img, float(SOFFSET))
    smooth = [Lt]
    lv[0]["Lt"], lv[0]["Lflow"] = Lt, None                     # (level 0 has no conductivity and no FED step)
    for i in range(1, len(lv)):
        if lv[i]["octave"] > lv[i - 1]["octave"]:
            Lt = O.akaze_halfsample(Lt)
            k = f32(k * f32(0.75))
        else:
            Lt = Lt.copy()
        Ls = O.akaze_gaussian(Lt, 1.0)
        lx, ly = O.akaze_scharr(Ls)
        inv_k = f32(f32(1.0) / f32(k * k))
        flow = f32(1.0) / (f32(1.0) + inv_k * (lx * lx + ly * ly))
        for tau in fed_tau(f32(lv[i]["etime"] - lv[i - 1]["etime"])):
            Lt = nld_step(Lt, flow, tau)
        smooth.append(Ls)
        lv[i]["Lt"], lv[i]["Lflow"] = Lt, flow                  # Lt as the level's FED steps leave it
    for e, Ls in zip(lv, smooth):
        s = e["sigma_size"]
        Lx = scaled_deriv(Ls, s, True)
        Ly = scaled_deriv(Ls, s, False)
        Lxx = scaled_deriv(Lx, s, True)
        Lyy = scaled_deriv(Ly, s, False)
        Lxy = scaled_deriv(Lx, s, False)
        e["Ldet"] = (Lxx * Lyy - Lxy * Lxy) * f32(s * s * s * s)
        e["Lx"], e["Ly"], e["Lsmooth"] = Lx, Ly, Ls
    return lv, k


# ---------------------------------------------------------------------------------------------------- detection
def candidates(ldet: np.ndarray, dthreshold) -> np.ndarray:
    """strict 3 x 3 maxima over dthreshold and min_dthreshold, rows 1..h-2 x columns 1..w-2, raster order: (row, col) pairs"""
    c = ldet[1:-1, 1:-1]
    m = (c > f32(dthreshold)) & (c >= MIN_DTHRESHOLD)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                m &= c > ldet[1 + dy:ldet.shape[0] - 1 + dy, 1 + dx:ldet.shape[1] - 1 + dx]
    ys, xs = np.nonzero(m)
    return np.stack([ys + 1, xs + 1], 1)


class AuxList:
    """kpts_aux of Find_Scale_Space_Extrema: slots of (x, y, size, response, class_id, octave)"""

    def __init__(self, cap: int):
        self.x = np.zeros(cap, np.float32); self.y = np.zeros(cap, np.float32)
        self.size = np.zeros(cap, np.float32); self.resp = np.zeros(cap, np.float32)
        self.cls = np.full(cap, -9, np.int64); self.octave = np.zeros(cap, np.int64)
        self.n = 0

    def put(self, slot, x, y, size, resp, cls, octave):
        self.x[slot], self.y[slot], self.size[slot], self.resp[slot] = x, y, size, resp
        self.cls[slot], self.octave[slot] = cls, octave


def offer(aux: AuxList, level: dict, i: int, row: int, col: int, value, cap_rows: int, cap_cols: int) -> None:
    """one extremum of level i at (row, col) through the sequential kpts_aux rule (AKAZE.cpp:288-350):
    the FIRST slot in list order of level i - 1 or i within size^2 decides -- a larger response replaces that slot in place, any other
    rejects the point; then the descriptor border test (smax = 10 sqrt 2); a surviving point is appended or written to its slot"""
    size = f32(level["esigma"] * DFAC)
    ratio = f32(level["ratio"])
    ss = fround(f32(size / ratio))
    px, py = f32(col), f32(row)
    n = aux.n
    is_rep, slot = False, -1
    if n:
        tx = f32(px * ratio) - aux.x[:n]
        ty = f32(py * ratio) - aux.y[:n]
        dist = tx * tx + ty * ty
        hit = ((aux.cls[:n] == i) | (aux.cls[:n] == i - 1)) & (dist <= f32(size * size))
        if hit.any():
            q = int(np.argmax(hit))
            if f32(value) > aux.resp[q]:
                is_rep, slot = True, q
            else:
                return
    r = f32(SMAX * f32(ss))
    left, right = fround(f32(px - r)) - 1, fround(f32(px + r)) + 1
    up, down = fround(f32(py - r)) - 1, fround(f32(py + r)) + 1
    if left < 0 or right >= cap_cols or up < 0 or down >= cap_rows:
        return
    off = 0.5 * (float(ratio) - 1.0)
    x, y = f32(float(f32(px * ratio)) + off), f32(float(f32(py * ratio)) + off)
    if not is_rep:
        slot = aux.n
        aux.n += 1
    aux.put(slot, x, y, size, f32(value), i, level["octave"])


def upper_filter(aux: AuxList) -> np.ndarray:
    """the upper-level filter (AKAZE.cpp:352-381): slot i goes if a LATER slot j > i of class_id + 1 lies within slot i's size and
    has a larger response.  Returns the kept slots in list order."""
    n = aux.n
    keep = []
    for i in range(n):
        tx = aux.x[i] - aux.x[i + 1:n]
        ty = aux.y[i] - aux.y[i + 1:n]
        dist = tx * tx + ty * ty
        drop = (aux.cls[i + 1:n] == aux.cls[i] + 1) & (dist <= f32(aux.size[i] * aux.size[i])) & (aux.resp[i] < aux.resp[i + 1:n])
        if not drop.any():
            keep.append(i)
    return np.array(keep, np.int64)


def refine(ldet: np.ndarray, x: float, y: float, octave: int):
    """Do_Subpixel_Refinement (AKAZE.cpp:389-460) for one keypoint: (x, y) refined, or None when |d| > 1 erases it.  The reference
    mixes double constants into float operands: Dx, Dy, Dxx, Dyy and Dxy are formed in double as written and stored as float;
    cv::solve(2 x 2, DECOMP_LU) is Cramer's rule in double (core/lapack.cpp), 0 when the determinant is 0."""
    ratio = f32(2.0 ** octave)
    xi, yi = fround(f32(f32(x) / ratio)), fround(f32(f32(y) / ratio))
    L = ldet
    c, l, r, u, d = L[yi, xi], L[yi, xi - 1], L[yi, xi + 1], L[yi - 1, xi], L[yi + 1, xi]
    Dx = f32(0.5 * float(f32(r - l)))
    Dy = f32(0.5 * float(f32(d - u)))
    Dxx = f32(float(f32(r + l)) - 2.0 * float(c))
    Dyy = f32(float(f32(d + u)) - 2.0 * float(c))
    Dxy = f32(0.25 * float(f32(L[yi + 1, xi + 1] + L[yi - 1, xi - 1])) - 0.25 * float(f32(L[yi - 1, xi + 1] + L[yi + 1, xi - 1])))
    b0, b1 = f32(-Dx), f32(-Dy)
    det = float(Dxx) * float(Dyy) - float(Dxy) * float(Dxy)
    dx = dy = f32(0.0)
    if det != 0.0:
        det = 1.0 / det
        t = f32((float(b0) * float(Dyy) - float(b1) * float(Dxy)) * det)
        dy = f32((float(b1) * float(Dxx) - float(b0) * float(Dxy)) * det)
        dx = t
    if abs(float(dx)) > 1.0 or abs(float(dy)) > 1.0:
        return None
    power = 1 << octave
    ox = f32(float(f32(f32(f32(xi) + dx) * f32(power))) + 0.5 * (power - 1))
    oy = f32(float(f32(f32(f32(yi) + dy) * f32(power))) + 0.5 * (power - 1))
    return ox, oy


_P = [f32(f32(c) * f32(180.0 / math.pi)) for c in (0.9997878412794807, -0.3258083974640975, 0.1555786518463281, -0.04432655554792128)]
_EPS = f32(2.220446049250313e-16)


def fast_atan2_deg(y: np.ndarray, x: np.ndarray) -> np.ndarray:
    """cv::fastAtan2 (OpenCV 4 core mathfuncs_core atan_f32): degrees in [0, 360]"""
    y = np.asarray(y, np.float32); x = np.asarray(x, np.float32)
    ax, ay = np.abs(x), np.abs(y)
    p1, p3, p5, p7 = _P
    with np.errstate(invalid="ignore", divide="ignore"):
        ge = ax >= ay
        cc = np.where(ge, ay / (ax + _EPS), ax / (ay + _EPS)).astype(np.float32)
        c2 = cc * cc
        poly = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * cc
        a = np.where(ge, poly, f32(90.0) - poly).astype(np.float32)
        a = np.where(x < 0, f32(180.0) - a, a).astype(np.float32)
        a = np.where(y < 0, f32(360.0) - a, a).astype(np.float32)
    return a


def _windows():
    """the ang1 sweep of Compute_Main_Orientation: ang1 += 0.15f in float while ang1 < 2 pi (double); ang2 in double, stored float"""
    out = []
    a1 = f32(0.0)
    while float(a1) < 2.0 * math.pi:
        if float(a1) + math.pi / 3.0 > 2.0 * math.pi:
            a2 = f32(float(a1) - 5.0 * math.pi / 3.0)
        else:
            a2 = f32(float(a1) + math.pi / 3.0)
        out.append((a1, a2))
        a1 = f32(a1 + f32(0.15))
    return out


WINDOWS = _windows()
_ID = [6, 5, 4, 3, 2, 1, 0, 1, 2, 3, 4, 5, 6]
_SAMPLES = [(i, j) for i in range(-6, 7) for j in range(-6, 7) if i * i + j * j < 36]
_SI = np.array([s[0] for s in _SAMPLES]); _SJ = np.array([s[1] for s in _SAMPLES])
_SW = np.array([GAUSS25[_ID[i + 6], _ID[j + 6]] for i, j in _SAMPLES], np.float32)


def orientation_deg(Lx: np.ndarray, Ly: np.ndarray, x, y, size, octave: int) -> np.float32:
    """Compute_Main_Orientation (AKAZE.cpp:563-625) -> degrees: the radian angle times 180 / pi in double, 360 wrapped to 0.
    Sample (i, j) reads column fRound(xf + i s), row fRound(yf + j s); each window sums its samples in order 0..108 in float."""
    ratio = f32(1 << octave)
    s = fround(f32(0.5 * float(size) / float(ratio)))
    xf, yf = f32(f32(x) / ratio), f32(f32(y) / ratio)
    iy = (yf + (_SJ * s).astype(np.float32) + f32(0.5)).astype(np.int64)
    ix = (xf + (_SI * s).astype(np.float32) + f32(0.5)).astype(np.int64)
    rx = _SW * Lx[iy, ix]
    ry = _SW * Ly[iy, ix]
    ang = (fast_atan2_deg(ry, rx).astype(np.float64) * (math.pi / 180.0)).astype(np.float32)
    angd = ang.astype(np.float64)
    masks = []
    for a1, a2 in WINDOWS:
        if a1 < a2:
            m = (a1 < ang) & (ang < a2)
        elif a2 < a1:
            m = ((ang > 0) & (ang < a2)) | ((ang > a1) & (angd < 2.0 * math.pi))
        else:
            m = np.zeros(ang.shape, bool)
        masks.append(m)
    M = np.array(masks)
    sx = np.cumsum(np.where(M, rx, f32(0.0)).astype(np.float32), axis=1, dtype=np.float32)[:, -1]
    sy = np.cumsum(np.where(M, ry, f32(0.0)).astype(np.float32), axis=1, dtype=np.float32)[:, -1]
    best, angle = f32(0.0), f32(0.0)
    for q in range(len(WINDOWS)):
        nrm = f32(sx[q] * sx[q] + sy[q] * sy[q])
        if nrm > best:
            best = nrm
            angle = f32(float(fast_atan2_deg(sy[q], sx[q])) * (math.pi / 180.0))
    deg = f32(float(angle) * (180.0 / math.pi))
    if deg >= f32(360.0):
        deg = f32(deg - f32(360.0))
    return deg


def detect(img: np.ndarray, threshold: float = 0.001):
    """the "AKAZE" arm: {"kps": [n, 4] (x, y, size, angle degrees), "responses": [n]} in the reference's order (kpts_aux slot
    order after the upper-level filter and the refinement's erasures)"""
    img = np.ascontiguousarray(img, np.float32)
    h, w = img.shape
    if w < 3 or h < 3:
        return {"kps": np.zeros((0, 4), np.float32), "responses": np.zeros(0, np.float32)}
    lv, _ = scale_space(img)
    thr = f32(threshold)
    cand = [candidates(e["Ldet"], thr) for e in lv]
    aux = AuxList(max(1, sum(len(c) for c in cand)))
    for i, e in enumerate(lv):
        L = e["Ldet"]
        for row, col in cand[i]:
            offer(aux, e, i, int(row), int(col), L[row, col], e["h"], e["w"])
    kps, resp = [], []
    for q in upper_filter(aux):
        e = lv[int(aux.cls[q])]
        r = refine(e["Ldet"], aux.x[q], aux.y[q], int(aux.octave[q]))
        if r is None:
            continue
        size = f32(aux.size[q] * f32(2.0))
        ang = orientation_deg(e["Lx"], e["Ly"], r[0], r[1], size, int(aux.octave[q]))
        kps.append((r[0], r[1], size, ang))
        resp.append(aux.resp[q])
    return {"kps": np.array(kps, np.float32).reshape(-1, 4), "responses": np.array(resp, np.float32)}
