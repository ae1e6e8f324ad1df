"""Images and determinant planes built for the edges of the classic A-KAZE head -- the k-contrast histogram, the FED steps, the
scale-normalised Scharr derivatives, the Hessian determinant, the extremum passes and the row scan ("The head,
plane by plane").  Shared by tests/test_akaze_classic_head_cases.py (CPU: every case reaches the edge it is named for, shown on the
reference alone) and tests/test_gpu_akaze_classic_head.py (GPU: the developer build's r3dm_dev_akaze_classic_head /
r3dm_dev_akaze_classic_extrema run the product's functions on the same inputs, every word, plane and list entry bit for bit).

The reference is tests/akaze_classic_restatement.py alone.  A case is dict(name, family, kind, thr, proof):
  kind "image":  image (a name kind-WxH of image()); reference(case) = the restatement's k-contrast words, planes and candidates
                 (head_reference); proof(case, ref) asserts on the reference that the edge is reached;
  kind "planes": size (w, h) of a level table and planes [n_levels] Ldet -- seeded values far below the threshold and the 1e-5 floor
                 with the engineered values written over them -- and want, the candidate list the plan of the case predicts;
                 reference(case) = R.candidates per level.
References are computed once per process and never written to.

The proof counts measured on the restatement (the proofs assert "at least one", not these counts):
  noise-163x83-1e-07   candidates of octave 0 on row 1 / row h-2 / column 1 / column w-2 / column 64 / column 65: 19 / 22 / 3 / 1 /
                       11 / 7; octave 1 (81 x 41) on columns 64 / 65: 3 / 5; strict maxima between the threshold and the 1e-5
                       floor: 3 to 15 on every level ([10, 7, 13, 3, 9, 9, 10, 15])
  noise-163x83-0.001   candidates per level [119, 45, 27, 11, 0, 0, 0, 0]: the upper octave is empty
  steps-163x83         the sigma-1 Scharr modulus is exactly 0 on 5650 of the 13041 interior pixels; the scan stops after 94 bins, it
                       would stop after 41 if zeros were counted.  NO plane of the reference holds a subnormal on this image: the
                       flat parts of Lt and Ldet are exact zeros (0 subnormals in Lt and in Ldet on all 8 levels)
  faint-67x45          Ldet holds 2875 / 2850 / 2841 / 2766 non-zero subnormals on levels 0 .. 3 (its largest magnitude is 0.014 of
                       the smallest normal; the rest underflowed to 0) beside the normal values of the level's Lsmooth, Lt, Lx and
                       Ly, which hold no subnormal; k = 4.84e-19, 1 / k^2 = 4.3e36 .. 2.4e38
  ramp-160x80          12324 counted moduli, 12012 of them in bin 299; the scan stops only after the last bin
  pixel-160x80         48 counted moduli around the pixel, 12276 zeros
  scene-321x161-0.001  candidates per octave 10 / 18 / 20; scene-640x320-0.001: 58 / 82 / 80 / 33
  dense-67x300         4917 candidates a level, 19668 in all, on concatenated rows 1 .. 1198; dense-131x45: 1430 a level"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import akaze_classic_restatement as R  # noqa: E402

F = np.float32
NBINS = 300
PTHR = F(1e-3)
FLOOR = R.MIN_DTHRESHOLD
PLANE_NAMES = ("Lsmooth", "Lflow", "Lt", "Lx", "Ly", "Ldet")          # the order a level's planes are compared in
TINY = np.finfo(np.float32).tiny
_IMAGES, _SPACE, _REF, _ALL = {}, {}, {}, None


# ------------------------------------------------------------------------------------------------ the images
def _scene(h, w, seed, n_blobs, noise=0.01, smin=2.0, smax=12.0):
    """smooth blobs on a slow wave, a little noise (the scenes of tests/test_gpu_akaze_classic.py)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = 0.5 + 0.1 * np.sin(xx / 17.0) * np.cos(yy / 23.0)
    for _ in range(n_blobs):
        mg = min(40, h // 4)
        cx, cy = rng.uniform(mg, w - mg), rng.uniform(mg, h - mg)
        s = rng.uniform(smin, smax); a = rng.uniform(0.15, 0.45) * rng.choice([-1, 1])
        th = rng.uniform(0, np.pi); e = rng.uniform(1.0, 2.5)
        u = (xx - cx) * np.cos(th) + (yy - cy) * np.sin(th); v = -(xx - cx) * np.sin(th) + (yy - cy) * np.cos(th)
        img = img + a * np.exp(-(u * u / (2 * s * s * e) + v * v / (2 * s * s / e)))
    img = img + rng.normal(0, noise, img.shape)
    return np.clip(img, 0, 1).astype(F)


def _steps(h, w):
    """piecewise constant: a black frame 9 wide, blocks of 11 x 11 with seeded levels, one flat block over the middle"""
    rng = np.random.default_rng(500 * w + h)
    img = np.zeros((h, w), F)
    for y0 in range(9, h - 9, 11):
        for x0 in range(9, w - 9, 11):
            img[y0:min(y0 + 11, h - 9), x0:min(x0 + 11, w - 9)] = F(rng.integers(1, 32)) / F(32)
    img[h // 4:h - h // 4, w // 4:w // 2 + w // 8] = F(0.5)
    return img


def _make_image(name):
    kind, size = name.split("-")
    w, h = (int(v) for v in size.split("x"))
    noise = lambda: np.random.default_rng(1000 * w + h).uniform(0, 1, (h, w)).astype(F)   # noqa: E731
    if kind == "noise":
        return noise()
    if kind == "faint":
        return noise() * F(2.0 ** -62)
    if kind == "scene":
        return _scene(h, w, 7000 * w + h, max(4, h * w // 8000))
    if kind == "steps":
        return _steps(h, w)
    if kind == "flat":
        return np.full((h, w), F(0.5))
    if kind == "ramp":
        return np.ascontiguousarray(np.broadcast_to((np.arange(w, dtype=F) / F(256))[None, :], (h, w)))
    if kind == "pixel":
        img = np.full((h, w), F(0.25)); img[h // 2, w // 2] = F(1.0)
        return img
    raise ValueError(name)


def image(name):
    """an image by name: kind-WxH, made once per process and never written to"""
    if name not in _IMAGES:
        _IMAGES[name] = _make_image(name)
        _IMAGES[name].setflags(write=False)
    return _IMAGES[name]


def size_of(name):
    w, h = (int(v) for v in name.split("-")[1].split("x"))
    return w, h


# ------------------------------------------------------------------------------------------------ the references
def inv_k2(k):
    """1 / k_o^2 of octaves 0 .. 7, k_o = k_{o-1} * 0.75 (Create_Nonlinear_Scale_Space, as _scale_space forms it per octave)"""
    out = []
    k = F(k)
    with np.errstate(divide="ignore"):
        for _ in range(8):
            out.append(F(F(1.0) / F(k * k))); k = F(k * F(0.75))
    return np.array(out, F)


def candidate_lists(planes, thr):
    """R.candidates of every level -> dict(counts [nl] uint32; x, y, level uint32 and value float32 in scan order)"""
    per = [R.candidates(P, thr) for P in planes]
    x = np.concatenate([c[:, 1] for c in per]).astype(np.uint32); y = np.concatenate([c[:, 0] for c in per]).astype(np.uint32)
    level = np.concatenate([np.full(len(c), i) for i, c in enumerate(per)]).astype(np.uint32)
    value = np.concatenate([P[c[:, 0], c[:, 1]] for P, c in zip(planes, per)]).astype(F)
    return dict(counts=np.array([len(c) for c in per], np.uint32), x=x, y=y, level=level, value=value)


def scale_space(name, step=None):
    """the restatement's k-contrast words and level planes of an image (step: another nld_step, for the mutation tests; not cached)"""
    if step is None and name in _SPACE:
        return _SPACE[name]
    img = image(name)
    hmax, hist, k = R.kcontrast_parts(img)
    keep = R.nld_step
    try:
        if step is not None:
            R.nld_step = step
        lv, _ = R.scale_space(img)
    finally:
        R.nld_step = keep
    out = dict(hmax=hmax, hist=hist.astype(np.uint32), k=k, inv_k2=inv_k2(k), levels=lv)
    if step is None:
        _SPACE[name] = out
    return out


def head_reference(name, thr, step=None, candidates=None):
    """what r3dm_dev_akaze_classic_head returns for the image, from the restatement (candidates: another candidate_lists)"""
    key = (name, float(thr))
    if step is None and candidates is None and key in _REF:
        return _REF[key]
    out = dict(scale_space(name, step))
    out.update((candidates or candidate_lists)([e["Ldet"] for e in out["levels"]], thr))
    if step is None and candidates is None:
        _REF[key] = out
    return out


def reference(case):
    if case["kind"] == "image":
        return head_reference(case["image"], case["thr"])
    if case["name"] not in _REF:
        _REF[case["name"]] = candidate_lists(case["planes"], case["thr"])
    return _REF[case["name"]]


# ------------------------------------------------------------------------------------------------ the comparison both halves use
def _differs(got, ref):
    """positions where two arrays differ: NaN against NaN agrees whatever the payload and sign, every other value bit for bit"""
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.dtype == ref.dtype, (got.dtype, ref.dtype)
    if got.dtype.kind == "f":
        bits = got.view(np.uint32) != ref.view(np.uint32)
        return bits & ~(np.isnan(got) & np.isnan(ref))
    return got != ref


def first_mismatch(got, ref, planes=True):
    """None, or (stage, text, first positions) of the FIRST stage at which a head result differs from another, in pipeline order: hmax bits, histogram,
    1 / k^2, then per level Lsmooth, Lflow, Lt, Lx, Ly, Ldet, then counts and the candidate list; planes=False: counts and list only"""
    def diff(stage, a, b):
        a, b = np.asarray(a), np.asarray(b)
        if a.shape != b.shape:
            return stage, f"{stage}: shape {a.shape} against {b.shape}", []
        d = _differs(a, b)
        if d.any():
            where = np.argwhere(np.atleast_1d(d))[:6].tolist()
            pick = lambda v: [np.atleast_1d(v)[tuple(p)].tolist() for p in where]   # noqa: E731
            return stage, f"{stage}: differs at {where} (row, column of a plane): got {pick(a)}, reference {pick(b)}", where
        return None
    checks = []
    if planes:
        checks += [("hmax bits", np.uint32(got["hmax_bits"]), F(ref["hmax"]).view(np.uint32) if "hmax" in ref else ref["hmax_bits"]),
                   ("histogram", got["hist"], ref["hist"]), ("1 / k^2 [0..7]", got["inv_k2"], ref["inv_k2"])]
        gl, rl = got["planes"], ref["levels"] if "levels" in ref else ref["planes"]
        if len(gl) != len(rl):
            return "levels", f"levels: {len(gl)} against {len(rl)}", []
        for i, (g, r) in enumerate(zip(gl, rl)):
            for q in PLANE_NAMES:
                if r[q] is None and g[q] is None:
                    continue
                checks.append((f"level {i} {q}", g[q], r[q]))
    checks += [("counts", got["counts"], ref["counts"])] + [(f"candidate {q}", got[q], ref[q]) for q in ("level", "y", "x", "value")]
    for stage, a, b in checks:
        m = diff(stage, a, b)
        if m:
            return m
    return None


# ------------------------------------------------------------------------------------------------ proofs of the image cases
def _on(ref, level_set, col=None, row=None):
    m = np.isin(ref["level"], list(level_set))
    if col is not None:
        m &= ref["x"] == col
    if row is not None:
        m &= ref["y"] == row
    return int(m.sum())


def below_floor(P, thr):
    """strict 3 x 3 maxima of a plane over thr that only the v >= 1e-5 floor excludes"""
    c = P[1:-1, 1:-1]
    m = (c > F(thr)) & (c < FLOOR)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                m &= c > P[1 + dy:P.shape[0] - 1 + dy, 1 + dx:P.shape[1] - 1 + dx]
    return int(m.sum())


def _table_proof(c, r):
    w, h = size_of(c["image"])
    lv = r["levels"]
    octaves = sorted({e["octave"] for e in lv})
    assert len(lv) == 4 * len(octaves) and (lv[0]["w"], lv[0]["h"]) == (w, h)
    want = {(67, 45): 1, (131, 43): 1, (160, 80): 2, (163, 83): 2, (321, 161): 3, (640, 320): 4}[(w, h)]
    assert len(octaves) == want, (w, h, len(octaves))
    if (w, h) == (160, 80):
        assert (lv[4]["w"], lv[4]["h"]) == (80, 40), "exactly the cut's boundary"
        assert len(R.levels(159, 80)) == 4 and len(R.levels(160, 79)) == 4, "one less on either axis ends the table after octave 0"
    if (w, h) == (163, 83):
        assert (lv[4]["w"], lv[4]["h"]) == (81, 41) and 2 * 81 != 163 and 2 * 41 != 83, "inexact INTER_AREA halving"
    if (w, h) == (640, 320):
        assert max(len(R.fed_tau(F(lv[i]["etime"] - lv[i - 1]["etime"]))) for i in range(1, 16)) == 29
    if (w, h) in ((67, 45), (131, 43)):
        assert (w + 63) // 64 == {67: 2, 131: 3}[w] and h % 4, "two / three 64-column blocks, a height that is no multiple of 4"


def _noise_proof(c, r):
    _table_proof(c, r)
    w, h = size_of(c["image"])
    lv = r["levels"]
    for e in lv:
        for q in PLANE_NAMES:
            assert e[q] is None or np.isfinite(e[q]).all()
    if (w, h) == (163, 83) and c["thr"] < 1e-5:
        l0 = range(4)
        edges = dict(row1=_on(r, l0, row=1), rowh2=_on(r, l0, row=h - 2), col1=_on(r, l0, col=1), colw2=_on(r, l0, col=w - 2),
                     col64=_on(r, l0, col=64), col65=_on(r, l0, col=65))
        assert all(v >= 1 for v in edges.values()), edges
        assert _on(r, range(4, 8), col=64) >= 1 and _on(r, range(4, 8), col=65) >= 1, "the chunk seam in octave 1 too"
        assert all(below_floor(e["Ldet"], c["thr"]) >= 1 for e in lv), "every level: maxima only the 1e-5 floor excludes"
    if (w, h) == (163, 83) and c["thr"] >= 1e-4:
        assert r["counts"][:4].all() and not r["counts"][4:].any(), ("the upper octave is empty", r["counts"].tolist())
    if c["thr"] < 1e-5:
        assert r["counts"].all()


def _scene_proof(c, r):
    _table_proof(c, r)
    per_octave = r["counts"].reshape(-1, 4).sum(1)
    assert per_octave.all(), ("candidates in every octave", per_octave.tolist())


def modulus(name):
    """the sigma-1 Scharr modulus over the interior, as kcontrast_parts forms it"""
    O = R._oracle()
    lx, ly = O.akaze_scharr(O.akaze_gaussian(image(name), 1.0))
    lx, ly = lx[1:-1, 1:-1], ly[1:-1, 1:-1]
    return np.sqrt(lx * lx + ly * ly)


def kscan(hist, npoints):
    """compute_k_percentile's scan over a histogram: the k it stops at (bins 0 .. k - 1 were added), or None if it runs out"""
    nthr = int(F(F(npoints) * R.KPERC))
    nel, k = 0, 0
    while nel < nthr and k < NBINS:
        nel += int(hist[k]); k += 1
    return None if nel < nthr else k


def subnormals(P):
    return int(((P != 0) & (np.abs(P) < TINY)).sum())


def _steps_proof(c, r):
    m = modulus(c["image"])
    zeros = int((m == 0).sum())
    assert zeros > m.size // 4 and m.size - zeros > m.size // 4, ("an exactly zero modulus on part of the interior", zeros, m.size)
    assert int(r["hist"].sum()) == m.size - zeros, "a zero modulus is not counted"
    k = kscan(r["hist"], m.size - zeros)
    with_zeros = r["hist"].astype(np.int64).copy(); with_zeros[0] += zeros
    k0 = kscan(with_zeros, m.size)
    assert k is not None and k0 is not None and k != k0, ("counting zeros would move the percentile", k, k0)
    assert r["k"] == F(r["hmax"] * F(F(k) / F(NBINS))) and r["k"] != F(r["hmax"] * F(F(k0) / F(NBINS)))
    # recorded: the flat parts are exact zeros, the reference holds no subnormal on this image
    assert sum(subnormals(e["Lt"]) + subnormals(e["Ldet"]) for e in r["levels"]) == 0


def _faint_proof(c, r):
    for i, e in enumerate(r["levels"]):
        assert subnormals(e["Ldet"]) >= 1, ("non-zero subnormals in Ldet", i)
        for q in ("Lsmooth", "Lt", "Lx", "Ly"):                              # beside normal values: what Ldet is formed from
            assert int((np.abs(e[q]) >= TINY).sum()) >= 1 and subnormals(e[q]) == 0, (i, q)
    assert 1e-19 < float(r["k"]) < 2e-18 and np.isfinite(r["inv_k2"]).all() and (r["inv_k2"] > 1e35).all(), (r["k"], r["inv_k2"])
    assert not r["counts"].any()


def _ramp_proof(c, r):
    n = int(r["hist"].sum())
    assert n > 0 and int(r["hist"][NBINS - 1]) > 0.9 * n, ("the counted moduli sit in the last bin", r["hist"][NBINS - 1], n)
    assert kscan(r["hist"], n) == NBINS and int(r["hist"][:NBINS - 1].sum()) < int(F(F(n) * R.KPERC)), "the percentile is met by the last bin alone"
    assert r["k"] == r["hmax"] != F(0.03)


def _pixel_proof(c, r):
    m = modulus(c["image"])
    ys, xs = np.nonzero(m)
    h, w = image(c["image"]).shape
    assert 0 < len(ys) <= 81 and np.all(np.abs(ys + 1 - h // 2) <= 4) and np.all(np.abs(xs + 1 - w // 2) <= 4), "one non-zero neighbourhood"
    assert int(r["hist"].sum()) == len(ys) and int(r["hist"][NBINS - 1]) >= 1, "only it is counted; its maximum lands in bin 299"
    k = kscan(r["hist"], len(ys))
    assert k is not None and 1 < k < NBINS and r["k"] == F(r["hmax"] * F(F(k) / F(NBINS)))


def _flat_proof(c, r):
    assert r["hmax"] == 0 and not r["hist"].any() and r["k"] == 0 and np.isinf(r["inv_k2"]).all(), "k = 0"
    lv = r["levels"]
    assert len(lv) >= 8
    assert all(np.isfinite(lv[0][q]).all() for q in PLANE_NAMES if lv[0][q] is not None)
    for i, e in enumerate(lv[1:], 1):
        assert np.isnan(e["Lflow"]).all() and np.isnan(e["Lt"]).all(), ("NaN conductivity from level 1 on", i)
    assert not r["counts"].any()


# ------------------------------------------------------------------------------------------------ planted determinant planes
TABLES = ((66, 45), (67, 45), (130, 45), (131, 45), (67, 300))


def blank_planes(size, seed):
    rng = np.random.default_rng(seed)
    lv = R.levels(*size)
    assert len(lv) == 4 and all((e["w"], e["h"]) == size for e in lv)
    return [(rng.uniform(-1, 1, (size[1], size[0])) * 1e-6).astype(F) for _ in lv]


def planted(size, seed, name, thr=PTHR):
    return dict(name=name, family="planted", kind="planes", size=size, planes=blank_planes(size, seed), thr=thr, want=[])


def plant(case, level, col, row, value, listed):
    """writes a determinant value; listed: the plan says it is a candidate"""
    case["planes"][level][row, col] = F(value)
    if listed:
        case["want"].append((level, row, col, F(value)))


def _want_proof(c, r):
    """the reference's list is the list the case was built to give, in scan order"""
    want = sorted(c["want"], key=lambda t: t[:3])
    got = list(zip(r["level"].tolist(), r["y"].tolist(), r["x"].tolist(), r["value"].tolist()))
    assert got == [(l, y, x, float(v)) for l, y, x, v in want], (c["name"], got[:8], want[:8])
    assert r["counts"].tolist() == [sum(t[0] == i for t in want) for i in range(4)]
    if c.get("extra"):
        c["extra"](c, r)


def _seams(size):
    w, h = size
    cols = sorted({x for x in (1, 63, 64, 65, 66, w - 2) if 1 <= x <= w - 2})
    odd, even = [x for x in cols if x % 2], [x for x in cols if not x % 2]      # no two neighbours in one group: isolated maxima
    c = planted(size, 10 + w, f"seams-{w}x{h}")
    k = 0
    for level, (first, last) in enumerate(((odd, even), (even, odd), (cols[::2], cols[1::2]), (cols[1::2], cols[::2]))):
        for row, group in ((1, first), (h - 2, last)):
            for x in group:
                plant(c, level, x, row, 0.01 + k / 1024, True); k += 1

    def extra(c, r):
        for x in cols:
            assert _on(r, range(4), col=x, row=1) >= 1 and _on(r, range(4), col=x, row=h - 2) >= 1, ("on the first and the last row", x)
        lane, chunk = (w - 2 - 1) % 64, (w - 2 - 1) // 64
        if w == 66:
            assert (chunk, lane) == (0, 63), "w - 2 is the last lane of the first chunk"
        if w in (67, 131):
            assert lane == 0 and chunk == (w - 3) // 64 and w - 2 - (1 + 64 * chunk) == 0, "w - 2 is a chunk of one lane"
    c["extra"] = extra
    return c


NEIGHBOURS = [(-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1)]


def _ties():
    size = (67, 45)
    w, h = size
    v = F(0.0123); up = np.nextafter(v, F(1))
    c = planted(size, 21, "ties")
    # level 0: the centre equals one neighbour (all eight directions, so horizontal, vertical and both diagonals, either order)
    for k, (dx, dy) in enumerate(NEIGHBOURS):
        plant(c, 0, 6 + 7 * k, 10, v, False); plant(c, 0, 6 + 7 * k + dx, 10 + dy, v, False)
    # level 1: a would-be maximum equals a pixel of the outer ring
    for col, row, rc, rr in ((10, 1, 10, 0), (20, 1, 21, 0), (1, 10, 0, 10), (1, 20, 0, 21), (30, h - 2, 30, h - 1), (40, h - 2, 39, h - 1),
                             (w - 2, 10, w - 1, 10), (w - 2, 20, w - 1, 19), (1, 1, 0, 0), (w - 2, h - 2, w - 1, h - 1)):
        plant(c, 1, col, row, v, False); c["planes"][1][rr, rc] = v
    # level 2: a larger value on the outer ring suppresses its neighbour and is never listed
    for col, row, rc, rr in ((10, 1, 10, 0), (1, 10, 0, 11), (30, h - 2, 31, h - 1), (w - 2, 20, w - 1, 20), (w - 2, 1, w - 1, 0)):
        plant(c, 2, col, row, v, False); c["planes"][2][rr, rc] = F(2) * v
    # level 3: one ulp above eight equal neighbours is a maximum, a 3 x 3 plateau has none; a maximum beside the ring stays one
    c["planes"][3][9:12, 9:12] = v; plant(c, 3, 10, 10, up, True)
    c["planes"][3][19:22, 19:22] = v
    plant(c, 3, 30, 1, v, True); plant(c, 3, 1, 30, v, True)

    def extra(c, r):
        P = c["planes"]
        assert all(P[0][10, 6 + 7 * k] == P[0][10 + dy, 6 + 7 * k + dx] == v for k, (dx, dy) in enumerate(NEIGHBOURS))
        assert r["counts"].tolist() == [0, 0, 0, 3] and up > v
    c["extra"] = extra
    return c


def _thresholds():
    size = (67, 45)
    a = planted(size, 22, "thresholds-0.001")
    plant(a, 0, 10, 10, PTHR, False); plant(a, 0, 20, 10, np.nextafter(PTHR, F(1)), True)
    plant(a, 3, 10, 1, PTHR, False); plant(a, 3, 65, 43, np.nextafter(PTHR, F(1)), True)
    b = planted(size, 23, "thresholds-1e-07", thr=F(1e-7))
    plant(b, 0, 10, 10, FLOOR, True); plant(b, 0, 20, 10, np.nextafter(FLOOR, F(0)), False)
    plant(b, 1, 10, 10, F(1e-7), False); plant(b, 1, 20, 10, np.nextafter(F(1e-7), F(1)), False)        # over the threshold, under the floor
    plant(b, 2, 64, 1, FLOOR, True); plant(b, 2, 65, 43, np.nextafter(FLOOR, F(0)), False)

    def extra(c, r):
        assert FLOOR == F(0.00001) and np.nextafter(FLOOR, F(0)) > c["thr"]
        assert below_floor(c["planes"][0], c["thr"]) >= 1 and below_floor(c["planes"][1], c["thr"]) >= 1
    b["extra"] = extra
    return [a, b]


def _nonfinite():
    size = (67, 45)
    v = F(0.02)
    c = planted(size, 24, "nonfinite_neighbours")
    for k, (dx, dy) in enumerate(NEIGHBOURS):
        plant(c, 0, 6 + 7 * k, 10, v, False); c["planes"][0][10 + dy, 6 + 7 * k + dx] = np.nan
        plant(c, 1, 6 + 7 * k, 10, v, True); c["planes"][1][10 + dy, 6 + 7 * k + dx] = -np.inf
    # +inf: on the outer ring, and as a pair in the interior (neither of the pair is over the other); every neighbour is suppressed
    plant(c, 2, 10, 1, v, False); c["planes"][2][0, 11] = np.inf
    plant(c, 2, 30, 20, v, False); c["planes"][2][20, 31] = np.inf; c["planes"][2][20, 32] = np.inf; plant(c, 2, 33, 21, v, False)
    plant(c, 3, 1, 43, v, True); c["planes"][3][44, 0] = -np.inf; plant(c, 3, 10, 43, v, False); c["planes"][3][44, 11] = np.nan

    def extra(c, r):
        assert np.isfinite(r["value"]).all(), "centres stay finite"
        assert sum(int((~np.isfinite(P)).sum()) for P in c["planes"]) == 8 + 8 + 3 + 2
    c["extra"] = extra
    return c


def _dense(size):
    w, h = size
    c = planted(size, 30 + w + h, f"dense-{w}x{h}")
    k = 0
    for level in range(4):
        for row in range(1, h - 1, 2):
            for col in range(1, w - 1, 2):
                plant(c, level, col, row, 0.01 + (k * 7919 % 65536) / 65536, True); k += 1

    def extra(c, r):
        assert r["counts"].tolist() == [((w - 1) // 2) * ((h - 1) // 2)] * 4, "the largest count a plane can hold"
        assert len(set(r["value"].tolist())) > 0.9 * len(r["value"])
        if h == 300:
            cat = r["level"].astype(np.int64) * h + r["y"]
            assert cat.min() < 1024 <= cat.max() and 4 * h == 1200, "the concatenated row index crosses 1024: the scan carries over its chunk"
    c["extra"] = extra
    return c


def _scan_chunk():
    size = (67, 300)
    c = planted(size, 40, "scan_chunk")
    k = 0
    for row in (122, 123, 124, 125):
        for col in range(3 + 5 * (row - 122), 64, 20):
            plant(c, 3, col, row, 0.01 + k / 1024, True); k += 1

    def extra(c, r):
        cat = r["level"].astype(np.int64) * 300 + r["y"]
        assert sorted(set(cat.tolist())) == [1022, 1023, 1024, 1025] and not r["counts"][:3].any()
    c["extra"] = extra
    return c


def empty_planes(size):
    c = planted(size, 99, f"empty-{size[0]}x{size[1]}")
    c["proof"] = _want_proof
    return c


# ------------------------------------------------------------------------------------------------ the table
def all_cases():
    global _ALL
    if _ALL is None:
        out = []
        img = lambda fam, kind, w, h, thr, proof: out.append(dict(name=f"{kind}-{w}x{h}-{thr:g}", family=fam, kind="image",   # noqa: E731
                                                                   image=f"{kind}-{w}x{h}", thr=thr, proof=proof))
        for w, h in ((67, 45), (131, 43), (160, 80)):
            img("noise", "noise", w, h, 1e-7, _noise_proof)
        img("noise", "noise", 163, 83, 1e-7, _noise_proof); img("noise", "noise", 163, 83, 1e-3, _noise_proof)
        img("scene", "scene", 321, 161, 1e-3, _scene_proof); img("scene", "scene", 640, 320, 1e-3, _scene_proof)
        img("kcontrast", "steps", 163, 83, 1e-3, _steps_proof); img("kcontrast", "faint", 67, 45, 1e-7, _faint_proof)
        img("kcontrast", "ramp", 160, 80, 1e-3, _ramp_proof); img("kcontrast", "pixel", 160, 80, 1e-3, _pixel_proof)
        img("kcontrast", "flat", 160, 80, 1e-3, _flat_proof)
        pl = [_seams(s) for s in TABLES[:4]] + [_ties()] + _thresholds() + [_nonfinite()] + [_dense((131, 45)), _dense((67, 300)), _scan_chunk()]
        for c in pl:
            c["proof"] = _want_proof
        out += pl
        assert len({c["name"] for c in out}) == len(out)
        _ALL = out
    return _ALL


FAMILIES = ("noise", "scene", "kcontrast", "planted")


def batches():
    """the B = 3 calls, the flat image (planes without a candidate) in the middle: (name, family, kind, thr, [three image names or
    planted cases]).  Per family and image size (table) the cases go in pairs, the last one with the first when the number is odd, so
    that the two outer totals differ from the middle's and mostly from each other: the candidate stride is another image's."""
    out = []
    for fam in FAMILIES:
        groups = {}
        for c in all_cases():
            if c["family"] != fam or (c["kind"] == "image" and c["image"].startswith("flat")):
                continue
            key = size_of(c["image"]) if c["kind"] == "image" else c["size"]
            groups.setdefault((key, float(c["thr"])), []).append(c)
        for (size, thr), cs in groups.items():
            for k in range(0, len(cs), 2):
                a, b = cs[k], cs[k + 1] if k + 1 < len(cs) else cs[0]
                name = f"{fam}-batch-{size[0]}x{size[1]}-{thr:g}-{k // 2}"
                if a["kind"] == "image":
                    out.append((name, fam, "image", a["thr"], [a["image"], f"flat-{size[0]}x{size[1]}", b["image"]]))
                else:
                    out.append((name, fam, "planes", a["thr"], [a, empty_planes(size), b]))
    return out


# ------------------------------------------------------------------------------------------------ the GPU child
def child_main(family, out_path):
    """runs in a child process of the GPU test (the session's process holds the product library): loads the developer library and runs,
    through r3dm_dev_akaze_classic_head / r3dm_dev_akaze_classic_extrema, every case of the family in a call of its own, then the
    family's batches, and pickles {key: per-image results, "__seconds__": wall time}.  Stops at the first error: the file then holds
    {"__error__": text} beside the results so far."""
    import pickle
    import time
    from regard3d_amd import api
    api.use_developer_library()
    res = {}
    t0 = time.perf_counter()

    def run(ctx, kind, thr, items):
        if kind == "image":
            return ctx.dev_akaze_classic_head([image(n) for n in items], thr)
        return ctx.dev_akaze_classic_extrema(items[0]["size"][0], items[0]["size"][1], [c["planes"] for c in items], thr)
    try:
        ctx = api.Context(0)
        for c in all_cases():
            if c["family"] == family:
                res[("single", c["name"])] = run(ctx, c["kind"], c["thr"], [c["image"] if c["kind"] == "image" else c])
        for name, fam, kind, thr, items in batches():
            if fam == family:
                res[("batch", name)] = run(ctx, kind, thr, items)
        ctx.close()
    except Exception as e:                        # (reported to the parent, which decides; nothing more runs on the GPU here)
        res["__error__"] = f"{type(e).__name__}: {e}"
    res["__seconds__"] = time.perf_counter() - t0
    pickle.dump(res, open(out_path, "wb"), protocol=pickle.HIGHEST_PROTOCOL)
    return 3 if "__error__" in res else 0
