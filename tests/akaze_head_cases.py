"""Images and determinant planes built for the edges of the Fast-A-KAZE head -- the scale space (Gaussians, k-contrast, half-sampling,
scaled derivatives, determinant, conductivity, FED launches), the extremum pass and the in-level pruning.  Shared
by tests/test_akaze_head_cases.py (CPU: every case reaches the edge it is named for, shown on the reference and on the product's launch
plan alone) and tests/test_gpu_akaze_head.py (GPU: the developer build's r3dm_dev_akaze_head / r3dm_dev_akaze_extrema run the product's
launches on the same inputs, every pixel of every plane and every list entry bit for bit against the reference).

The reference is oracle/akaze.c's orc_akaze_head and orc_akaze_extrema, the serial code the oracle's detector itself runs.  A case is
dict(name, family, kind, proof[, plan_proof]):
  kind "image":  image (a name in images()), thr; reference(case) = orc_akaze_head; proof(case, ref) asserts on the reference that the
                 edge is reached, plan_proof(case, plan) on the launch plan the product reports for the image's size;
  kind "planes": planes [n_levels] Ldet of the 187 x 123 table -- seeded values far below the threshold with the engineered values
                 written over them -- and thr; reference(case) = orc_akaze_extrema per level."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import pyoracle as O  # noqa: E402

F = np.float32
NBINS = 300
PW, PH = 187, 123                                  # the table of the planted planes
PTHR = F(1e-3)
_IMAGES, _REF, _ALL = {}, {}, None


def _assert(cond, *what):
    assert cond, what


def levels(w, h):
    return O.akaze_levels(w, h)


# ------------------------------------------------------------------------------------------------ the images
def _scene(h, w, seed):
    """smooth blobs on a slow wave, a little noise (the scenes of tests/test_gpu_akaze.py)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = 0.5 + 0.1 * np.sin(xx / 17.0) * np.cos(yy / 23.0)
    for _ in range(max(4, h * w // 2000)):
        mg = min(40, h // 4)
        cx, cy = rng.uniform(mg, w - mg), rng.uniform(mg, h - mg)
        s = rng.uniform(2, 12); a = rng.uniform(0.15, 0.45) * rng.choice([-1, 1])
        th = rng.uniform(0, np.pi); e = rng.uniform(1.0, 2.5)
        u = (xx - cx) * np.cos(th) + (yy - cy) * np.sin(th); v = -(xx - cx) * np.sin(th) + (yy - cy) * np.cos(th)
        img = img + a * np.exp(-(u * u / (2 * s * s * e) + v * v / (2 * s * s / e)))
    img = img + rng.normal(0, 0.01, img.shape)
    return np.clip(img, 0, 1).astype(F)


def _make_image(name):
    kind, size = name.split("-")
    w, h = (int(v) for v in size.split("x"))
    if kind == "noise":
        return np.random.default_rng(1000 * w + h).uniform(0, 1, (h, w)).astype(F)
    if kind == "scene":
        return _scene(h, w, 7000 * w + h)
    if kind == "flat":
        return np.full((h, w), F(0.5))
    if kind == "stripes":
        img = np.empty((h, w), F)
        img[:, :] = np.where((np.arange(w) + 2) % 3 == 0, F(0.25), F(0.75))[None, :]
        return img
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


def reference(case):
    """the oracle's outputs of a case, computed once per process and shared by every test that needs them"""
    if case["kind"] == "image":
        return head_reference(case["image"], case["thr"])
    if case["name"] not in _REF:
        lv = levels(PW, PH)
        out = [O.akaze_extrema(P, e["border"], e["ratio"], e["psize"], case["thr"]) for P, e in zip(case["planes"], lv)]
        _REF[case["name"]] = dict(n_cand=np.array([o[0] for o in out], np.uint32), lists=[o[1] for o in out])
    return _REF[case["name"]]


def head_reference(name, thr):
    key = (name, float(thr))
    if key not in _REF:
        _REF[key] = O.akaze_head(image(name), thr)
    return _REF[key]


# ------------------------------------------------------------------------------------------------ proofs on the reference
def kscan(ref, total):
    """compute_k_percentileV2's scan over the reference's own histogram -> (nthreshold, the bin the loop breaks at or None)"""
    hist = ref["hist"]
    nthr = int(F(total - int(hist[0])) * F(0.7))
    nel = 0
    for k in range(1, NBINS):
        if nel >= nthr:
            return nthr, k
        nel += int(hist[k])
    return nthr, None


def _inv_k2(k):
    out = []
    k = F(k)
    for _ in range(8):
        out.append(F(1) / F(k * k)); k = F(k * F(0.75))
    return np.array(out, F)


def _interior(e):
    return e["w"] - 2 * e["border"], e["h"] - 2 * e["border"]


def _on_edges(ref):
    """per edge of the interior (first row, last row, first column, last column): the levels with a kept point on it"""
    hit = {k: [] for k in ("first_row", "last_row", "first_col", "last_col")}
    for i, (e, l) in enumerate(zip(ref["levels"], ref["lists"])):
        col, row = l[:, 0] / F(e["ratio"]), l[:, 1] / F(e["ratio"])
        if np.any(row == e["border"]): hit["first_row"].append(i)
        if np.any(row == e["h"] - e["border"] - 1): hit["last_row"].append(i)
        if np.any(col == e["border"]): hit["first_col"].append(i)
        if np.any(col == e["w"] - e["border"] - 1): hit["last_col"].append(i)
    return hit


def _textured(c, r):
    total = (r["levels"][0]["w"] - 2) * (r["levels"][0]["h"] - 2)
    if len(r["levels"]) > 1:
        nthr, k = kscan(r, total)
        assert r["hmax"] > 0 and k is not None and 1 < k < NBINS - 1 and r["kcontrast"] == F(F(r["hmax"] * F(k)) / F(NBINS)), "the percentile, met inside the histogram"
        assert int(r["hist"].sum()) == total
    else:
        assert r["hmax"] == 0 and not r["hist"].any() and r["kcontrast"] == F(0.03), "one level: no histogram is formed"
    assert np.array_equal(r["inv_k2"], _inv_k2(r["kcontrast"]))
    for i, (e, pl) in enumerate(zip(r["levels"], r["planes"])):
        for q, P in enumerate(pl):
            assert np.isfinite(P).all() and len(np.unique(P)) > P.size // 4, ("a textured plane", i, q)
    assert all(n >= len(l) for n, l in zip(r["n_cand"], r["lists"]))
    if c["thr"] < 1e-5 and c["image"].startswith("noise") and len(r["levels"]) > 1:
        assert any(n > len(l) > 0 for n, l in zip(r["n_cand"], r["lists"])), "the pruning drops candidates on some level"


def _size_proof(w, h):
    def proof(c, r):
        _textured(c, r)
        lv = r["levels"]
        if (w, h) == (163, 121):
            assert len(lv) == 5 and (lv[4]["w"], lv[4]["h"]) == (81, 60) and lv[3]["w"] % 2 == 1 and lv[3]["h"] % 2 == 1, "odd to odd: the area path"
            assert _interior(lv[0]) == (105, 63)
        if (w, h) == (187, 123):
            iw, ih = _interior(lv[0])
            assert (iw, ih) == (129, 65) and (iw + 63) // 64 == 3 and iw - 128 == 1 and ih - 64 == 1, "three mask words, one valid column in the last; a second tile of one row"
            if c["image"].startswith("noise") and c["thr"] < 1e-5:
                hit = _on_edges(r)
                assert all(0 in v for v in hit.values()), ("a kept point on every edge of level 0's interior", hit)
        if (w, h) == (160, 120):
            assert len(lv) == 5 and lv[4]["w"] * 2 == lv[3]["w"] and lv[4]["h"] * 2 == lv[3]["h"], "even to half: the fast path"
        if (w, h) == (327, 245):
            assert len(lv) == 9 and [e["octave"] for e in lv] == [0, 0, 0, 0, 1, 1, 1, 1, 2]
            assert (lv[4]["w"], lv[4]["h"]) == (163, 122) and (lv[8]["w"], lv[8]["h"]) == (81, 61)
        if (w, h) in ((60, 90), (61, 61)):
            assert len(lv) == 1
        if c["image"].startswith("noise") and c["thr"] < 1e-5 and (w, h) in ((163, 121), (187, 123)):
            assert all(v for v in _on_edges(r).values()), ("a kept point on every edge of some level's interior", _on_edges(r))
    return proof


def strips(plan, lv):
    """per marching launch of the plan: (level, stored columns per strip, rows per band)"""
    return [(i, 64 - 2 * steps, rows) for i, p in enumerate(plan) for form, steps, rows in p["launches"] if form == 2]


def _size_plan_proof(w, h):
    def plan_proof(c, plan):
        lv = levels(w, h)
        assert len(plan) == len(lv) and not plan[0]["launches"]
        assert all(p["launches"] and sum(s for _, s, _ in p["launches"]) == p["n_steps"] for p in plan[1:])
        assert all(form == 2 and not p["head_form"] for p in plan for form, _, _ in p["launches"]), "the product: marching strips, four launches"
        if (w, h) == (327, 245):
            assert [[s for _, s, _ in p["launches"]] for p in plan[1:]] == [[3], [3], [4], [4], [5], [6], [3, 4], [4, 4]]
            assert sorted({64 - 2 * s for _, s, _ in sum((p["launches"] for p in plan), [])}) == [52, 54, 56, 58]
    return plan_proof


SEAM_SIZES = ((174, 128), (175, 129), (173, 127))     # 3 x 58 columns and 8 x 16 rows at levels 1 and 2: exactly, one more, one less


def _seam_plan_proof(w, h):
    def plan_proof(c, plan):
        lv = levels(w, h)
        off = {(174, 128): 0, (175, 129): 1, (173, 127): -1}[(w, h)]
        cols = [(i, vw) for i, vw, rows in strips(plan, lv) if (lv[i]["w"] - off) % vw == 0]
        rws = [(i, rows) for i, vw, rows in strips(plan, lv) if (lv[i]["h"] - off) % rows == 0]
        assert cols and rws, ("the level's width and height are a multiple of the strip and of the band", off, cols, rws)
        assert all(lv[i]["w"] > vw and lv[i]["h"] > rows for i, vw in cols for _, rows in rws), "more than one strip and band"
    return plan_proof


# ------------------------------------------------------------------------------------------------ the k-contrast
def _flat_proof(c, r):
    assert len(r["levels"]) > 1 and r["hmax"] == 0 and not r["hist"].any() and r["kcontrast"] == F(0.03), "hmax == 0: the default"
    assert np.array_equal(r["inv_k2"], _inv_k2(0.03))
    assert all(not len(l) for l in r["lists"]) and not r["n_cand"].any()
    for pl in r["planes"]:
        assert np.all(pl[3] == pl[3][0, 0]) and not pl[0].any(), "a flat Lt, a zero determinant"


def _stripes_proof(c, r):
    total = 160 * 118
    nthr, k = kscan(r, total)
    assert r["hmax"] > 0 and k is None and r["kcontrast"] == F(0.03), "the scan ends without a break: the default, with a non-zero maximum"
    assert int(r["hist"][1:NBINS - 1].sum()) < nthr <= int(r["hist"][1:].sum()), (nthr, r["hist"][NBINS - 1])
    assert np.array_equal(r["inv_k2"], _inv_k2(0.03))


def _ramp_proof(c, r):
    total = 158 * 118
    nthr, k = kscan(r, total)
    assert k == NBINS - 1, ("the percentile is met only when the last bin is reached", k)
    assert r["kcontrast"] == F(F(r["hmax"] * F(NBINS - 1)) / F(NBINS)) and r["kcontrast"] != F(0.03)
    assert np.array_equal(r["inv_k2"], _inv_k2(r["kcontrast"]))


def _pixel_proof(c, r):
    total = 158 * 118
    nthr, k = kscan(r, total)
    assert r["hist"][0] > 0.99 * total and 0 < nthr < 100 and k is not None and 1 < k < NBINS - 1, (r["hist"][0], nthr, k)
    assert nthr == int(F(total - int(r["hist"][0])) * F(0.7)) and r["kcontrast"] == F(F(r["hmax"] * F(k)) / F(NBINS))


# ------------------------------------------------------------------------------------------------ planted determinant planes
def blank_planes(seed):
    rng = np.random.default_rng(seed)
    return [(rng.uniform(-1, 1, (e["h"], e["w"])) * 1e-5).astype(F) for e in levels(PW, PH)]


def plant(case, level, col, row, value, tag=None):
    """writes a determinant value at a level position inside the interior"""
    e = levels(PW, PH)[level]
    assert e["border"] <= col < e["w"] - e["border"] and e["border"] <= row < e["h"] - e["border"], (level, col, row)
    case["planes"][level][row, col] = F(value)
    if tag:
        case["tags"][tag] = (level, col, row)


def planted(seed, name, proof):
    return dict(name=name, family="planted", kind="planes", planes=blank_planes(seed), thr=PTHR, proof=proof, tags={})


def triple(level, col, row, value):
    """the list entry of a kept point"""
    r = F(levels(PW, PH)[level]["ratio"])
    return (F(F(col) * r), F(F(row) * r), F(value))


def _is_list(ref, level, want):
    got = ref["lists"][level]
    want = np.array(want, F).reshape(-1, 3)
    assert got.shape == want.shape and got.tobytes() == want.tobytes(), (level, got.tolist(), want.tolist())


def _corners_and_seams():
    lv = levels(PW, PH)
    e0, e4 = lv[0], lv[4]
    b, x1, y1 = e0["border"], e0["w"] - e0["border"] - 1, e0["h"] - e0["border"] - 1
    spots0 = [(b, b), (x1, b), (b + 63, b + 6), (b + 64, b + 9), (b + 127, b + 6), (b + 128, b + 9), (60, b + 15), (70, b + 16), (b + 63, b + 15),
              (b + 67, b + 16), (60, b + 63), (70, b + 64), (b, y1), (b + 64, y1 - 3), (b + 63, y1), (x1, y1)]
    spots4 = [(e4["border"], e4["border"]), (e4["w"] - e4["border"] - 1, e4["border"]), (e4["border"], e4["h"] - e4["border"] - 1),
              (e4["w"] - e4["border"] - 1, e4["h"] - e4["border"] - 1)]

    def proof(c, r):
        assert _interior(e0) == (129, 65) and _interior(e4) == (35, 3)
        words = {((col - b) // 64, (col - b) % 64) for col, _ in spots0}
        assert {(0, 0), (0, 63), (1, 0), (1, 63), (2, 0)} <= words, "the first and last bit of a full mask word, the one bit of the last word"
        rows = {row - b for _, row in spots0}
        assert {0, 15, 16, 63, 64} <= rows, "the first and last row of a wave and of a tile, the one row of the second tile"
        order = sorted(range(len(spots0)), key=lambda k: (spots0[k][1], spots0[k][0]))
        _is_list(r, 0, [triple(0, *spots0[k], 0.01 + k / 1024) for k in order])
        # level 4: an interior of three rows, ratio 2 -- its corners of one column lie 4 apart, within psize 4.8: the later, larger
        # ones take the earlier ones' slots
        _is_list(r, 4, [triple(4, *spots4[k], 0.02 + k / 1024) for k in (2, 3)])
        assert r["n_cand"].tolist() == [len(spots0), 0, 0, 0, 4] and r["lists"][4][1, 0] == 2 * spots4[3][0], "level 4: positions times the ratio"
    c = planted(1, "corners_and_seams", proof)
    for k, (col, row) in enumerate(spots0):
        plant(c, 0, col, row, 0.01 + k / 1024)
    for k, (col, row) in enumerate(spots4):
        plant(c, 4, col, row, 0.02 + k / 1024)
    return c


NEIGHBOURS = [(-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1)]


def _threshold_and_ties():
    v = F(0.0123); up = np.nextafter(v, F(1)); thr_up = np.nextafter(PTHR, F(1))

    def proof(c, r):
        P = c["planes"][0]
        assert P[35, 40] == PTHR and P[35, 50] == thr_up and thr_up > PTHR
        for k, (dx, dy) in enumerate(NEIGHBOURS):
            assert P[45, 40 + 10 * k] == v == P[45 + dy, 40 + 10 * k + dx], "the centre equals one neighbour"
        assert P[55, 50] == up and np.all(np.delete(P[54:57, 49:52].ravel(), 4) == v), "one ulp above all eight neighbours"
        assert np.all(P[64:67, 49:52] == v), "a 3 x 3 plateau"
        _is_list(r, 0, [triple(0, 50, 35, thr_up), triple(0, 50, 55, up)])
        assert r["n_cand"].tolist() == [2, 0, 0, 0, 0], "the threshold itself, a tie with any neighbour and the plateau are no extrema"
    c = planted(2, "threshold_and_ties", proof)
    plant(c, 0, 40, 35, PTHR); plant(c, 0, 50, 35, thr_up)
    for k, (dx, dy) in enumerate(NEIGHBOURS):
        plant(c, 0, 40 + 10 * k, 45, v); plant(c, 0, 40 + 10 * k + dx, 45 + dy, v)
    c["planes"][0][54:57, 49:52] = v; plant(c, 0, 50, 55, up)
    c["planes"][0][64:67, 49:52] = v
    return c


def _d2(level, a, b):
    """squared distance of two level positions as the pruning forms it"""
    (ax, ay, _), (bx, by, _) = triple(level, a[0], a[1], 0), triple(level, b[0], b[1], 0)
    dx, dy = F(ax - bx), F(ay - by)
    return F(dx * dx + dy * dy)


def _r2(level):
    p = F(levels(PW, PH)[level]["psize"])
    return F(p * p)


def _pruning_chains():
    def proof(c, r):
        r0, r1, r4 = _r2(0), _r2(1), _r2(4)
        # A, B, C on a row, 2 apart: B in A's radius, C in B's but not in A's
        assert _d2(0, (40, 31), (42, 31)) <= r0 < _d2(0, (40, 31), (44, 31))
        want = [triple(0, 40, 31, 0.3), triple(0, 44, 31, 0.1)]              # B weaker: dropped; C is no one's neighbour: appended
        want += [triple(0, 62, 31, 0.3)]                                    # B stronger: takes A's slot; C, weaker, in B's radius: dropped
        want += [triple(0, 80, 31, 0.2)]                                    # equal responses: the earlier stays
        # B replaces A in place; C, later, inside A's old radius but outside B's: appended.  D inside B's, outside A's: meets B, dropped
        assert _d2(0, (58, 37), (60, 36)) <= r0 < _d2(0, (58, 37), (62, 36)) and _d2(0, (104, 37), (102, 36)) <= r0 < _d2(0, (104, 37), (100, 36))
        want += [triple(0, 62, 36, 0.2), triple(0, 102, 36, 0.2), triple(0, 58, 37, 0.05)]
        # the radius itself: squared distances are integers times ratio^2 and psize^2 = 5.76 2^(k / 2) is none, so equality cannot be
        # planted; the nearest distances on either side are (level 1: 8 <= 8.146 < 9)
        assert all(float(_r2(i)) != round(float(_r2(i))) for i in range(5)), "no level's psize^2 is an integer"
        assert _d2(0, (40, 42), (42, 43)) == 5 <= r0 < 8 == _d2(0, (60, 42), (62, 44))
        want += [triple(0, 40, 42, 0.2), triple(0, 60, 42, 0.2), triple(0, 62, 44, 0.1)]
        got0 = r["lists"][0]
        assert got0[:len(want)].tobytes() == np.array(want, F).tobytes(), (got0[:len(want)].tolist(), want)
        assert _d2(1, (60, 50), (62, 52)) == 8 <= r1 < 9 == _d2(1, (90, 50), (93, 50))
        _is_list(r, 1, [triple(1, 60, 50, 0.2), triple(1, 90, 50, 0.2), triple(1, 93, 50, 0.1)])
        assert _d2(4, (40, 29), (42, 30)) == 20 <= r4 < 32 == _d2(4, (50, 29), (52, 31))
        _is_list(r, 4, [triple(4, 40, 29, 0.2), triple(4, 50, 29, 0.2), triple(4, 52, 31, 0.1)])
        # two components far apart, interleaved in raster order: X at columns 40 .. 41, Y at 120 .. 121, rows 70, 72, 74
        rest = got0[len(want):]
        tail = [triple(0, 41, 72, 0.3), triple(0, 120, 70, 0.3), triple(0, 120, 74, 0.2)]
        assert rest[-3:].tobytes() == np.array(tail, F).tobytes(), rest[-3:].tolist()
        # the long components: 20 candidates on row 50, 2 x 64 on rows 60 and 62, every one within 2 of the next
        mid = rest[:-3]
        n20, n128 = int((mid[:, 1] == 50).sum()), int((mid[:, 1] >= 60).sum())
        assert components(c, 0)[:2] == [128, 20], components(c, 0)
        assert 1 < n20 < 20 and 8 < n128 < 128 and n20 + n128 == len(mid), "both drop candidates; the larger keeps more slots alive than the live cap of 8"
        assert int(r["n_cand"][0]) == 24 + 20 + 128 and r["n_cand"].tolist()[1:] == [4, 0, 0, 4]
        assert np.any(np.diff(mid[n20:, 1]) < 0), "a candidate of row 62 took a slot of row 60 in place: list order is not raster order"
    c = planted(3, "pruning_chains", proof)
    plant(c, 0, 40, 31, 0.3); plant(c, 0, 42, 31, 0.2); plant(c, 0, 44, 31, 0.1)
    plant(c, 0, 60, 31, 0.1); plant(c, 0, 62, 31, 0.3); plant(c, 0, 64, 31, 0.2)
    plant(c, 0, 80, 31, 0.2); plant(c, 0, 82, 31, 0.2)
    plant(c, 0, 60, 36, 0.1); plant(c, 0, 62, 36, 0.2); plant(c, 0, 58, 37, 0.05)
    plant(c, 0, 100, 36, 0.1); plant(c, 0, 102, 36, 0.2); plant(c, 0, 104, 37, 0.05)
    plant(c, 0, 40, 42, 0.2); plant(c, 0, 42, 43, 0.1); plant(c, 0, 60, 42, 0.2); plant(c, 0, 62, 44, 0.1)
    rng = np.random.default_rng(33)
    resp = (rng.permutation(200)[:148] + 100).astype(F) / F(1024)
    for k in range(20):
        plant(c, 0, 40 + 2 * k, 50, resp[k])
    for k in range(64):
        plant(c, 0, 30 + 2 * k, 60, resp[20 + k]); plant(c, 0, 30 + 2 * k, 62, resp[84 + k])
    plant(c, 0, 40, 70, 0.1); plant(c, 0, 120, 70, 0.3); plant(c, 0, 41, 72, 0.3); plant(c, 0, 121, 72, 0.2); plant(c, 0, 40, 74, 0.2); plant(c, 0, 120, 74, 0.2)
    plant(c, 1, 60, 50, 0.2); plant(c, 1, 62, 52, 0.1); plant(c, 1, 90, 50, 0.2); plant(c, 1, 93, 50, 0.1)
    plant(c, 4, 40, 29, 0.2); plant(c, 4, 42, 30, 0.1); plant(c, 4, 50, 29, 0.2); plant(c, 4, 52, 31, 0.1)
    return c


def components(case, level):
    """sizes, largest first, of the components the candidates of a planted level form when every pair within psize is linked"""
    e = levels(PW, PH)[level]
    P = case["planes"][level]
    pts = [(x, y) for y in range(e["border"], e["h"] - e["border"]) for x in range(e["border"], e["w"] - e["border"]) if P[y, x] > case["thr"]]
    par = list(range(len(pts)))

    def find(a):
        while par[a] != a:
            par[a] = par[par[a]]; a = par[a]
        return a
    for a in range(len(pts)):
        for b in range(a):
            if _d2(level, pts[a], pts[b]) <= _r2(level):
                par[find(a)] = find(b)
    sizes = {}
    for a in range(len(pts)):
        sizes[find(a)] = sizes.get(find(a), 0) + 1
    return sorted(sizes.values(), reverse=True)


def empty_planes():
    return planted(99, "empty", lambda c, r: _assert(not r["n_cand"].any()))


# ------------------------------------------------------------------------------------------------ the table
SIZES = ((163, 121), (187, 123), (160, 120), (327, 245), (60, 90), (61, 61))
THRS = (1e-7, 1e-3)


def all_cases():
    global _ALL
    if _ALL is None:
        out = []
        for w, h in SIZES:
            for kind in ("noise", "scene"):
                for thr in THRS:
                    out.append(dict(name=f"{kind}-{w}x{h}-{thr:g}", family="sizes", kind="image", image=f"{kind}-{w}x{h}", thr=thr,
                                    proof=_size_proof(w, h), plan_proof=_size_plan_proof(w, h)))
        for w, h in SEAM_SIZES:
            for kind in ("noise", "scene"):
                out.append(dict(name=f"seam-{kind}-{w}x{h}", family="seams", kind="image", image=f"{kind}-{w}x{h}", thr=1e-7,
                                proof=lambda c, r: _textured(c, r), plan_proof=_seam_plan_proof(w, h)))
        for name, img, proof in (("flat", "flat-160x120", _flat_proof), ("stripes_default_with_a_maximum", "stripes-162x120", _stripes_proof),
                                 ("ramp_percentile_at_the_last_bin", "ramp-160x120", _ramp_proof), ("isolated_pixel", "pixel-160x120", _pixel_proof)):
            out.append(dict(name=name, family="kcontrast", kind="image", image=img, thr=1e-3, proof=proof, plan_proof=None))
        out += [_corners_and_seams(), _threshold_and_ties(), _pruning_chains()]
        assert len({c["name"] for c in out}) == len(out)
        _ALL = out
    return _ALL


FAMILIES = ("sizes", "seams", "kcontrast", "planted")


def size_of(name):
    w, h = (int(v) for v in name.split("-")[1].split("x"))
    return w, h


def batches():
    """the B = 3 calls, the flat image (the planes without a candidate) in the middle: (name, family, kind, thr, [three image names or
    planted cases]).  Per family and image size one call at the family's lower threshold, over the size's two images (twice the one when
    there is only one)."""
    out = []
    for fam in FAMILIES[:3]:
        by_size = {}
        for c in all_cases():
            if c["family"] == fam and not c["image"].startswith("flat") and c["image"] not in by_size.setdefault(size_of(c["image"]), []):
                by_size[size_of(c["image"])].append(c["image"])
        thr = 1e-3 if fam == "kcontrast" else 1e-7
        for (w, h), names in by_size.items():
            out.append((f"{fam}-batch-{w}x{h}", fam, "image", thr, [names[0], f"flat-{w}x{h}", names[-1]]))
    pl = [c for c in all_cases() if c["family"] == "planted"]
    out.append(("planted-batch-0", "planted", "planes", PTHR, [pl[0], empty_planes(), pl[1]]))
    out.append(("planted-batch-1", "planted", "planes", PTHR, [pl[2], empty_planes(), pl[0]]))
    return out


# the developer build's launch forms, one process each (the knobs are read once per process): environment, what the plan must show
VARIANTS = {
    "fed_through_lds": dict(R3DM_AK_FED_MARCH="0"),
    "fed_one_step_per_launch": dict(R3DM_AK_FED_MARCH="0", R3DM_AK_FED_MULTI="0"),
    "march_two_steps": dict(R3DM_AK_FED_KMAX="2", R3DM_AK_FED_WAVES="300"),
    "one_pass_level_head": dict(R3DM_AK_HEAD="1"),
    "prune_one_wavefront": dict(R3DM_AK_PRUNE="0"),
    "prune_live_cap_8": dict(R3DM_AK_LIVE_CAP="8"),
}
VARIANT_IMAGE_CASES = ("noise-163x121-1e-07", "scene-327x245-0.001", "stripes_default_with_a_maximum")


def variant_cases():
    return [c for c in all_cases() if c["name"] in VARIANT_IMAGE_CASES or c["family"] == "planted"]


def variant_plan_proof(variant, plan):
    """what the plan of an image must show for the variant to have run"""
    launches = [l for p in plan for l in p["launches"]]
    forms = {f for f, _, _ in launches}
    if variant == "fed_through_lds":
        assert forms == {1} and all(s == min(4, p["n_steps"] - 4 * m) for p in plan for m, (_, s, _) in enumerate(p["launches"])), "steps through LDS, four at a time"
    elif variant == "fed_one_step_per_launch":
        assert forms == {0} and all(len(p["launches"]) == p["n_steps"] for p in plan), "one step per launch"
    elif variant == "march_two_steps":
        assert forms == {2} and max(s for _, s, _ in launches) == 2 and any(len(p["launches"]) >= 2 for p in plan), "marching strips of 60 columns"
    elif variant == "one_pass_level_head":
        assert all(p["head_form"] == 1 and p["head_rows"] >= 32 for p in plan[1:]) and not plan[0]["head_form"], "the one-pass head on every level above 0"
    else:
        assert forms == {2} and not any(p["head_form"] for p in plan), "the product's scale space"


# ------------------------------------------------------------------------------------------------ the GPU child
def child_main(family, out_path):
    """runs in a child process of the GPU test (the session's process holds the product library): loads the developer library and runs,
    through r3dm_dev_akaze_head / r3dm_dev_akaze_extrema, every case of the family in a call of its own, then the family's batches --
    or, for family "variant:<name>" (the parent has set the variant's environment), the variant's cases -- and pickles {key: per-image
    results}.  Stops at the first error: the file then holds {"__error__": text} beside the results so far."""
    import pickle
    from regard3d_amd import api
    api.use_developer_library()
    res = {}

    def run(ctx, kind, thr, items):
        if kind == "image":
            out, plan = ctx.dev_akaze_head([image(n) for n in items], thr)
            return dict(images=out, plan=plan)
        return dict(images=ctx.dev_akaze_extrema(PW, PH, [c["planes"] for c in items], thr))
    try:
        ctx = api.Context(0)
        if family.startswith("variant:"):
            for c in variant_cases():
                res[("single", c["name"])] = run(ctx, c["kind"], c["thr"], [c["image"] if c["kind"] == "image" else c])
        else:
            for c in all_cases():
                if c["family"] == family:
                    res[("single", c["name"])] = run(ctx, c["kind"], c["thr"], [c["image"] if c["kind"] == "image" else c])
            for name, fam, kind, thr, items in batches():
                if fam == family:
                    res[("batch", name)] = run(ctx, kind, thr, items)
        ctx.close()
    except Exception as e:                        # (reported to the parent, which decides; nothing more runs on the GPU here)
        res["__error__"] = f"{type(e).__name__}: {e}"
    pickle.dump(res, open(out_path, "wb"), protocol=pickle.HIGHEST_PROTOCOL)
    return 3 if "__error__" in res else 0
