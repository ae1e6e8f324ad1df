"""The case table of the classic A-KAZE head (tests/akaze_classic_head_cases.py) proved on the CPU, and the parts of the CPU restatement
(tests/akaze_classic_restatement.py) that the GPU half compares the head with pinned against plain forms of their own: every case
reaches the edge it is named for on the reference alone; nld_step against a float64 zero-flux divergence form; scaled_deriv against a
float64 separable filter over np.pad(mode="reflect"); candidates against a triple-loop brute force on every planted plane; the histogram
on hand-built moduli; mutated copies of the step and of candidates are each noticed by a named case through the comparison the GPU half
uses; r3dm_dev_akaze_classic_head_check / _extrema_check accept every case and refuse each clause of their contracts.  The GPU half is
tests/test_gpu_akaze_classic_head.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import akaze_classic_head_cases as T

R = T.R
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = T.all_cases()
INVALID = -1
U = 2.0 ** -24                                     # unit roundoff of float32


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_case_reaches_its_edge_on_the_reference(case):
    case["proof"](case, T.reference(case))


def test_every_case_of_the_issue_is_in_the_table():
    names = {c["name"] for c in CASES}
    want = {"noise-67x45-1e-07", "noise-131x43-1e-07", "noise-160x80-1e-07", "noise-163x83-1e-07", "noise-163x83-0.001", "scene-321x161-0.001",
            "scene-640x320-0.001", "steps-163x83-0.001", "faint-67x45-1e-07", "ramp-160x80-0.001", "pixel-160x80-0.001", "flat-160x80-0.001",
            "seams-66x45", "seams-67x45", "seams-130x45", "seams-131x45", "ties", "thresholds-0.001", "thresholds-1e-07", "nonfinite_neighbours",
            "dense-131x45", "dense-67x300", "scan_chunk"}
    assert want <= names, want - names
    assert {c["size"] for c in CASES if c["kind"] == "planes"} == set(T.TABLES)
    assert len(R.levels(160, 80)) == 8 and len(R.levels(159, 80)) == 4 and len(R.levels(160, 79)) == 4
    assert np.array_equal(T.image("faint-67x45"), T.image("noise-67x45") * F(2.0 ** -62)) and T.image("faint-67x45").max() < 2.0 ** -62
    assert sum(T.image(c["image"]).size for c in CASES if c["kind"] == "image") < 500000, "a few hundred thousand pixels in all"
    # every image and every planted case rides in a batch of three with an image without a candidate in the middle
    in_batches = set()
    for name, fam, kind, thr, items in T.batches():
        assert len(items) == 3
        if kind == "image":
            assert items[1].startswith("flat") and len({T.size_of(i) for i in items}) == 1
            assert not T.head_reference(items[1], thr)["counts"].any()
            in_batches |= {(items[0], float(thr)), (items[2], float(thr))}
        else:
            assert len({i["size"] for i in items}) == 1 and not T.reference(items[1])["counts"].any()
            in_batches |= {items[0]["name"], items[2]["name"]}
    assert in_batches >= {(c["image"], float(c["thr"])) for c in CASES if c["kind"] == "image" and not c["image"].startswith("flat")}
    assert in_batches >= {c["name"] for c in CASES if c["kind"] == "planes"}


def test_added_outputs_leave_the_restatement_as_it_was():
    """kcontrast is the third part of kcontrast_parts, and the planes scale_space now keeps are the ones the detector's inputs came from"""
    img = T.image("noise-163x83")
    hmax, hist, k = R.kcontrast_parts(img)
    assert R.kcontrast(img) == k and hist.sum() == (T.modulus("noise-163x83") != 0).sum() and hmax == T.modulus("noise-163x83").max()
    lv, k_last = R.scale_space(img)
    assert k_last == F(k * F(0.75)) and lv[0]["Lt"] is lv[0]["Lsmooth"] and lv[0]["Lflow"] is None
    for i in range(1, 8):
        assert lv[i]["Lt"].shape == lv[i]["Lflow"].shape == lv[i]["Lsmooth"].shape == lv[i]["Ldet"].shape == (lv[i]["h"], lv[i]["w"])
        assert np.array_equal(R.scaled_deriv(lv[i]["Lsmooth"], lv[i]["sigma_size"], True), lv[i]["Lx"])
    assert np.array_equal(R._oracle().akaze_gaussian(lv[1]["Lt"], 1.0), lv[2]["Lsmooth"]), "level 2 starts from level 1's Lt"


# ---------------------------------------------------------------------------------------------------- nld_step
def _divergence_f64(L, c, half_step):
    """L + half_step * sum over the neighbours q inside the image of (c_p + c_q) (L_q - L_p), in float64: the zero-flux divergence
    form -> (the result, half_step * the sum of |fluxes| of every pixel)"""
    L, c = L.astype(np.float64), c.astype(np.float64)
    h, w = L.shape
    s, a = np.zeros((h, w)), np.zeros((h, w))
    for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0)):
        p = (slice(max(0, -dy), h - max(0, dy)), slice(max(0, -dx), w - max(0, dx)))
        q = (slice(max(0, dy), h - max(0, -dy)), slice(max(0, dx), w - max(0, -dx)))
        flux = (c[p] + c[q]) * (L[q] - L[p])
        s[p] += flux; a[p] += np.abs(flux)
    return L + half_step * s, half_step * a


def _step_inputs():
    rng = np.random.default_rng(11)
    for h, w in ((45, 67), (3, 3), (3, 64)):
        yield rng.uniform(0, 1, (h, w)).astype(F), rng.uniform(0, 1, (h, w)).astype(F), F(0.37 + 0.1 * h)


def _step_error_ratio(step):
    """the worst |got - ref| / bound over the inputs, and the worst |sum of the step| / sum of the bounds.

    The bound, with u = 2^-24: a flux (c_p + c_q) * (L_q - L_p) has 3 roundings; it then passes through at most 3 additions of fluxes,
    1 multiplication by the half step (0.5f * stepsize is exact) and the final addition to L: 3 + 3 + 1 = 7 roundings on every flux
    and 1 on the result, so |got - ref| <= 8 u (half_step * sum |fluxes of the pixel| + |ref|); second-order terms lie within the slack
    between 7 and 8."""
    worst, worst_mass = 0.0, 0.0
    for L, c, tau in _step_inputs():
        got = step(L, c, tau).astype(np.float64)
        hs = float(F(F(0.5) * tau))
        ref, flux = _divergence_f64(L, c, hs)
        bound = 8 * U * (flux + np.abs(ref))
        worst = max(worst, float((np.abs(got - ref) / bound).max()))
        worst_mass = max(worst_mass, abs(float((got - L.astype(np.float64)).sum())) / float(bound.sum()))
    return worst, worst_mass


def test_nld_step_is_the_zero_flux_divergence_form():
    """(measured: 0.229 of the bound at worst, that is 1.83 u (hs sum |flux| + |ref|); the step's sum is 0.0006 of the summed bounds)"""
    worst, mass = _step_error_ratio(R.nld_step)
    print(f"nld_step: worst |got - ref| / bound = {worst:.3f} ({8 * worst:.2f} u), |sum of the step| / sum of bounds = {mass:.4f}")
    assert worst <= 1.0, worst
    assert mass <= 1.0, ("mass conservation: the float64 sum of the step over the image is 0 to rounding", mass)


def _step_last_row_reads_below(L, c, stepsize):
    """MUTATION: the last row's flux is read from the row below, clamped, instead of the row above -- the clamped row is the row
    itself, so the flux is (c + c) * (L - L)"""
    return _mutated_step(L, c, stepsize, "last_row")


def _step_corner_uses_the_edge_form(L, c, stepsize):
    """MUTATION: the corners use their row's edge form (xpos - xneg + ypos), whose missing x neighbour is then the neighbour in memory:
    the last pixel of the row above for the bottom-left corner, the first pixel of the row below for the top-right one (the other
    two corners' memory neighbours lie outside the plane and stay clamped)"""
    return _mutated_step(L, c, stepsize, "corner")


_TRUE_STEP = R.nld_step                            # (the mutations run while R.nld_step is replaced by them)


def _mutated_step(L, c, stepsize, which):
    out = _TRUE_STEP(L, c, stepsize)
    hs = F(F(0.5) * F(stepsize))
    flux = lambda p, q: F(F(c[p] + c[q]) * F(L[q] - L[p]))   # noqa: E731
    h, w = L.shape
    if which == "last_row":
        for x in range(w):
            p = (h - 1, x)
            xpos = flux(p, (h - 1, x + 1)) if x < w - 1 else None
            xneg = flux((h - 1, x - 1), p) if x > 0 else None
            v = xpos if xneg is None else F(-xneg) if xpos is None else F(xpos - xneg)
            out[p] = F(L[p] + F(hs * F(v + flux(p, p))))
    else:
        p = (h - 1, 0)
        out[p] = F(L[p] + F(hs * F(F(flux(p, (h - 1, 1)) - flux((h - 2, w - 1), p)) + flux(p, (h - 2, 0)))))
        p = (0, w - 1)
        out[p] = F(L[p] + F(hs * F(F(flux(p, (1, 0)) - flux((0, w - 2), p)) + flux(p, (1, w - 1)))))
    return out


def test_the_divergence_form_notices_a_wrong_edge_or_corner():
    for step in (_step_last_row_reads_below, _step_corner_uses_the_edge_form):
        worst, mass = _step_error_ratio(step)
        assert worst > 1000 and mass > 1.0, (step.__name__, worst, mass)


# ---------------------------------------------------------------------------------------------------- scaled_deriv
def _separable_f64(src, s, dx, absolute=False):
    """the float64 separable filter of compute_derivative_kernels' taps over np.pad(mode="reflect"); absolute: |taps| over |src|"""
    norm, kc = (float(v) for v in R.deriv_taps(s))
    diff, smooth = {-s: -1.0, s: 1.0}, {-s: norm, 0: kc, s: norm}
    kx, ky = (diff, smooth) if dx else (smooth, diff)
    P = np.pad(np.abs(src.astype(np.float64)) if absolute else src.astype(np.float64), s, mode="reflect")
    h, w = src.shape
    out = np.zeros((h, w))
    for oy, ty in ky.items():
        for ox, tx in kx.items():
            t = ty * tx
            out += (abs(t) if absolute else t) * P[s + oy:s + oy + h, s + ox:s + ox + w]
    return out


def test_scaled_deriv_is_the_separable_filter_on_reflected_borders():
    """The bound: n u x (the filter with |taps| over |src|), n = 4 float operations on the longest path of every form -- dx: the row
    difference (1; the negation is exact), d + u (1), norm * (1), the last addition (1); dy, s = 2: a + b (1), * norm (1), + (1), the
    column difference (1); dy, s >= 3: norm * a (1), + (1), + (1), the column difference (1).  n u / (1 - n u) covers the second order.
    (measured: 0.411 of the bound at worst)"""
    rng = np.random.default_rng(12)
    worst = 0.0
    for h, w in ((45, 67), (7, 3), (3, 9), (2, 2), (4, 64)):           # 7 x 3, 3 x 9 and 2 x 2: narrower than s + 1, the reflection loops
        src = rng.uniform(0.1, 0.3, (h, w)).astype(F)
        for s in (2, 3, 4):
            for dx in (True, False):
                got = R.scaled_deriv(src, s, dx).astype(np.float64)
                ref = _separable_f64(src, s, dx)
                bound = (4 * U / (1 - 4 * U)) * _separable_f64(src, s, dx, absolute=True)
                assert (np.abs(got - ref) <= bound).all(), (h, w, s, dx, float((np.abs(got - ref) / bound).max()))
                worst = max(worst, float((np.abs(got - ref) / bound).max()))
    print(f"scaled_deriv: worst |got - ref| / bound = {worst:.3f}")


# ---------------------------------------------------------------------------------------------------- candidates
def _brute_force(P, thr):
    """strict 3 x 3 maxima over the threshold and the 1e-5 floor, rows 1 .. h - 2 x columns 1 .. w - 2, one pixel at a time"""
    h, w = P.shape
    out = []
    for y in range(1, h - 1):
        for x in range(1, w - 1):
            v = P[y, x]
            if not (v > thr and v >= F(0.00001)):
                continue
            if all(v > P[y + dy, x + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dy or dx):
                out.append((y, x))
    return out


@pytest.mark.parametrize("case", [c for c in CASES if c["kind"] == "planes"], ids=[c["name"] for c in CASES if c["kind"] == "planes"])
def test_candidates_equal_a_brute_force_on_the_planted_planes(case):
    for level, P in enumerate(case["planes"]):
        assert [tuple(t) for t in R.candidates(P, case["thr"]).tolist()] == _brute_force(P, case["thr"]), (case["name"], level)


def _candidates_mutation(which):
    def lists(planes, thr):
        def one(ldet):
            c = ldet[1:-1, 1:-1]
            m = (c > F(thr)) & ((c >= R.MIN_DTHRESHOLD) | (which == "no_floor"))
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if dy or dx:
                        n = ldet[1 + dy:ldet.shape[0] - 1 + dy, 1 + dx:ldet.shape[1] - 1 + dx]
                        m &= (c >= n) if which == "ge" else (c > n)
            if which == "short_columns":
                m[:, -1] = False                                             # columns stop at w - 3
            ys, xs = np.nonzero(m)
            return np.stack([ys + 1, xs + 1], 1)
        keep = R.candidates
        try:
            R.candidates = lambda P, t: one(P)
            return T.candidate_lists(planes, thr)
        finally:
            R.candidates = keep
    return lists


def _as_result(ref):
    """a reference in the form the developer entries return"""
    out = dict(ref)
    if "levels" in ref:
        out.update(hmax_bits=F(ref["hmax"]).view(np.uint32), planes=ref["levels"])
    return out


NOTICED_BY = {                                      # mutation -> (the named case that must notice it, the stage the comparison names)
    "step:last_row": ("noise-163x83-1e-07", "level 1 Lt"),
    "step:corner": ("noise-163x83-1e-07", "level 1 Lt"),
    "candidates:ge": ("ties", "counts"),
    "candidates:no_floor": ("thresholds-1e-07", "counts"),
    "candidates:short_columns": ("seams-67x45", "counts"),
}


def test_head_cases_notice_a_wrong_step_and_a_wrong_extremum_pass():
    """the comparison the GPU half applies (T.first_mismatch), fed a head whose step or extremum pass is subtly wrong, names the stage"""
    by_name = {c["name"]: c for c in CASES}
    steps = {"last_row": _step_last_row_reads_below, "corner": _step_corner_uses_the_edge_form}
    for mutation, (name, stage) in NOTICED_BY.items():
        case = by_name[name]
        kind, which = mutation.split(":")
        ref = T.reference(case)
        assert T.first_mismatch(_as_result(ref), ref, planes=case["kind"] == "image") is None, "the comparison passes the reference itself"
        if kind == "step":
            wrong = T.head_reference(case["image"], case["thr"], step=steps[which])
        elif case["kind"] == "image":
            wrong = T.head_reference(case["image"], case["thr"], candidates=_candidates_mutation(which))
        else:
            wrong = _candidates_mutation(which)(case["planes"], case["thr"])
        m = T.first_mismatch(_as_result(wrong), ref, planes=case["kind"] == "image")
        assert m is not None and m[0] == stage, (mutation, name, m)
        if kind == "step":                          # level 1's n steps carry the error at most n - 1 pixels away from where it was made
            h, w = ref["levels"][1]["Lt"].shape
            n = len(R.fed_tau(F(ref["levels"][1]["etime"] - ref["levels"][0]["etime"])))
            near = (lambda y, x: y >= h - n) if which == "last_row" else (lambda y, x: min(h - 1 - y + x, y + w - 1 - x) < n)
            assert m[2] and all(near(y, x) for y, x in m[2]), ("beside the mutated row / corners", n, m[1])
    # the image cases notice the extremum mutations too: the floor and the >= on the noise image's own planes
    noise = by_name["noise-163x83-1e-07"]
    wrong = T.head_reference(noise["image"], noise["thr"], candidates=_candidates_mutation("no_floor"))
    assert T.first_mismatch(_as_result(wrong), T.reference(noise))[0] == "counts"
    # and a NaN in the place of a number, or a number in the place of a NaN, is a mismatch; a NaN of another payload is none
    flat = T.reference(by_name["flat-160x80-0.001"])
    other = _as_result(flat); other["planes"] = [dict(e) for e in flat["levels"]]
    other["planes"][1]["Lt"] = -flat["levels"][1]["Lt"]
    assert T.first_mismatch(other, flat) is None
    other["planes"][1]["Lt"] = np.zeros_like(flat["levels"][1]["Lt"])
    assert T.first_mismatch(other, flat)[0] == "level 1 Lt"
    other["planes"][1]["Lt"] = flat["levels"][1]["Lt"]
    other["planes"][0]["Ldet"] = flat["levels"][0]["Ldet"].copy(); other["planes"][0]["Ldet"][3, 4] = np.nan
    assert T.first_mismatch(other, flat)[0] == "level 0 Ldet"


# ---------------------------------------------------------------------------------------------------- the histogram
def test_histogram_on_hand_built_moduli():
    m = np.array([[0.0, 1.0, 0.5, 2.0], [0.001, 1.99, 0.0, 2.0], [1.0, 0.0, 0.0, 0.0078125]], F)
    hmax, hist, n = R.modulus_histogram(m)
    assert hmax == 2.0 and n == 8 and hist.sum() == 8, "a zero modulus is not counted"
    want = np.zeros(300); want[150] = 2; want[75] = 1; want[299] = 2; want[0] = 1; want[298] = 1; want[1] = 1
    assert np.array_equal(hist, want), "value == hmax goes in bin 299; bins are floor(300 * (modg / hmax)); a tiny non-zero modulus is counted in bin 0"
    assert int(np.floor(F(300) * (F(1.99) / F(2.0)))) == 298 and int(np.floor(F(300) * (F(0.0078125) / F(2.0)))) == 1
    hmax, hist, n = R.modulus_histogram(np.zeros((3, 3), F))
    assert hmax == 0 and n == 0 and not hist.any()
    hmax, hist, n = R.modulus_histogram(np.full((2, 2), F(0.7)))
    assert hist[299] == 4 and hist.sum() == 4, "one value: everything equals hmax"


# ---------------------------------------------------------------------------------------------------- the developer library, in a child
def _in_child(fn):
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; import test_akaze_classic_head_cases as M; M.{fn}()"
    e = {k: v for k, v in os.environ.items() if not k.startswith("R3DM_")}
    r = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]


def _dev():
    from regard3d_amd import api
    return api, api.bind_dev_akaze_classic_head(C.CDLL(api.DEV_LIB_PATH))


def test_dev_entries_exist_in_the_developer_build_only():
    from regard3d_amd import api
    syms = subprocess.run(["nm", "-D", api.LIB_PATH], capture_output=True, text=True).stdout
    dsyms = subprocess.run(["nm", "-D", api.DEV_LIB_PATH], capture_output=True, text=True).stdout
    assert "r3dm_dev_" not in syms
    for name in ("r3dm_dev_akaze_classic_head", "r3dm_dev_akaze_classic_head_check", "r3dm_dev_akaze_classic_extrema",
                 "r3dm_dev_akaze_classic_extrema_check", "r3dm_dev_akaze_classic_levels"):
        assert f" T {name}\n" in dsyms, name
    hdr = "".join(open(os.path.join(ROOT, "include", f)).read() for f in os.listdir(os.path.join(ROOT, "include")))
    assert "r3dm_dev_akaze_classic" not in hdr


def test_the_level_table_is_the_products():
    _in_child("_level_table")


def _level_table():
    api, L = _dev()
    sizes = {T.size_of(c["image"]) for c in CASES if c["kind"] == "image"} | set(T.TABLES) | {(159, 80), (160, 79), (999, 757), (3, 3)}
    for w, h in sorted(sizes):
        mine, theirs = R.levels(w, h), api.dev_akaze_classic_levels(L, w, h)
        assert len(mine) == len(theirs) > 0, (w, h)
        for a, b in zip(mine, theirs):
            assert (a["w"], a["h"], a["octave"]) == (b["w"], b["h"], b["octave"]), (w, h)
            assert F(a["esigma"]).tobytes() == F(b["esigma"]).tobytes() and F(a["ratio"]).tobytes() == F(b["ratio"]).tobytes(), (w, h)
    assert api.dev_classic_bound(R.levels(67, 300)) == 4 * 4917 == len(T.reference(next(c for c in CASES if c["name"] == "dense-67x300"))["value"])


def test_checks_accept_every_case_and_refuse_each_clause():
    _in_child("_validation_checks")


def _head_check(dev, images, w=None, h=None, B=None):
    api, L = dev
    ptrs, keep = api.dev_head_images(images)
    hh, ww = keep[0].shape
    return L.r3dm_dev_akaze_classic_head_check(len(images) if B is None else B, C.addressof(ptrs), ww if w is None else w, hh if h is None else h)


def _extrema_check(dev, planes, size, n_levels=None, dims=None, B=None):
    api, L = dev
    nl, d, ptrs, keep = api.dev_extrema_args(planes)
    if dims is not None:
        d = np.ascontiguousarray(dims, np.uint32)
    return L.r3dm_dev_akaze_classic_extrema_check(size[0], size[1], len(planes) if B is None else B, nl if n_levels is None else n_levels,
                                                  api._ptr(d), C.addressof(ptrs))


def _validation_checks():
    dev = _dev()
    api, L = dev
    for c in CASES:
        if c["kind"] == "image":
            assert _head_check(dev, [T.image(c["image"])]) == 0, c["name"]
        else:
            assert _extrema_check(dev, [c["planes"]], c["size"]) == 0, c["name"]
    for name, fam, kind, thr, items in T.batches():
        assert (_head_check(dev, [T.image(i) for i in items]) if kind == "image"
                else _extrema_check(dev, [i["planes"] for i in items], items[0]["size"])) == 0, name
    # ---- the head check: B outside 1 .. 1024, sizes below 3 or above 65536, null pointers, values outside [0, 1]
    tiny = np.zeros((3, 3), F)
    assert _head_check(dev, [tiny]) == 0 and _head_check(dev, [tiny] * 1024) == 0 and _head_check(dev, [tiny] * 1025) == INVALID
    assert _head_check(dev, [tiny], B=0) == INVALID
    assert _head_check(dev, [np.zeros((3, 2), F)]) == INVALID and _head_check(dev, [np.zeros((2, 3), F)]) == INVALID
    wide = np.zeros((3, 65536), F)
    assert _head_check(dev, [wide]) == 0 and _head_check(dev, [wide.reshape(65536, 3)]) == 0
    assert _head_check(dev, [wide], w=65537, h=3) == INVALID and _head_check(dev, [wide], w=3, h=65537) == INVALID
    flat = T.image("flat-160x80")
    edge = flat.copy(); edge[0, 0] = 0.0; edge[-1, -1] = 1.0
    assert _head_check(dev, [edge]) == 0, "0 and 1 themselves are taken"
    for v in (np.nan, np.inf, -np.inf, np.nextafter(F(1), F(2)), -np.nextafter(F(0), F(1)), -1.0, 2.0):
        bad = flat.copy(); bad[-1, -1] = v
        assert _head_check(dev, [bad]) == INVALID, v
        assert _head_check(dev, [flat, flat, bad]) == INVALID, "in a later image of the batch too"
    ptrs, keep = api.dev_head_images([flat])
    assert L.r3dm_dev_akaze_classic_head_check(1, None, 160, 80) == INVALID
    null = (C.c_void_p * 2)(ptrs[0], None)
    assert L.r3dm_dev_akaze_classic_head_check(2, C.addressof(null), 160, 80) == INVALID
    out = [np.zeros(4096, np.uint8) for _ in range(5)]
    bad = flat.copy(); bad[3, 3] = np.nan
    pb, kb = api.dev_head_images([bad])
    assert L.r3dm_dev_akaze_classic_head(None, 1, C.addressof(pb), 160, 80, 0.001, api._ptr(out[0]), api._ptr(out[1]), api._ptr(out[2]), 16,
                                         api._ptr(out[3]), api._ptr(out[4])) == INVALID, "refused before a context is asked for"
    assert L.r3dm_dev_akaze_classic_head(None, 1, C.addressof(ptrs), 160, 80, 0.001, api._ptr(out[0]), api._ptr(out[1]), api._ptr(out[2]), 16,
                                         api._ptr(out[3]), api._ptr(out[4])) == INVALID, "a null context"
    lv = (api.DevAcLevel * 16)(); n = C.c_uint32(0)
    assert L.r3dm_dev_akaze_classic_levels(2, 100, C.addressof(lv), C.addressof(n)) == INVALID
    assert L.r3dm_dev_akaze_classic_levels(100, 65537, C.addressof(lv), C.addressof(n)) == INVALID
    assert L.r3dm_dev_akaze_classic_levels(100, 100, None, C.addressof(n)) == INVALID and L.r3dm_dev_akaze_classic_levels(100, 100, C.addressof(lv), None) == INVALID
    # ---- the extrema check: the table's plane dimensions, B, sizes, null pointers; any value is taken
    size = (67, 45)
    base = T.blank_planes(size, 1)
    assert _extrema_check(dev, [base], size) == 0
    odd = [p.copy() for p in base]; odd[0][0, 0] = np.nan; odd[3][-1, -1] = np.inf; odd[2][5, 5] = -np.inf; odd[1][7, 7] = F(3e38)
    assert _extrema_check(dev, [odd], size) == 0, "any value, on the rim too"
    dims = np.array([[67, 45]] * 4, np.uint32)
    assert _extrema_check(dev, [base], size, dims=dims) == 0
    for level, k in ((0, 0), (3, 1), (2, 0)):
        for step in (-1, 1):
            bad = dims.astype(np.int64); bad[level, k] += step
            assert _extrema_check(dev, [base], size, dims=bad) == INVALID, (level, k, step)
    assert _extrema_check(dev, [base], size, n_levels=3) == INVALID and _extrema_check(dev, [base], size, n_levels=5) == INVALID
    assert _extrema_check(dev, [base], (66, 45)) == INVALID and _extrema_check(dev, [base], (67, 300)) == INVALID, "the planes of another table"
    assert _extrema_check(dev, [base], (2, 45)) == INVALID and _extrema_check(dev, [base], (67, 65537)) == INVALID
    assert _extrema_check(dev, [base] * 1024, size) == 0 and _extrema_check(dev, [base] * 1025, size) == INVALID and _extrema_check(dev, [base], size, B=0) == INVALID
    nl, d, ptrs, keep = api.dev_extrema_args([base])
    assert L.r3dm_dev_akaze_classic_extrema_check(67, 45, 1, nl, None, C.addressof(ptrs)) == INVALID
    assert L.r3dm_dev_akaze_classic_extrema_check(67, 45, 1, nl, api._ptr(d), None) == INVALID
    null = (C.c_void_p * nl)(*[None if k == 2 else ptrs[k] for k in range(nl)])
    assert L.r3dm_dev_akaze_classic_extrema_check(67, 45, 1, nl, api._ptr(d), C.addressof(null)) == INVALID
    assert L.r3dm_dev_akaze_classic_extrema(None, 67, 45, 1, nl, api._ptr(d), C.addressof(ptrs), 0.001, api._ptr(out[0]), 16, api._ptr(out[1]),
                                            api._ptr(out[2])) == INVALID, "a null context"
