"""Level table, reference chain and case tables of the M-SURF-64 descriptor arm (r3dm_detect_akaze_msurf(_batch), R3DM_DESCRIPTOR_MSURF,
R3DM_STAGE_DESCRIPTOR_MSURF, the developer build's r3dm_dev_akaze_msurf).  TEST INFRASTRUCTURE ONLY, shared by test_msurf_cases.py
(which holds the tables' promises on the reference alone, without a GPU), test_gpu_msurf_kernel.py and test_gpu_msurf_arm.py.

The reference chain of an image is composed from what the oracle exposes: orc_akaze_head called with the M-SURF LEVEL TABLE (borders from
12 sqrt(2), Allocate_Memory_Evolution of the vendored Fast-A-KAZE :78-84,105,112 -- the head honours the borders and the level count it is
given), then orc_akaze_tail without MLDB, then the serial restatement tests/cpp/msurf_restatement.cpp per keypoint.

Images: the two sizes and scenes of mldb_arm_cases.py.  Under the M-SURF border the (240, 320) images keep seven of their nine levels
and the (120, 160) images three of their five."""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np

import mldb_arm_cases as M
from oracle import pyoracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "msurf_restatement.cpp")
HDR = os.path.join(ROOT, "regard3d_amd", "csrc", "ak_expf.hpp")
KP_PER_GROUP = 4                                    # kernels_akaze.hip: kAkMsurfPerGroup (one keypoint per wavefront, four per workgroup)
THR = M.THR
SIZES = sorted(M.BATCHES)


# ------------------------------------------------------------------------------------------------ the restatement
def _build_dir():
    h = hashlib.sha256(open(SRC, "rb").read() + open(HDR, "rb").read()).hexdigest()[:16]
    d = os.path.join(tempfile.gettempdir(), f"r3d_msurf_{os.getuid()}_{h}")
    os.makedirs(d, exist_ok=True)
    return d


def _compile(out, extra):
    tmp = f"{out}.{os.getpid()}.tmp"
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-o", tmp, SRC], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        if os.path.exists(tmp):
            os.remove(tmp)
        return r.stderr
    os.replace(tmp, out)
    return None


_LIB = None


def restatement():
    """the restatement as a shared library (built once per source text, g++ -O2 -ffp-contract=off)"""
    global _LIB
    if _LIB is None:
        so = os.path.join(_build_dir(), "libmsurf_restatement.so")
        if not os.path.exists(so):
            err = _compile(so, ["-shared", "-fPIC"])
            assert err is None, err[-3000:]
        L = C.CDLL(so)
        L.msurf_restate.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.msurf_restate.restype = C.c_int
        L.msurf_expf.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.msurf_expf.restype = None
        _LIB = L
    return _LIB


def sanitized_program():
    """-> (path, None) of the stand-alone restatement built with -fsanitize=address,undefined, or (None, why) where that does not link"""
    exe = os.path.join(_build_dir(), "msurf_restatement_asan")
    if not os.path.exists(exe):
        # (the runtimes linked statically: the program then carries its own and asks nothing of the process environment)
        flags = ["-DMSURF_MAIN", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        err = _compile(exe, flags + ["-static-libasan", "-static-libubsan"])
        if err is not None:
            err = _compile(exe, flags)
        if err is not None:
            return None, err[-500:]
    return exe, None


def expf(x, libm):
    """ak_expf (libm False) or libm's expf (True) of float32 values"""
    x = np.ascontiguousarray(x, np.float32).ravel()
    out = np.zeros(x.size, np.float32)
    restatement().msurf_expf(x.ctypes.data, x.size, int(bool(libm)), out.ctypes.data)
    return out


def restate(lx, ly, items, libm=False, want_args=False):
    """rows [n, 64] float32 of the keypoints `items` ([n, 5]: xf, yf, co, si, scale) on one level's Lx / Ly planes [h, w]
    -> (rows, (smallest, largest) exponent argument[, the 1312 arguments of every keypoint])"""
    lx = np.ascontiguousarray(lx, np.float32); ly = np.ascontiguousarray(ly, np.float32)
    assert lx.shape == ly.shape and lx.ndim == 2
    items = np.ascontiguousarray(items, np.float32).reshape(-1, 5)
    n = len(items)
    rows = np.zeros((n, 64), np.float32); rng = np.zeros(2, np.float32)
    args = np.zeros((n, 1312), np.float32) if want_args else None
    left = restatement().msurf_restate(lx.ctypes.data, ly.ctypes.data, lx.shape[1], lx.shape[0], n, items.ctypes.data, int(bool(libm)), rows.ctypes.data,
                                       args.ctypes.data if want_args else None, rng.ctypes.data)
    assert left == 0, f"{left} keypoints read outside their plane"
    return (rows, (float(rng[0]), float(rng[1])), args) if want_args else (rows, (float(rng[0]), float(rng[1])))


# ------------------------------------------------------------------------------------------------ the level table
SMAX_MLDB = np.float32(10.0) * np.sqrt(np.float32(2.0))
SMAX_MSURF = np.float32(12.0) * np.sqrt(np.float32(2.0))


def _border(smax, sigma_size):
    return int(np.float32(smax * np.float32(sigma_size)) + np.float32(0.5)) + 1        # fRound(smax sigma_size) + 1, in float as :105


def levels(w, h):
    """the level table under the KAZE descriptors: the oracle's (MLDB) table with border = fRound(12 sqrt(2) sigma_size) + 1, cut at the
    first level with 2 border + 1 >= w or h of the level (:112) -- a prefix of the oracle's"""
    out = []
    for e in O.akaze_levels(w, h):
        assert e["border"] == _border(SMAX_MLDB, e["sigma_size"])                       # the oracle's table is the MLDB one
        e = dict(e, border=_border(SMAX_MSURF, e["sigma_size"]))
        if 2 * e["border"] + 1 >= e["w"] or 2 * e["border"] + 1 >= e["h"]:
            break
        out.append(e)
    return out


def head(img, threshold, lv=None):
    """orc_akaze_head on the level table `lv` (default: the M-SURF table of the image) -> planes [n_levels] of (Ldet, Lx, Ly, Lt), lists"""
    img = np.ascontiguousarray(img, np.float32)
    h, w = img.shape
    lv = levels(w, h) if lv is None else lv
    nl = len(lv)
    if nl == 0:
        return lv, [], []
    tab = (O.AkHeadLevel * 16)(*[O.AkHeadLevel(*[e[k] for k, _ in O.AkHeadLevel._fields_]) for e in lv])
    planes = [[np.zeros((e["h"], e["w"]), np.float32) for _ in range(4)] for e in lv]
    caps = np.array([((e["w"] + 1) // 2) * ((e["h"] + 1) // 2) for e in lv], np.int32)
    lists = [np.zeros((int(c) + 1, 3), np.float32) for c in caps]
    n_cand = np.zeros(nl, np.int32); n_list = np.zeros(nl, np.int32); kstate = np.zeros(10, np.float32); hist = np.zeros(300, np.int32)
    pp = (C.c_void_p * (4 * nl))(*[q.ctypes.data for lev in planes for q in lev])
    lp = (C.c_void_p * nl)(*[l.ctypes.data for l in lists])
    L = O.lib()
    L.orc_akaze_head.restype = None
    L.orc_akaze_head.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int] + [C.c_void_p] * 8
    L.orc_akaze_head(img.ctypes.data, w, h, float(threshold), nl, C.addressof(tab), C.addressof(pp), C.addressof(lp), caps.ctypes.data, n_cand.ctypes.data,
                     n_list.ctypes.data, kstate.ctypes.data, hist.ctypes.data)
    return lv, planes, [l[:int(n)].copy() for l, n in zip(lists, n_list)]


def fround(v):
    return int(np.float32(v) + np.float32(0.5))


def items_of(lv, t):
    """the tail's keypoints as the descriptor takes them: per keypoint (level, xf, yf, co, si, scale) with xf = x / ratio (:1454-1455),
    scale = fRound(0.5 size / ratio) (:1452)"""
    out = np.zeros((t["n"], 6), np.float64)
    for k in range(t["n"]):
        e = lv[int(t["level"][k])]
        ratio = np.float32(e["ratio"])
        out[k] = (t["level"][k], np.float32(t["x"][k]) / ratio, np.float32(t["y"][k]) / ratio, t["cos"][k], t["sin"][k],
                  fround(np.float32(0.5) * np.float32(t["size"][k]) / ratio))
    return out


def detect(img, threshold, libm=False, lv=None, want_args=False):
    """the reference chain of one image -> dict: kps [n, 4] (x, y, size, angle in degrees), rows [n, 64], items [n, 6] (items_of), levels,
    planes, arg_range (smallest, largest exponent argument; (0, 0) without keypoints)[, args [n, 1312]]"""
    lv, planes, lists = head(img, threshold, lv)
    if not lv:
        return dict(kps=np.zeros((0, 4), np.float32), rows=np.zeros((0, 64), np.float32), items=np.zeros((0, 6)), levels=lv, planes=planes,
                    arg_range=(0.0, 0.0), args=np.zeros((0, 1312), np.float32))
    t = O.akaze_tail(lv, planes, lists, want_desc=False)
    it = items_of(lv, t)
    rows = np.zeros((t["n"], 64), np.float32); args = np.zeros((t["n"], 1312), np.float32)
    lo, hi = 0.0, -100.0
    for i, e in enumerate(lv):
        sel = np.flatnonzero(it[:, 0] == i)
        if len(sel):
            assert (it[sel, 5] == e["sigma_size"]).all()                                 # scale == sigma_size
            r = restate(planes[i][1], planes[i][2], it[sel, 1:], libm, want_args)
            rows[sel] = r[0]; lo = min(lo, r[1][0]); hi = max(hi, r[1][1])
            if want_args:
                args[sel] = r[2]
    kps = np.stack([t["x"], t["y"], t["size"], t["angle_deg"]], axis=1).astype(np.float32) if t["n"] else np.zeros((0, 4), np.float32)
    return dict(kps=kps, rows=rows, items=it, levels=lv, planes=planes, arg_range=(lo, hi if t["n"] else 0.0), args=args)


# ------------------------------------------------------------------------------------------------ the batches
# size -> (threshold, the four images): [scene a, blank, scene b, scene c].  The blank image sits in the MIDDLE; the three textured
# scenes have keypoint counts = 1, 2, 3 mod KP_PER_GROUP under the M-SURF table (test_msurf_cases.py asserts it on the reference), so the
# launch's last workgroup holds one, two and three keypoints in the single-image calls.  Seeds were searched on the reference chain.
BATCH_SEEDS = {(240, 320): (102, 105, 107), (120, 160): (201, 203, 200)}
BLANK_INDEX = 1


def batch_images(size):
    h, w = size
    thr, nb, _, _ = M.BATCHES[size]
    a, b, c = BATCH_SEEDS[size]
    return thr, [M.scene(h, w, a, nb), M.blank(h, w), M.scene(h, w, b, nb), M.scene(h, w, c, nb)]


_REFS = {}


def batch_refs(size):
    """(threshold, images, per image the reference chain's detect()) -- computed once per process, never changed"""
    if size not in _REFS:
        thr, ims = batch_images(size)
        _REFS[size] = (thr, ims, [detect(im, thr, want_args=True) for im in ims])
    return _REFS[size]


# ------------------------------------------------------------------------------------------------ the stage
STAGE_RATIO = 0.8
STAGE_FILTER_SEED = M.STAGE_FILTER_SEED


def stage_images():
    return M.stage_images()


def oracle_stage(ims):
    """the chain the stage serves under R3DM_STAGE_DESCRIPTOR_MSURF: detect() per view, the exhaustive float matcher with the facade's
    SQUARED ratio on every pair (as LIOP rows are matched), positions as the .feat text carries them"""
    refs = [detect(im, THR) for im in ims]
    descs = [r["rows"] for r in refs]; xys = [M.g6(r["kps"][:, :2]) for r in refs]
    i, j = np.triu_indices(len(ims), k=1)
    pairs = np.stack([i, j], axis=1).astype(np.uint32)
    counts, matches = O.match_collection(descs, xys, pairs, STAGE_RATIO, True)
    return refs, descs, xys, pairs, counts, matches


def desc_file(path):
    """(count, rows [count, 64] float32) of an M-SURF .desc file"""
    raw = np.fromfile(path, np.uint8)
    n = int(np.frombuffer(raw[:8].tobytes(), np.uint64)[0])
    assert raw.size == 8 + 256 * n, (path, raw.size, n)
    return n, np.frombuffer(raw[8:].tobytes(), np.float32).reshape(n, 64).copy()


def same_rows(a, b):
    """bit for bit, except that a row of NaN equals a row of NaN (the window without gradient: 0 / 0, whose sign and payload are not held)"""
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a).all(axis=1), np.isnan(b).all(axis=1)
    return bool((na == nb).all()) and a[~na].tobytes() == b[~nb].tobytes()


# ------------------------------------------------------------------------------------------------ the kernel cases
# Synthetic Lx / Ly planes of an image size, items placed by hand: what images hardly produce.  KERNEL_SIZES: (h, w) of the image.
# (96, 128) has ONE level under the M-SURF table (sigma_size 2); (160, 192) is the smallest size whose table holds sigma_size 2, 3 and 4
# and a second octave (five levels: four planes of 160 x 192 and one of 80 x 96).  A 48 x 64 image has no level at all under this border
# (2 x 35 + 1 >= 48), so no item on such a plane can pass the check: test_msurf_cases.py holds that.
KERNEL_SIZES = [(96, 128), (160, 192)]
ANGLES = {"0": (1.0, 0.0), "45": (np.cos(np.float32(np.pi / 4)), np.sin(np.float32(np.pi / 4))), "90": (0.0, 1.0),
          "225": (-np.cos(np.float32(np.pi / 4)), -np.sin(np.float32(np.pi / 4))), "pi": (-1.0, 0.0),
          "libm-0": (np.cos(np.float32(0.0)), np.sin(np.float32(0.0))), "libm-pi": (np.cos(np.float32(np.pi)), np.sin(np.float32(np.pi)))}


def textured(lv, seed, kind="signed"):
    """Lx / Ly planes of every level: signed noise on a smooth field; 'positive' (one sign: dx == mdx); 'alternating' (checkerboard sign:
    cancellation); 'zero'"""
    rng = np.random.default_rng(seed)
    out = []
    for e in lv:
        yy, xx = np.mgrid[0:e["h"], 0:e["w"]]
        pl = []
        for q in range(2):
            a = (0.02 * np.sin(xx / (5.0 + q)) * np.cos(yy / (7.0 - q)) + rng.normal(0, 0.01, xx.shape)).astype(np.float32)
            if kind == "positive":
                a = np.abs(a) + np.float32(1e-4)
            elif kind == "alternating":
                a = (np.abs(a) + np.float32(1e-3)) * np.where((xx + yy) % 2 == 0, 1, -1).astype(np.float32)
            elif kind == "zero":
                a = np.zeros_like(a)
            pl.append(np.ascontiguousarray(a, np.float32))
        out.append(pl)
    return out


def item(level, xf, yf, angle, lv):
    co, si = ANGLES[angle] if isinstance(angle, str) else angle
    return (level, np.float32(xf), np.float32(yf), np.float32(co), np.float32(si), lv[level]["sigma_size"])


def kernel_cases():
    """-> list of dicts: name, size (h, w), levels, planes [n_levels] of (Lx, Ly), items [n, 6] (level, xf, yf, co, si, scale), nan_rows
    (indices whose row must be all NaN)"""
    cases = []

    def add(name, size, planes, items, nan_rows=()):
        cases.append(dict(name=name, size=size, levels=levels(size[1], size[0]), planes=planes, items=np.array(items, np.float64).reshape(-1, 6),
                          nan_rows=list(nan_rows)))

    for size in KERNEL_SIZES:
        h, w = size
        lv = levels(w, h)
        tag = f"{h}x{w}"
        tex = textured(lv, 7 + h)
        # the reach extremes: a keypoint at border - 1 and one at dim - border, in both coordinates, at four angles, on every level
        its = []
        for i, e in enumerate(lv):
            b = e["border"]
            for ang in ("0", "45", "90", "225"):
                its.append(item(i, b - 1, b - 1, ang, lv)); its.append(item(i, e["w"] - b, e["h"] - b, ang, lv))
                its.append(item(i, b - 1, e["h"] - b, ang, lv)); its.append(item(i, e["w"] - b, b - 1, ang, lv))
        add(f"border-{tag}", size, tex, its)
        # sample coordinates on exact .5 boundaries (fRound): at angle 0 a sample is position + integer, so position x.5 puts every one there
        mid = [(i, e["w"] // 2, e["h"] // 2) for i, e in enumerate(lv)]
        its = [item(i, x + 0.5, y + 0.5, a, lv) for i, x, y in mid for a in ("0", "90", "pi")]
        its += [item(i, x + 0.5, y, "0", lv) for i, x, y in mid] + [item(i, x, y - 0.5, "libm-pi", lv) for i, x, y in mid]
        add(f"half-{tag}", size, tex, its)
        # angles exactly 0 and pi, by hand and as libm forms them; a general one
        its = [item(i, x + 0.25, y - 0.125, a, lv) for i, x, y in mid for a in ("0", "pi", "libm-0", "libm-pi")]
        its += [item(i, x, y, (np.cos(np.float32(1.234)), np.sin(np.float32(1.234))), lv) for i, x, y in mid]
        add(f"angles-{tag}", size, tex, its)
        add(f"one_sign-{tag}", size, textured(lv, 11, "positive"), [item(i, x + 0.3, y + 0.7, a, lv) for i, x, y in mid for a in ("0", "45")])
        add(f"alternating-{tag}", size, textured(lv, 12, "alternating"), [item(i, x + 0.5, y + 0.5, a, lv) for i, x, y in mid for a in ("0", "45", "90")])
        # a window without gradient among windows with: the NaN row must not leak into its neighbours of the workgroup
        zero = textured(lv, 13)
        e = lv[0]
        x0, y0 = e["border"] - 1, e["border"] - 1
        for q in range(2):
            zero[0][q][:2 * e["border"], :2 * e["border"]] = 0.0
        add(f"nan_row-{tag}", size, zero, [item(0, e["w"] - e["border"], e["h"] - e["border"], "45", lv), item(0, x0, y0, "45", lv),
                                             item(0, e["w"] // 2 + 20, e["h"] // 2, "0", lv)] * 2, nan_rows=[1, 4])
        add(f"all_zero-{tag}", size, textured(lv, 14, "zero"), [item(0, e["w"] // 2, e["h"] // 2, "0", lv)], nan_rows=[0])
    # launch sizes: 0, 1, one workgroup's worth -1, +0, +1, four workgroups' worth + 1, 37
    size = KERNEL_SIZES[1]
    lv = levels(size[1], size[0])
    tex = textured(lv, 21)
    rng = np.random.default_rng(5)
    for n in (0, 1, KP_PER_GROUP - 1, KP_PER_GROUP, KP_PER_GROUP + 1, 4 * KP_PER_GROUP + 1, 37):
        its = []
        for k in range(n):
            i = int(rng.integers(len(lv))); e = lv[i]; b = e["border"]
            th = np.float32(rng.uniform(0, 2 * np.pi))
            its.append(item(i, rng.uniform(b - 1, e["w"] - b), rng.uniform(b - 1, e["h"] - b), (np.cos(th), np.sin(th)), lv))
        add(f"count-{n}", size, tex, its)
    return cases


_KREF = {}


def kernel_reference(case, libm=False):
    """rows [n, 64] of a kernel case by the restatement"""
    key = (case["name"], libm)
    if key not in _KREF:
        it = case["items"]
        rows = np.zeros((len(it), 64), np.float32)
        for i in range(len(case["levels"])):
            sel = np.flatnonzero(it[:, 0] == i)
            if len(sel):
                rows[sel] = restate(case["planes"][i][0], case["planes"][i][1], it[sel, 1:], libm)[0]
        _KREF[key] = rows
    return _KREF[key]


def api_items(case):
    from regard3d_amd import api
    it = case["items"]
    out = np.zeros(len(it), api.MSURF_ITEM)
    for j, k in enumerate(("level", "xf", "yf", "co", "si", "scale")):
        out[k] = it[:, j]
    return out


def child_main(out_path):
    """runs in a child process of the GPU test (the session's process holds the product library): loads the developer library, runs every
    kernel case through r3dm_dev_akaze_msurf (which passes it through r3dm_dev_akaze_msurf_check first), pickles {name: rows}.  Stops at
    the first error: the file then holds {"__error__": text} beside the results so far, and nothing more runs on the GPU."""
    import pickle
    from regard3d_amd import api
    api.use_developer_library()
    res = {}
    try:
        ctx = api.Context(0)
        for c in kernel_cases():
            res[c["name"]] = ctx.dev_akaze_msurf(c["size"][1], c["size"][0], c["planes"], api_items(c))
        ctx.close()
    except Exception as e:
        res["__error__"] = f"{type(e).__name__}: {e}"
    pickle.dump(res, open(out_path, "wb"))
    return 3 if "__error__" in res else 0
