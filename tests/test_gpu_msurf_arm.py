"""The M-SURF-64 descriptor arm from the batch entry to the stage, bit-exact against the reference chain of tests/msurf_cases.py (the
oracle's head on the M-SURF level table, its tail, the serial restatement with ak_expf; then oracle/matching.c and acransac.c): `-m gpu`.

* r3dm_detect_akaze_msurf_batch: B images in one detector pass and ONE M-SURF launch == the chain and the single-image entry per image,
  with an image without keypoints in the middle of the batch and keypoint counts of every remainder mod the kernel's four keypoints per
  workgroup; `cap` below the count.  The (120, 160) images lose levels and keypoints to the M-SURF border: a build that detects on the
  MLDB table fails here;
* r3dm_set_descriptor_arm(R3DM_DESCRIPTOR_MSURF) on the features entries: the .desc of 64-float rows, skip rule, deferred files, sink (its
  pointer registered straight into a matcher), refusals, the device list;
* LIOP -> MSURF -> MLDB -> LIOP on one context writes a fresh context's files, byte for byte;
* the stage from pixels under R3DM_STAGE_DESCRIPTOR_MSURF against the chain, registered from the device and from files."""
import ctypes as C
import os
import shutil
import threading

import numpy as np
import pytest

import msurf_cases as S
from regard3d_amd import api
from stage_cases import _check_filter, _g

pytestmark = pytest.mark.gpu
BIG = (240, 320)
SMALL = (120, 160)
R3DM_ERR_INVALID, R3DM_ERR_UNSUPPORTED = -1, -5


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _paths(d, n, tag="v"):
    return [str(d / f"{tag}{k}.feat") for k in range(n)], [str(d / f"{tag}{k}.desc") for k in range(n)]


SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p)


def _hip_memcpy():
    """hipMemcpy of the HIP runtime libr3dm.so itself is linked to, so that the sink reads device memory through the runtime that allocated it"""
    fn = api.load_library().hipMemcpy
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    fn.restype = C.c_int
    return fn


class Sink:
    """a r3dm_features_sink that copies each image's rows back from the device while it runs (on the library's helper threads)"""

    def __init__(self, row_bytes):
        self.rows, self.lock, self.row_bytes, self.memcpy = {}, threading.Lock(), row_bytes, _hip_memcpy()
        self.fn = SINK(self._call)

    def _call(self, user, index, n, rows, xy):
        buf = np.zeros(n * self.row_bytes, np.uint8)
        rc = self.memcpy(buf.ctypes.data, rows, buf.size, 2) if n else 0        # 2 = hipMemcpyDeviceToHost
        with self.lock:
            self.rows[int(index)] = (int(n), buf.tobytes(), bool(rows))
        return 1 if rc else 0

    def attach(self, c):
        assert c._L.r3dm_set_features_sink(C.c_void_p(c._h), self.fn, None) == 0

    @staticmethod
    def detach(c):
        assert c._L.r3dm_set_features_sink(C.c_void_p(c._h), None, None) == 0


@pytest.fixture(scope="module")
def refs(oracle):
    """size -> (threshold, images, per image the reference chain's result): computed once, never changed"""
    return {size: S.batch_refs(size) for size in S.SIZES}


# ---- 1. the batch entry against the chain and the single-image entry
@pytest.mark.parametrize("which", ["four", "one"])
@pytest.mark.parametrize("size", S.SIZES)
def test_msurf_batch_equals_the_reference_chain_and_the_single_entry(ctx, refs, size, which):
    thr, ims, ref = refs[size]
    n = [len(r["kps"]) for r in ref]
    assert n[S.BLANK_INDEX] == 0 and sorted(k % S.KP_PER_GROUP for b, k in enumerate(n) if b != S.BLANK_INDEX) == [1, 2, 3]   # the case keeps its purpose
    batches = [list(range(4))] if which == "four" else [[0], [S.BLANK_INDEX], [2], [3]]
    for idx in batches:
        res = ctx.detect_akaze_msurf_batch([ims[b] for b in idx], thr)
        assert len(res) == len(idx)
        for (kps, rows), b in zip(res, idx):
            assert kps.shape == ref[b]["kps"].shape and rows.shape == ref[b]["rows"].shape, (b, kps.shape, ref[b]["kps"].shape)
            assert kps.tobytes() == ref[b]["kps"].tobytes(), b
            assert S.same_rows(rows, ref[b]["rows"]) and np.isfinite(rows).all(), b
            k1, r1 = ctx.detect_akaze_msurf_batch([ims[b]], thr, single=True)[0]
            assert k1.tobytes() == kps.tobytes() and r1.tobytes() == rows.tobytes(), b


def test_msurf_detection_is_not_the_mldb_arms_on_small_images(ctx, refs):
    """the border is the descriptor's: fewer keypoints than the MLDB entry finds on the same image, all of them inside the M-SURF border"""
    thr, ims, ref = refs[SMALL]
    km, _ = ctx.detect_akaze_mldb(ims[0], thr)
    ks, _ = ctx.detect_akaze_msurf_batch(ims[:1], thr)[0]
    assert len(ks) == len(ref[0]["kps"]) < len(km)


@pytest.mark.parametrize("size", S.SIZES)
def test_msurf_batch_cap_below_the_count_and_counts_only(ctx, refs, size):
    thr, ims, ref = refs[size]
    B, cap, room = 4, 7, 5
    kps = [np.full((cap + room, 4), np.float32(-7.5)) for _ in range(B)]
    desc = [np.full((cap + room, 64), np.float32(-3.25)) for _ in range(B)]
    ip = (C.c_void_p * B)(*[im.ctypes.data for im in ims])
    kp_p = (C.c_void_p * B)(*[k.ctypes.data for k in kps]); dp_p = (C.c_void_p * B)(*[d.ctypes.data for d in desc])
    n = np.zeros(B, np.uint32)
    assert ctx._L.r3dm_detect_akaze_msurf_batch(ctx._h, B, ip, size[1], size[0], thr, kp_p, dp_p, cap, n.ctypes.data) == 0
    for b in range(B):
        assert n[b] == len(ref[b]["kps"])                                              # the full count is reported
        w = min(cap, len(ref[b]["kps"]))
        assert kps[b][:w].tobytes() == ref[b]["kps"][:w].tobytes() and S.same_rows(desc[b][:w], ref[b]["rows"][:w]), b
        assert (kps[b][w:] == np.float32(-7.5)).all() and (desc[b][w:] == np.float32(-3.25)).all(), b       # nothing beyond the rows written
    assert min(len(r["kps"]) for b, r in enumerate(ref) if b != S.BLANK_INDEX) > cap
    n[:] = 0
    assert ctx._L.r3dm_detect_akaze_msurf_batch(ctx._h, B, ip, size[1], size[0], thr, None, None, 0, n.ctypes.data) == 0      # cap 0: counts only
    assert n.tolist() == [len(r["kps"]) for r in ref]


# ---- the features entries
@pytest.fixture(scope="module")
def raw_fctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture
def fctx(raw_fctx):
    """a features context of this module, handed out and taken back in the default state"""
    yield raw_fctx
    Sink.detach(raw_fctx)
    raw_fctx.set_deferred_feature_files(False)
    raw_fctx.set_keypoint_detector("Fast-AKAZE")
    raw_fctx.set_descriptor_arm("LIOP")


def _fresh_files(ims, thr, d, arm):
    """the (.feat, .desc) bytes a context that did nothing else writes for the batch under `arm`"""
    c = api.Context(0)
    try:
        c.set_descriptor_arm(arm)
        fp, dp = _paths(d, len(ims), arm.lower())
        nf = c.extract_features_batch(ims, fp, dp, thr)
    finally:
        c.close()
    return nf.tolist(), [(_read(fp[k]), _read(dp[k])) for k in range(len(ims))]


def _check_msurf_files(fp, dp, ref):
    for k in range(len(fp)):
        n, rows = S.desc_file(dp[k])
        assert n == len(ref[k]["kps"]) and S.same_rows(rows, ref[k]["rows"]), k
        if n == 0:
            assert os.path.getsize(fp[k]) == 0, k
            continue
        txt = np.loadtxt(fp[k], dtype=np.float32).reshape(-1, 4)                        # same .feat format as the Fast arm: x y size/2 angle
        want = ref[k]["kps"].copy(); want[:, 2] /= 2.0
        assert np.array_equal(txt, _g(want)), k


# ---- 2. files, skip rule, deferred files
@pytest.mark.parametrize("size", S.SIZES)
def test_msurf_arm_files_skip_rule_and_deferred_files(fctx, refs, tmp_path, size):
    thr, ims, ref = refs[size]
    fctx.set_descriptor_arm("MSURF")
    bat = tmp_path / "bat"; one = tmp_path / "one"; dfr = tmp_path / "dfr"
    for p in (bat, one, dfr):
        p.mkdir()
    fp, dp = _paths(bat, 4)
    nf = fctx.extract_features_batch(ims, fp, dp, thr)
    assert nf.tolist() == [len(r["kps"]) for r in ref]
    _check_msurf_files(fp, dp, ref)
    assert os.path.getsize(dp[S.BLANK_INDEX]) == 8 and os.path.getsize(fp[S.BLANK_INDEX]) == 0
    assert all(os.path.getsize(dp[k]) == 8 + 256 * nf[k] for k in range(4))
    # the one-image work item writes the same files, and leaves a pair that exists alone: mtime and bytes
    fo, do = _paths(one, 4)
    for k in range(4):
        assert fctx.extract_features_to_files(ims[k], fo[k], do[k], thr) == nf[k]
        assert (_read(fo[k]), _read(do[k])) == (_read(fp[k]), _read(dp[k])), k
    with open(fo[0], "wb") as f:
        f.write(b"1 2 3 4\n5 6 7 8\n")
    with open(do[0], "wb") as f:
        f.write(np.uint64(2).tobytes() + bytes(512))
    os.utime(fo[0], (1000, 1000)); os.utime(do[0], (2000, 2000))
    assert fctx.extract_features_to_files(ims[0], fo[0], do[0], thr) == 2              # rows of the existing .desc
    assert _read(fo[0]) == b"1 2 3 4\n5 6 7 8\n" and _read(do[0]) == np.uint64(2).tobytes() + bytes(512)
    assert os.stat(fo[0]).st_mtime == 1000 and os.stat(do[0]).st_mtime == 2000
    # deferred files are the same files
    fctx.set_deferred_feature_files(True)
    fd, dd = _paths(dfr, 4)
    nd = fctx.extract_features_batch(ims, fd, dd, thr)
    fctx.features_files_wait()
    assert nd.tolist() == nf.tolist()
    for k in range(4):
        assert (_read(fd[k]), _read(dd[k])) == (_read(fp[k]), _read(dp[k])), k


# ---- 3. switching arms on one context
def test_switching_arms_on_one_context_writes_a_fresh_contexts_files(refs, tmp_path):
    """LIOP -> MSURF -> MLDB -> LIOP, on the small images where the two level tables differ in their level count and on the big ones:
    no file depends on what the context computed before"""
    for size in (SMALL, BIG):
        thr, ims, ref = refs[size]
        d = tmp_path / f"s{size[0]}"; d.mkdir()
        fresh = {arm: _fresh_files(ims, thr, d, arm) for arm in ("LIOP", "MSURF", "MLDB")}
        assert fresh["MSURF"][0] == [len(r["kps"]) for r in ref]
        assert fresh["LIOP"][0] == fresh["MLDB"][0] and fresh["LIOP"][0] != fresh["MSURF"][0]
        c = api.Context(0)
        try:
            for step, arm in enumerate(("LIOP", "MSURF", "MLDB", "LIOP", "MSURF")):
                c.set_descriptor_arm(arm)
                fp, dp = _paths(d, 4, f"w{step}")
                nf = c.extract_features_batch(ims, fp, dp, thr)
                assert nf.tolist() == fresh[arm][0], (size, step, arm)
                assert [(_read(fp[k]), _read(dp[k])) for k in range(4)] == fresh[arm][1], (size, step, arm)
            # ... and the detect entries do not depend on the arm the context was left in
            k1, r1 = c.detect_akaze_msurf_batch(ims[:1], thr)[0]
            c.set_descriptor_arm("LIOP")
            k2, r2 = c.detect_akaze_msurf_batch(ims[:1], thr)[0]
            assert k1.tobytes() == k2.tobytes() == ref[0]["kps"].tobytes() and r1.tobytes() == r2.tobytes()
            km, _ = c.detect_akaze_mldb(ims[0], thr)
            assert len(km) == fresh["MLDB"][0][0]
        finally:
            c.close()


# ---- 4. the sink: the payload on the device, and its pointer registered straight into a matcher
@pytest.mark.parametrize("mode", ["immediate", "deferred"])
def test_msurf_arm_sink_sees_the_desc_payload_on_the_device(fctx, refs, tmp_path, mode):
    thr, ims, ref = refs[BIG]
    fctx.set_descriptor_arm("MSURF")
    fctx.set_deferred_feature_files(mode == "deferred")
    sink = Sink(256); sink.attach(fctx)
    fp, dp = _paths(tmp_path, 4)
    nf = fctx.extract_features_batch(ims, fp, dp, thr)
    if mode == "deferred":
        fctx.features_files_wait()
    assert sorted(sink.rows) == [0, 1, 2, 3]
    for k in range(4):
        n, rows, has_rows = sink.rows[k]
        assert n == nf[k] == len(ref[k]["kps"]) and has_rows == (n > 0)
        assert rows == _read(dp[k])[8:], k
        assert S.same_rows(np.frombuffer(rows, np.float32).reshape(-1, 64), ref[k]["rows"]), k


def test_sink_pointer_registers_straight_into_a_matcher(refs, tmp_path):
    """r3dm_set_image(dim 64, R3DM_F32) takes the sink's device pointer as it is: the putative graph of views registered that way equals
    the oracle's matcher on the restated rows"""
    thr, ims, ref = refs[BIG]
    views = [0, 2, 3]
    fc = api.Context(0); mc = api.Context(0)
    L = fc._L
    done, lock = {}, threading.Lock()

    def call(user, index, n, rows, xy):                                                # (from the library's helper threads: one registration at a time)
        with lock:
            done[int(index)] = L.r3dm_set_image(C.c_void_p(mc._h), C.c_uint32(int(index)), C.c_uint32(320), C.c_uint32(240), C.c_void_p(rows), C.c_uint32(n),
                                                C.c_uint32(64), api.F32, C.c_void_p(xy))
        return 0

    fn = SINK(call)
    try:
        fc.set_descriptor_arm("MSURF")
        assert L.r3dm_set_features_sink(C.c_void_p(fc._h), fn, None) == 0
        fp, dp = _paths(tmp_path, 3)
        fc.extract_features_batch([ims[v] for v in views], fp, dp, thr)
        assert done == {0: 0, 1: 0, 2: 0}
        pairs = np.array([[0, 1], [0, 2], [1, 2]], np.uint32)
        g = mc.match_pairs(pairs, 0.8, True)
        descs = [ref[v]["rows"] for v in views]; xys = [_g(ref[v]["kps"][:, :2]) for v in views]
        from oracle import pyoracle as O
        counts, matches = O.match_collection(descs, xys, pairs, 0.8, True)
        gp, gc, gm = _graph(g)
        assert np.array_equal(gp, pairs[counts > 0]) and np.array_equal(gc, counts[counts > 0]) and np.array_equal(gm, matches)
    finally:
        assert L.r3dm_set_features_sink(C.c_void_p(fc._h), None, None) == 0
        fc.close(); mc.close()


def _graph(g):
    """(pairs, counts, matches) of a match graph as the Python face hands it out"""
    return g.pairs.copy(), np.diff(g.offsets.astype(np.int64)).astype(np.uint32), g.matches.copy()


# ---- 5. refusals
def test_msurf_with_the_classic_detector_is_refused_by_name_and_leaves_nothing(fctx, refs, tmp_path):
    thr, ims, ref = refs[BIG]
    L, h = fctx._L, C.c_void_p(fctx._h)
    assert L.r3dm_set_descriptor_arm(h, 2) == R3DM_ERR_INVALID and L.r3dm_set_descriptor_arm(h, 4) == R3DM_ERR_INVALID
    assert L.r3dm_set_descriptor_arm(h, 3) == 0
    fctx.set_keypoint_detector("AKAZE")
    fp, dp = _paths(tmp_path, 4, "r")
    ip = (C.c_void_p * 4)(*[im.ctypes.data for im in ims])
    fpp = (C.c_char_p * 4)(*[p.encode() for p in fp]); dpp = (C.c_char_p * 4)(*[p.encode() for p in dp])
    nf = np.zeros(4, np.uint32)
    assert L.r3dm_extract_features_batch(h, 4, ip, None, 320, 240, C.c_float(thr), fpp, dpp, nf.ctypes.data) == R3DM_ERR_UNSUPPORTED
    assert "R3DM_DESCRIPTOR_MSURF" in L.r3dm_last_error(h).decode()
    n1 = C.c_uint32(5)
    assert L.r3dm_extract_features_to_files(h, ims[0].ctypes.data, 320, 240, C.c_float(thr), fpp[0], dpp[0], C.byref(n1)) == R3DM_ERR_UNSUPPORTED
    assert not any(os.path.exists(p) for p in fp + dp)
    # both switches are where the caller left them: the Fast detector makes the same call succeed
    fctx.set_keypoint_detector("Fast-AKAZE")
    assert fctx.extract_features_batch(ims, fp, dp, thr).tolist() == [len(r["kps"]) for r in ref]


# ---- 6. the device list
@pytest.mark.parametrize("n_ctx", [1, 2])
def test_msurf_arm_over_a_device_list(refs, tmp_path, n_ctx):
    thr, ims, ref = refs[BIG]
    m = api.MultiContext([0] * n_ctx)
    try:
        assert m._L.r3dm_multi_set_descriptor_arm(C.c_void_p(m._h), 2) == R3DM_ERR_INVALID
        m.set_descriptor_arm("MSURF")
        fp, dp = _paths(tmp_path, 4)
        nf, sk = m.extract_features(ims, fp, dp, thr, batch=2)
        assert nf.tolist() == [len(r["kps"]) for r in ref] and not sk.any()
        _check_msurf_files(fp, dp, ref)
        nf2, sk2 = m.extract_features(ims, fp, dp, thr, batch=2)                       # the skip rule: counts from the 64-float files
        assert sk2.all() and nf2.tolist() == nf.tolist()
        m.set_keypoint_detector("AKAZE")
        with pytest.raises(api.R3dmError, match="R3DM_DESCRIPTOR_MSURF"):
            m.extract_features(ims, *_paths(tmp_path, 4, "x"), thr)
        assert not os.path.exists(str(tmp_path / "x0.feat"))
    finally:
        m.close()


# ---- 7. the stage from pixels
def _views(ims, with_pixels=True):
    return [dict(id=k, width=320, height=240, basename=f"img{k:03d}", gray=ims[k] if with_pixels else None) for k in range(len(ims))]


def test_stage_from_pixels_on_the_msurf_arm_equals_the_reference_chain(oracle, tmp_path):
    """R3DM_STAGE_DESCRIPTOR_MSURF: pixels -> .feat / 64-float .desc -> float 2-NN with the squared ratio 0.8 -> F filter, registered from
    the device; then the same collection registered from its files.  Real-valued rows: the putative graph must equal the oracle's (every
    ratio decision of these views has a margin above 1e-5 d2, test_msurf_cases.py), the F graph by the helper of the LIOP stage tests."""
    ims = S.stage_images()
    refs_, descs, xys, pairs, counts, matches = S.oracle_stage(ims)
    W = np.full(4, 320, np.uint32); H = np.full(4, 240, np.uint32)
    oc, om = oracle.filter_F_collection(xys, W, H, pairs, counts, matches, 4.0, 2048, S.STAGE_FILTER_SEED)
    assert (oc > 0).sum() >= 3 and (counts > 0).all()                                 # the oracle alone keeps pairs through F
    d1 = tmp_path / "direct"; d2 = tmp_path / "files"; d1.mkdir(); d2.mkdir()
    rep = api.compute_matches_stage([0], str(d1), _views(ims), S.THR, S.STAGE_RATIO, 9, True, False, False, S.STAGE_FILTER_SEED, 2, 2, descriptor="MSURF")
    assert rep.descriptor_arm == api.DESCRIPTOR_ARMS["MSURF"] == 3 and rep.images_extracted == 4 and rep.match_was_exhaustive == 1
    assert rep.n_keypoints == sum(len(d) for d in descs)
    for k in range(4):
        n, rows = S.desc_file(str(d1 / f"img{k:03d}.desc"))
        assert n == len(descs[k]) and S.same_rows(rows, descs[k]), k
    p, c, m = oracle.load_matches(str(d1 / "matches.putative.txt"))
    assert np.array_equal(p, pairs[counts > 0]) and np.array_equal(c, counts[counts > 0]) and np.array_equal(m, matches)
    assert _check_filter(oracle, str(d1 / "matches.f.txt"), pairs, oc, om) == rep.n_F_pairs >= 3
    # registered from files: the views come with their .feat / .desc and without pixels
    for k in range(4):
        for ext in ("feat", "desc"):
            shutil.copy(str(d1 / f"img{k:03d}.{ext}"), str(d2 / f"img{k:03d}.{ext}"))
    rep2 = api.compute_matches_stage([0], str(d2), _views(ims, False), S.THR, S.STAGE_RATIO, 9, True, False, False, S.STAGE_FILTER_SEED, 2, 2, descriptor="MSURF")
    assert rep2.images_extracted == 0 and rep2.descriptor_arm == 3
    for name in ("matches.putative.txt", "matches.f.txt"):
        assert _read(str(d1 / name)) == _read(str(d2 / name)), name
    # the arm with the classic detector: refused by name, nothing written
    d3 = tmp_path / "refused"; d3.mkdir()
    with pytest.raises(api.R3dmError, match="R3DM_DESCRIPTOR_MSURF"):
        api.compute_matches_stage([0], str(d3), _views(ims), S.THR, S.STAGE_RATIO, 9, True, False, False, descriptor="MSURF", detector="AKAZE")
    assert not any(f.endswith((".feat", ".desc", ".txt", ".bin")) for f in os.listdir(str(d3)))
