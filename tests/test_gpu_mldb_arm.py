"""The MLDB-486 descriptor arm from the kernel to the stage, bit-exact against the CPU restatement (oracle/akaze.c, matching.c,
acransac.c): `-m gpu`.

* r3dm_detect_akaze_mldb_batch: B images in one detector pass and ONE MLDB launch == the oracle and the single-image entry per image,
  with an image without keypoints in the middle of the batch and an odd keypoint count (the kernel holds two keypoints per wavefront);
  `cap` below the count;
* r3dm_set_descriptor_arm on the features entries: the .desc of 61-byte rows, the .feat of the LIOP arm, skip rule, deferred files, sink,
  refusals, the device list;
* the default arm untouched by the switch;
* the stage from pixels under R3DM_STAGE_DESCRIPTOR_MLDB against the oracle chain, registered from the device and from files.

Images: tests/mldb_arm_cases.py (240 x 320 and 120 x 160, tens of keypoints each)."""
import ctypes as C
import os
import shutil
import threading

import numpy as np
import pytest

import mldb_arm_cases as M
from regard3d_amd import api

pytestmark = pytest.mark.gpu
SIZES = sorted(M.BATCHES)
BIG = (240, 320)
R3DM_ERR_INVALID, R3DM_ERR_UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def refs(oracle):
    """size -> (threshold, images, per image the oracle's (keypoints, descriptors)): computed once, never changed"""
    out = {}
    for size in SIZES:
        thr, ims = M.batch_images(size)
        out[size] = (thr, ims, [oracle.akaze_detect_mldb(im, thr)[:2] for im in ims])
    return out


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _paths(d, n, tag="v"):
    return [str(d / f"{tag}{k}.feat") for k in range(n)], [str(d / f"{tag}{k}.desc") for k in range(n)]


# ---- 1. the batch entry against the oracle and the single-image entry
@pytest.mark.parametrize("which", ["four", "one"])
@pytest.mark.parametrize("size", SIZES)
def test_mldb_batch_equals_the_cpu_restatement_and_the_single_entry(ctx, refs, size, which):
    thr, ims, ref = refs[size]
    assert len(ref[M.ODD_INDEX][0]) % 2 == 1 and len(ref[M.BLANK_INDEX][0]) == 0        # the case keeps its purpose
    assert all(len(ref[b][0]) >= 30 for b in range(4) if b != M.BLANK_INDEX)
    batches = [list(range(4))] if which == "four" else [[M.ODD_INDEX], [M.BLANK_INDEX], [0]]
    for idx in batches:
        res = ctx.detect_akaze_mldb_batch([ims[b] for b in idx], thr)
        assert len(res) == len(idx)
        for (kps, desc), b in zip(res, idx):
            okp, odesc = ref[b]
            assert kps.shape == okp.shape and desc.shape == odesc.shape, (b, kps.shape, okp.shape)
            assert np.array_equal(kps, okp), b
            assert np.array_equal(desc, odesc), b
            assert not (desc[:, 60] & 0xC0).any()                                      # 486 bits: the top two of byte 60 stay clear
            k1, d1 = ctx.detect_akaze_mldb(ims[b], thr)
            assert np.array_equal(k1, kps) and np.array_equal(d1, desc), b


def test_mldb_batch_reports_counts_of_every_image(ctx, refs):
    thr, ims, ref = refs[BIG]
    B = 4
    ip = (C.c_void_p * B)(*[im.ctypes.data for im in ims])
    n = np.zeros(B, np.uint32)
    assert ctx._L.r3dm_detect_akaze_mldb_batch(ctx._h, B, ip, 320, 240, thr, None, None, 0, n.ctypes.data) == 0      # cap 0: counts only
    assert n.tolist() == [len(r[0]) for r in ref]


# ---- 2. cap below the count
@pytest.mark.parametrize("size", SIZES)
def test_mldb_batch_cap_below_the_count(ctx, refs, size):
    thr, ims, ref = refs[size]
    B, cap, room = 4, 7, 5
    kps = [np.full((cap + room, 4), np.float32(-7.5)) for _ in range(B)]
    desc = [np.full((cap + room, 61), 0xA5, np.uint8) for _ in range(B)]
    ip = (C.c_void_p * B)(*[im.ctypes.data for im in ims])
    kp_p = (C.c_void_p * B)(*[k.ctypes.data for k in kps]); dp_p = (C.c_void_p * B)(*[d.ctypes.data for d in desc])
    n = np.zeros(B, np.uint32)
    assert ctx._L.r3dm_detect_akaze_mldb_batch(ctx._h, B, ip, size[1], size[0], thr, kp_p, dp_p, cap, n.ctypes.data) == 0
    for b in range(B):
        okp, odesc = ref[b]
        assert n[b] == len(okp)                                                        # the full count is reported
        w = min(cap, len(okp))
        assert np.array_equal(kps[b][:w], okp[:w]) and np.array_equal(desc[b][:w], odesc[:w]), b
        assert (kps[b][w:] == np.float32(-7.5)).all() and (desc[b][w:] == 0xA5).all(), b       # nothing beyond the rows written
    assert min(len(r[0]) for b, r in enumerate(ref) if b != M.BLANK_INDEX) > cap


# ---- the features entries
def _hip_memcpy():
    """hipMemcpy of the HIP runtime libr3dm.so itself is linked to (looked up through the library's handle: its dependencies are searched),
    so that the sink reads device memory through the runtime that allocated it"""
    fn = api.load_library().hipMemcpy
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    fn.restype = C.c_int
    return fn


SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p)


class Sink:
    """a r3dm_features_sink that copies each image's rows back from the device while it runs (on the library's helper threads)"""

    def __init__(self, row_bytes):
        self.rows, self.threads, self.lock, self.row_bytes, self.memcpy = {}, set(), threading.Lock(), row_bytes, _hip_memcpy()
        self.fn = SINK(self._call)

    def _call(self, user, index, n, rows, xy):
        buf = np.zeros(n * self.row_bytes, np.uint8)
        rc = self.memcpy(buf.ctypes.data, rows, buf.size, 2) if n else 0        # 2 = hipMemcpyDeviceToHost
        with self.lock:
            self.rows[int(index)] = (int(n), buf.tobytes(), bool(rows))
            self.threads.add(threading.get_ident())
        return 1 if rc else 0

    def attach(self, c):
        assert c._L.r3dm_set_features_sink(C.c_void_p(c._h), self.fn, None) == 0

    @staticmethod
    def detach(c):
        assert c._L.r3dm_set_features_sink(C.c_void_p(c._h), None, None) == 0


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


@pytest.fixture(scope="module")
def liop_ref(refs, tmp_path_factory):
    """the LIOP arm on a context that never touches the descriptor switch: (.feat, .desc) bytes and the sink's rows of the big batch"""
    d = tmp_path_factory.mktemp("liop_ref")
    _, ims, _ = refs[BIG]
    c = api.Context(0)
    sink = Sink(144 * 4); sink.attach(c)
    fp, dp = _paths(d, 4)
    nf = c.extract_features_batch(ims, fp, dp, M.THR)
    c.close()
    return dict(files=[(_read(fp[k]), _read(dp[k])) for k in range(4)], sink=dict(sink.rows), nf=nf.tolist())


def _check_mldb_files(fp, dp, ref, liop_files):
    for k in range(len(fp)):
        n, rows = M.desc_file(dp[k])
        assert n == len(ref[k][0]) and np.array_equal(rows, ref[k][1]), k
        assert _read(fp[k]) == liop_files[k][0], k                                     # the .feat of the LIOP arm, byte for byte


# ---- 3. files
def test_mldb_arm_files_skip_rule_and_deferred_files(fctx, refs, liop_ref, tmp_path):
    thr, ims, ref = refs[BIG]
    fctx.set_descriptor_arm("MLDB")
    bat = tmp_path / "bat"; one = tmp_path / "one"; dfr = tmp_path / "dfr"
    for p in (bat, one, dfr):
        p.mkdir()
    fp, dp = _paths(bat, 4)
    nf = fctx.extract_features_batch(ims, fp, dp, thr)
    assert nf.tolist() == [len(r[0]) for r in ref] == liop_ref["nf"]
    _check_mldb_files(fp, dp, ref, liop_ref["files"])
    assert os.path.getsize(dp[M.BLANK_INDEX]) == 8 and os.path.getsize(fp[M.BLANK_INDEX]) == 0
    # the one-image work item writes the same files, and leaves a pair that exists alone: mtime and bytes
    fo, do = _paths(one, 4)
    for k in range(4):
        assert fctx.extract_features_to_files(ims[k], fo[k], do[k], thr) == nf[k]
        assert (_read(fo[k]), _read(do[k])) == (_read(fp[k]), _read(dp[k])), k
    with open(fo[0], "wb") as f:
        f.write(b"1 2 3 4\n")
    with open(do[0], "wb") as f:
        f.write(np.uint64(1).tobytes() + bytes(61))
    os.utime(fo[0], (1000, 1000)); os.utime(do[0], (2000, 2000))
    assert fctx.extract_features_to_files(ims[0], fo[0], do[0], thr) == 1              # rows of the existing .desc
    assert _read(fo[0]) == b"1 2 3 4\n" and _read(do[0]) == np.uint64(1).tobytes() + bytes(61)
    assert os.stat(fo[0]).st_mtime == 1000 and os.stat(do[0]).st_mtime == 2000
    # deferred files are the same files
    fctx.set_deferred_feature_files(True)
    fd, dd = _paths(dfr, 4)
    nd = fctx.extract_features_batch(ims, fd, dd, thr)
    fctx.features_files_wait()
    assert nd.tolist() == nf.tolist()
    for k in range(4):
        assert (_read(fd[k]), _read(dd[k])) == (_read(fp[k]), _read(dp[k])), k


# ---- 4. the default arm
def test_default_arm_is_untouched_by_the_switch(refs, liop_ref, tmp_path):
    thr, ims, ref = refs[BIG]
    c = api.Context(0)
    try:
        c.set_descriptor_arm("MLDB")
        fp, dp = _paths(tmp_path, 4, "m")
        c.extract_features_batch(ims, fp, dp, thr)
        c.set_descriptor_arm("LIOP")
        sink = Sink(144 * 4); sink.attach(c)
        fp, dp = _paths(tmp_path, 4, "l")
        nf = c.extract_features_batch(ims, fp, dp, thr)
    finally:
        c.close()
    assert nf.tolist() == liop_ref["nf"]
    assert [(_read(fp[k]), _read(dp[k])) for k in range(4)] == liop_ref["files"]
    assert sink.rows == liop_ref["sink"]
    for k in range(4):                                                                 # (and the reference itself: the .desc payload is what its sink saw)
        assert liop_ref["sink"][k][1] == liop_ref["files"][k][1][8:], k


# ---- 6. the sink
@pytest.mark.parametrize("mode", ["immediate", "deferred"])
def test_mldb_arm_sink_sees_the_desc_payload_on_the_device(fctx, refs, tmp_path, mode):
    thr, ims, ref = refs[BIG]
    fctx.set_descriptor_arm("MLDB")
    fctx.set_deferred_feature_files(mode == "deferred")
    sink = Sink(61); sink.attach(fctx)
    fp, dp = _paths(tmp_path, 4)
    nf = fctx.extract_features_batch(ims, fp, dp, thr)
    if mode == "deferred":
        fctx.features_files_wait()
    assert sorted(sink.rows) == [0, 1, 2, 3]
    for k in range(4):
        n, rows, has_rows = sink.rows[k]
        assert n == nf[k] == len(ref[k][0]) and has_rows == (n > 0)
        assert rows == _read(dp[k])[8:] == ref[k][1].tobytes(), k


# ---- 7. refusals and history
def test_descriptor_arm_refusals_leave_nothing_behind(fctx, refs, liop_ref, tmp_path):
    thr, ims, ref = refs[BIG]
    L, h = fctx._L, C.c_void_p(fctx._h)
    for bad in (2, -1):
        assert L.r3dm_set_descriptor_arm(h, bad) == R3DM_ERR_INVALID
    fctx.set_descriptor_arm("MLDB")
    fctx.set_keypoint_detector("AKAZE")
    fp, dp = _paths(tmp_path, 4, "r")
    ip = (C.c_void_p * 4)(*[im.ctypes.data for im in ims])
    fpp = (C.c_char_p * 4)(*[p.encode() for p in fp]); dpp = (C.c_char_p * 4)(*[p.encode() for p in dp])
    nf = np.zeros(4, np.uint32)
    assert L.r3dm_extract_features_batch(h, 4, ip, None, 320, 240, C.c_float(thr), fpp, dpp, nf.ctypes.data) == R3DM_ERR_UNSUPPORTED
    assert "R3DM_DESCRIPTOR_MLDB" in L.r3dm_last_error(h).decode()
    n1 = C.c_uint32(5)
    assert L.r3dm_extract_features_to_files(h, ims[0].ctypes.data, 320, 240, C.c_float(thr), fpp[0], dpp[0], C.byref(n1)) == R3DM_ERR_UNSUPPORTED
    assert not any(os.path.exists(p) for p in fp + dp)
    # both switches are where the caller left them: the Fast detector makes the same call succeed, the classic one with LIOP too
    fctx.set_keypoint_detector("Fast-AKAZE")
    assert fctx.extract_features_batch(ims, fp, dp, thr).tolist() == [len(r[0]) for r in ref]
    fctx.set_keypoint_detector("AKAZE"); fctx.set_descriptor_arm("LIOP")
    fctx.extract_features_batch(ims[:1], fp[:1], dp[:1], thr)
    # ... and the next LIOP call equals a fresh context's
    fctx.set_keypoint_detector("Fast-AKAZE")
    fl, dl = _paths(tmp_path, 4, "l")
    assert fctx.extract_features_batch(ims, fl, dl, thr).tolist() == liop_ref["nf"]
    assert [(_read(fl[k]), _read(dl[k])) for k in range(4)] == liop_ref["files"]


# ---- 8. the device list
@pytest.mark.parametrize("n_ctx", [1, 2])
def test_mldb_arm_over_a_device_list(refs, liop_ref, tmp_path, n_ctx):
    thr, ims, ref = refs[BIG]
    thr_s, ims_s, ref_s = refs[(120, 160)]
    m = api.MultiContext([0] * n_ctx)
    try:
        assert m._L.r3dm_multi_set_descriptor_arm(C.c_void_p(m._h), 2) == R3DM_ERR_INVALID
        m.set_descriptor_arm("MLDB")
        fp, dp = _paths(tmp_path, 4)
        nf, sk = m.extract_features(ims, fp, dp, thr, batch=2)
        assert nf.tolist() == [len(r[0]) for r in ref] and not sk.any()
        _check_mldb_files(fp, dp, ref, liop_ref["files"])
        nf2, sk2 = m.extract_features(ims, fp, dp, thr, batch=2)                       # the skip rule: counts from the 61-byte files
        assert sk2.all() and nf2.tolist() == nf.tolist()
        m.set_keypoint_detector("AKAZE")
        with pytest.raises(api.R3dmError, match="R3DM_DESCRIPTOR_MLDB"):
            m.extract_features(ims, *_paths(tmp_path, 4, "x"), thr)
        assert not os.path.exists(str(tmp_path / "x0.feat"))
    finally:
        m.close()


# ---- 5. the stage from pixels
def _views(ims, with_pixels=True):
    return [dict(id=k, width=320, height=240, basename=f"img{k:03d}", gray=ims[k] if with_pixels else None) for k in range(len(ims))]


def test_stage_from_pixels_on_the_mldb_arm_equals_the_cpu_restatement(oracle, tmp_path):
    """R3DM_STAGE_DESCRIPTOR_MLDB: pixels -> .feat / 61-byte .desc -> Hamming 2-NN with the unsquared ratio 0.8 -> F filter, registered from
    the device; then the same collection registered from its files"""
    ims = M.stage_images()
    kps, descs, xys, pairs, counts, matches = M.oracle_stage(oracle, ims)
    W = np.full(4, 320, np.uint32); H = np.full(4, 240, np.uint32)
    oc, om = oracle.filter_F_collection(xys, W, H, pairs, counts, matches, 4.0, 2048, M.STAGE_FILTER_SEED)
    assert (oc > 0).sum() >= 1 and (counts > 0).all()                                 # the oracle alone keeps pairs through F
    d1 = tmp_path / "direct"; d2 = tmp_path / "files"; d1.mkdir(); d2.mkdir()
    rep = api.compute_matches_stage([0], str(d1), _views(ims), M.THR, M.STAGE_RATIO, 9, True, False, False, M.STAGE_FILTER_SEED, 2, 2, descriptor="MLDB")
    assert rep.descriptor_arm == api.DESCRIPTORS["MLDB"] and rep.images_extracted == 4 and rep.match_was_exhaustive == 1
    assert rep.n_keypoints == sum(len(k) for k in kps)
    for k in range(4):
        n, rows = M.desc_file(str(d1 / f"img{k:03d}.desc"))
        assert n == len(kps[k]) and np.array_equal(rows, descs[k]), k
    p, c, m = oracle.load_matches(str(d1 / "matches.putative.txt"))
    assert np.array_equal(p, pairs[counts > 0]) and np.array_equal(c, counts[counts > 0]) and np.array_equal(m, matches)
    pf, cf, mf = oracle.load_matches(str(d1 / "matches.f.txt"))
    assert np.array_equal(pf, pairs[oc > 0]) and np.array_equal(cf, oc[oc > 0])
    off = np.concatenate([[0], np.cumsum(oc.astype(np.int64))])
    got = 0
    for q in np.flatnonzero(oc > 0):
        seg = mf[got:got + int(oc[q])]; got += int(oc[q])
        assert set(map(tuple, seg.tolist())) == set(map(tuple, om[off[q]:off[q + 1]].tolist())), q
    assert rep.n_F_pairs == int((oc > 0).sum())
    # registered from files: the views come with their .feat / .desc and without pixels
    for k in range(4):
        for ext in ("feat", "desc"):
            shutil.copy(str(d1 / f"img{k:03d}.{ext}"), str(d2 / f"img{k:03d}.{ext}"))
    rep2 = api.compute_matches_stage([0], str(d2), _views(ims, False), M.THR, M.STAGE_RATIO, 9, True, False, False, M.STAGE_FILTER_SEED, 2, 2, descriptor="MLDB")
    assert rep2.images_extracted == 0 and rep2.descriptor_arm == api.DESCRIPTORS["MLDB"]
    for name in ("matches.putative.txt", "matches.f.txt"):
        assert _read(str(d1 / name)) == _read(str(d2 / name)), name
