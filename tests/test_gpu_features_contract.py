"""What the features stage promises its callers, pinned for both detector arms (Fast-A-KAZE and classic A-KAZE): `-m gpu`.

* a blank image inside a batch: empty .feat, 8-byte .desc, no effect on its batch-mates -- immediately and with deferred files;
* an all-blank deferred batch followed at once by a normal one on the same context: one wait, both batches' files, no error left;
* the sink (r3dm_set_features_sink): once per image, the image's index, its count, a row pointer exactly when there are rows, the
  positions as the .feat file holds them -- on one context and through a multi-context's work list (the caller's indices);
* a sink that refuses an image: the error text, and which files exist;
* R3DM_LIOP_FUSED=0 (developer build) on the batch path: the same .desc bytes;
* the five detect entries: `cap` rows written, the full count reported, the single entry == element 0 of the batch entry.

Images of 240 x 320 and of 243 x 325: the odd size makes the octave transition a non-exact halving (the INTER_AREA tables)."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from regard3d_amd import api, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARMS = ["Fast-AKAZE", "AKAZE"]
SIZES = [(240, 320), (243, 325)]
MODES = ["immediate", "deferred"]
THR = 0.001


def _photos(size):
    ims, _ = synth.make_photo_set(3, size[0], size[1], seed=21 + size[0], device="cpu")
    return [np.ascontiguousarray(im.numpy(), np.float32) for im in ims]


def _read(path):
    return open(path, "rb").read()


def _paths(d, n, tag="v"):
    return [str(d / f"{tag}{k}.feat") for k in range(n)], [str(d / f"{tag}{k}.desc") for k in range(n)]


@pytest.fixture(scope="module")
def photos():
    return {s: _photos(s) for s in SIZES}


@pytest.fixture(scope="module")
def raw_ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture
def fctx(raw_ctx):
    """the module's context, handed out in its default state: Fast arm, immediate files, no sink"""
    yield raw_ctx
    raw_ctx._L.r3dm_set_features_sink(C.c_void_p(raw_ctx._h), None, None)
    raw_ctx._L.r3dm_set_deferred_feature_files(C.c_void_p(raw_ctx._h), 0)
    raw_ctx.set_keypoint_detector("Fast-AKAZE")


@pytest.fixture(scope="module")
def refs(raw_ctx, photos, tmp_path_factory):
    """(arm, size) -> per photograph the (.feat, .desc) bytes of the one-image work item: computed once, never changed"""
    d = tmp_path_factory.mktemp("one")
    out = {}
    for arm in ARMS:
        raw_ctx.set_keypoint_detector(arm)
        for s in SIZES:
            files = []
            for k, im in enumerate(photos[s]):
                fp, dp = str(d / f"{arm}_{s[0]}_{k}.feat"), str(d / f"{arm}_{s[0]}_{k}.desc")
                n = raw_ctx.extract_features_to_files(im, fp, dp, THR)
                assert n > 20, (arm, s, k, n)
                files.append((_read(fp), _read(dp)))
                assert np.frombuffer(files[-1][1][:8], np.uint64)[0] == n and len(files[-1][1]) == 8 + n * 144 * 4
            out[(arm, s)] = files
    raw_ctx.set_keypoint_detector("Fast-AKAZE")
    return out


def _blank(size):
    return np.full(size, 0.25, np.float32)


def _assert_blank_files(fp, dp):
    assert _read(fp) == b""
    assert _read(dp) == np.uint64(0).tobytes()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("arm", ARMS)
def test_blank_image_inside_a_batch(fctx, photos, refs, tmp_path, arm, size, mode):
    fctx.set_keypoint_detector(arm)
    fctx.set_deferred_feature_files(mode == "deferred")
    ims = [photos[size][0], _blank(size), photos[size][1]]
    fp, dp = _paths(tmp_path, 3)
    nf = fctx.extract_features_batch(ims, fp, dp, THR)
    if mode == "deferred":
        fctx.features_files_wait()
    assert nf[1] == 0
    _assert_blank_files(fp[1], dp[1])
    for b, k in ((0, 0), (2, 1)):
        assert (_read(fp[b]), _read(dp[b])) == refs[(arm, size)][k], (b, k)
        assert nf[b] == np.frombuffer(refs[(arm, size)][k][1][:8], np.uint64)[0]


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("arm", ARMS)
def test_all_blank_deferred_batch_then_a_normal_batch(fctx, photos, refs, tmp_path, arm, size):
    fctx.set_keypoint_detector(arm)
    fctx.set_deferred_feature_files(True)
    fa, da = _paths(tmp_path, 3, "blank")
    fb, db = _paths(tmp_path, 3, "photo")
    na = fctx.extract_features_batch([_blank(size)] * 3, fa, da, THR)
    nb = fctx.extract_features_batch(photos[size], fb, db, THR)
    fctx.features_files_wait()
    assert na.tolist() == [0, 0, 0]
    for k in range(3):
        _assert_blank_files(fa[k], da[k])
        assert (_read(fb[k]), _read(db[k])) == refs[(arm, size)][k], k
        assert nb[k] == np.frombuffer(refs[(arm, size)][k][1][:8], np.uint64)[0]
    fctx.features_files_wait()                                        # no error is pending: a second wait is as clean as the first
    fctx.set_deferred_feature_files(False)                            # (switching off joins the writer and reports its error, if any)


SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p)


class Sink:
    """a r3dm_features_sink that records its calls (it runs on the library's helper threads) and refuses the listed images"""

    def __init__(self, refuse=()):
        self.calls, self.lock, self.refuse = [], threading.Lock(), set(refuse)
        self.fn = SINK(self._call)

    def _call(self, user, index, n, rows, xy):
        pos = np.frombuffer(C.string_at(xy, 8 * n), np.float32).reshape(n, 2).copy() if n else np.zeros((0, 2), np.float32)
        with self.lock:
            self.calls.append((int(index), int(n), bool(rows), pos))
        return 1 if index in self.refuse else 0


def _feat_xy(path):
    if os.path.getsize(path) == 0:
        return np.zeros((0, 2), np.float32)
    return np.loadtxt(path, dtype=np.float32, ndmin=2).reshape(-1, 4)[:, :2]


def _assert_sink_calls(calls, nf, fp):
    assert sorted(c[0] for c in calls) == list(range(len(nf)))       # once per image, by its index
    for index, n, has_rows, pos in calls:
        assert n == nf[index]
        assert has_rows == (n > 0)
        assert np.array_equal(pos, _feat_xy(fp[index])), index


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("arm", ARMS)
def test_sink_sees_every_image_once(fctx, photos, tmp_path, arm, size, mode):
    fctx.set_keypoint_detector(arm)
    fctx.set_deferred_feature_files(mode == "deferred")
    sink = Sink()
    assert fctx._L.r3dm_set_features_sink(C.c_void_p(fctx._h), sink.fn, None) == 0
    ims = [photos[size][0], _blank(size), photos[size][1]]
    fp, dp = _paths(tmp_path, 3)
    nf = fctx.extract_features_batch(ims, fp, dp, THR)
    if mode == "deferred":
        fctx.features_files_wait()
    assert nf[0] > 0 and nf[1] == 0 and nf[2] > 0
    _assert_sink_calls(sink.calls, nf, fp)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("arm", ARMS)
def test_sink_of_a_work_list_sees_the_callers_indices(photos, refs, tmp_path, arm, mode):
    lst = photos[SIZES[0]] + photos[SIZES[1]][:2]                      # five images of two sizes over two contexts, batches of two
    m = api.MultiContext([0, 0])
    try:
        m.set_keypoint_detector(arm)
        m._check(m._L.r3dm_multi_set_deferred_feature_files(C.c_void_p(m._h), int(mode == "deferred")), "r3dm_multi_set_deferred_feature_files")
        sink = Sink()
        assert m._L.r3dm_multi_set_features_sink(C.c_void_p(m._h), sink.fn, None) == 0
        fp, dp = _paths(tmp_path, 5)
        nf, sk = m.extract_features(lst, fp, dp, THR, batch=2)
        if mode == "deferred":
            err = C.create_string_buffer(512)
            assert m._L.r3dm_multi_features_files_wait(C.c_void_p(m._h), err, 512) == 0, err.value
    finally:
        m.close()
    assert not sk.any()
    _assert_sink_calls(sink.calls, nf, fp)
    for k in range(5):
        assert (_read(fp[k]), _read(dp[k])) == refs[(arm, SIZES[k // 3])][k % 3], k


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("arm", ARMS)
def test_sink_refusal(fctx, photos, tmp_path, arm, size, mode):
    fctx.set_keypoint_detector(arm)
    fctx.set_deferred_feature_files(mode == "deferred")
    sink = Sink(refuse=[1])
    assert fctx._L.r3dm_set_features_sink(C.c_void_p(fctx._h), sink.fn, None) == 0
    fp, dp = _paths(tmp_path, 3)
    with pytest.raises(api.R3dmError, match="the features sink refused image 1"):
        fctx.extract_features_batch(photos[size], fp, dp, THR)
    if mode == "deferred":
        fctx.features_files_wait()                                    # reports no error
        assert not any(os.path.exists(p) for p in fp + dp)            # a failed deferred batch starts no writer
    else:
        assert all(os.path.exists(p) for p in fp + dp)                # the files were written before the sink was asked


def test_unfused_liop_on_the_batch_path_writes_the_same_descriptors(photos, refs, tmp_path):
    """R3DM_LIOP_FUSED=0 (developer build, in a child process): patch extraction and description as two launches through HBM"""
    for s in SIZES:
        np.save(str(tmp_path / f"ims{s[0]}.npy"), np.stack(photos[s]))
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); import numpy as np; from regard3d_amd import api; api.use_developer_library(); "
            f"c = api.Context(0); d = {str(tmp_path)!r}\n"
            f"for arm in {ARMS!r}:\n"
            f"    c.set_keypoint_detector(arm)\n"
            f"    for h in {[s[0] for s in SIZES]!r}:\n"
            f"        ims = list(np.load(d + '/ims%d.npy' % h))\n"
            f"        c.extract_features_batch(ims, [d + '/%s_%d_%d.feat' % (arm, h, k) for k in range(3)], [d + '/%s_%d_%d.desc' % (arm, h, k) for k in range(3)], {THR!r})\n")
    env = dict({k: v for k, v in os.environ.items() if not k.startswith("R3DM_")}, R3DM_LIOP_FUSED="0")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for arm in ARMS:
        for s in SIZES:
            for k in range(3):
                assert _read(str(tmp_path / f"{arm}_{s[0]}_{k}.desc")) == refs[(arm, s)][k][1], (arm, s, k)
                assert _read(str(tmp_path / f"{arm}_{s[0]}_{k}.feat")) == refs[(arm, s)][k][0], (arm, s, k)


def _detect_raw(c, entry, ims, cap, rows):
    """a detect entry called through the handle: buffers of `rows` rows filled with NaN, so that every row written shows"""
    L, h, w = c._L, ims[0].shape[0], ims[0].shape[1]
    B = len(ims)
    kps = [np.full((rows, 4), np.nan, np.float32) for _ in range(B)]
    resp = [np.full(rows, np.nan, np.float32) for _ in range(B)]
    n = np.zeros(B, np.uint32)
    hd = C.c_void_p(c._h)
    if entry in ("r3dm_detect_akaze_batch", "r3dm_detect_akaze_classic_batch"):
        ip = (C.c_void_p * B)(*[im.ctypes.data for im in ims])
        kp_p = (C.c_void_p * B)(*[k.ctypes.data for k in kps]); rp_p = (C.c_void_p * B)(*[r.ctypes.data for r in resp])
        rc = getattr(L, entry)(hd, B, ip, w, h, C.c_float(THR), kp_p, rp_p, cap, n.ctypes.data_as(C.POINTER(C.c_uint32)))
    elif entry == "r3dm_detect_akaze_mldb":
        resp = [np.full((rows, 61), 0xA5, np.uint8)]
        rc = L.r3dm_detect_akaze_mldb(hd, ims[0].ctypes.data_as(C.c_void_p), w, h, C.c_float(THR), kps[0].ctypes.data_as(C.c_void_p),
                                      resp[0].ctypes.data_as(C.c_void_p), cap, n.ctypes.data_as(C.POINTER(C.c_uint32)))
    else:
        rc = getattr(L, entry)(hd, ims[0].ctypes.data_as(C.c_void_p), w, h, C.c_float(THR), kps[0].ctypes.data_as(C.c_void_p),
                               resp[0].ctypes.data_as(C.c_void_p), cap, n.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert rc == 0, (entry, rc)
    return kps, resp, n


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("arm", ARMS)
def test_detect_entries_keep_cap_and_count(fctx, photos, arm, size):
    single, batch = ("r3dm_detect_akaze", "r3dm_detect_akaze_batch") if arm == "Fast-AKAZE" else ("r3dm_detect_akaze_classic", "r3dm_detect_akaze_classic_batch")
    ims = photos[size]
    CAP, ROWS = 7, 4096
    full_k, full_r, full_n = _detect_raw(fctx, batch, ims, ROWS, ROWS)
    assert all(CAP < int(n) < ROWS for n in full_n)
    for b in range(3):
        assert not np.isnan(full_k[b][:full_n[b]]).any() and np.isnan(full_k[b][full_n[b]:]).all()
        assert not np.isnan(full_r[b][:full_n[b]]).any() and np.isnan(full_r[b][full_n[b]:]).all()
    # cap below the count: exactly cap rows, the full count
    k, r, n = _detect_raw(fctx, batch, ims, CAP, ROWS)
    assert n.tolist() == full_n.tolist()
    for b in range(3):
        assert np.array_equal(k[b][:CAP], full_k[b][:CAP]) and np.isnan(k[b][CAP:]).all()
        assert np.array_equal(r[b][:CAP], full_r[b][:CAP]) and np.isnan(r[b][CAP:]).all()
    # the single entry == element 0 of the batch entry, responses included; and its cap
    k1, r1, n1 = _detect_raw(fctx, single, ims[:1], ROWS, ROWS)
    assert n1[0] == full_n[0] and np.array_equal(k1[0], full_k[0], equal_nan=True) and np.array_equal(r1[0], full_r[0], equal_nan=True)
    k1c, r1c, n1c = _detect_raw(fctx, single, ims[:1], CAP, ROWS)
    assert n1c[0] == full_n[0]
    assert np.array_equal(k1c[0][:CAP], full_k[0][:CAP]) and np.isnan(k1c[0][CAP:]).all()
    assert np.array_equal(r1c[0][:CAP], full_r[0][:CAP]) and np.isnan(r1c[0][CAP:]).all()
    if arm == "Fast-AKAZE":                                           # the fifth entry: keypoints + MLDB rows
        km, dm, nm = _detect_raw(fctx, "r3dm_detect_akaze_mldb", ims[:1], ROWS, ROWS)
        assert nm[0] == full_n[0] and np.array_equal(km[0], full_k[0], equal_nan=True)
        assert (dm[0][nm[0]:] == 0xA5).all()
        kc, dc, nc = _detect_raw(fctx, "r3dm_detect_akaze_mldb", ims[:1], CAP, ROWS)
        assert nc[0] == full_n[0]
        assert np.array_equal(kc[0][:CAP], full_k[0][:CAP]) and np.isnan(kc[0][CAP:]).all()
        assert np.array_equal(dc[0][:CAP], dm[0][:CAP]) and (dc[0][CAP:] == 0xA5).all()
