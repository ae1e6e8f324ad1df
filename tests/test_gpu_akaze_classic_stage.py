"""Regard3D's default detector, classic A-KAZE ("AKAZE"), served end to end: the parallel kpts_aux walk, the
features entries with R3DM_DETECTOR_AKAZE, the stage with R3DM_STAGE_DETECTOR_AKAZE and the C++ facades with {"AKAZE"}.  Every result
is compared bit for bit: against the one-wavefront form of the walk (developer build), against the restatement
tests/akaze_classic_restatement.py + oracle LIOP, and against the oracle's matcher and filters on the restated features."""
import os
import subprocess
import sys

import numpy as np
import pytest

import akaze_classic_restatement as R
from regard3d_amd import api, synth
from test_gpu_akaze_classic import _scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _image(kind, seed=3):
    rng = np.random.default_rng(seed)
    if kind == "scene":
        return _scene(600, 800, seed, n_blobs=60)
    if kind == "noise":
        return np.clip(0.5 + rng.normal(0, 0.2, (500, 700)), 0, 1).astype(np.float32)
    if kind == "smooth":
        from scipy.ndimage import gaussian_filter
        return np.clip(0.5 + 4.0 * gaussian_filter(rng.normal(0, 0.2, (600, 800)), 1.2), 0, 1).astype(np.float32)
    return _scene(600, 800, 21, n_blobs=1500, noise=0.02, smin=1.5, smax=4.0)          # dense blobs


def _dev_detect(tmp_path, img, thr, env, tag):
    """the developer library in a child process (one at a time): the keypoints and responses of r3dm_detect_akaze_classic"""
    p = str(tmp_path / f"img_{tag}.npy")
    np.save(p, img)
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); import numpy as np; from regard3d_amd import api; api.use_developer_library(); "
            f"c = api.Context(0); k, r = c.detect_akaze_classic(np.load({p!r}), {thr!r}); "
            f"np.save({str(tmp_path / f'k_{tag}.npy')!r}, k); np.save({str(tmp_path / f'r_{tag}.npy')!r}, r)")
    r = subprocess.run([sys.executable, "-c", code], env=dict({k: v for k, v in os.environ.items() if not k.startswith("R3DM_")}, **env),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(str(tmp_path / f"k_{tag}.npy")), np.load(str(tmp_path / f"r_{tag}.npy"))


@pytest.mark.parametrize("thr", [0.001, 0.0001])
@pytest.mark.parametrize("kind", ["scene", "noise", "smooth", "dense"])
def test_parallel_walk_equals_the_one_wavefront_form(ctx, tmp_path, kind, thr):
    """the product (components in parallel, upper-level filter by cells) against the developer build's R3DM_AC_AUX=0 (one wavefront
    per image over every candidate, every later slot) and R3DM_AC_AUX_BOUND=1 (every component of two or more candidates handed back
    to the one-wavefront walk): keypoints, their order and responses identical"""
    img = _image(kind)
    kps, resp = ctx.detect_akaze_classic(img, thr)
    if kind != "scene" or thr < 0.001:
        assert len(kps) > 100
    for tag, env in (("serial", {"R3DM_AC_AUX": "0"}), ("handback", {"R3DM_AC_AUX_BOUND": "1"})):
        k2, r2 = _dev_detect(tmp_path, img, thr, env, tag)
        assert np.array_equal(k2, kps) and np.array_equal(r2, resp), tag
    hist = ctx.akaze_classic_components()
    assert hist[1:].sum() > 0                                     # components of two and more candidates were walked


@pytest.mark.parametrize("h,w,seed", [(480, 640, 7), (757, 999, 8)])
def test_parallel_walk_equals_the_restatement(ctx, oracle, h, w, seed):
    img = _scene(h, w, seed, n_blobs=max(4, h * w // 4000), noise=0.02, smin=1.5, smax=8.0)
    ref = R.detect(img, 0.0001)
    kps, resp = ctx.detect_akaze_classic(img, 0.0001)
    assert len(kps) == len(ref["kps"]) > 100
    assert np.array_equal(kps, ref["kps"]) and np.array_equal(resp, ref["responses"])


def _g(v):
    """the value a "%g" line of a .feat file holds (6 significant digits), as the loaders parse it back"""
    return np.array([np.float32(float("%g" % x)) for x in np.asarray(v, np.float32).ravel()], np.float32).reshape(np.shape(v))


def _restated(oracle, im, thr=0.001):
    kp = R.detect(im, thr)["kps"]
    d = oracle.liop_describe(oracle.liop_extract_patches(im, kp, 8.0)) if len(kp) else np.zeros((0, 144), np.float32)
    return kp, d


def _check_files(d, name, kp, desc):
    raw = np.fromfile(os.path.join(d, f"{name}.desc"), np.uint8)
    assert int(np.frombuffer(raw[:8].tobytes(), np.uint64)[0]) == len(kp)
    assert np.array_equal(np.frombuffer(raw[8:].tobytes(), np.float32).reshape(-1, 144), desc)
    txt = np.loadtxt(os.path.join(d, f"{name}.feat"), dtype=np.float32, ndmin=2).reshape(-1, 4)
    want = kp.copy(); want[:, 2] /= 2.0
    assert np.array_equal(txt, _g(want))


def _read(path):
    return open(path, "rb").read()


def test_features_entries_with_the_classic_arm(ctx, oracle, tmp_path):
    ims, _ = synth.make_photo_set(3, 360, 480, seed=31, device="cpu")
    ims = [im.numpy() for im in ims]
    ref = [_restated(oracle, im) for im in ims]
    assert min(len(r[0]) for r in ref) > 50
    c = api.Context(0)
    with pytest.raises(api.R3dmError):
        c._check(c._L.r3dm_set_keypoint_detector(c._h, 2), "r3dm_set_keypoint_detector")       # an unknown arm is refused
    c.set_keypoint_detector("AKAZE")
    one = tmp_path / "one"; bat = tmp_path / "bat"; bgrd = tmp_path / "bgr"; mul = tmp_path / "multi"; dfr = tmp_path / "deferred"
    for p in (one, bat, bgrd, mul, dfr):
        p.mkdir()
    # the one-image work item and the batch of three
    for k, im in enumerate(ims):
        assert c.extract_features_to_files(im, str(one / f"v{k}.feat"), str(one / f"v{k}.desc"), 0.001) == len(ref[k][0])
        _check_files(str(one), f"v{k}", *ref[k])
    nb = c.extract_features_batch(ims, [str(bat / f"v{k}.feat") for k in range(3)], [str(bat / f"v{k}.desc") for k in range(3)], 0.001)
    assert nb.tolist() == [len(r[0]) for r in ref]
    for k in range(3):
        for ext in ("feat", "desc"):
            assert _read(str(bat / f"v{k}.{ext}")) == _read(str(one / f"v{k}.{ext}"))
    # 8-bit BGR: converted on the device, the same as r3dm_gray_from_bgr8 then the gray entry
    rng = np.random.default_rng(4)
    bgr = [np.stack([np.clip(np.rint(im * 255) + rng.integers(-6, 7, im.shape), 0, 255).astype(np.uint8) for _ in range(3)], axis=2) for im in ims]
    grays = [c.gray_from_bgr8(b) for b in bgr]
    nbg = c.extract_features_batch(bgr, [str(bgrd / f"b{k}.feat") for k in range(3)], [str(bgrd / f"b{k}.desc") for k in range(3)], 0.001, bgr=True)
    kp0, d0 = _restated(oracle, grays[0])
    assert nbg[0] == len(kp0)
    _check_files(str(bgrd), "b0", kp0, d0)
    for k in range(3):
        assert c.extract_features_to_files(grays[k], str(bgrd / f"g{k}.feat"), str(bgrd / f"g{k}.desc"), 0.001) == nbg[k]
        for ext in ("feat", "desc"):
            assert _read(str(bgrd / f"b{k}.{ext}")) == _read(str(bgrd / f"g{k}.{ext}"))
    # deferred files: the same bytes once the writer is joined
    c.set_deferred_feature_files(True)
    c.extract_features_batch(ims, [str(dfr / f"v{k}.feat") for k in range(3)], [str(dfr / f"v{k}.desc") for k in range(3)], 0.001)
    c.features_files_wait()
    c.set_deferred_feature_files(False)
    for k in range(3):
        for ext in ("feat", "desc"):
            assert _read(str(dfr / f"v{k}.{ext}")) == _read(str(one / f"v{k}.{ext}"))
    # a blank image: empty files
    blank = np.full((360, 480), 0.3, np.float32)
    assert c.extract_features_to_files(blank, str(one / "blank.feat"), str(one / "blank.desc"), 0.001) == 0
    assert _read(str(one / "blank.feat")) == b"" and np.frombuffer(_read(str(one / "blank.desc")), np.uint64).tolist() == [0]
    # back to the default arm: the Fast arm's bytes, as a context that never switched writes them
    c.set_keypoint_detector("Fast-AKAZE")
    c.extract_features_to_files(ims[0], str(one / "fast.feat"), str(one / "fast.desc"), 0.001)
    ctx.extract_features_to_files(ims[0], str(one / "fast_ref.feat"), str(one / "fast_ref.desc"), 0.001)
    assert _read(str(one / "fast.desc")) == _read(str(one / "fast_ref.desc")) != _read(str(one / "v0.desc"))
    c.close()
    # four contexts, mixed sizes, the skip rule: byte-identical files, existing files left alone
    other, _ = synth.make_photo_set(2, 300, 440, seed=33, device="cpu")
    lst = ims + [o.numpy() for o in other]
    fp = [str(mul / f"m{k}.feat") for k in range(5)]; dp = [str(mul / f"m{k}.desc") for k in range(5)]
    open(fp[1], "w").close(); open(dp[1], "wb").write(np.uint64(7).tobytes())        # both files exist: skipped
    m = api.MultiContext([0, 0, 0, 0])
    m.set_keypoint_detector("AKAZE")
    nf, sk = m.extract_features(lst, fp, dp, 0.001, batch=2)
    m.close()
    assert sk.tolist() == [False, True, False, False, False] and nf[1] == 7
    for k in (0, 2):
        for ext in ("feat", "desc"):
            assert _read(str(mul / f"m{k}.{ext}")) == _read(str(one / f"v{k}.{ext}"))
    kp3, d3 = _restated(oracle, lst[3])
    _check_files(str(mul), "m3", kp3, d3)


def _oracle_stage(oracle, ims, dist_ratio=0.6):
    kps, descs, xys = [], [], []
    for im in ims:
        kp, d = _restated(oracle, im)
        kps.append(kp); descs.append(d); xys.append(_g(kp[:, :2]))
    i, j = np.triu_indices(len(ims), k=1)
    pairs = np.stack([i, j], axis=1).astype(np.uint32)
    counts, matches = oracle.match_collection(descs, xys, pairs, dist_ratio, True)
    return kps, descs, xys, pairs, counts, matches


def _check_filter(oracle, path, pairs, oc, om):
    p, c, m = oracle.load_matches(path)
    assert np.array_equal(p, pairs[oc > 0]) and np.array_equal(c, oc[oc > 0])
    off = 0; ooff = np.concatenate([[0], np.cumsum(np.asarray(oc, np.int64))]).astype(np.int64)
    for k, cnt in enumerate(c):
        seg = m[off:off + cnt]; off += cnt
        q = int(np.flatnonzero(oc > 0)[k])
        exp = om[int(ooff[q]):int(ooff[q]) + int(cnt)]
        assert set(map(tuple, seg.tolist())) == set(map(tuple, exp.tolist())), (path, k)
    return int((oc > 0).sum())


@pytest.fixture(scope="module")
def stage_case(oracle):
    h, w = 360, 480
    ims, K = synth.make_photo_set(4, h, w, seed=41, device="cpu")
    ims = [im.numpy() for im in ims]
    return ims, K, _oracle_stage(oracle, ims)


def _check_stage_dir(oracle, d, ims, case):
    kps, descs, xys, pairs, counts, matches = case
    h, w = ims[0].shape
    for k in range(len(ims)):
        _check_files(d, f"img{k:03d}", kps[k], descs[k])
    p, c, m = oracle.load_matches(os.path.join(d, "matches.putative.txt"))
    assert np.array_equal(p, pairs[counts > 0]) and np.array_equal(c, counts[counts > 0]) and np.array_equal(m, matches)
    W = np.full(len(ims), w, np.uint32); H = np.full(len(ims), h, np.uint32)
    oc, om = oracle.filter_F_collection(xys, W, H, pairs, counts, matches, 4.0, 2048, 5489)
    return int((counts > 0).sum()), _check_filter(oracle, os.path.join(d, "matches.f.txt"), pairs, oc, om)


def test_stage_with_the_classic_arm_equals_the_cpu_restatement(oracle, tmp_path, stage_case):
    ims, K, case = stage_case
    h, w = ims[0].shape
    views = [dict(id=k, width=w, height=h, basename=f"img{k:03d}", gray=ims[k], focal_px=K[0, 0], ppx=K[0, 2], ppy=K[1, 2]) for k in range(4)]
    d = str(tmp_path / "a"); os.mkdir(d)
    rep = api.compute_matches_stage([0], d, views, 0.001, 0.6, 9, True, False, False, 5489, 2, 2, detector="AKAZE")
    assert rep.images_extracted == 4 and rep.n_keypoints == sum(len(k) for k in case[0])
    n_put, n_f = _check_stage_dir(oracle, d, ims, case)
    assert n_put == rep.n_putative_pairs >= 1 and n_f == rep.n_F_pairs
    # one Stage object: Fast-AKAZE first, then AKAZE -- each arm's own files
    st = api.Stage([0])
    df = str(tmp_path / "fast"); da = str(tmp_path / "akaze"); dr = str(tmp_path / "fast_ref")
    for p in (df, da, dr):
        os.mkdir(p)
    st.run(df, views, 0.001, 0.6, 9, True, False, False)
    st.run(da, views, 0.001, 0.6, 9, True, False, False, detector="AKAZE")
    st.close()
    api.compute_matches_stage([0], dr, views, 0.001, 0.6, 9, True, False, False)
    for name in ("img000.feat", "img000.desc", "img003.desc", "matches.putative.txt", "matches.f.txt"):
        assert _read(os.path.join(da, name)) == _read(os.path.join(d, name)), name
        assert _read(os.path.join(df, name)) == _read(os.path.join(dr, name)), name
    assert _read(os.path.join(df, "img000.desc")) != _read(os.path.join(da, "img000.desc"))
    with pytest.raises(ValueError):
        api.compute_matches_stage([0], str(tmp_path), views, detector="MSER")


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "akaze_classic_host")
    lib = os.path.join(ROOT, "regard3d_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fopenmp", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "akaze_classic_host.cpp"), "-o", out,
                           "-L" + lib, "-lr3dm", "-Wl,-rpath," + lib])
    return out


def test_cpp_facades_with_the_classic_arm(oracle, tmp_path, host_exe, stage_case):
    ims, K, case = stage_case
    h, w = ims[0].shape
    paths = []
    for k, im in enumerate(ims):
        p = str(tmp_path / f"g{k}.f32"); np.ascontiguousarray(im, np.float32).tofile(p); paths.append(p)
    out = str(tmp_path / "feats.txt")
    r = subprocess.run([host_exe, "features", paths[0], str(w), str(h), out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = np.loadtxt(out, dtype=np.float32, ndmin=2)
    kp, desc = case[0][0], case[1][0]
    want = kp.copy(); want[:, 2] /= 2.0
    assert got.shape == (len(kp), 148) and np.array_equal(got[:, :4], want) and np.array_equal(got[:, 4:], desc)
    d = str(tmp_path / "stage"); os.mkdir(d)
    r = subprocess.run([host_exe, "stage", d, str(w), str(h)] + paths, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    _check_stage_dir(oracle, d, ims, case)
    d2 = str(tmp_path / "refuse"); os.mkdir(d2)
    r = subprocess.run([host_exe, "refuse", d2, str(w), str(h), paths[0]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
