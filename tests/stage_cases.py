"""The CPU restatement of the stage from pixels (Fast-A-KAZE -> LIOP -> 2-NN + ratio) and the comparison of a filter's match file with
the oracle's collection result.  TEST INFRASTRUCTURE ONLY, shared by test_gpu_stage.py and test_gpu_filter_views.py."""
import numpy as np


def _g(v):
    """the value a "%g" line of a .feat file holds (6 significant digits), as the loaders parse it back"""
    return np.array([np.float32(float("%g" % x)) for x in np.asarray(v, np.float32).ravel()], np.float32).reshape(np.shape(v))


def _oracle_stage(oracle, ims, K, dist_ratio=0.6):
    kps, descs, xys = [], [], []
    for im in ims:
        kp = oracle.akaze_detect(im, 0.001)["kps"]
        d = oracle.liop_describe(oracle.liop_extract_patches(im, kp, 8.0))
        kps.append(kp); descs.append(d); xys.append(_g(kp[:, :2]))                    # positions as the .feat text carries them
    n = len(ims)
    i, j = np.triu_indices(n, k=1)
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
