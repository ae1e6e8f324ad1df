"""Images and case tables of the MLDB descriptor arm (r3dm_detect_akaze_mldb_batch, r3dm_set_descriptor_arm, R3DM_STAGE_DESCRIPTOR_MLDB).
TEST INFRASTRUCTURE ONLY, shared by test_gpu_mldb_arm.py and test_mldb_arm_cases.py (which holds the tables' promises against the CPU
restatement, without a GPU).

Small images on purpose: 240 x 320 has twelve evolution levels, 120 x 160 loses the upper ones to the border rule; the thresholds give
tens to a few hundred keypoints, so the oracle's part of a test stays well below a second per image."""
import numpy as np

THR = 0.001


def scene(h, w, seed, n_blobs=None, noise=0.01):
    """a smooth background with oriented Gaussian blobs of both signs and a little sensor noise, in [0, 1]"""
    rng = np.random.default_rng(seed)
    n_blobs = max(4, h * w // 1600) if n_blobs is None else n_blobs
    yy, xx = np.mgrid[0:h, 0:w]
    img = 0.5 + 0.1 * np.sin(xx / 17.0) * np.cos(yy / 23.0)
    mg = min(24, h // 5)
    for _ in range(n_blobs):
        cx, cy = rng.uniform(mg, w - mg), rng.uniform(mg, h - mg)
        s = rng.uniform(1.5, 7.0); a = rng.uniform(0.15, 0.45) * rng.choice([-1, 1])
        th = rng.uniform(0, np.pi); e = rng.uniform(1.0, 2.5)
        u = (xx - cx) * np.cos(th) + (yy - cy) * np.sin(th); v = -(xx - cx) * np.sin(th) + (yy - cy) * np.cos(th)
        img = img + a * np.exp(-(u * u / (2 * s * s * e) + v * v / (2 * s * s / e)))
    img = img + rng.normal(0, noise, img.shape)
    return np.clip(img, 0, 1).astype(np.float32)


def blank(h, w, value=0.25):
    return np.full((h, w), value, np.float32)


# size -> (threshold, blobs per scene, seeds of the two textured scenes, seed of the scene whose keypoint count at that threshold is
# ODD).  The batch of a size is [scene a, blank, scene b, odd scene]: the image without keypoints sits in the MIDDLE of the batch, the
# odd count makes the MLDB kernel's last wavefront hold one keypoint.  The small size needs a lower threshold for tens of keypoints.
# (test_mldb_arm_cases.py asserts the parities on the CPU, the GPU test asserts them again.)
BATCHES = {(240, 320): (THR, 48, (101, 102), 103), (120, 160): (0.0001, 40, (204, 206), 203)}


def batch_images(size):
    """-> (threshold, [scene a, blank, scene b, odd scene])"""
    h, w = size
    thr, nb, (a, b), odd = BATCHES[size]
    return thr, [scene(h, w, a, nb), blank(h, w), scene(h, w, b, nb), scene(h, w, odd, nb)]


ODD_INDEX = 3            # position of the odd-count scene in batch_images()
BLANK_INDEX = 1


# ---- the stage from pixels: four 240 x 320 views of one scene, shifted by a few pixels and with noise of their own, so that every
# pair of views overlaps almost completely (the oracle alone keeps pairs through the F filter: test_mldb_arm_cases.py)
STAGE_SEED = 301
STAGE_SHIFTS = [(0, 0), (5, 3), (9, 8), (3, 12)]          # (dy, dx) of the view's window inside the scene
STAGE_RATIO = 0.8
STAGE_FILTER_SEED = 5489


def stage_images():
    h, w, pad = 240, 320, 16
    rng = np.random.default_rng(STAGE_SEED + 1)
    big = scene(h + pad, w + pad, STAGE_SEED, n_blobs=90, noise=0.0).astype(np.float64)
    out = []
    for dy, dx in STAGE_SHIFTS:
        out.append(np.clip(big[dy:dy + h, dx:dx + w] + rng.normal(0, 0.004, (h, w)), 0, 1).astype(np.float32))
    return out


def g6(v):
    """the value a "%g" field of a .feat file holds (6 significant digits), as the loaders parse it back"""
    return np.array([np.float32(float("%g" % x)) for x in np.asarray(v, np.float32).ravel()], np.float32).reshape(np.shape(v))


def oracle_stage(oracle, ims):
    """the chain the stage serves under R3DM_STAGE_DESCRIPTOR_MLDB: akaze_detect_mldb per view, the exhaustive Hamming matcher with the
    facade's unsquared ratio on every pair, positions as the .feat text carries them"""
    kps, descs, xys = [], [], []
    for im in ims:
        kp, d, _ = oracle.akaze_detect_mldb(im, THR)
        kps.append(kp); descs.append(d); xys.append(g6(kp[:, :2]))
    i, j = np.triu_indices(len(ims), k=1)
    pairs = np.stack([i, j], axis=1).astype(np.uint32)
    counts, matches = oracle.match_collection(descs, xys, pairs, STAGE_RATIO, False, binary=True)
    return kps, descs, xys, pairs, counts, matches


def desc_file(path):
    """(count, rows [count, 61] uint8) of a binary .desc file"""
    raw = np.fromfile(path, np.uint8)
    n = int(np.frombuffer(raw[:8].tobytes(), np.uint64)[0])
    assert raw.size == 8 + 61 * n, (path, raw.size, n)
    return n, raw[8:].reshape(n, 61).copy()
