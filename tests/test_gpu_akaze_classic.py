"""GPU parity of the classic A-KAZE detector (r3dm_detect_akaze_classic, Regard3D's "AKAZE" arm) against the CPU restatement
tests/akaze_classic_restatement.py (libAKAZE).  The determinism rules of tests/test_gpu_akaze.py apply: the
device uses + - * / sqrt in float without contraction, double where libAKAZE's expression is double, and the host forms the evolution
table and the FED steps with the same libm as the restatement, so keypoints, sizes, angles and responses are compared BIT-EXACTLY."""
import numpy as np
import pytest

import akaze_classic_restatement as R

pytestmark = pytest.mark.gpu


def _scene(h, w, seed, n_blobs=40, noise=0.01, smin=2.0, smax=12.0):
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
    return np.clip(img, 0, 1).astype(np.float32)


def _same(got, ref):
    kps, resp = got
    assert len(kps) == len(ref["kps"])
    assert np.array_equal(resp, ref["responses"])
    assert np.array_equal(kps, ref["kps"])


@pytest.mark.parametrize("thr", [0.001, 0.0001])
@pytest.mark.parametrize("h,w,seed", [(480, 640, 1), (757, 999, 2), (120, 160, 5), (60, 90, 6), (1500, 2000, 4)])
def test_detector_equals_the_restatement(ctx, oracle, h, w, seed, thr):
    img = _scene(h, w, seed, n_blobs=max(4, h * w // 8000))
    ref = R.detect(img, thr)
    _same(ctx.detect_akaze_classic(img, thr), ref)
    if h >= 400:
        assert len(ref["kps"]) > 20


def test_dense_blobs_form_large_components(ctx, oracle):
    """many small blobs close together: long runs of kpts_aux hits and replacements across neighbouring levels"""
    img = _scene(600, 800, 21, n_blobs=1500, noise=0.02, smin=1.5, smax=4.0)
    ref = R.detect(img, 0.0001)
    assert len(ref["kps"]) > 300
    _same(ctx.detect_akaze_classic(img, 0.0001), ref)


@pytest.mark.parametrize("h,w", [(480, 640), (757, 999)])
def test_batch_equals_single(ctx, oracle, h, w):
    """757 x 999: every octave transition is an INTER_AREA table (no exact halving), shared by the batch"""
    imgs = [_scene(h, w, 30 + b, n_blobs=max(4, h * w // 8000)) for b in range(3)]
    out = ctx.detect_akaze_classic_batch(imgs, 0.001)
    for b, im in enumerate(imgs):
        k1, r1 = ctx.detect_akaze_classic(im, 0.001)
        assert np.array_equal(out[b][0], k1) and np.array_equal(out[b][1], r1)
    _same(out[1], R.detect(imgs[1], 0.001))
    _same(out[2], R.detect(imgs[2], 0.001))


def test_blank_image_gives_nothing(ctx):
    kps, resp = ctx.detect_akaze_classic(np.full((300, 400), 0.5, np.float32), 0.001)
    assert len(kps) == 0 and len(resp) == 0


def test_cap_smaller_than_the_count(ctx, oracle):
    img = _scene(480, 640, 1, n_blobs=38)
    full, _ = ctx.detect_akaze_classic(img, 0.0001)
    part, _ = ctx.detect_akaze_classic(img, 0.0001, cap=5)
    assert len(full) > 5 and np.array_equal(part, full[:5])
