"""The promises of tests/mldb_arm_cases.py, held against the CPU restatement without a GPU: each batch has an image without keypoints in
its middle and a scene with an ODD keypoint count, tens of keypoints per textured scene, the small size loses evolution levels, and the
stage's scene keeps pairs through the oracle's own F filter."""
import numpy as np
import pytest

import mldb_arm_cases as M


@pytest.mark.parametrize("size", sorted(M.BATCHES))
def test_batch_tables_keep_their_purpose(oracle, size):
    thr, ims = M.batch_images(size)
    n = [len(oracle.akaze_detect_mldb(im, thr)[0]) for im in ims]
    assert n[M.BLANK_INDEX] == 0 and n[M.ODD_INDEX] % 2 == 1
    assert all(30 <= n[b] <= 400 for b in range(4) if b != M.BLANK_INDEX), n
    assert M.BLANK_INDEX not in (0, len(ims) - 1)


def test_small_size_drops_upper_evolution_levels(oracle):
    lv = {}
    for size in sorted(M.BATCHES):
        thr, ims = M.batch_images(size)
        lv[size] = int(oracle.akaze_detect(ims[0], thr)["levels"].max())
    assert lv[(120, 160)] < lv[(240, 320)], lv


def test_stage_scene_survives_the_oracle_chain(oracle):
    ims = M.stage_images()
    kps, descs, xys, pairs, counts, matches = M.oracle_stage(oracle, ims)
    assert all(30 <= len(k) <= 400 for k in kps) and (counts > 0).all()
    W = np.full(4, 320, np.uint32); H = np.full(4, 240, np.uint32)
    oc, _ = oracle.filter_F_collection(xys, W, H, pairs, counts, matches, 4.0, 2048, M.STAGE_FILTER_SEED)
    assert (oc > 0).sum() >= 1
