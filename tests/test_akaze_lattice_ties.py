"""CPU proof that the lattice images of tests/akaze_lattices.py make the Fast arm's in-level rule meet EQUAL responses: the inputs of
the GPU tie tests (tests/test_gpu_akaze.py, `lattice`) are shown to be adequate by the oracle alone."""
import numpy as np
import pytest

import akaze_lattices as L

# measured with the committed seed (rng 20261), 240 x 320, identical at both thresholds:
#   tile3 : 8790 candidates, 1428 hits on a kept point, 1428 ties (every hit), 0 replacements, 6648 keypoints
#   diag13: 16846 candidates, 6337 hits, 1136 ties, 47 replacements, 3668 keypoints
# no determinant above the threshold is a subnormal float on either image


@pytest.mark.parametrize("thr", L.THRESHOLDS)
@pytest.mark.parametrize("name", ["tile3", "diag13"])
def test_lattice_images_produce_equal_responses_inside_the_pruning_radius(oracle, name, thr):
    img = L.lattice_images()[name]
    assert img.shape == (L.H, L.W) and img.dtype == np.float32
    e = L.tie_events(oracle, img, thr)
    print(name, thr, e)
    assert e["ties"] >= 500
    assert e["subnormal"] == 0                                      # no determinant above the threshold is a subnormal float: denormal handling is not in play
    assert e["hits"] >= e["ties"] + e["replacements"] and e["candidates"] > e["hits"]
    n = len(oracle.akaze_detect(img, thr)["kps"])
    assert n > 1000                                                 # the lattices keep keypoints: the tie rule decides visible output


def test_the_ordinary_dense_image_has_no_ties(oracle):
    """the comparison the lattices are measured against: smooth noise, the suite's "dense" image, meets kept points but no equal response"""
    from scipy.ndimage import gaussian_filter
    rng = np.random.default_rng(21)
    img = np.clip(0.5 + 4.0 * gaussian_filter(rng.normal(0, 0.2, (L.H, L.W)), 1.2), 0, 1).astype(np.float32)
    e = L.tie_events(oracle, img, 1e-8)
    assert e["ties"] == 0 and e["candidates"] > 100
