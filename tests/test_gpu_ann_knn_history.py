"""The k-lists of the approximate arms do not depend on what the context computed before (`-m gpu`), in the style of
tests/test_gpu_history.py: the k = 8 results of each arm on a fresh context, and on a context that has just run the 2-NN arms and an
exhaustive r3dm_knn on LARGER views -- its scratch (d_knn_idx / d_knn_dist sized for other strides, d_nn, d_cnt, the job tables) then
holds valid-looking leftovers of those calls.  Nothing writes patterns into device memory; each context is opened and closed here."""
import numpy as np
import pytest

from regard3d_amd import api
from test_gpu_ann_knn import _arms, _mrpt_views, _same, _views

pytestmark = pytest.mark.gpu


def _k8(ctx, arms):
    return {name: knn(ctx, 8) for name, (knn, _) in arms.items()}


def test_k8_lists_do_not_depend_on_the_contexts_history():
    d0, d1 = _mrpt_views()                                     # 600 x 300 rows
    arms = _arms(d0, d1)
    fresh = api.Context(0)
    try:
        want = _k8(fresh, arms)
    finally:
        fresh.close()
    assert all((want[a][0][:, 0] >= 0).any() for a in want)
    used = api.Context(0)
    try:
        b0, b1 = _views("sift", 1100, 29)                      # other shapes: more rows, more queries, another stride of the k-lists
        for _, knn2 in _arms(b0, b1).values():
            knn2(used)
        used.knn(b0, b1, 5)
        used.knn(b0[:, :64].copy(), b1[:700, :64].copy(), 8)
        got = _k8(used, arms)
        again = _k8(used, arms)
    finally:
        used.close()
    for a in want:
        assert _same(got[a], want[a]), a
        assert _same(again[a], want[a]), a
