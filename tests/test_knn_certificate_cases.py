"""The k-NN certificate (kernels_match_knn.hip: knnk_finish) evaluated in numpy on the certificate cases, without a GPU: K-lists per
lane half over emulated f32 keys, bound = the smaller (KL + 1)-th key, re-scored nominees, e_k < (bound + ||q||^2) - slack.
Whatever order the keys were summed in, a CERTIFIED query's k nominees are the restatement's k nearest, indices and distances; the
exact-scan share is 0 where 2-NN is easy and >= 0.95 where the keys' rounding exceeds every gap."""
import numpy as np
import pytest

import certificate_cases as CC
import knn_restatement as R


def emulate(a, b, k, order):
    KL = 4 if k <= 4 else 8
    keys = CC.emulated_keys(a, b, order)
    dist = CC.ref_distances(a, b)
    nb = CC.norms_f32(b)
    slack = CC.case_slack("f32", a, b)
    half = (np.arange(a.shape[0]) >> 2) & 1
    answers, certified = [], np.zeros(b.shape[0], bool)
    for q in range(b.shape[0]):
        nominees, bound = [], np.float32(np.inf)
        for h in (0, 1):
            rows = np.flatnonzero(half == h)
            o = rows[np.argsort(keys[q, rows], kind="stable")]
            nominees += o[:KL].tolist()
            if len(o) > KL:
                bound = min(bound, keys[q, o[KL]])
        nominees = np.array(nominees)
        e = dist[q, nominees]
        o = np.lexsort((nominees, e))[:k]
        answers.append((nominees[o], e[o]))
        certified[q] = e[o][-1] < np.float32(np.float32(bound + nb[q]) - slack[q])
    return answers, certified


@pytest.mark.parametrize("k", (3, 8))
@pytest.mark.parametrize("order", ("seq", "block2"))
@pytest.mark.parametrize("case,lo,hi", [("offset_f32_d128_t0", 0.0, 0.0), ("offset_f32_d128_t20", None, None), ("offset_f32_d128_t1000", 0.95, 1.0),
                                        ("mixed_large_last_f32", None, None), ("mixed_large_row0_f32", None, None)])
def test_certified_answers_are_the_restatement(case, lo, hi, order, k):
    a, b = CC.CASES[case].make()
    b = b[:96]
    ri, rd = R.knn(a, b, k)
    answers, certified = emulate(a, b, k, order)
    for q in np.flatnonzero(certified):
        assert np.array_equal(answers[q][0], ri[q]) and np.array_equal(answers[q][1], rd[q])
    share = 1.0 - certified.mean()
    print(f"{case}, k = {k}, {order}: exact-scan share {share:.3f}")
    if lo is not None:
        assert lo <= share <= hi
