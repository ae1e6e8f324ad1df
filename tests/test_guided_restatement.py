"""Known answers of the guided-matching restatement (tests/guided_restatement.py; DESIGN.md section 2, "Guided matching").

Hand-built two-view cases whose guided sets follow from the rules by hand: the strict gate at err == errTh, the strict ratio test at
bd == R * sbd, the first-j tie rules, a query with exactly one candidate, and E's threshold squared once more.  CPU only."""
import numpy as np
import pytest

import guided_restatement as G

# F of a pure horizontal translation: l = F x_i = (0, -1, y_i), so err(i, j) = (y_i - y_j)^2 exactly
F_T = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], np.float64)
# H = a translation by (5, 0): err(i, j) = (x_j - x_i - 5)^2 + (y_j - y_i)^2
H_T = np.array([1, 0, 5, 0, 1, 0, 0, 0, 1], np.float64)

XY_I = np.array([[10, 100], [20, 200], [30, 300], [40, 400]], np.float32)
XY_J = np.array([[5, 101], [50, 199.5], [7, 300], [9, 500], [11, 299], [12, 99], [13, 402]], np.float32)


@pytest.fixture(autouse=True, scope="module")
def _oracle(oracle):
    return oracle


def _set(m):
    return [tuple(r) for r in np.asarray(m).tolist()]


def test_geometric_errors_are_the_oracles():
    assert G.geometric_error("F", F_T, 10, 100, 5, 101) == 1.0
    assert G.geometric_error("H", H_T, 10, 100, 16, 102) == 5.0


def test_F_geometry_only_by_hand():
    # thr 2 -> errTh 4, candidates |dy| < 2: i0 -> j0 (err 1), j5 (err 1): tie -> first j; i1 -> j1 (0.25); i2 -> j2 (0), j4 (1);
    # i3 -> j6 has |dy| = 2: err == errTh is rejected (strict <), so i3 has no match
    m = G.guided_pair("F", F_T, 2.0, -1.0, XY_I, XY_J)
    assert _set(m) == [(0, 0), (1, 1), (2, 2)]


def test_F_descriptor_mode_by_hand():
    dI = np.array([[0, 0], [0, 0], [0, 0], [0, 0]], np.float32)
    dJ = np.array([[1, 0], [3, 0], [2, 0], [0, 0], [3, 0], [1.5, 0], [0, 0]], np.float32)
    # i0: candidates j0 (d 1), j5 (d 2.25): 1 < 0.36 * 2.25 = 0.81? no -> no match; with ratio 0.7 (R 0.49): 1 < 1.1025 -> (0, 0)
    # i1: ONE candidate (j1) -> no match in descriptor mode; i2: j2 (d 4), j4 (d 9): 4 < 0.49 * 9 = 4.41 -> (2, 2)
    assert _set(G.guided_pair("F", F_T, 2.0, 0.6, XY_I, XY_J, dI, dJ)) == []
    assert _set(G.guided_pair("F", F_T, 2.0, 0.7, XY_I, XY_J, dI, dJ)) == [(0, 0), (2, 2)]


def test_ratio_boundary_is_strict():
    dI = np.zeros((4, 2), np.float32)
    # i2: d 1 (j2) and 4 (j4); ratio 0.5 -> R * sbd = 1.0 == bd: rejected; a hair more ratio accepts
    dJ = np.array([[9, 9], [9, 9], [1, 0], [9, 9], [2, 0], [9, 9], [9, 9]], np.float32)
    assert (2, 2) not in _set(G.guided_pair("F", F_T, 2.0, 0.5, XY_I, XY_J, dI, dJ))
    assert (2, 2) in _set(G.guided_pair("F", F_T, 2.0, float(np.nextafter(0.5, 1.0)), XY_I, XY_J, dI, dJ))


def test_descriptor_ties_keep_the_first_j():
    dI = np.zeros((4, 2), np.float32)
    dJ = np.array([[1, 0], [9, 9], [1, 0], [9, 9], [1, 0], [1, 0], [9, 9]], np.float32)
    # i0: j0 and j5 at equal distance 1 -> bd = sbd = 1: only a ratio above 1 accepts, and then the FIRST j (j0); i2 likewise j2 before j4
    assert _set(G.guided_pair("F", F_T, 2.0, 0.99, XY_I, XY_J, dI, dJ)) == []
    assert _set(G.guided_pair("F", F_T, 2.0, 1.5, XY_I, XY_J, dI, dJ)) == [(0, 0), (2, 2)]


def test_one_candidate_matches_in_geometry_mode_only():
    xyJ = np.array([[0, 100.5]], np.float32)
    assert _set(G.guided_pair("F", F_T, 2.0, -1.0, XY_I, xyJ)) == [(0, 0)]
    assert _set(G.guided_pair("F", F_T, 2.0, 0.6, XY_I, xyJ, np.zeros((4, 2), np.float32), np.ones((1, 2), np.float32))) == []


def test_hamming_distance_on_binary_rows():
    dI = np.zeros((4, 2), np.uint8)
    dJ = np.array([[1, 0], [0, 0], [255, 255], [0, 0], [7, 0], [3, 0], [0, 0]], np.uint8)
    # i0: j0 (1 bit), j5 (2 bits): 1 < 0.36 * 2 -> no; ratio 0.8 (0.64 * 2 = 1.28) -> (0, 0); i2: j2 (16), j4 (3) -> best j4: 3 < 0.64 * 16
    assert _set(G.guided_pair("F", F_T, 2.0, 0.8, XY_I, XY_J, dI, dJ, binary=True)) == [(0, 0), (2, 4)]


def test_E_threshold_is_squared_once_more():
    # K = identity: F = E.  E's threshold_px is already a squared bound; thr 4 -> errTh 16 -> |dy| < 4.  A bound of 2 px reported as
    # 4 therefore gates at 4 px, not 2 px: j6 (|dy| = 2 for i3) is a match.
    K = np.eye(3)
    m = G.guided_pair("E", F_T, 4.0, -1.0, XY_I, XY_J, KI=K, KJ=K)
    assert (3, 6) in _set(m)
    assert (3, 6) not in _set(G.guided_pair("F", F_T, 2.0, -1.0, XY_I, XY_J))


def test_H_geometry_only_with_coordinate_dedup():
    xyI = np.array([[10, 100], [10, 100], [20, 200]], np.float32)          # features 0 and 1 of I share a position
    xyJ = np.array([[15, 100.5], [25, 200], [16, 100]], np.float32)
    # i0, i1 -> j0 (err 0.25) before j2 (err 1); the second match repeats the coordinates of the first and goes; i2 -> j1 (err 0)
    assert _set(G.guided_pair("H", H_T, 1.5, -1.0, xyI, xyJ)) == [(0, 0), (2, 1)]
    # geometry-only F keeps both (only IndMatch::getDeduplicated, which drops nothing with one match per i)
    assert len(G.guided_pair("F", F_T, 1.5, -1.0, xyI, xyJ)) == 3
