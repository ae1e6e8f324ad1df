"""Known answers of the classic A-KAZE restatement (tests/akaze_classic_restatement.py; DESIGN.md section 7, "The classic AKAZE arm").

Hand-built cases whose outcome follows from libAKAZE's rules by hand: the evolution table and its octave cut, the FED step lists, the
sequential kpts_aux rule (first hit decides, equal responses, in-place replacement, chains, the same / lower level window), the
descriptor border test at its boundary, the upper-level filter and the refinement's erasure.  CPU only."""
import numpy as np
import pytest

import akaze_classic_restatement as R

f32 = np.float32


def test_evolution_table_and_octave_cut():
    lv = R.levels(640, 480)
    assert [(e["w"], e["h"]) for e in lv] == [(640 >> o, 480 >> o) for o in range(4) for _ in range(4)]
    assert [e["sigma_size"] for e in lv] == [2, 3, 3, 4] * 4
    assert [e["octave"] for e in lv] == [o for o in range(4) for _ in range(4)]
    assert lv[0]["esigma"] == f32(1.6) and lv[4]["esigma"] == f32(3.2)
    assert len(R.levels(160, 120)) == 8           # octave 2 would be 40 x 30: < 80 wide
    assert len(R.levels(159, 120)) == 4           # octave 1 would be 79 wide
    assert len(R.levels(200, 79)) == 4            # octave 1 would be 39 high
    assert len(R.levels(90, 60)) == 4 and len(R.levels(20, 10)) == 4      # octave 0 always exists


def test_fed_step_lists():
    lv = R.levels(640, 480)
    n = [len(R.fed_tau(f32(lv[i]["etime"] - lv[i - 1]["etime"]))) for i in range(1, 16)]
    assert n == [3, 3, 4, 4, 5, 6, 7, 8, 10, 12, 14, 17, 20, 24, 29]
    for i in range(1, 16):
        T = float(f32(lv[i]["etime"] - lv[i - 1]["etime"]))
        assert abs(float(sum(R.fed_tau(T))) - T) < 1e-5 * T        # the FED cycle reaches the stopping time
    tau = R.fed_tau(f32(1.0))                   # n = 3, kappa = 1, prime 5: tauh reordered 0, 1, 2
    assert len(tau) == 3 and tau[0] < tau[1] < tau[2]
    tau = R.fed_tau(f32(67.86474609375))        # n = 29, reordered with kappa 14 over the prime 31
    assert len(tau) == 29 and sorted(tau) != tau


LV0 = dict(esigma=f32(1.6), ratio=f32(1.0), octave=0)     # size 2.4, size^2 5.76, sigma_size 2, border reach 28.28


def _aux(entries):
    a = R.AuxList(16)
    for x, y, resp, cls in entries:
        a.put(a.n, f32(x), f32(y), f32(2.4), f32(resp), cls, 0)
        a.n += 1
    return a


def test_the_first_hit_decides_and_breaks():
    a = _aux([(100, 100, 0.5, 0), (101, 100, 0.1, 0)])
    R.offer(a, LV0, 0, 101, 101, f32(0.3), 500, 500)          # slot 0 is hit first: 0.3 < 0.5 rejects, slot 1 is never looked at
    assert a.n == 2 and a.x[0] == 100 and a.resp[1] == f32(0.1)


def test_equal_response_does_not_replace():
    a = _aux([(100, 100, 0.5, 0)])
    R.offer(a, LV0, 0, 101, 101, f32(0.5), 500, 500)
    assert a.n == 1 and a.x[0] == 100 and a.y[0] == 100


def test_replacement_keeps_the_slot():
    a = _aux([(100, 100, 0.5, 0), (200, 200, 0.1, 0)])
    R.offer(a, LV0, 0, 101, 101, f32(0.9), 500, 500)
    assert a.n == 2 and (a.x[0], a.y[0], a.resp[0]) == (101, 101, f32(0.9)) and a.x[1] == 200


def test_a_chain_of_replacements():
    a = R.AuxList(16)
    for x, y, v in [(100, 100, 0.1), (101, 101, 0.2), (102, 102, 0.3), (104, 102, 0.4)]:
        R.offer(a, LV0, 0, y, x, f32(v), 500, 500)
    assert a.n == 1 and (a.x[0], a.y[0], a.resp[0]) == (104, 102, f32(0.4))
    R.offer(a, LV0, 0, 102, 107, f32(0.05), 500, 500)         # 3 px from the moved slot: 9 > 5.76, appended
    assert a.n == 2 and a.x[1] == 107


def test_same_or_lower_level_window():
    lv2 = dict(esigma=f32(1.6), ratio=f32(1.0), octave=0)
    a = _aux([(100, 100, 0.1, 0), (150, 150, 0.1, 1)])
    R.offer(a, lv2, 2, 100, 100, f32(0.05), 500, 500)         # class 0 is two levels down: not compared, appended
    assert a.n == 3 and a.cls[2] == 2
    R.offer(a, lv2, 2, 150, 150, f32(0.9), 500, 500)          # class 1 is one level down: replaced in place, now class 2
    assert a.n == 3 and a.cls[1] == 2 and a.resp[1] == f32(0.9)


@pytest.mark.parametrize("x,cols,inside", [(29, 59, True), (28, 500, False), (29, 58, False)])
def test_descriptor_border_at_its_boundary(x, cols, inside):
    a = R.AuxList(4)
    R.offer(a, LV0, 0, 100, x, f32(0.5), 500, cols)           # reach = fRound(x -/+ 10 sqrt(2) * 2) -/+ 1
    assert (a.n == 1) == inside


def test_upper_level_filter():
    a = _aux([(100, 100, 0.1, 0), (101, 100, 0.2, 1)])
    assert list(R.upper_filter(a)) == [1]                     # a later, stronger slot of class + 1 within size removes slot 0
    a = _aux([(101, 100, 0.2, 1), (100, 100, 0.1, 0)])
    assert list(R.upper_filter(a)) == [0, 1]                  # only LATER slots are compared
    a = _aux([(100, 100, 0.2, 0), (101, 100, 0.2, 1)])
    assert list(R.upper_filter(a)) == [0, 1]                  # equal responses keep it
    a = _aux([(100, 100, 0.1, 0), (101, 100, 0.2, 2)])
    assert list(R.upper_filter(a)) == [0, 1]                  # class + 2 is not the upper level


def test_refinement_erases_beyond_one_pixel():
    L = np.zeros((5, 5), np.float32)
    L[2, 1], L[2, 2], L[2, 3] = 0.0, 1.0, 0.99
    L[1, 2], L[3, 2] = 0.5, 0.5
    x, y = R.refine(L, 2.0, 2.0, 0)
    assert 2.0 < x < 3.0 and y == f32(2.0)
    L[2, 3] = 1.9                                             # Dx = 0.95, Dxx = -0.1: the step is 9.5 px
    assert R.refine(L, 2.0, 2.0, 0) is None


def test_orientation_of_a_pure_x_gradient_is_zero_degrees():
    Lx = np.ones((64, 64), np.float32); Ly = np.zeros((64, 64), np.float32)
    assert R.orientation_deg(Lx, Ly, 32.0, 32.0, f32(4.8), 0) == f32(0.0)
    d = R.orientation_deg(Ly, Lx, 32.0, 32.0, f32(4.8), 0)  # pure y gradient: 90 degrees (fastAtan2's polynomial)
    assert abs(float(d) - 90.0) < 0.01
