"""The measured margin of the 2-NN certificate's slack over the case table of tests/certificate_cases.py: every case through r3dm_knn2
of the developer build with MatchParams::err_scale scaled by R3DM_CERT_SLACK_PERMILLE = 1000, 500, 250, ... 1, 0, against the
oracle.  Prints, per path and setting, the cases and queries whose 2-NN differ and the exact-scan fractions, then the smallest
setting at which every case of a path still equals the oracle (DESIGN.md 4.1 "Certification" records one run).
Usage: certificate_margin.py [CASE-SUBSTRING ...]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
from oracle import pyoracle as O  # noqa: E402
from regard3d_amd import api  # noqa: E402
import certificate_cases as CC  # noqa: E402

PERMILLE = (1000, 500, 250, 125, 62, 31, 16, 8, 4, 2, 1, 0)

api.use_developer_library()          # the knob exists only there; it is read at every call
O.build()
names = [n for n in CC.CASES if not sys.argv[1:] or any(s in n for s in sys.argv[1:])]
expect = {n: O.knn2(*CC.CASES[n].make()) for n in names}
c = api.Context(0)
clean = {p: [] for p in CC.PATHS}
for permille in PERMILLE:
    os.environ["R3DM_CERT_SLACK_PERMILLE"] = str(permille)
    bad = {p: [0, 0, 0.0, 0.0, 0] for p in CC.PATHS}          # cases, queries that differ; largest and summed exact-scan fraction; cases run
    for n in names:
        case = CC.CASES[n]
        a, b = case.make()
        c.set_split_mfma(case.path != "f32")
        idx, dist = c.knn2(a, b)
        frac = c.stats().n_exact_fallback / len(b)
        nd = int((np.any(idx != expect[n][0], axis=1) | np.any(dist != expect[n][1], axis=1)).sum())
        r = bad[case.path]
        r[0] += nd > 0; r[1] += nd; r[2] = max(r[2], frac); r[3] += frac; r[4] += 1
        if nd and permille >= 31:
            print(f"  permille {permille}: {n} differs in {nd} of {len(b)} queries", flush=True)
    for p, r in bad.items():
        if r[4]:
            print(f"permille {permille:4d}  {p:6s} cases that differ {r[0]:3d} of {r[4]:3d}  queries that differ {r[1]:5d}  "
                  f"exact-scan fraction mean {r[3] / r[4]:.3f} largest {r[2]:.3f}", flush=True)
            if r[0] == 0:
                clean[p].append(permille)
c.close()
for p in CC.PATHS:
    ok = [v for v in PERMILLE if all(w in clean[p] for w in PERMILLE if w >= v)]
    if ok:
        print(f"{p}: every case equals the oracle down to permille {min(ok)}")
