"""Cost of mutual matching (r3dm_set_mutual_matching) at BASELINE config C2's size -- 200 views x 8,192 SIFT-128 rows,
19,900 pairs, ratio 0.6 -- on the f32 tiles and on the integer tiles, with the switch off and on:
    python tools/mutual_perf.py [--package-root DIR] [--label NAME] [--images N] [--reps R]
One process, one context, the collection registered once.  Per tile format the switch-off and the switch-on pass ALTERNATE in one loop
(off, on, off, on ...), so both see the same clocks; a line holds the median wall time of r3dm_match_pairs with its smallest and largest
repetition, the matches returned and the two counters.  One JSON line per (tiles, switch).

--package-root: import regard3d_amd from DIR instead of this tree -- a build of the PARENT commit, which has no switch: only its
switch-off lines are written.  profiles/mutual_perf.txt was taken by running parent and tree alternately in one session (parent, tree,
parent, tree); the condition on this change is that the tree's switch-off time lies within the parent's own run-to-run spread."""
import argparse
import json
import os
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="tree")
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--feat", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    sys.path.insert(0, a.package_root)
    from regard3d_amd import api, synth

    sc = synth.make_scene(a.images, a.feat, "sift", seed=2002)
    pairs = sc.exhaustive_pairs()
    c = api.Context(0)
    for i in range(sc.n_images):
        c.set_image(i, sc.descs[i], sc.xys[i], int(sc.widths[i]), int(sc.heights[i]))
    has_switch = hasattr(c, "set_mutual_matching")

    def one_pass(mutual):
        if has_switch:
            c.set_mutual_matching(mutual)
        t0 = time.perf_counter()
        g = c.match_pairs(pairs, 0.6, True)
        ms = (time.perf_counter() - t0) * 1e3
        s = c.stats()
        return ms, s.ms_match_kernels, int(g.num_matches), int(getattr(s, "n_mutual_checked", 0)), int(getattr(s, "n_mutual_dropped", 0))

    for tiles, integer in (("f32", False), ("integer (bf16)", True)):
        c.set_integer_mfma(integer)
        switches = (False, True) if has_switch else (False,)
        for m in switches:                                   # warm-up: layouts staged, buffers grown
            one_pass(m)
        runs = {m: [] for m in switches}
        for _ in range(a.reps):
            for m in switches:
                runs[m].append(one_pass(m))
        for m in switches:
            ms = [r[0] for r in runs[m]]
            print(json.dumps({"build": a.label, "images": a.images, "rows": a.feat, "pairs": int(len(pairs)), "tiles": tiles, "mutual": m,
                              "ms_wall_median": round(float(np.median(ms)), 1), "ms_wall_min": round(min(ms), 1), "ms_wall_max": round(max(ms), 1),
                              "ms_tile_kernel": round(float(np.median([r[1] for r in runs[m]])), 1), "matches": runs[m][0][2],
                              "n_mutual_checked": runs[m][0][3], "n_mutual_dropped": runs[m][0][4]}), flush=True)
    if has_switch:
        c.set_mutual_matching(False)
    c.set_integer_mfma(False)
    c.close()


if __name__ == "__main__":
    main()
