"""Cost of the symmetric ratio test (r3dm_set_symmetric_ratio) at BASELINE config C2's size -- 200 views x 8,192
SIFT-128 rows, 19,900 pairs, ratio 0.6 -- on the f32 tiles and on the integer tiles:
    python tools/symmetric_ratio_perf.py [--package-root DIR] [--label NAME] [--images N] [--reps R] [--kind sift|liop|akaze] [--dim D]
One process, one context, the collection registered once.  Per tile format the legs the library offers ALTERNATE in one loop (off,
mutual, symmetric, off, ...), so all see the same clocks; a line holds the median wall time of r3dm_match_pairs with its smallest and
largest repetition, the matches returned and the three counters.  One JSON line per (tiles, leg).

--kind / --dim go to synth.make_scene and choose the kernel of kernels_match_mutual.hip that the mutual and symmetric legs run: --dim 64 |
128 | 144 | 256 the tile kernel of G = 8 | 16 | 18 | 32, a length without a tensor kernel (--dim 100) the rows-based kernel, --kind akaze
(registered with binary=True: 61 bytes of bits in --dim >= 61 bytes, i.e. rows of 16 words) the Hamming kernel.

--package-root: import regard3d_amd from DIR instead of this tree -- a build of the PARENT commit, which has the mutual switch only: its
legs are "off" and "mutual".  profiles/symmetric_ratio_perf.txt was taken by running parent and tree alternately in one session (parent,
tree, parent, tree); the conditions on this change are that the tree's "off" and "mutual" times lie within the range the parent's own
sessions span.  The cost of "symmetric" over "mutual" is reported as measured."""
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
    ap.add_argument("--kind", choices=("sift", "liop", "akaze"), default="sift")
    ap.add_argument("--dim", type=int, default=None)
    a = ap.parse_args()
    sys.path.insert(0, a.package_root)
    from regard3d_amd import api, synth

    sc = synth.make_scene(a.images, a.feat, a.kind, seed=2002, dim=a.dim)
    pairs = sc.exhaustive_pairs()
    c = api.Context(0)
    for i in range(sc.n_images):
        c.set_image(i, sc.descs[i], sc.xys[i], int(sc.widths[i]), int(sc.heights[i]), binary=a.kind == "akaze")
    has_symmetric = hasattr(c, "set_symmetric_ratio")
    legs = ("off", "mutual", "symmetric") if has_symmetric else ("off", "mutual")

    def one_pass(leg):
        c.set_mutual_matching(leg == "mutual")
        if has_symmetric:
            c.set_symmetric_ratio(leg == "symmetric")
        t0 = time.perf_counter()
        g = c.match_pairs(pairs, 0.6, True)
        ms = (time.perf_counter() - t0) * 1e3
        s = c.stats()
        rep = c.symmetric_ratio_report() if has_symmetric else (0, 0, 0)
        return ms, s.ms_match_kernels, int(g.num_matches), int(s.n_mutual_checked), int(s.n_mutual_dropped), int(rep[2])

    for tiles, integer in (("f32", False), ("integer (bf16)", True)):
        c.set_integer_mfma(integer)
        for leg in legs:                                     # warm-up: layouts staged, buffers grown
            one_pass(leg)
        runs = {leg: [] for leg in legs}
        for _ in range(a.reps):
            for leg in legs:
                runs[leg].append(one_pass(leg))
        for leg in legs:
            ms = [r[0] for r in runs[leg]]
            print(json.dumps({"build": a.label, "images": a.images, "rows": a.feat, "pairs": int(len(pairs)), "tiles": tiles, "leg": leg,
                              "ms_wall_median": round(float(np.median(ms)), 1), "ms_wall_min": round(min(ms), 1), "ms_wall_max": round(max(ms), 1),
                              "ms_tile_kernel": round(float(np.median([r[1] for r in runs[leg]])), 1), "matches": runs[leg][0][2],
                              "n_mutual_checked": runs[leg][0][3], "n_mutual_dropped": runs[leg][0][4], "dropped_ratio": runs[leg][0][5]}), flush=True)
    c.set_mutual_matching(False)
    if has_symmetric:
        c.set_symmetric_ratio(False)
    c.set_integer_mfma(False)
    c.close()


if __name__ == "__main__":
    main()
