"""Cost and effect of preemptive matching (r3dm_set_preemptive_matching):
    python tools/preselect_perf.py --mode off|gate|buys [--package-root DIR] [--label NAME] [--reps R]
One JSON line per measurement.

off    the switch-off pass at BASELINE config C2's size -- 200 views x 8,192 SIFT-128 rows, 19,900 pairs, ratio 0.6 -- on the f32 and
       on the integer tiles: median [min, max] wall time of r3dm_match_pairs.  --package-root imports regard3d_amd from DIR instead of
       this tree: a build of the PARENT commit, for a session in which parent and tree alternate; the condition on this change is that
       the tree's time lies within the parent's own run-to-run spread.
gate   the gate alone: r3dm_preselect_report's ms_kernels for C2's 19,900 pairs at h = 128 and h = 256 on SIFT-128, LIOP-144 and BIN-61
       views (--gate-feat rows each: the gate reads heads only), heads cached (the first call, which builds them, is reported apart).
       Beside it the paper estimate of the issue scaled to the pair count: 0.1 s per 499,500 pairs at h = 128 on LIOP-144.
buys   what the gate buys and costs at 128 / 4 on a synthetic strip of --buys-images views in which only neighbouring views share
       structure (synth.make_scene: a view overlaps the three views on either side); one scale per scene point, carried to every
       observation of it, random scales for the distractors.  Pairs kept, wall time of the gated pass against the exhaustive pass, and
       the share of the pairs with >= 16 F-inliers under exhaustive matching that the gate keeps.  No bar is set on these figures."""
import argparse
import json
import os
import sys
import time

import numpy as np


def _median_pass(fn, reps):
    fn()                                                     # warm-up: layouts staged, buffers grown
    ms = []
    out = None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_wall_median": round(float(np.median(ms)), 1), "ms_wall_min": round(min(ms), 1), "ms_wall_max": round(max(ms), 1)}, out


def mode_off(a, api, synth):
    sc = synth.make_scene(a.images, a.feat, "sift", seed=2002)
    pairs = sc.exhaustive_pairs()
    c = api.Context(0)
    for i in range(sc.n_images):
        c.set_image(i, sc.descs[i], sc.xys[i], int(sc.widths[i]), int(sc.heights[i]))
    for tiles, integer in (("f32", False), ("integer (bf16)", True)):
        c.set_integer_mfma(integer)
        t, g = _median_pass(lambda: c.match_pairs(pairs, 0.6, True), a.reps)
        print(json.dumps({"mode": "off", "build": a.label, "images": a.images, "rows": a.feat, "pairs": int(len(pairs)), "tiles": tiles, **t,
                          "ms_tile_kernel": round(c.stats().ms_match_kernels, 1), "matches": int(g.num_matches)}), flush=True)
    c.close()


def mode_gate(a, api, synth):
    rng = np.random.default_rng(7)
    for name, kind, cut, binary, ratio, squared in (("SIFT-128", "sift", None, False, 0.6, True), ("LIOP-144", "liop", None, False, 0.6, True),
                                                     ("BIN-61", "akaze", 61, True, 0.8, False)):
        sc = synth.make_scene(a.images, a.gate_feat, kind, seed=2002)
        pairs = sc.exhaustive_pairs()
        c = api.Context(0)
        for i in range(sc.n_images):
            d = sc.descs[i] if cut is None else np.ascontiguousarray(sc.descs[i][:, :cut])
            c.set_image(i, d, None, int(sc.widths[i]), int(sc.heights[i]), binary=binary)
            c.set_view_priority(i, rng.random(len(d)).astype(np.float32) * 20.0)
        for h in (128, 256):
            counts = c.preselect_pairs(pairs, h, ratio, squared)
            first = c.preselect_report()
            ms = []
            for _ in range(a.reps):
                c.preselect_pairs(pairs, h, ratio, squared)
                ms.append(c.preselect_report()["ms_kernels"])
            print(json.dumps({"mode": "gate", "build": a.label, "rows": name, "views": a.images, "rows_per_view": a.gate_feat, "pairs": int(len(pairs)), "h": h,
                              "ms_kernels_median": round(float(np.median(ms)), 3), "ms_kernels_min": round(min(ms), 3), "ms_kernels_max": round(max(ms), 3),
                              "ms_kernels_first_call_with_heads": round(first["ms_kernels"], 3), "ms_wall_first_call": round(first["ms_wall"], 3),
                              "paper_estimate_ms_h128_liop": round(100.0 * len(pairs) / 499500.0, 3), "pairs_with_count_ge_4": int((counts >= 4).sum())}), flush=True)
        c.close()


def mode_buys(a, api, synth):
    sc = synth.make_scene(a.buys_images, a.buys_feat, "sift", seed=2002)
    pairs = sc.exhaustive_pairs()
    rng = np.random.default_rng(11)
    n_world = max(int(w.max()) for w in sc.world_ids) + 1
    world_scale = (1.5 * np.exp(rng.normal(0.0, 0.8, n_world))).astype(np.float32)       # one scale per scene point
    c = api.Context(0)
    for i in range(sc.n_images):
        c.set_image(i, sc.descs[i], sc.xys[i], int(sc.widths[i]), int(sc.heights[i]))
        wid = sc.world_ids[i]
        s = np.where(wid >= 0, world_scale[np.maximum(wid, 0)], (1.5 * np.exp(rng.normal(0.0, 0.8, len(wid)))).astype(np.float32)).astype(np.float32)
        c.set_view_priority(i, s)
    t_ex, g = _median_pass(lambda: c.match_pairs(pairs, 0.6, True), a.reps)
    gf = c.filter_F(g, 4.0, 2048, seed=5489)
    good = {(int(p[0]), int(p[1])) for p, n in zip(gf.pairs, np.diff(gf.offsets.astype(np.int64))) if n >= 16}
    c.set_preemptive_matching(True, 128, 4)
    t_on, g_on = _median_pass(lambda: c.match_pairs(pairs, 0.6, True), a.reps)
    rep = c.preselect_report()
    kept = {(int(p[0]), int(p[1])) for p in g_on.pairs}
    counts = c.preselect_pairs(pairs, 128, 0.6, True)
    kept_all = {(int(p[0]), int(p[1])) for p, n in zip(pairs, counts) if n >= 4}
    print(json.dumps({"mode": "buys", "build": a.label, "views": a.buys_images, "rows_per_view": a.buys_feat, "pairs": int(len(pairs)), "h": 128, "t": 4,
                      "pairs_kept": int(rep["n_kept"]), "pairs_with_matches_exhaustive": int(g.num_pairs), "pairs_with_matches_gated": len(kept),
                      "exhaustive": t_ex, "gated": t_on, "gate_ms_kernels": round(rep["ms_kernels"], 3), "gate_ms_wall": round(rep["ms_wall"], 3),
                      "pairs_ge_16_F_inliers": len(good), "of_those_kept": len(good & kept_all),
                      "share_kept": round(len(good & kept_all) / max(len(good), 1), 4)}), flush=True)
    c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("off", "gate", "buys"), required=True)
    ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="tree")
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--feat", type=int, default=8192)
    ap.add_argument("--gate-feat", type=int, default=1024)
    ap.add_argument("--buys-images", type=int, default=64)
    ap.add_argument("--buys-feat", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    sys.path.insert(0, a.package_root)
    from regard3d_amd import api, synth
    {"off": mode_off, "gate": mode_gate, "buys": mode_buys}[a.mode](a, api, synth)


if __name__ == "__main__":
    main()
