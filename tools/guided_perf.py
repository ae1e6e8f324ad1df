"""Cost and yield of guided matching (r3dm_guided_match / r3dm_set_guided_matching) next to putative matching of the same pairs:
    python tools/guided_perf.py c2 [images]         C2-sized collection (SIFT-128, 8,192 features per view; default 200 views): putative
                                                    matching, the F filter, guided matching of the F-accepted pairs (ratio 0.6 and geometry only)
    python tools/guided_perf.py stage [images]      the stage's photographs (4000 x 3000, default 24): computeMatches with the flag off and on,
                                                    then F / E / H with the switch on over the stage's own files
Prints one JSON line per measurement: milliseconds per accepted pair, candidates per query, matches gained per accepted pair."""
import json, os, shutil, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from regard3d_amd import api, synth


def guided_leg(c, g, kind, models, thr, ratio, inliers):
    c.guided_match(g, kind, models, thr, ratio)                         # warm (buffers, row layouts)
    t = time.perf_counter()
    gg = c.guided_match(g, kind, models, thr, ratio)
    wall = (time.perf_counter() - t) * 1e3
    r = c.guided_report()
    n = max(r["n_pairs"], 1)
    return dict(kind=kind, ratio=ratio, pairs=r["n_pairs"], ms_kernels=round(r["ms_kernels"], 3), ms_wall=round(wall, 3),
                ms_kernels_per_pair=round(r["ms_kernels"] / n, 4), candidates_per_query=round(r["candidates_per_query"], 2),
                guided_matches=gg.num_matches, filter_inliers=inliers, gained_per_pair=round((gg.num_matches - inliers) / n, 1))


def accepted(c, g, kind):
    f = {"F": c.filter_F, "E": c.filter_E, "H": c.filter_H}[kind]
    gf, M = f(g, **{"want_" + kind: True})
    rep = c.filter_report()
    where = {(int(I), int(J)): k for k, (I, J) in enumerate(g.pairs)}
    thr = np.array([rep[where[(int(I), int(J))]][0] for I, J in gf.pairs], np.float64)
    return gf, M, thr


def putative_ms(c, pairs, ratio=0.6):
    c.match_pairs(pairs, ratio, True)
    t = time.perf_counter()
    c.match_pairs(pairs, ratio, True)
    return (time.perf_counter() - t) * 1e3, c.stats().ms_match_kernels


def c2(n_images):
    sc = synth.make_scene(n_images, 8192, "sift", seed=2002)
    c = api.Context(0)
    for i in range(sc.n_images):
        c.set_image(i, sc.descs[i], sc.xys[i], int(sc.widths[i]), int(sc.heights[i]))
    g = c.match_pairs(sc.exhaustive_pairs(), 0.6, True)
    gf, M, thr = accepted(c, g, "F")
    wall, kern = putative_ms(c, gf.pairs)
    print(json.dumps(dict(leg="c2", images=n_images, F_pairs=gf.num_pairs, putative_ms_wall_same_pairs=round(wall, 3),
                          putative_ms_kernels_same_pairs=round(kern, 3), putative_ms_kernels_per_pair=round(kern / max(gf.num_pairs, 1), 4))))
    for ratio in (0.6, -1.0):
        print(json.dumps(dict(leg="c2", **guided_leg(c, gf, "F", M, thr, ratio, gf.num_matches))))
    c.close()


def stage(n_images):
    W, H = 4000, 3000
    imgs, K = synth.make_photo_set(n_images, H, W, seed=7007, device="cuda")
    views = [dict(id=k, width=W, height=H, basename=f"img{k:04d}", gray=imgs[k], focal_px=K[0, 0], ppx=K[0, 2], ppy=K[1, 2]) for k in range(n_images)]
    bare = [dict(v, gray=None) for v in views]
    d = tempfile.mkdtemp(prefix="r3dm_guided_")
    try:
        st = api.Stage([0])
        r0 = st.run(d, views, 0.001, 0.6, 9, True, True, True, 5489, 3, 8)     # features once; later runs reuse the files
        empty = [k for k in range(n_images) if os.path.getsize(os.path.join(d, f"img{k:04d}.feat")) == 0]
        print(json.dumps(dict(leg="stage", first_call=dict(images_extracted=r0.images_extracted, keypoints=r0.n_keypoints,
                                                           F_pairs=r0.n_F_pairs, empty_feat_files=empty))))
        out = {}
        for guided in (False, True, False, True):
            t = time.perf_counter()
            r = st.run(d, bare, 0.001, 0.6, 9, True, True, True, 5489, 3, 8, guided=guided)
            out.setdefault(guided, []).append(dict(ms_call=round((time.perf_counter() - t) * 1e3, 1), ms_total=round(r.ms_total, 1),
                                                    ms_filters_wall=round(r.ms_filters_wall, 1), F=(r.n_F_pairs, r.n_F_matches),
                                                    E=(r.n_E_pairs, r.n_E_matches), H=(r.n_H_pairs, r.n_H_matches)))
        st.close()
        print(json.dumps(dict(leg="stage", images=n_images, computeMatches_off=out[False], computeMatches_on=out[True])))
        # the guided step itself on the stage's own data (.feat / .desc / matches.putative), with the switch on
        c = api.Context(0)
        c.set_split_mfma(True)
        for k in range(n_images):
            xy = np.loadtxt(os.path.join(d, f"img{k:04d}.feat"), dtype=np.float32).reshape(-1, 4)[:, :2].copy()
            raw = np.fromfile(os.path.join(d, f"img{k:04d}.desc"), np.uint8)
            desc = np.frombuffer(raw[8:].tobytes(), np.float32).reshape(-1, 144)
            c.set_image(k, desc, xy, W, H)
            c.set_intrinsics(k, K)
        put = api.Graph.load(os.path.join(d, "matches.putative.txt"))
        for kind, ratio in (("F", 0.6), ("E", 0.6), ("H", -1.0)):
            gk, M, thr = accepted(c, put, kind)
            if gk.num_pairs == 0:
                continue
            wall, kern = putative_ms(c, gk.pairs)
            print(json.dumps(dict(leg="stage", putative_ms_kernels_same_pairs=round(kern, 3), putative_ms_wall_same_pairs=round(wall, 3),
                                  **guided_leg(c, gk, kind, M, thr, ratio, gk.num_matches))))
        c.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    mode = sys.argv[1]
    n = int(sys.argv[2]) if len(sys.argv) > 2 else (200 if mode == "c2" else 24)
    {"c2": c2, "stage": stage}[mode](n)
