"""Measurement of pair proposal on one MI355X (profiles/vocab_perf.txt):
    python tools/vocab_perf.py <n_views> <exhaustive 0|1> [<output file> [train]]
bench.py's synthetic SIFT-128 views (8,192 rows each): HIP-event times of the phases of r3dm_propose_pairs at 4,096 and 16,384 words,
top_k 20; the fraction of pairs proposed; recall of the pairs with F-inliers in an exhaustive run (exhaustive = 1) or of the pairs of
views that share features in the scene (0: sizes at which a pass over all pairs is too long); r3dm_match_pairs on all pairs and on
the proposed ones; the preemptive gate on the same views.
With `train` (profiles/vocab_train_perf.txt) instead: r3dm_vocab_train from the sampled vocabulary, 10
iterations, at both word counts -- HIP-event ms per iteration of assignment, sort and update, the update's bytes per second -- and the
recall of the same target at top_k 2, 4, 8 and 20 for the sampled, the trained and the trained + idf-weighted vocabulary."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from regard3d_amd import api, synth  # noqa: E402

n_views, exhaustive = int(sys.argv[1]), int(sys.argv[2]) != 0
out = open(sys.argv[3] if len(sys.argv) > 3 else os.devnull, "w")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    out.write(line + "\n"); out.flush()


def med(xs):
    return sorted(xs)[len(xs) // 2]


descs, xys, _ = synth.make_scene_torch(n_views, 8192, seed=2002, device="cuda:0", kind="sift")
hd = [descs[i].cpu().numpy() for i in range(n_views)]
hx = [xys[i].cpu().numpy() for i in range(n_views)]
del descs, xys
torch.cuda.empty_cache()
ctx = api.Context(0)
ids = list(range(n_views))
ctx.set_images(ids, hd, hx, synth.WIDTH, synth.HEIGHT, wait=True)
ii, jj = np.triu_indices(n_views, k=1)
allp = np.stack([ii, jj], 1).astype(np.uint32)
truth = {(int(a), int(b)) for a, b in allp if b - a < 4}           # the views that share features in this scene
say(f"# {n_views} views x 8192 x SIFT-128 (synth.make_scene_torch seed 2002: bench.py's views), {len(allp)} pairs, {len(truth)} pairs of views that share features")


def timed_match(p):
    torch.cuda.synchronize()
    t = time.perf_counter()
    g = ctx.match_pairs(p, 0.6, True)
    torch.cuda.synchronize()
    return g, (time.perf_counter() - t) * 1e3


inlier_pairs = None
if exhaustive:
    g, _ = timed_match(allp)                                        # warm-up
    gf = ctx.filter_F(g, 4.0, 2048, seed=5489)
    inlier_pairs = {(int(a), int(b)) for a, b in gf.pairs}
    say(f"exhaustive run: {g.num_pairs} putative pairs, {len(inlier_pairs)} pairs with F inliers ({100.0 * len(inlier_pairs) / len(allp):.2f} % of all pairs)")
target = inlier_pairs if inlier_pairs is not None else truth
target_name = "pairs with F inliers in the exhaustive run" if inlier_pairs is not None else "pairs of views that share features (scene truth; no exhaustive run at this size)"

HBM_BYTES_PER_S = 8.0e12                                            # MI355X HBM3E peak

for n_words in (4096, 16384) if len(sys.argv) > 4 and sys.argv[4] == "train" else ():
    init = ctx.vocab_sample(ids, n_words)
    reps = []
    for it in range(4):                                             # the first is the warm-up
        v = ctx.vocab_train(init, ids, 10)
        r = ctx.vocab_train_report(v)
        if it:
            reps.append(r)
        if it < 3:
            v.close()
    n_assign = reps[0]["n_rows_assigned"] // (n_views * 8192)
    n_upd = reps[0]["n_updates"]
    a, s_, u = (med([r[k] for r in reps]) for k in ("ms_assign", "ms_sort", "ms_update"))
    row_bytes = n_views * 8192 * 128 * 4
    say(f"n_words {n_words} train 10: {n_upd} updates, {n_assign} assignments, converged {reps[0]['converged']}, moved at the last {reps[0]['n_moved']}, "
        f"empty {reps[0]['n_empty']}, largest word {reps[0]['max_members']}")
    say(f"  per iteration: assignment {a / n_assign:.2f} ms, sort {s_ / n_upd:.3f} ms, update {u / n_upd:.3f} ms (HIP events, medians of 3 after a warm-up); "
        f"sort + update {'<' if (s_ + u) / n_upd < a / n_assign else '>='} assignment")
    say(f"  update reads {row_bytes / 1e9:.3f} GB of rows: {row_bytes / (u / n_upd * 1e-3) / 1e12:.3f} TB/s, {100.0 * row_bytes / (u / n_upd * 1e-3) / HBM_BYTES_PER_S:.1f} % of {HBM_BYTES_PER_S / 1e12:.0f} TB/s")
    for name, vv, idf in (("sampled", init, False), ("trained", v, False), ("trained + idf", v, True)):
        vv.set_weighting(api.VOCAB_WEIGHT_IDF if idf else api.VOCAB_WEIGHT_COUNTS)
        cells = []
        for top_k in (2, 4, 8, 20):
            ps = {(int(x), int(y)) for x, y in ctx.propose_pairs(vv, ids, top_k)}
            cells.append(f"top_k {top_k}: {len(ps & target) / max(len(target), 1):.4f} ({len(ps)} pairs)")
        say(f"  recall of the {target_name}, {name}: " + ", ".join(cells))
    v.close(); init.close()
if len(sys.argv) > 4 and sys.argv[4] == "train":
    ctx.close()
    out.close()
    sys.exit(0)

for n_words in (4096, 16384):
    reps = []
    for it in range(4):                                             # the first is the warm-up
        v = ctx.vocab_sample(ids, n_words)
        torch.cuda.synchronize()
        t = time.perf_counter()
        prop = ctx.propose_pairs(v, ids, 20)
        wall = (time.perf_counter() - t) * 1e3
        r = ctx.vocab_report(v); r["wall"] = wall
        v.close()
        if it:
            reps.append(r)
    ps = {(int(a), int(b)) for a, b in prop}
    rec = len(ps & target) / max(len(target), 1)
    say(f"n_words {n_words} top_k 20: quantise {med([r['ms_quantise'] for r in reps]):.2f} ms, histogram {med([r['ms_histogram'] for r in reps]):.3f} ms, "
        f"score {med([r['ms_score'] for r in reps]):.3f} ms, select {med([r['ms_select'] for r in reps]):.3f} ms, call wall {med([r['wall'] for r in reps]):.2f} ms "
        f"(medians of 3 after a warm-up; {reps[0]['n_rows_quantised']} rows quantised per call)")
    say(f"  proposed {len(ps)} of {len(allp)} pairs ({100.0 * len(ps) / len(allp):.2f} %), recall of the {target_name}: {rec:.4f} ({len(ps & target)} / {len(target)})")
    if exhaustive:
        ta, tp = [], []
        for _ in range(3):                                          # alternating, one process
            ta.append(timed_match(allp)[1]); tp.append(timed_match(prop)[1])
        say(f"  r3dm_match_pairs: all pairs {med(ta):.1f} ms, proposed pairs {med(tp):.1f} ms (medians of 3, alternating)")
    else:
        tp = [timed_match(prop)[1] for _ in range(4)][1:]
        say(f"  r3dm_match_pairs on the proposed pairs: {med(tp):.1f} ms (median of 3 after a warm-up)")

# the preemptive gate on the same views (no priorities: the head of a view is its first 128 rows), threshold 4
tg = []
for it in range(4):
    counts = ctx.preselect_pairs(allp, 128, 0.6, True)
    r = ctx.preselect_report()
    if it:
        tg.append((r["ms_kernels"], r["ms_wall"]))
kept = {(int(a), int(b)) for (a, b), c in zip(allp, counts) if c >= 4}
say(f"preemptive gate (r3dm_preselect_pairs, head 128, min_matches 4, views without priorities): kernels {med([t[0] for t in tg]):.2f} ms, wall {med([t[1] for t in tg]):.2f} ms, "
    f"kept {len(kept)} of {len(allp)} pairs ({100.0 * len(kept) / len(allp):.2f} %), recall of the {target_name}: {len(kept & target) / max(len(target), 1):.4f}")
ctx.close()
out.close()
