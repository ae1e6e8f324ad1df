"""Cost and effect of the match budget on one MI355X (r3dm_set_match_budget; profiles/budget_perf.txt):
    python tools/budget_perf.py [<output file>] [<n_views>]
bench.py's C2 views (200 x 8,192 x SIFT-128, synth.make_scene_torch seed 2002) with one priority per WORLD point, so that shared points
rank alike across views (an unshared feature gets a priority of its own), at N = 2,048 and N = 4,096: HIP-event times of the select,
gather and remap kernels of the call that builds the sub-views; wall time of r3dm_match_pairs with the switch on (sub-views cached) and
off, alternating in one process; the share of the exhaustive run's pairs with F-inliers, and of their inlier matches, that survive
under the budget.  Reported, not gated: what the budget buys depends on real scales."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from regard3d_amd import api, synth  # noqa: E402

out = open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, "a")
n_views = int(sys.argv[2]) if len(sys.argv) > 2 else 200


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    out.write(line + "\n"); out.flush()


def med(xs):
    return sorted(xs)[len(xs) // 2]


descs, xys, wids = synth.make_scene_torch(n_views, 8192, seed=2002, device="cuda:0", kind="sift")
hd = [descs[i].cpu().numpy() for i in range(n_views)]
hx = [xys[i].cpu().numpy() for i in range(n_views)]
hw = [wids[i].cpu().numpy() for i in range(n_views)]
del descs, xys, wids
torch.cuda.empty_cache()
rng = np.random.default_rng(2002)
world_prio = rng.random(int(max(w.max() for w in hw)) + 1).astype(np.float32)
prios = [np.where(w >= 0, world_prio[np.maximum(w, 0)], rng.random(len(w)).astype(np.float32)).astype(np.float32) for w in hw]
ctx = api.Context(0)
ids = list(range(n_views))
ctx.set_images(ids, hd, hx, synth.WIDTH, synth.HEIGHT, wait=True)
for v in ids:
    ctx.set_view_priority(v, prios[v])
ii, jj = np.triu_indices(n_views, k=1)
allp = np.stack([ii, jj], 1).astype(np.uint32)
say(f"# {n_views} views x 8192 x SIFT-128 (synth.make_scene_torch seed 2002: bench.py's C2 views), {len(allp)} pairs, one priority per world point")


def timed_match():
    torch.cuda.synchronize()
    t = time.perf_counter()
    g = ctx.match_pairs(allp, 0.6, True)
    torch.cuda.synchronize()
    return g, (time.perf_counter() - t) * 1e3


def inliers(g):
    gf = ctx.filter_F(g, 4.0, 2048, seed=5489)
    return {(int(a), int(b)) for a, b in gf.pairs}, gf.num_matches


timed_match()                                                       # warm-up
g_off, _ = timed_match()
pairs_off, m_off = inliers(g_off)
say(f"switch off: {g_off.num_pairs} putative pairs / {g_off.num_matches} matches, {len(pairs_off)} pairs with F inliers / {m_off} inlier matches")
for N in (2048, 4096):
    ctx.set_match_budget(True, N)
    g_on, t_build = timed_match()
    r = ctx.budget_report()
    say(f"N {N}: the call that builds the sub-views: select {r['ms_select']:.3f} ms, gather {r['ms_gather']:.3f} ms, remap {r['ms_remap']:.3f} ms (HIP events), "
        f"budget's share of the wall {r['ms_wall']:.1f} ms of {t_build:.1f} ms; {r['n_views_budgeted']} views budgeted, {r['n_subviews_built']} sub-views built, "
        f"{r['n_rows_selected']} rows selected, {r['n_matches_remapped']} matches remapped")
    t_on, t_off = [], []
    for _ in range(3):                                              # alternating, one process
        ctx.set_match_budget(True, N); t_on.append(timed_match()[1]); share = ctx.budget_report()
        ctx.set_match_budget(False, N); t_off.append(timed_match()[1])
    say(f"  r3dm_match_pairs wall: switch on {med(t_on):.1f} ms [{min(t_on):.1f}, {max(t_on):.1f}] (sub-views cached: budget's share {share['ms_wall']:.2f} ms, "
        f"remap {share['ms_remap']:.3f} ms), switch off {med(t_off):.1f} ms [{min(t_off):.1f}, {max(t_off):.1f}] (medians of 3, alternating)")
    pairs_on, m_on = inliers(g_on)
    say(f"  {g_on.num_pairs} putative pairs / {g_on.num_matches} matches; pairs with F inliers {len(pairs_on & pairs_off)} of {len(pairs_off)} "
        f"({100.0 * len(pairs_on & pairs_off) / max(len(pairs_off), 1):.1f} %), inlier matches {m_on} of {m_off} ({100.0 * m_on / max(m_off, 1):.1f} %)")
ctx.close()
out.close()
