"""Within-process A/B of the L2 kernel variants is not possible (variant is latched per process), so this
runs one variant per invocation on a mid-size workload and prints kernel TFLOP/s (HIP events)."""
import os, sys, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from regard3d_amd import api, synth
import os as _os
if any(k.startswith("R3DM_") for k in _os.environ):
    api.use_developer_library()      # R3DM_* knobs / traces exist only in the developer build (build.sh dev); otherwise measure the product
n_img = int(sys.argv[1]) if len(sys.argv) > 1 else 48
kind = sys.argv[2] if len(sys.argv) > 2 else "sift"
if kind == "sift":
    descs, xys, _ = synth.make_scene_torch(n_img, 8192, seed=2002, device="cuda")
else:
    sc = synth.make_scene(n_img, 8192, kind, seed=2002)
    descs = [torch.from_numpy(d).cuda() for d in sc.descs]; xys = [torch.from_numpy(x).cuda() for x in sc.xys]
c = api.Context(0)
if len(sys.argv) > 3 and sys.argv[3] == "noprune":
    c.set_prefix_pruning(False)          # the kernel without prefix pruning (R3DM_L2_VARIANT 109 .. 112: the prefix test alone with GP = 9 .. 12; 120: the pair-norm filter alone; default: the cascade)
if len(sys.argv) > 3 and sys.argv[3] == "nohalf":
    c.set_half_filter(False)             # the cascade without the f16 level in front (R3DM_L2_VARIANT 130: the f16 level, then straight to the restart; 131 / 132: its window 1 / 2 blocks deep; 133: the three levels without the skip of level 2; default: the three levels, level 2 skipped where it cannot prune)
if len(sys.argv) > 3 and sys.argv[3] == "nomin":
    c.set_min_tile_test(False)           # the three levels with the general form of their tile tests (R3DM_L2_VARIANT 136 forces it too; 134: level 1 alone, no tile ever goes on; 135: level 1 alone without its decision -- both timing only; default: the min form where the norms allow it)
if len(sys.argv) > 3 and sys.argv[3] == "noprefix16":
    c.set_half_prefix(False)             # the three levels without the f16 prefix test in front of the restart (R3DM_L2_VARIANT 139 forces that too; 137 / 138: 134 / 135 in the min form, timing only; default: the test runs where the three levels do)
for i in range(n_img): c.set_image(i, descs[i], xys[i], 4000, 3000)
ii, jj = np.triu_indices(n_img, k=1); pairs = np.stack([ii, jj], 1).astype(np.uint32)
res = []
for rep in range(4):
    g = c.match_pairs(pairs, 0.6, True); s = c.stats()
    res.append(s.algorithmic_flops / (s.ms_match_kernels * 1e-3) / 1e12)
tested, pruned = c.prefix_pruning_counts()
print(json.dumps({"variant": os.environ.get("R3DM_L2_VARIANT", "default"), "tiles_pruned_share": round(pruned / tested, 4) if tested else None,
                  "tiles_filtered_share": round(c.pair_filter_counts() / tested, 4) if tested else None,
                  "tiles_half_share": round(c.half_filter_counts() / tested, 4) if tested else None,
                  "tiles_level2_skipped_share": round(c.level2_skip_counts() / tested, 4) if tested else None, "pairs_min_form_general_form": c.min_tile_test_counts(), "tiles_f16_prefix_reached_pruned": c.half_prefix_counts(), "kernel_ms": round(s.ms_match_kernels, 2), "pairs": len(pairs), "tflops": [round(x, 2) for x in res], "kind": kind, "matches": g.num_matches, "queries": s.n_queries, "fallback": s.n_exact_fallback}))
