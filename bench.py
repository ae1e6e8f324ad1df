#!/usr/bin/env python
"""bench.py -- image-pairs matched/sec (+ F-inlier filter) on MI355X, BASELINE.json's metric.

A "step" = one pass of the hot path over the whole pair list of the workload: 2-NN matching (fused MFMA squared-L2 /
popcount Hamming / graph search, exact re-scoring, ratio test), per-pair finalisation, the AC-RANSAC fundamental-matrix
filter, the result graphs back in host RAM and -- for N > 1 -- the single all-gather that reassembles the pairwise match
graph on every rank.  Descriptors are resident in HBM before the timed region starts (r3dm_set_images copied them from host
memory and laid them out: `detail.register_ms`; `detail.value_from_host` is one measured pass that starts at the host arrays).

--config (default c2; the driver runs the default):
  c2       BASELINE configs[1]: 200 images x 8192 SIFT-128 f32 (integer-valued bins), exhaustive 19,900 pairs, brute-force L2
           2-NN + ratio 0.6 + F AC-RANSAC (4 px, 2048 it).  The metric ("200 img x 8k SIFT-128, 1/2/4/8 GPU") is quoted on it.
  c3       configs[2]: 200 x 8192 x 486-bit A-KAZE MLDB (61 bytes, stored 64), Hamming brute force (popcount), ratio 0.8.
  c4       configs[3]: 1000 x 8192 SIFT-128, 499,500 pairs, sharded over the GPUs + one all-gather.
  c5       configs[4]: 1000 x 16384 SIFT-128, KGraph-style approximate 2-NN (graph index + graph search) + F filter.
  liop144  what Regard3D actually matches (src/Regard3DFeatures.h:44-48): 200 x 8192 x f32[144], real-valued, unit length.
  liop144c the same collection in the form vl_liop.c EMITS its rows (integer votes divided by their norm, vl_liop.c:553-575): the opt-in
           leg then nominates on count tiles (one f16 MFMA per 16 dimensions instead of the split nominator's three).
  stage    the reference's DEFAULT stage end to end, one facade call per step (R3DComputeMatches::computeMatches): N synthetic
           4000 x 3000 photographs resident in HBM -> Fast-A-KAZE + LIOP -> .feat/.desc -> LIOP-144 matching (arm 9, and arm 0 =
           the GUI default) -> F + E + H AC-RANSAC -> matches.*.txt/.bin; per-phase times, a roofline for the detector and one
           for the essential-matrix kernel (N = 1 only; --images sets N, default 32).
N > 1 (one rank per GPU, torchrun): the SAME collection, pairs dealt to the ranks by rows of I (r3dm_shard_pairs), descriptors
replicated -- "scaling": "strong", exactly the metric's "1/2/4/8 GPU" -- unless --scaling weak (image count grows so that
the pair count is ~N x the base).  --emulate-world W at N = 1 runs shard 0 of a W-way job (what one GPU of a W-GPU node
does for c4 / c5, whose full pair lists take minutes on one GPU); --images overrides the collection size; both are
spelled out in config.workload.

Prints ONE JSON line (rank 0).  `roofline` is for the dominant kernel of the config, timed live with HIP events on the
library's stream; `cpu_baseline` times the CPU restatement (oracle/, OpenMP over J like the reference) on a bounded
sample of the same workload on the host cores of this box, and doubles as a full-size parity check.
"""
import argparse
import ctypes
import hashlib
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from regard3d_amd import api, dist as r3dist, synth

from bench_legs import (FP32_MFMA_PEAK_TFLOPS, BF16_MFMA_PEAK_TFLOPS, HBM_PEAK_GBS, attach_traffic, opt_in_hamming, opt_in_integer, opt_in_split,
                        roofline, stage_main)

CONFIGS = {
    "c2": dict(kind="sift", images=200, feat=8192, seed=2002, matcher="brute", ratio=0.6, squared=True,
               what="SIFT-128 f32 descriptors (integer-valued bins)", how="brute-force L2 2-NN"),
    "c3": dict(kind="akaze", images=200, feat=8192, seed=3003, matcher="brute", ratio=0.8, squared=False,
               what="A-KAZE MLDB 486-bit binary descriptors (61 bytes, stored 64)", how="brute-force Hamming 2-NN (popcount)"),
    "c4": dict(kind="sift", images=1000, feat=8192, seed=4004, matcher="brute", ratio=0.6, squared=True,
               what="SIFT-128 f32 descriptors (integer-valued bins)", how="brute-force L2 2-NN"),
    "c5": dict(kind="sift", images=1000, feat=16384, seed=5005, matcher="kgraph", ratio=0.6, squared=True,
               what="SIFT-128 f32 descriptors (integer-valued bins)", how="KGraph-style approximate 2-NN (graph index K 24 + pool search P 10 S 10)"),
    "liop144": dict(kind="liop", images=200, feat=8192, seed=2002, matcher="brute", ratio=0.6, squared=True,
                    what="LIOP-like f32[144] descriptors (real-valued, unit length)", how="brute-force L2 2-NN"),
    "liop144c": dict(kind="liopc", images=200, feat=8192, seed=2002, matcher="brute", ratio=0.6, squared=True,
                     what="LIOP-144 f32 descriptors in the form vl_liop emits (integer votes over their norm, unit length)", how="brute-force L2 2-NN"),
}


def images_for_weak(n_gpus: int, base_images: int) -> int:
    if n_gpus <= 1:
        return base_images
    target = n_gpus * base_images * (base_images - 1) // 2
    return int(round((1 + math.sqrt(1 + 8 * target)) / 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--config", choices=sorted(CONFIGS) + ["stage"], default="c2")
    ap.add_argument("--stage-size", default="4000x3000", help="--config stage: image size WxH")
    ap.add_argument("--stage-features", default="3x8", help="--config stage: detector batches in flight x images per batch")
    ap.add_argument("--stage-quick", action="store_true", help="--config stage: the timed steps only (no arm re-runs, rooflines or CPU leg): tuning runs")
    ap.add_argument("--images", type=int, default=0, help="override the collection size of the config (stated in config.workload)")
    ap.add_argument("--feat", type=int, default=0, help="override the features per image of the config")
    ap.add_argument("--scaling", choices=["strong", "weak"], default="strong")
    ap.add_argument("--via-c-abi", action="store_true",
                    help="reassemble the graphs through the library's own RCCL entry (r3dm_allgather_graphs) instead of torch.distributed; same graphs_sha16")
    ap.add_argument("--emulate-world", type=int, default=0, help="N = 1 only: run shard 0 of a W-way job")
    ap.add_argument("--views-from", choices=["rank0", "each"], default="rank0",
                    help="N > 1: rank 0 generates the synthetic collection and broadcasts it (default), or every rank generates it from the seed")
    ap.add_argument("--cpu-seconds", type=float, default=20.0, help="rough budget of the CPU baseline leg")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-stage-leg", action="store_true", help="skip the short pass of the stage leg (pixels -> matches.*) appended to the default line as `stage_leg`")
    ap.add_argument("--no-opt-in", action="store_true", help="skip the extra (untimed-region) pass on the opt-in fast path of the config")
    ap.add_argument("--dump-outputs", metavar="DIR", default="",
                    help="write the graphs the last timed step returned as DIR/<name>.npy (see dump_outputs); not with --config stage")
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    if a.dump_outputs and a.config == "stage":
        ap.error("--dump-outputs covers the collection configs; the stage leg writes its results as files")
    if a.config == "stage":
        return stage_main(a, cpu_baseline_fn=stage_cpu_baseline)
    cfg = dict(CONFIGS[a.config])
    if a.feat:
        cfg["feat"] = a.feat

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != max(a.gpus, 1) and rank == 0:
        print(f"# note: --gpus {a.gpus} but WORLD_SIZE={world}; using WORLD_SIZE", file=sys.stderr)
    # test hooks (CI on a 1-GPU box): R3DM_SHARE_GPU=1 maps every rank to cuda:0, R3DM_DIST_BACKEND=gloo exchanges
    # the graphs through host tensors; the defaults are one GPU per rank and RCCL
    if os.environ.get("R3DM_SHARE_GPU") == "1":
        local_rank = 0
    backend = os.environ.get("R3DM_DIST_BACKEND", "nccl")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    xdev = dev if backend == "nccl" else torch.device("cpu")
    if world > 1:
        import torch.distributed as td
        if backend == "nccl":
            td.init_process_group("nccl", device_id=dev)      # RCCL over xGMI
        else:
            td.init_process_group(backend)

    base_images = a.images or cfg["images"]
    n_images = images_for_weak(world, base_images) if a.scaling == "weak" else base_images
    n_feat = cfg["feat"]
    kind = cfg["kind"]
    binary = kind == "akaze"
    if world > 1 and a.views_from == "rank0":
        # the collection exists ONCE: rank 0 generates it and every other rank receives the same bytes (each GPU matches its rows of I
        # against all later views, so every rank needs (nearly) every view: descriptors are replicated by design) -- one
        # broadcast over the fabric instead of N generations, and no reliance on N devices drawing identical random streams
        import torch.distributed as td
        meta = [None]
        if rank == 0:
            descs, xys, _ = synth.make_scene_torch(n_images, n_feat, seed=cfg["seed"], device=dev, kind=kind)
            meta = [(tuple(descs.shape), str(descs.dtype), tuple(xys.shape), str(xys.dtype))]
        td.broadcast_object_list(meta, src=0)
        if rank != 0:
            dsh, ddt, xsh, xdt = meta[0]
            descs = torch.empty(dsh, dtype=getattr(torch, ddt.split(".")[-1]), device=dev)
            xys = torch.empty(xsh, dtype=getattr(torch, xdt.split(".")[-1]), device=dev)
        for t in (descs, xys):
            if xdev.type == "cpu":                          # (the gloo test hook: through host memory)
                h = t.cpu()
                td.broadcast(h, src=0)
                if rank != 0:
                    t.copy_(h)
            else:
                td.broadcast(t, src=0)
    else:
        descs, xys, _ = synth.make_scene_torch(n_images, n_feat, seed=cfg["seed"], device=dev, kind=kind)
    dim = int(descs.shape[2])
    torch.cuda.synchronize()
    # SURVEY.md section 8(d) starts the metric at "descriptors resident in host RAM": the collection goes to the host (pageable numpy
    # arrays, what a caller that loaded .desc files holds) and is REGISTERED FROM THERE -- r3dm_set_images: page-locked ring, one DMA +
    # one kernel per view -- cold (the context allocates the views' buffers) and warm (recycled buffers: a long-lived stage object).
    # `value` times the steps with the views resident, as the bench contract prescribes; `detail.value_from_host` is a measured full
    # pass that starts at the host arrays: clear -> register -> match -> filter -> exchange.
    hd = [descs[i].cpu().numpy() for i in range(n_images)]
    hx = [xys[i].cpu().numpy() for i in range(n_images)]
    del descs, xys
    torch.cuda.empty_cache()
    view_ids = list(range(n_images))
    raw_bytes = sum(d.nbytes for d in hd)
    ctx = api.Context(local_rank)
    hbm_free0 = torch.cuda.mem_get_info(local_rank)[0]

    def register():
        t = time.perf_counter()
        ctx.set_images(view_ids, hd, hx, synth.WIDTH, synth.HEIGHT, binary=binary, wait=True)
        return (time.perf_counter() - t) * 1e3
    register_ms_cold = register()
    hbm_views = hbm_free0 - torch.cuda.mem_get_info(local_rank)[0]
    reg = []
    for _ in range(3):
        ctx.clear_images()
        reg.append(register())
    register_ms = sorted(reg)[1]
    ii, jj = np.triu_indices(n_images, k=1)
    pairs = np.stack([ii, jj], 1).astype(np.uint32)
    emu = a.emulate_world if (world == 1 and a.emulate_world > 1) else 0
    mine = r3dist.shard_pairs(pairs, 0, emu) if emu else r3dist.shard_pairs(pairs, rank, world)
    job_pairs = mine.shape[0] if emu else pairs.shape[0]          # pairs the whole (measured) job processes per step
    kp = api.KGraphParams.preset(3) if cfg["matcher"] == "kgraph" else None

    comm = None
    if a.via_c_abi:
        # RCCL communicator of the library itself: rank 0 draws the id, the other ranks receive its 128 bytes (here through the
        # torch.distributed group that exists anyway; a C++ host would use MPI_Bcast or a file)
        uid = [api.Comm.unique_id() if rank == 0 else None]
        if world > 1:
            td.broadcast_object_list(uid, src=0)
        comm = api.Comm(uid[0], rank, world, local_rank)
        ctx.set_device_graphs(True)      # the graphs of a step keep a device mirror: r3dm_allgather_graphs sends them from device memory

    def match(p):
        if kp is not None:
            ctx.drop_indices()       # every pass builds the index of each image I again, as kgraph_match does (the build is inside the timed step)
            return ctx.match_pairs_kgraph(p, cfg["ratio"], kp)
        return ctx.match_pairs(p, cfg["ratio"], cfg["squared"])

    def step():
        g = match(mine)
        s_match = ctx.stats()
        gf = ctx.filter_F(g, 4.0, 2048, seed=5489)
        s_all = ctx.stats()
        # the one exchange of the path: through torch.distributed (default), or through the library's own RCCL entry (--via-c-abi:
        # r3dm_allgather_graphs, what a C++ host with one process per GPU calls)
        full = comm.allgather_graphs([g, gf]) if comm is not None else r3dist.all_gather_graphs([g, gf], device=xdev)
        return g, gf, full, s_match, s_all

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            td.barrier()
        torch.cuda.synchronize()

    for _ in range(a.warmup):
        step()
    fence()
    t0 = time.perf_counter()
    acc = dict(kernel_ms=0.0, flops=0.0, launches=0, filter_ms=0.0, fallback=0, queries=0, ann_ms=0.0, ann_dist=0, ann_build_ms=0.0)
    wall = {"match": 0.0, "match_post": 0.0, "filter": 0.0}
    for _ in range(a.steps):
        g, gf, full, s_match, s_all = step()
        acc["kernel_ms"] += s_match.ms_match_kernels; acc["flops"] += s_match.algorithmic_flops
        acc["launches"] += s_match.n_match_launches; acc["filter_ms"] += s_all.ms_filter_kernels
        acc["fallback"] += s_match.n_exact_fallback; acc["queries"] += s_match.n_queries
        acc["ann_ms"] += s_match.ms_ann_search; acc["ann_dist"] += s_match.n_ann_dist; acc["ann_build_ms"] += s_match.ms_ann_build
        acc["ann_rows16"] = acc.get("ann_rows16", 0) + int(s_match.n_ann_rows16); acc["ann_rows8"] = acc.get("ann_rows8", 0) + int(s_match.n_ann_rows8); acc["ann_dot8"] = acc.get("ann_dot8", 0) + int(s_match.n_ann_dot8); acc["ann_launches"] = acc.get("ann_launches", 0) + int(s_match.n_match_launches)
        wall["match"] += s_all.ms_wall_match; wall["match_post"] += s_all.ms_wall_match_post; wall["filter"] += s_all.ms_wall_filter
        acc["pairs"] = acc.get("pairs", 0) + int(mine.shape[0])
    fence()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=xdev)
        td.all_reduce(t, op=td.ReduceOp.MAX)
        elapsed = float(t.item())

    value = job_pairs * a.steps / elapsed
    dumped = dump_outputs(a.dump_outputs, {"putative": full[0], "F": full[1]}) if (a.dump_outputs and rank == 0) else None
    # one more full pass, measured from the host arrays (never `value`)
    fence()
    t0h = time.perf_counter()
    ctx.clear_images()
    ctx.set_images(view_ids, hd, hx, synth.WIDTH, synth.HEIGHT, binary=binary)
    step()
    fence()
    from_host_s = time.perf_counter() - t0h
    if world > 1:
        t = torch.tensor([from_host_s], dtype=torch.float64, device=xdev)
        td.all_reduce(t, op=td.ReduceOp.MAX)
        from_host_s = float(t.item())
    scope = (f"shard 0 of {emu} of the exhaustive {pairs.shape[0]} pairs = {job_pairs} pairs (what one GPU of a {emu}-GPU node runs)" if emu
             else f"exhaustive {pairs.shape[0]} pairs")
    note = "" if (base_images == CONFIGS[a.config]["images"] and n_feat == CONFIGS[a.config]["feat"]) else \
        f" [collection size overridden: BASELINE names {CONFIGS[a.config]['images']} x {CONFIGS[a.config]['feat']}]"
    out = {
        "metric": "image-pairs matched/sec (+ F-inlier filter)",
        "value": value, "unit": "pairs/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
        "ms_per_step": elapsed / a.steps * 1e3, "higher_is_better": True, "scaling": a.scaling if world > 1 else "strong",
        "vs_baseline": None, "dtype": "u32 (xor + popcount)" if binary else "f32", "data": "synthetic",
        "config": {"workload": f"{a.config}: {n_images} images x {n_feat} {cfg['what']}, {scope}, {cfg['how']} + ratio {cfg['ratio']} "
                               "+ F-matrix AC-RANSAC (4 px, 2048 it)" + note
                               + ("" if world == 1 else f", pairs sharded over {world} GPUs by rows of I + 1 all-gather"),
                   "name": a.config, "images": n_images, "features_per_image": n_feat, "dim": dim, "pairs": int(job_pairs),
                   "pairs_this_rank": int(mine.shape[0]), "parallelism": f"pair-shard x{world}"},
    }
    out["roofline"] = roofline(a.config, cfg, acc, dim, world)
    out["detail"] = {"register_ms": register_ms, "register_ms_cold": register_ms_cold, "register_GB_per_s": raw_bytes / (register_ms * 1e-3) / 1e9,
                     "register": (f"r3dm_set_images of the {n_images} views from pageable host memory ({raw_bytes / 1e6:.0f} MB of rows) until resident and laid out "
                                  "(median of 3 with recycled buffers; _cold: the first, buffers allocated)" + (" -- on every rank: descriptors are replicated" if world > 1 else "")),
                     "hbm_views_MB": hbm_views / 1e6, "hbm_views_over_raw_rows": hbm_views / max(raw_bytes, 1),
                     "value_from_host": job_pairs / from_host_s, "ms_from_host": from_host_s * 1e3,
                     "from_host": "one measured pass that starts at the host arrays: clear_images + r3dm_set_images + match + F filter + exchange (SURVEY 8(d)'s clock)",
                     "filter_kernel_ms_per_step": acc["filter_ms"] / a.steps, "match_kernel_ms_per_step": (acc["kernel_ms"] + acc["ann_ms"]) / a.steps,
                     "wall_ms_per_step": {k: v / a.steps for k, v in wall.items()},
                     "match_only_pairs_per_s_this_rank": (mine.shape[0] * a.steps / (wall["match"] * 1e-3)) if wall["match"] > 0 else None,
                     "exact_fallback_queries_per_step": acc["fallback"] / a.steps, "queries_per_step": acc["queries"] / a.steps,
                     "exact_fallback_fraction": acc["fallback"] / max(acc["queries"], 1),
                     "exchange": (f"r3dm_allgather_graphs: the library's RCCL entry (C ABI), sizes + padded payload; {comm.last_device_graphs} of 2 local graphs sent from their device mirror" if comm is not None else
                                  "torch.distributed all_gather of sizes + padded payload (" + (backend if world > 1 else "one rank: nothing to exchange") + ")"),
                     "putative_pairs": int(full[0].num_pairs), "putative_matches": int(full[0].num_matches),
                     "F_pairs": int(full[1].num_pairs), "F_matches": int(full[1].num_matches),
                     # identity of the reassembled graphs (pairs, offsets, matches of both): equal across N for the same collection
                     "graphs_sha16": hashlib.sha256(b"".join(np.ascontiguousarray(getattr(gr, f)).tobytes() for gr in full for f in ("pairs", "offsets", "matches"))).hexdigest()[:16]}
    if kp is not None:
        out["detail"].update({"ann_index_build_ms_per_step": acc["ann_build_ms"] / a.steps, "ann_search_ms_per_step": acc["ann_ms"] / a.steps,
                              "ann_evaluations_per_query": acc["ann_dist"] / max(acc["queries"], 1)})
        if world == 1:
            # what BASELINE config 5 exists to report: "ANN vs brute-force recall / throughput" (outside the timed region)
            out["detail"].update(ann_vs_exhaustive(ctx, cfg, kp, mine, hd, value))
            r = out["roofline"]
            # the second bound SURVEY 8(d) names for this config: the bytes the search gathers against the HBM roof
            gb = r.get("gathered_GB_per_s", 0.0)
            r["bounds"] = {"valu_issue": {"achieved": r["achieved"], "peak": r["peak"], "unit": r["unit"], "frac": r["frac"]},
                           "gathered_bytes_over_hbm": {"achieved": gb, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gb / HBM_PEAK_GBS,
                                                       "note": "evaluations x row bytes / search time: what the search asks its caches for; "
                                                               "99 % of it is served by L1 / L2 (traffic: the HBM-side bytes)"}}

    # Outside the timed region, N = 1 only: the same step on the opt-in fast path of the config (bit-identical results;
    # DESIGN.md).  Reported beside the headline, never as `value`: the headline stays on the arithmetic the north star names.
    named_size = (not emu) and base_images == CONFIGS[a.config]["images"] and n_feat == CONFIGS[a.config]["feat"]
    if world == 1 and not a.no_opt_in and kp is None and kind == "sift":
        out["opt_in_integer_mfma"] = opt_in_integer(ctx, step, fence, g, gf, job_pairs)
        attach_traffic(out["opt_in_integer_mfma"]["roofline"], a.config, "l2_knn2_int_kernel", named_size)
    if world == 1 and not a.no_opt_in and kp is None and kind == "akaze":
        out["opt_in_hamming_mfma"] = opt_in_hamming(ctx, step, fence, g, gf, job_pairs)
    if world == 1 and not a.no_opt_in and kp is None and kind in ("liop", "liopc"):
        out["opt_in_split_mfma"] = opt_in_split(ctx, step, fence, g, gf, job_pairs)
        attach_traffic(out["opt_in_split_mfma"]["roofline"], a.config, out["opt_in_split_mfma"]["roofline"]["kernel"].split("<")[0], named_size)
    if world == 1:
        attach_traffic(out["roofline"], a.config, out["roofline"]["kernel"].split("<")[0], named_size)
    if rank == 0 and world == 1 and not a.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(a.config, cfg, ctx, hd, hx, g, gf, a.cpu_seconds, kp)
    # Outside the timed region, N = 1, the default leg only: a short pass of the STAGE leg (`--config stage`: 16 photographs of 12 Mpx from
    # pixels to matches.{putative,f,e,h} through the one facade call), so that the line the driver records also carries what the reference's
    # default stage costs around the headline kernel.  Never part of `value`.
    if rank == 0 and world == 1 and a.config == "c2" and not a.no_stage_leg and not emu and not a.images and not a.feat:
        try:
            del hd, hx
            ctx.clear_images()
            torch.cuda.empty_cache()
            out["stage_leg"] = stage_main(a, embed={"images": 16, "steps": 3, "warmup": 2})
            out["stage_leg"]["note"] = ("python bench.py --config stage is the full leg (per-phase ms, detector and E-filter rooflines, CPU baseline, "
                                        "the GUI's default arm); profiles/r03_end_bench_stage.json")
        except Exception as e:                    # the headline stands on its own
            out["stage_leg"] = {"error": str(e)[:300]}
    if dumped is not None:
        out["dump_outputs"] = dumped
    if rank == 0:
        print(json.dumps(out))
    if world > 1:
        td.barrier()
        td.destroy_process_group()


DUMP_LIMIT_BYTES = 64 * 10**6        # the .npy files of a dump in all, headers included


def _pair_draw(pairs):
    """a fixed pseudo-random number in [0, 1) per pair (I, J) (splitmix64 of I * 2^32 + J): a sample drawn with it keeps the same
    pairs whatever else a graph holds, so that the dumps of two builds stay comparable pair by pair"""
    with np.errstate(over="ignore"):
        z = (pairs[:, 0].astype(np.uint64) << np.uint64(32)) | pairs[:, 1].astype(np.uint64)
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) / float(1 << 53)


def dump_outputs(out_dir, graphs):
    """What the last timed step returned, the reassembled graphs {name: api.Graph}, as out_dir/<name>_{pairs,offsets,matches}.npy:
    pairs (view ids) and matches (feature indices) in float32, where every index below 2^24 is exact; offsets in float64.  Above
    DUMP_LIMIT_BYTES in all, every graph is cut to the pairs whose _pair_draw falls below one fraction (offsets rebuilt for the
    sample).  Returns what was written, for the JSON line."""
    arrays = {n: (g.pairs, g.offsets.astype(np.int64), g.matches) for n, g in graphs.items()}
    for p, _, m in arrays.values():
        assert (p.size == 0 or int(p.max()) < 1 << 24) and (m.size == 0 or int(m.max()) < 1 << 24), "index not exact in float32"

    def nbytes(arr):
        return sum(p.size * 4 + o.size * 8 + m.size * 4 + 3 * 128 for p, o, m in arr.values())      # (128 B: one .npy header)
    frac, sampled = 1.0, dict(arrays)
    while nbytes(sampled) > DUMP_LIMIT_BYTES:
        frac *= 0.9 * DUMP_LIMIT_BYTES / nbytes(sampled)
        sampled = {}
        for n, (p, o, m) in arrays.items():
            keep = np.flatnonzero(_pair_draw(p) < frac)
            counts = o[keep + 1] - o[keep]
            rows = np.concatenate([np.arange(o[k], o[k + 1]) for k in keep]) if keep.size else np.zeros(0, np.int64)
            sampled[n] = (p[keep], np.concatenate([[0], np.cumsum(counts)]), m[rows])
    os.makedirs(out_dir, exist_ok=True)
    files = {}
    for n, (p, o, m) in sampled.items():
        for what, arr in (("pairs", p.astype(np.float32)), ("offsets", o.astype(np.float64)), ("matches", m.astype(np.float32))):
            np.save(os.path.join(out_dir, f"{n}_{what}.npy"), arr)
            files[f"{n}_{what}"] = list(arr.shape)
    return {"dir": out_dir, "files": files, "bytes": nbytes(sampled), "pairs_fraction": frac,
            "note": "the graphs the last timed step returned (pairs / matches float32, offsets float64)"
                    + ("" if frac == 1.0 else f"; a fixed per-pair sample (_pair_draw < {frac:.6g}) to stay within {DUMP_LIMIT_BYTES // 10**6} MB")}


def ann_vs_exhaustive(ctx, cfg, kp, mine, hd, ann_value):
    """C5 is 'KGraph-style approximate kNN ... (ANN vs brute-force recall / throughput)': on a seeded sample of this rank's pairs the
    graph matcher's putative matches against the exhaustive matcher's (precision / recall / F1 of the match SET, what the stage
    consumes), raw recall@1 / recall@2 of the 2-NN on a few pairs (r3dm_kgraph_knn2 vs r3dm_knn2), and what the exhaustive matcher does
    on the same 16 k-row views -- f32 tiles (the default) and the opt-in integer tiles.
    Reference: kgraph_match presets /root/reference/src/R3DComputeMatches.cpp:808-902, search src/thirdparty/kgraph/kgraph.cpp:411-552."""
    rng = np.random.default_rng(5005)
    S = int(min(400, mine.shape[0]))
    sample = mine[np.sort(rng.choice(mine.shape[0], S, replace=False))]
    ga = ctx.match_pairs_kgraph(sample, cfg["ratio"], kp)

    def timed(fn):
        fn()                                                # (layouts staged on first use, kernels loaded)
        torch.cuda.synchronize()
        t = time.perf_counter()
        g = fn()
        torch.cuda.synchronize()
        return g, time.perf_counter() - t
    ge, t_f32 = timed(lambda: ctx.match_pairs(sample, cfg["ratio"], cfg["squared"]))
    ctx.set_integer_mfma(True)
    try:
        gi, t_int = timed(lambda: ctx.match_pairs(sample, cfg["ratio"], cfg["squared"]))
    finally:
        ctx.set_integer_mfma(False)
    same_int = all(np.array_equal(getattr(ge, f), getattr(gi, f)) for f in ("pairs", "offsets", "matches"))
    da, de = ga.as_dict(), ge.as_dict()
    tp = n_a = n_e = 0
    for k in set(da) | set(de):
        A = set(map(tuple, da.get(k, np.zeros((0, 2), np.uint32)).tolist())); E = set(map(tuple, de.get(k, np.zeros((0, 2), np.uint32)).tolist()))
        tp += len(A & E); n_a += len(A); n_e += len(E)
    prec = tp / max(n_a, 1); rec = tp / max(n_e, 1)
    f1 = 2 * prec * rec / max(prec + rec, 1e-30)
    # raw 2-NN recall on a few pairs
    r1 = r2 = nq = rm = nm = 0
    R = cfg["ratio"] ** 2 if cfg["squared"] else cfg["ratio"]
    # (on the six sampled pairs with the most exhaustive matches: most pairs of a 1000-view collection do not overlap at all)
    richest = sorted(de, key=lambda k: -len(de[k]))[:6] or [tuple(p) for p in sample[:6].tolist()]
    for (I, J) in richest:
        ai, _ = ctx.kgraph_knn2(hd[I], hd[J], kp, pair=(int(I), int(J)))
        ei, ed = ctx.knn2(hd[I], hd[J])
        ok = ed[:, 0] != ed[:, 1]                         # (a tied pair of nearest rows has no defined first)
        r1 += int((ai[ok, 0] == ei[ok, 0]).sum())
        r2 += int(sum(len({int(x), int(y)} & {int(u), int(v)}) for (x, y), (u, v) in zip(ai[ok].tolist(), ei[ok].tolist())))
        nq += int(ok.sum())
        hit = ok & (ed[:, 0] < np.float32(R) * ed[:, 1])   # queries WITH a counterpart in I: the ones the ratio test lets through
        rm += int((ai[hit, 0] == ei[hit, 0]).sum()); nm += int(hit.sum())
    return {"ann_vs_exhaustive_sample_pairs": S,
            "recall_at_1": r1 / max(nq, 1), "recall_at_2": r2 / max(2 * nq, 1), "recall_queries": nq,
            "recall_at_1_of_queries_with_a_match": rm / max(nm, 1), "queries_with_a_match": nm,
            "recall_note": "recall_at_1 / _at_2 are over ALL queries of the 6 sampled pairs with the most matches: most rows of a view have no counterpart in the other view, their "
                           "nearest row is one of 16 k near-equidistant strangers and nothing downstream reads it; the ratio test keeps the queries WITH a "
                           "counterpart -- recall_at_1_of_queries_with_a_match, and match_set_recall / _f1 over the whole sample, are what the stage consumes",
            "match_set_precision": prec, "match_set_recall": rec, "match_set_f1": f1,
            "putative_matches_ann": n_a, "putative_matches_exhaustive": n_e,
            "exhaustive_pairs_per_s": {"f32_tiles": S / t_f32, "integer_tiles_opt_in": S / t_int, "integer_graphs_identical_to_f32": bool(same_int)},
            "ann_over_exhaustive": {"vs_f32_tiles": ann_value / (S / t_f32), "vs_integer_tiles": ann_value / (S / t_int)},
            "ann_vs_exhaustive": (f"graph matcher {ann_value:.0f} pairs/s (match + F filter + index build, the timed step) vs exhaustive matching alone "
                                  f"{S / t_f32:.0f} (f32 tiles) / {S / t_int:.0f} (integer tiles) pairs/s on the same views at match-set recall {rec:.4f}: "
                                  "on this GPU the approximate arm is the slower one against the integer tiles (DESIGN.md section 4.7)")}


def host_cores():
    """(cores this process may really use, processors it sees): the affinity mask AND the cgroup CPU quota -- a container can show 256
    processors and own 16 (`cpu.max = 1600000 100000`); OpenMP teams of 256 threads are then throttled, and `cores: 256` would overstate
    what the CPU baseline ran on."""
    seen = os.cpu_count() or 1
    n = seen
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except (AttributeError, OSError):
        pass
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            parts = open(path).read().split()
            if parts and parts[0].lstrip("-").isdigit() and int(parts[0]) > 0:
                period = int(parts[1]) if len(parts) > 1 else int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                n = max(1, min(n, int(parts[0]) // period))
            break
        except (OSError, ValueError, IndexError):
            continue
    return n, seen


def use_host_cores():
    """OpenMP teams of the oracle sized to the cores the process owns; -> (cores, processors seen)"""
    cores, seen = host_cores()
    try:
        ctypes.CDLL("libgomp.so.1").omp_set_num_threads(cores)
    except OSError:
        pass
    return cores, seen


def stage_cpu_baseline(ctx, imgs, d, K, W, H, budget_s):
    """the CPU restatement of the same chain on a bounded sample: Fast-A-KAZE + LIOP on the top-left crop of image 0 (cost is per pixel,
    so images/s scales with the crop's share of the image), then matching + F / E / H of one pair with the descriptors the stage wrote.
    The crop also goes through the GPU detector: same keypoints or the leg reports the mismatch."""
    from oracle import pyoracle as O
    O.build()
    cores, seen = use_host_cores()
    cw, ch = W // 2, H // 2
    crop = imgs[0][:ch, :cw].contiguous().cpu().numpy()
    t0 = time.perf_counter()
    ok = O.akaze_detect(crop, 0.001)["kps"]
    t_det = time.perf_counter() - t0
    t0 = time.perf_counter()
    od = O.liop_describe(O.liop_extract_patches(crop, ok, 8.0))
    t_liop = time.perf_counter() - t0
    gk, _ = ctx.detect_akaze(crop, 0.001)
    gd = ctx.extract_liop(crop, gk, 8.0)
    feats = []
    for k in (0, 1):
        raw = np.fromfile(os.path.join(d, f"img{k:04d}.desc"), np.uint8)
        n = int(np.frombuffer(raw[:8].tobytes(), np.uint64)[0])
        feats.append((np.loadtxt(os.path.join(d, f"img{k:04d}.feat"), dtype=np.float32).reshape(-1, 4)[:, :2].copy(),
                      np.frombuffer(raw[8:].tobytes(), np.float32).reshape(n, 144).copy()))
    pairs = np.array([[0, 1]], np.uint32)
    xys = [feats[0][0], feats[1][0]]; descs = [feats[0][1], feats[1][1]]
    t0 = time.perf_counter()
    counts, matches = O.match_collection(descs, xys, pairs, 0.6, True)
    t_match = time.perf_counter() - t0
    Wd = np.full(2, W, np.uint32); Hd = np.full(2, H, np.uint32)
    t0 = time.perf_counter()
    oc, om = O.filter_F_collection(xys, Wd, Hd, pairs, counts, matches, 4.0, 2048, 5489)
    O.filter_E_collection(xys, Wd, Hd, np.stack([K, K]), pairs, counts, matches, 4.0, 2048, 5489)
    O.filter_H_collection(xys, Wd, Hd, pairs, counts, matches, 4.0, 2048, 5489)
    t_filt = time.perf_counter() - t0
    g = api.Graph.load(os.path.join(d, "matches.putative.bin")).as_dict()
    gf = api.Graph.load(os.path.join(d, "matches.f.bin")).as_dict()
    share = (cw * ch) / float(W * H)
    return {"value": 1.0 / (t_match + t_filt), "unit": "pairs/s", "cores": cores, "processors_seen": seen, "kind": "port",
            "sample": f"features: the {cw}x{ch} top-left crop of image 0 through oracle/akaze.c ({t_det:.1f} s) + liop.c ({t_liop:.1f} s), OpenMP on {cores} threads; "
                      f"matching: pair (0,1) of the stage's own descriptors, brute-force L2 2-NN + ratio ({t_match:.1f} s) + F / E / H AC-RANSAC ({t_filt:.2f} s)",
            "features_images_per_s_full_size_equivalent": share / (t_det + t_liop),
            "crop_keypoints": int(len(ok)), "crop_keypoints_equal_gpu": bool(np.array_equal(ok, gk)), "crop_descriptors_equal_gpu": bool(np.array_equal(od, gd)),
            "putative_pair_0_1_equal_gpu": bool(np.array_equal(g.get((0, 1), np.zeros((0, 2), np.uint32)), matches)),
            "F_inlier_set_pair_0_1_equal_gpu": bool(set(map(tuple, gf.get((0, 1), np.zeros((0, 2), np.uint32)).tolist())) == set(map(tuple, om[:oc[0]].tolist())))}


def cpu_baseline(name, cfg, ctx, descs, xys, g, gf, budget_s, kp):
    """CPU restatement (oracle/) timed on this box's host cores on a bounded sample: image 0 against images 1..S (the
    reference's loop: I fixed, `omp parallel for schedule(dynamic)` over J, /root/reference/src/R3DComputeMatches.cpp:465;
    kgraph_match :808-902 for c5: NN-descent index of image 0 with the reference's parameters, then the searches) + the
    AC-RANSAC F filter of those pairs.  The same pairs are then compared with the GPU result (parity check for free)."""
    from oracle import pyoracle as O
    cores, seen = use_host_cores()
    n_images = len(descs)
    binary = cfg["kind"] == "akaze"
    n = int(descs[0].shape[0])
    # seconds per pair on one core, scalar code like OpenMVG's metrics: 8192^2 x 128 f32 ~ 9 s, Hamming 16 words ~ 0.7 s, graph search ~ 0.1 s
    per_pair = {"sift": 9.0, "liop": 10.0, "liopc": 10.0, "akaze": 0.7}[cfg["kind"]] * (n / 8192.0) ** 2
    if kp is not None:
        per_pair = 0.12 * (n / 16384.0)
    S = int(min(n_images - 1, max(min(cores, 16), int(cores * budget_s / per_pair))))
    if kp is not None:
        S = min(S, 96)                    # the index build of image 0 dominates; more searches add little
    hd = [descs[i] for i in range(S + 1)]
    hx = [xys[i] for i in range(S + 1)]
    sub = np.stack([np.zeros(S, np.uint32), np.arange(1, S + 1, dtype=np.uint32)], 1)
    O.build()
    t0 = time.perf_counter()
    if kp is not None:
        counts, matches, _ = O.match_collection_kgraph(hd, hx, sub, cfg["ratio"], builder="nndescent", K=16, L=24, recall=0.99, P=10, S=10)
    else:
        counts, matches = O.match_collection(hd, hx, sub, cfg["ratio"], cfg["squared"], binary=binary)
    t_match = time.perf_counter() - t0
    W = np.full(S + 1, synth.WIDTH, np.uint32); H = np.full(S + 1, synth.HEIGHT, np.uint32)
    t1 = time.perf_counter()
    oc, om = O.filter_F_collection(hx, W, H, sub, counts, matches, 4.0, 2048, 5489)
    t_filter = time.perf_counter() - t1
    how = ("NN-descent index of image 0 (K 16, L 24, the reference's default block) + graph searches" if kp is not None
           else ("brute-force Hamming 2-NN + ratio" if binary else "brute-force L2 2-NN + ratio"))
    out = {"value": S / (t_match + t_filter), "unit": "pairs/s", "cores": cores, "processors_seen": seen, "kind": "port",
           "sample": f"pairs (0,1..{S}) of the same workload: {how} ({t_match:.1f} s) + AC-RANSAC F filter ({t_filter:.2f} s), "
                     f"OpenMP over J on {cores} threads"}
    # parity of the sampled pairs at full size.  The GPU graph matcher is deterministic where the reference's NN-descent is
    # not (decision 11), so for c5 the parity model is the oracle's exact-index builder on a few pairs.
    if kp is not None:
        Sp = min(S, 3)
        counts, matches, _ = O.match_collection_kgraph(hd[:Sp + 1], hx[:Sp + 1], sub[:Sp], cfg["ratio"], builder="exact", K=kp.index_K,
                                                       L=kp.index_K, cap=64, P=kp.search_P, S=kp.search_S, seed=kp.seed, min_rows=128)
        oc, om = O.filter_F_collection(hx[:Sp + 1], W[:Sp + 1], H[:Sp + 1], sub[:Sp], counts, matches, 4.0, 2048, 5489)
        S_par = Sp
    else:
        S_par = S
    dg, dgf = g.as_dict(), gf.as_dict()
    bad_put = bad_f = 0; off = offf = 0
    for p in range(S_par):
        key = (0, p + 1)
        exp = matches[off:off + counts[p]]; off += counts[p]
        got = dg.get(key, np.zeros((0, 2), np.uint32))
        bad_put += int(not np.array_equal(got, exp))
        expf = om[offf:offf + oc[p]]; offf += oc[p]
        gotf = dgf.get(key, np.zeros((0, 2), np.uint32))
        bad_f += int(set(map(tuple, gotf.tolist())) != set(map(tuple, expf.tolist())))
    out.update({"parity_pairs_checked": S_par, "putative_mismatches": bad_put, "F_inlier_set_mismatches": bad_f})
    if name in ("c2", "c4"):
        out.update(cpu_baseline_extras(O, ctx, hd, hx, cores, S))
    return out


def cpu_baseline_extras(O, ctx, hd, hx, cores, S):
    """the same restatement on ONE thread, and an "optimised CPU" figure so that the speed-up is
    not quoted against a strawman: the reference's own vendored hnswlib::BruteforceSearch + L2Space (AVX L2Sqr loop,
    oracle/_ref, built from /root/reference/src/thirdparty/hnswlib), one image pair per host thread, 2-NN only.  Its output
    is also the reference-BUILT second opinion on the GPU path at full size: r3dm_knn2 of the same pairs must return the
    same indices (rows whose three smallest distances are distinct -- equal distances have no defined order in either
    implementation) and bit-equal distances."""
    import ctypes
    extra = {}
    try:
        gomp = ctypes.CDLL("libgomp.so.1")
        gomp.omp_set_num_threads(1)
        try:
            t0 = time.perf_counter()
            O.match_collection(hd[:2], hx[:2], np.array([[0, 1]], np.uint32), 0.6, True)
            t1 = time.perf_counter() - t0
        finally:
            gomp.omp_set_num_threads(cores)
        extra["one_thread"] = {"value": 1.0 / t1, "unit": "pairs/s", "cores": 1, "kind": "port",
                               "sample": f"pair (0,1): brute-force L2 2-NN + ratio, {t1:.1f} s"}
    except OSError:
        pass
    if O.ref_lib() is not None:
        from concurrent.futures import ThreadPoolExecutor
        n = int(min(cores, S))

        def one(p):                                    # ctypes drops the GIL: the pairs run concurrently
            return O.ref_knn(hd[0], hd[p + 1], 3)
        t0 = time.perf_counter()
        with ThreadPoolExecutor(n) as ex:
            ref = list(ex.map(one, range(n)))
        t = time.perf_counter() - t0
        idx_bad = dist_bad = rows = 0
        for p in range(n):
            ridx, rdist = ref[p]
            gidx, gdist = ctx.knn2(hd[0], hd[p + 1])
            ok = (rdist[:, 0] != rdist[:, 1]) & (rdist[:, 1] != rdist[:, 2])
            idx_bad += int((gidx[ok] != ridx[ok, :2]).any(axis=1).sum())
            dist_bad += int((gdist != rdist[:, :2]).any(axis=1).sum())
            rows += int(ok.sum())
        extra["optimised_cpu"] = {"value": n / t, "unit": "pairs/s", "cores": n, "kind": "reference",
                                  "sample": f"pairs (0,1..{n}): hnswlib::BruteforceSearch + L2Space (AVX L2Sqr) built from the "
                                            f"reference's vendored source, one pair per thread, 3-NN only (no ratio / filter), {t:.1f} s",
                                  "reference_built_pairs_checked": n, "reference_built_rows_checked": rows,
                                  "reference_built_index_mismatches": idx_bad, "reference_built_distance_mismatches": dist_bad}
    return extra


if __name__ == "__main__":
    main()
