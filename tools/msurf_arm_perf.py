"""Cost of the features batch per descriptor arm with the M-SURF-64 arm among them: B same-size photographs resident in
HBM through
    detect   r3dm_detect_akaze_batch alone (counts only)
    liop     r3dm_extract_features_batch under R3DM_DESCRIPTOR_LIOP, no files (null paths): detector + patch maps + LIOP + rows to the host
    mldb     the same under R3DM_DESCRIPTOR_MLDB
    msurf    the same under R3DM_DESCRIPTOR_MSURF: detector on the M-SURF level table + items + the one M-SURF launch + rows to the host
then the split of the M-SURF batch (r3dm_stats: the launch's HIP-event time, per keypoint, with the gathered bytes / s and f64
operations / s it amounts to) and the matcher's rate on two such views as f32[64] against the same keypoints as LIOP f32[144].
    python tools/msurf_arm_perf.py [--images 8] [--size 3000 4000] [--threshold 0.001] [--reps 5] [--rounds 3] [--parent-lib PATH] [--out FILE]
Every leg runs in a process of its own (one library per process) and the legs ALTERNATE over --rounds rounds, so that a drift of the
machine shows as spread inside a leg instead of as a difference between legs.  --parent-lib names a libr3dm.so built from the parent
commit: its detect / liop / mldb legs -- and its msurf leg when that library exports the arm -- run between this tree's; they must not move
beyond the spread, which the summary states (min .. max of the rounds' medians).  A leg's figure is the median of --reps calls after one warm-up call, host clock around calls that
end in a stream synchronise, divided by the images of the batch.  One JSON line per leg and round, then a summary line.  The tool does
not time single kernels beyond the descriptor launch's event time: run `--leg msurf` under `rocprofv3 --kernel-trace --stats` for that
(tools/rocprof_summary.py)."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
THIS_LIB = os.path.join(ROOT, "regard3d_amd", "libr3dm.so")
from regard3d_amd import api        # (the arm ids: importing the package loads no library, so a leg on --parent-lib still holds that one alone)
ARM = {name.lower(): arm_id for name, arm_id in api.DESCRIPTOR_ARMS.items()}
# per keypoint (kernels_akaze.hip, ak_msurf_kernel): 16 x 81 samples, each 8 gathered floats and one ak_expf; + 16 subregion weights
SAMPLES = 16 * 81
GATHER_BYTES = SAMPLES * 8 * 4
F64_OPS = (SAMPLES + 16) * (1 + 4 + 2 * 14 + 1)        # per ak_expf: x log2e, the two-constant reduction, 14 Horner steps, the scaling


def _photos(n, h, w):
    import torch
    torch.cuda.init()          # before the library: torch's HIP runtime has to come up first in a process that uses both
    from regard3d_amd import synth
    imgs, K = synth.make_photo_set(n, h, w, seed=7007, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    return imgs, K


def leg_batch(a):
    """detect / liop / mldb / msurf through the C ABI of the library at a.lib (plain ctypes: api.Context would load this tree's library)"""
    imgs, _ = _photos(a.images, *a.size)
    B, (h, w) = a.images, a.size
    L = C.CDLL(a.lib)
    ctx = C.c_void_p()
    if L.r3dm_create(0, C.byref(ctx)) != 0:
        raise SystemExit("r3dm_create failed: no gfx950 GPU")
    L.r3dm_last_error.restype = C.c_char_p
    if a.leg in ARM and ARM[a.leg] and L.r3dm_set_descriptor_arm(ctx, ARM[a.leg]) != 0:
        raise SystemExit("r3dm_set_descriptor_arm failed")
    ip = (C.c_void_p * B)(*[im.data_ptr() for im in imgs])
    none = (C.c_char_p * B)()
    n = (C.c_uint32 * B)()
    thr = C.c_float(a.threshold)

    def call():
        if a.leg == "detect":
            rc = L.r3dm_detect_akaze_batch(ctx, C.c_uint32(B), ip, C.c_uint32(w), C.c_uint32(h), thr, None, None, C.c_uint32(0), n)
        else:
            rc = L.r3dm_extract_features_batch(ctx, C.c_uint32(B), ip, None, C.c_uint32(w), C.c_uint32(h), thr, none, none, n)
        if rc != 0:
            raise SystemExit(f"{a.leg}: rc {rc}: {L.r3dm_last_error(ctx).decode()}")

    call()                      # warm-up: work buffers, code objects
    ms, kern, parts, st = [], [], [], api.Stats()
    for _ in range(a.reps):
        t = time.perf_counter(); call(); ms.append((time.perf_counter() - t) * 1e3 / B)
        L.r3dm_get_stats(ctx, C.byref(st)); kern.append(st.ms_liop_kernel)      # the descriptor launch's event time, whichever arm (outside the timed call)
        parts.append((st.ms_detect, st.ms_liop_wall, st.ms_feature_files))      # the call's host phases: detector, keypoints + descriptor pass + rows to the host, delivery
    L.r3dm_destroy.restype = None
    L.r3dm_destroy(ctx)
    print(json.dumps(dict(leg=a.leg, lib=a.tag, images=B, image=[h, w], threshold=a.threshold, keypoints=int(sum(n)),
                          ms_per_image=round(statistics.median(ms), 3), ms_per_image_min=round(min(ms), 3), ms_per_image_max=round(max(ms), 3),
                          ms_descriptor_kernel=None if a.leg == "detect" else round(statistics.median(kern), 3),
                          ms_detect_wall=round(statistics.median(p[0] for p in parts), 3),
                          ms_descriptor_wall=None if a.leg == "detect" else round(statistics.median(p[1] for p in parts), 3),
                          ms_delivery_wall=None if a.leg == "detect" else round(statistics.median(p[2] for p in parts), 3))), flush=True)


def leg_split(a):
    """the M-SURF batch's parts from r3dm_stats, and the launch against what it moves and computes"""
    imgs, _ = _photos(a.images, *a.size)
    ctx = api.Context(0)
    ctx.set_descriptor_arm("MSURF")
    B, (h, w) = a.images, a.size
    ip = (C.c_void_p * B)(*[im.data_ptr() for im in imgs])
    none = (C.c_char_p * B)()
    nf = (C.c_uint32 * B)()
    for rep in range(a.reps + 1):
        t = time.perf_counter()
        rc = ctx._L.r3dm_extract_features_batch(ctx._h, B, ip, None, w, h, a.threshold, none, none, nf)
        ms = (time.perf_counter() - t) * 1e3
        if rc != 0:
            raise SystemExit(f"split: rc {rc}")
        s = ctx.stats()
        nk = int(sum(nf))
        if rep and nk:
            k = s.ms_liop_kernel
            print(json.dumps(dict(leg="split", rep=rep, keypoints=nk, ms_call=round(ms, 2), ms_detect=round(s.ms_detect, 2), ms_detect_kernels=round(s.ms_detect_kernels, 2),
                                  ms_msurf_kernel=round(k, 3), ms_msurf_wall=round(s.ms_liop_wall, 2), ns_per_keypoint=round(k * 1e6 / nk, 1),
                                  gathered_GB_per_s=round(nk * GATHER_BYTES / (k * 1e-3) / 1e9, 1), f64_Gop_per_s=round(nk * F64_OPS / (k * 1e-3) / 1e9, 1))), flush=True)
    ctx.close()


def leg_match(a):
    """r3dm_match_pairs on two views: the M-SURF rows of two photographs as f32[64], and LIOP f32[144] of the SAME keypoints"""
    import numpy as np
    imgs, _ = _photos(2, *a.size)
    ctx = api.Context(0)
    res = ctx.detect_akaze_msurf_batch(imgs, a.threshold)
    liop = [ctx.extract_liop(imgs[k], res[k][0]) for k in range(2)]
    pairs = np.array([[0, 1]], np.uint32)
    for name, rows in (("msurf-64", [r[1] for r in res]), ("liop-144", liop)):
        m = api.Context(0)
        for k in range(2):
            m.set_image(k, np.ascontiguousarray(rows[k], np.float32), res[k][0][:, :2].copy(), a.size[1], a.size[0])
        m.match_pairs(pairs, 0.8, True)                 # warm-up
        ms, kern = [], []
        for _ in range(a.reps):
            t = time.perf_counter(); g = m.match_pairs(pairs, 0.8, True); ms.append((time.perf_counter() - t) * 1e3)
            kern.append(m.stats().ms_match_kernels)
        print(json.dumps(dict(leg="match", rows=name, n=[len(r) for r in rows], dim=int(rows[0].shape[1]), matches=int(g.num_matches),
                              ms_call=round(statistics.median(ms), 3), ms_kernels=round(statistics.median(kern), 3),
                              pairs_per_s=round(1e3 / statistics.median(ms), 1))), flush=True)
        m.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--size", type=int, nargs=2, default=[3000, 4000], metavar=("H", "W"))
    ap.add_argument("--threshold", type=float, default=0.001)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", choices=["detect", "liop", "mldb", "msurf", "split", "match"], default=None, help="(internal) run one leg in this process")
    ap.add_argument("--lib", default=THIS_LIB)
    ap.add_argument("--tag", default="this")
    a = ap.parse_args()
    if a.leg:
        return {"split": leg_split, "match": leg_match}.get(a.leg, leg_batch)(a)
    lines = []

    def child(leg, lib, tag):
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--lib", lib, "--tag", tag, "--images", str(a.images), "--size", str(a.size[0]),
               str(a.size[1]), "--threshold", repr(a.threshold), "--reps", str(a.reps), "--rounds", str(a.rounds)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:            # a leg that failed ends the session: nothing more is started on the device
            raise SystemExit(f"leg {leg} ({tag}) failed with {r.returncode}: {r.stderr[-1500:]}")
        for ln in r.stdout.splitlines():
            if ln.startswith("{"):
                print(ln, flush=True); lines.append(json.loads(ln))

    legs = []
    for leg in ("detect", "liop", "mldb", "msurf"):
        if a.parent_lib and (leg != "msurf" or b"r3dm_detect_akaze_msurf" in open(a.parent_lib, "rb").read()):     # (a parent from before the arm lacks the symbol)
            legs.append((leg, a.parent_lib, "parent"))
        legs.append((leg, THIS_LIB, "this"))
    for _ in range(a.rounds):
        for leg, lib, tag in legs:
            child(leg, lib, tag)
    child("split", THIS_LIB, "this")
    child("match", THIS_LIB, "this")
    summary = {}
    for leg, _, tag in legs:
        v = [ln["ms_per_image"] for ln in lines if ln["leg"] == leg and ln.get("lib") == tag]
        summary[f"{leg}_{tag}"] = dict(median=round(statistics.median(v), 3), min=min(v), max=max(v), rounds=len(v))
        k = [ln["ms_descriptor_kernel"] for ln in lines if ln["leg"] == leg and ln.get("lib") == tag and ln.get("ms_descriptor_kernel") is not None]
        if k:
            summary[f"{leg}_{tag}"]["descriptor_kernel_ms"] = dict(median=round(statistics.median(k), 3), min=min(k), max=max(k))
    tail = json.dumps(dict(summary=summary, unit="ms per image"))
    print(tail, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"# python tools/msurf_arm_perf.py --images {a.images} --size {a.size[0]} {a.size[1]} --threshold {a.threshold!r} --reps {a.reps} "
                    f"--rounds {a.rounds}{' --parent-lib <parent build>' if a.parent_lib else ''}\n")
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
            f.write(tail + "\n")


if __name__ == "__main__":
    main()
