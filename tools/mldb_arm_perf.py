"""Cost of the features batch per descriptor arm: B same-size photographs resident in HBM through
    detect   r3dm_detect_akaze_batch alone (counts only)
    liop     r3dm_extract_features_batch under R3DM_DESCRIPTOR_LIOP, no files (null paths): detector + patch maps + LIOP + rows to the host
    mldb     the same under R3DM_DESCRIPTOR_MLDB: detector + MLDB items + the one MLDB launch + rows to the host
and the whole stage from pixels (r3dm_stage_run, 3 batches of 8 in flight) on N photographs with and without R3DM_STAGE_DESCRIPTOR_MLDB.
    python tools/mldb_arm_perf.py [--images 8] [--size 3000 4000] [--threshold 0.001] [--reps 5] [--rounds 3]
                                  [--parent-lib PATH] [--stage-images 24] [--out FILE]
Every leg runs in a process of its own (one library per process) and the legs ALTERNATE over --rounds rounds, so that a drift of the
machine shows as spread inside a leg instead of as a difference between legs.  --parent-lib names a libr3dm.so built from the parent
commit: its legs (`mldb` too when that library exports the arm) run between this tree's -- they must not move beyond the spread, which
the summary states (min .. max of the rounds' medians).  A leg's figure is the median of --reps calls after one warm-up call, host clock around calls that end in a
stream synchronise, divided by the images of the batch.  One JSON line per leg and round, then a summary line.  The tool does not time
single kernels: run a leg under `rocprofv3 --kernel-trace --stats` for that split (tools/rocprof_summary.py)."""
import argparse
import ctypes as C
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
THIS_LIB = os.path.join(ROOT, "regard3d_amd", "libr3dm.so")
from regard3d_amd import api        # (the arm ids: importing the package loads no library, so a leg on --parent-lib still holds that one alone)


def _photos(n, h, w):
    import torch
    torch.cuda.init()          # before the library: torch's HIP runtime has to come up first in a process that uses both
    from regard3d_amd import synth
    imgs, K = synth.make_photo_set(n, h, w, seed=7007, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    return imgs, K


def leg_batch(a):
    """detect / liop / mldb through the C ABI of the library at a.lib (plain ctypes: the parent's library lacks the new symbols)"""
    imgs, _ = _photos(a.images, *a.size)
    B, (h, w) = a.images, a.size
    L = C.CDLL(a.lib)
    ctx = C.c_void_p()
    if L.r3dm_create(0, C.byref(ctx)) != 0:
        raise SystemExit("r3dm_create failed: no gfx950 GPU")
    L.r3dm_last_error.restype = C.c_char_p
    if a.leg == "mldb" and L.r3dm_set_descriptor_arm(ctx, api.DESCRIPTOR_ARMS["MLDB"]) != 0:
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
    ms = []
    for _ in range(a.reps):
        t = time.perf_counter(); call(); ms.append((time.perf_counter() - t) * 1e3 / B)
    L.r3dm_destroy.restype = None
    L.r3dm_destroy(ctx)
    print(json.dumps(dict(leg=a.leg, lib=a.tag, images=B, image=[h, w], threshold=a.threshold, keypoints=int(sum(n)),
                          ms_per_image=round(statistics.median(ms), 3), ms_per_image_min=round(min(ms), 3), ms_per_image_max=round(max(ms), 3))), flush=True)


def leg_stage(a):
    N, (h, w) = a.stage_images, a.size
    imgs, K = _photos(N, h, w)
    views = [dict(id=k, width=w, height=h, basename=f"img{k:04d}", gray=imgs[k], focal_px=K[0, 0], ppx=K[0, 2], ppy=K[1, 2]) for k in range(N)]
    d = tempfile.mkdtemp(prefix="r3dm_mldb_stage_")
    st = api.Stage([0])
    try:
        for rep in range(a.rounds + 1):          # the first pass of each arm allocates its work buffers: not reported
            for arm, ratio in (("LIOP", 0.6), ("MLDB", 0.8)):
                for f in os.listdir(d):
                    os.remove(os.path.join(d, f))
                t = time.perf_counter()
                r = st.run(d, views, a.threshold, ratio, 9, True, True, True, 5489, 3, 8, background_nice=True, descriptor=arm)
                ms = (time.perf_counter() - t) * 1e3
                if rep:
                    print(json.dumps(dict(leg="stage", descriptor=arm, reported_arm=int(r.descriptor_arm), images=N, image=[h, w], dist_ratio=ratio,
                                          ms_call=round(ms, 1), ms_features=round(r.ms_features, 1), ms_features_per_image=round(r.ms_features / N, 2),
                                          ms_match=round(r.ms_match, 1), keypoints=int(r.n_keypoints), putative_pairs=int(r.n_putative_pairs),
                                          F_pairs=int(r.n_F_pairs))), flush=True)
    finally:
        st.close()
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--size", type=int, nargs=2, default=[3000, 4000], metavar=("H", "W"))
    ap.add_argument("--threshold", type=float, default=0.001)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--stage-images", type=int, default=24)
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", choices=["detect", "liop", "mldb", "stage"], default=None, help="(internal) run one leg in this process")
    ap.add_argument("--lib", default=THIS_LIB)
    ap.add_argument("--tag", default="this")
    a = ap.parse_args()
    if a.leg:
        return leg_stage(a) if a.leg == "stage" else leg_batch(a)
    lines = []

    def child(leg, lib, tag):
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--lib", lib, "--tag", tag, "--images", str(a.images), "--size", str(a.size[0]),
               str(a.size[1]), "--threshold", repr(a.threshold), "--reps", str(a.reps), "--rounds", str(a.rounds), "--stage-images", str(a.stage_images)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:            # a leg that failed ends the session: nothing more is started on the device
            raise SystemExit(f"leg {leg} ({tag}) failed with {r.returncode}: {r.stderr[-1500:]}")
        for ln in r.stdout.splitlines():
            if ln.startswith("{"):
                print(ln, flush=True); lines.append(json.loads(ln))

    legs = []
    for leg in ("detect", "liop", "mldb"):
        if a.parent_lib and (leg != "mldb" or b"r3dm_detect_akaze_mldb_batch" in open(a.parent_lib, "rb").read()):     # (a parent from before the arm lacks it)
            legs.append((leg, a.parent_lib, "parent"))
        legs.append((leg, THIS_LIB, "this"))
    for _ in range(a.rounds):
        for leg, lib, tag in legs:
            child(leg, lib, tag)
    if a.stage_images > 0:
        child("stage", THIS_LIB, "this")
    summary = {}
    for leg, _, tag in legs:
        v = [ln["ms_per_image"] for ln in lines if ln["leg"] == leg and ln.get("lib") == tag]
        summary[f"{leg}_{tag}"] = dict(median=round(statistics.median(v), 3), min=min(v), max=max(v), rounds=len(v))
    for arm in ("LIOP", "MLDB"):
        v = [ln["ms_call"] for ln in lines if ln["leg"] == "stage" and ln["descriptor"] == arm]
        if v:
            summary[f"stage_{arm}_ms_call"] = dict(median=round(statistics.median(v), 1), min=min(v), max=max(v), rounds=len(v))
    print(json.dumps(dict(summary=summary, unit="ms per image (batch legs), ms per call (stage)")), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"# python tools/mldb_arm_perf.py --images {a.images} --size {a.size[0]} {a.size[1]} --threshold {a.threshold!r} --reps {a.reps} "
                    f"--rounds {a.rounds} --stage-images {a.stage_images}{' --parent-lib <parent build>' if a.parent_lib else ''}\n")
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
            f.write(json.dumps(dict(summary=summary, unit="ms per image (batch legs), ms per call (stage)")) + "\n")


if __name__ == "__main__":
    main()
