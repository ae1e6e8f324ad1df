"""What every path that the descriptor arms' table, pass and entry serve produces, as one text file of hashes: run once per
library, each in a process of its own, and compare the files byte for byte.
    python tools/descriptor_arms_dump.py --lib PATH/libr3dm.so --out FILE
On fixed synthetic photographs (two of 240 x 320, two of 243 x 325, one of 96 x 128) through plain ctypes, so that it runs unchanged on a
library built from an earlier commit:
    the four describing detect entries (r3dm_detect_akaze_mldb / _mldb_batch / _msurf / _msurf_batch), full and with `cap` below the count;
    r3dm_extract_features_batch, immediate and with deferred files, under each of the three arms, from gray and from 8-bit BGR: every
    .feat and .desc, and what the features sink was handed (the rows read back from the device, the positions);
    the refusal of MLDB and M-SURF under the classic detector, and of an unknown arm id on a context and on a device list: code and text;
    every field of r3dm_stats / r3dm_features_totals that is not a time, after each call.
The file holds no time, path or address."""
import argparse
import ctypes as C
import hashlib
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from regard3d_amd import api, synth        # (the structs of the statistics and the photographs: importing the package loads no library)

THR, CAP, FULL = 0.0005, 5, 8192
SIZES = {(240, 320): (11, 12), (243, 325): (13, 14), (96, 128): (15,)}
ARMS = {"LIOP": (0, 576), "MLDB": (1, 61), "MSURF": (3, 256)}         # literal on purpose: id and row bytes as the ABI has them, whatever the library's tables say
ENTRIES = {"r3dm_detect_akaze_mldb": (False, 61), "r3dm_detect_akaze_mldb_batch": (True, 61),
           "r3dm_detect_akaze_msurf": (False, 256), "r3dm_detect_akaze_msurf_batch": (True, 256)}
SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p)
vp, u32 = C.c_void_p, C.c_uint32


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()[:32]


def photos():
    out = {}
    for (h, w), seeds in SIZES.items():
        gray = [np.ascontiguousarray(synth.make_photo(h, w, seed), np.float32) for seed in seeds]
        bgr = []
        for g in gray:                       # three different channels, so that the conversion's weights matter
            g8 = np.round(g * 255.0).astype(np.uint8)
            bgr.append(np.ascontiguousarray(np.stack([g8, np.roll(g8, 1, axis=1), np.roll(g8, 2, axis=0)], axis=2)))
        out[h, w] = (gray, bgr)
    return out


class Dump:
    def __init__(self, lib):
        self.L = L = C.CDLL(lib)
        L.r3dm_last_error.restype = C.c_char_p; L.r3dm_last_error.argtypes = [vp]
        L.r3dm_multi_last_error.restype = C.c_char_p; L.r3dm_multi_last_error.argtypes = [vp]
        L.r3dm_destroy.restype = None; L.r3dm_destroy.argtypes = [vp]
        L.r3dm_multi_destroy.restype = None; L.r3dm_multi_destroy.argtypes = [vp]
        for e, (batch, _) in ENTRIES.items():
            getattr(L, e).argtypes = [vp, u32, vp, u32, u32, C.c_float, vp, vp, u32, vp] if batch else [vp, vp, u32, u32, C.c_float, vp, vp, u32, vp]
        L.r3dm_extract_features_batch.argtypes = [vp, u32, vp, vp, u32, u32, C.c_float, vp, vp, vp]
        L.r3dm_set_features_sink.argtypes = [vp, SINK, vp]
        L.r3dm_get_stats.argtypes = [vp, C.POINTER(api.Stats)]
        L.r3dm_get_features_totals.argtypes = [vp, C.POINTER(api.FeaturesTotals)]
        for f in ("r3dm_set_descriptor_arm", "r3dm_set_keypoint_detector", "r3dm_set_deferred_feature_files"):
            getattr(L, f).argtypes = [vp, C.c_int]
        L.r3dm_features_files_wait.argtypes = [vp]
        L.r3dm_multi_set_descriptor_arm.argtypes = [vp, C.c_int]
        L.hipMemcpy.argtypes = [vp, vp, C.c_size_t, C.c_int]
        self.lines = []

    def context(self):
        h = vp()
        if self.L.r3dm_create(0, C.byref(h)) != 0:
            raise SystemExit("r3dm_create failed: no gfx950 GPU")
        return h

    def put(self, label, *values):
        self.lines.append(" ".join([label] + [str(v) for v in values]))

    def counters(self, ctx, label):
        s, t = api.Stats(), api.FeaturesTotals()
        assert self.L.r3dm_get_stats(ctx, C.byref(s)) == 0 and self.L.r3dm_get_features_totals(ctx, C.byref(t)) == 0
        for tag, st in (("stats", s), ("totals", t)):
            self.put(f"{label} {tag}", *[f"{k}={getattr(st, k)!r}" for k, _ in st._fields_ if not k.startswith("ms_")])

    def entries(self, ctx, size, gray):
        h, w = size
        for entry, (batch, row_bytes) in ENTRIES.items():
            ims = gray if batch else gray[:1]
            B = len(ims)
            for cap in (FULL, CAP):
                kps = [np.full((cap, 4), np.float32(-7.5)) for _ in range(B)]
                desc = [np.full((cap, row_bytes), 0xA5, np.uint8) for _ in range(B)]
                n = np.full(B, 0xDEADBEEF, np.uint32)
                if batch:
                    rc = getattr(self.L, entry)(ctx, B, (vp * B)(*[im.ctypes.data for im in ims]), w, h, THR, (vp * B)(*[k.ctypes.data for k in kps]),
                                                (vp * B)(*[d.ctypes.data for d in desc]), cap, n.ctypes.data)
                else:
                    rc = getattr(self.L, entry)(ctx, ims[0].ctypes.data, w, h, THR, kps[0].ctypes.data, desc[0].ctypes.data, cap, n.ctypes.data)
                label = f"{entry} {h}x{w} cap={cap}"
                self.put(label, f"rc={rc}", *[f"n={int(x)} kps={sha(k)} desc={sha(d)}" for x, k, d in zip(n, kps, desc)])
                self.counters(ctx, label)

    def features(self, ctx, size, gray, bgr, tmp):
        h, w = size
        B = len(gray)
        seen = {}

        def sink(user, index, n, rows, xy):
            buf = np.zeros(n * row_bytes, np.uint8)
            rc = self.L.hipMemcpy(buf.ctypes.data, rows, buf.size, 2) if n else 0            # 2 = hipMemcpyDeviceToHost
            pos = C.string_at(xy, 8 * n) if n else b""
            seen[int(index)] = (int(n), rc, sha(buf), sha(pos))
            return 0

        fn = SINK(sink)
        assert self.L.r3dm_set_features_sink(ctx, fn, None) == 0
        for arm, (arm_id, row_bytes) in ARMS.items():
            assert self.L.r3dm_set_descriptor_arm(ctx, arm_id) == 0
            for deferred in (0, 1):
                assert self.L.r3dm_set_deferred_feature_files(ctx, deferred) == 0
                for src in ("gray", "bgr"):
                    tag = f"{arm}_{deferred}_{src}_{h}x{w}"
                    fp = [os.path.join(tmp, f"{tag}_{b}.feat").encode() for b in range(B)]
                    dp = [os.path.join(tmp, f"{tag}_{b}.desc").encode() for b in range(B)]
                    n = np.full(B, 0xDEADBEEF, np.uint32)
                    seen.clear()
                    ims = (vp * B)(*[im.ctypes.data for im in (gray if src == "gray" else bgr)])
                    rc = self.L.r3dm_extract_features_batch(ctx, B, ims if src == "gray" else None, ims if src == "bgr" else None, w, h, THR,
                                                            (C.c_char_p * B)(*fp), (C.c_char_p * B)(*dp), n.ctypes.data)
                    wrc = self.L.r3dm_features_files_wait(ctx)
                    label = f"features {tag}"
                    self.put(label, f"rc={rc} wait={wrc}", *[f"n={int(x)}" for x in n])
                    for b in range(B):
                        self.put(f"{label} image {b}", f"feat={sha(open(fp[b], 'rb').read())} desc={sha(open(dp[b], 'rb').read())} desc_bytes={os.path.getsize(dp[b])}",
                                 "sink=" + ",".join(str(v) for v in seen.get(b, ("none",))))
                    self.counters(ctx, label)
        assert self.L.r3dm_set_features_sink(ctx, SINK(), None) == 0
        assert self.L.r3dm_set_deferred_feature_files(ctx, 0) == 0 and self.L.r3dm_set_descriptor_arm(ctx, 0) == 0

    def refusals(self, size, gray):
        h, w = size
        ctx = self.context()
        assert self.L.r3dm_set_keypoint_detector(ctx, 1) == 0                                    # R3DM_DETECTOR_AKAZE, the classic detector
        for arm in ("MLDB", "MSURF"):
            assert self.L.r3dm_set_descriptor_arm(ctx, ARMS[arm][0]) == 0
            n = np.full(1, 0xDEADBEEF, np.uint32)
            none = (C.c_char_p * 1)()
            rc = self.L.r3dm_extract_features_batch(ctx, 1, (vp * 1)(gray[0].ctypes.data), None, w, h, THR, none, none, n.ctypes.data)
            self.put(f"refusal classic {arm}", f"rc={rc} n={int(n[0])}", self.L.r3dm_last_error(ctx).decode())
            self.counters(ctx, f"refusal classic {arm}")
        for arm_id in (2, 4, -1):
            rc = self.L.r3dm_set_descriptor_arm(ctx, arm_id)
            self.put(f"refusal arm {arm_id} context", f"rc={rc}", self.L.r3dm_last_error(ctx).decode())
        self.L.r3dm_destroy(ctx)
        m = vp()
        assert self.L.r3dm_multi_create((C.c_int * 1)(0), 1, C.byref(m)) == 0
        for arm_id in (2, 4, -1, 3, 0):
            rc = self.L.r3dm_multi_set_descriptor_arm(m, arm_id)
            self.put(f"refusal arm {arm_id} device list", f"rc={rc}", (self.L.r3dm_multi_last_error(m) or b"").decode())
        self.L.r3dm_multi_destroy(m)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    d = Dump(a.lib)
    ph = photos()
    tmp = tempfile.mkdtemp(prefix="r3dm_descriptor_arms_dump_")
    try:
        ctx = d.context()
        for size, (gray, bgr) in ph.items():
            d.entries(ctx, size, gray)
            d.features(ctx, size, gray, bgr, tmp)
        d.L.r3dm_destroy(ctx)
        d.refusals((240, 320), ph[240, 320][0])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    text = "\n".join(d.lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(f"{len(d.lines)} lines, {len(text.encode())} bytes -> {a.out}")


if __name__ == "__main__":
    main()
