"""k-NN kernels against the 2-NN kernel on one pair of 8,192 x 8,192 rows:
    python tools/knn_perf.py [out.txt]
Data: D = 128 integer bins (C2-like), D = 128 real-valued, D = 144 LIOP (tests/golden/liop_match_ref.npz), 64-byte binary rows
(C3-like).  Per data set, in one process and one context: the 2-NN tile kernel (r3dm_match_pairs on the registered pair: the kernel
r3dm_knn2 runs, timed by the library's HIP events around it) and r3dm_knn at k = 3, 4, 8 (HIP events around its first kernel: the
nominator / the popcount kernel).  Warm-up calls first, then the median of REPS; the k-kernel's share of the f32 MFMA peak counts the
padded tile products (2 nI nJ Dpad) against 157.3 TFLOP/s; exact = share of the queries answered by the exact scan."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from regard3d_amd import api, synth

REPS, WARM = 7, 2
PEAK_F32_MFMA = 157.3e12
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 8192


def datasets():
    rng = np.random.default_rng(8192)
    sc = synth.make_scene(2, N, "sift", seed=3003)
    yield "D=128 integer-valued (SIFT bins)", np.ascontiguousarray(sc.descs[0]), np.ascontiguousarray(sc.descs[1]), False
    yield "D=128 real-valued", rng.standard_normal((N, 128)).astype(np.float32), rng.standard_normal((N, 128)).astype(np.float32), False
    z = np.load(os.path.join(ROOT, "tests", "golden", "liop_match_ref.npz"))
    yield ("D=144 LIOP fixture", (z["hist0"].astype(np.float32) / z["norm0"][:, None]).astype(np.float32),
           (z["hist1"].astype(np.float32) / z["norm1"][:, None]).astype(np.float32), False)
    sk = synth.make_scene(2, N, "akaze", seed=3004)
    yield "binary, 486 bits in 64 bytes (A-KAZE MLDB)", np.ascontiguousarray(sk.descs[0]), np.ascontiguousarray(sk.descs[1]), True


def median_of(fn):
    for _ in range(WARM):
        fn()
    return float(np.median([fn() for _ in range(REPS)]))


def main():
    c = api.Context(0)
    lines = ["data | call | kernel ms (median of %d) | vs 2-NN | share of f32 MFMA peak | exact-scan share" % REPS]
    for name, a, b, binary in datasets():
        c.clear_images()
        c.set_image(0, a, None, 4000, 3000, binary=binary); c.set_image(1, b, None, 4000, 3000, binary=binary)
        pair = np.array([[0, 1]], np.uint32)
        ratio, sq = (0.8, False) if binary else (0.6, True)
        state = {}

        def two():
            c.match_pairs(pair, ratio, sq); s = c.stats(); state["fb"] = s.n_exact_fallback / b.shape[0]; return s.ms_match_kernels
        t2 = median_of(two)
        dpad = 0 if binary else {128: 128, 144: 144}[a.shape[1]]
        share = lambda ms: "-" if binary else "%.1f %%" % (100.0 * 2.0 * a.shape[0] * b.shape[0] * dpad / (ms * 1e-3) / PEAK_F32_MFMA)
        lines.append(f"{name} | 2-NN tile kernel (r3dm_match_pairs) | {t2:.3f} | 1.00 | {share(t2)} | {state['fb']:.4f}")
        for k in (3, 4, 8):
            def kn():
                c.knn(a, b, k, binary=binary); s = c.stats(); state["fb"] = s.n_exact_fallback / b.shape[0]; return s.ms_match_kernels
            tk = median_of(kn)
            lines.append(f"{name} | r3dm_knn k = {k} | {tk:.3f} | {tk / t2:.2f} | {share(tk)} | {state['fb']:.4f}")
    c.close()
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
