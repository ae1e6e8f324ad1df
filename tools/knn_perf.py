"""k-NN kernels against the 2-NN kernel on one pair of 8,192 x 8,192 rows:
    python tools/knn_perf.py [out.txt] [--dev]
Data: D = 128 integer bins as f32 rows and as unsigned char rows (C2-like), D = 128 real-valued, D = 144 LIOP
(tests/golden/liop_match_ref.npz), 64-byte binary rows (C3-like).  Per data set, in one process and one context: the 2-NN tile kernel
(r3dm_match_pairs on the registered pair: the kernel r3dm_knn2 runs, timed by the library's HIP events around it) and r3dm_knn at
k = 3, 4, 8 (HIP events around its first kernel: the nominator / the popcount kernel).  Warm-up calls first, then the median of REPS
with the smallest and largest repetition beside it; the k-kernel's share of the f32 MFMA peak counts the padded tile products
(2 nI nJ Dpad) against 157.3 TFLOP/s; exact = share of the queries answered by the exact scan.

Narrow tiles (r3dm_set_knn_narrow_tiles): for every L2 data set and k the same call with the switch on, ALTERNATED with the switch-off
call in the same loop (off, on, off, on ...), so both see the same clocks and cache state.  The ratio is f32 K-list kernel / narrow
kernel on the medians; "beyond spread" says whether the narrow median lies below the f32 median by more than the f32 line's own
max - min.  --dev: the developer library, plus the integer kernel at one query tile per wave (R3DM_KNN_INT_NJ1) beside the product's.

i8 tiles (r3dm_set_knn_hamming_tiles): binary rows of 32 and of 61 bytes, 8,192 x 8,192, k = 3, 4, 8, the popcount K-list
kernel (switch off) alternated with the i8-tile kernel (switch on) in the same way; "beyond spread" is taken against the popcount line's
max - min.  --hamming-only: these lines alone."""
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
    yield "D=128 integer-valued (SIFT bins), f32 rows", np.ascontiguousarray(sc.descs[0]), np.ascontiguousarray(sc.descs[1]), False
    yield ("D=128 integer-valued (SIFT bins), u8 rows", np.ascontiguousarray(sc.descs[0]).astype(np.uint8),
           np.ascontiguousarray(sc.descs[1]).astype(np.uint8), False)
    yield "D=128 real-valued", rng.standard_normal((N, 128)).astype(np.float32), rng.standard_normal((N, 128)).astype(np.float32), False
    z = np.load(os.path.join(ROOT, "tests", "golden", "liop_match_ref.npz"))
    yield ("D=144 LIOP fixture", (z["hist0"].astype(np.float32) / z["norm0"][:, None]).astype(np.float32),
           (z["hist1"].astype(np.float32) / z["norm1"][:, None]).astype(np.float32), False)
    sk = synth.make_scene(2, N, "akaze", seed=3004)
    yield "binary, 486 bits in 64 bytes (A-KAZE MLDB)", np.ascontiguousarray(sk.descs[0]), np.ascontiguousarray(sk.descs[1]), True


def binary_datasets():
    """random rows; half of the queries are 5 %-flipped copies of dataset rows, so that true neighbours exist as in a matching pair"""
    for nbytes in (32, 61):
        rng = np.random.default_rng([8192, nbytes])
        a = rng.integers(0, 256, (N, nbytes), dtype=np.uint8); b = rng.integers(0, 256, (N, nbytes), dtype=np.uint8)
        b[:N // 2] = a[rng.permutation(N)[:N // 2]] ^ np.packbits(rng.random((N // 2, nbytes * 8)) < 0.05, axis=1)
        yield f"binary, {nbytes} bytes ({(nbytes + 3) // 4} words)", a, b


def hamming_tiles(c):
    out = ["data | k | popcount K-list ms [min .. max] | i8 tiles ms [min .. max] | popcount / i8 | beyond the popcount spread"]
    for name, a, b in binary_datasets():
        for k in (3, 4, 8):
            def kn(on):
                c.set_knn_hamming_tiles(on)
                try:
                    c.knn(a, b, k, binary=True)
                finally:
                    c.set_knn_hamming_tiles(False)
                s = c.stats()
                assert s.n_knn_hamming_tiles == int(on) and s.n_exact_fallback == 0
                return s.ms_match_kernels
            (tp, lo, hi), (tn, nlo, nhi) = alternated([lambda: kn(False), lambda: kn(True)])
            beyond = "yes" if tp - tn > hi - lo else "NO"
            out.append(f"{name} | {k} | {tp:.3f} [{lo:.3f} .. {hi:.3f}] | {tn:.3f} [{nlo:.3f} .. {nhi:.3f}] | {tp / tn:.2f} | {beyond}")
    return out


def median_of(fn):
    for _ in range(WARM):
        fn()
    return float(np.median([fn() for _ in range(REPS)]))


def alternated(fns):
    """every function WARM times, then REPS rounds of (f0, f1, ...): -> per function (median, min, max)"""
    for _ in range(WARM):
        for f in fns:
            f()
    t = [[] for _ in fns]
    for _ in range(REPS):
        for i, f in enumerate(fns):
            t[i].append(f())
    return [(float(np.median(x)), float(min(x)), float(max(x))) for x in t]


def main():
    args = [x for x in sys.argv[1:] if not x.startswith("--")]
    dev = "--dev" in sys.argv
    if dev:
        api.use_developer_library()
    c = api.Context(0)
    lines = ["data | call | kernel ms (median of %d) [min .. max] | vs 2-NN | share of f32 MFMA peak | exact-scan share" % REPS]
    narrow = ["data | k | tiles | f32 K-list ms [min .. max] | narrow ms [min .. max] | f32 / narrow | beyond the f32 spread | exact-scan share f32 / narrow"]
    for name, a, b, binary in (() if "--hamming-only" in sys.argv else datasets()):
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
            def kn(on=False, nj1=False, tag="off"):
                if dev:
                    os.environ["R3DM_KNN_INT_NJ1"] = "1" if nj1 else "0"
                c.set_knn_narrow_tiles(on)
                try:
                    c.knn(a, b, k, binary=binary)
                finally:
                    c.set_knn_narrow_tiles(False)
                s = c.stats()
                state[tag] = (s.n_exact_fallback / b.shape[0], "bf16" if s.n_knn_integer_tiles else "split f16" if s.n_knn_split_tiles else "f32")
                return s.ms_match_kernels
            fns = [lambda: kn(False, False, "off")]
            if not binary:
                fns.append(lambda: kn(True, False, "on"))
                if dev and not (np.asarray(a, np.float32) != np.rint(a)).any():      # integer rows: the bf16 kernel's A/B
                    fns.append(lambda: kn(True, True, "on1"))
            res = alternated(fns)
            tk, lo, hi = res[0]
            lines.append(f"{name} | r3dm_knn k = {k} | {tk:.3f} [{lo:.3f} .. {hi:.3f}] | {tk / t2:.2f} | {share(tk)} | {state['off'][0]:.4f}")
            for (tn, nlo, nhi), tag in zip(res[1:], ("on", "on1")):
                tiles = state[tag][1] + (", one query tile per wave" if tag == "on1" else "")
                beyond = "yes" if tk - tn > hi - lo else "NO"
                narrow.append(f"{name} | {k} | {tiles} | {tk:.3f} [{lo:.3f} .. {hi:.3f}] | {tn:.3f} [{nlo:.3f} .. {nhi:.3f}] | {tk / tn:.2f} | {beyond} | "
                              f"{state['off'][0]:.4f} / {state[tag][0]:.4f}")
    ham = hamming_tiles(c)
    c.close()
    text = "\n".join(["i8 tiles (r3dm_set_knn_hamming_tiles), alternated with the popcount K-list kernel in one loop"] + ham)
    if "--hamming-only" not in sys.argv:
        text = "\n".join(lines + ["", "narrow tiles (r3dm_set_knn_narrow_tiles), alternated with the f32 K-list kernel in one loop"] + narrow + ["", text])
    print(text)
    if args:
        with open(args[0], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
