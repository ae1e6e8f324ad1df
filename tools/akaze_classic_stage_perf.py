"""The stage leg's photographs through both detector arms: R3DComputeMatches::computeMatches from pixels (r3dm_stage_run) with
{"Fast-AKAZE"} and with {"AKAZE"} (R3DM_STAGE_DETECTOR_AKAZE) on N synthetic 4000 x 3000 photographs resident in HBM (bench --config
stage's set, seed 7007), 3 batches of 8 in flight.  Reports per arm the whole call and the features phase in ms (per image too), the
keypoint count, then the classic arm's component-size histogram over the same photographs (r3dm_akaze_classic_components of one
context: bin k = components of 2^k .. 2^(k+1) - 1 candidates of the kpts_aux walk)."""
import sys, os, time, json, shutil, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
torch.cuda.init()          # before the library: torch's HIP runtime has to come up first in a process that uses both
from regard3d_amd import api, synth

N = int(os.environ.get("AK_STAGE_IMAGES", "24"))
H, W = 3000, 4000
imgs, K = synth.make_photo_set(N, H, W, seed=7007, device=torch.device("cuda", 0))
torch.cuda.synchronize()
views = [dict(id=k, width=W, height=H, basename=f"img{k:04d}", gray=imgs[k], focal_px=K[0, 0], ppx=K[0, 2], ppy=K[1, 2]) for k in range(N)]
d = tempfile.mkdtemp(prefix="r3dm_ac_stage_")
st = api.Stage([0])
try:
    for rep in range(2):                     # the first pass of each arm allocates its work buffers: report the second
        for arm in ("Fast-AKAZE", "AKAZE"):
            for f in os.listdir(d):
                os.remove(os.path.join(d, f))
            torch.cuda.synchronize()
            t = time.perf_counter()
            r = st.run(d, views, 0.001, 0.6, 9, True, True, True, 5489, 3, 8, background_nice=True, detector=arm)
            ms = (time.perf_counter() - t) * 1e3
            if rep == 1:
                print(json.dumps(dict(arm=arm, images=N, image=[H, W], ms_call=round(ms, 1), ms_features=round(r.ms_features, 1),
                                      ms_features_per_image=round(r.ms_features / N, 2), ms_detect_kernels=round(r.features.ms_detect_kernels, 1),
                                      keypoints=int(r.n_keypoints), putative_pairs=int(r.n_putative_pairs), F_pairs=int(r.n_F_pairs))), flush=True)
finally:
    st.close()
    shutil.rmtree(d, ignore_errors=True)
c = api.Context(0)
for thr in (0.001, 0.0001):
    h0 = c.akaze_classic_components().astype(np.int64)
    for b0 in range(0, N, 8):
        c.detect_akaze_classic_batch(imgs[b0:b0 + 8], thr)
    hist = c.akaze_classic_components().astype(np.int64) - h0
    top = int(np.flatnonzero(hist)[-1]) if hist.any() else 0
    print(json.dumps(dict(arm="AKAZE", threshold=thr, images=N, component_size_histogram={f"{1 << k}-{(2 << k) - 1}": int(hist[k]) for k in range(top + 1)})), flush=True)
c.close()
