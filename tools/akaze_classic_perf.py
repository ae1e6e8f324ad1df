"""Classic A-KAZE probe (r3dm_detect_akaze_classic_batch, Regard3D's "AKAZE" arm) on synthetic 4000 x 3000 images resident in HBM:
wall and kernel ms per image at B = 1 and B = 8 and thresholds 0.001 and 0.0001, beside the Fast arm (r3dm_detect_akaze_batch) on the same images.  The kernel time is
the span from the first scale-space launch to the end of the orientation pass; the wall time adds the buffer allocation and the two
host visits (candidate count, results)."""
import sys, os, time, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
torch.cuda.init()          # before the library: torch's HIP runtime has to come up first in a process that uses both
from regard3d_amd import api, synth

h, w = 3000, 4000
imgs = [synth.make_photo(h, w, seed=100 + k) for k in range(8)]
dimgs = [torch.from_numpy(im).cuda() for im in imgs]
torch.cuda.synchronize()
c = api.Context(0)
for thr, B in [(t, int(x)) for t in (0.001, 0.0001) for x in os.environ.get("AK_BATCHES", "1,8").split(",")]:
    for arm, fn in (("AKAZE", c.detect_akaze_classic_batch), ("Fast-AKAZE", c.detect_akaze_batch)):
        for rep in range(3):
            t = time.time(); res = fn(dimgs[:B], thr); dt = time.time() - t
        s = c.stats()
        print(json.dumps(dict(arm=arm, image=[h, w], threshold=thr, batch=B, keypoints=[len(r[0]) for r in res],
                              ms_wall_per_image=round(dt / B * 1e3, 3), ms_kernels_per_image=round(s.ms_detect_kernels / B, 3))), flush=True)
