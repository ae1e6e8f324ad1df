"""The contract of the four describing detect entries -- r3dm_detect_akaze_mldb, _mldb_batch, _msurf, _msurf_batch -- at their edges, held
by every entry in the same words (the entries are one function over the descriptor arm's row): `-m gpu`.

* `cap` > 0 with descriptors_out null, or (batch forms) one image's descriptors_out[b] / keypoints_out[b] null: R3DM_ERR_INVALID, n_out
  keeps what it held, no output byte is written;
* `cap` == 0 with null outputs: R3DM_OK and n_out is the count -- r3dm_detect_akaze_batch's for the MLDB entries (same level table), the
  count of a full call for the M-SURF entries (their own level table);
* `cap` below the count: exactly `cap` keypoints and rows, equal to the first `cap` of a full call, the bytes behind them untouched, n_out
  the full count;
* after a refused call the next valid call on the same context returns what a fresh context returns.

Images of 96 x 128 and 160 x 192 (tests/msurf_cases.py KERNEL_SIZES): the smallest on which the M-SURF level table has a level and on
which the two tables differ.  What the entries return is compared with what the entries return; the values themselves are held to the
reference chains by test_gpu_mldb_arm.py and test_gpu_msurf_arm.py."""
import ctypes as C

import numpy as np
import pytest

import mldb_arm_cases as M
from regard3d_amd import api

pytestmark = pytest.mark.gpu
R3DM_OK, R3DM_ERR_INVALID = 0, -1
SIZES = [(96, 128), (160, 192)]
THR = 0.0001
CAP, ROOM, FULL = 3, 4, 4096
SENTINEL_N = 0xDEADBEEF
# entry -> (batch form, numpy dtype of a row, its length)
ENTRIES = {"r3dm_detect_akaze_mldb": (False, np.uint8, 61), "r3dm_detect_akaze_mldb_batch": (True, np.uint8, 61),
           "r3dm_detect_akaze_msurf": (False, np.float32, 64), "r3dm_detect_akaze_msurf_batch": (True, np.float32, 64)}
KP_FILL, ROW_FILL = np.float32(-7.5), {np.uint8: np.uint8(0xA5), np.float32: np.float32(-3.25)}


# two scenes per size; on the reference chains they hold 15, 14 / 31, 36 keypoints under the M-SURF table and 22, 23 / 42, 48 under the detector's
SEEDS = {(96, 128): (305, 308), (160, 192): (191, 217)}
_IMAGES = {}


def _images(size):
    if size not in _IMAGES:
        _IMAGES[size] = [M.scene(size[0], size[1], seed, 40) for seed in SEEDS[size]]
    return _IMAGES[size]


class Call:
    """one call of an entry on the context `c`: `rows` rows of room per image, filled with sentinels; null: which outputs are passed as null
    ("desc": descriptors_out itself, ("desc", b) / ("kps", b): image b's entry of the batch forms' arrays, "all": every output)"""

    def __init__(self, c, entry, ims, cap, rows, null=None):
        batch, dtype, dim = ENTRIES[entry]
        ims = [np.ascontiguousarray(im, np.float32) for im in (ims if batch else ims[:1])]
        B = len(ims); h, w = ims[0].shape
        self.kps = [np.full((rows, 4), KP_FILL) for _ in range(B)]
        self.desc = [np.full((rows, dim), ROW_FILL[dtype]) for _ in range(B)]
        self.n = np.full(B, SENTINEL_N, np.uint32)
        kp = [k.ctypes.data for k in self.kps]; dp = [d.ctypes.data for d in self.desc]
        if isinstance(null, tuple):
            (dp if null[0] == "desc" else kp)[null[1]] = None
        L = c._L
        if batch:
            kp_p = None if null == "all" else (C.c_void_p * B)(*kp)
            dp_p = None if null in ("all", "desc") else (C.c_void_p * B)(*dp)
            ip = (C.c_void_p * B)(*[im.ctypes.data for im in ims])
            self.rc = getattr(L, entry)(c._h, B, ip, w, h, THR, kp_p, dp_p, cap, self.n.ctypes.data)
        else:
            self.rc = getattr(L, entry)(c._h, ims[0].ctypes.data, w, h, THR, None if null == "all" else kp[0], None if null in ("all", "desc") else dp[0], cap,
                                        self.n.ctypes.data_as(C.POINTER(C.c_uint32)))

    def untouched(self, from_row=0):
        return all((k[from_row:] == KP_FILL).all() for k in self.kps) and all((d[from_row:] == d.dtype.type(ROW_FILL[d.dtype.type])).all() for d in self.desc)

    def result(self):
        return [(int(n), k[:min(int(n), len(k))].tobytes(), d[:min(int(n), len(d))].tobytes()) for n, k, d in zip(self.n, self.kps, self.desc)]


@pytest.fixture(scope="module")
def full(ctx):
    """(entry, size) -> the full call's result per image, on the session's context: computed once, never changed"""
    out = {}
    for size in SIZES:
        for entry in ENTRIES:
            r = Call(ctx, entry, _images(size), FULL, FULL)
            assert r.rc == R3DM_OK, (entry, size, r.rc)
            out[entry, size] = r.result()
    return out


CASES = [(e, s) for e in ENTRIES for s in SIZES]


@pytest.mark.parametrize("entry,size", CASES)
def test_the_images_keep_their_purpose(full, entry, size):
    """more keypoints than `cap` on every image, fewer than the full call's room; and the two level tables differ at these sizes"""
    for n, _, _ in full[entry, size]:
        assert CAP < n < FULL, (entry, size, n)
    other = entry.replace("msurf", "mldb") if "msurf" in entry else entry.replace("mldb", "msurf")
    assert [r[0] for r in full[entry, size]] != [r[0] for r in full[other, size]]


@pytest.mark.parametrize("entry,size", CASES)
def test_cap_without_descriptors_out_is_refused_and_writes_nothing(ctx, entry, size):
    r = Call(ctx, entry, _images(size), CAP, CAP + ROOM, null="desc")
    assert r.rc == R3DM_ERR_INVALID and (r.n == SENTINEL_N).all() and r.untouched()


@pytest.mark.parametrize("which", ["desc", "kps"])
@pytest.mark.parametrize("entry,size", [(e, s) for e, s in CASES if ENTRIES[e][0]])
def test_batch_with_one_null_output_entry_is_refused_the_same_way(ctx, entry, size, which):
    for b in (0, 1):
        r = Call(ctx, entry, _images(size), CAP, CAP + ROOM, null=(which, b))
        assert r.rc == R3DM_ERR_INVALID and (r.n == SENTINEL_N).all() and r.untouched(), (which, b)


@pytest.mark.parametrize("entry,size", CASES)
def test_cap_zero_with_null_outputs_reports_the_count(ctx, full, entry, size):
    r = Call(ctx, entry, _images(size), 0, 1, null="all")
    assert r.rc == R3DM_OK and r.untouched()
    assert [int(n) for n in r.n] == [f[0] for f in full[entry, size]]
    if "mldb" in entry:                      # the MLDB entries detect on the detector's own level table
        ims = _images(size)[:len(r.n)]
        assert [int(n) for n in r.n] == [len(k) for k, _ in ctx.detect_akaze_batch(ims, THR, FULL)]


@pytest.mark.parametrize("entry,size", CASES)
def test_cap_below_the_count_writes_exactly_cap_rows(ctx, full, entry, size):
    r = Call(ctx, entry, _images(size), CAP, CAP + ROOM)
    assert r.rc == R3DM_OK and r.untouched(from_row=CAP)
    _, dtype, dim = ENTRIES[entry]
    kp_bytes, row_bytes = 16 * CAP, CAP * dim * np.dtype(dtype).itemsize
    for (n, k, d), kps, desc, nb in zip(full[entry, size], r.kps, r.desc, r.n):
        assert int(nb) == n
        assert kps[:CAP].tobytes() == k[:kp_bytes] and desc[:CAP].tobytes() == d[:row_bytes]


@pytest.mark.parametrize("entry,size", CASES)
def test_a_refused_call_leaves_the_context_as_a_fresh_one(full, entry, size):
    fresh = api.Context(0)
    try:
        a = Call(fresh, entry, _images(size), FULL, FULL)
        assert a.rc == R3DM_OK and a.result() == full[entry, size]
    finally:
        fresh.close()
    used = api.Context(0)
    try:
        assert Call(used, entry, _images(size), CAP, CAP + ROOM, null="desc").rc == R3DM_ERR_INVALID
        b = Call(used, entry, _images(size), FULL, FULL)
        assert b.rc == R3DM_OK and b.result() == full[entry, size]
    finally:
        used.close()
