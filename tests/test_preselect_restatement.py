"""The restatement of preemptive matching (preselect_restatement.py: heads by a stable argsort, counts through
pyoracle.match_distance_ratio) against a brute-force loop that shares no code with it, on the cases where the two could part: ties in
priority (the h-th and the (h + 1)-th equal), n < h, n == h, n == 1, binary rows, a 37-element scalar tail.  And the .feat reader of the
facade keeps the scale column as written (a small C++ host on regard3d_amd/csrc/feat_text.hpp).  No GPU."""
import os
import struct
import subprocess

import numpy as np
import pytest

import preselect_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n,h", [(1, 2), (2, 2), (5, 8), (8, 8), (9, 8), (40, 8), (40, 33), (300, 256), (257, 256)])
def test_head_rows_against_sorted(n, h):
    rng = np.random.default_rng(n * 1000 + h)
    for p in (None, rng.integers(0, 4, n).astype(np.float32), rng.random(n).astype(np.float32), np.zeros(n, np.float32)):
        got = R.head_rows(p, n, h)
        assert got.tolist() == R.brute_force_head(p, n, h)
        assert len(got) == min(n, h) and np.all(np.diff(got) > 0)


def test_head_tie_at_the_cut_keeps_the_lower_row():
    p = np.array([1, 3, 2, 2, 2, 0], np.float32)            # h = 3: row 1, then rows 2 and 3 of the three equal ones
    assert R.head_rows(p, 6, 3).tolist() == [1, 2, 3] == R.brute_force_head(p, 6, 3)
    assert R.head_rows(p, 6, 2).tolist() == [1, 2]
    z = np.array([0.0, -0.0, 0.0, -0.0], np.float32)        # -0.0 is +0.0: all equal, the first rows
    assert R.head_rows(z, 4, 2).tolist() == [0, 1] == R.brute_force_head(z, 4, 2)


@pytest.mark.parametrize("dim,dtype,nbytes", [(64, np.float32, None), (37, np.float32, None), (128, np.uint8, None), (0, np.uint8, 32), (0, np.uint8, 61)])
@pytest.mark.parametrize("h", [2, 8, 40])
def test_counts_against_the_brute_force_loop(oracle, dim, dtype, nbytes, h):
    rows = (1, 2, 8, 9, 40, 41, 12)
    descs, prios = R.related_views(rows, dim, 7 + dim + (nbytes or 0), dtype, nbytes)
    prios[3] = None                                          # a view without priority
    binary = nbytes is not None
    ratio, squared = (0.8, False) if binary else (0.6, True)
    pairs = [(i, j) for i in range(len(rows)) for j in range(len(rows)) if i != j]
    got = R.collection_counts(oracle, descs, prios, pairs, h, ratio, squared, binary)
    want = [R.brute_force_count(descs[i], descs[j], prios[i], prios[j], h, ratio, squared, binary) for i, j in pairs]
    print(f"dim {dim} nbytes {nbytes} h {h}: counts {sorted(set(want))}")
    assert got.tolist() == want
    assert max(want) > 0 and min(want) == 0
    for (i, j), c in zip(pairs, want):
        if rows[i] < 2:
            assert c == 0                                    # a head of I with fewer than two rows
    counts, keep = R.gate_collection(oracle, descs, prios, pairs, h, 2, ratio, squared, binary)
    assert keep.tolist() == [c >= 2 for c in want]


def test_restrict_graph():
    pairs = np.array([[0, 1], [0, 2], [1, 2]], np.uint32)
    offsets = np.array([0, 2, 2, 5], np.uint64)
    matches = np.arange(10, dtype=np.uint32).reshape(5, 2)
    p, c, m = R.restrict_graph(pairs, offsets, matches, [(1, 2), (0, 2)])
    assert p.tolist() == [[0, 2], [1, 2]] and c.tolist() == [0, 3] and np.array_equal(m, matches[2:])


def test_feat_scale_column_is_parsed_as_written(tmp_path):
    exe = str(tmp_path / "feat_scale_test")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", "feat_scale_test.cpp")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    rows = [("1.5", "2.25", "3", "0.5"), ("100.125", "7", "0.1", "-1"), ("0", "0", "12.3456789", "359.9"), ("4e2", "3", "1e-3", "0"),
            ("7", "8", "0", "90"), ("9", "10", "2.4000001", "45")]
    f = tmp_path / "v.feat"
    f.write_text("".join(" ".join(r_) + "\n" for r_ in rows) + "11 12 13\n")          # an incomplete last group ends the file
    r = subprocess.run([exe, str(f)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    assert int(lines[0]) == len(rows)
    bits = lambda s: struct.unpack("<I", struct.pack("<f", float(np.float32(s))))[0]
    for row, line in zip(rows, lines[1:]):
        assert [int(x, 16) for x in line.split()] == [bits(row[0]), bits(row[1]), bits(row[2])], row


def test_symbols_and_structures_are_declared():
    """the four entries, the two multi forms, the layout bit and the stage flag, in the header as in api.py"""
    import re
    from regard3d_amd import api
    L = api.load_library()
    for name in ("r3dm_set_view_priority", "r3dm_preselect_pairs", "r3dm_set_preemptive_matching", "r3dm_preselect_report",
                 "r3dm_multi_set_view_priority", "r3dm_multi_set_preemptive_matching"):
        assert name in api.EXPORTS and hasattr(L, name), name
    assert L.r3dm_set_preemptive_matching(None, 1, 128, 4) != 0 and L.r3dm_preselect_report(None, None) != 0
    hdr = open(os.path.join(ROOT, "include", "r3dm.h")).read()
    body = hdr[:hdr.index("} r3dm_preselect_stats;")]
    body = re.sub(r"/\*.*?\*/", "", body[body.rindex("typedef struct"):], flags=re.S)
    assert re.findall(r"\b(?:uint64_t|double)\s+(\w+)\s*;", body) == [f[0] for f in api.PreselectStats._fields_]
    assert "#define R3DM_LAYOUT_HEAD   32u" in hdr and api.LAYOUT_HEAD == 32
    fac = open(os.path.join(ROOT, "include", "r3d_compute_matches.hpp")).read()
    assert "#define R3DM_STAGE_PREEMPTIVE_MATCHING 256u" in fac and api.STAGE_PREEMPTIVE_MATCHING == 256
    for m in ("set_view_priority", "preselect_pairs", "set_preemptive_matching", "preselect_report"):
        assert hasattr(api.Context, m)
    assert hasattr(api.MultiContext, "set_view_priority") and hasattr(api.MultiContext, "set_preemptive_matching")
