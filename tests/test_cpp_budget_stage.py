"""The match budget through the stage (include/r3d_compute_matches.hpp) from a small host program (tests/cpp/budget_stage_main.cpp) over
a directory of .feat / .desc files: the stage flag R3DM_STAGE_MATCH_BUDGET against R3DComputeMatches::setMatchBudget(true, 8192) and
against the flag-off files, and setMatchBudget at a small budget against the restatement.  The scale column of the .feat files is
every view's priority.  The program's compile-and-link part runs without a GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import budget_restatement as B
from regard3d_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIM = 64
ROWS = (8300, 8250, 300)                                             # two views above the flag's 8,192 rows, one whole


@pytest.fixture(scope="module")
def budget_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp_budget_stage") / "budget_stage_main")
    lib = os.path.join(ROOT, "regard3d_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fopenmp", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "budget_stage_main.cpp"), "-o", out, "-L" + lib, "-lr3dm", "-Wl,-rpath," + lib])
    return out


def test_budget_stage_program_compiles_and_links(budget_exe):
    assert subprocess.run([budget_exe], capture_output=True).returncode == 2           # usage; the program loaded libr3dm.so


def _views():
    rng = np.random.default_rng(51)
    n = max(ROWS)
    dI = rng.integers(0, 121, (n, DIM)).astype(np.float32)
    dJ = np.clip(dI + rng.integers(-2, 3, (n, DIM)).astype(np.float32), 0, 255).astype(np.float32)
    scale = (rng.integers(0, 8, n).astype(np.float32) * np.float32(0.75) + np.float32(0.5)).astype(np.float32)
    scale[:200] = np.float32(0.25)                                   # the first rows rank last: S is not a prefix
    descs = [np.ascontiguousarray((dI if k % 2 == 0 else dJ)[:m]) for k, m in enumerate(ROWS)]
    prios = [np.ascontiguousarray(scale[:m]) for m in ROWS]
    xys = [np.stack([np.arange(m) * 0.5 + k, np.arange(m) * 0.25 + 5.0], 1).astype(np.float32) for k, m in enumerate(ROWS)]
    return descs, xys, prios


def _write(oracle, d, descs, xys, prios):
    for k, desc in enumerate(descs):
        name = f"img{k:03d}"
        assert oracle.lib().orc_save_desc(str(d / (name + ".desc")).encode(), ctypes.c_uint64(desc.shape[0]), ctypes.c_size_t(DIM * 4),
                                          desc.ctypes.data_as(ctypes.c_void_p)) == 0
        with open(d / (name + ".feat"), "w") as f:                   # full-precision text so positions and scales round-trip exactly
            for (x, y), s in zip(xys[k], prios[k]):
                f.write("%.9g %.9g %.9g 0\n" % (x, y, s))


def _run(exe, d, mode, max_rows):
    r = subprocess.run([exe, str(d), mode, str(max_rows), str(DIM), str(len(ROWS))], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return int(r.stdout.split()[0])


@pytest.mark.gpu
def test_stage_flag_against_set_match_budget_and_the_flag_off_files(oracle, budget_exe, ctx, tmp_path):
    descs, xys, prios = _views()
    pairs = np.array([(0, 1), (0, 2), (1, 2)], np.uint32)
    files = {}
    for mode, max_rows in (("off", 0), ("flag", 0), ("set", 8192), ("set", 50)):
        d = tmp_path / f"{mode}{max_rows}"
        d.mkdir()
        _write(oracle, d, descs, xys, prios)
        n_put = _run(budget_exe, d, mode, max_rows)
        files[(mode, max_rows)] = oracle.load_matches(os.path.join(str(d), "matches.putative.txt"))
        assert n_put == len(files[(mode, max_rows)][0])
    flag, setb, off, small = files[("flag", 0)], files[("set", 8192)], files[("off", 0)], files[("set", 50)]
    assert all(np.array_equal(a, b) for a, b in zip(flag, setb))
    # the library's own graphs of the same views: whole, and under the budget of 8,192 rows
    ctx.clear_images()
    try:
        for v, d in enumerate(descs):
            ctx.set_image(v, d, xys[v], 4000, 3000)
            ctx.set_view_priority(v, prios[v])
        g = ctx.match_pairs(pairs, 0.8, True)
        assert np.array_equal(off[0], g.pairs) and np.array_equal(off[2], g.matches)
        ctx.set_match_budget(True, 8192)
        gb = ctx.match_pairs(pairs, 0.8, True)
        assert np.array_equal(flag[0], gb.pairs) and np.array_equal(flag[1], np.diff(gb.offsets.astype(np.int64))) and np.array_equal(flag[2], gb.matches)
        assert ctx.budget_report()["n_views_budgeted"] == 2 and ctx.budget_report()["n_views_whole"] == 1
    finally:
        ctx.set_match_budget(False)
        ctx.clear_images()
    assert flag[2].tobytes() != off[2].tobytes()                     # the flag changes the file ...
    rows = [set(B.selected_rows(prios[v], ROWS[v], 8192).tolist()) for v in range(3)]
    o = 0
    for (I, J), c in zip(flag[0], flag[1]):                          # ... and every match lies inside the selected rows
        m = flag[2][o:o + int(c)]; o += int(c)
        assert set(m[:, 0].tolist()) <= rows[int(I)] and set(m[:, 1].tolist()) <= rows[int(J)]
    # a small budget through setMatchBudget against the restatement
    counts, mapped, sub = B.match_collection(oracle, descs, xys, prios, pairs, 50, 0.8, True)
    assert len(mapped) and (mapped != sub).any()
    assert np.array_equal(small[0], pairs[counts > 0]) and np.array_equal(small[1], counts[counts > 0]) and np.array_equal(small[2], mapped)
