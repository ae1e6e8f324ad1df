"""No result depends on what a context computed before (`-m gpu`).

The buffers of a context grow and never shrink (DevBuf::ensure), the arena hands a freed view block to a view as small as 0.8 of it
(DevArena::alloc), every zero fill is written by hand and sized by the current call, d_cnt / coop_sched / liop_cnt are shared between
operations, and the context pool leases the same contexts for the life of the host process: history is the normal case.  The other
GPU tests run on memory that has held little else.  These run the case table of tests/history_cases.py in schedules that leave
valid-looking leftovers of LARGER calls everywhere, and compare every output, bytes for bytes, with its expected value: the CPU
restatement where one is bit-equal, the same call on a fresh context in a child process where none is (history_cases says which).

Nothing here writes patterns into device memory: the leftovers are outputs of valid larger calls, so a wrongly read index still
points inside a buffer the large call sized.  Every test opens its own api.Context(0) and closes it.
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import history_cases as HC
from regard3d_amd import api, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WALK_SEEDS = (20261, 20262, 20263)
WALK_STEPS = 60
CASE_NAMES = sorted(HC.CASES)

_EXPECT = {}          # expect_key -> the restatement's dict            } computed once per session
_FRESH = {}           # expect_key -> the fresh-context child's dict     }
CPU_SECONDS = [0.0]   # time spent in restatements (printed by the walks, not GPU time)


def _restated(oracle, case, variant, on):
    key = case.expect_key(variant, on)
    if key not in _EXPECT:
        t = time.time()
        _EXPECT[key] = case.expect(oracle, case.make(variant), on)
        CPU_SECONDS[0] += time.time() - t
    return _EXPECT[key]


def _child(key, tmp_dir):
    name, variant, guided = key
    out = os.path.join(tmp_dir, f"{name}_{variant}_{int(guided)}.npz")
    env = {k: v for k, v in os.environ.items() if not k.startswith("R3DM_")}
    r = subprocess.run(HC.fresh_command(out, name, variant, ["guided"] if guided else []), capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (key, r.stderr[-2000:])
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="session")
def fresh(tmp_path_factory):
    """key -> output of the case on a fresh context in a process of its own, computed on first use and kept for the session.  One
    child at a time, and a child that fails ends the series: nothing more is started on the GPU after it."""
    tmp_dir = str(tmp_path_factory.mktemp("fresh"))
    failed = []

    def get(key):
        if key not in _FRESH:
            assert not failed, f"an earlier fresh-context child failed ({failed[0]}): no further children are started"
            try:
                _FRESH[key] = _child(key, tmp_dir)
            except BaseException:
                failed.append(key)
                raise
        return _FRESH[key]
    return get


def _check(oracle, fresh, case, variant, on, got, trail=""):
    """`got` against the expected value of (case, variant, switches): restated keys against the restatement, the others against the
    fresh context"""
    exp = _restated(oracle, case, variant, on)
    bad = HC.differences(got, exp)
    assert not bad, f"{case.name}/{variant}/{sorted(on)}: {bad} differ from the CPU restatement\n{trail}"
    rest = [k for k in got if k not in exp]
    if rest:
        assert case.fresh, f"{case.name}: keys {rest} are not restated and the case names no reason"
        f = fresh(case.expect_key(variant, on))
        bad = HC.differences(got, f, rest)
        assert not bad, f"{case.name}/{variant}/{sorted(on)}: {bad} differ from a fresh context's\n{trail}"
        restated_bad = HC.differences(f, exp)
        assert not restated_bad, f"{case.name}/{variant}: the FRESH context differs from the restatement in {restated_bad}"


def _open():
    return api.Context(0)


# ---- a. repeatability first -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_small_variant_repeats_on_two_fresh_contexts(oracle, fresh, name):
    case = HC.CASES[name]
    inp = case.make("small")
    outs = []
    for _ in range(2):
        ctx = _open()
        try:
            outs.append(case.run(ctx, inp))
        finally:
            ctx.close()
    assert outs[0].keys() == outs[1].keys()
    assert not HC.differences(outs[0], outs[1]), f"{name}: two fresh contexts disagree -- not a history effect, explain this first"
    _check(oracle, fresh, case, "small", frozenset(), outs[0])


# ---- b. large, small, large, small on one context ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_large_then_small_then_large_then_small(oracle, fresh, name):
    case = HC.CASES[name]
    fast = frozenset(case.switches) - {"guided"}        # the fast paths and device graphs on: more layouts and mirrors to leave behind
    ctx = _open()
    try:
        # the cases that read set_guided_matching (the filters) run the schedule a second time with it on, on the same context
        for on in [fast] + ([fast | {"guided"}] if "guided" in case.switches else []):
            smalls = []
            for step, variant in enumerate(("large", "small", "large", "small")):
                got = case.run(ctx, case.make(variant), on)
                _check(oracle, fresh, case, variant, on, got, trail=f"step {step} of large, small, large, small; switches {sorted(on)}")
                if variant == "small":
                    smalls.append(got)
            assert not HC.differences(smalls[0], smalls[1])
    finally:
        ctx.close()


def test_preset_constants_of_the_case_table_are_the_librarys():
    """history_cases restates with plain numbers (the CPU proof loads no GPU library); they are the presets the runs use"""
    kp, hf, hm, mp = api.KGraphParams.preset("default"), api.HnswParams.preset("fast"), api.HnswParams.preset("medium"), api.MrptParams.preset()
    assert dict(index_K=kp.index_K, search_P=kp.search_P, search_S=kp.search_S, seed=kp.seed) == HC.KGRAPH_DEFAULT
    assert dict(M=hf.M, ef_construction=hf.ef_construction, ef=hf.ef, seed=hf.seed) == HC.HNSW_FAST
    assert dict(M=hm.M, ef_construction=hm.ef_construction, ef=hm.ef, seed=hm.seed) == HC.HNSW_MEDIUM
    assert dict(n_trees=mp.n_trees, depth=mp.depth, votes=mp.votes, density=mp.density, seed=mp.seed) == HC.MRPT_PRESET


@pytest.mark.parametrize("name", HC.DEV_CASES)
def test_large_small_large_small_past_the_branches_only_the_developer_build_reaches(oracle, fresh, name, tmp_path):
    """The classic arm's hand-back of a component above the wavefront bound and guided matching's candidate chunks are out of reach
    of the product's constants at test sizes (history_cases says why).  The developer build moves the two bounds between the small
    and the large variant (HC.DEV_KNOBS; tests/test_history_cases.py proves the placement), and a child process runs
    large, small, large, small on one context of it: same expected values, the bounds change no result."""
    case = HC.CASES[name]
    on = frozenset({"guided"}) if "guided" in case.switches else frozenset()
    variants = ("large", "small", "large", "small")
    out = str(tmp_path / "dev.npz")
    env = dict({k: v for k, v in os.environ.items() if not k.startswith("R3DM_")}, **HC.DEV_KNOBS)
    r = subprocess.run(HC.fresh_command(out, name, variants, on, developer=True), capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    with np.load(out) as z:
        flat = {k: z[k] for k in z.files}
    for step, variant in enumerate(variants):
        got = {k[len(str(step)) + 1:]: v for k, v in flat.items() if k.startswith(f"{step}_")}
        _check(oracle, fresh, case, variant, on, got, trail=f"developer build, {HC.DEV_KNOBS}, step {step}")


# ---- c. replace and shrink views ---------------------------------------------------------------------------------------------------
def _shrink_views(kind, rows, seed):
    sc = synth.make_scene(len(rows), max(rows), "sift" if kind == "u8" else kind, seed=seed)
    descs = [np.ascontiguousarray(d[:n]) for d, n in zip(sc.descs, rows)]
    if kind == "u8":
        descs = [d.astype(np.uint8) for d in descs]
    return descs, [np.ascontiguousarray(x[:n]) for x, n in zip(sc.xys, rows)]


@pytest.mark.parametrize("kind,switch,counter", [("sift", "integer_mfma", "n_integer_mfma"), ("u8", "integer_mfma", None), ("liop", "split_mfma", "n_split_mfma"),
                                                 ("liopc", "split_mfma", "n_counts_mfma"), ("akaze", "hamming_mfma", "n_hamming_mfma")])
def test_replaced_and_shrunk_views_match_like_fresh_ones(oracle, kind, switch, counter):
    """Views are replaced by views of 0.8 - 0.95 of their size.  A replaced view keeps its slot and its buffers (DevBuf::ensure
    returns at once when bytes <= cap), so the old view's last tiles stay behind the new one's (the matching kernels read rows behind
    a view by design: tile padding, kSlackBytes).  With the fast-path layout of
    the descriptor type staged (bf16 tiles, split planes, count tiles -- whose padding rows no kernel writes --, byte tiles) and without; then after clear_images() and a
    registration in another order."""
    binary = kind == "akaze"
    ratio, squared = (0.8, False) if binary else (0.6, True)
    big_rows = [b for b, _ in HC.SHRINK_ROWS] + [1000]
    small_rows = [s for _, s in HC.SHRINK_ROWS] + [1000]
    big = _shrink_views(kind, big_rows, 7100)
    small = _shrink_views(kind, small_rows, 7200)
    pairs = np.array([(i, j) for i in range(4) for j in range(i + 1, 4)], np.uint32)

    def expect(descs, xys):
        c, m = oracle.match_collection(descs, xys, pairs, ratio, squared, binary=binary)
        return HC._expected_graph(pairs, c, m)
    def mix(which):                                                      # view v from `small` where which[v], else from `big`
        return ([(small if w else big)[0][v] for v, w in enumerate(which)], [(small if w else big)[1][v] for v, w in enumerate(which)])
    e_big, e_small = expect(*big), expect(*small)
    e_shrunk, e_regrown = expect(*mix((1, 1, 1, 0))), expect(*mix((1, 0, 1, 0)))
    ctx = _open()
    try:
        for on in (frozenset({switch}), frozenset()):
            HC.apply_switches(ctx, on)

            def register(views, order):
                for v in order:
                    ctx.set_image(v, views[0][v], views[1][v], 4000, 3000, binary=binary)

            def matched(exp, what):
                bad = HC.differences(HC._graph(ctx.match_pairs(pairs, ratio, squared)), exp)
                assert not bad, f"{kind}, switches {sorted(on)}: {bad} differ after {what}"
                if on and counter:
                    assert getattr(ctx.stats(), counter) == 1, f"{kind}: the {switch} path did not run after {what}"
            register(big, range(4)); matched(e_big, "the first registration")
            register(small, range(3)); matched(e_shrunk, "replacing views 0-2 by smaller ones")
            register(big, (1,)); matched(e_regrown, "growing view 1 back")
            ctx.clear_images()
            register(small, (3, 1, 2, 0)); matched(e_small, "clear_images and a registration in another order")
            ctx.clear_images()
    finally:
        ctx.close()


# ---- d. ordered pairs inside the families that share scratch -----------------------------------------------------------------------
@pytest.mark.parametrize("family", sorted(HC.FAMILIES))
def test_every_ordered_pair_inside_a_family(oracle, fresh, family):
    """A (large) then B (small), B checked, for every ordered pair of operations that share d_cnt / d_fb / d_nn (the matchers), coop_sched
    and fb[] (the filter kinds and filter_FEH subsets), liop_cnt (the LIOP entries), the detector planes (Fast, classic, extract_liop);
    one context per family, so that the pairs also follow each other"""
    members = HC.FAMILIES[family]
    ctx = _open()
    try:
        for a in members:
            for b in members:
                if a == b:
                    continue
                A, B = HC.CASES[a], HC.CASES[b]
                got_a = A.run(ctx, A.make("large"))
                _check(oracle, fresh, A, "large", frozenset(), got_a, trail=f"{a} (large) before {b}")
                got_b = B.run(ctx, B.make("small"))
                _check(oracle, fresh, B, "small", frozenset(), got_b, trail=f"{b} (small) after {a} (large)")
    finally:
        ctx.close()


# ---- e. after an error -------------------------------------------------------------------------------------------------------------
def test_a_refused_call_leaves_nothing_behind(oracle, fresh, tmp_path):
    """every documented refusal, followed by a normal operation of the same family whose output is checked"""
    from test_oracle_hnsw import load_case
    ctx = _open()

    def then(name, variant="small", on=frozenset()):
        case = HC.CASES[name]
        _check(oracle, fresh, case, variant, on, case.run(ctx, case.make(variant), on), trail=f"{name} after a refused call")
    try:
        big = HC.CASES["mrpt_knn2"].make("large")
        HC.CASES["mrpt_knn2"].run(ctx, big)                                          # (something large first: there are leftovers to meet)
        with pytest.raises(api.R3dmError):
            ctx.mrpt_knn2(big["dataset"][:100], big["query"][:4], api.MrptParams.preset())          # fewer than 128 rows
        then("mrpt_knn2")
        with pytest.raises(api.R3dmError):
            ctx.mrpt_knn2(big["dataset"], big["query"][:4], api.MrptParams(4, 6, 5, -1.0, 0))       # votes > trees
        then("mrpt_knn2"); then("match_mrpt", "large")
        d0, d1, ix, _, _ = load_case("sift", "fast")
        M = oracle.HNSW_PRESETS["fast"][0]
        bad = dict(ix); bad["links0"] = ix["links0"].copy(); bad["links0"][5, 1] = len(d0)        # a link past the last row
        with pytest.raises(api.R3dmError):
            ctx.hnsw_knn2_on_index(d0, bad, M, d1, 5)
        then("hnsw_knn2"); then("match_hnsw", "large")
        inp = HC.filter_inputs("large")
        put = HC._filter_register(ctx, inp)
        for fn in (ctx.filter_F, ctx.filter_E, ctx.filter_H):
            with pytest.raises(api.R3dmError):
                fn(put, 4.0, 0)                                                           # max_iter == 0
        with pytest.raises(api.R3dmError):
            ctx.filter_FEH(put, "FEH", 4.0, 0)
        then("filter_F"); then("filter_FEH", "large"); then("filter_E", "small", frozenset({"guided"}))
        ims = HC.features_inputs("large")["images"]
        ctx.set_deferred_feature_files(True)
        ctx.extract_features_batch(ims[:1], [str(tmp_path / "no_such_dir" / "a.feat")], [str(tmp_path / "no_such_dir" / "a.desc")])
        with pytest.raises(api.R3dmError):
            ctx.features_files_wait()                                                     # the unwritable path, reported by the wait
        then("extract_features_batch", "small", frozenset({"deferred"})); then("extract_features_to_files", "large")
        with pytest.raises(api.R3dmError):
            ctx._check(ctx._L.r3dm_set_keypoint_detector(ctx._h, 2), "r3dm_set_keypoint_detector")      # a detector the library does not serve
        then("detect_akaze"); then("detect_akaze_classic"); then("extract_features_to_files")
        with pytest.raises(api.R3dmError):
            ctx.knn2(np.zeros((1, 128), np.float32), np.zeros((4, 128), np.float32))      # NN = 2 > rows
        then("knn2_int"); then("knn2_bin", "small", frozenset({"hamming_mfma"}))
    finally:
        ctx.close()


# ---- f. seeded walks ---------------------------------------------------------------------------------------------------------------
def _walk(seed, steps):
    rng = np.random.default_rng(seed)
    for _ in range(steps):
        name = CASE_NAMES[int(rng.integers(len(CASE_NAMES)))]
        variant = HC.VARIANTS[int(rng.integers(2))] if rng.random() < 0.8 else "small"
        on = frozenset(s for s in HC.CASES[name].switches if rng.random() < 0.5)
        yield name, variant, on


@pytest.mark.parametrize("seed", WALK_SEEDS)
def test_a_seeded_walk_over_all_cases(oracle, fresh, seed):
    """60 steps over all cases, variants and switches on one context, every step checked.  A failure names the seed and the trail up
    to the failing step: replay it with _walk(seed, n) and cut it down by hand."""
    ctx = _open()
    trail = []
    try:
        for step, (name, variant, on) in enumerate(_walk(seed, WALK_STEPS)):
            trail.append(f"{step}: {name}/{variant}/{'+'.join(sorted(on)) or '-'}")
            case = HC.CASES[name]
            got = case.run(ctx, case.make(variant), on)
            _check(oracle, fresh, case, variant, on, got, trail=f"seed {seed}, trail:\n  " + "\n  ".join(trail))
        print(f"walk {seed}: {CPU_SECONDS[0]:.1f} s of CPU restatements so far this session ({len(_EXPECT)} expected values, {len(_FRESH)} fresh-context children)")
    finally:
        ctx.close()


def test_a_walk_over_the_entries_of_a_multi_context(oracle, fresh, tmp_path):
    """MultiContext([0, 0]): set_image, match_pairs*, filter_*, extract_features in a seeded order, large and small collections
    alternating; graphs against the single-context expectations (the multi entries promise the same graphs)"""
    m = api.MultiContext([0, 0])
    rng = np.random.default_rng(20264)
    trail = []
    try:
        for step in range(16):
            variant = HC.VARIANTS[step % 2] if step < 8 else HC.VARIANTS[int(rng.integers(2))]
            op = ["match_sift", "match_kgraph", "match_hnsw", "filter_F", "filter_E", "filter_H", "features"][int(rng.integers(7))]
            trail.append(f"{step}: {op}/{variant}")
            msg = "MultiContext walk, trail:\n  " + "\n  ".join(trail)
            if op == "features":
                inp = HC.features_inputs(variant)
                d = tmp_path / f"s{step}"; d.mkdir()
                fs = [str(d / f"i{k}.feat") for k in range(3)]; ss = [str(d / f"i{k}.desc") for k in range(3)]
                nf, sk = m.extract_features(inp["images"], fs, ss, inp["thr"])
                assert not sk.any(), msg
                case = HC.CASES["extract_features_batch"]
                got = dict(n=np.asarray(nf, np.uint32))
                for k in range(3):
                    got[f"feat{k}"] = HC._read(fs[k]); got[f"desc{k}"] = HC._read(ss[k])
                _check(oracle, fresh, case, variant, frozenset(), {k: np.ascontiguousarray(v) for k, v in got.items()}, trail=msg)
                continue
            case = HC.CASES[op]
            inp = case.make(variant)
            for v, (dsc, xy) in enumerate(zip(inp["descs"], inp["xys"])):
                m.set_image(v, dsc, xy, 4000, 3000)
            if op.startswith("filter_"):
                kind = op[-1]
                for v in range(len(inp["descs"])):
                    m.set_intrinsics(v, inp["K"])
                put = api.Graph.from_csr(inp["pairs"], inp["offsets"], inp["matches"])
                g, M = {"F": m.filter_F, "E": m.filter_E, "H": m.filter_H}[kind](put, **{"want_" + kind: True})
                got = HC._filter_out(kind, g, M)
            elif op == "match_sift":
                got = HC._graph(m.match_pairs(inp["pairs"], 0.6, True))
            elif op == "match_kgraph":
                got = HC._graph(m.match_pairs_kgraph(inp["pairs"], 0.6, api.KGraphParams.preset("default")))
            else:
                got = HC._graph(m.match_pairs_hnsw(inp["pairs"], 0.8, api.HnswParams.preset("fast")))
            _check(oracle, fresh, case, variant, frozenset(), {k: np.ascontiguousarray(v) for k, v in got.items()}, trail=msg)
    finally:
        m.close()


# ---- the regression the lattice images exposed ------------------------------------------------------------------------------------------
def test_lattice_levels_of_one_giant_component_repeat_on_one_context(oracle):
    """Named regression (found by the first run of the lattice tests of tests/test_gpu_akaze.py): on the exactly periodic images whole
    levels are ONE connected component of the in-level pruning.  ak_prune_flatten_kernel used the path-halving find, so another lane's
    halving store could put a mere ancestor back over a root just stored; the member then failed `par[j] == root`, the gather of the
    queued component filled fewer than `sz` indices, and the rest were whatever out1 (the gather area, never cleared) held from the
    call before: r3dm_detect_akaze ended in an illegal memory access on a context that had detected before, while the same calls on
    fresh memory had passed.  Timing-dependent, so this test cannot be made to fail at will; it keeps the schedule: each lattice
    image three times on one context, every result against the oracle."""
    import akaze_lattices
    imgs = akaze_lattices.lattice_images()
    ref = {name: oracle.akaze_detect(img, 0.0) for name, img in imgs.items()}
    ctx = _open()
    try:
        for rep in range(3):
            for name in sorted(imgs):
                kps, resp = ctx.detect_akaze(imgs[name], 0.0)
                assert np.array_equal(kps, ref[name]["kps"]) and np.array_equal(resp, ref[name]["responses"]), (name, rep)
    finally:
        ctx.close()


# ---- g. the C++ facade: two stages on one stage object ----------------------------------------------------------------------------------
def test_second_stage_of_a_host_process_writes_the_files_of_a_single_stage_run(oracle, tmp_path):
    """tests/cpp/adapter_main.cpp `stages`: two computeMatches on ONE kept-alive R3DComputeMatches object (clearViews between them),
    the larger collection first.  The object owns its context for its lifetime, so the second stage runs in the buffers the first one
    grew and over its registered views.  The second stage's files are byte-equal to those of a process that ran only that stage."""
    from test_cpp_host import _write_views
    exe = str(tmp_path / "adapter_main")
    lib = os.path.join(ROOT, "regard3d_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fopenmp", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "adapter_main.cpp"),
                           "-o", exe, "-L" + lib, "-lr3dm", "-Wl,-rpath," + lib])
    big = synth.make_scene(6, 2000, "sift", seed=8101); small = synth.make_scene(4, 700, "sift", seed=8102)
    dirs = {}
    for tag in ("big", "small_after_big", "small_alone"):
        d = tmp_path / tag; d.mkdir(); dirs[tag] = str(d)
    names_big = _write_views(oracle, dirs["big"], big)
    names_small = _write_views(oracle, dirs["small_after_big"], small)
    _write_views(oracle, dirs["small_alone"], small)
    env = {k: v for k, v in os.environ.items() if not k.startswith("R3DM_")}
    r = subprocess.run([exe, "stages", "128", dirs["big"], str(len(names_big))] + names_big + [dirs["small_after_big"]] + names_small,
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    r1 = subprocess.run([exe, "stage", dirs["small_alone"], "128"] + names_small, capture_output=True, text=True, timeout=600, env=env)
    assert r1.returncode == 0, r1.stderr[-2000:]
    assert r.stdout.split()[2:] == r1.stdout.split() and int(r1.stdout.split()[0]) >= 3
    files = ("matches.putative.bin", "matches.putative.txt", "matches.f.bin", "matches.f.txt", "matches.e.bin", "matches.h.bin")
    for f in files:
        a = open(os.path.join(dirs["small_after_big"], f), "rb").read(); b = open(os.path.join(dirs["small_alone"], f), "rb").read()
        assert a == b and len(b) > 0, f
    pairs = small.exhaustive_pairs()
    c, mm = oracle.match_collection(small.descs, small.xys, pairs, 0.6, True)
    p, cc, m2 = oracle.load_matches(os.path.join(dirs["small_after_big"], "matches.putative.bin"))
    assert np.array_equal(p, pairs[c > 0]) and np.array_equal(cc, c[c > 0]) and np.array_equal(m2, mm)
