"""The case table of pair proposal (include/r3dm.h, "Pair proposal"), shared by the CPU proofs (test_vocab_cases.py) and the GPU tests
(test_gpu_vocab.py).  Every case is the smallest shape at which its kernel can still go wrong; `expected` is the restatement's
answer, computed once per case and never changed."""
import functools
import os
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

import vocab_restatement as R
from regard3d_amd import synth

HIST_LDS_WORDS = 8192          # R3DM_VOCAB_HIST_LDS_WORDS
WORD_CHUNK = 32                # R3DM_VOCAB_WORD_CHUNK
VIEW_TILE = 64                 # views per side of a score tile (kVocabTile)


@dataclass
class Case:
    name: str
    descs: List[np.ndarray]
    ids: List[int]
    top_k: int
    n_words: int = 0                          # sampled vocabulary of this many words ...
    vocab: Optional[np.ndarray] = None        # ... or the caller's rows
    binary: bool = False

    def vocab_rows(self):
        return self.vocab if self.vocab is not None else R.sample_vocab(self.descs, self.n_words)

    @property
    def ns(self):
        return [len(d) for d in self.descs]


def _ids(n):
    """view ids that are neither 0 .. n-1 nor in list order"""
    return [10 + (7 * k) % n for k in range(n)] if n % 7 else [10 + 3 * (n - 1 - k) for k in range(n)]


def _scene(name, n_views, n_rows, kind, n_words, top_k, seed, u8=False):
    sc = synth.make_scene(n_views, n_rows, kind, seed=seed, dim=61 if kind == "akaze" else None)
    descs = [d.astype(np.uint8) for d in sc.descs] if u8 else sc.descs
    return Case(name, descs, _ids(n_views), top_k, n_words=n_words, binary=kind == "akaze")


def _one_hot_vocab(n_words=16, dim=16):
    v = np.zeros((n_words, dim), np.float32)
    v[np.arange(n_words), np.arange(n_words) % dim] = 100.0
    return v


def _view_of(vocab, hist):
    """rows that quantise to exactly `hist`: hist[w] copies of word w"""
    return np.ascontiguousarray(np.repeat(vocab[:len(hist)], hist, axis=0))


def _hist(n_words, **at):
    h = np.zeros(n_words, np.int64)
    for w, c in at.items():
        h[int(w[1:])] = c
    return h


def _key_case(name, hists, ids, top_k=1):
    """view 0 (the highest id) ranks B and C; each of them has a twin (D, E) that it prefers to view 0, so with top_k 1 the pair
    that view 0 proposes is in the union only because view 0 proposed it"""
    vocab = _one_hot_vocab()
    h0, hb, hc = hists
    assert len(ids) == 5 and ids[0] == max(ids)
    return Case(name, [_view_of(vocab, h) for h in (h0, hb, hc, hb, hc)], ids, top_k, vocab=vocab)


def _small_int_views(n_views, n_rows, dim, n_words, seed):
    rng = np.random.default_rng(seed)
    vocab = rng.integers(0, 256, (n_words, dim)).astype(np.float32)
    descs = []
    for _ in range(n_views):
        base = vocab[rng.integers(0, n_words, n_rows)]
        descs.append(np.clip(base + rng.integers(-3, 4, base.shape), 0, 255).astype(np.float32))
    return vocab, descs


def _build(name):
    if name == "sift":
        return _scene(name, 12, 96, "sift", 64, 3, 41)
    if name == "liop":
        return _scene(name, 12, 96, "liop", 64, 3, 42)
    if name == "akaze":
        return _scene(name, 12, 96, "akaze", 64, 3, 43)
    if name == "sift_u8":
        return _scene(name, 12, 96, "sift", 64, 3, 41, u8=True)
    if name == "views13":
        return _scene(name, 13, 40, "sift", 64, 2, 44)
    if name == "views17":
        return _scene(name, 17, 40, "sift", 64, 2, 45)
    if name == "views_two_tiles":                               # one more view than a score tile holds
        vocab, descs = _small_int_views(VIEW_TILE + 3, 6, 8, 16, 46)
        return Case(name, descs, _ids(VIEW_TILE + 3), 2, vocab=vocab)
    if name == "words67":
        return _scene(name, 12, 48, "sift", 67, 3, 47)
    if name == "words_chunk_plus_1":
        return _scene(name, 12, 48, "sift", WORD_CHUNK + 1, 3, 48)
    if name in ("hist_lds_bound", "hist_lds_bound_plus_1"):
        nw = HIST_LDS_WORDS + (name.endswith("plus_1"))
        vocab, descs = _small_int_views(3, 50, 8, nw, 49)
        descs[1][:5] = vocab[nw - 1]                            # the last word is counted
        return Case(name, descs, [4, 2, 9], 1, vocab=vocab)
    if name == "ties":
        # words 0 / 2 and 1 / 3 are the same rows: ties go to the lower word, the duplicates count nothing
        vocab = _one_hot_vocab(6, 8)
        vocab[2] = vocab[0]; vocab[3] = vocab[1]
        hs = [[3, 2, 0, 0, 1, 0], [1, 4, 0, 0, 0, 2], [2, 2, 0, 0, 2, 2]]
        base = _one_hot_vocab(6, 8)
        base[2] = base[0]; base[3] = base[1]
        descs = [_view_of(base, h) for h in hs]
        descs[0] = np.concatenate([descs[0], vocab[2:4]])       # rows that ARE the duplicates: words 0 and 1 still
        return Case(name, descs, [7, 3, 5], 1, vocab=vocab)
    if name == "key_beats_raw_score":
        # for view 0 (20 rows): B has 3 of 3 rows in common (fraction 1), C 10 of 20 (fraction 1/2, the larger raw score)
        return _key_case(name, [_hist(16, w0=10, w1=3, w2=7), _hist(16, w1=3), _hist(16, w0=10, w3=10)], [9, 2, 3, 1, 4])
    if name == "key_equal_fractions":
        # 3/6 (B, D) and 2/4 (C, E) tie as keys: the lowest view id comes first, and that is C's; raw s would take a 3
        return _key_case(name, [_hist(16, w0=2, w1=3, w2=5), _hist(16, w1=3, w3=3), _hist(16, w0=2, w4=2)], [9, 8, 4, 7, 5])
    if name == "key_below_float_resolution":
        a, b = float_tie()
        (s1, n1), (s2, n2) = a, b                               # s1 / n1 < s2 / n2 as integers, equal as float32; the first has the lower id
        return _key_case(name, [_hist(16, w0=s1, w1=s2), _hist(16, w0=n1), _hist(16, w1=n2)], [9, 5, 7, 6, 8])
    if name == "empty_view":
        c = _scene(name, 5, 40, "sift", 32, 2, 50)
        c.descs[2] = np.zeros((0, 128), np.float32)
        return c
    if name == "every_row_a_word":
        c = _scene(name, 4, 16, "sift", 64, 1, 51)
        return c
    if name == "top_k_1":
        return _scene(name, 6, 40, "sift", 32, 1, 52)
    if name == "top_k_everything":
        return _scene(name, 6, 40, "sift", 32, 5, 53)
    raise KeyError(name)


NAMES = ["sift", "liop", "akaze", "sift_u8", "views13", "views17", "views_two_tiles", "words67", "words_chunk_plus_1", "hist_lds_bound",
         "hist_lds_bound_plus_1", "ties", "key_beats_raw_score", "key_equal_fractions", "key_below_float_resolution", "empty_view",
         "every_row_a_word", "top_k_1", "top_k_everything"]

# what r3dm_vocab_sample / r3dm_propose_pairs must refuse with R3DM_ERR_INVALID (test_gpu_vocab.py builds each on the "sift" case)
REFUSALS = ["n_words_above_T", "n_words_1", "top_k_0", "unknown_view", "duplicate_id", "mixed_type", "mixed_length", "view_unlike_vocab",
            "cap_pairs_too_small"]


@functools.lru_cache(maxsize=None)
def float_tie():
    """two fractions s / n below 1 that differ as integers by less than float32 resolution: (s1, n1), (s2, n2) with
    s1 / n1 < s2 / n2 exactly and float32(s1) / float32(n1) == float32(s2) / float32(n2)"""
    for n1 in range(5000, 5200):
        s1 = n1 - 1
        for n2 in range(2 * n1 - 3, 2 * n1 + 4):
            for s2 in (n2 - 2, n2 - 1):
                if s1 * n2 < s2 * n1 and np.float32(s1) / np.float32(n1) == np.float32(s2) / np.float32(n2):
                    return (s1, n1), (s2, n2)
    raise AssertionError("no float32 tie in the searched range")


@functools.lru_cache(maxsize=None)
def case(name) -> Case:
    return _build(name)


_EXPECTED = {}


def expected(oracle, name):
    """the restatement's words vocabulary, histograms, scores and pairs of a case (computed once)"""
    if name not in _EXPECTED:
        c = case(name)
        vocab = c.vocab_rows()
        hist = R.signatures(oracle, vocab, c.descs, c.binary)
        s = R.scores(hist)
        _EXPECTED[name] = dict(vocab=vocab, hist=hist, scores=s, pairs=R.propose(s, c.ns, c.ids, c.top_k))
    return _EXPECTED[name]


def raw_score(s, ni, nj):
    return int(s)


def float_fraction(s, ni, nj):
    return float(np.float32(s) / np.float32(min(ni, nj)))


def assert_files_restricted(oracle, off_dir, on_dir, keep):
    """matches.putative.txt / matches.f.txt of on_dir are those of off_dir restricted to the pairs `keep`"""
    for name in ("matches.putative.txt", "matches.f.txt"):
        p, c, m = oracle.load_matches(os.path.join(off_dir, name))
        off = np.concatenate([[0], np.cumsum(c.astype(np.int64))])
        rp, rn, rm = R.restrict_graph(p, off, m, keep)
        q, qc, qm = oracle.load_matches(os.path.join(on_dir, name))
        assert np.array_equal(q, rp) and np.array_equal(qc, rn) and np.array_equal(qm, rm), name
