"""The case table of vocabulary training and idf-weighted scores (include/r3dm.h, "Trained vocabularies", "idf-weighted scores"),
shared by the CPU proofs (test_vocab_train_cases.py) and the GPU tests (test_gpu_vocab_train.py).  Every case is the smallest shape at
which its kernel can still go wrong; `expected` is the restatement's answer, computed once per case and never changed."""
import functools
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

import vocab_cases as VC
import vocab_restatement as R
import vocab_train_restatement as TR
from regard3d_amd import synth

BLOCK = TR.BLOCK


@dataclass
class TrainCase:
    name: str
    descs: List[np.ndarray]
    ids: List[int]
    max_iterations: int
    n_words: int = 0                          # init: a sampled vocabulary of this many words ...
    vocab: Optional[np.ndarray] = None        # ... or the caller's rows
    binary: bool = False

    def init_rows(self):
        return self.vocab if self.vocab is not None else R.sample_vocab(self.descs, self.n_words)

    @property
    def ns(self):
        return [len(d) for d in self.descs]


def _from(vc, max_iterations):
    return TrainCase(vc.name, vc.descs, vc.ids, max_iterations, n_words=vc.n_words, vocab=vc.vocab, binary=vc.binary)


def _keyed(dim, n_words, key_step, dtype=np.float32):
    """words that differ only in their last element (k * key_step): rows that carry a word's key belong to it whatever else they hold"""
    v = np.zeros((n_words, dim), dtype)
    v[:, dim - 1] = (np.arange(n_words) * key_step).astype(dtype)
    return v


def _deal(rows, sizes):
    """consecutive rows dealt to views of the given sizes"""
    assert sum(sizes) == len(rows)
    at = np.concatenate([[0], np.cumsum(sizes)])
    return [np.ascontiguousarray(rows[at[k]:at[k + 1]]) for k in range(len(sizes))]


@functools.lru_cache(maxsize=None)
def float_division_differs():
    """an integer s = 2^24 + r whose third differs between (float)(s / 3.0) and float(s) / 3.0f"""
    for r in range(1, 4096):
        s = (1 << 24) + r
        if np.float32(np.float64(s) / np.float64(3)) != np.float32(s) / np.float32(3):
            return s
    raise AssertionError("no such sum in the searched range")


def seam_rows(counts, seed, dim=16, jitter=0.5):
    """planted one-hot words plus jitter: counts[w] rows around word w, shuffled (seeded) so that every word's members spread over the views"""
    rng = np.random.default_rng(seed)
    vocab = VC._one_hot_vocab(len(counts), dim)
    rows = np.repeat(vocab, counts, axis=0) + rng.normal(0.0, jitter, (sum(counts), dim)).astype(np.float32)
    return vocab, np.ascontiguousarray(rows[rng.permutation(len(rows))], np.float32)


def _build(name):
    if name in ("sift", "sift_u8", "liop", "akaze"):            # 12 views x 96 rows, 64 sampled words, cap 12
        return _from(VC.case(name), 12)
    if name == "msurf":                                         # real-valued f32 x 64, as M-SURF rows are; a cap it reaches while rows still move
        sc = synth.make_scene(12, 96, "liop", seed=61, dim=64)
        return TrainCase(name, sc.descs, VC._ids(12), 6, n_words=64)
    if name == "multi_block":                                   # every word has several hundred members
        sc = synth.make_scene(6, 400, "sift", seed=62)
        return TrainCase(name, sc.descs, VC._ids(6), 3, n_words=5)
    if name == "block_seam":
        # one word with exactly 256 members, one with 257, one with 255; a 33-row view, an empty view in the middle, ids out of order
        vocab, rows = seam_rows([BLOCK, BLOCK + 1, BLOCK - 1, 40, 1, 0], 63)
        return TrainCase(name, _deal(rows, [33, 300, 0, len(rows) - 333]), [8, 3, 11, 5], 3, vocab=vocab)
    if name == "view_seams":
        vocab, rows = seam_rows([70, 31, 64, 3], 64)
        return TrainCase(name, _deal(rows, [33, 0, 32, 1, len(rows) - 66]), [4, 9, 2, 7, 1], 3, vocab=vocab)
    if name == "one_big_word":
        sc = synth.make_scene(3, 200, "sift", seed=65)
        vocab = np.full((4, 128), 4000.0, np.float32)
        vocab[0] = sc.descs[0][0]
        vocab[1:, 0] += np.arange(3, dtype=np.float32)          # distinct far words
        return TrainCase(name, sc.descs, [2, 0, 1], 3, vocab=vocab)
    if name == "duplicate_words":
        c = VC.case("sift")
        vocab = R.sample_vocab(c.descs, 16)
        vocab[5] = vocab[2]
        return TrainCase(name, c.descs, c.ids, 1, vocab=vocab)
    if name == "distance_tie":
        vocab = np.zeros((3, 8), np.float32)
        vocab[1, 0] = 2.0; vocab[2, 0] = 100.0
        rows = np.zeros((9, 8), np.float32)
        rows[:4, 0] = 1.0                                       # as far from word 0 as from word 1
        rows[4:6, 0] = 0.0; rows[6:8, 0] = 2.0; rows[8, 0] = 100.0
        return TrainCase(name, _deal(rows, [5, 4]), [1, 0], 1, vocab=vocab)
    if name == "f32_arithmetic":
        vocab = _keyed(8, 3, 2.0 ** 32)
        a = np.zeros((2 * BLOCK, 8), np.float32)                # word 0: two blocks
        a[0, 0] = 2.0 ** 30; a[1, 0] = 64.0; a[2:, 0] = 2.0 ** -25          # dimension 0: the second block's increments survive only as a block sum
        a[0, 1] = 2.0 ** 30; a[1, 1] = 64.0; a[2:BLOCK, 1] = 2.0 ** -25     # dimension 1: the increments survive only when added first
        s = float_division_differs()
        b = np.zeros((3, 8), np.float32)                        # word 1: three members whose third is another float when divided in float
        b[0, 2] = 2.0 ** 24; b[1, 2] = float(s - (1 << 24)); b[:, 7] = 2.0 ** 32
        c = np.zeros((2, 8), np.float32)
        c[:, 7] = 2.0 ** 33; c[0, 3] = 1.0
        return TrainCase(name, _deal(np.concatenate([a, b, c]), [300, 2 * BLOCK + 5 - 300]), [0, 1], 2, vocab=vocab)
    if name == "u8_rounding":
        vocab = _keyed(8, 3, 100, np.uint8)
        w0 = np.array([[1, 255, 0, 0, 7, 0, 0, 0], [2, 254, 1, 0, 7, 0, 0, 0]], np.uint8)                    # x.5 thrice: up
        w1 = np.array([[1, 1, 0, 0, 0, 0, 0, 100], [1, 2, 0, 0, 0, 0, 0, 100], [2, 2, 1, 0, 0, 0, 0, 100]], np.uint8)   # 4/3, 5/3, 1/3
        w2 = np.array([[1, 1, 1, 0, 0, 0, 0, 200], [1, 1, 2, 0, 0, 0, 0, 200], [2, 1, 2, 0, 0, 0, 0, 200], [2, 2, 2, 0, 0, 0, 0, 200]], np.uint8)  # 6/4, 5/4, 7/4
        return TrainCase(name, _deal(np.concatenate([w0, w1, w2]), [4, 5]), [3, 1], 2, vocab=vocab)
    if name == "bin_majority":
        vocab = np.zeros((2, 32), np.uint8)
        vocab[1, 8:] = 0xFF
        w0 = np.zeros((4, 32), np.uint8)                        # an even count: bit 0 in half (0), bit 1 in half + 1 (1), bit 2 in all, bit 3 in one
        w0[:, 0] = [0b1111, 0b0111, 0b0110, 0b0100]
        w0[:, 31] = [0x80, 0x80, 0x80, 0x00]                    # the row's last bit, in three of four
        w1 = np.full((3, 32), 0xFF, np.uint8)
        w1[:, :8] = 0
        w1[0, 9] = 0x0F; w1[1, 9] = 0x3C                        # an odd count: bits of byte 9 set in 1, 2 or 3 of 3
        return TrainCase(name, _deal(np.concatenate([w0, w1]), [3, 4]), [6, 2], 2, vocab=vocab, binary=True)
    if name == "max_iterations_1":
        return _from(VC.case("sift"), 1)
    if name == "fixed_point":                                   # every row is a word: the first update changes nothing
        return _from(VC.case("every_row_a_word"), 5)
    raise KeyError(name)


SCENES = ["sift", "sift_u8", "liop", "akaze", "msurf"]
NAMES = SCENES + ["multi_block", "block_seam", "view_seams", "one_big_word", "duplicate_words", "distance_tie", "f32_arithmetic",
                  "u8_rounding", "bin_majority", "max_iterations_1", "fixed_point"]

# what r3dm_vocab_train must refuse (test_gpu_vocab_train.py builds each on the "sift" case).  Two refusals of the header are left out:
# another device's vocabulary (needs a second GPU; the check is the comparison of devices that r3dm_propose_pairs makes, which
# test_gpu_vocab.py cannot reach either) and T >= 2^32 (a view holds fewer than 2^22 rows, so it takes more than 1,024 full views,
# 4 Gi rows of any length: beyond a test)
REFUSALS = ["unknown_view", "duplicate_id", "mixed_type", "mixed_length", "view_unlike_vocab", "max_iterations_0", "no_rows"]


@functools.lru_cache(maxsize=None)
def case(name) -> TrainCase:
    return _build(name)


_EXPECTED = {}


def expected(oracle, name):
    """the restatement's training result of a case (computed once)"""
    if name not in _EXPECTED:
        c = case(name)
        _EXPECTED[name] = TR.train(oracle, c.init_rows(), c.descs, c.max_iterations, c.binary)
    return _EXPECTED[name]


# ------------------------------------------------------------------------------------------------- idf-weighted scores
def _idf_views(hists, ids, top_k=1):
    vocab = VC._one_hot_vocab()
    return VC.Case("idf", [VC._view_of(vocab, VC._hist(16, **h)) for h in hists], ids, top_k, vocab=vocab)


def _build_idf(name):
    if name == "idf_rank_differs":
        # view 0 shares 6 rows of a word that three views hold with C, and 4 rows of a word that only B holds besides itself: counts
        # prefer C, idf prefers B.  Word 0 is in every view and weighs nothing.  B and C have twins they prefer, so view 0's pick shows in
        # the union
        return _idf_views([dict(w0=2, w1=4, w2=6), dict(w0=2, w1=4, w4=6), dict(w0=2, w2=6, w3=4), dict(w0=2, w4=6, w5=9), dict(w0=2, w2=6, w3=4, w6=1)],
                          [9, 2, 3, 1, 4])
    if name == "idf_zero_view":
        # view 2 holds only the word every view holds: W = 0, it proposes nothing and is proposed by nobody
        return _idf_views([dict(w0=3, w1=2), dict(w0=1, w1=2, w2=2), dict(w0=7), dict(w0=2, w2=2)], [5, 1, 8, 3], top_k=3)
    if name == "idf_key_tie":
        # for view 0, B and C give the same key (same weighted intersection, same W): the lower view id comes first, and it is listed second
        return _idf_views([dict(w0=1, w1=3, w2=3), dict(w0=1, w2=3, w3=1), dict(w0=1, w1=3, w4=1), dict(w0=1, w3=1, w4=1)], [9, 7, 4, 2])
    raise KeyError(name)


IDF_NAMES = ["idf_rank_differs", "idf_zero_view", "idf_key_tie"]


@functools.lru_cache(maxsize=None)
def idf_case(name) -> VC.Case:
    return _build_idf(name)


_IDF_EXPECTED = {}


def idf_expected(oracle, name, ids=None):
    """hist, counts result and idf result of an idf case (or of its views `ids` alone), by the restatement"""
    c = idf_case(name)
    key = (name, tuple(ids) if ids is not None else None)
    if key not in _IDF_EXPECTED:
        sel = list(range(len(c.ids))) if ids is None else [c.ids.index(i) for i in ids]
        descs = [c.descs[k] for k in sel]
        lids = [c.ids[k] for k in sel]
        ns = [len(d) for d in descs]
        hist = R.signatures(oracle, c.vocab, descs)
        s = R.scores(hist)
        _IDF_EXPECTED[key] = dict(hist=hist, ns=ns, ids=lids, counts=dict(scores=s, pairs=R.propose(s, ns, lids, c.top_k)),
                                  idf=TR.propose_idf(hist, ns, lids, c.top_k))
    return _IDF_EXPECTED[key]
