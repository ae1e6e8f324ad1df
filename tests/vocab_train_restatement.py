"""numpy restatement of vocabulary training and idf-weighted scores (include/r3dm.h, "Trained vocabularies" and "idf-weighted scores";
DESIGN.md section 4.30).  The assignment is the word rule of vocab_restatement.py on the oracle's exact 2-NN; the update adds in the
order the header states -- np.cumsum is sequential, np.sum is pairwise and is not used on floats --; log2_q8 and the keys are Python
integers."""
import numpy as np

import vocab_restatement as R

BLOCK = 256                    # R3DM_VOCAB_TRAIN_BLOCK


def _seq_sum(x, acc):
    """the rows of x added one after the other from 0.0, per column, in `acc` precision"""
    return np.cumsum(np.concatenate([np.zeros((1, x.shape[1]), acc), x.astype(acc)]), axis=0, dtype=acc)[-1]


def mean_f32(members, order="tree", acc=np.float64, divide=np.float64):
    """the F32 update of one word from its member rows (ascending g).  order: "tree" (the rule: blocks of 256 members, then the block
    sums), "flat" (one sequential sum), "reversed" (the tree over the members in descending g); acc / divide: the accumulator's and the
    division's type -- the rule is float64 for both"""
    m = members[::-1] if order == "reversed" else members
    if order == "flat":
        s = _seq_sum(m, acc)
    else:
        s = _seq_sum(np.stack([_seq_sum(m[b:b + BLOCK], acc) for b in range(0, len(m), BLOCK)]), acc)
    return (s.astype(divide) / divide(len(m))).astype(np.float32)


def mean_u8(members):
    s = members.astype(np.int64).sum(axis=0)                   # integers: any order
    c = len(members)
    return ((2 * s + c) // (2 * c)).astype(np.uint8)


def mean_bin(members):
    ones = np.unpackbits(members, axis=1, bitorder="little").astype(np.int64).sum(axis=0)
    return np.packbits((2 * ones > len(members)).astype(np.uint8), bitorder="little")


def update(words, rows, a, binary=False, **how):
    """the words after one update: every word with members becomes their mean under the rule of its type"""
    out = words.copy()
    for w in range(len(words)):
        g = np.flatnonzero(a == w)                             # ascending g
        if len(g) == 0:
            continue                                           # an empty word keeps its row
        m = rows[g]
        out[w] = mean_bin(m) if binary else (mean_u8(m) if words.dtype == np.uint8 else mean_f32(m, **how))
    return out


def train(oracle, init, descs, max_iterations, binary=False, **how):
    """r3dm_vocab_train over the rows of descs in list order -> dict(words, assign, n_updates, converged, n_moved, n_empty, max_members,
    n_rows_assigned, history = moved_t of every assignment)"""
    assert max_iterations >= 1
    rows = np.concatenate([d for d in descs if len(d)], axis=0)
    T = len(rows)
    words = np.ascontiguousarray(init).copy()
    prev, n_updates, converged, assigned, history = None, 0, False, 0, []
    while True:
        a = R.words_of(oracle, words, rows, binary)
        assigned += T
        moved = T if prev is None else int((a != prev).sum())
        history.append(moved)
        prev = a
        if len(history) > 1 and moved == 0:
            converged = True
            break
        words = update(words, rows, a, binary, **how)
        n_updates += 1
        if n_updates == max_iterations:
            break
    cnt = np.bincount(prev, minlength=len(words))
    return dict(words=words, assign=prev, n_updates=n_updates, converged=converged, n_moved=moved, n_empty=int((cnt == 0).sum()),
                max_members=int(cnt.max()), n_rows_assigned=assigned, history=history)


# ------------------------------------------------------------------------------------------------- idf weights
def log2_q8(N, df):
    """256 log2(N / df) by the header's integer procedure, N >= df >= 1"""
    N, df = int(N), int(df)
    assert N >= df >= 1
    e = 0
    while (df << (e + 1)) <= N:
        e += 1
    x = (N << (62 - e)) // df
    assert (1 << 62) <= x < (1 << 63)
    q = e
    for _ in range(8):
        x = (x * x) >> 62
        q *= 2
        if x >= (1 << 63):
            x >>= 1
            q += 1
    return q


def weights(hist, ns):
    N = sum(1 for n in ns if n)
    df = (np.asarray(hist)[[k for k, n in enumerate(ns) if n]] > 0).sum(axis=0) if N else np.zeros(hist.shape[1], np.int64)
    return np.array([log2_q8(N, d) if d else 0 for d in df.tolist()], np.uint32)


def weighted_scores(hist, q):
    """(s, W) under IDF as Python-exact int64: s(i, j) = sum_w q[w] min(h_i[w], h_j[w]), W_i = sum_w q[w] h_i[w]"""
    h = hist.astype(np.int64)
    qq = q.astype(np.int64)
    s = (np.minimum(h[:, None, :], h[None, :, :]) * qq).sum(axis=2)
    np.fill_diagonal(s, 0)
    return s, (h * qq).sum(axis=1)


def propose_idf(hist, ns, ids, top_k):
    """dict(q, W, scores, pairs) of r3dm_propose_pairs under R3DM_VOCAB_WEIGHT_IDF; pairs is None where the call refuses (a W >= 2^32)"""
    q = weights(hist, ns)
    s, W = weighted_scores(hist, q)
    if (W >= (1 << 32)).any():
        return dict(q=q, W=W, scores=None, pairs=None)
    return dict(q=q, W=W, scores=s.astype(np.uint32), pairs=R.propose(s, [int(x) for x in W], ids, top_k))
