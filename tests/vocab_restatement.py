"""numpy restatement of pair proposal from bag-of-words view signatures (include/r3dm.h, "Pair proposal"): the
sample rule, the word of a row, the histogram, the score, the key, the rank and the union -- every quantity an integer, the key in
Python integers.  The word rule runs on the oracle's exact 2-NN (oracle/pyoracle.py: knn2, ties to the lowest row)."""
import numpy as np


def sample_rows(ns, n_words):
    """rows of the concatenation (list order) that become words: floor((2 t + 1) T / (2 n_words))"""
    T = int(sum(ns))
    assert 2 <= n_words <= T
    return [((2 * t + 1) * T) // (2 * n_words) for t in range(n_words)]


def sample_vocab(descs, n_words):
    return np.ascontiguousarray(np.concatenate([d for d in descs if len(d)], axis=0)[sample_rows([len(d) for d in descs], n_words)])


def words_of(oracle, vocab, rows, binary=False):
    """the word of every row: its first neighbour among the vocabulary's rows"""
    if len(rows) == 0:
        return np.zeros(0, np.int64)
    idx, _ = oracle.knn2(vocab, rows, binary=binary)
    return idx[:, 0].astype(np.int64)


def signatures(oracle, vocab, descs, binary=False):
    return np.stack([np.bincount(words_of(oracle, vocab, d, binary), minlength=len(vocab)).astype(np.uint32) for d in descs])


def scores(hist):
    h = hist.astype(np.int64)
    s = np.minimum(h[:, None, :], h[None, :, :]).sum(axis=2)
    np.fill_diagonal(s, 0)
    return s.astype(np.uint32)


def key(s, ni, nj):
    return (int(s) << 32) // min(int(ni), int(nj))


def rank(i, s, ns, ids, order_by=None):
    """the candidates of listed view i (list indices), best first: key descending, view id ascending.  order_by: another figure of
    merit with the signature of key (the tests show that raw s and a float32 division rank otherwise)"""
    f = order_by or key
    if ns[i] == 0:
        return []
    cand = [j for j in range(len(ns)) if j != i and ns[j] > 0]
    return sorted(cand, key=lambda j: (-f(s[i, j], ns[i], ns[j]), int(ids[j])))


def propose(s, ns, ids, top_k, order_by=None):
    out = set()
    for i in range(len(ns)):
        for j in rank(i, s, ns, ids, order_by)[:top_k]:
            out.add((min(int(ids[i]), int(ids[j])), max(int(ids[i]), int(ids[j]))))
    return np.array(sorted(out), np.uint32).reshape(-1, 2)


def restrict_graph(pairs, offsets, matches, keep_pairs):
    """(pairs, counts, matches) of a match graph restricted to the pairs listed in keep_pairs"""
    keep = {(int(a), int(b)) for a, b in keep_pairs}
    cnt = np.diff(np.asarray(offsets).astype(np.int64))
    sel = [p for p in range(len(pairs)) if (int(pairs[p][0]), int(pairs[p][1])) in keep]
    m = [np.asarray(matches)[int(offsets[p]):int(offsets[p + 1])] for p in sel]
    return (np.asarray(pairs)[sel].reshape(-1, 2), cnt[sel],
            np.concatenate(m).reshape(-1, 2) if m else np.zeros((0, 2), np.uint32))
