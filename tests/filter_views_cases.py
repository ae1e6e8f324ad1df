"""What the CPU restatement (oracle/acransac.c) gives on a filter_audit.Collection, pair by pair, and the audit of such results.

TEST INFRASTRUCTURE ONLY, shared by test_filter_audit.py (CPU) and test_gpu_filter_views.py.  The oracle is called per pair with the
pair's view IDS (they seed its sample stream), the sizes of the two views and their pinhole matrices."""
from __future__ import annotations

import numpy as np

import filter_audit as A


def expected(oracle, col: A.Collection, kind: str, precision_px=4.0, max_iter=2048, seed=5489, min_count=50, min_ratio=0.3):
    """one entry per pair row: None where the pair is not estimated (too short, or E without both pinhole matrices), else
    {"inliers" (rows of the putative list, AC-RANSAC's order), "model" [9], "threshold", "nfa", "iterations", "models", "n_inliers",
    "kept": accepted by the > 2.5 SS rule and, for E, by Regard3D's overlap rule}"""
    out = []
    for p in range(len(col.pairs)):
        I, J, mm, xI, xJ = col.putatives(p)
        wI, hI, wJ, hJ = col.sizes(p)
        KI, KJ = col.views[I]["K"], col.views[J]["K"]
        if len(mm) <= A.SS[kind] or (kind == "E" and (KI is None or KJ is None)):
            out.append(None)
            continue
        if kind == "E":
            inl, fr = oracle.acransac_E(xI, xJ, wI, hI, wJ, hJ, KI, KJ, precision_px, max_iter, seed, I, J)
        else:
            fn = oracle.acransac_F if kind == "F" else oracle.acransac_H
            inl, fr = fn(xI, xJ, wI, hI, wJ, hJ, precision_px, max_iter, seed, I, J)
        kept = bool(fr.accepted)
        if kept and kind == "E" and (len(inl) < min_count or np.float32(len(inl)) / np.float32(len(mm)) < np.float32(min_ratio)):
            kept = False
        out.append(dict(inliers=inl.astype(np.int64), model=np.array(list(fr.F)), threshold=float(fr.threshold), nfa=float(fr.nfa),
                        iterations=int(fr.n_iter), models=int(fr.n_models), n_inliers=int(fr.n_inliers), kept=kept))
    return out


def audit_pair(col: A.Collection, kind: str, p: int, precision_px, model, inliers, threshold, nfa, swap_sizes=False, swap_K=False,
               transpose=False):
    """filter_audit.audit of pair row p with the sizes and pinhole matrices of ITS views; the three switches audit a deliberately wrong
    reading instead (sizes of I and J exchanged, K_I and K_J exchanged, the model transposed: the roles of I and J exchanged)"""
    I, J, _, xI, xJ = col.putatives(p)
    wI, hI, wJ, hJ = col.sizes(p)
    KI, KJ = col.views[I]["K"], col.views[J]["K"]
    if swap_sizes:
        wI, hI, wJ, hJ = wJ, hJ, wI, hI
    if swap_K:
        KI, KJ = KJ, KI
    M = np.asarray(model, np.float64).reshape(3, 3)
    return A.audit(kind, xI, xJ, (wI, hI, wJ, hJ), precision_px, M.T if transpose else M, inliers, threshold, nfa, KI, KJ)


def rows_of(mm: np.ndarray, kept: np.ndarray) -> np.ndarray:
    """the rows of the putative list mm [m, 2] that the matches kept [k, 2] are (every (i, j) of a putative list is distinct)"""
    where = {(int(i), int(j)): r for r, (i, j) in enumerate(mm)}
    return np.array([where[(int(i), int(j))] for i, j in kept], np.int64)
