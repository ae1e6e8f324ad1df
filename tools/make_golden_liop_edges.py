"""Generates tests/golden/liop_edge_ref.npz (run in the authoring container, needs the reference tree for oracle/_ref/libref_liop.so).

For every patch family of tests/liop_cases.py: the descriptors the REFERENCE's own r3d_vl_liopdesc_process (vl_liop.c, compiled
where it lies) makes of the family's patches.  Data only -- no reference source, and no patches: those are regenerated from seeds.

A LIOP descriptor is an integer vote histogram divided by its float norm, so a family is stored as <name>_hist (u16), <name>_norm (f32)
and <name>_crc (CRC-32 of the patches the descriptors were made from); the loader rebuilds the floats with one IEEE division per bin.
This script asserts that the rebuilt rows equal the reference-built rows BIT FOR BIT before it writes anything.
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from oracle import pyoracle as O
import liop_cases as L

O.build()
assert O.ref_liop_lib() is not None, "oracle/_ref not built: needs the reference tree"
out = {}
for name in L.PATCH_FAMILIES:
    P = L.patches_of(name)
    ref = O.ref_liop(P)                                    # the reference's own descriptor routine
    votes = O.liop_votes(P)                                # the restatement's votes: only a (histogram, norm) pair that reproduces ref is stored
    assert (votes == np.rint(votes)).all() and votes.min() >= 0 and votes.max() < 65536
    desc, norm = L.normalise(votes)
    assert np.array_equal(desc.view(np.uint32), ref.view(np.uint32)), f"{name}: votes / norm do not reproduce the reference's descriptors"
    hist = votes.astype(np.uint16)
    assert np.array_equal(L.desc_from(hist, norm).view(np.uint32), ref.view(np.uint32))
    out[name + "_hist"] = hist; out[name + "_norm"] = norm; out[name + "_crc"] = np.uint32(L.crc(P))
    print(f"{name:15s} {len(P):4d} patches, {int((hist.sum(1) == 0).sum())} all-zero descriptors")
path = os.path.join(ROOT, "tests", "golden", "liop_edge_ref.npz")
np.savez_compressed(path, **out)
print("liop_edge_ref.npz:", os.path.getsize(path), "bytes")
