"""The layout of the kernel sources: a translation unit is one thing.  No file includes a .hip file, and the
macros under which kernels_filter.hip used to be compiled three times, with the switches of the essential-matrix bisect, stay gone.
No file includes one text twice, and the bodies the KGraph, HNSW and MRPT searches used to include once per tail stay gone (section 4.22).
A plain text search."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "regard3d_amd", "csrc")
TOOLS = os.path.join(ROOT, "tools")
RETIRED = ("R3DM_FILTER_ONLY_E", "R3DM_FILTER_DEVICE_ONLY", "R3DM_BISECT_")
RETIRED_SEARCH = ("R3DM_ANN_KNN", "R3DM_HNSW_KNN", "R3DM_MRPT_KNN", "ann_search_body.inc", "hnsw_search_body.inc", "mrpt_query_body.inc")
RETIRED_SYMRATIO = ("l2_symratio_", "hamming_symratio_")      # the ratio forms are the RATIO instantiations of the mutual kernels
INCLUDES_HIP = re.compile(r'^[ \t]*#[ \t]*include[ \t]*["<][^">\n]*\.hip[">]', re.M)
INCLUDES = re.compile(r'^[ \t]*#[ \t]*include[ \t]*["<]([^">\n]*)[">]', re.M)


def _files(*tops):
    for top in tops:
        if os.path.isfile(top):
            yield top
        for d, _, names in os.walk(top):
            for n in names:
                yield os.path.join(d, n)


def _text(path):
    with open(path, "rb") as f:
        return f.read().decode("utf-8", "ignore")


def test_no_file_includes_a_hip_file():
    files = list(_files(CSRC, TOOLS))
    assert any(f.endswith("kernels_filter.hip") for f in files) and any(f.endswith("build_bisect.sh") for f in files)
    bad = [os.path.relpath(f, ROOT) for f in files if INCLUDES_HIP.search(_text(f))]
    assert not bad, f"these files include a .hip file: {bad}"


def test_no_file_includes_the_same_file_twice():
    """a text included twice under a macro is how the KGraph, HNSW and MRPT searches made their k-list kernels"""
    files = list(_files(CSRC))
    assert any(f.endswith("kernels_ann.hip") for f in files)
    bad = []
    for f in files:
        names = [os.path.basename(n) for n in INCLUDES.findall(_text(f))]
        bad += [(os.path.relpath(f, ROOT), n) for n in sorted(set(names)) if names.count(n) > 1]
    assert not bad, f"included more than once by one file: {bad}"


def test_retired_search_bodies_stay_gone():
    files = list(_files(CSRC, os.path.join(ROOT, "build.sh"), TOOLS))
    assert len(files) > 10
    bad = [(os.path.relpath(f, ROOT), s) for f in files for s in RETIRED_SEARCH if s in _text(f)]
    assert not bad, f"the macro-cut search bodies are back: {bad}"


def test_symmetric_ratio_has_no_kernels_of_its_own():
    files = list(_files(CSRC))
    assert any(f.endswith("kernels_match_mutual.hip") for f in files)
    bad = [(os.path.relpath(f, ROOT), s) for f in files for s in RETIRED_SYMRATIO if s in _text(f)]
    assert not bad, f"the copies of the mutual kernels are back: {bad}"


def test_retired_filter_macros_stay_gone():
    files = list(_files(CSRC, os.path.join(ROOT, "build.sh"), os.path.join(TOOLS, "build_bisect.sh")))
    assert len(files) > 10
    bad = [(os.path.relpath(f, ROOT), s) for f in files for s in RETIRED if s in _text(f)]
    assert not bad, f"retired macros are back: {bad}"
