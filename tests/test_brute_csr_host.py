"""The brute force over CSR rows and the batched recallWith are declared at every layer (no GPU):
the C header, the ctypes table, the Python and C++ mirrors, the option's documentation."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "rptree_hip.h")).read()


def _decl(name):
    m = re.search(r"int32_t\s+%s\s*\(([^;]*)\)\s*;" % name, HEADER)
    assert m, name
    return re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)


def test_header_declares_the_new_entry_points():
    dev = _decl("rpt_brute_knn_dev")
    assert dev.count(",") == 6 and "ids_dev" in dev and "dist_dev" in dev and "flags" in dev
    rec = _decl("rpt_recall_hits_host")
    assert rec.count(",") == 7
    for word in ("rpt_forest*", "hits_host", "truth_ids_host", "flags"):
        assert word in rec
    # the reference lines the entry point replaces, and the CSR rules of the brute force
    assert "RPTree.hs:259-282" in HEADER and "Internal.hs:389-393" in HEADER
    assert "RPT_KNN_METRIC_COSINE / _INNER on CSR data: RPT_E_UNSUPPORTED" in HEADER


def test_ctypes_table_has_them():
    from rptree_amd import _lib
    assert len(_lib.SYMBOLS["rpt_brute_knn_dev"][1]) == 7
    assert len(_lib.SYMBOLS["rpt_recall_hits_host"][1]) == 8
    declared = set(re.findall(r"^\s*(?:int32_t|const char\*)\s+(rpt_\w+)\s*\(", HEADER, flags=re.M))
    assert declared == set(_lib.SYMBOLS)


def test_python_mirror_exports():
    import inspect

    import rptree_amd as rp
    for name in ("recallWithBatch", "recallHits", "recallWith", "bruteKnn"):
        assert name in rp.__all__ and callable(getattr(rp, name))
    assert list(inspect.signature(rp.recallWithBatch).parameters) == ["distf", "forest", "k", "qs",
                                                                     "reference_metric"]
    assert inspect.signature(rp.recallWith).parameters["reference_metric"].default is False
    assert inspect.signature(rp.bruteKnn).parameters["reference_metric"].default is False


def test_option_is_documented():
    comment = HEADER[HEADER.index("Algorithm switches of a context"):HEADER.index("int32_t rpt_ctx_set_option")]
    assert "brute_csr_tile" in comment
    assert "brute_csr_tile" in open(os.path.join(ROOT, "README.md")).read()
    api = open(os.path.join(ROOT, "rp-tree_amd", "csrc", "api.hip")).read()
    assert '{"brute_csr_tile", &rpt_options::brute_csr_tile}' in api


def test_cpp_mirror_and_example():
    hpp = open(os.path.join(ROOT, "rp-tree_amd", "host", "rptree.hpp")).read()
    for name in ("bruteKnn", "recallHits", "recallWithBatch", "recallWith", "rpt_recall_hits_host"):
        assert name in hpp
    assert os.path.exists(os.path.join(ROOT, "rp-tree_amd", "host", "example_sparse_recall.cpp"))
