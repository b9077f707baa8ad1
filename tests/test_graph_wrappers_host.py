"""The graph operations' host-array wrappers have one body per family in the Python package and in
the C++ header: a private helper holds it, and each public function is a call of that helper that
names its own rpt_*_host entry point (no GPU)."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# public function -> the one _host entry point it names, per family
BUILD = {"knnGraph": "rpt_knn_graph_host", "knnGraphMetric": "rpt_knn_graph_metric_host",
         "knnGraphSV": "rpt_knn_graph_csr_host", "knnGraphMetricSV": "rpt_knn_graph_csr_metric_host"}
REFINE = {"knnGraphRefine": "rpt_knn_graph_refine_host", "knnGraphRefineMetric": "rpt_knn_graph_refine_metric_host",
          "knnGraphRefineSV": "rpt_knn_graph_refine_csr_host",
          "knnGraphRefineMetricSV": "rpt_knn_graph_refine_csr_metric_host"}
SEARCH = {"graphSearch": "rpt_graph_search_host", "graphSearchSV": "rpt_graph_search_csr_host",
          "graphSearchMetricSV": "rpt_graph_search_csr_metric_host"}
FAMILIES = (("_knn_graph", BUILD), ("_knn_graph_refine", REFINE), ("_graph_search", SEARCH))


def test_each_python_helper_is_defined_once():
    import rptree_amd as rp
    text = inspect.getsource(rp)
    for helper in ("_knn_graph", "_knn_graph_refine", "_graph_search", "_graph_prepare"):
        assert len(re.findall(r"^def %s\(" % helper, text, flags=re.M)) == 1, helper
        assert callable(getattr(rp, helper))


def test_python_wrappers_name_their_own_entry_point_and_hold_no_body():
    import rptree_amd as rp
    assert sum(len(names) for _, names in FAMILIES) == 11
    for helper, names in FAMILIES:
        for fn, entry in names.items():
            src = inspect.getsource(getattr(rp, fn))
            assert set(re.findall(r"\brpt_\w+_host\b", src)) == {entry}, fn
            assert "lib().%s," % entry in src, fn                      # in the code, not only in the docstring
            assert len(re.findall(r"\b%s\(" % helper, src)) == 1, fn
            # none of the moved body: no allocation, no array adoption, no check, no call of its own
            for word in ("np.empty(", "np.array(", "np.ascontiguousarray(", "ValueError", "check(", "_vp("):
                assert word not in src, (fn, word)


def test_cpp_header_names_each_entry_point_once():
    hpp = open(os.path.join(ROOT, "rp-tree_amd", "host", "rptree.hpp")).read()
    code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", hpp, flags=re.S))
    for names in (BUILD, REFINE, SEARCH):
        for entry in names.values():
            assert len(re.findall(r"\b%s\b" % entry, code)) == 1, entry
    for via in ("knnGraphVia", "knnGraphRefineVia", "graphSearchVia", "graphPrepareVia", "forestSeeds"):
        assert len(re.findall(r"^inline \S+ %s\(" % via, code, flags=re.M)) == 1, via
