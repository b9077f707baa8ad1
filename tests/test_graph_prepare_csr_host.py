"""The search-graph preparation on SVector (CSR) rows (rpt_graph_prepare_csr_*) is declared at every
layer, shares the reverse lists, the merge and the keep rule with the dense path, and is worth what
the README says on the sparse golden rows: recall of the beam search on the prepared graph against
the raw one, with the restatements (no GPU)."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_graph_csr_ref as cref  # noqa: E402
import knn_graph_metric_ref as mref  # noqa: E402
import graph_search_ref as sref  # noqa: E402
import graph_search_csr_ref as scref  # noqa: E402
import graph_prepare_ref as pref  # noqa: E402

HEADER = open(os.path.join(ROOT, "include", "rptree_hip.h")).read()
CSRC = os.path.join(ROOT, "rp-tree_amd", "csrc")


def _decl(name):
    m = re.search(r"int32_t\s+%s\s*\(([^;]*)\)\s*;" % name, HEADER)
    assert m, name
    return re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)


def _words(decl):
    return [re.sub(r"\s+", " ", a.strip()) for a in decl.split(",")]


def test_header_declares_the_entry_points():
    dev = _words(_decl("rpt_graph_prepare_csr_dev"))
    assert dev == _words(_decl("rpt_graph_prepare_dev")) and len(dev) == 12 and "int32_t metric" in dev
    host = _words(_decl("rpt_graph_prepare_csr_host"))
    assert host == _words(_decl("rpt_graph_prepare_host")) == [w.replace("_dev", "_host") for w in dev]
    assert re.search(r"#define\s+RPT_ABI_VERSION\s+1\b", HEADER)
    comment = HEADER[HEADER.index("prepare the kNN graph for the search on SVector (CSR) rows"):
                     HEADER.index("int32_t rpt_graph_prepare_csr_dev")]
    flat = re.sub(r"\s*\n \*\s*", " ", comment)
    for phrase in ("absent columns are +0.0", "widened exactly", "a stored zero is a zero", "word for word",
                   "metricDDL2's left fold over dense(x_l), dense(x_m)", "no FMA", "one sqrt", "plain <",
                   "NaN behind every number", "id -1, distance +inf", "the three statistics",
                   "before anything is uploaded", "clamping a count to [0, k]", "RPT_E_NOMEM", "class 3",
                   "rpt_knn_last_*", "n = 0 and n = 1 valid", "rpt_graph_prepare_last serves both",
                   "any ascending superset of the union of the two supports", "bit-equal",
                   "0 < 0 is false", "RPT_E_UNSUPPORTED", "RPT_E_ARG", "names rpt_graph_prepare_*",
                   "at most 1536 entries", "graph_prepare_csr_resident", "no limit on a row's length or on d",
                   "stays in bounds and terminates", "keeps refusing CSR data"):
        assert phrase in flat, phrase
    options = HEADER[HEADER.index("Algorithm switches of a context"):HEADER.index("int32_t rpt_ctx_set_option")]
    assert "graph_prepare_csr_resident" in options
    api = open(os.path.join(CSRC, "api.hip")).read()
    assert '{"graph_prepare_csr_resident", &rpt_options::graph_prepare_csr_resident}' in api
    assert "int64_t graph_prepare_csr_resident = 0;" in open(os.path.join(CSRC, "common.h")).read()


def test_ctypes_table_and_python_mirror():
    import rptree_amd as rp
    from rptree_amd import _lib
    assert _lib.SYMBOLS["rpt_graph_prepare_csr_dev"] == _lib.SYMBOLS["rpt_graph_prepare_dev"]
    assert _lib.SYMBOLS["rpt_graph_prepare_csr_host"] == _lib.SYMBOLS["rpt_graph_prepare_host"]
    L = _lib.lib()
    for name in ("rpt_graph_prepare_csr_dev", "rpt_graph_prepare_csr_host"):
        assert hasattr(L, name), name
    for name in ("graphPrepareSV", "graphPrepareSVDev"):
        assert name in rp.__all__ and callable(getattr(rp, name))
    sv = inspect.signature(rp.graphPrepareSV).parameters
    assert list(sv) == ["graph", "data", "kout", "diversify", "reverse", "ctx"]
    assert [sv[p].default for p in ("kout", "diversify", "reverse", "ctx")] == [None, True, True, None]
    assert [p for p in inspect.signature(rp.graphPrepare).parameters if p != "metric"] == list(sv)
    assert [p for p in inspect.signature(rp.graphPrepareDev).parameters if p != "metric"] == list(
        inspect.signature(rp.graphPrepareSVDev).parameters)
    assert "graphPrepareSV" in rp.graphPrepareLast.__doc__


def test_other_layers_name_it():
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "graph_prepare_csr_resident" in readme and "graphPrepareSV" in readme
    assert "graph_prepare_csr_times" in readme
    assert "the missing preparation step" not in readme
    hpp = open(os.path.join(ROOT, "rp-tree_amd", "host", "rptree.hpp")).read()
    assert "rpt_graph_prepare_csr_host" in hpp and len(re.findall(r"\bgraphPrepareSV\(", hpp)) >= 2
    example = os.path.join(ROOT, "rp-tree_amd", "host", "example_graph_prepare_sparse.cpp")
    text = open(example).read()
    for word in ("knnGraphSV(", "graphPrepareSV(", "graphSearchSV(", "unionFold(", 'printf("ok\\n")'):
        assert word in text, word
    assert "example_graph_prepare_sparse" in open(os.path.join(ROOT, "rp-tree_amd", "host", "Makefile")).read()
    hs = open(os.path.join(ROOT, "haskell", "Data", "RPTree", "HIP.hs")).read()
    assert "graphPrepareSVHIP" in hs and "rpt_graph_prepare_csr_host" in hs
    assert "rpt_graph_prepare_csr_host" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "graph_diversify_csr_kernel" in design and "kResCap" in design
    assert os.path.exists(os.path.join(ROOT, "tools", "graph_prepare_csr_times.py"))
    assert "graph_prepare_csr_times.py" in open(os.path.join(ROOT, "tools", "README.md")).read()
    assert "graph_prepare_csr_times.json" in open(os.path.join(ROOT, "profiles", "README.md")).read()


def test_one_definition_of_what_the_two_kernels_share():
    """the reverse lists and the merge read only the graph: one definition each; the keep rule (ballots ->
    kept) is one device function that both diversify kernels call; the kernel bodies stay apart"""
    src = open(os.path.join(CSRC, "graph_prepare.hip")).read()
    dev = open(os.path.join(CSRC, "graph_dev.h")).read()
    assert len(re.findall(r"__global__[^;{]*\bprep_merge_kernel\(", src)) == 1
    assert len(re.findall(r"hipLaunchKernelGGL\(prep_merge_kernel,", src)) == 1
    for kern in ("rev_zero_kernel", "rev_degree_kernel", "rev_scan_kernel", "rev_fill_kernel"):
        assert len(re.findall(r"__global__[^;{]*\b%s\(" % kern, dev)) == 1, kern
        assert not re.search(r"__global__[^;{]*\b%s\(" % kern, src)
        assert len(re.findall(r"hipLaunchKernelGGL\(%s," % kern, src)) == 1, kern
    for fn in ("div_row", "div_keep", "div_store"):
        assert len(re.findall(r"__device__ __forceinline__ \w[\w ]* %s\(" % fn, src)) == 1, fn
        assert len(re.findall(r"\b%s\(" % fn, src)) == 3, fn       # the definition and a call per kernel
    assert src.count("om & kept") == 1                               # the serial rule itself
    assert len(re.findall(r"__global__[^;{]*\bgraph_diversify_kernel\(", src)) == 1
    assert len(re.findall(r"__global__[^;{]*\bgraph_diversify_csr_kernel\(", src)) == 1
    assert "template <class TV, int NA>" in src and "fold_step<kGraphL2>" in src
    assert re.search(r"constexpr int kResCap = 1536;", src)
    make = open(os.path.join(ROOT, "rp-tree_amd", "Makefile")).read()
    assert "csrc/graph_prepare.hip" in make and "-ffp-contract=off" in make


# ------------------------------------------------------------------ what the step is worth
@pytest.fixture(scope="module")
def golden():
    """the setup of test_graph_search_csr_host.py: the sparse golden rows, their exact 10-NN graph, 200
    stored rows with perturbed stored values as queries, 16 random seeds each"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "forest_sparse_600x12.npz"))
    csrX = (z["rowptr"], z["col"], z["val"], int(z["d"]))
    X = cref.densify(csrX)
    n = X.shape[0]
    rng = np.random.default_rng(2025)
    pick = rng.choice(n, 200, replace=False)
    rows = cref.rows_of(csrX)
    csrQ = cref.from_rows([(rows[i][0], rows[i][1] + 0.1 * rng.standard_normal(len(rows[i][1]))) for i in pick],
                          int(z["d"]))
    D = sref.query_matrix(X, cref.densify(csrQ), "l2")
    graph = cref.exact_graph(X, 10)
    seeds = np.stack([np.random.default_rng(qi).choice(n, 16, replace=False) for qi in range(200)]).astype(np.int32)
    truth = np.stack([np.lexsort((np.arange(n), D[i]))[:10] for i in range(200)])
    return csrX, csrQ, D, graph, mref.metric_matrix(X, "l2"), seeds, truth


def _recalls(golden, graph):
    csrX, csrQ, D, _, _, seeds, truth = golden
    out = []
    for ef in (10, 32, 64):
        (ids, _, _), _, _, _ = scref.graph_search_csr_ref(csrX, csrQ, graph[0], graph[2], seeds, 10, ef, D=D)
        hits = sum(len(set(ids[i].tolist()) & set(truth[i].tolist())) for i in range(len(truth)))
        out.append(hits / (10.0 * len(truth)))
    return out


def test_recall_of_the_prepared_graphs_on_the_golden_rows(golden):
    """recall@10 at ef 10 / 32 / 64, k = 10, L2.  Measured when the feature was written: raw 0.5090 /
    0.7740 / 0.8625; reverse, kout 20: 0.7650 / 0.9985 / 1.0000; diversify + reverse, kout 16: 0.6780
    / 0.9365 / 0.9950; diversify only, kout 10: 0.4080 / 0.6265 / 0.7395 (printed, not bounded: the
    expected cost of diversifying without the reverse union)"""
    graph, PD = golden[3], golden[4]
    raw = _recalls(golden, graph)
    rev, rst = pref.graph_prepare_ref(graph, PD, 20, pref.REVERSE)
    both, bst = pref.graph_prepare_ref(graph, PD, 16, pref.DIVERSIFY | pref.REVERSE)
    div, dst = pref.graph_prepare_ref(graph, PD, 10, pref.DIVERSIFY)
    r_rev, r_both, r_div = _recalls(golden, rev), _recalls(golden, both), _recalls(golden, div)
    for name, g, r, st in (("raw", graph, raw, None), ("reverse, kout 20", rev, r_rev, rst),
                           ("diversify + reverse, kout 16", both, r_both, bst),
                           ("diversify only, kout 10", div, r_div, dst)):
        print("%-30s mean degree %5.2f  recall@10 %s at ef 10 / 32 / 64  stats %s"
              % (name, float(np.mean(g[2])), ["%.4f" % x for x in r], st))
    assert r_rev[1] >= 0.95 and r_rev[2] > raw[2]
    assert r_both[2] >= 0.95
    assert rst[0] == 0 and rst[1] == 0 and bst[0] == dst[0] == 600 * 45 and bst[1] == dst[1] > 0
