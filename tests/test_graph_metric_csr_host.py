"""The graph search and the graph preparation on SVector (CSR) rows under the cosine and inner-product
distances (rpt_graph_search_csr_metric_*, rpt_graph_prepare_csr_metric_*) are declared at every layer;
the dotS distance matrices the GPU tests hand to the restatements equal the dense ones for finite
values and do NOT with a stored inf or NaN; and the restatement searches a sparse graph as a beam
search should (no GPU)."""
import ast
import inspect
import os
import re
import shutil
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graph_metric_csr_ref as gm  # noqa: E402
from test_knn_graph_metric_csr_host import awkward_set  # noqa: E402

HEADER = open(os.path.join(ROOT, "include", "rptree_hip.h")).read()
NAMES = ("rpt_graph_search_csr_metric_dev", "rpt_graph_search_csr_metric_host",
         "rpt_graph_prepare_csr_metric_dev", "rpt_graph_prepare_csr_metric_host")


def _decl(name):
    m = re.search(r"int32_t\s+%s\s*\(([^;]*)\)\s*;" % name, HEADER)
    assert m, name
    return re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)


def _words(decl):
    return [re.sub(r"\s+", " ", a.strip()) for a in decl.split(",")]


def test_header_declares_the_entry_points():
    sdev = _words(_decl("rpt_graph_search_csr_metric_dev"))
    assert sdev == ["rpt_ctx* ctx", "const rpt_dataset* data", "const rpt_dataset* queries", "int32_t kg",
                    "const int32_t* gids_dev", "const int32_t* gcount_dev", "int32_t s", "const int32_t* seeds_dev",
                    "int32_t k", "int32_t ef", "int32_t metric", "int32_t flags", "int32_t* ids_dev",
                    "double* dist_dev", "int32_t* count_dev"]
    pdev = _words(_decl("rpt_graph_prepare_csr_metric_dev"))
    assert pdev == ["rpt_ctx* ctx", "const rpt_dataset* data", "int32_t k", "const int32_t* ids_dev",
                    "const double* dist_dev", "const int32_t* count_dev", "int32_t kout", "int32_t metric",
                    "int32_t flags", "int32_t* out_ids_dev", "double* out_dist_dev", "int32_t* out_count_dev"]
    for stage in ("search", "prepare"):
        for end in ("dev", "host"):
            new = _words(_decl("rpt_graph_%s_csr_metric_%s" % (stage, end)))
            assert new == _words(_decl("rpt_graph_%s_csr_%s" % (stage, end))), (stage, end)
            assert new == _words(_decl("rpt_graph_%s_%s" % (stage, end))), (stage, end)
    assert re.search(r"#define\s+RPT_ABI_VERSION\s+1\b", HEADER)


def test_header_comment_states_the_definition():
    comment = HEADER[HEADER.index("query and prepare the kNN graph on SVector (CSR) rows, under cosine / inner product"):
                     HEADER.index("int32_t rpt_graph_search_csr_metric_dev")]
    flat = re.sub(r"\s*\n \*\s*", " ", comment)
    for phrase in ("the same parameter lists, word for word", "`metric` already stands before `flags`",
                   "rpt_knn_csr_metric_*", "rpt_knn_graph_csr_metric_*", "starts at +0.0",
                   "stored in BOTH rows in ascending column order", "acc = acc + x_c * y_c",
                   "every product and sum rounded on its own", "widened exactly", "no FMA",
                   "the bits of rpt_graph_search_csr_* / rpt_graph_prepare_csr_*", "-dotS(x, y)",
                   "1 - dotS(x, y) / (sqrt(dotS(x, x)) * sqrt(dotS(y, y)))", "on the query set",
                   "NaN ranks behind every number", "by id", "-0.0", "ties with +0.0", "plain <",
                   "only where both cursors stand on one column", "no tail", "inf * 0 = NaN",
                   "The answer is dotS in both cases", "80 928 B at k = 64", "by shuffle",
                   "rpt_graph_search_last and rpt_graph_prepare_last serve these calls too",
                   "graph_search_nofilter", "graph_search_csr_stream", "graph_prepare_csr_resident",
                   "rpt_prof_* class 3", "RPT_E_ARG", "RPT_E_UNSUPPORTED", "RPT_KNN_METRIC_REFERENCE",
                   "a metric bit in `flags` too", "Dense data", "an error leaves the context usable",
                   "right-fold innerSS", "in bounds, terminates"):
        assert phrase in flat, phrase
    # the L2 CSR entry points and the graph builders point at the new ones, and no longer call them not built
    for anchor, end in (("query the kNN graph on SVector (CSR) rows, under L2", "int32_t rpt_graph_search_csr_dev"),
                        ("prepare the kNN graph for the search on SVector (CSR) rows, under L2",
                         "int32_t rpt_graph_prepare_csr_dev")):
        text = HEADER[HEADER.index(anchor):HEADER.index(end)]
        assert "_csr_metric_*" in text and "RPT_E_UNSUPPORTED" in text
    built = HEADER[HEADER.index("on SVector (CSR) rows, under cosine / inner product"):
                   HEADER.index("int32_t rpt_knn_graph_csr_metric_dev")]
    flat = re.sub(r"\s*\n \*\s*", " ", built)
    assert "rpt_graph_prepare_csr_metric_* and rpt_graph_search_csr_metric_*" in flat
    assert "Not built: rpt_graph_search_csr_*" not in flat
    opts = HEADER[HEADER.index("Algorithm switches of a context"):HEADER.index("int32_t rpt_ctx_set_option")]
    assert "rpt_graph_search_csr_metric_*" in opts and "rpt_graph_prepare_csr_metric_*" in opts


def test_header_still_compiles_as_c99():
    gcc = shutil.which("gcc")
    assert gcc, "no gcc"
    pr = subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c",
                         os.path.join(ROOT, "include", "rptree_hip.h")], stdout=subprocess.PIPE,
                        stderr=subprocess.STDOUT)
    assert pr.returncode == 0, pr.stdout.decode()


def test_ctypes_table_and_python_mirror():
    import rptree_amd as rp
    from rptree_amd import _lib
    for name in NAMES:
        assert _lib.SYMBOLS[name] == _lib.SYMBOLS[name.replace("_csr_metric_", "_csr_")], name
        assert _lib.SYMBOLS[name] == _lib.SYMBOLS[name.replace("_csr_metric_", "_")], name
    declared = set(re.findall(r"^\s*(?:int32_t|const char\*)\s+(rpt_\w+)\s*\(", HEADER, flags=re.M))
    assert declared == set(_lib.SYMBOLS)
    for fn, l2, params in (
            (rp.graphSearchMetricSV, rp.graphSearchSV,
             ["distf", "graph", "data", "qs", "k", "ef", "seeds", "forest", "seed_k", "ctx"]),
            (rp.graphSearchMetricSVDev, rp.graphSearchSVDev,
             ["distf", "data", "queries", "kg", "gids_ptr", "gcount_ptr", "s", "seeds_ptr", "k", "ef", "ids_ptr",
              "dist_ptr", "count_ptr"]),
            (rp.graphPrepareMetricSV, rp.graphPrepareSV, ["distf", "graph", "data", "kout", "diversify", "reverse", "ctx"]),
            (rp.graphPrepareMetricSVDev, rp.graphPrepareSVDev,
             ["distf", "k", "data", "ids_ptr", "dist_ptr", "count_ptr", "kout", "out_ids_ptr", "out_dist_ptr",
              "out_count_ptr", "diversify", "reverse"])):
        assert fn.__name__ in rp.__all__ and callable(fn)
        assert list(inspect.signature(fn).parameters) == params
        # distf in front of the L2 function's own parameters, defaults included
        assert str(inspect.signature(fn)) == str(inspect.signature(l2)).replace("(", "(distf, ", 1)
        assert "metric" not in inspect.signature(l2).parameters
    assert str(inspect.signature(rp.graphSearchMetricSV)) == \
        "(distf, graph, data, qs, k, ef=None, seeds=None, forest=None, seed_k=8, ctx=None)"
    assert str(inspect.signature(rp.graphPrepareMetricSV)) == \
        "(distf, graph, data, kout=None, diversify=True, reverse=True, ctx=None)"
    # the dense functions say where CSR rows go
    assert "graphSearchMetricSV" in rp.graphSearch.__doc__ and "graphPrepareMetricSV" in rp.graphPrepare.__doc__
    # the seeds a forest gives are taken under distf: the shared body hands seed_metric to knnBatch, and
    # graphSearchMetricSV's one call of it binds distf there (and its own entry point to `entry`)
    assert re.search(r"knnBatch\(int\(seed_k\), forest, qd, dedup=True, metric=seed_metric\)",
                     inspect.getsource(rp._graph_search))
    src = inspect.getsource(rp.graphSearchMetricSV)
    assert "rpt_graph_search_csr_metric_host" in src
    calls = [c for c in ast.walk(ast.parse(src)) if isinstance(c, ast.Call) and
             isinstance(c.func, ast.Name) and c.func.id == "_graph_search"]
    assert len(calls) == 1 and not calls[0].keywords
    bound = dict(zip(inspect.signature(rp._graph_search).parameters, calls[0].args))
    assert ast.unparse(bound["seed_metric"]) == "distf"
    assert ast.unparse(bound["metric_flag"]) == "_metric_flag(distf)"
    assert ast.unparse(bound["entry"]) == "lib().rpt_graph_search_csr_metric_host"
    assert "rpt_graph_prepare_csr_metric_host" in inspect.getsource(rp.graphPrepareMetricSV)


def test_library_exports_them():
    from rptree_amd import _lib
    L = _lib.lib()
    for name in NAMES:
        assert hasattr(L, name), name


def test_kernel_source_instantiates_the_existing_kernels():
    csrc = os.path.join(ROOT, "rp-tree_amd", "csrc")
    search = open(os.path.join(csrc, "graph_search_csr.hip")).read()
    prep = open(os.path.join(csrc, "graph_prepare.hip")).read()
    api = open(os.path.join(csrc, "api.hip")).read()
    # one body per kernel, instantiated on the distance
    assert len(re.findall(r"template <class TV, int M>\s*__global__[^;{]*\bgraph_search_csr_kernel\(", search)) == 1
    assert len(re.findall(r"template <class TV, int M, int NA>\s*__global__[^;{]*\bgraph_diversify_csr_kernel\(",
                          prep)) == 1
    assert len(re.findall(r"\bdouble merge_piece\(", search)) == 1 and len(re.findall(r"\bdouble pair_fold\(", prep)) == 1
    for word in ("merge_piece<TV, M>", "fold_step<M>", "fold_finish<M>(acc, qnorm, nrm)", "fold_step<kGraphL2>",
                 "kGraphCosine", "kGraphInner", "a.qn[qi]", "a.rn[my]", "ensure_sqnorm(ctx, data)",
                 "ensure_sqnorm(ctx, queries)", "__ballot(w.jp < w.je)", "constexpr int kQCap = 2048;"):
        assert word in search, word
    for word in ("pair_fold<M>(LdsRows{ec, ev}", "pair_fold<M>(GlobalRows<TV>{col, val}", "fold_step<M>",
                 "fold_finish<M>(acc, n_l, n_m) < sd[m]", "__shfl(nrm, l)", "__shfl(nrm, m)",
                 "constexpr int kResCap = 1536;", "80 928 B at k = 64", "82 976 B", "81 920 B"):
        assert word in prep, word
    # the norms of the cosine preparation take no LDS: the per-wave layout is the L2 kernel's
    assert "(cap + 2 * k + na + 1) * 8 + (size_t)(cap + 2 * k) * 4" in prep
    k, cap, na = 64, 1536, 32
    assert 4 * (((cap + 2 * k + na + 1) * 8 + (cap + 2 * k) * 4 + 7) & ~7) == 80928 <= 81920
    for name in NAMES:
        assert re.search(r"int32_t %s\(" % name, api), name
    # the old entry points keep refusing a metric and name the new ones; so do the dense ones
    assert "the graph search on CSR rows is built under metricL2 only" in api
    assert "the graph preparation on CSR rows is built under metricL2 only" in api
    assert api.count("rpt_graph_search_csr_metric_*") >= 3 and api.count("rpt_graph_prepare_csr_metric_*") >= 3


def test_other_layers_name_it():
    hpp = open(os.path.join(ROOT, "rp-tree_amd", "host", "rptree.hpp")).read()
    assert "rpt_graph_search_csr_metric_host" in hpp and "rpt_graph_prepare_csr_metric_host" in hpp
    assert re.search(r"KnnResult graphSearchSV\(Context& ctx, const Dataset& data, const GraphResult& g,\s*"
                     r"const Dataset& qs,\s*Metric metric", hpp)
    assert re.search(r"GraphResult graphPrepareSV\(Context& ctx, const Dataset& data, const GraphResult& g,\s*"
                     r"Metric metric", hpp)
    host = os.path.join(ROOT, "rp-tree_amd", "host")
    assert os.path.exists(os.path.join(host, "example_graph_search_sparse_metric.cpp"))
    assert "example_graph_search_sparse_metric" in open(os.path.join(host, "Makefile")).read()
    assert "example_graph_search_sparse_metric" in open(os.path.join(ROOT, ".gitignore")).read()
    hs = open(os.path.join(ROOT, "haskell", "Data", "RPTree", "HIP.hs")).read()
    for word in ("graphSearchMetricSVHIP", "graphPrepareMetricSVHIP", "rpt_graph_search_csr_metric_host",
                 "rpt_graph_prepare_csr_metric_host"):
        assert word in hs, word
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "rpt_graph_search_csr_metric_host" in integ and "rpt_graph_prepare_csr_metric_host" in integ
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "graphSearchMetricSV" in readme and "graphPrepareMetricSV" in readme
    assert "Not built: graph search and graph preparation on CSR rows under these distances" not in readme
    assert "graph_metric_csr_times.py" in readme
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "rpt_graph_search_csr_metric" in design and "rpt_graph_prepare_csr_metric" in design
    assert "the search and the preparation on SVector rows stay L2 only" not in design
    assert "graph_metric_csr_times.py" in open(os.path.join(ROOT, "tools", "README.md")).read()
    assert "graph_metric_csr_times.json" in open(os.path.join(ROOT, "profiles", "README.md")).read()
    assert os.path.exists(os.path.join(ROOT, "tools", "graph_metric_csr_times.py"))


# ------------------------------------------------------------------ the distance matrices, in numpy
def awkward_queries(bad=False):
    """40 x 70 queries: empty ones, stored rows of awkward_set themselves, stored +0.0 and -0.0, a full
    query, f32-rounded values, queries scaled by 10; bad: two also store an inf and a NaN"""
    rows = [(c.copy(), v.copy()) for c, v in gm.rows_of(gm.make_csr(43, 40, 70, 0.15))]
    stored = gm.rows_of(awkward_set())
    rows[0] = (np.zeros(0, dtype=np.int32), np.zeros(0))
    rows[1], rows[2], rows[3] = stored[17], stored[20], stored[22]
    rows[4] = (np.array([69], dtype=np.int32), np.array([-0.0]))
    rows[5] = (np.array([0, 7, 69], dtype=np.int32), np.array([-0.0, 2.5, 0.0]))
    for i in range(10, 20):
        rows[i] = (rows[i][0], rows[i][1].astype(np.float32).astype(np.float64))
    for i in range(20, 25):
        rows[i] = (rows[i][0], rows[i][1] * 10.0)
    if bad:
        rows[30] = (rows[30][0], np.concatenate([[np.inf], rows[30][1][1:]]))
        rows[31] = (rows[31][0], np.concatenate([rows[31][1][:-1], [np.nan]]))
        assert len(rows[30][0]) > 1 and len(rows[31][0]) > 1
    return gm.from_rows(rows, 70)


def test_dotS_matrices_equal_the_dense_ones_for_finite_values():
    """all 40 x 200 query-row pairs and all 200 x 200 row pairs: the D handed to graph_search_ref and
    graph_prepare_ref is the dense metric matrix of the dense-ified rows bit for bit, which is why the
    GPU tests may compare with rp.graphSearch(metric=) / rp.graphPrepare(metric=) there"""
    csrX, csrQ = awkward_set(), awkward_queries()
    for metric in gm.METRICS:
        DQ = gm.query_matrix(csrX, csrQ, metric)
        assert DQ.shape == (40, 200)
        assert np.array_equal(gm.bits(DQ), gm.bits(gm.dense_query_matrix(csrX, csrQ, metric))), metric
        DX = gm.rows_matrix(csrX, metric)
        assert DX.shape == (200, 200)
        assert np.array_equal(gm.bits(DX), gm.bits(gm.dense_rows_matrix(csrX, metric))), metric
        assert np.array_equal(gm.bits(DX), gm.bits(DX.T)), metric
        # a stored row as a query: its column of DQ is its row of DX
        assert np.array_equal(gm.bits(DQ[1]), gm.bits(DX[17])) and np.array_equal(gm.bits(DQ[3]), gm.bits(DX[22]))
        if metric == "cosine":
            assert np.isnan(DQ[0]).all() and np.isnan(DQ[4]).all() and np.isnan(DQ[:, 13]).all()
        else:
            assert np.all(DQ[0] == 0.0) and np.signbit(DQ[0]).all()       # an empty query: -0.0 from every row
    # the two-pointer merge the kernels run gives the same sums
    X, Q = gm.rows_of(csrX), gm.rows_of(csrQ)
    G = -gm.query_matrix(csrX, csrQ, "inner")
    got = np.array([[gm.mc.dot_pair(cq, vq, cx, vx) for cx, vx in X] for cq, vq in Q])
    assert np.array_equal(gm.bits(got), gm.bits(G))


def test_dotS_matrices_differ_from_the_dense_ones_with_a_stored_inf_or_nan():
    """the same sets with an inf and a NaN stored in two rows and in two queries: the dense fold meets
    inf * 0 = NaN where dotS takes no product, so the GPU tests hold those cases to dotS alone"""
    csrX, csrQ = awkward_set(bad=True), awkward_queries(bad=True)
    for metric in gm.METRICS:
        DQ, ZQ = gm.query_matrix(csrX, csrQ, metric), gm.dense_query_matrix(csrX, csrQ, metric)
        differ = gm.bits(DQ) != gm.bits(ZQ)
        assert differ[30].any() and differ[:, 30].any(), metric
        # a stored NaN makes the norm NaN, so the cosine is NaN either way; the inner product tells them apart
        assert (differ[31].any() and differ[:, 31].any()) == (metric == "inner"), metric
        fine_q = [i for i in range(40) if i not in (30, 31)]
        fine_x = [i for i in range(200) if i not in (30, 31)]
        assert not differ[np.ix_(fine_q, fine_x)].any(), metric
        DX, ZX = gm.rows_matrix(csrX, metric), gm.dense_rows_matrix(csrX, metric)
        differ = gm.bits(DX) != gm.bits(ZX)
        assert differ[30].any() and differ[31].any() == (metric == "inner"), metric
        assert not differ[np.ix_(fine_x, fine_x)].any(), metric


# ------------------------------------------------------------------ the restatement on a small sparse set
def test_recall_grows_with_ef_and_the_reverse_union_does_not_lower_it():
    """the sparse golden rows (600 x 12), the exact 10-NN graph under each distance, 200 perturbed stored
    rows as queries, 16 random seeds: recall@10 against the exact answer does not fall from ef = 10 to
    32 to 64, on the raw graph and on its reverse union (kout 20), and the reverse union does not
    lower it at ef = 32"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "forest_sparse_600x12.npz"))
    csr = (z["rowptr"], z["col"], z["val"], int(z["d"]))
    n, k = int(z["n"]), 10
    rng = np.random.default_rng(2024)
    rows = gm.rows_of(csr)
    full = np.flatnonzero(np.diff(z["rowptr"]) > 0)
    pick = rng.choice(full, size=200, replace=False)
    csrQ = gm.from_rows([(rows[i][0], rows[i][1] + 0.1 * rng.standard_normal(len(rows[i][1]))) for i in pick], csr[3])
    seeds = rng.integers(0, n, size=(200, 16)).astype(np.int32)
    for metric in gm.METRICS:
        DX, DQ = gm.rows_matrix(csr, metric), gm.query_matrix(csr, csrQ, metric)
        truth = np.stack([gm.sref.order_of(DQ[i], np.arange(n))[:k] for i in range(200)])
        raw = gm.exact_graph(DX, k)
        union, _ = gm.graph_prepare_ref(raw, csr, 20, gm.REVERSE, metric, D=DX)
        recall = {}
        for name, g in (("raw", raw), ("reverse union", union)):
            for ef in (10, 32, 64):
                (ids, _, cnt), _, _, _ = gm.graph_search_ref(csr, csrQ, g[0], g[2], seeds, k, ef, metric, D=DQ)
                assert np.all(cnt == k)
                recall[name, ef] = np.mean([len(set(ids[i]) & set(truth[i])) / k for i in range(200)])
            print("sparse 600 x 12, %s, %s graph: recall@10 at ef 10 / 32 / 64: %s"
                  % (metric, name, " / ".join("%.3f" % recall[name, ef] for ef in (10, 32, 64))))
            assert recall[name, 10] <= recall[name, 32] <= recall[name, 64], (metric, name, recall)
        assert recall["reverse union", 32] >= recall["raw", 32], (metric, recall)
