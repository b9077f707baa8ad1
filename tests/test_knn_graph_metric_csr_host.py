"""The kNN graph and its NN-descent rounds on SVector (CSR) rows under the cosine and inner-product
distances (rpt_knn_graph_csr_metric_*, rpt_knn_graph_refine_csr_metric_*) are declared at every
layer; the zero-fill argument their leaf kernels rest on holds in numpy for finite values and FAILS
for a stored inf or NaN (which is why the presence-masked fold exists); and the restatement behaves
as NN-descent should on sparse rows (no GPU)."""
import inspect
import os
import re
import shutil
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_graph_metric_csr_ref as mc  # noqa: E402

HEADER = open(os.path.join(ROOT, "include", "rptree_hip.h")).read()
NAMES = ("rpt_knn_graph_csr_metric_dev", "rpt_knn_graph_csr_metric_host", "rpt_knn_graph_refine_csr_metric_dev",
         "rpt_knn_graph_refine_csr_metric_host")


def _decl(name):
    m = re.search(r"int32_t\s+%s\s*\(([^;]*)\)\s*;" % name, HEADER)
    assert m, name
    return re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)


def _words(decl):
    return [re.sub(r"\s+", " ", a.strip()) for a in decl.split(",")]


def test_header_declares_the_entry_points():
    dev = _words(_decl("rpt_knn_graph_csr_metric_dev"))
    assert dev == ["rpt_ctx* ctx", "rpt_forest* f", "const rpt_dataset* data", "int32_t k", "int32_t metric",
                   "int32_t flags", "int32_t* ids_dev", "double* dist_dev", "int32_t* count_dev"]
    assert dev == _words(_decl("rpt_knn_graph_metric_dev"))
    assert _words(_decl("rpt_knn_graph_csr_metric_host")) == _words(_decl("rpt_knn_graph_metric_host"))
    rdev = _words(_decl("rpt_knn_graph_refine_csr_metric_dev"))
    assert rdev == ["rpt_ctx* ctx", "const rpt_dataset* data", "int32_t k", "int32_t reverse", "int32_t iters",
                    "int32_t metric", "int32_t flags", "int32_t* ids_dev", "double* dist_dev", "int32_t* count_dev"]
    assert rdev == _words(_decl("rpt_knn_graph_refine_metric_dev"))
    assert _words(_decl("rpt_knn_graph_refine_csr_metric_host")) == _words(_decl("rpt_knn_graph_refine_metric_host"))
    # the L2 entry points keep their shape
    assert _words(_decl("rpt_knn_graph_csr_dev")) == _words(_decl("rpt_knn_graph_dev"))
    assert _words(_decl("rpt_knn_graph_refine_csr_dev")) == _words(_decl("rpt_knn_graph_refine_dev"))
    assert re.search(r"#define\s+RPT_ABI_VERSION\s+1\b", HEADER)


def test_header_comment_states_the_definition():
    comment = HEADER[HEADER.index("on SVector (CSR) rows, under cosine / inner product"):
                     HEADER.index("int32_t rpt_knn_graph_csr_metric_dev")]
    flat = re.sub(r"\s*\n \*\s*", " ", comment)
    for phrase in ("`metric` (before `flags`)", "word for word", "rpt_knn_csr_metric_*", "starts at +0.0",
                   "stored in BOTH rows in ascending column order", "acc = acc + x_c * y_c",
                   "every product and sum rounded on its own", "widened exactly", "no FMA",
                   "the bits of rpt_knn_graph_csr_* / rpt_knn_graph_refine_csr_*", "-dotS(x_i, x_j)",
                   "1 - dotS(x_i, x_j) / (sqrt(dotS(x_i, x_i)) * sqrt(dotS(x_j, x_j)))", "ranks last, by id",
                   "-0.0", "ties with +0.0", "symmetric bit for bit", "still evaluated once",
                   "inf * 0 = NaN", "dotS of {0: inf} and {1: 1.0} is +0.0", "never -0.0",
                   "The answer is dotS in both cases", "presence word", "graph_csr_masked",
                   "the answer does not depend on it", "RPT_GRAPH_ACCUMULATE", "rpt_knn_graph_last_pairs",
                   "rpt_knn_graph_refine_last", "graph_general", "graph_refine_general", "RPT_E_ARG",
                   "RPT_E_UNSUPPORTED", "streamed forest", "RPT_KNN_METRIC_REFERENCE", "Dense data",
                   "an error leaves the context usable", "rpt_graph_search_csr_*", "rpt_graph_prepare_csr_*",
                   "right-fold innerSS"):
        assert phrase in flat, phrase
    opts = HEADER[HEADER.index("Algorithm switches of a context"):HEADER.index("int32_t rpt_ctx_set_option")]
    assert "graph_csr_masked (0 / 1)" in opts


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
    for csr, dense in (("rpt_knn_graph_csr_metric_dev", "rpt_knn_graph_metric_dev"),
                       ("rpt_knn_graph_csr_metric_host", "rpt_knn_graph_metric_host"),
                       ("rpt_knn_graph_refine_csr_metric_dev", "rpt_knn_graph_refine_metric_dev"),
                       ("rpt_knn_graph_refine_csr_metric_host", "rpt_knn_graph_refine_metric_host")):
        assert _lib.SYMBOLS[csr] == _lib.SYMBOLS[dense]
    declared = set(re.findall(r"^\s*(?:int32_t|const char\*)\s+(rpt_\w+)\s*\(", HEADER, flags=re.M))
    assert declared == set(_lib.SYMBOLS)
    for sv, dense, params in (
            (rp.knnGraphMetricSV, rp.knnGraphMetric, ["distf", "k", "forest", "accumulate"]),
            (rp.knnGraphMetricSVDev, rp.knnGraphMetricDev,
             ["distf", "k", "forest", "ids_ptr", "dist_ptr", "count_ptr", "accumulate"]),
            (rp.knnGraphRefineMetricSV, rp.knnGraphRefineMetric, ["distf", "graph", "data", "iters", "reverse", "ctx"]),
            (rp.knnGraphRefineMetricSVDev, rp.knnGraphRefineMetricDev,
             ["distf", "k", "data", "ids_ptr", "dist_ptr", "count_ptr", "iters", "reverse"])):
        assert sv.__name__ in rp.__all__ and callable(sv)
        assert list(inspect.signature(sv).parameters) == params
        assert str(inspect.signature(sv)) == str(inspect.signature(dense))
    # the dense functions say where CSR rows go
    assert "knnGraphMetricSV" in rp.knnGraphMetric.__doc__
    assert "knnGraphRefineMetricSV" in rp.knnGraphRefineMetric.__doc__


def test_library_exports_them():
    from rptree_amd import _lib
    L = _lib.lib()
    for name in NAMES:
        assert hasattr(L, name), name


def test_kernel_source_instantiates_the_existing_kernels():
    csrc = os.path.join(ROOT, "rp-tree_amd", "csrc")
    src = open(os.path.join(csrc, "graph_csr.hip")).read()
    api = open(os.path.join(csrc, "api.hip")).read()
    # one body per kernel, instantiated on the distance
    for kern in ("graph_csr_leaf_kernel", "graph_csr_tiled_kernel", "refine_join_csr_kernel"):
        assert len(re.findall(r"template <class TV, int M>\s*__global__[^;{]*\b%s\(" % kern, src)) == 1, kern
    for word in ("fold_step<M>", "fold_finish<M>", "kGraphCosine", "kGraphInner", "tile_fold_masked<M>",
                 "masked_fold(stats, force_masked)", "graph_csr_masked", "ensure_sqnorm(ctx, data)", "wave_merge("):
        assert word in src, word
    assert '{"graph_csr_masked", &rpt_options::graph_csr_masked}' in api
    for name in NAMES:
        assert re.search(r"int32_t %s\(" % name, api), name
    # graph search and preparation on CSR rows keep refusing a metric
    assert "the graph search on CSR rows is built under metricL2 only" in api
    # the error text of the dense entry points names the CSR ones
    assert "rpt_knn_graph_csr_metric_*" in api and "rpt_knn_graph_refine_csr_metric_*" in api


def test_other_layers_name_it():
    hpp = open(os.path.join(ROOT, "rp-tree_amd", "host", "rptree.hpp")).read()
    assert "rpt_knn_graph_csr_metric_host" in hpp and "rpt_knn_graph_refine_csr_metric_host" in hpp
    assert re.search(r"GraphResult knnGraphSV\(const RPForest& tts, int k, Metric metric", hpp)
    assert re.search(r"GraphResult knnGraphRefineSV\(Context& ctx, const Dataset& data, const GraphResult& g, "
                     r"Metric metric", hpp)
    host = os.path.join(ROOT, "rp-tree_amd", "host")
    assert os.path.exists(os.path.join(host, "example_knn_graph_sparse_metric.cpp"))
    assert "example_knn_graph_sparse_metric" in open(os.path.join(host, "Makefile")).read()
    hs = open(os.path.join(ROOT, "haskell", "Data", "RPTree", "HIP.hs")).read()
    for word in ("knnGraphMetricSVHIP", "knnGraphRefineMetricSVHIP", "rpt_knn_graph_csr_metric_host",
                 "rpt_knn_graph_refine_csr_metric_host"):
        assert word in hs, word
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "rpt_knn_graph_csr_metric_host" in integ and "rpt_knn_graph_refine_csr_metric_host" in integ
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "knnGraphMetricSV" in readme and "knnGraphRefineMetricSV" in readme and "graph_csr_masked" in readme
    assert "cosine / inner product on CSR rows and streamed forests are not built" not in readme
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "rpt_knn_graph_csr_metric" in design and "graph_csr_masked" in design
    assert "knn_graph_metric_csr_times.py" in open(os.path.join(ROOT, "tools", "README.md")).read()
    assert os.path.exists(os.path.join(ROOT, "tools", "knn_graph_metric_csr_times.py"))


# ------------------------------------------------------------------ the zero-fill argument, in numpy
def awkward_set(bad=False):
    """200 x 70 rows: empty rows, duplicates, stored +0.0 and -0.0, one full row, rows scaled by 10,
    f32-rounded values; bad: two rows also store an inf and a NaN"""
    rows = [(c.copy(), v.copy()) for c, v in mc.rows_of(mc.make_csr(42, 200, 70, 0.15))]
    none = (np.zeros(0, dtype=np.int32), np.zeros(0))
    for e in (0, 13, 14, 199):
        rows[e] = none
    rows[5] = rows[17]
    rows[150] = rows[17]
    for i in range(40, 80):
        rows[i] = (rows[i][0], rows[i][1].astype(np.float32).astype(np.float64))
    rows[20] = (np.array([0, 3, 33, 69], dtype=np.int32), np.array([0.0, -0.0, 1.25, -0.0]))
    rows[21] = (np.array([69], dtype=np.int32), np.array([-0.0]))
    rows[22] = (np.arange(70, dtype=np.int32), np.random.default_rng(1).standard_normal(70))     # a full row
    for i in range(90, 100):
        rows[i] = (rows[i][0], rows[i][1] * 10.0)
    if bad:
        rows[30] = (rows[30][0], np.concatenate([[np.inf], rows[30][1][1:]]))
        rows[31] = (rows[31][0], np.concatenate([rows[31][1][:-1], [np.nan]]))
        assert len(rows[30][0]) > 1 and len(rows[31][0]) > 1
    return mc.from_rows(rows, 70)


def test_zero_filled_fold_equals_dotS_for_finite_values():
    """x * (+0.0) is +-0.0 and an accumulator that starts at +0.0 is never -0.0, so acc + (+-0.0) is
    acc: the fold over zero-filled windows is dotS bit for bit, all 40 000 ordered pairs"""
    csr = awkward_set()
    X, P = mc.dense(csr)
    assert X.shape == (200, 70) and P[20, 3] and np.signbit(X[20, 3]) and P[22].all() and not P[0].any()
    G = mc.dots_matrix(X, P)
    Z = mc.zero_filled_matrix(X)
    assert np.array_equal(G.view(np.uint64), Z.view(np.uint64))
    assert not np.signbit(G[G == 0.0]).any()                  # the accumulator is never -0.0
    assert np.array_equal(G.view(np.uint64), G.T.view(np.uint64))      # symmetric bit for bit
    for metric in mc.METRICS:
        D = mc.dist_matrix(metric, G)
        assert np.array_equal(mc.bits(D), mc.bits(D.T)), metric
    cos = mc.dist_matrix("cosine", G)
    assert np.isnan(cos[0]).all() and np.isnan(cos[21]).all() and np.isnan(cos[:, 13]).all()   # empty, all-zero rows
    inner = mc.dist_matrix("inner", G)
    assert inner[0, 1] == 0.0 and np.signbit(inner[0, 1])      # no shared column: -0.0


def test_zero_filled_fold_is_not_dotS_with_a_stored_inf_or_nan():
    """the counter-example the presence-masked path exists for: inf * 0 = NaN"""
    one = mc.from_rows([(np.array([0], dtype=np.int32), np.array([np.inf])),
                        (np.array([1], dtype=np.int32), np.array([1.0]))], 2)
    X, P = mc.dense(one)
    G = mc.dots_matrix(X, P)
    assert G[0, 1] == 0.0 and not np.signbit(G[0, 1]) and np.isposinf(G[0, 0]) and G[1, 1] == 1.0
    assert np.isnan(mc.zero_filled_matrix(X)[0, 1])
    assert mc.dot_pair([0], [np.inf], [1], [1.0]) == 0.0
    # ... and in the awkward set: the rows that do not share the inf's / the NaN's column
    csr = awkward_set(bad=True)
    X, P = mc.dense(csr)
    G, Z = mc.dots_matrix(X, P), mc.zero_filled_matrix(X)
    differ = mc.bits(G) != mc.bits(Z)
    assert differ.any() and differ[30].any() and differ[31].any()
    rows = np.nonzero(differ.any(axis=1))[0]
    assert set(rows.tolist()) - {30, 31}                         # their mates' rows differ too
    others = [i for i in range(200) if i not in (30, 31)]
    assert not differ[np.ix_(others, others)].any()
    assert np.array_equal(mc.bits(G), mc.bits(G.T))
    # where a row shares the column, dotS itself is inf or NaN: the definition, not an accident
    c30, c31 = mc.rows_of(csr)[30][0][0], mc.rows_of(csr)[31][0][-1]
    assert np.all(~np.isfinite(G[30, P[:, c30]])) and np.all(np.isnan(G[31, P[:, c31]]))
    assert np.all(np.isfinite(G[30, ~P[:, c30]])) and np.all(np.isfinite(G[31, ~P[:, c31]]))


def test_two_pointer_merge_equals_the_matrix():
    for bad in (False, True):
        csr = awkward_set(bad)
        X, P = mc.dense(csr)
        G = mc.dots_matrix(X, P)
        rows = mc.rows_of(csr)
        got = np.array([[mc.dot_pair(ci, vi, cj, vj) for cj, vj in rows] for ci, vi in rows])
        assert np.array_equal(mc.bits(got), mc.bits(G)), bad


# ------------------------------------------------------------------ the restatement on a small sparse set
def test_rounds_never_lower_recall_and_the_first_raises_it():
    """on the sparse golden forest (3 trees, k = 10, reverse = 10): C(i) contains F(i), so recall
    against the exact graph under the same distance never falls round over round, and round 1
    raises it"""
    import rptree_amd as rp
    z = np.load(os.path.join(ROOT, "tests", "golden", "forest_sparse_600x12.npz"))
    csr = (z["rowptr"], z["col"], z["val"], int(z["d"]))
    X, P = mc.dense(csr)
    G = mc.dots_matrix(X, P)
    empty = int((np.diff(z["rowptr"]) == 0).sum())
    leaves = mc.leaf_slices(rp.topology(int(z["n"]), int(z["L"]), int(z["min_leaf"])))
    k = 10
    for metric in mc.METRICS:
        D = mc.dist_matrix(metric, G)
        g = mc.knn_graph_ref(X, z["perm"], leaves, k, D)
        exact = mc.exact_graph(D, k)
        recalls = [mc.recall(g, exact)]
        for _ in range(3):
            g, rounds, updates, cands = mc.refine_ref(X, g, k, 10, 1, D)
            assert rounds == 1 and cands >= updates
            ids, dist, cnt = g
            for i in range(X.shape[0]):
                c = cnt[i]
                assert i not in ids[i] and len(set(ids[i, :c].tolist())) == c
                assert np.all(ids[i, c:] == -1) and np.all(np.isposinf(dist[i, c:]))
                assert np.array_equal(np.lexsort((ids[i, :c], dist[i, :c])), np.arange(c))
            recalls.append(mc.recall(g, exact))
        print("sparse 600 x 12, %s (%d empty rows): recall %s" % (metric, empty, ["%.3f" % x for x in recalls]))
        assert all(b >= a for a, b in zip(recalls, recalls[1:])), (metric, recalls)
        assert recalls[1] > recalls[0], (metric, recalls)
