"""The kNN graph and its refinement under the cosine and inner-product distances
(rpt_knn_graph_metric_*, rpt_knn_graph_refine_metric_*) are declared at every layer, and the numpy
restatement that the GPU tests compare with is the stated definition (no GPU)."""
import inspect
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_graph_ref as ref  # noqa: E402
import knn_graph_metric_ref as mref  # noqa: E402
import knn_graph_refine_ref as rref  # noqa: E402

HEADER = open(os.path.join(ROOT, "include", "rptree_hip.h")).read()
NAMES = ("rpt_knn_graph_metric_dev", "rpt_knn_graph_metric_host", "rpt_knn_graph_refine_metric_dev",
         "rpt_knn_graph_refine_metric_host")


def _decl(name):
    m = re.search(r"int32_t\s+%s\s*\(([^;]*)\)\s*;" % name, HEADER)
    assert m, name
    return re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)


def _words(decl):
    return [re.sub(r"\s+", " ", a.strip()) for a in decl.split(",")]


def test_header_declares_the_entry_points():
    dev = _words(_decl("rpt_knn_graph_metric_dev"))
    assert dev == ["rpt_ctx* ctx", "rpt_forest* f", "const rpt_dataset* data", "int32_t k", "int32_t metric",
                   "int32_t flags", "int32_t* ids_dev", "double* dist_dev", "int32_t* count_dev"]
    host = _words(_decl("rpt_knn_graph_metric_host"))
    assert host[:6] == dev[:6] and host[6:] == ["int32_t* ids_host", "double* dist_host", "int32_t* count_host"]
    rdev = _words(_decl("rpt_knn_graph_refine_metric_dev"))
    assert rdev == ["rpt_ctx* ctx", "const rpt_dataset* data", "int32_t k", "int32_t reverse", "int32_t iters",
                    "int32_t metric", "int32_t flags", "int32_t* ids_dev", "double* dist_dev", "int32_t* count_dev"]
    rhost = _words(_decl("rpt_knn_graph_refine_metric_host"))
    assert rhost[:7] == rdev[:7] and rhost[7:] == ["int32_t* ids_host", "double* dist_host", "int32_t* count_host"]
    # the old entry points keep their signatures
    assert _decl("rpt_knn_graph_dev").count(",") == 7 and _decl("rpt_knn_graph_refine_dev").count(",") == 8
    assert re.search(r"#define\s+RPT_ABI_VERSION\s+1\b", HEADER)


def test_header_comment_states_the_definition():
    comment = HEADER[HEADER.index("the kNN graph and its refinement under the cosine and inner-product"):
                     HEADER.index("int32_t rpt_knn_graph_metric_dev")]
    flat = re.sub(r"\s*\n \*\s*", " ", comment)
    for phrase in ("RPT_KNN_METRIC_COSINE", "RPT_KNN_METRIC_INNER", "dist(i, j) = -dot(x_i, x_j)",
                   "1 - dot(x_i, x_j) / (sqrt(dot(x_i, x_i)) * sqrt(dot(x_j, x_j)))", "no FMA", "zero row gives NaN",
                   "the same bits as the entry points without `metric`", "symmetric bit for bit",
                   "a pair is still evaluated once", "-0.0 ties with +0.0 and the id decides",
                   "stored bits are the computed ones", "not a metric", "excluded by id",
                   "is NOT detected", "taken as stored", "RPT_E_ARG", "RPT_KNN_METRIC_REFERENCE",
                   "RPT_E_UNSUPPORTED", "graph_general", "graph_refine_general", "class 3",
                   "rpt_knn_graph_last_pairs", "rpt_knn_graph_refine_last", "8 bytes per row", "must not change"):
        assert phrase in flat, phrase
    # the old entry points still state their refusal of the metric bits
    old = HEADER[HEADER.index("kNN graph of the indexed points: knn"):HEADER.index("int32_t rpt_knn_graph_dev")]
    assert "RPT_KNN_METRIC_* flags: RPT_E_UNSUPPORTED" in re.sub(r"\s*\n \*\s*", " ", old)


def test_sources_instantiate_the_kernels_on_the_metric():
    """one kernel body per kernel, instantiated on the distance; the norms come from the dataset's cache"""
    csrc = os.path.join(ROOT, "rp-tree_amd", "csrc")
    graph = open(os.path.join(csrc, "graph.hip")).read()
    refine = open(os.path.join(csrc, "graph_refine.hip")).read()
    dev = open(os.path.join(csrc, "graph_dev.h")).read()
    assert len(re.findall(r"__global__[^;{]*\bgraph_leaf_kernel\(", graph)) == 1
    assert len(re.findall(r"__global__[^;{]*\bgraph_tiled_kernel\(", graph)) == 1
    assert len(re.findall(r"__global__[^;{]*\brefine_join_kernel\(", refine)) == 1
    for src in (graph, refine):
        assert "template <class TD, int M>" in src and "fold_step<M>" in src and "fold_finish<M>" in src
        assert "ensure_sqnorm(ctx, data)" in src
    assert "fold_step" in dev and "fold_finish" in dev
    common = open(os.path.join(csrc, "common.h")).read()
    assert re.search(r"int32_t ensure_sqnorm\(rpt_ctx\* ctx, const rpt_dataset\* data\);", common)
    knn = open(os.path.join(csrc, "knn.hip")).read()
    assert len(re.findall(r"\bint32_t ensure_sqnorm\(", knn)) == 1 and "static int32_t ensure_sqnorm" not in knn
    mk = open(os.path.join(ROOT, "rp-tree_amd", "Makefile")).read()
    assert "-ffp-contract=off" in mk and "fast-math" not in mk


def test_ctypes_table_and_python_mirror():
    import rptree_amd as rp
    from rptree_amd import _lib
    assert len(_lib.SYMBOLS["rpt_knn_graph_metric_dev"][1]) == 9
    assert len(_lib.SYMBOLS["rpt_knn_graph_metric_host"][1]) == 9
    assert len(_lib.SYMBOLS["rpt_knn_graph_refine_metric_dev"][1]) == 10
    assert len(_lib.SYMBOLS["rpt_knn_graph_refine_metric_host"][1]) == 10
    declared = set(re.findall(r"^\s*(?:int32_t|const char\*)\s+(rpt_\w+)\s*\(", HEADER, flags=re.M))
    assert declared == set(_lib.SYMBOLS)
    for name in ("knnGraphMetric", "knnGraphMetricDev", "knnGraphRefineMetric", "knnGraphRefineMetricDev"):
        assert name in rp.__all__ and callable(getattr(rp, name))
    sig = inspect.signature(rp.knnGraphMetric)
    assert list(sig.parameters) == ["distf", "k", "forest", "accumulate"] and sig.parameters["accumulate"].default is None
    sig = inspect.signature(rp.knnGraphMetricDev)
    assert list(sig.parameters) == ["distf", "k", "forest", "ids_ptr", "dist_ptr", "count_ptr", "accumulate"]
    assert sig.parameters["accumulate"].default is False
    sig = inspect.signature(rp.knnGraphRefineMetric)
    assert list(sig.parameters) == ["distf", "graph", "data", "iters", "reverse", "ctx"]
    assert sig.parameters["iters"].default == 1 and sig.parameters["reverse"].default is None
    sig = inspect.signature(rp.knnGraphRefineMetricDev)
    assert list(sig.parameters) == ["distf", "k", "data", "ids_ptr", "dist_ptr", "count_ptr", "iters", "reverse"]
    # the old mirrors are unchanged
    assert list(inspect.signature(rp.knnGraph).parameters) == ["k", "forest", "accumulate"]
    assert list(inspect.signature(rp.knnGraphRefine).parameters) == ["graph", "data", "iters", "reverse", "ctx"]


def test_distf_goes_through_metric_flag():
    """an unknown distf is refused before any handle is touched"""
    import rptree_amd as rp
    assert rp._metric_flag(None) == 0 and rp._metric_flag(rp.metricL2) == 0
    assert rp._metric_flag(rp.metricCosine) == rp.RPT_KNN_METRIC_COSINE
    assert rp._metric_flag(rp.metricInner) == rp.RPT_KNN_METRIC_INNER
    for call in (lambda: rp.knnGraphMetric(max, 3, None), lambda: rp.knnGraphMetricDev("cosine", 3, None, 0, 0, 0),
                 lambda: rp.knnGraphRefineMetric(max, None, None), lambda: rp.knnGraphRefineMetricDev(1, 3, None, 0, 0, 0)):
        with pytest.raises(NotImplementedError):
            call()


def test_library_exports_them():
    from rptree_amd import _lib
    L = _lib.lib()
    for name in NAMES:
        assert hasattr(L, name), name


def test_header_still_compiles_as_c99():
    gcc = shutil.which("gcc")
    assert gcc, "no gcc"
    pr = subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c",
                         os.path.join(ROOT, "include", "rptree_hip.h")], stdout=subprocess.PIPE,
                        stderr=subprocess.STDOUT)
    assert pr.returncode == 0, pr.stdout.decode()


def test_other_layers_name_it():
    hpp = open(os.path.join(ROOT, "rp-tree_amd", "host", "rptree.hpp")).read()
    assert "rpt_knn_graph_metric_host" in hpp and "rpt_knn_graph_refine_metric_host" in hpp
    assert re.search(r"GraphResult knnGraph\(const RPForest& tts, int k, Metric metric", hpp)
    assert re.search(r"GraphResult knnGraphRefine\(Context& ctx, const Dataset& data, const GraphResult& g, Metric metric", hpp)
    assert os.path.exists(os.path.join(ROOT, "rp-tree_amd", "host", "example_knn_graph_metric.cpp"))
    assert "example_knn_graph_metric" in open(os.path.join(ROOT, "rp-tree_amd", "host", "Makefile")).read()
    hs = open(os.path.join(ROOT, "haskell", "Data", "RPTree", "HIP.hs")).read()
    for word in ("knnGraphMetricHIP", "knnGraphRefineMetricHIP", "rpt_knn_graph_metric_host",
                 "rpt_knn_graph_refine_metric_host"):
        assert word in hs, word
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "rpt_knn_graph_metric_host" in integ and "rpt_knn_graph_refine_metric_host" in integ
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "knnGraphMetric" in readme and "knnGraphRefineMetric" in readme
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "rpt_knn_graph_metric" in design
    assert "knn_graph_metric_times.py" in open(os.path.join(ROOT, "tools", "README.md")).read()
    assert os.path.exists(os.path.join(ROOT, "tools", "knn_graph_metric_times.py"))


# ------------------------------------------------------------------ the restatement on the golden forest
@pytest.fixture(scope="module")
def golden():
    import rptree_amd as rp
    z = np.load(os.path.join(ROOT, "tests", "golden", "forest_dense_1000x16.npz"))
    X, perm = z["X"], z["perm"]
    leaves = ref.leaf_slices(rp.topology(int(z["n"]), int(z["L"]), int(z["min_leaf"])))
    return X, perm, leaves, {m: mref.metric_matrix(X, m) for m in mref.METRICS}


@pytest.mark.parametrize("metric", mref.METRICS)
def test_restatement_is_symmetric_bit_for_bit(golden, metric):
    """IEEE multiplication commutes and the fold visits the same products in the same order: the
    1000 x 1000 matrix equals its transpose exactly"""
    D = golden[3][metric]
    assert np.array_equal(ref.bits(D), ref.bits(D.T))
    assert not np.isnan(D).any()


@pytest.mark.parametrize("metric", mref.METRICS)
def test_restatement_equals_the_host_metrics_on_sampled_pairs(golden, metric):
    import rptree_amd as rp
    X, D = golden[0], golden[3][metric]
    f = {"cosine": rp.metricCosine, "inner": rp.metricInner}[metric]
    rng = np.random.default_rng(5)
    pairs = [(int(a), int(b)) for a, b in rng.integers(0, X.shape[0], size=(300, 2))] + [(7, 7), (0, 999)]
    for i, j in pairs:
        assert ref.bits(np.array([f(X[i], X[j])]))[0] == ref.bits(D[i, j:j + 1])[0], (i, j)
    # ... and the np.cumsum fold of the issue's wording gives the same rows
    for i in (0, 123, 999):
        assert np.array_equal(ref.bits(mref.metric_dist(metric, X[i], X)), ref.bits(D[i]))
    # f32 and bf16 rows widen exactly: the same on the widened doubles
    X32 = X[:40].astype(np.float32)
    D32 = mref.metric_matrix(X32.astype(np.float64), metric)
    for i, j in ((0, 1), (5, 39), (17, 17)):
        assert ref.bits(np.array([f(X32[i], X32[j])]))[0] == ref.bits(D32[i, j:j + 1])[0]


def test_signed_zero_and_zero_rows():
    """-dot is -0.0 for orthogonal rows (the fold from +0.0 never gives a -0.0 dot); the order ties
    -0.0 with +0.0 and the id decides; a zero row is NaN under cosine against everything, itself included"""
    X = np.array([[1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, 2.0], [0.0, 0.0, 0.0], [-1.0, 0.0, 0.0]])
    D = mref.metric_matrix(X, "inner")
    assert D[0, 1] == 0.0 and np.signbit(D[0, 1]) and np.signbit(D[0, 3]) and D[0, 4] == 1.0 and D[0, 0] == -1.0
    C = mref.metric_matrix(X, "cosine")
    assert np.isnan(C[3]).all() and np.isnan(C[:, 3]).all() and C[0, 1] == 1.0 and C[0, 4] == 2.0 and C[0, 0] == 0.0
    m = np.array([1, 2, 3, 5], dtype=np.int32)
    dv = np.array([0.0, -0.0, 0.0, -0.0])
    assert m[np.lexsort((m, dv))].tolist() == [1, 2, 3, 5]
    mr, dr = m[::-1].copy(), dv[::-1].copy()
    assert mr[np.lexsort((mr, dr))].tolist() == [1, 2, 3, 5]


@pytest.mark.parametrize("metric", mref.METRICS)
def test_rounds_never_lower_recall_and_the_first_raises_it(golden, metric):
    """C(i) contains F(i), so a true neighbour never leaves a row: recall against the exact graph
    under the same metric is non-decreasing round over round, and strictly higher after round 1"""
    X, perm, leaves, Ds = golden
    D = Ds[metric]
    k = 10
    g = mref.knn_graph_metric_ref(X, perm, leaves, k, D)
    exact = mref.exact_graph(D, k)
    recalls = [rref.recall(g, exact)]
    for _ in range(3):
        g, rounds, updates, cands = mref.refine_ref(X, g, k, 10, 1, D)
        assert rounds == 1 and cands >= updates
        ids, dist, cnt = g
        for i in range(X.shape[0]):
            c = cnt[i]
            assert i not in ids[i] and len(set(ids[i, :c].tolist())) == c
            assert np.all(ids[i, c:] == -1) and np.all(np.isposinf(dist[i, c:]))
            assert np.array_equal(np.lexsort((ids[i, :c], dist[i, :c])), np.arange(c))
        recalls.append(rref.recall(g, exact))
    print("%s: recall %s" % (metric, ["%.3f" % x for x in recalls]))
    assert all(b >= a for a, b in zip(recalls, recalls[1:])), recalls
    assert recalls[1] > recalls[0], recalls


def test_mixing_metrics_is_taken_as_stored(golden):
    """accumulating a graph built under another metric is not detected: the stored distances rank as
    stored (the restatement's accumulate does what the header says the device does).  Inner-product
    distances of neighbours are negative, so an inner-product prior takes over a cosine graph."""
    X, perm, leaves, Ds = golden
    k = 5
    prior = mref.knn_graph_metric_ref(X, perm[:1], leaves, k, Ds["inner"])
    mixed = mref.knn_graph_metric_ref(X, perm[1:2], leaves, k, Ds["cosine"], prior=prior)
    pure = mref.knn_graph_metric_ref(X, perm[1:2], leaves, k, Ds["cosine"])
    differs = 0
    for i in range(X.shape[0]):
        c = mixed[2][i]
        assert np.array_equal(np.lexsort((mixed[0][i, :c], mixed[1][i, :c])), np.arange(c))
        differs += int(not np.array_equal(mixed[0][i], pure[0][i]))
    assert differs > 0 and (mixed[1][:, 0] < 0).any()


def test_metric_zero_restatement_is_the_l2_one(golden):
    X, perm, leaves, _ = golden
    D = mref.metric_matrix(X, "l2")
    ref.assert_same_graph(mref.knn_graph_metric_ref(X, perm, leaves, 10, D), ref.knn_graph_ref(X, perm, leaves, 10), "l2")
