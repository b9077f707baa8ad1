"""The beam search over the kNN graph (rpt_graph_search_*) is declared at every layer, and the numpy
restatement that the GPU tests compare with behaves as the header says (no GPU)."""
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
import graph_search_ref as sref  # noqa: E402

HEADER = open(os.path.join(ROOT, "include", "rptree_hip.h")).read()
NAMES = ("rpt_graph_search_dev", "rpt_graph_search_host", "rpt_graph_search_last")


def _decl(name):
    m = re.search(r"int32_t\s+%s\s*\(([^;]*)\)\s*;" % name, HEADER)
    assert m, name
    return re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)


def _words(decl):
    return [re.sub(r"\s+", " ", a.strip()) for a in decl.split(",")]


def test_header_declares_the_entry_points():
    dev = _words(_decl("rpt_graph_search_dev"))
    assert _decl("rpt_graph_search_dev").count(",") == 14 and _decl("rpt_graph_search_host").count(",") == 14
    assert dev == ["rpt_ctx* ctx", "const rpt_dataset* data", "const rpt_dataset* queries", "int32_t kg",
                   "const int32_t* gids_dev", "const int32_t* gcount_dev", "int32_t s", "const int32_t* seeds_dev",
                   "int32_t k", "int32_t ef", "int32_t metric", "int32_t flags", "int32_t* ids_dev",
                   "double* dist_dev", "int32_t* count_dev"]
    host = _words(_decl("rpt_graph_search_host"))
    assert host == [w.replace("_dev", "_host") for w in dev]
    assert _decl("rpt_graph_search_last").count(",") == 2
    assert _words(_decl("rpt_graph_search_last")) == ["rpt_ctx* ctx", "int64_t* expansions", "int64_t* evaluated"]
    assert re.search(r"#define\s+RPT_GRAPH_SEARCH_MAX_EF\s+256\b", HEADER)
    assert re.search(r"#define\s+RPT_ABI_VERSION\s+1\b", HEADER)
    # the graph entry points keep their signatures
    assert _decl("rpt_knn_graph_dev").count(",") == 7 and _decl("rpt_knn_graph_refine_dev").count(",") == 8


def test_header_comment_states_the_definition():
    comment = HEADER[HEADER.index("query the kNN graph: best-first beam search"):
                     HEADER.index("int32_t rpt_graph_search_dev")]
    flat = re.sub(r"\s*\n \*\s*", " ", comment)
    for phrase in ("first unexpanded", "(distance, id)", "NaN behind every number", "id -1", "+inf",
                   "does NOT validate", "graph_search_nofilter", "RPT_E_UNSUPPORTED", "class 3",
                   "RPT_E_ARG", "RPT_E_NOMEM", "every id once", "at most n expansions", "an exact visited set, a lossy one, or none",
                   "BEFORE anything is uploaded", "naming the row", "count = min(k, |B|)", "no FMA",
                   "RPT_KNN_METRIC_REFERENCE", "rpt_knn_last_*"):
        assert phrase in flat, phrase
    options = HEADER[HEADER.index("Algorithm switches of a context"):HEADER.index("int32_t rpt_ctx_set_option")]
    assert "graph_search_nofilter" in options
    api = open(os.path.join(ROOT, "rp-tree_amd", "csrc", "api.hip")).read()
    assert '{"graph_search_nofilter", &rpt_options::graph_search_nofilter}' in api


def test_kernel_source_lifts_the_shared_helpers():
    csrc = os.path.join(ROOT, "rp-tree_amd", "csrc")
    src = open(os.path.join(csrc, "graph_search.hip")).read()
    dev = open(os.path.join(csrc, "graph_dev.h")).read()
    assert len(re.findall(r"__global__[^;{]*\bgraph_search_kernel\(", src)) == 1
    for word in ("template <class TD, int M>", "fold_step<M>", "fold_finish<M>", "wave_stage<TD>", "before(",
                 "ensure_sqnorm(ctx, data)", "ensure_sqnorm(ctx, queries)", "RPT_PROF_KNN_TOPK"):
        assert word in src, word
    assert "wave_stage" in dev and "widen16" in dev
    # one definition of the staging, shared with the refinement
    refine = open(os.path.join(csrc, "graph_refine.hip")).read()
    assert "wave_stage<TD>" in refine and "inline void wave_stage" not in refine and "inline void wave_stage" in dev
    assert "inline void wave_stage" not in src
    # the loops are bounded by the definition
    assert "expanded >= a.n" in src


def test_ctypes_table_and_python_mirror():
    import rptree_amd as rp
    from rptree_amd import _lib
    assert len(_lib.SYMBOLS["rpt_graph_search_dev"][1]) == 15
    assert len(_lib.SYMBOLS["rpt_graph_search_host"][1]) == 15
    assert len(_lib.SYMBOLS["rpt_graph_search_last"][1]) == 3
    declared = set(re.findall(r"^\s*(?:int32_t|const char\*)\s+(rpt_\w+)\s*\(", HEADER, flags=re.M))
    assert declared == set(_lib.SYMBOLS)
    assert _lib.RPT_GRAPH_SEARCH_MAX_EF == 256
    for name in ("graphSearch", "graphSearchDev", "graphSearchLast"):
        assert name in rp.__all__ and callable(getattr(rp, name))
    sig = inspect.signature(rp.graphSearch)
    assert list(sig.parameters) == ["graph", "data", "qs", "k", "ef", "seeds", "forest", "seed_k", "metric", "ctx"]
    p = sig.parameters
    assert p["ef"].default is None and p["seeds"].default is None and p["forest"].default is None
    assert p["seed_k"].default == 8 and p["metric"].default is None and p["ctx"].default is None
    sig = inspect.signature(rp.graphSearchDev)
    assert list(sig.parameters) == ["data", "queries", "kg", "gids_ptr", "gcount_ptr", "s", "seeds_ptr", "k", "ef",
                                    "ids_ptr", "dist_ptr", "count_ptr", "metric"]
    assert list(inspect.signature(rp.graphSearchLast).parameters) == ["ctx"]
    with pytest.raises(NotImplementedError):               # an unknown metric is refused before any handle is touched
        rp.graphSearch(None, None, None, 3, metric=max)
    with pytest.raises(NotImplementedError):
        rp.graphSearchDev(None, None, 3, 0, 0, 1, 0, 1, 1, 0, 0, 0, metric="cosine")


def test_library_exports_them():
    from rptree_amd import _lib
    L = _lib.lib()
    for name in NAMES:
        assert hasattr(L, name), name


def test_makefile_builds_the_kernel_without_contraction():
    make = shutil.which("make")
    assert make, "no make"
    pr = subprocess.run([make, "-n", "-B", "-C", os.path.join(ROOT, "rp-tree_amd")], stdout=subprocess.PIPE,
                        stderr=subprocess.STDOUT)
    assert pr.returncode == 0, pr.stdout.decode()
    lines = pr.stdout.decode().splitlines()
    comp = [ln for ln in lines if "csrc/graph_search.hip" in ln and " -c " in ln]
    assert len(comp) == 1 and "-ffp-contract=off" in comp[0] and "--offload-arch=gfx950" in comp[0], comp
    link = [ln for ln in lines if "-shared" in ln]
    assert len(link) == 1 and "build/graph_search.o" in link[0], link


def test_header_still_compiles_as_c99():
    gcc = shutil.which("gcc")
    assert gcc, "no gcc"
    pr = subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c",
                         os.path.join(ROOT, "include", "rptree_hip.h")], stdout=subprocess.PIPE,
                        stderr=subprocess.STDOUT)
    assert pr.returncode == 0, pr.stdout.decode()


def test_other_layers_name_it():
    hpp = open(os.path.join(ROOT, "rp-tree_amd", "host", "rptree.hpp")).read()
    assert "rpt_graph_search_host" in hpp and "rpt_graph_search_last" in hpp
    assert re.search(r"KnnResult graphSearch\(Context& ctx, const Dataset& data, const GraphResult& g,", hpp)
    assert len(re.findall(r"\bgraphSearch\(", hpp)) >= 2 and "Metric metric" in hpp
    assert os.path.exists(os.path.join(ROOT, "rp-tree_amd", "host", "example_graph_search.cpp"))
    assert "example_graph_search" in open(os.path.join(ROOT, "rp-tree_amd", "host", "Makefile")).read()
    hs = open(os.path.join(ROOT, "haskell", "Data", "RPTree", "HIP.hs")).read()
    for word in ("graphSearchHIP", "rpt_graph_search_host"):
        assert word in hs, word
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "rpt_graph_search_host" in integ and "rpt_graph_search_dev" in integ
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "graphSearch" in readme and "graph_search_times" in readme
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "graph_search_kernel" in design and "ten lanes" in design
    assert "graph_search_times.py" in open(os.path.join(ROOT, "tools", "README.md")).read()
    assert os.path.exists(os.path.join(ROOT, "tools", "graph_search_times.py"))


# ------------------------------------------------------------------ the restatement on the golden data
K = 10


@pytest.fixture(scope="module")
def golden():
    """the 1000 x 16 golden rows, the forest's graph and the exact graph (k = 10, L2), 200 perturbed
    stored rows as queries with 16 seeds each, and the true neighbours of the queries"""
    import rptree_amd as rp
    z = np.load(os.path.join(ROOT, "tests", "golden", "forest_dense_1000x16.npz"))
    X, perm = z["X"], z["perm"]
    n = X.shape[0]
    leaves = ref.leaf_slices(rp.topology(int(z["n"]), int(z["L"]), int(z["min_leaf"])))
    Dx = mref.metric_matrix(X, "l2")
    forest_graph = mref.knn_graph_metric_ref(X, perm, leaves, K, Dx)
    exact_graph = mref.exact_graph(Dx, K)
    rng = np.random.default_rng(2024)
    rows = rng.choice(n, 200, replace=False)
    Q = X[rows] + 0.1 * rng.standard_normal((200, X.shape[1]))
    seeds = np.stack([np.random.default_rng(qi).choice(n, 16, replace=False) for qi in range(200)]).astype(np.int32)
    D = sref.query_matrix(X, Q, "l2")
    truth = np.stack([np.lexsort((np.arange(n), D[i]))[:K] for i in range(200)])
    return X, Q, seeds, D, truth, forest_graph, exact_graph


@pytest.mark.parametrize("which", ["forest", "exact"])
@pytest.mark.parametrize("ef", [10, 32, 64])
def test_visited_set_changes_nothing(golden, which, ef):
    """a rejected or evicted id never comes back: with and without the visited set the beam and the
    number of expansions are the same for every query; the first 40 also against the literal form"""
    X, Q, seeds, D, truth, fg, eg = golden
    gids, _, gcnt = fg if which == "forest" else eg
    for i in range(Q.shape[0]):
        drow, srow = D[i].tolist(), seeds[i].tolist()
        b1, e1, o1, u1 = sref.search_one(drow, gids, gcnt, srow, ef, visited=True)
        b0, e0, o0, u0 = sref.search_one(drow, gids, gcnt, srow, ef, visited=False)
        assert b1 == b0 and e1 == e0 and o1 == o0 and u1 == u0, i
        assert o1 <= u1 and e1 <= X.shape[0]
        if i < 40:
            bl, el = sref.search_literal(drow, gids, gcnt, srow, ef)
            assert bl == b1 and el == e1, i


@pytest.mark.parametrize("which", ["forest", "exact"])
def test_answers_are_sorted_duplicate_free_and_no_worse_than_the_seeds(golden, which):
    X, Q, seeds, D, truth, fg, eg = golden
    gids, _, gcnt = fg if which == "forest" else eg
    for ef in (10, 32):
        (ids, dist, cnt), exp, off, up = sref.graph_search_ref(X, Q, gids, gcnt, seeds, K, ef, "l2", D=D)
        assert off <= up and exp >= Q.shape[0]
        for i in range(Q.shape[0]):
            c = cnt[i]
            assert c == K and len(set(ids[i, :c].tolist())) == c
            assert np.array_equal(np.lexsort((ids[i, :c], dist[i, :c])), np.arange(c))
            assert np.array_equal(sref.bits(dist[i, :c]), sref.bits(D[i, ids[i, :c]]))
            best = np.sort(D[i, seeds[i]])[K - 1]          # the k-th of the seeds alone
            assert dist[i, K - 1] <= best


def test_short_beams_and_padding(golden):
    """fewer reachable points than k: the count says so, the rest is id -1 / +inf; no seed: count 0"""
    X, Q, seeds, D, truth, fg, eg = golden
    n = X.shape[0]
    gids = np.full((n, 2), -1, dtype=np.int32)
    gcnt = np.zeros(n, dtype=np.int32)
    gids[0, :2], gcnt[0] = [1, 2], 2
    gids[1, 0], gcnt[1] = 0, 1
    s = np.array([[0, -1, 0], [-1, -1, -1]], dtype=np.int32)
    (ids, dist, cnt), exp, off, up = sref.graph_search_ref(X, Q[:2], gids, gcnt, s, 5, 8, "l2")
    assert cnt.tolist() == [3, 0] and sorted(ids[0, :3].tolist()) == [0, 1, 2]
    assert np.all(ids[0, 3:] == -1) and np.all(np.isposinf(dist[0, 3:])) and np.all(ids[1] == -1)
    assert (exp, off, up) == (3, 3, 2 + 2 + 1 + 0)
    # a count outside [0, kg] and ids outside [0, n) offer nothing
    gcnt[2] = 7
    gids[1, 0] = n
    (ids2, _, cnt2), exp2, off2, up2 = sref.graph_search_ref(X, Q[:2], gids, gcnt, s, 5, 8, "l2")
    assert cnt2.tolist() == [3, 0] and exp2 == 3 and off2 == 3


def test_recall_with_the_exact_graph_from_random_seeds(golden):
    """ef = 64, 16 random seeds per query, the exact 10-NN graph: recall@10 over 200 perturbed stored
    rows is at least 0.90"""
    X, Q, seeds, D, truth, fg, eg = golden
    gids, _, gcnt = eg
    (ids, dist, cnt), exp, off, up = sref.graph_search_ref(X, Q, gids, gcnt, seeds, K, 64, "l2", D=D)
    hits = sum(len(set(ids[i].tolist()) & set(truth[i].tolist())) for i in range(Q.shape[0]))
    recall = hits / (K * Q.shape[0])
    print("recall@10 %.4f, %.1f expansions and %.1f distance evaluations per query" % (
        recall, exp / Q.shape[0], off / Q.shape[0]))
    assert recall >= 0.90
