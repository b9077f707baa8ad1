"""The kNN graph and its NN-descent rounds on SVector (CSR) rows (rpt_knn_graph_csr_*,
rpt_knn_graph_refine_csr_*) are declared at every layer, the zero-column argument their kernels rest
on holds in numpy, and the restatement behaves as NN-descent should on sparse rows (no GPU)."""
import inspect
import os
import re
import shutil
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_graph_csr_ref as cref  # noqa: E402

HEADER = open(os.path.join(ROOT, "include", "rptree_hip.h")).read()
NAMES = ("rpt_knn_graph_csr_dev", "rpt_knn_graph_csr_host", "rpt_knn_graph_refine_csr_dev",
         "rpt_knn_graph_refine_csr_host")


def _decl(name):
    m = re.search(r"int32_t\s+%s\s*\(([^;]*)\)\s*;" % name, HEADER)
    assert m, name
    return re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)


def _words(decl):
    return [re.sub(r"\s+", " ", a.strip()) for a in decl.split(",")]


def test_header_declares_the_entry_points():
    dev = _words(_decl("rpt_knn_graph_csr_dev"))
    assert dev == ["rpt_ctx* ctx", "rpt_forest* f", "const rpt_dataset* data", "int32_t k", "int32_t flags",
                   "int32_t* ids_dev", "double* dist_dev", "int32_t* count_dev"]
    assert dev == _words(_decl("rpt_knn_graph_dev"))
    host = _words(_decl("rpt_knn_graph_csr_host"))
    assert host[:5] == dev[:5] and host[5:] == ["int32_t* ids_host", "double* dist_host", "int32_t* count_host"]
    rdev = _words(_decl("rpt_knn_graph_refine_csr_dev"))
    assert rdev == ["rpt_ctx* ctx", "const rpt_dataset* data", "int32_t k", "int32_t reverse", "int32_t iters",
                    "int32_t flags", "int32_t* ids_dev", "double* dist_dev", "int32_t* count_dev"]
    assert rdev == _words(_decl("rpt_knn_graph_refine_dev"))
    rhost = _words(_decl("rpt_knn_graph_refine_csr_host"))
    assert rhost[:6] == rdev[:6] and rhost[6:] == ["int32_t* ids_host", "double* dist_host", "int32_t* count_host"]
    assert re.search(r"#define\s+RPT_ABI_VERSION\s+1\b", HEADER)


def test_header_comment_states_the_definition():
    comment = HEADER[HEADER.index("the kNN graph and its NN-descent rounds on SVector (CSR) rows"):
                     HEADER.index("int32_t rpt_knn_graph_csr_dev")]
    flat = re.sub(r"\s*\n \*\s*", " ", comment)
    for phrase in ("absent columns are +0.0", "widened exactly", "a stored zero is a zero", "word for word",
                   "metricDDL2's left fold over dense(x_i), dense(x_j)", "mates(i)", "F / Rev_r / B / C",
                   "NaN behind every number", "id -1, distance +inf", "RPT_GRAPH_ACCUMULATE", "one owner per list",
                   "no atomics on a list", "a round that changes nothing ends the sequence",
                   "_dev enqueues and does not synchronise", "graph_general", "graph_refine_general",
                   "rpt_knn_graph_last_pairs", "rpt_knn_graph_refine_last", "class 3",
                   "do not visit all d columns", "acc + (+0.0)", "never becomes -0.0",
                   "any ascending superset of the union of the two supports", "bit-equal",
                   "symmetric bit for bit", "still evaluated once", "at distance 0", "ascend strictly",
                   "checks only col < d", "unspecified", "stay in bounds and terminate",
                   "no limit on a row's length or on d", "RPT_E_ARG", "RPT_E_UNSUPPORTED", "streamed forest",
                   "n = 0, n = 1, depth 0 and rows with no nonzeros"):
        assert phrase in flat, phrase
    # the dense entry points still state their refusal of CSR rows
    old = HEADER[HEADER.index("kNN graph of the indexed points: knn"):HEADER.index("int32_t rpt_knn_graph_dev")]
    assert "CSR data, a streamed forest" in re.sub(r"\s*\n \*\s*", " ", old)


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
    assert _lib.SYMBOLS["rpt_knn_graph_csr_dev"] == _lib.SYMBOLS["rpt_knn_graph_dev"]
    assert _lib.SYMBOLS["rpt_knn_graph_csr_host"] == _lib.SYMBOLS["rpt_knn_graph_host"]
    assert _lib.SYMBOLS["rpt_knn_graph_refine_csr_dev"] == _lib.SYMBOLS["rpt_knn_graph_refine_dev"]
    assert _lib.SYMBOLS["rpt_knn_graph_refine_csr_host"] == _lib.SYMBOLS["rpt_knn_graph_refine_host"]
    declared = set(re.findall(r"^\s*(?:int32_t|const char\*)\s+(rpt_\w+)\s*\(", HEADER, flags=re.M))
    assert declared == set(_lib.SYMBOLS)
    for name in ("knnGraphSV", "knnGraphSVDev", "knnGraphRefineSV", "knnGraphRefineSVDev"):
        assert name in rp.__all__ and callable(getattr(rp, name))
    # the shapes mirror the dense functions, which are unchanged
    for sv, dense, params in ((rp.knnGraphSV, rp.knnGraph, ["k", "forest", "accumulate"]),
                              (rp.knnGraphSVDev, rp.knnGraphDev,
                               ["k", "forest", "ids_ptr", "dist_ptr", "count_ptr", "accumulate"]),
                              (rp.knnGraphRefineSV, rp.knnGraphRefine, ["graph", "data", "iters", "reverse", "ctx"]),
                              (rp.knnGraphRefineSVDev, rp.knnGraphRefineDev,
                               ["k", "data", "ids_ptr", "dist_ptr", "count_ptr", "iters", "reverse"])):
        assert list(inspect.signature(dense).parameters) == params
        assert str(inspect.signature(sv)) == str(inspect.signature(dense))


def test_library_exports_them():
    from rptree_amd import _lib
    L = _lib.lib()
    for name in NAMES:
        assert hasattr(L, name), name


def test_makefile_builds_the_new_source_without_contraction():
    out = subprocess.run(["make", "-n", "-B", "-C", os.path.join(ROOT, "rp-tree_amd")], capture_output=True,
                         text=True)
    assert out.returncode == 0, out.stderr
    line = [ln for ln in out.stdout.splitlines() if "csrc/graph_csr.hip" in ln]
    assert line and "-ffp-contract=off" in line[0] and "--offload-arch=gfx950" in line[0]
    assert "fast-math" not in line[0]
    assert any("-shared" in ln and "build/graph_csr.o" in ln for ln in out.stdout.splitlines())


def test_kernel_source_shares_the_helpers():
    csrc = os.path.join(ROOT, "rp-tree_amd", "csrc")
    src = open(os.path.join(csrc, "graph_csr.hip")).read()
    refine = open(os.path.join(csrc, "graph_refine.hip")).read()
    shared = open(os.path.join(csrc, "graph_refine_dev.h")).read()
    for kern in ("graph_csr_leaf_kernel", "graph_csr_tiled_kernel", "refine_join_csr_kernel"):
        assert len(re.findall(r"__global__[^;{]*\b%s\(" % kern, src)) == 1, kern
    for word in ("fold_step<kGraphL2>", "fold_finish<kGraphL2>", "wave_merge(", "rev_fill_kernel", "kLS", "kCW",
                 "set_insert(", "RPT_PROF_KNN_TOPK", "graph_general", "graph_refine_general"):
        assert word in src, word
    # one definition of the round's state and bookkeeping kernels, shared with the dense refinement
    for kern in ("refine_begin_kernel", "refine_end_kernel", "refine_copy_kernel"):
        assert len(re.findall(r"__global__[^;{]*\b%s\(" % kern, shared)) == 1, kern
        assert kern in src and kern in refine
        assert not re.search(r"__global__[^;{]*\b%s\(" % kern, src + refine)
    assert "struct RefineState" in shared and "struct RefineState" not in src + refine
    assert "inline bool wave_merge" not in src and "inline bool before" not in src


def test_other_layers_name_it():
    hpp = open(os.path.join(ROOT, "rp-tree_amd", "host", "rptree.hpp")).read()
    assert "rpt_knn_graph_csr_host" in hpp and "rpt_knn_graph_refine_csr_host" in hpp
    assert "knnGraphSV" in hpp and "knnGraphRefineSV" in hpp
    assert os.path.exists(os.path.join(ROOT, "rp-tree_amd", "host", "example_knn_graph_sparse.cpp"))
    assert "example_knn_graph_sparse" in open(os.path.join(ROOT, "rp-tree_amd", "host", "Makefile")).read()
    hs = open(os.path.join(ROOT, "haskell", "Data", "RPTree", "HIP.hs")).read()
    for word in ("knnGraphSVHIP", "knnGraphRefineSVHIP", "rpt_knn_graph_csr_host", "rpt_knn_graph_refine_csr_host"):
        assert word in hs, word
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "rpt_knn_graph_csr_host" in integ and "rpt_knn_graph_refine_csr_host" in integ
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "knnGraphSV" in readme and "knnGraphRefineSV" in readme
    assert "rpt_knn_graph_csr" in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "knn_graph_csr_times.py" in open(os.path.join(ROOT, "tools", "README.md")).read()
    assert os.path.exists(os.path.join(ROOT, "tools", "knn_graph_csr_times.py"))


# ------------------------------------------------------------------ the zero-column argument, in numpy
def awkward_set():
    """200 x 70 rows: empty rows, duplicates, f32-rounded values, stored +0.0 and -0.0, an inf and a NaN"""
    rows = [(c.copy(), v.copy()) for c, v in cref.rows_of(cref.make_csr(42, 200, 70, 0.15))]
    none = (np.zeros(0, dtype=np.int32), np.zeros(0))
    for e in (0, 13, 14, 199):
        rows[e] = none
    rows[5] = rows[17]
    rows[150] = rows[17]
    for i in range(40, 80):
        rows[i] = (rows[i][0], rows[i][1].astype(np.float32).astype(np.float64))
    rows[20] = (np.array([0, 3, 33, 69], dtype=np.int32), np.array([0.0, -0.0, 1.25, -0.0]))
    rows[21] = (np.array([69], dtype=np.int32), np.array([0.0]))
    rows[30] = (rows[30][0], np.concatenate([[np.inf], rows[30][1][1:]]))
    rows[31] = (rows[31][0], np.concatenate([rows[31][1][:-1], [np.nan]]))
    assert len(rows[30][0]) > 1 and len(rows[31][0]) > 1
    return cref.from_rows(rows, 70)


def test_union_fold_equals_the_dense_fold_bit_for_bit():
    """acc + (+0.0) is acc for every acc the fold can hold, so skipping the columns where both rows
    hold +0.0 changes no bit: all 40 000 ordered pairs"""
    csr = awkward_set()
    X = cref.densify(csr)
    assert X.shape == (200, 70) and np.signbit(X[20, 3]) and not np.signbit(X[20, 1])
    rows = cref.rows_of(csr)
    differing = 0
    for i in range(200):
        want = cref.bits(cref.fold_dist(X[i], X))
        got = cref.bits([cref.union_fold(rows[i][0], rows[i][1], c, v) for c, v in rows])
        differing += int((want != got).sum())
    assert differing == 0
    D = np.array([cref.fold_dist(X[i], X) for i in range(200)])
    assert np.array_equal(cref.bits(D), cref.bits(D.T))    # symmetric bit for bit
    assert D[0, 13] == 0.0 and D[13, 199] == 0.0 and D[0, 21] == 0.0      # empty rows, a row of one stored zero
    assert np.isnan(D[31]).sum() == 200 and np.isposinf(D[30, 0])
    assert not np.signbit(D[np.isfinite(D)]).any()


# ------------------------------------------------------------------ the restatement on a small sparse set
def test_rounds_never_lower_recall_and_the_first_raises_it():
    """on the sparse golden forest: C(i) contains F(i), so recall against the exact graph of the
    dense-ified rows never falls round over round, and round 1 raises it"""
    import rptree_amd as rp
    z = np.load(os.path.join(ROOT, "tests", "golden", "forest_sparse_600x12.npz"))
    csr = (z["rowptr"], z["col"], z["val"], int(z["d"]))
    X = cref.densify(csr)
    leaves = cref.leaf_slices(rp.topology(int(z["n"]), int(z["L"]), int(z["min_leaf"])))
    k = 10
    g = cref.knn_graph_ref(X, z["perm"], leaves, k)
    exact = cref.exact_graph(X, k)
    recalls = [cref.recall(g, exact)]
    for _ in range(3):
        g, rounds, updates, cands = cref.refine_ref(X, g, k, 10, 1)
        assert rounds == 1 and cands >= updates
        ids, dist, cnt = g
        for i in range(X.shape[0]):
            c = cnt[i]
            assert i not in ids[i] and len(set(ids[i, :c].tolist())) == c
            assert np.all(ids[i, c:] == -1) and np.all(np.isposinf(dist[i, c:]))
            assert np.array_equal(np.lexsort((ids[i, :c], dist[i, :c])), np.arange(c))
        recalls.append(cref.recall(g, exact))
    print("sparse 600 x 12: recall %s" % ["%.3f" % x for x in recalls])
    assert all(b >= a for a, b in zip(recalls, recalls[1:])), recalls
    assert recalls[1] > recalls[0], recalls
