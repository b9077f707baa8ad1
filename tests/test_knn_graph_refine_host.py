"""The kNN graph refinement (rpt_knn_graph_refine_*) is declared at every layer, and the numpy
restatement of its definition that the GPU tests compare with behaves as NN-descent should (no GPU)."""
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
import knn_graph_refine_ref as rref  # noqa: E402

HEADER = open(os.path.join(ROOT, "include", "rptree_hip.h")).read()
NAMES = ("rpt_knn_graph_refine_dev", "rpt_knn_graph_refine_host", "rpt_knn_graph_refine_last")


def _decl(name):
    m = re.search(r"int32_t\s+%s\s*\(([^;]*)\)\s*;" % name, HEADER)
    assert m, name
    return re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)


def test_header_declares_the_entry_points():
    dev = _decl("rpt_knn_graph_refine_dev")
    assert dev.count(",") == 8
    for word in ("rpt_ctx*", "const rpt_dataset*", "int32_t k", "int32_t reverse", "int32_t iters",
                 "int32_t flags", "ids_dev", "dist_dev", "count_dev"):
        assert word in dev, word
    host = _decl("rpt_knn_graph_refine_host")
    assert host.count(",") == 8 and "ids_host" in host and "dist_host" in host and "count_host" in host
    last = _decl("rpt_knn_graph_refine_last")
    assert last.count(",") == 3 and last.count("int64_t*") == 3
    assert re.search(r"#define\s+RPT_ABI_VERSION\s+1\b", HEADER)


def test_header_comment_states_the_definition_and_the_option():
    comment = HEADER[HEADER.index("NN-descent rounds over a kNN graph"):HEADER.index("int32_t rpt_knn_graph_refine_dev")]
    for phrase in ("Rev_r(i)", "B(i)", "C(i)", "a SET", "(distance, id)", "NaN behind every number", "id -1",
                   "+inf", "does NOT validate", "graph_refine_general", "RPT_E_UNSUPPORTED", "RPT_E_NOMEM",
                   "rounds", "updates", "candidates", "class 3"):
        assert phrase in comment, phrase
    options = HEADER[HEADER.index("Algorithm switches of a context"):HEADER.index("int32_t rpt_ctx_set_option")]
    assert "graph_refine_general" in options
    api = open(os.path.join(ROOT, "rp-tree_amd", "csrc", "api.hip")).read()
    assert '{"graph_refine_general", &rpt_options::graph_refine_general}' in api


def test_ctypes_table_and_python_mirror():
    import rptree_amd as rp
    from rptree_amd import _lib
    assert len(_lib.SYMBOLS["rpt_knn_graph_refine_dev"][1]) == 9
    assert len(_lib.SYMBOLS["rpt_knn_graph_refine_host"][1]) == 9
    assert len(_lib.SYMBOLS["rpt_knn_graph_refine_last"][1]) == 4
    declared = set(re.findall(r"^\s*(?:int32_t|const char\*)\s+(rpt_\w+)\s*\(", HEADER, flags=re.M))
    assert declared == set(_lib.SYMBOLS)
    for name in ("knnGraphRefine", "knnGraphRefineDev", "knnGraphRefineLast"):
        assert name in rp.__all__ and callable(getattr(rp, name))
    sig = inspect.signature(rp.knnGraphRefine)
    assert list(sig.parameters) == ["graph", "data", "iters", "reverse", "ctx"]
    assert sig.parameters["iters"].default == 1 and sig.parameters["reverse"].default is None
    assert sig.parameters["ctx"].default is None
    sig = inspect.signature(rp.knnGraphRefineDev)
    assert list(sig.parameters) == ["k", "data", "ids_ptr", "dist_ptr", "count_ptr", "iters", "reverse"]
    assert sig.parameters["iters"].default == 1 and sig.parameters["reverse"].default is None
    assert list(inspect.signature(rp.knnGraphRefineLast).parameters) == ["ctx"]


def test_library_exports_them():
    from rptree_amd import _lib
    L = _lib.lib()
    for name in NAMES:
        assert hasattr(L, name), name


def test_makefile_builds_the_new_source():
    out = subprocess.run(["make", "-n", "-B", "-C", os.path.join(ROOT, "rp-tree_amd")], capture_output=True,
                         text=True)
    assert out.returncode == 0, out.stderr
    line = [ln for ln in out.stdout.splitlines() if "csrc/graph_refine.hip" in ln]
    assert line and "-ffp-contract=off" in line[0] and "--offload-arch=gfx950" in line[0]
    assert any("-shared" in ln and "build/graph_refine.o" in ln for ln in out.stdout.splitlines())


def test_header_still_compiles_as_c99():
    gcc = shutil.which("gcc")
    assert gcc, "no gcc"
    pr = subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c",
                         os.path.join(ROOT, "include", "rptree_hip.h")], stdout=subprocess.PIPE,
                        stderr=subprocess.STDOUT)
    assert pr.returncode == 0, pr.stdout.decode()


def test_other_layers_name_it():
    hpp = open(os.path.join(ROOT, "rp-tree_amd", "host", "rptree.hpp")).read()
    assert "knnGraphRefine" in hpp and "rpt_knn_graph_refine_host" in hpp
    assert os.path.exists(os.path.join(ROOT, "rp-tree_amd", "host", "example_knn_graph_refine.cpp"))
    assert "example_knn_graph_refine" in open(os.path.join(ROOT, "rp-tree_amd", "host", "Makefile")).read()
    hs = open(os.path.join(ROOT, "haskell", "Data", "RPTree", "HIP.hs")).read()
    assert "knnGraphRefineHIP" in hs and "rpt_knn_graph_refine_host" in hs
    assert "rpt_knn_graph_refine_host" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "knnGraphRefine" in open(os.path.join(ROOT, "README.md")).read()
    assert "knn_graph_refine_times.py" in open(os.path.join(ROOT, "tools", "README.md")).read()


# ------------------------------------------------------------------ the restatement on the golden forest
@pytest.fixture(scope="module")
def golden():
    import rptree_amd as rp
    z = np.load(os.path.join(ROOT, "tests", "golden", "forest_dense_1000x16.npz"))
    X, perm = z["X"], z["perm"]
    leaves = ref.leaf_slices(rp.topology(int(z["n"]), int(z["L"]), int(z["min_leaf"])))
    k = 10
    return X, k, ref.knn_graph_ref(X, perm, leaves, k), rref.exact_graph(X, k)


def _slot_keys(g, i):
    """(is NaN, distance, id) of every slot: the (distance, id) order with NaN last, padding behind"""
    return [(bool(np.isnan(dv)), float(0.0 if np.isnan(dv) else dv), int(j) if j >= 0 else 1 << 40)
            for dv, j in zip(g[1][i], g[0][i])]


@pytest.mark.parametrize("reverse", [0, 10])
def test_rounds_raise_recall_and_keep_the_layout(golden, reverse):
    X, k, g0, exact = golden
    n = X.shape[0]
    recalls = [rref.recall(g0, exact)]
    g = g0
    for rnd in range(3):
        new, rounds, updates, cands = rref.refine_ref(X, g, k, reverse, 1)
        assert rounds == 1 and updates > 0 and cands >= updates
        ids, dist, cnt = new
        for i in range(n):
            c = cnt[i]
            assert i not in ids[i]
            assert np.all(ids[i, c:] == -1) and np.all(np.isposinf(dist[i, c:]))
            assert len(set(ids[i, :c].tolist())) == c
            keys = _slot_keys(new, i)
            assert keys == sorted(keys)
            assert all(a <= b for a, b in zip(keys, _slot_keys(g, i))), "row %d moved backwards" % i
        g = new
        recalls.append(rref.recall(g, exact))
    print("reverse %d: recall %s" % (reverse, ["%.4f" % x for x in recalls]))
    assert all(b > a for a, b in zip(recalls, recalls[1:])), recalls
    if reverse == 10:
        assert recalls[3] >= 0.90, recalls                 # the feature's quality claim
    # three single rounds are one call with iters = 3
    g3, rounds, _, _ = rref.refine_ref(X, g0, k, reverse, 3)
    assert rounds == 3
    ref.assert_same_graph(g3, g, "iters 3")


def test_complete_graph_is_a_fixed_point(golden):
    X = golden[0][:60]
    full = rref.exact_graph(X, 59)
    assert np.all(full[2] == 59)
    g, rounds, updates, cands = rref.refine_ref(X, full, 59, 59, 5)
    assert (rounds, updates, cands) == (1, 0, 0)
    ref.assert_same_graph(g, full, "complete graph")


def test_iterating_to_the_fixed_point(golden):
    X, k, g0, _ = golden
    X = X[:300]
    keep = (g0[0][:300] < 300) & (g0[0][:300] >= 0)         # the golden graph cut down to 300 rows
    ids = np.full((300, k), -1, dtype=np.int32)
    dist = np.full((300, k), np.inf)
    cnt = keep.sum(axis=1).astype(np.int32)
    for i in range(300):
        ids[i, :cnt[i]] = g0[0][i][keep[i]]
        dist[i, :cnt[i]] = g0[1][i][keep[i]]
    start = (ids, dist, cnt)
    whole, rounds, updates, cands = rref.refine_ref(X, start, k, 4, 50)
    assert 1 < rounds < 50
    g, steps, tot_u, tot_c = start, 0, 0, 0
    while True:
        g, r1, u, c = rref.refine_ref(X, g, k, 4, 1)
        steps += r1
        tot_u += u
        tot_c += c
        if u == 0:
            break
    assert (steps, tot_u, tot_c) == (rounds, updates, cands)
    ref.assert_same_graph(whole, g, "iters 50")
