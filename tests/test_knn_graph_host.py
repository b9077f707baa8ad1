"""The kNN graph of the indexed points (rpt_knn_graph_*) is declared at every layer, and the numpy
restatement of its definition that the GPU tests compare with is self-consistent (no GPU)."""
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

HEADER = open(os.path.join(ROOT, "include", "rptree_hip.h")).read()


def _decl(name):
    m = re.search(r"int32_t\s+%s\s*\(([^;]*)\)\s*;" % name, HEADER)
    assert m, name
    return re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)


def test_header_declares_the_entry_points():
    dev = _decl("rpt_knn_graph_dev")
    assert dev.count(",") == 7
    for word in ("rpt_ctx*", "rpt_forest*", "const rpt_dataset*", "int32_t k", "int32_t flags", "ids_dev",
                 "dist_dev", "count_dev"):
        assert word in dev, word
    host = _decl("rpt_knn_graph_host")
    assert host.count(",") == 7 and "ids_host" in host and "dist_host" in host and "count_host" in host
    pairs = _decl("rpt_knn_graph_last_pairs")
    assert pairs.count(",") == 1 and "int64_t*" in pairs
    assert re.search(r"#define\s+RPT_GRAPH_ACCUMULATE\s+1\b", HEADER)
    m = re.search(r"#define\s+RPT_GRAPH_MAX_K\s+(\d+)", HEADER)
    assert m and int(m.group(1)) >= 64
    assert re.search(r"#define\s+RPT_ABI_VERSION\s+1\b", HEADER)


def test_header_comment_states_the_definition():
    start = HEADER.index("kNN graph of the indexed points")
    comment = HEADER[start:HEADER.index("#define RPT_GRAPH_ACCUMULATE")]
    assert "RPTree.hs:174-176" in comment and "Internal.hs:403-406" in comment
    for phrase in ("never its", "bit-exact", "(distance, id)", "NaN ranks behind every number", "id -1",
                   "+inf", "NOT defined as", "RPT_E_UNSUPPORTED", "graph_general", "f32 arithmetic"):
        assert phrase in comment, phrase
    options = HEADER[HEADER.index("Algorithm switches of a context"):HEADER.index("int32_t rpt_ctx_set_option")]
    assert "graph_general" in options
    api = open(os.path.join(ROOT, "rp-tree_amd", "csrc", "api.hip")).read()
    assert '{"graph_general", &rpt_options::graph_general}' in api


def test_ctypes_table_and_python_mirror():
    import inspect

    import rptree_amd as rp
    from rptree_amd import _lib
    assert len(_lib.SYMBOLS["rpt_knn_graph_dev"][1]) == 8
    assert len(_lib.SYMBOLS["rpt_knn_graph_host"][1]) == 8
    assert len(_lib.SYMBOLS["rpt_knn_graph_last_pairs"][1]) == 2
    assert _lib.RPT_GRAPH_ACCUMULATE == 1
    declared = set(re.findall(r"^\s*(?:int32_t|const char\*)\s+(rpt_\w+)\s*\(", HEADER, flags=re.M))
    assert declared == set(_lib.SYMBOLS)
    for name in ("knnGraph", "knnGraphDev", "knnGraphLastPairs"):
        assert name in rp.__all__ and callable(getattr(rp, name))
    assert list(inspect.signature(rp.knnGraph).parameters) == ["k", "forest", "accumulate"]
    assert inspect.signature(rp.knnGraph).parameters["accumulate"].default is None


def test_library_exports_them():
    from rptree_amd import _lib
    L = _lib.lib()
    for name in ("rpt_knn_graph_dev", "rpt_knn_graph_host", "rpt_knn_graph_last_pairs"):
        assert hasattr(L, name), name


def test_makefile_builds_the_new_source():
    out = subprocess.run(["make", "-n", "-B", "-C", os.path.join(ROOT, "rp-tree_amd")], capture_output=True,
                         text=True)
    assert out.returncode == 0, out.stderr
    line = [ln for ln in out.stdout.splitlines() if "csrc/graph.hip" in ln]
    assert line and "-ffp-contract=off" in line[0] and "--offload-arch=gfx950" in line[0]
    assert any("-shared" in ln and "build/graph.o" in ln for ln in out.stdout.splitlines())


def test_header_still_compiles_as_c99():
    gcc = shutil.which("gcc")
    assert gcc, "no gcc"
    pr = subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c",
                         os.path.join(ROOT, "include", "rptree_hip.h")], stdout=subprocess.PIPE,
                        stderr=subprocess.STDOUT)
    assert pr.returncode == 0, pr.stdout.decode()


def test_other_layers_name_it():
    hpp = open(os.path.join(ROOT, "rp-tree_amd", "host", "rptree.hpp")).read()
    assert "knnGraph" in hpp and "rpt_knn_graph_host" in hpp
    assert os.path.exists(os.path.join(ROOT, "rp-tree_amd", "host", "example_knn_graph.cpp"))
    hs = open(os.path.join(ROOT, "haskell", "Data", "RPTree", "HIP.hs")).read()
    assert "knnGraphHIP" in hs and "rpt_knn_graph_host" in hs
    assert "rpt_knn_graph_host" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "knnGraph" in open(os.path.join(ROOT, "README.md")).read()
    assert "knn_graph_times.py" in open(os.path.join(ROOT, "tools", "README.md")).read()


@pytest.fixture(scope="module")
def golden():
    import rptree_amd as rp
    z = np.load(os.path.join(ROOT, "tests", "golden", "forest_dense_1000x16.npz"))
    X, perm = z["X"], z["perm"]
    leaves = ref.leaf_slices(rp.topology(int(z["n"]), int(z["L"]), int(z["min_leaf"])))
    return X, perm, leaves


def test_restatement_is_self_consistent(golden, oracle):
    X, perm, leaves = golden
    n = X.shape[0]
    assert sum(s for _, s in leaves) == n
    full = ref.knn_graph_ref(X, perm, leaves, n)           # k = n: every mate of every point
    ids, dist, cnt = full
    lists = [dict(zip(ids[i, :cnt[i]].tolist(), ref.bits(dist[i, :cnt[i]]).tolist())) for i in range(n)]
    checked = 0
    for i in range(n):
        assert i not in lists[i] and cnt[i] > 0
        assert np.all(ids[i, cnt[i]:] == -1) and np.all(np.isposinf(dist[i, cnt[i]:]))
        # sorted by (distance, id)
        key = list(zip(dist[i, :cnt[i]].tolist(), ids[i, :cnt[i]].tolist()))
        assert key == sorted(key)
        for j, b in lists[i].items():
            assert lists[j].get(i) == b, "not symmetric: %d %d" % (i, j)
        if i % 25 == 0:                                    # the fold is the oracle's metricDDL2
            for j in ids[i, :cnt[i]][:40]:
                want = np.array([oracle.metric_dd(X[i], X[j])]).view(np.uint64)[0]
                assert lists[i][int(j)] == want
                checked += 1
    assert checked >= 1000
    # the first k of the full lists are the k-lists; folding in an earlier answer changes nothing
    k10 = ref.knn_graph_ref(X, perm, leaves, 10)
    assert np.array_equal(k10[0], ids[:, :10]) and np.array_equal(ref.bits(k10[1]), ref.bits(dist[:, :10]))
    half = ref.knn_graph_ref(X, perm[:1], leaves, 10)
    rest = ref.knn_graph_ref(X, perm[1:], leaves, 10, prior=half)
    ref.assert_same_graph(rest, k10, "accumulate")
