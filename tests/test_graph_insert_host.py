"""Inserting new rows into a kNN graph (rpt_graph_insert_*) is declared at every layer, and the numpy
restatement that the GPU tests compare with behaves as the header says: its two forms agree, a chunk
is graph_search_ref's answers over the rows visible so far, one call equals the sequence of
single-chunk calls, every stored distance is the fold of its two rows, and a graph that grew by
insertion answers queries about as well as the exact graph of all rows (no GPU)."""
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
import knn_graph_metric_ref as mref  # noqa: E402
import graph_search_ref as sref  # noqa: E402
import graph_insert_ref as iref  # noqa: E402

HEADER = open(os.path.join(ROOT, "include", "rptree_hip.h")).read()
NAMES = ("rpt_graph_insert_dev", "rpt_graph_insert_host", "rpt_graph_insert_last")


def _decl(name):
    m = re.search(r"int32_t\s+%s\s*\(([^;]*)\)\s*;" % name, HEADER)
    assert m, name
    return re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)


def _words(decl):
    return [re.sub(r"\s+", " ", a.strip()) for a in decl.split(",")]


# ------------------------------------------------------------------ declarations
def test_header_declares_the_entry_points():
    dev = _words(_decl("rpt_graph_insert_dev"))
    assert dev == ["rpt_ctx* ctx", "const rpt_dataset* data", "int32_t kg", "const int32_t* gids_dev",
                   "const double* gdist_dev", "const int32_t* gcount_dev", "int64_t m", "int32_t s",
                   "const int32_t* seeds_dev", "int32_t ef", "int64_t batch", "int32_t metric", "int32_t flags",
                   "int32_t* oids_dev", "double* odist_dev", "int32_t* ocount_dev"]
    assert _words(_decl("rpt_graph_insert_host")) == [w.replace("_dev", "_host") for w in dev]
    assert _words(_decl("rpt_graph_insert_last")) == ["rpt_ctx* ctx", "int64_t* chunks", "int64_t* evaluated",
                                                      "int64_t* offered", "int64_t* accepted"]
    assert re.search(r"#define\s+RPT_ABI_VERSION\s+1\b", HEADER)
    # the neighbouring entry points keep their signatures
    assert _decl("rpt_graph_search_dev").count(",") == 14 and _decl("rpt_graph_search_allow_dev").count(",") == 16


def test_header_comment_states_the_definition():
    comment = HEADER[HEADER.index("insert new rows into a kNN graph"):HEADER.index("int32_t rpt_graph_insert_dev")]
    flat = re.sub(r"\s*\n \*\s*", " ", comment)
    for phrase in ("its LAST m rows are the new ones", "The stored distances ARE read", "read only",
                   "G_0 is the input graph followed by m empty rows", "v_0 = n", "P_c = [v_c, min(v_c + batch, N))",
                   "word for word", "n replaced by v_c", "EARLIER chunk", "k = kg", "symmetric bit for bit",
                   "Row p of G_{c+1} is A_p", "count = |A_p|", "id -1", "+inf", "the first kg by (distance, id)",
                   "NaN behind every number",
                   "(valid entries of row o of G_c) u {(d, p) : p in P_c, (d, o) in A_p}",
                   "carried over unchanged", "v_{c+1} = v_c + |P_c|", "a pure function of",
                   "The order in which reverse offers arrive plays no part", "do not see each other",
                   "m = 0 copies the graph", "gets count 0 and links nothing", "copied verbatim by _dev",
                   "ids outside [0, N)", "graph_search_nofilter", "graph_search_csr_stream", "O(|P_c| kg)",
                   "RPT_E_ARG", "RPT_E_NOMEM", "seeds in {-1} u [0, N)", "does NOT validate",
                   "A refused call leaves the context usable", "chunks = the number of chunks"):
        assert phrase in flat, phrase
    api = open(os.path.join(ROOT, "rp-tree_amd", "csrc", "api.hip")).read()
    for msg in ("batch must be at least 1", "ef must be at least kg", "m must be in [0, data.n]"):
        assert msg in api, msg


def test_kernel_source_links_a_chunk_without_a_pass_over_all_rows():
    csrc = os.path.join(ROOT, "rp-tree_amd", "csrc")
    src = open(os.path.join(csrc, "graph_insert.hip")).read()
    for kern in ("link_count_kernel", "link_scan_kernel", "link_fill_kernel", "link_merge_kernel"):
        assert len(re.findall(r"__global__[^;{]*\b%s\(" % kern, src)) == 1, kern
    # the searches are the existing launches, called from here: no second beam
    assert "graph_search_dev(ctx, &dv, &qv" in src and "graph_search_csr_dev(ctx, &dv, &qv" in src
    assert "beam_insert" not in src and "wave_merge(" in src
    for name in ("graph_search.hip", "graph_search_csr.hip"):
        assert "graph_insert" not in open(os.path.join(csrc, name)).read()
    # one zeroing of the degree array per call, outside the chunk loop; grids sized by the chunk
    head, loop = src[src.index("int32_t graph_insert_dev("):].split("for (int64_t v = n; v < N;)")
    assert head.count("hipMemsetAsync(deg.p") == 1 and "hipMemsetAsync" not in loop and "hipMemcpyAsync" not in loop
    assert "RPT_PROF_GRAPH_LINK" in loop and "cnt * kg" in loop
    make = open(os.path.join(ROOT, "rp-tree_amd", "Makefile")).read()
    assert "csrc/graph_insert.hip" in make


def test_ctypes_table_and_python_mirror():
    import rptree_amd as rp
    from rptree_amd import _lib
    assert len(_lib.SYMBOLS["rpt_graph_insert_dev"][1]) == 16 and len(_lib.SYMBOLS["rpt_graph_insert_host"][1]) == 16
    assert len(_lib.SYMBOLS["rpt_graph_insert_last"][1]) == 5
    assert _lib.SYMBOLS["rpt_graph_insert_dev"][1][6] is _lib.i64 and _lib.SYMBOLS["rpt_graph_insert_dev"][1][10] is _lib.i64
    declared = set(re.findall(r"^\s*(?:int32_t|const char\*)\s+(rpt_\w+)\s*\(", HEADER, flags=re.M))
    assert declared == set(_lib.SYMBOLS)
    for name in ("graphInsert", "graphInsertDev", "graphInsertLast"):
        assert name in rp.__all__ and callable(getattr(rp, name))
    sig = inspect.signature(rp.graphInsert)
    assert list(sig.parameters) == ["graph", "data", "m", "ef", "batch", "seeds", "forest", "seed_k", "metric", "ctx"]
    p = sig.parameters
    assert p["ef"].default is None and p["batch"].default is None and p["seeds"].default is None
    assert p["forest"].default is None and p["seed_k"].default == 8 and p["metric"].default is None
    assert list(inspect.signature(rp.graphInsertDev).parameters) == [
        "data", "kg", "gids_ptr", "gdist_ptr", "gcount_ptr", "m", "s", "seeds_ptr", "ef", "batch", "oids_ptr",
        "odist_ptr", "ocount_ptr", "metric"]
    assert list(inspect.signature(rp.graphInsertLast).parameters) == ["ctx"]
    src = inspect.getsource(rp.graphInsert)
    assert set(re.findall(r"\brpt_\w+_host\b", src)) == {"rpt_graph_insert_host"}       # one body for every layout
    assert "min(m, 4096)" in src and "graph_insert_times" in src          # the default and where it was measured
    with pytest.raises(NotImplementedError):               # an unknown metric is refused before any handle is touched
        rp.graphInsert(None, None, 3, metric=max)


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
    code = re.sub(r"//[^\n]*", "", hpp)
    assert len(re.findall(r"\brpt_graph_insert_host\b", code)) == 1 and "rpt_graph_insert_last" in code
    assert len(re.findall(r"^inline GraphResult graphInsert\(", hpp, flags=re.M)) == 2
    host = os.path.join(ROOT, "rp-tree_amd", "host")
    example = open(os.path.join(host, "example_graph_insert.cpp")).read()
    assert "graphInsert(" in example and "graphSearch(" in example
    make = open(os.path.join(host, "Makefile")).read()
    assert re.search(r"^all:.*\bexample_graph_insert\b", make, flags=re.M)
    assert re.search(r"^example_graph_insert: example_graph_insert.cpp rptree.hpp", make, flags=re.M)
    assert re.search(r"^\trm -f .*\bexample_graph_insert\b", make, flags=re.M)
    assert "rp-tree_amd/host/example_graph_insert" in open(os.path.join(ROOT, ".gitignore")).read()
    hs = open(os.path.join(ROOT, "haskell", "Data", "RPTree", "HIP.hs")).read()
    assert hs.count("graphInsertHIP") >= 3 and "rpt_graph_insert_host" in hs
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "rpt_graph_insert_host" in integ and "rpt_graph_insert_dev" in integ
    readme = open(os.path.join(ROOT, "README.md")).read()
    for word in ("graphInsert", "graph_insert_times", "Not built", "not measured"):
        assert word in readme, word
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for word in ("link_merge_kernel", "link_count_kernel", "visible prefix"):
        assert word in design, word
    assert "graph_insert_times.py" in open(os.path.join(ROOT, "tools", "README.md")).read()
    assert os.path.exists(os.path.join(ROOT, "tools", "graph_insert_times.py"))


# ------------------------------------------------------------------ the restatement, fuzzed
def _fuzz_case(rng):
    """lattice distances (heavy ties, some NaN), a junk graph over the first n rows, junk seeds"""
    n, m = int(rng.integers(0, 40)), int(rng.integers(0, 25))
    N = n + m
    kg = int(rng.integers(1, 6))
    D = rng.integers(0, 5, size=(N, N)).astype(np.float64)
    D = np.minimum(D, D.T)
    nan = rng.random((N, N)) < 0.05
    D[nan | nan.T] = np.nan
    gids = rng.integers(-2, N + 3, size=(n, kg)).astype(np.int32)          # junk ids on both sides of [0, N)
    gdist = rng.integers(0, 5, size=(n, kg)).astype(np.float64)
    gdist[rng.random((n, kg)) < 0.05] = np.nan
    gcnt = rng.integers(-1, kg + 2, size=n).astype(np.int32)               # junk counts
    seeds = rng.integers(-1, N + 1, size=(m, int(rng.integers(1, 5)))).astype(np.int32)
    ef = kg + int(rng.integers(0, 8))
    batch = int(rng.integers(1, m + 3))
    return D, (gids, gdist, gcnt), m, seeds, ef, batch


def _same(a, b):
    return all(np.array_equal(sref.bits(x), sref.bits(y)) for x, y in zip(a, b))


def test_fuzz_the_two_forms_agree_whatever_the_order_of_the_offers():
    """(a) the bounded sorted list of the chunk loop, with its offers shuffled, against the literal
    re-sort of the whole union; without the visited set too"""
    rng = np.random.default_rng(4711)
    hubs = 0
    for case in range(250):
        D, graph, m, seeds, ef, batch = _fuzz_case(rng)
        a, sa, ba = iref.graph_insert_ref(D, graph, m, seeds, ef, batch)
        b, sb, bb = iref.graph_insert_ref(D, graph, m, seeds, ef, batch, literal=True)
        c, sc, _ = iref.graph_insert_ref(D, graph, m, seeds, ef, batch, rng=np.random.default_rng(case))
        e, se, _ = iref.graph_insert_ref(D, graph, m, seeds, ef, batch, visited=False)
        assert _same(a, b) and _same(a, c) and _same(a, e), case
        assert sa == sb == sc == se and ba == bb, case
        chunks, offered, accepted = sa
        assert chunks == -(-m // batch) and accepted <= offered and ba[0] <= ba[1], case
        hubs += offered > accepted
    assert hubs > 50                      # offers that lost against what the row held


# ------------------------------------------------------------------ the restatement on the golden data
K = 10


@pytest.fixture(scope="module")
def golden():
    """the 1000 x 16 golden rows under L2: the exact 10-NN graph of the first 800 and of all 1000, 16
    random seeds among the old rows per new row, and the queries of test_graph_search_host.py (200
    perturbed stored rows, 16 random seeds each) with their true neighbours"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "forest_dense_1000x16.npz"))
    X = z["X"]
    N, n = X.shape[0], 800
    D = iref.pair_matrix(X, "l2")
    old = mref.exact_graph(D[:n, :n], K)
    full = mref.exact_graph(D, K)
    iseeds = np.stack([np.random.default_rng(1000 + i).choice(n, 16, replace=False) for i in range(N - n)]).astype(np.int32)
    rng = np.random.default_rng(2024)
    rows = rng.choice(N, 200, replace=False)
    Q = X[rows] + 0.1 * rng.standard_normal((200, X.shape[1]))
    qseeds = np.stack([np.random.default_rng(qi).choice(N, 16, replace=False) for qi in range(200)]).astype(np.int32)
    DQ = sref.query_matrix(X, Q, "l2")
    truth = np.stack([np.lexsort((np.arange(N), DQ[i]))[:K] for i in range(200)])
    return X, D, old, full, iseeds, (Q, qseeds, DQ, truth)


_runs = {}


def _inserted(golden, ef, batch):
    """one restatement per (ef, batch), shared by the tests below and left unchanged"""
    if (ef, batch) not in _runs:
        X, D, old, full, iseeds, _ = golden
        _runs[ef, batch] = iref.graph_insert_ref(D, old, 200, iseeds, ef, batch)
    return _runs[ef, batch]


def test_the_symmetric_folds_are_symmetric(golden):
    X, D, *_ = golden
    assert np.array_equal(sref.bits(D), sref.bits(D.T))
    assert np.array_equal(sref.bits(D), sref.bits(mref.metric_matrix(X, "l2")))
    for metric in ("cosine", "inner"):
        Dm = iref.pair_matrix(X[:100], metric)
        assert np.array_equal(sref.bits(Dm), sref.bits(Dm.T)), metric


def test_one_chunk_is_the_search_of_the_old_graph(golden):
    """(b) batch >= m: the new rows are graph_search_ref's answers with k = kg on the old graph"""
    X, D, old, full, iseeds, _ = golden
    n, m = 800, 200
    for batch in (m, m + 5):
        got, (chunks, offered, accepted), (lo, hi) = (_inserted(golden, 32, m) if batch == m else
                                                      iref.graph_insert_ref(D, old, m, iseeds, 32, batch))
        want, _, o, u = sref.graph_search_ref(X[:n], X[n:], old[0], old[2], iseeds, K, 32, D=D[n:, :n])
        iref.assert_same_graph(tuple(a[n:] for a in got), want, "batch %d" % batch)
        assert chunks == 1 and offered == int(want[2].sum()) and (lo, hi) == (o, u)
        assert 0 < accepted < offered
    # the old rows: untouched ones verbatim, touched ones hold a new id
    got = _inserted(golden, 32, m)[0]
    changed = np.flatnonzero((got[0][:n] != old[0]).any(axis=1))
    named = np.unique(got[0][n:][got[0][n:] >= 0])
    assert set(changed.tolist()) <= set(named.tolist()) and len(changed) > 50
    assert all((got[0][o] >= n).any() for o in changed)


def test_one_call_is_the_sequence_of_single_chunk_calls(golden):
    """(c) batch = b in one call against one single-chunk call per chunk over the growing prefix"""
    X, D, old, full, iseeds, _ = golden
    n, m, b = 800, 200, 70                                  # chunks of 70, 70 and 60 rows
    want, stats, bounds = iref.graph_insert_ref(D, old, m, iseeds, 32, b)
    g, tot, lohi = old, [0, 0, 0], [0, 0]
    for v in range(n, n + m, b):
        cnt = min(b, n + m - v)
        g, s, lh = iref.graph_insert_ref(D[:v + cnt, :v + cnt], g, cnt, iseeds[v - n:v - n + cnt], 32, cnt)
        assert s[0] == 1
        tot = [tot[0] + s[0], tot[1] + s[1], tot[2] + s[2]]
        lohi = [lohi[0] + lh[0], lohi[1] + lh[1]]
    iref.assert_same_graph(g, want, "chunks of %d" % b)
    assert tuple(tot) == stats == (3, stats[1], stats[2]) and tuple(lohi) == bounds
    # rows of one chunk do not see each other; rows of a later chunk see the earlier ones
    ids = want[0]
    last = n + 2 * b
    assert (ids[last:] < last).all() and (ids[n + b:] >= n).any()
    assert (_inserted(golden, 32, m)[0][0][n:] < n).all()


@pytest.mark.parametrize("batch", [1, 50, 200])
def test_every_stored_distance_is_the_fold_of_its_two_rows(golden, batch):
    """(d) and the rows are strictly sorted by (distance, id): no self entry, no id twice"""
    X, D, *_ = golden
    (ids, dist, cnt), _, _ = _inserted(golden, 32, batch)
    N = ids.shape[0]
    assert cnt.min() >= 1 and cnt.max() <= K
    for i in range(N):
        c = int(cnt[i])
        row = ids[i, :c]
        assert np.array_equal(sref.bits(dist[i, :c]), sref.bits(D[i, row])), i
        keys = [sref.key(d, j) for d, j in zip(dist[i, :c].tolist(), row.tolist())]
        assert all(a < b for a, b in zip(keys, keys[1:])), i
        assert i not in row and len(set(row.tolist())) == c, i
        assert (ids[i, c:] == -1).all() and np.isposinf(dist[i, c:]).all()


def test_no_new_rows_is_the_identity(golden):
    """(e)"""
    X, D, old, *_ = golden
    got, stats, bounds = iref.graph_insert_ref(D[:800, :800], old, 0, np.zeros((0, 16), dtype=np.int32), 32, 50)
    iref.assert_same_graph(got, old, "m = 0")
    assert stats == (0, 0, 0) and bounds == (0, 0)
    junk = (np.array([[5, -1, 99]], dtype=np.int32), np.array([[np.nan, 2.0, 1.0]]), np.array([7], dtype=np.int32))
    got, _, _ = iref.graph_insert_ref(np.zeros((1, 1)), junk, 0, np.zeros((0, 1), dtype=np.int32), 3, 1)
    iref.assert_same_graph(got, junk, "m = 0, a junk row is copied as it is")


def _search_recall(golden, graph, ef=32):
    Q, qseeds, DQ, truth = golden[5]
    N = DQ.shape[1]
    (ids, _, cnt), _, _, _ = sref.graph_search_ref(np.zeros((N, 1)), Q, graph[0], graph[2], qseeds, K, ef, D=DQ)
    new = truth >= 800
    hit = np.array([[t in ids[i, :cnt[i]] for t in truth[i]] for i in range(len(truth))])
    return hit.mean(), hit[new].mean(), int(new.sum())


def test_recall_of_the_grown_graph_against_the_exact_graph_of_all_rows(golden):
    """(f) the exact 10-NN graph of the first 800 golden rows, the last 200 inserted at ef 32 from 16
    random seeds in chunks of 50; 200 perturbed stored rows searched at ef 32 from 16 random seeds.
    The yardstick is the exact 10-NN graph of all 1000 rows under the same queries, seeds and ef; the
    grown graph may be at most 0.02 below it."""
    X, D, old, full, iseeds, _ = golden
    ref_all, ref_new, n_new = _search_recall(golden, full)
    print("\nrecall@10 of 200 queries at ef 32 (among the %d true neighbours that are new rows)" % n_new)
    print("exact 10-NN graph of all 1000 rows: %.4f (%.4f)" % (ref_all, ref_new))
    print("inserted at ef (rows) in chunks of (columns)    1       10       50      200")
    table = {}
    for ef in (10, 32, 64):
        for batch in (1, 10, 50, 200):
            graph, stats, _ = _inserted(golden, ef, batch)
            table[ef, batch] = _search_recall(golden, graph)
        print("ef %2d  " % ef + "  ".join("%.4f (%.4f)" % table[ef, b][:2] for b in (1, 10, 50, 200)))
    got_all, got_new, _ = table[32, 50]
    assert got_all >= ref_all - 0.02, (got_all, ref_all)
