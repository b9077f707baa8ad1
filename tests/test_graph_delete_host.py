"""Deleting rows from a kNN graph (rpt_graph_delete_*) is declared at every layer, and the numpy
restatement that the GPU tests compare with behaves as the header says: its two forms agree, keeping
every row is the identity, no entry names a deleted row, the compact form is the other form through
newid, a second call changes nothing, every new entry stores the fold of its two rows, and a repaired
graph answers queries better than one whose dead entries were merely dropped (no GPU)."""
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
import graph_delete_ref as dref  # noqa: E402

HEADER = open(os.path.join(ROOT, "include", "rptree_hip.h")).read()
NAMES = ("rpt_graph_delete_dev", "rpt_graph_delete_host", "rpt_graph_delete_last")


def _decl(name):
    m = re.search(r"int32_t\s+%s\s*\(([^;]*)\)\s*;" % name, HEADER)
    assert m, name
    return re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)


def _words(decl):
    return [re.sub(r"\s+", " ", a.strip()) for a in decl.split(",")]


# ------------------------------------------------------------------ declarations
def test_header_declares_the_entry_points():
    dev = _words(_decl("rpt_graph_delete_dev"))
    assert dev == ["rpt_ctx* ctx", "const rpt_dataset* data", "int32_t kg", "const int32_t* gids_dev",
                   "const double* gdist_dev", "const int32_t* gcount_dev", "const uint32_t* keep_dev", "int32_t metric",
                   "int32_t flags", "int32_t* oids_dev", "double* odist_dev", "int32_t* ocount_dev", "int32_t* newid_dev"]
    assert _words(_decl("rpt_graph_delete_host")) == [w.replace("_dev", "_host") for w in dev]
    assert _words(_decl("rpt_graph_delete_last")) == ["rpt_ctx* ctx", "int64_t* kept", "int64_t* touched",
                                                      "int64_t* evaluated", "int64_t* dropped"]
    assert re.search(r"#define\s+RPT_ABI_VERSION\s+1\b", HEADER)
    assert re.search(r"#define\s+RPT_GRAPH_DELETE_COMPACT\s+1\b", HEADER)
    # the neighbouring entry points keep their signatures
    assert _decl("rpt_graph_insert_dev").count(",") == 15 and _decl("rpt_graph_search_allow_dev").count(",") == 16


def test_header_comment_states_the_definition():
    comment = HEADER[HEADER.index("delete rows from a kNN graph"):HEADER.index("int32_t rpt_graph_delete_dev")]
    flat = re.sub(r"\s*\n \*\s*", " ", comment)
    for phrase in ("The stored distances ARE read", "read only", "A set bit means the row STAYS", "NULL = every row stays",
                   "bits at positions >= n ignored", "passed unchanged", "0 or RPT_GRAPH_DELETE_COMPACT",
                   "newid[n] (int32; may be NULL)", "Ids are old ids throughout", "clamped to [0, kg]",
                   "is not j", "counts once, at its first slot", "with their STORED distances",
                   "copied slot for slot", "distance bits verbatim", "replaced by newid of it", "the count is verbatim",
                   "e is kept, e != p, e is not an id of K(p)", "K(p) u { (dist(p, e), e) : e in C(p) }",
                   "NaN behind every number", "-0.0 ties with +0.0", "id -1", "+inf", "symmetric bit for bit",
                   "One hop only", "are not followed", "rpt_knn_graph_refine_* round afterwards repairs such rows",
                   "a deleted row has count 0", "newid[i] is i, or -1", "only seeds can reach one",
                   "the number of kept rows below i", "n' = popcount rows", "rows n' .. n of the output arrays are not written",
                   "Compacting the data set is the caller's business", "a pure function of", "every launch shape",
                   "No atomics touch a row and one wave writes it", "graph_delete_general", "Scratch is sized by n alone",
                   "evaluated = the sum of |C(p)|", "dropped = the sum of |D(p)|", "All four are sums",
                   "RPT_E_ARG", "RPT_E_NOMEM", "names the offending row", "does NOT validate",
                   "stays in bounds and terminates", "n = 0, keep = nothing and keep = everything are valid",
                   "A refused call leaves the context usable"):
        assert phrase in flat, phrase
    api = open(os.path.join(ROOT, "rp-tree_amd", "csrc", "api.hip")).read()
    assert "flags must be 0 or RPT_GRAPH_DELETE_COMPACT" in api
    assert '{"graph_delete_general", &rpt_options::graph_delete_general}' in api
    assert "graph_delete_general (0 / 1)" in HEADER


def test_kernel_source_has_one_body_per_step():
    csrc = os.path.join(ROOT, "rp-tree_amd", "csrc")
    src = open(os.path.join(csrc, "graph_delete.hip")).read()
    for kern in ("delete_mark_kernel", "delete_scan_kernel", "delete_copy_kernel", "delete_repair_kernel",
                 "delete_repair_csr_kernel"):
        assert len(re.findall(r"__global__[^;{]*\b%s\(" % kern, src)) == 1, kern
    # the repair reuses the refinement's helpers: no second merge, hash set, staging or fold
    for helper in ("wave_merge(", "set_insert(", "wave_stage<TD>(", "fold_step<M>(", "fold_finish<M>("):
        assert helper in src, helper
    assert '#include "graph_refine_dev.h"' in src and "ensure_sqnorm" in src and "RPT_PROF_GRAPH_DELETE" in src
    assert "graph_delete_general" in src and "hipMemGetInfo" not in src          # scratch by (n, kg), not by free memory
    body = src[src.index("__global__ __launch_bounds__(256) void delete_repair_kernel"):]
    assert not re.search(r"atomic\w*\(&?o(ids|dist|count)", src) and body.count("atomicAdd(&st->evaluated") == 2
    for name in ("graph_refine.hip", "graph_csr.hip", "graph_insert.hip", "graph_search.hip"):
        assert "graph_delete" not in open(os.path.join(csrc, name)).read()
    make = open(os.path.join(ROOT, "rp-tree_amd", "Makefile")).read()
    assert "csrc/graph_delete.hip" in make


def test_ctypes_table_and_python_mirror():
    import rptree_amd as rp
    from rptree_amd import _lib
    assert len(_lib.SYMBOLS["rpt_graph_delete_dev"][1]) == 13 and len(_lib.SYMBOLS["rpt_graph_delete_host"][1]) == 13
    assert len(_lib.SYMBOLS["rpt_graph_delete_last"][1]) == 5
    declared = set(re.findall(r"^\s*(?:int32_t|const char\*)\s+(rpt_\w+)\s*\(", HEADER, flags=re.M))
    assert declared == set(_lib.SYMBOLS)
    assert rp.RPT_GRAPH_DELETE_COMPACT == 1
    for name in ("graphDelete", "graphDeleteDev", "graphDeleteLast", "compactRows"):
        assert name in rp.__all__ and callable(getattr(rp, name))
    sig = inspect.signature(rp.graphDelete)
    assert list(sig.parameters) == ["keep", "graph", "data", "compact", "metric", "ctx"]
    assert sig.parameters["compact"].default is True and sig.parameters["metric"].default is None
    assert list(inspect.signature(rp.graphDeleteDev).parameters) == [
        "data", "kg", "gids_ptr", "gdist_ptr", "gcount_ptr", "keep_ptr", "oids_ptr", "odist_ptr", "ocount_ptr",
        "newid_ptr", "compact", "metric"]
    assert list(inspect.signature(rp.graphDeleteLast).parameters) == ["ctx"]
    assert list(inspect.signature(rp.compactRows).parameters) == ["data", "keep"]
    src = inspect.getsource(rp.graphDelete)
    assert set(re.findall(r"\brpt_\w+_host\b", src)) == {"rpt_graph_delete_host"}       # one body for every layout
    with pytest.raises(NotImplementedError):               # an unknown metric is refused before any handle is touched
        rp.graphDelete(None, None, None, metric=max)


def test_compact_rows_keeps_the_kept_rows():
    import rptree_amd as rp
    rng = np.random.default_rng(1)
    X = rng.standard_normal((70, 3))
    keep = rng.random(70) < 0.6
    assert np.array_equal(rp.compactRows(X, keep), X[keep])
    assert np.array_equal(rp.compactRows(X.astype(np.float32), rp.allowBitmap(keep, 70)), X.astype(np.float32)[keep])
    rowptr = np.array([0, 2, 2, 5, 6], dtype=np.int64)
    col = np.array([0, 3, 1, 2, 4, 0], dtype=np.int32)
    val = np.arange(6, dtype=np.float64)
    out = rp.compactRows((rowptr, col, val, 5), np.array([True, False, True, False]))
    assert out[0].tolist() == [0, 2, 5] and out[1].tolist() == [0, 3, 1, 2, 4] and out[2].tolist() == [0, 1, 2, 3, 4]
    assert out[3] == 5
    with pytest.raises(ValueError):
        rp.compactRows(X, keep[:-1])


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
    assert len(re.findall(r"\brpt_graph_delete_host\b", code)) == 1 and "rpt_graph_delete_last" in code
    assert len(re.findall(r"^inline DeleteResult graphDelete\(", hpp, flags=re.M)) == 2          # one takes a Metric
    host = os.path.join(ROOT, "rp-tree_amd", "host")
    example = open(os.path.join(host, "example_graph_delete.cpp")).read()
    assert "graphDelete(" in example and "graphSearch(" in example and "allowBitmap(" in example
    make = open(os.path.join(host, "Makefile")).read()
    assert re.search(r"^all:.*\bexample_graph_delete\b", make, flags=re.M)
    assert re.search(r"^example_graph_delete: example_graph_delete.cpp rptree.hpp", make, flags=re.M)
    assert re.search(r"^\trm -f .*\bexample_graph_delete\b", make, flags=re.M)
    assert "rp-tree_amd/host/example_graph_delete" in open(os.path.join(ROOT, ".gitignore")).read()
    hs = open(os.path.join(ROOT, "haskell", "Data", "RPTree", "HIP.hs")).read()
    assert hs.count("graphDeleteHIP") >= 3 and "rpt_graph_delete_host" in hs
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "rpt_graph_delete_host" in integ and "rpt_graph_delete_dev" in integ
    readme = open(os.path.join(ROOT, "README.md")).read()
    for word in ("graphDelete", "compactRows", "graph_delete_times", "Not built"):
        assert word in readme, word
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for word in ("delete_repair_kernel", "delete_mark_kernel", "graph_delete_general"):
        assert word in design, word
    assert "graph_delete_times.py" in open(os.path.join(ROOT, "tools", "README.md")).read()
    assert "graph_delete_times.json" in open(os.path.join(ROOT, "profiles", "README.md")).read()
    assert os.path.exists(os.path.join(ROOT, "tools", "graph_delete_times.py"))


# ------------------------------------------------------------------ the restatement, fuzzed
def _fuzz_case(rng):
    """lattice distances (heavy ties, some NaN, -0.0), a junk graph, any keep"""
    n = int(rng.integers(0, 45))
    kg = int(rng.integers(1, 7))
    D = rng.integers(0, 5, size=(n, n)).astype(np.float64)
    D = np.minimum(D, D.T)
    D[D == 0] = rng.choice([0.0, -0.0])
    nan = rng.random((n, n)) < 0.05
    D[nan | nan.T] = np.nan
    gids = rng.integers(-2, n + 3, size=(n, kg)).astype(np.int32)          # junk ids on both sides of [0, n), itself
    gdist = rng.integers(0, 5, size=(n, kg)).astype(np.float64)
    gdist[rng.random((n, kg)) < 0.05] = np.nan
    gcnt = rng.integers(-1, kg + 2, size=n).astype(np.int32)               # junk counts
    keep = rng.random(n) < rng.choice([0.0, 0.3, 0.5, 0.7, 0.9, 0.95, 1.0])
    return D, (gids, gdist, gcnt), keep


def _same(a, b):
    return all(np.array_equal(sref.bits(x), sref.bits(y)) for x, y in zip(a, b))


def test_fuzz_the_two_forms_agree_whatever_the_order():
    """the bounded sorted list that visits D(p) and its rows in a shuffled order against the literal
    re-sort of the whole union, in old ids and compact"""
    rng = np.random.default_rng(4711)
    repaired = shrunk = 0
    for case in range(300):
        D, graph, keep = _fuzz_case(rng)
        for compact in (False, True):
            a, ia, sa = dref.graph_delete_ref(D, graph, keep, compact)
            b, ib, sb = dref.graph_delete_ref(D, graph, keep, compact, literal=True)
            c, ic, sc = dref.graph_delete_ref(D, graph, keep, compact, rng=np.random.default_rng(case))
            assert _same(a, b) and _same(a, c), case
            assert np.array_equal(ia, ib) and np.array_equal(ia, ic) and sa == sb == sc, case
        kept, touched, evaluated, dropped = sa
        assert kept == int(keep.sum()) and touched <= min(kept, dropped) and (touched > 0) == (dropped > 0), case
        repaired += evaluated > 0
        shrunk += touched > 0 and evaluated == 0
        # the words of the bitmap, junk bits behind n included, are the mask
        n = len(keep)
        bits = np.zeros(((n + 31) // 32) * 32, dtype=np.uint8)
        bits[:n] = keep
        bits[n:] = 1
        words = np.packbits(bits, bitorder="little").view("<u4").astype(np.uint32)
        w, iw, sw = dref.graph_delete_ref(D, graph, words, True)
        assert _same(w, a) and np.array_equal(iw, ia) and sw == sa, case
    assert repaired > 100 and shrunk > 5


# ------------------------------------------------------------------ the restatement on the golden data
K = 10
FRACTIONS = (0.05, 0.2, 0.5, 0.8)


@pytest.fixture(scope="module")
def golden():
    """the 1000 x 16 golden rows under L2 with their exact 10-NN graph"""
    X = np.load(os.path.join(ROOT, "tests", "golden", "forest_dense_1000x16.npz"))["X"]
    D = dref.pair_matrix(X, "l2")
    return X, D, mref.exact_graph(D, K)


_runs = {}


def _case(golden, f):
    """per deleted fraction, once: the mask of the issue's sketch, the repaired graph in both forms, the
    drop-only graph and the exact graph of the survivors (compact ids)"""
    if f not in _runs:
        X, D, full = golden
        keep = ~(np.random.default_rng(7).random(X.shape[0]) < f)
        old = dref.graph_delete_ref(D, full, keep, False)
        tight = dref.graph_delete_ref(D, full, keep, True)
        drop = dref.drop_only(full, keep, True)
        exact = mref.exact_graph(D[np.ix_(keep, keep)], K)
        _runs[f] = (keep, old, tight, drop, exact)
    return _runs[f]


def test_keeping_every_row_is_the_identity(golden):
    """(a)"""
    X, D, full = golden
    n = X.shape[0]
    for keep in (None, np.ones(n, dtype=bool)):
        for compact in (False, True):
            got, newid, stats = dref.graph_delete_ref(D, full, keep, compact)
            dref.assert_same_graph(got, full, "keep = all")
            assert np.array_equal(newid, np.arange(n)) and stats == (n, 0, 0, 0)
    junk = (np.array([[5, -1, 0, 0]], dtype=np.int32), np.array([[np.nan, 2.0, 1.0, -0.0]]), np.array([7], dtype=np.int32))
    got, _, _ = dref.graph_delete_ref(np.zeros((1, 1)), junk, None)
    dref.assert_same_graph(got, junk, "an untouched junk row is copied as it is")


@pytest.mark.parametrize("f", FRACTIONS)
def test_no_entry_names_a_deleted_row_and_the_compact_form_is_the_other_through_newid(golden, f):
    """(b), (c)"""
    keep, (og, oid, ostats), (cg, cid, cstats), _, _ = _case(golden, f)
    n = len(keep)
    gone = np.flatnonzero(~keep)
    assert not np.isin(og[0], gone).any() and np.all(og[2][gone] == 0) and np.all(og[0][gone] == -1)
    assert np.all(np.isposinf(og[1][gone]))
    assert np.array_equal(oid, np.where(keep, np.arange(n), -1))
    kept = np.flatnonzero(keep)
    assert np.array_equal(cid[kept], np.arange(len(kept))) and np.all(cid[gone] == -1) and ostats == cstats
    mapped = np.where(og[0][kept] >= 0, cid[np.where(og[0][kept] >= 0, og[0][kept], 0)], -1)
    assert np.array_equal(cg[0], mapped) and np.array_equal(sref.bits(cg[1]), sref.bits(og[1][kept]))
    assert np.array_equal(cg[2], og[2][kept])


@pytest.mark.parametrize("f", FRACTIONS)
def test_a_second_call_touches_no_row_and_changes_no_bit(golden, f):
    """(d)"""
    X, D, full = golden
    keep, (og, oid, ostats), _, _, _ = _case(golden, f)
    again, aid, astats = dref.graph_delete_ref(D, og, keep, False)
    dref.assert_same_graph(again, og, "second call")
    assert np.array_equal(aid, oid) and astats == (ostats[0], 0, 0, 0)


@pytest.mark.parametrize("f", FRACTIONS)
def test_every_entry_is_the_fold_of_its_two_rows(golden, f):
    """(e) new entries and kept ones alike, and the rows are strictly sorted by (distance, id)"""
    X, D, full = golden
    keep, (og, oid, ostats), _, _, _ = _case(golden, f)
    fresh = 0
    for p in np.flatnonzero(keep):
        c = int(og[2][p])
        row = og[0][p, :c]
        assert np.array_equal(sref.bits(og[1][p, :c]), sref.bits(D[p, row])), p
        keys = [sref.key(d, j) for d, j in zip(og[1][p, :c].tolist(), row.tolist())]
        assert all(a < b for a, b in zip(keys, keys[1:])) and p not in row, p
        assert (og[0][p, c:] == -1).all() and np.isposinf(og[1][p, c:]).all()
        fresh += len(set(row.tolist()) - set(full[0][p].tolist()))
    assert 0 < fresh <= ostats[2]


def test_deleting_nothing_from_an_inserted_graph_leaves_it_unchanged(golden):
    """(f) a graph that graph_insert_ref grew"""
    X, D, full = golden
    n, m = 300, 60
    old = mref.exact_graph(D[:n, :n], K)
    seeds = np.stack([np.random.default_rng(i).choice(n, 8, replace=False) for i in range(m)]).astype(np.int32)
    grown, _, _ = iref.graph_insert_ref(D[:n + m, :n + m], old, m, seeds, 32, 16)
    got, newid, stats = dref.graph_delete_ref(D[:n + m, :n + m], grown, np.ones(n + m, dtype=bool), True)
    dref.assert_same_graph(got, grown, "nothing deleted")
    assert stats == (n + m, 0, 0, 0) and np.array_equal(newid, np.arange(n + m))


# ------------------------------------------------------------------ recall
def _graph_recall(graph, exact):
    hit = sum(len(set(a[:c].tolist()) & set(b.tolist())) for a, c, b in zip(graph[0], graph[2], exact[0]))
    return hit / float(exact[0].size)


def _queries(X, keep):
    """the queries and seeds of test_graph_search_host.py, re-drawn among the survivors: up to 200
    perturbed stored rows, 16 random seeds each (compact ids)"""
    Xs = X[keep]
    ns = Xs.shape[0]
    nq = min(200, ns)
    rng = np.random.default_rng(2024)
    rows = rng.choice(ns, nq, replace=False)
    Q = Xs[rows] + 0.1 * rng.standard_normal((nq, X.shape[1]))
    qseeds = np.stack([np.random.default_rng(qi).choice(ns, 16, replace=False) for qi in range(nq)]).astype(np.int32)
    DQ = sref.query_matrix(Xs, Q, "l2")
    truth = np.stack([np.lexsort((np.arange(ns), DQ[i]))[:K] for i in range(nq)])
    return Q, qseeds, DQ, truth


def _search_recall(graph, queries, ef=32):
    Q, qseeds, DQ, truth = queries
    ns = DQ.shape[1]
    (ids, _, cnt), _, _, _ = sref.graph_search_ref(np.zeros((ns, 1)), Q, graph[0], graph[2], qseeds, K, ef, D=DQ)
    hit = sum(len(set(a[:c].tolist()) & set(t.tolist())) for a, c, t in zip(ids, cnt, truth))
    return hit / float(truth.size)


_table = {}


def _row(golden, f):
    if f not in _table:
        X, D, full = golden
        keep, (og, _, stats), (cg, _, _), (dg, _, _), exact = _case(golden, f)
        q = _queries(X, keep)
        _table[f] = dict(graph=(_graph_recall(dg, exact), _graph_recall(cg, exact)),
                         degree=(dg[2].mean(), cg[2].mean()),
                         search=(_search_recall(dg, q), _search_recall(cg, q), _search_recall(exact, q)),
                         evaluated=stats[2], touched=stats[1], queries=len(q[0]))
    return _table[f]


def test_recall_table_of_the_repaired_graph(golden):
    """The exact 10-NN graph of the 1000 golden rows, rows deleted with the mask
    np.random.default_rng(7).random(1000) < f; "drop" removes the dead entries only, "repair" is the
    definition, "exact" the exact 10-NN graph of the survivors; the search is graph_search_ref at ef 32
    over the compacted survivors.  Measured with the folds (this table is the README's):
      deleted  graph recall drop/repair  degree drop/repair  search recall@10 drop/repair/exact  candidates
        5 %    0.9536 / 0.9629           9.54 / 10.00        0.9525 / 0.9555 / 0.9575            3 344
       20 %    0.7863 / 0.8615           7.86 / 10.00        0.9360 / 0.9555 / 0.9680            9 708
       50 %    0.5056 / 0.7382           5.06 / 10.00        0.8745 / 0.9515 / 0.9805            7 823
       80 %    0.2010 / 0.5898           2.01 /  9.54        0.6447 / 0.9157 / 0.9909            1 899
    (200 queries; 197 at 80 %, where 197 rows survive.)
    Asserted: at every f the repaired graph's recall against the exact graph of the survivors is strictly
    above drop-only's and its search recall is not below drop-only's; at f = 0.2 it is at most 0.02
    below the exact graph of the survivors (the margin the sketch behind the feature set: twice its own
    shortfall of 0.0095)."""
    print("\ndeleted | graph recall drop / repair | mean degree drop / repair | search recall@10 at ef 32: "
          "drop / repair / exact | candidates evaluated | touched rows | queries")
    for f in FRACTIONS:
        r = _row(golden, f)
        print("%3.0f %% | %.4f / %.4f | %.2f / %.2f | %.4f / %.4f / %.4f | %d | %d | %d" % (
            100 * f, r["graph"][0], r["graph"][1], r["degree"][0], r["degree"][1], r["search"][0], r["search"][1],
            r["search"][2], r["evaluated"], r["touched"], r["queries"]))
    for f in FRACTIONS:
        r = _row(golden, f)
        assert r["graph"][1] > r["graph"][0], (f, r)
        assert r["search"][1] >= r["search"][0], (f, r)
    r = _row(golden, 0.2)
    assert r["search"][1] >= r["search"][2] - 0.02, r
