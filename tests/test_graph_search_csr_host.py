"""The beam search over the kNN graph on SVector (CSR) rows (rpt_graph_search_csr_*) is declared at
every layer, the union fold its kernel rests on equals the dense fold bit for bit for queries
against rows, and the restatement behaves as a beam search should on sparse rows (no GPU)."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_graph_csr_ref as cref  # noqa: E402
import graph_search_ref as sref  # noqa: E402
import graph_search_csr_ref as scref  # noqa: E402
from test_knn_graph_csr_host import awkward_set  # noqa: E402

HEADER = open(os.path.join(ROOT, "include", "rptree_hip.h")).read()


def _decl(name):
    m = re.search(r"int32_t\s+%s\s*\(([^;]*)\)\s*;" % name, HEADER)
    assert m, name
    return re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)


def _words(decl):
    return [re.sub(r"\s+", " ", a.strip()) for a in decl.split(",")]


def test_header_declares_the_entry_points():
    dev = _words(_decl("rpt_graph_search_csr_dev"))
    assert dev == _words(_decl("rpt_graph_search_dev")) and len(dev) == 15
    host = _words(_decl("rpt_graph_search_csr_host"))
    assert host == _words(_decl("rpt_graph_search_host")) == [w.replace("_dev", "_host") for w in dev]
    assert re.search(r"#define\s+RPT_ABI_VERSION\s+1\b", HEADER)
    comment = HEADER[HEADER.index("query the kNN graph on SVector (CSR) rows"):
                     HEADER.index("int32_t rpt_graph_search_csr_dev")]
    flat = re.sub(r"\s*\n \*\s*", " ", comment)
    for phrase in ("absent columns are +0.0", "widened exactly", "a stored zero is a zero", "word for word",
                   "metricDDL2's left fold over dense(q), dense(x_v)", "no FMA", "one sqrt",
                   "NaN behind every number", "id -1, distance +inf", "at most n expansions",
                   "any ascending superset of the union of the two supports", "bit-equal",
                   "rpt_graph_search_last serves both", "graph_search_csr_stream", "RPT_E_UNSUPPORTED",
                   "RPT_E_ARG", "names rpt_graph_search_*", "stays in bounds and terminates", "class 3",
                   "rpt_knn_last_*"):
        assert phrase in flat, phrase
    options = HEADER[HEADER.index("Algorithm switches of a context"):HEADER.index("int32_t rpt_ctx_set_option")]
    assert "graph_search_csr_stream" in options
    api = open(os.path.join(ROOT, "rp-tree_amd", "csrc", "api.hip")).read()
    assert '{"graph_search_csr_stream", &rpt_options::graph_search_csr_stream}' in api


def test_ctypes_table_and_python_mirror():
    import rptree_amd as rp
    from rptree_amd import _lib
    assert _lib.SYMBOLS["rpt_graph_search_csr_dev"] == _lib.SYMBOLS["rpt_graph_search_dev"]
    assert _lib.SYMBOLS["rpt_graph_search_csr_host"] == _lib.SYMBOLS["rpt_graph_search_host"]
    L = _lib.lib()
    for name in ("rpt_graph_search_csr_dev", "rpt_graph_search_csr_host"):
        assert hasattr(L, name), name
    for name in ("graphSearchSV", "graphSearchSVDev"):
        assert name in rp.__all__ and callable(getattr(rp, name))
    sv = inspect.signature(rp.graphSearchSV).parameters
    assert list(sv) == ["graph", "data", "qs", "k", "ef", "seeds", "forest", "seed_k", "ctx"]
    assert [sv[p].default for p in ("ef", "seeds", "forest", "seed_k", "ctx")] == [None, None, None, 8, None]
    dense = list(inspect.signature(rp.graphSearch).parameters)
    assert [p for p in dense if p != "metric"] == list(sv)
    assert list(inspect.signature(rp.graphSearchSVDev).parameters) == [
        "data", "queries", "kg", "gids_ptr", "gcount_ptr", "s", "seeds_ptr", "k", "ef", "ids_ptr", "dist_ptr",
        "count_ptr"]
    assert [p for p in inspect.signature(rp.graphSearchDev).parameters if p != "metric"] == list(
        inspect.signature(rp.graphSearchSVDev).parameters)


def test_other_layers_name_it():
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "graph_search_csr_stream" in readme and "graphSearchSV" in readme
    assert "graph_search_csr_times" in readme
    hpp = open(os.path.join(ROOT, "rp-tree_amd", "host", "rptree.hpp")).read()
    assert "rpt_graph_search_csr_host" in hpp and len(re.findall(r"\bgraphSearchSV\(", hpp)) >= 2
    assert os.path.exists(os.path.join(ROOT, "rp-tree_amd", "host", "example_graph_search_sparse.cpp"))
    assert "example_graph_search_sparse" in open(os.path.join(ROOT, "rp-tree_amd", "host", "Makefile")).read()
    hs = open(os.path.join(ROOT, "haskell", "Data", "RPTree", "HIP.hs")).read()
    assert "graphSearchSVHIP" in hs and "rpt_graph_search_csr_host" in hs
    assert "rpt_graph_search_csr_host" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "graph_search_csr_kernel" in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert os.path.exists(os.path.join(ROOT, "tools", "graph_search_csr_times.py"))
    # one definition of the beam, shared by the dense and the CSR kernel
    csrc = os.path.join(ROOT, "rp-tree_amd", "csrc")
    dev = open(os.path.join(csrc, "graph_dev.h")).read()
    for src in ("graph_search.hip", "graph_search_csr.hip"):
        text = open(os.path.join(csrc, src)).read()
        for fn in ("beam_next_offer", "beam_admit", "beam_insert", "beam_answer"):
            assert fn + "(" in text and not re.search(r"\b(?:void|bool|int) %s\(" % fn, text), (src, fn)
            assert len(re.findall(r"\b(?:void|bool|int) %s\(" % fn, dev)) == 1, fn
    make = open(os.path.join(ROOT, "rp-tree_amd", "Makefile")).read()
    assert "csrc/graph_search_csr.hip" in make


# ------------------------------------------------------------------ the union fold, queries against rows
def awkward_queries():
    """40 queries over 70 columns: an empty one, stored rows themselves, nothing but a stored -0.0,
    only column 0, only column 69, a full one, an inf and a NaN entry"""
    X = cref.rows_of(awkward_set())
    rows = [(c.copy(), v.copy()) for c, v in cref.rows_of(cref.make_csr(43, 40, 70, 0.2))]
    rows[0] = (np.zeros(0, dtype=np.int32), np.zeros(0))
    rows[1] = X[17]                                         # a stored row with duplicates under other ids
    rows[2] = X[20]                                         # the row of stored +0.0 and -0.0
    rows[3] = (np.array([5], dtype=np.int32), np.array([-0.0]))
    rows[4] = (np.array([0], dtype=np.int32), np.array([1.5]))
    rows[5] = (np.array([69], dtype=np.int32), np.array([-2.5]))
    rows[6] = (np.arange(70, dtype=np.int32), np.random.default_rng(6).standard_normal(70))
    rows[7] = (rows[7][0], np.concatenate([[np.inf], rows[7][1][1:]]))
    rows[8] = (rows[8][0], np.concatenate([rows[8][1][:-1], [np.nan]]))
    rows[9] = X[30]                                         # the stored row with an inf
    rows[10] = X[0]                                         # a stored empty row
    assert len(rows[7][0]) > 1 and len(rows[8][0]) > 1
    return cref.from_rows(rows, 70)


def test_union_fold_equals_the_dense_fold_for_awkward_queries():
    csrX, csrQ = awkward_set(), awkward_queries()
    want = sref.query_matrix(cref.densify(csrX), cref.densify(csrQ), "l2")
    got = scref.query_matrix_csr(csrX, csrQ)
    assert got.shape == (40, 200)
    assert int((scref.bits(got) != scref.bits(want)).sum()) == 0
    assert got[0, 0] == 0.0 and got[0, 21] == 0.0 and got[3, 13] == 0.0      # nothing against nothing
    assert got[1, 17] == 0.0 and got[1, 5] == 0.0 and got[1, 150] == 0.0     # a stored row and its duplicates
    assert np.isnan(got[8]).all() and np.isnan(got[:, 31]).all()
    assert not np.signbit(got[np.isfinite(got)]).any()


@pytest.fixture(scope="module")
def golden():
    """the sparse golden rows, their exact 10-NN graph, 200 stored rows with perturbed stored values
    as queries, 16 random seeds each, the queries' distances and true neighbours"""
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
    gids, _, gcnt = cref.exact_graph(X, 10)
    seeds = np.stack([np.random.default_rng(qi).choice(n, 16, replace=False) for qi in range(200)]).astype(np.int32)
    truth = np.stack([np.lexsort((np.arange(n), D[i]))[:10] for i in range(200)])
    return csrX, csrQ, D, gids, gcnt, seeds, truth


def test_union_fold_equals_the_dense_fold_on_the_golden_rows(golden):
    csrX, csrQ, D, _, _, _, _ = golden
    got = scref.query_matrix_csr(csrX, csrQ)                # all 120 000 pairs
    assert got.shape == D.shape == (200, 600)
    assert int((scref.bits(got) != scref.bits(D)).sum()) == 0


def test_restatement_on_the_golden_rows(golden):
    """the visited set changes no beam; answers are sorted, duplicate-free, padded and no worse than
    the seeds; recall@10 from random seeds on the raw exact graph is printed, not bounded (sparse
    random rows are hub-heavy and the raw graph is directed: what the preparation step is for), and
    only must not fall as ef grows"""
    csrX, csrQ, D, gids, gcnt, seeds, truth = golden
    K, nq = 10, D.shape[0]
    recalls = []
    for ef in (10, 32, 64):
        for i in range(nq):
            drow, srow = D[i].tolist(), seeds[i].tolist()
            assert sref.search_one(drow, gids, gcnt, srow, ef, True) == sref.search_one(drow, gids, gcnt, srow, ef,
                                                                                        False), (ef, i)
        (ids, dist, cnt), exp, off, up = scref.graph_search_csr_ref(csrX, csrQ, gids, gcnt, seeds, K, ef, D=D)
        assert off <= up and exp >= nq
        for i in range(nq):
            c = cnt[i]
            assert 0 < c <= K and len(set(ids[i, :c].tolist())) == c
            assert np.all(ids[i, c:] == -1) and np.all(np.isposinf(dist[i, c:]))
            assert np.array_equal(np.lexsort((ids[i, :c], dist[i, :c])), np.arange(c))
            assert np.array_equal(scref.bits(dist[i, :c]), scref.bits(D[i, ids[i, :c]]))
            assert c == K and dist[i, K - 1] <= np.sort(D[i, seeds[i]])[K - 1]   # the k-th of the seeds alone
        hits = sum(len(set(ids[i].tolist()) & set(truth[i].tolist())) for i in range(nq))
        recalls.append(hits / (K * nq))
    print("sparse 600 x 12, exact 10-NN graph, 16 random seeds: recall@10 %s at ef 10 / 32 / 64"
          % ["%.4f" % r for r in recalls])
    assert recalls[0] <= recalls[1] <= recalls[2], recalls
    # without D the reference folds the dense-ified sets itself: the same answer
    again = scref.graph_search_csr_ref(csrX, csrQ, gids, gcnt, seeds, K, 64)
    scref.assert_same_answer(again[0], (ids, dist, cnt), "D given or not")
    assert again[1:] == (exp, off, up)
