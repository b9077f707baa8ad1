"""Host side of the vote-threshold kNN (rpt_knn_vote_*, rpt_vote_candidates_host): the numpy
restatement tests/knn_vote_ref.py pinned to the CPU oracle's keepCounts and voting kNN on the
1000 x 16 golden forest, what the threshold does to the lists and to recall there, and the header /
library / ctypes / Python surface.  No GPU needed."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import knn_vote_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "rptree_hip.h")).read()
ENTRY_POINTS = ("rpt_knn_vote_host", "rpt_knn_vote_dev", "rpt_vote_candidates_host", "rpt_knn_last_voted")


@pytest.fixture(scope="module")
def golden(oracle):
    g = np.load(os.path.join(ROOT, "tests", "golden", "forest_dense_1000x16.npz"))
    f = oracle.Forest(int(g["n"]), int(g["d"]), g["R"], int(g["L"]), int(g["min_leaf"]), g["perm"], g["thr"],
                      g["mglo"], g["mghi"])
    return g, f, int(g["T"])


def thresholds(T):
    return sorted({1, 2, 3, T, T + 1})


def test_voted_equals_keep_counts(oracle, golden):
    g, _, T = golden
    off, cids = g["cand_off"], g["cand_ids"]
    for v in thresholds(T):
        for i in range(len(g["Q"])):
            c = cids[off[i * T]:off[(i + 1) * T]]
            wi, wc = oracle.keep_counts(c, v)
            gi, gc = ref.voted(c, v)
            assert np.array_equal(gi, wi) and np.array_equal(gc, wc), (v, i)
        voff, vids, vcnt = ref.voted_batch(off, cids, T, v)
        assert voff[-1] == len(vids) == len(vcnt) and (vcnt >= v).all() and (vcnt <= T).all()


def test_knn_vote_equals_the_oracle(oracle, golden):
    g, f, T = golden
    X, Q, k = g["X"], g["Q"], 10
    for v in thresholds(T):
        wi, wd, wc = oracle.knn_dense_batch(f, X, Q, k, vote_thr=v)
        gi, gd, gc = ref.knn_vote_batch(g["cand_off"], g["cand_ids"], T, v,
                                        lambda i, ids: ref.l2_f64(X[ids], Q[i]), k)
        assert np.array_equal(gc, wc), v
        assert np.array_equal(gi, wi), v
        for i in range(len(Q)):
            assert np.allclose(gd[i, :gc[i]], wd[i, :wc[i]], rtol=1e-12), (v, i)
            assert (gi[i, gc[i]:] == -1).all() and np.isposinf(gd[i, gc[i]:]).all()
        if v == T + 1:
            assert (gc == 0).all()


def test_lists_shrink_as_the_threshold_rises(golden):
    g, _, T = golden
    off, cids = g["cand_off"], g["cand_ids"]
    totals = []
    for v in range(1, T + 2):
        voff, vids, _ = ref.voted_batch(off, cids, T, v)
        totals.append(len(vids))
        if v > 1:
            for i in range(len(voff) - 1):
                assert np.isin(vids[voff[i]:voff[i + 1]], prev[1][prev[0][i]:prev[0][i + 1]]).all(), (v, i)
        prev = (voff, vids)
    assert totals[0] > totals[1] > totals[2] and totals[-1] == 0, totals
    assert totals[0] < len(cids)            # some id is proposed by more than one tree


def test_recall_and_distances_per_query(oracle, golden, capsys):
    """the README's table: recall@10 against the exhaustive search and distances evaluated per query"""
    g, _, T = golden
    X, Q, k = g["X"], g["Q"], 10
    truth = [np.argsort(ref.l2_f64(X, q), kind="stable")[:k] for q in Q]
    rows = []
    for v in (1, 2, 3):
        gi, _, gc = ref.knn_vote_batch(g["cand_off"], g["cand_ids"], T, v,
                                       lambda i, ids: ref.l2_f64(X[ids], Q[i]), k)
        hit = sum(len(np.intersect1d(gi[i, :gc[i]], truth[i])) for i in range(len(Q)))
        nvoted = ref.voted_batch(g["cand_off"], g["cand_ids"], T, v)[0][-1]
        rows.append((v, hit / (k * len(Q)), nvoted / len(Q)))
    with capsys.disabled():
        print("\nvote threshold on the 1000 x 16 golden forest (T = %d, k = %d, %d queries)" % (T, k, len(Q)))
        for v, rec, per in rows:
            print("  v = %d: recall@10 %.3f, %.1f distances per query" % (v, rec, per))
    assert rows[0][1] >= rows[1][1] >= rows[2][1] and rows[0][2] > rows[1][2] > rows[2][2]


def test_header_states_the_definition_and_the_refusals():
    for name in ENTRY_POINTS:
        assert re.search(r"int32_t\s+%s\s*\(" % name, HEADER), name
    flat = re.sub(r"\s*\n\s*\*\s*", " ", HEADER)
    for phrase in ("The voted list is the ids with count >= v, ascending, each once",
                   "the first k of the voted list by (distance, id)",
                   "count[q] = min(k, number of voted ids)",
                   "The RPT_KNN_VOTE flag of rpt_knn_* keeps its fused path and its caps",
                   "v in [1, 65535] (else RPT_E_ARG)",
                   "RPT_KNN_METRIC_REFERENCE on dense data",
                   "any duplicate-rule bit",
                   "a RPT_KNN_VOTE field",
                   "No query is refused for its candidate count",
                   "knn_vote_lds", "knn_vote_slice",
                   "The answer does not depend on either option",
                   "rpt_knn_last_tier and rpt_knn_last_retries read 0"):
        assert phrase in flat, phrase
    # the old flag's own words stay
    assert "Dense data, k <= 64; or-ed into the knn flags: RPT_KNN_VOTE(v), v in [1, 65535]." in HEADER
    assert re.search(r"#define RPT_ABI_VERSION 1\b", HEADER)


def test_header_still_compiles_as_c99():
    gcc = shutil.which("gcc")
    assert gcc, "no gcc"
    pr = subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c",
                         os.path.join(ROOT, "include", "rptree_hip.h")], stdout=subprocess.PIPE,
                        stderr=subprocess.STDOUT)
    assert pr.returncode == 0, pr.stdout.decode()


def test_library_is_built_from_the_new_file_and_exports_the_symbols():
    out = subprocess.run(["make", "-n", "-B", "-C", os.path.join(ROOT, "rp-tree_amd")], stdout=subprocess.PIPE,
                         universal_newlines=True, check=True)
    link = [ln for ln in out.stdout.splitlines() if "-shared" in ln]
    assert len(link) == 1 and "build/knn_vote.o" in link[0], link
    assert any("csrc/knn_vote.hip" in ln and "--offload-arch=gfx950" in ln for ln in out.stdout.splitlines())
    from rptree_amd import _lib
    L = _lib.lib()
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name


def test_ctypes_table_and_python_signatures():
    import rptree_amd as rp
    from rptree_amd import _lib
    i32, i64, vp = _lib.i32, _lib.i64, _lib.vp
    assert _lib.SYMBOLS["rpt_knn_vote_host"] == (i32, [vp, vp, vp, vp, i32, i32, i32, vp, vp, vp])
    assert _lib.SYMBOLS["rpt_knn_vote_dev"] == _lib.SYMBOLS["rpt_knn_vote_host"]
    assert _lib.SYMBOLS["rpt_vote_candidates_host"] == (i32, [vp, vp, vp, i32, vp, vp, vp, i64, _lib.p_i64])
    assert _lib.SYMBOLS["rpt_knn_last_voted"] == _lib.SYMBOLS["rpt_knn_last_candidates"]
    assert list(inspect.signature(rp.knnVote).parameters) == ["k", "forest", "qs", "v", "metric",
                                                              "reference_metric"]
    assert list(inspect.signature(rp.knnVoteDev).parameters) == ["k", "forest", "queries", "v", "ids_ptr",
                                                                 "dist_ptr", "count_ptr", "metric",
                                                                 "reference_metric"]
    assert list(inspect.signature(rp.voteCandidates).parameters) == ["forest", "qs", "v"]
    assert list(inspect.signature(rp.knnVoteLast).parameters) == ["ctx"]
    # knnBatch keeps its signature: the old flag and the new entry points are two routes
    assert list(inspect.signature(rp.knnBatch).parameters) == ["k", "forest", "qs", "dedup", "vote",
                                                               "reference_metric", "metric"]
    for name in ("knnVote", "knnVoteDev", "voteCandidates", "knnVoteLast"):
        assert name in rp.__all__, name


def test_other_layers_name_it():
    hpp = open(os.path.join(ROOT, "rp-tree_amd", "host", "rptree.hpp")).read()
    assert "rpt_knn_vote_host" in hpp and "knnVote" in hpp and "voteCandidates" in hpp
    assert os.path.exists(os.path.join(ROOT, "rp-tree_amd", "host", "example_knn_vote.cpp"))
    assert "example_knn_vote" in open(os.path.join(ROOT, "rp-tree_amd", "host", "Makefile")).read()
    hs = open(os.path.join(ROOT, "haskell", "Data", "RPTree", "HIP.hs")).read()
    assert "knnVoteHIP" in hs and "voteCandidatesHIP" in hs and "rpt_knn_vote_host" in hs
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "rpt_knn_vote" in open(os.path.join(ROOT, doc)).read(), doc
