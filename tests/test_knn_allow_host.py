"""Host side of the allow-list on the forest query and on the exhaustive kNN (rpt_knn_allow_*,
rpt_allow_candidates_host, rpt_brute_knn_allow_*, rpt_recall_hits_allow_host): the numpy restatement
tests/knn_allow_ref.py pinned to the golden answers of the 1000 x 16 forest, the order of filter and
duplicate rule, what the filter does to recall there, and the header / library / ctypes / Python
surface.  No GPU needed."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import knn_allow_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "rptree_hip.h")).read()
ENTRY_POINTS = ("rpt_knn_allow_host", "rpt_knn_allow_dev", "rpt_allow_candidates_host", "rpt_brute_knn_allow_host",
                "rpt_brute_knn_allow_dev", "rpt_recall_hits_allow_host", "rpt_knn_allow_last")
FRACTIONS = (1.0, 0.5, 0.1, 0.02)
# the README's table: (allowed, filter then take k: recall, answers / query, take k then filter: recall, answers / query)
TABLE = ((1.0, 0.3656, 10.0, 0.3656, 10.0), (0.5, 0.2938, 10.0, 0.2906, 4.84), (0.1, 0.1906, 4.34, 0.0844, 0.84),
         (0.02, 0.0656, 0.66, 0.0063, 0.06))


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "forest_dense_1000x16.npz"))
    X, Q = g["X"], g["Q"]
    return g, int(g["T"]), (lambda i, ids: ref.l2_f64(X[ids], Q[i]))


def mask_of(f, n=1000):
    return np.random.default_rng(7).random(n) < f


def test_every_id_allowed_is_the_golden_answer(golden):
    g, T, dist = golden
    every = np.ones(int(g["n"]), dtype=bool)
    off, cids = g["cand_off"], g["cand_ids"]
    aoff, aids = ref.allowed_batch(off, cids, T, every)
    assert np.array_equal(aoff, off[::T]) and np.array_equal(aids, cids)
    gi, gd, gc = ref.batch(ref.knn_allow, off, cids, T, every, dist, 10, ref.KEEP)
    assert np.array_equal(gi, g["knn_ids"]) and (gc == 10).all()
    assert np.allclose(gd, g["knn_dist"], rtol=1e-12)
    gi, _, _ = ref.batch(ref.knn_allow, off, cids, T, every, dist, 10, ref.EACH_ID_ONCE)
    assert np.array_equal(gi, g["knn_ids_dedup"])


def test_filter_then_rank_equals_rank_then_filter(golden):
    g, T, dist = golden
    off, cids = g["cand_off"], g["cand_ids"]
    for f in FRACTIONS:
        mask = mask_of(f)
        aoff, aids = ref.allowed_batch(off, cids, T, mask)
        assert mask[aids].all() and aoff[-1] == len(aids) == int(mask[cids].sum())
        for rule in ref.RULES:          # the rule is applied after the filter in both
            a = ref.batch(ref.knn_allow, off, cids, T, mask, dist, 10, rule)
            b = ref.batch(ref.knn_rank_then_filter, off, cids, T, mask, dist, 10, rule)
            assert np.array_equal(a[0], b[0]) and ref.same_bits(a[1], b[1]) and np.array_equal(a[2], b[2]), (f, rule)
        for rule in (ref.KEEP, ref.EACH_ID_ONCE):   # these two rules commute with the filter as well
            a = ref.batch(ref.knn_allow, off, cids, T, mask, dist, 10, rule)
            c = ref.batch(ref.knn_rule_then_filter, off, cids, T, mask, dist, 10, rule)
            assert np.array_equal(a[0], c[0]) and np.array_equal(a[2], c[2]), (f, rule)


def test_one_per_distance_does_not_commute_with_the_filter():
    """rows 0 and 1 lie at the same distance, row 0 first in the list and not allowed: nub before the
    filter keeps row 0 for that distance and the filter then drops it: row 1 is lost"""
    cands = np.array([0, 1, 2], dtype=np.int32)
    dv = np.array([1.0, 1.0, 2.0])
    mask = np.array([False, True, True])
    distance = lambda ids: dv[ids]
    oi, od, cnt = ref.knn_allow(cands, mask, distance, 3, ref.ONE_PER_DISTANCE)
    assert cnt == 2 and oi.tolist() == [1, 2, -1] and od[:2].tolist() == [1.0, 2.0] and np.isposinf(od[2])
    wi, _, wcnt = ref.knn_rule_then_filter(cands, mask, distance, 3, ref.ONE_PER_DISTANCE)
    assert wcnt == 1 and wi.tolist() == [2, -1, -1]
    ri, _, rcnt = ref.knn_rank_then_filter(cands, mask, distance, 3, ref.ONE_PER_DISTANCE)
    assert rcnt == 2 and ri.tolist() == [1, 2, -1]


def test_recall_under_a_filter(golden, capsys):
    """the README's table: recall@10 against the 10 nearest ALLOWED rows and answers per query, each
    id once, for the filtered query and for today's route (take k, then filter)"""
    g, T, dist = golden
    X, Q, k = g["X"], g["Q"], 10
    off, cids = g["cand_off"], g["cand_ids"]
    rows = []
    for f in FRACTIONS:
        mask = mask_of(f)
        truth = [ref.brute_allow(ref.l2_f64(X, q), mask, k)[0] for q in Q]
        row = [f]
        for fn in (ref.knn_allow, ref.knn_take_k_then_filter):
            gi, _, gc = ref.batch(fn, off, cids, T, mask, dist, k, ref.EACH_ID_ONCE)
            hit = sum(len(np.intersect1d(gi[i, :gc[i]], truth[i][truth[i] >= 0])) for i in range(len(Q)))
            row += [hit / (k * len(Q)), float(gc.mean())]
        rows.append(row)
    with capsys.disabled():
        print("\nallow-list on the 1000 x 16 golden forest (T = %d, k = %d, %d queries)" % (T, k, len(Q)))
        for f, r1, a1, r2, a2 in rows:
            print("  %5.1f %% allowed: filter then take k: recall %.4f, %.2f answers/query; take k then filter: "
                  "recall %.4f, %.2f answers/query" % (100 * f, r1, a1, r2, a2))
    for (f, r1, a1, r2, a2), want in zip(rows, TABLE):
        assert r1 >= r2, f
        assert (round(r1, 4), round(a1, 2), round(r2, 4), round(a2, 2)) == want[1:], (f, r1, a1, r2, a2)
    assert rows[0][1] == rows[0][3] and rows[0][2] == rows[0][4]      # 100 %: the same answer
    assert rows[2][1] > rows[2][3]                                    # 10 %: strictly above


def test_bitmap_words():
    mask = mask_of(0.5, 600)
    w = ref.bitmap(mask)
    assert w.dtype == np.uint32 and w.shape == (19,)
    assert all(bool((w[i >> 5] >> np.uint32(i & 31)) & np.uint32(1)) == bool(mask[i]) for i in range(600))
    wt = ref.bitmap(mask, tail=True)
    assert np.array_equal(wt[:-1], w[:-1]) and wt[-1] == w[-1] | np.uint32(0xff000000)


def test_header_states_the_definition_and_the_refusals():
    for name in ENTRY_POINTS:
        assert re.search(r"int32_t\s+%s\s*\(" % name, HEADER), name
    flat = re.sub(r"\s*\n\s*\*\s*", " ", HEADER)
    for phrase in ("ceil(n / 32) uint32 words", "id i is bit i & 31 of word i >> 5",
                   "bits at positions >= n are ignored", "NULL means every id", "one bitmap serves the batch",
                   "trees ascending, leaves left to right, duplicates kept",
                   "The allowed list is that list with every entry whose id is not allowed removed, in the same order",
                   "the k best by (distance, position in the allowed list) under the duplicate rule",
                   "NaN ranks last", "count = min(k, entries the rule leaves)",
                   "unused slots are id -1, distance +inf",
                   "The duplicate rule applies after the filter",
                   "with every id allowed the answer is rpt_knn_*'s, bit for bit",
                   "rank the whole candidate list, then drop disallowed entries, then apply the rule and cut to k",
                   "the k best allowed rows by (distance, id)",
                   "except true L2 on CSR rows",
                   "One entry point routes every cell",
                   "A RPT_KNN_VOTE field is RPT_E_UNSUPPORTED",
                   "RPT_KNN_METRIC_REFERENCE on dense rows",
                   "knn_allow_slice", "never from the free memory",
                   "rpt_knn_last_uncertified serves these calls; rpt_knn_last_tier / _retries read 0",
                   "Not built: a bitmap per query", "the fused kernels under a filter", "rpt_knnh_host"):
        assert phrase in flat, phrase
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
    assert len(link) == 1 and "build/knn_allow.o" in link[0], link
    assert any("csrc/knn_allow.hip" in ln and "--offload-arch=gfx950" in ln for ln in out.stdout.splitlines())
    from rptree_amd import _lib
    L = _lib.lib()
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name


def test_ctypes_table_and_python_signatures():
    import rptree_amd as rp
    from rptree_amd import _lib
    i32, i64, vp, p_i64 = _lib.i32, _lib.i64, _lib.vp, _lib.p_i64
    assert _lib.SYMBOLS["rpt_knn_allow_host"] == (i32, [vp, vp, vp, vp, vp, i32, i32, vp, vp, vp])
    assert _lib.SYMBOLS["rpt_knn_allow_dev"] == _lib.SYMBOLS["rpt_knn_allow_host"]
    assert _lib.SYMBOLS["rpt_allow_candidates_host"] == (i32, [vp, vp, vp, vp, vp, vp, i64, p_i64])
    assert _lib.SYMBOLS["rpt_brute_knn_allow_host"] == (i32, [vp, vp, vp, vp, i32, i32, vp, vp])
    assert _lib.SYMBOLS["rpt_brute_knn_allow_dev"] == _lib.SYMBOLS["rpt_brute_knn_allow_host"]
    assert _lib.SYMBOLS["rpt_recall_hits_allow_host"] == (i32, [vp, vp, vp, vp, vp, i32, i32, vp, vp])
    assert _lib.SYMBOLS["rpt_knn_allow_last"] == (i32, [vp, p_i64, p_i64])
    params = lambda fn: list(inspect.signature(fn).parameters)
    assert params(rp.knnAllow) == ["allow", "k", "forest", "qs", "dedup", "metric", "reference_metric"]
    assert params(rp.knnAllowDev) == ["allow_ptr", "k", "forest", "queries", "ids_ptr", "dist_ptr", "count_ptr",
                                      "dedup", "metric", "reference_metric"]
    assert params(rp.allowCandidates) == ["allow", "forest", "qs"]
    assert params(rp.bruteKnnAllow) == ["allow", "forest_or_data", "qs", "k", "ctx", "metric", "reference_metric"]
    assert params(rp.bruteKnnAllowDev)[:2] == ["allow_ptr", "data"]
    assert params(rp.recallHitsAllow) == ["allow", "distf", "forest", "k", "qs", "reference_metric"]
    assert params(rp.recallWithAllowBatch) == ["allow", "distf", "forest", "k", "qs", "reference_metric"]
    assert params(rp.knnAllowLast) == ["ctx"]
    # the unfiltered functions keep their signatures
    assert params(rp.knnBatch) == ["k", "forest", "qs", "dedup", "vote", "reference_metric", "metric"]
    assert params(rp.bruteKnn) == ["forest_or_data", "qs", "k", "ctx", "metric", "reference_metric"]
    assert params(rp.recallHits) == ["distf", "forest", "k", "qs", "reference_metric"]
    assert params(rp.graphSearchAllow) == ["allow", "graph", "data", "qs", "k", "ef", "width", "seeds", "forest",
                                           "seed_k", "metric", "ctx"]
    for name in ("knnAllow", "knnAllowDev", "allowCandidates", "knnAllowLast", "bruteKnnAllow", "bruteKnnAllowDev",
                 "recallHitsAllow", "recallWithAllowBatch"):
        assert name in rp.__all__, name


def test_other_layers_name_it():
    hpp = open(os.path.join(ROOT, "rp-tree_amd", "host", "rptree.hpp")).read()
    for word in ("rpt_knn_allow_host", "knnAllow", "allowCandidates", "bruteKnnAllow", "recallHitsAllow"):
        assert word in hpp, word
    assert os.path.exists(os.path.join(ROOT, "rp-tree_amd", "host", "example_knn_allow.cpp"))
    assert "example_knn_allow" in open(os.path.join(ROOT, "rp-tree_amd", "host", "Makefile")).read()
    hs = open(os.path.join(ROOT, "haskell", "Data", "RPTree", "HIP.hs")).read()
    for word in ("knnAllowHIP", "bruteKnnAllowHIP", "recallWithAllowHIP", "rpt_knn_allow_host"):
        assert word in hs, word
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md", os.path.join("tools", "README.md"),
                os.path.join("profiles", "README.md")):
        assert "knn_allow" in open(os.path.join(ROOT, doc)).read(), doc
