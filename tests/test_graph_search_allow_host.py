"""The beam search over an allow-list of ids (rpt_graph_search_allow_*) is declared at every layer,
and the numpy restatement that the GPU tests compare with behaves as the header says: its three forms
agree, the all-allowed case is graph_search_ref's, and the frontier is what pays under a narrow
filter (no GPU)."""
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
import graph_search_allow_ref as aref  # noqa: E402

HEADER = open(os.path.join(ROOT, "include", "rptree_hip.h")).read()
NAMES = ("rpt_graph_search_allow_dev", "rpt_graph_search_allow_host")


def _decl(name):
    m = re.search(r"int32_t\s+%s\s*\(([^;]*)\)\s*;" % name, HEADER)
    assert m, name
    return re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)


def _words(decl):
    return [re.sub(r"\s+", " ", a.strip()) for a in decl.split(",")]


# ------------------------------------------------------------------ declarations
def test_header_declares_the_entry_points():
    dev = _words(_decl("rpt_graph_search_allow_dev"))
    plain = _words(_decl("rpt_graph_search_dev"))
    want = list(plain)
    want.insert(want.index("const int32_t* seeds_dev") + 1, "const uint32_t* allow_dev")
    want.insert(want.index("int32_t ef") + 1, "int32_t width")
    assert dev == want and len(dev) == 17
    host = _words(_decl("rpt_graph_search_allow_host"))
    assert host == [w.replace("_dev", "_host") for w in dev]
    assert re.search(r"#define\s+RPT_GRAPH_SEARCH_MAX_WIDTH\s+1024\b", HEADER)
    assert re.search(r"#define\s+RPT_GRAPH_SEARCH_MAX_EF\s+256\b", HEADER)
    assert re.search(r"#define\s+RPT_ABI_VERSION\s+1\b", HEADER)
    # the existing entry points keep their signatures
    assert _decl("rpt_graph_search_dev").count(",") == 14 and _decl("rpt_graph_search_csr_metric_host").count(",") == 14


def test_header_comment_states_the_definition():
    comment = HEADER[HEADER.index("query the kNN graph over an allow-list of ids"):
                     HEADER.index("#define RPT_GRAPH_SEARCH_MAX_WIDTH")]
    flat = re.sub(r"\s*\n \*\s*", " ", comment)
    for phrase in ("bit i & 31 of word i >> 5", "ceil(n / 32)", "Bits at positions >= n are ignored",
                   "A null pointer means every id is allowed", "One bitmap serves the whole batch",
                   "the ef-th allowed entry", "the width-th entry", "not after min(t_a, t_w)", "cut(U) = U",
                   "ENDS at its ef-th allowed entry", "cut(B u {(dist(q, v), v) : v in S})", "every id once",
                   "expanded like any other", "the first k allowed entries", "count = min(k, allowed entries of B)",
                   "id -1", "+inf", "cut(cut(A) u S) = cut(A u S)", "at most n expansions",
                   "an exact visited set, a lossy one, or none", "whatever `width` is", "is post-filtering",
                   "RPT_GRAPH_SEARCH_MAX_WIDTH", "NaN behind every number", "(distance, id)", "4, 2 or 1 waves",
                   "Every valid combination of arguments launches", "rpt_graph_search_last reports these calls too",
                   "RPT_E_ARG", "an all-zero bitmap", "does NOT validate", "longest sorted prefix",
                   "graph_search_nofilter", "graph_search_csr_stream", "Seeds need not be allowed"):
        assert phrase in flat, phrase
    api = open(os.path.join(ROOT, "rp-tree_amd", "csrc", "api.hip")).read()
    assert "width must be in [ef, 1024] (RPT_GRAPH_SEARCH_MAX_WIDTH)" in api


def test_kernel_sources_keep_one_body_of_the_beam():
    csrc = os.path.join(ROOT, "rp-tree_amd", "csrc")
    dev = open(os.path.join(csrc, "graph_dev.h")).read()
    for fn in ("beam_next_offer", "beam_admit", "beam_insert", "beam_answer"):
        assert len(re.findall(r"\b(?:void|bool|int) %s\(" % fn, dev)) == 1, fn
    assert "template <bool F = false, int J = kBeamJ>" in dev and "if constexpr (F)" in dev
    assert "search_waves" in dev
    dense = open(os.path.join(csrc, "graph_search.hip")).read()
    sparse = open(os.path.join(csrc, "graph_search_csr.hip")).read()
    assert len(re.findall(r"__global__[^;{]*\bgraph_search_kernel\(", dense)) == 1
    assert len(re.findall(r"__global__[^;{]*\bgraph_search_allow_kernel\(", dense)) == 1
    assert len(re.findall(r"__global__[^;{]*\bgraph_search_csr_kernel\(", sparse)) == 1
    assert len(re.findall(r"__global__[^;{]*\bgraph_search_csr_allow_kernel\(", sparse)) == 1
    # each file has one body, which both of its kernels call
    assert len(re.findall(r"\bvoid graph_search_body\(", dense)) == 1 and dense.count("graph_search_body<") == 2
    assert len(re.findall(r"\bvoid graph_search_csr_body\(", sparse)) == 1 and sparse.count("graph_search_csr_body<") == 2
    for src in (dense, sparse):
        assert src.count("expanded >= a.n") == 1 and "search_waves(a.wave_bytes, kLdsMax)" in src


def test_ctypes_table_and_python_mirror():
    import rptree_amd as rp
    from rptree_amd import _lib
    for name in NAMES:
        assert len(_lib.SYMBOLS[name][1]) == 17
    declared = set(re.findall(r"^\s*(?:int32_t|const char\*)\s+(rpt_\w+)\s*\(", HEADER, flags=re.M))
    assert declared == set(_lib.SYMBOLS)
    assert _lib.RPT_GRAPH_SEARCH_MAX_WIDTH == 1024
    for name in ("graphSearchAllow", "graphSearchAllowDev", "allowBitmap", "graphSearchLast"):
        assert name in rp.__all__ and callable(getattr(rp, name))
    sig = inspect.signature(rp.graphSearchAllow)
    assert list(sig.parameters) == ["allow", "graph", "data", "qs", "k", "ef", "width", "seeds", "forest", "seed_k",
                                    "metric", "ctx"]
    p = sig.parameters
    assert p["ef"].default is None and p["width"].default is None and p["seeds"].default is None
    assert p["forest"].default is None and p["seed_k"].default == 8 and p["metric"].default is None
    assert list(inspect.signature(rp.graphSearchAllowDev).parameters) == [
        "data", "queries", "kg", "gids_ptr", "gcount_ptr", "s", "seeds_ptr", "allow_ptr", "k", "ef", "width",
        "ids_ptr", "dist_ptr", "count_ptr", "metric"]
    assert list(inspect.signature(rp.allowBitmap).parameters) == ["mask_or_ids", "n"]
    src = inspect.getsource(rp.graphSearchAllow)
    assert set(re.findall(r"\brpt_\w+_host\b", src)) == {"rpt_graph_search_allow_host"}
    assert len(re.findall(r"\b_graph_search\(", src)) == 1 and "check(" not in src and "np.empty(" not in src
    assert "min(RPT_GRAPH_SEARCH_MAX_WIDTH, 8 * int(ef))" in inspect.getsource(rp._graph_search)
    with pytest.raises(NotImplementedError):               # an unknown metric is refused before any handle is touched
        rp.graphSearchAllow(None, None, None, None, 3, metric=max)


def test_allow_bitmap_packs_masks_ids_and_words():
    import rptree_amd as rp
    rng = np.random.default_rng(3)
    for n in (0, 1, 31, 32, 33, 64, 500):
        mask = rng.random(n) < 0.4
        w = rp.allowBitmap(mask, n)
        assert w.dtype == np.uint32 and w.shape == ((n + 31) // 32,)
        assert np.array_equal(w, aref.words_of(mask))
        assert np.array_equal(aref.mask_of(w, n), mask)
        assert np.array_equal(rp.allowBitmap(np.flatnonzero(mask), n), w)
        assert rp.allowBitmap(w, n) is w or np.array_equal(rp.allowBitmap(w, n), w)
    with pytest.raises(ValueError):
        rp.allowBitmap(np.ones(5, dtype=bool), 6)
    with pytest.raises(ValueError):
        rp.allowBitmap(np.array([6]), 6)
    with pytest.raises(ValueError):
        rp.allowBitmap(np.zeros(2, dtype=np.uint32), 100)


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
    assert len(re.findall(r"\brpt_graph_search_allow_host\b", code)) == 1
    assert len(re.findall(r"^inline KnnResult graphSearchAllow\(", hpp, flags=re.M)) == 2 and "allowBitmap(" in hpp
    assert len(re.findall(r"^inline \S+ graphSearchVia\(", hpp, flags=re.M)) == 1
    host = os.path.join(ROOT, "rp-tree_amd", "host")
    example = open(os.path.join(host, "example_graph_search_allow.cpp")).read()
    assert "graphSearchAllow(" in example and "allowBitmap(" in example
    make = open(os.path.join(host, "Makefile")).read()
    assert re.search(r"^all:.*\bexample_graph_search_allow\b", make, flags=re.M)
    assert re.search(r"^example_graph_search_allow: example_graph_search_allow.cpp rptree.hpp", make, flags=re.M)
    assert re.search(r"^\trm -f .*\bexample_graph_search_allow\b", make, flags=re.M)
    hs = open(os.path.join(ROOT, "haskell", "Data", "RPTree", "HIP.hs")).read()
    assert hs.count("graphSearchAllowHIP") >= 3 and "rpt_graph_search_allow_host" in hs
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "rpt_graph_search_allow_host" in integ and "rpt_graph_search_allow_dev" in integ
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "graphSearchAllow" in readme and "graph_search_allow_times" in readme and "allowBitmap" in readme
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for word in ("graph_search_allow_kernel", "graph_search_csr_allow_kernel", "cut(cut(A)", "search_waves"):
        assert word in design, word
    assert "graph_search_allow_times.py" in open(os.path.join(ROOT, "tools", "README.md")).read()
    assert os.path.exists(os.path.join(ROOT, "tools", "graph_search_allow_times.py"))


# ------------------------------------------------------------------ the three forms agree
def _fuzz_case(rng):
    n = int(rng.integers(1, 61))
    kg = int(rng.integers(1, 7))
    drow = rng.integers(0, 6, size=n).astype(np.float64)
    drow[rng.random(n) < 0.1] = np.nan
    gids = rng.integers(-3, n + 3, size=(n, kg)).astype(np.int32)        # junk ids on both sides of [0, n)
    gcount = rng.integers(-1, kg + 2, size=n).astype(np.int32)          # junk counts
    seeds = rng.integers(-1, n + 1, size=int(rng.integers(1, 6))).tolist()
    frac = (0.0, 0.1, 0.5, 1.0)[int(rng.integers(0, 4))]
    allowed = (rng.random(n) < frac).tolist() if frac < 1.0 else [True] * n
    ef = int(rng.integers(1, 12))
    width = ef + int(rng.integers(0, 20))
    return drow.tolist(), gids, gcount, seeds, ef, width, allowed, frac


def test_fuzz_the_three_forms_agree():
    rng = np.random.default_rng(20260)
    cut_several = 0
    for case in range(300):
        drow, gids, gcount, seeds, ef, width, allowed, frac = _fuzz_case(rng)
        b1, e1, o1, u1 = aref.search_one(drow, gids, gcount, seeds, ef, width, allowed, visited=True)
        b0, e0, o0, u0 = aref.search_one(drow, gids, gcount, seeds, ef, width, allowed, visited=False)
        bl, el = aref.search_literal(drow, gids, gcount, seeds, ef, width, allowed)
        s1, s0, sl = ([(sref.key(*b), b[1]) for b in x] for x in (b1, b0, bl))      # NaN != NaN: compare keys
        assert s1 == s0 == sl and e1 == e0 == el and (o1, u1) == (o0, u0), case
        assert len(b1) <= width and sum(allowed[b[1]] for b in b1) <= ef, case
        assert e1 <= len(drow) and o1 <= u1, case
        if frac == 1.0:
            bs, es, os_, us = sref.search_one(drow, gids, gcount, seeds, ef)
            assert [(sref.key(*b), b[1]) for b in bs] == s1 and (es, os_, us) == (e1, o1, u1), case
            assert len(b1) <= ef
        else:
            cut_several += len(b1) < width and sum(allowed[b[1]] for b in b1) == ef
    assert cut_several > 10          # beams that ended at their ef-th allowed entry, short of width


def test_the_prefix_rule_depends_on_the_visited_set_and_the_definition_does_not():
    """ef = 1; ids 0 .. 3 at distances 1 (allowed), 2 (disallowed), 3 (allowed), 4 (disallowed).  The
    seeds offer 0, 1, 2; row 0 offers 3 and row 1 offers 2 again.  Under the prefix rule the beam is
    {0, 1} after the seeds and has forgotten that 2 was rejected, so 3 enters although it lies behind
    2.  With a visited set 2 is never looked at again and 3 stays; without one 2 comes back, is cut
    again and takes 3 with it.  Under the definition the beam ends at its first allowed entry: it is
    {0} either way, and 1, 2 and 3 never enter."""
    drow = [1.0, 2.0, 3.0, 4.0]
    allowed = [True, False, True, False]
    gids = np.array([[3], [2], [-1], [-1]], dtype=np.int32)
    gcount = np.array([1, 1, 0, 0], dtype=np.int32)
    seeds, ef, width = [0, 1, 2], 1, 8
    # the rule itself, on the trap's three entries and then the offer of the fourth
    k = [sref.key(drow[v], v) for v in range(4)]
    assert aref.prefix_rule(sorted(k[:3]), allowed, ef, width) == [k[0], k[1]]
    assert aref.prefix_rule(sorted([k[0], k[1], k[3]]), allowed, ef, width) == [k[0], k[1], k[3]]  # behind the rejected 2
    assert aref.cut(sorted(k[:3]), allowed, ef, width) == [k[0]]
    assert aref.cut(sorted([k[0], k[3]]), allowed, ef, width) == [k[0]]
    # the search under the rule: what the beam holds depends on the visited set
    pv, _ = aref.search_prefix(drow, gids, gcount, seeds, ef, width, allowed, visited=True)
    pn, _ = aref.search_prefix(drow, gids, gcount, seeds, ef, width, allowed, visited=False)
    assert [b[1] for b in pv] == [0, 1, 3] and [b[1] for b in pn] == [0, 1]
    # the definition does not
    got = [aref.search_one(drow, gids, gcount, seeds, ef, width, allowed, visited=v) for v in (True, False)]
    lit = aref.search_literal(drow, gids, gcount, seeds, ef, width, allowed)
    assert got[0] == got[1] and got[0][0] == lit[0] == [(1.0, 0)] and got[0][1] == lit[1] == 1


# ------------------------------------------------------------------ the restatement on the golden data
K = 10


@pytest.fixture(scope="module")
def golden():
    """the setup of test_graph_search_host.py: the 1000 x 16 golden rows, their exact 10-NN graph, 200
    perturbed stored rows as queries with 16 seeds each"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "forest_dense_1000x16.npz"))
    X = z["X"]
    n = X.shape[0]
    exact_graph = mref.exact_graph(mref.metric_matrix(X, "l2"), K)
    rng = np.random.default_rng(2024)
    rows = rng.choice(n, 200, replace=False)
    Q = X[rows] + 0.1 * rng.standard_normal((200, X.shape[1]))
    seeds = np.stack([np.random.default_rng(qi).choice(n, 16, replace=False) for qi in range(200)]).astype(np.int32)
    D = sref.query_matrix(X, Q, "l2")
    return X, Q, seeds, D, exact_graph


def _recall(ids, D, allow):
    """recall@10 against the first 10 ALLOWED rows by (distance, id)"""
    n = D.shape[1]
    hits = want = 0
    idx = np.flatnonzero(allow)
    for i in range(D.shape[0]):
        truth = idx[np.lexsort((idx, D[i, idx]))[:K]]
        want += len(truth)
        hits += len(set(ids[i].tolist()) & set(truth.tolist()))
    assert n == len(allow)
    return hits / want


@pytest.mark.parametrize("ef", [10, 32])
def test_all_allowed_is_the_unfiltered_search_whatever_the_width(golden, ef):
    X, Q, seeds, D, (gids, _, gcnt) = golden
    want, exp, off, up = sref.graph_search_ref(X, Q, gids, gcnt, seeds, K, ef, "l2", D=D)
    for width in sorted({ef, 64, 256}):
        for allow in (None, np.ones(X.shape[0], dtype=bool)):
            got, g_exp, g_off, g_up = aref.graph_search_allow_ref(X, Q, gids, gcnt, seeds, K, ef, width, allow, D=D)
            sref.assert_same_answer(got, want, "ef %d width %d" % (ef, width))
            assert (g_exp, g_off, g_up) == (exp, off, up)


@pytest.mark.parametrize("ef", [10, 32])
def test_width_equal_to_ef_is_post_filtering(golden, ef):
    X, Q, seeds, D, (gids, _, gcnt) = golden
    allow = np.random.default_rng(7).random(X.shape[0]) < 0.5
    got, g_exp, _, _ = aref.graph_search_allow_ref(X, Q, gids, gcnt, seeds, K, ef, ef, allow, D=D)
    exp = 0
    for i in range(Q.shape[0]):
        beam, e, _, _ = sref.search_one(D[i].tolist(), gids, gcnt, seeds[i].tolist(), ef)
        exp += e
        keep = [b for b in beam if allow[b[1]]][:K]
        assert got[2][i] == len(keep) and got[0][i, :len(keep)].tolist() == [b[1] for b in keep], i
        assert np.array_equal(sref.bits(got[1][i, :len(keep)]), sref.bits(np.array([b[0] for b in keep]))), i
        assert np.all(got[0][i, len(keep):] == -1) and np.all(np.isposinf(got[1][i, len(keep):]))
    assert g_exp == exp


def test_the_frontier_is_what_pays_under_a_narrow_filter(golden):
    """10 % allowed (generator seed 7): recall@10 at (ef 32, width 256) is at least 0.95 (the
    restatement gives 0.9855), at (32, 32), which is post-filtering, at most 0.40 (0.3135)"""
    X, Q, seeds, D, (gids, _, gcnt) = golden
    n, nq = X.shape[0], Q.shape[0]
    table = {}
    for frac, cells in ((0.5, ((10, 10), (32, 32), (10, 64), (32, 128))),
                        (0.1, ((10, 10), (32, 32), (32, 128), (32, 256))), (0.02, ((32, 32), (32, 256)))):
        allow = np.random.default_rng(7).random(n) < frac
        for ef, width in cells:
            got, exp, off, up = aref.graph_search_allow_ref(X, Q, gids, gcnt, seeds, K, ef, width, allow, D=D)
            table[frac, ef, width] = (_recall(got[0], D, allow), off / nq)
            print("allowed %4.0f %%  ef %3d  width %4d  recall@10 %.4f  %.0f distances per query" % (
                100 * frac, ef, width, table[frac, ef, width][0], off / nq))
            for i in range(nq):                               # only allowed rows, sorted, their own distances
                c = got[2][i]
                assert allow[got[0][i, :c]].all() and np.array_equal(np.lexsort((got[0][i, :c], got[1][i, :c])), np.arange(c))
                assert np.array_equal(sref.bits(got[1][i, :c]), sref.bits(D[i, got[0][i, :c]]))
    assert table[0.1, 32, 256][0] >= 0.95
    assert table[0.1, 32, 32][0] <= 0.40
    assert table[0.5, 32, 128][0] > table[0.5, 32, 32][0] and table[0.1, 32, 128][0] > table[0.1, 32, 32][0]


# ------------------------------------------------------------------ edge cases
def test_an_all_zero_bitmap_gives_count_zero_everywhere(golden):
    X, Q, seeds, D, (gids, _, gcnt) = golden
    for allow in (np.zeros(X.shape[0], dtype=bool), aref.words_of(np.zeros(X.shape[0], dtype=bool))):
        got, exp, off, up = aref.graph_search_allow_ref(X, Q[:20], gids, gcnt, seeds[:20], K, 10, 40, allow, D=D[:20])
        assert np.all(got[2] == 0) and np.all(got[0] == -1) and np.all(np.isposinf(got[1]))
        assert exp >= 20 * 40                                 # the frontier is still walked: 40 entries, all expanded


def test_one_allowed_row_behind_disallowed_ones_is_found():
    """a chain 0 -> 1 -> ... -> 9 where only row 9 is allowed and lies FARTHEST from the query"""
    n = 10
    drow = [float(i) for i in range(n)]
    gids = np.array([[i + 1] for i in range(n)], dtype=np.int32)
    gcount = np.array([1] * (n - 1) + [0], dtype=np.int32)
    allowed = [False] * 9 + [True]
    beam, exp, _, _ = aref.search_one(drow, gids, gcount, [0], 1, 16, allowed)
    assert aref.answer_of(beam, allowed, 3) == ([9], [9.0]) and exp == 10 and len(beam) == 10
    assert aref.search_literal(drow, gids, gcount, [0], 1, 16, allowed)[0] == beam
    # a frontier of 5 still gets there: the chain is walked with the nearest entries falling out behind
    beam, exp, _, _ = aref.search_one(drow, gids, gcount, [0], 1, 5, allowed)
    assert aref.answer_of(beam, allowed, 3)[0] == [] and exp == 5      # 0 .. 4 fill the beam, 5 is rejected
    # ... unless the walk approaches the query: the same chain entered from its far end
    drow = [float(n - i) for i in range(n)]
    beam, exp, _, _ = aref.search_one(drow, gids, gcount, [0], 1, 5, allowed)
    assert aref.answer_of(beam, allowed, 3) == ([9], [1.0]) and exp == 10 and [b[1] for b in beam] == [9]


@pytest.mark.parametrize("n", [33, 64])
def test_bits_beyond_n_are_ignored(n):
    rng = np.random.default_rng(n)
    X = rng.standard_normal((n, 5))
    Q = rng.standard_normal((6, 5))
    gids = np.array([[(i + 1) % n, (i + 7) % n] for i in range(n)], dtype=np.int32)
    gcnt = np.full(n, 2, dtype=np.int32)
    seeds = rng.integers(0, n, size=(6, 2)).astype(np.int32)
    mask = rng.random(n) < 0.5
    words = aref.words_of(mask)
    assert words.shape == ((n + 31) // 32,)
    dirty = words.copy()
    if n % 32:
        dirty[-1] |= np.uint32((0xffffffff << (n % 32)) & 0xffffffff)       # every bit at a position >= n
        assert not np.array_equal(dirty, words)
    assert np.array_equal(aref.mask_of(dirty, n), mask)
    a = aref.graph_search_allow_ref(X, Q, gids, gcnt, seeds, 4, 5, 12, mask)
    b = aref.graph_search_allow_ref(X, Q, gids, gcnt, seeds, 4, 5, 12, dirty)
    sref.assert_same_answer(a[0], b[0], "dirty tail")
    assert a[1:] == b[1:] and mask[a[0][0][a[0][0] >= 0]].all()
