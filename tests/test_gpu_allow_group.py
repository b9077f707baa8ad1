"""Allow-lists per query group on the device (rpt_graph_search_allow_group_*, rpt_knn_allow_group_*,
rpt_allow_group_candidates_host, rpt_brute_knn_allow_group_*, rpt_recall_hits_allow_group_host).

The definition is a composition: the answer of query q is the single-bitmap entry point's for that
query under bitmap allow[group[q]] (no bitmap for -1), bit for bit.  Every case is therefore held to
two things: the numpy restatement tests/allow_group_ref.py, which composes the single-bitmap
restatements per query, and one single-bitmap call per group over that group's queries (the only route
before), ids, counts, padding and distance BITS.  No tolerance anywhere.  tests/test_allow_group_host.py
shows, without a GPU, that the standing case tells the bitmaps apart."""
import contextlib
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import allow_group_ref as gref  # noqa: E402
import graph_search_ref as sref  # noqa: E402
import graph_metric_csr_ref as gm  # noqa: E402
import knn_allow_ref as kref  # noqa: E402
import test_gpu_graph_search_allow as gsa  # noqa: E402  (helpers: the lattice, the graph, the seeds, csr_case)
import test_gpu_knn_allow as gka  # noqa: E402  (helpers: the masks, the rows, the forests' shapes)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RPT_E_ARG = -1
N, NQ = gsa.N, gsa.NQ
EF_WIDTH = [(32, 32), (32, 128), (16, 1024)]          # both J shapes of the beam: up to 256 entries, beyond
T = gka.T


@pytest.fixture(scope="module")
def rp():
    import rptree_amd
    return rptree_amd


@pytest.fixture(scope="module")
def ctx(rp):
    return rp.default_context()


@contextlib.contextmanager
def option(ctx, name, value):
    old = ctx.set_option(name, value)
    try:
        yield
    finally:
        ctx.set_option(name, old)


def same(a, b, tag):
    """tuples of arrays: equal shapes and values, float arrays by their bits"""
    assert len(a) == len(b), tag
    for i, (x, y) in enumerate(zip(a, b)):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape, (tag, i)
        if x.dtype.kind == "f":
            bad = x.view(np.int64) != y.view(np.int64)
        else:
            bad = x != y
        assert not bad.any(), (tag, i, np.argwhere(bad)[:4].tolist())


def take_queries(qs, rows):
    """rows of a dense query array or of a CSR tuple (rowptr, col, val, d)"""
    if not isinstance(qs, tuple):
        return qs[rows]
    rowptr, col, val, d = qs
    lens = (rowptr[1:] - rowptr[:-1])[rows]
    idx = np.concatenate([np.arange(rowptr[r], rowptr[r + 1]) for r in rows] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), col[idx], val[idx], d


# ------------------------------------------------------------------ J. poisoned scratch (first: the
# child starts before this module's own GPU calls)
POISON_NODES = ["tests/test_gpu_allow_group.py::test_graph_search_dense[24-10-l2]",
                "tests/test_gpu_allow_group.py::test_forest_query[dense_f64_l2-slice7]",
                "tests/test_gpu_allow_group.py::test_exhaustive[dense_f64_l2]"]


def test_no_scratch_word_is_read_unwritten():
    """one case each of A (width 1024 among its beams), C (slice 7) and D (three passes and more) in a
    fresh child whose allocator fills every block with 0xff: an unwritten group entry, list offset, range
    or id read anywhere would change an answer"""
    env = dict(os.environ)
    env["RPT_POOL_POISON"] = "255"
    cmd = ["timeout", "-k", "10", "240", sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider"]
    pr = subprocess.run(cmd + POISON_NODES, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                        timeout=280)
    tail = pr.stdout.decode("utf-8", "replace")[-4000:]
    assert pr.returncode == 0, "exit status %d\n%s" % (pr.returncode, tail)
    summary = tail.strip().splitlines()[-1]
    assert "3 passed" in summary and "skipped" not in summary, summary


# ------------------------------------------------------------------ A. graph search, dense rows
def per_group_search(rp, ctx, masks, group, graph, ds, qs, k, ef, width, seeds, metric):
    """one graphSearchAllow call per group over that group's queries -> (answer, summed statistics)"""
    nq = len(group)
    ids = np.zeros((nq, k), dtype=np.int32)
    dist = np.zeros((nq, k))
    cnt = np.zeros(nq, dtype=np.int32)
    stats = [0, 0]
    for g, rows in gref.queries_of(group).items():
        got = rp.graphSearchAllow(None if g == -1 else masks[g], graph, ds, take_queries(qs, rows), k, ef=ef, width=width,
                                  seeds=seeds[rows], metric=gsa.distf(rp, metric))
        ids[rows], dist[rows], cnt[rows] = got
        e, v = rp.graphSearchLast(ctx)
        stats = [stats[0] + e, stats[1] + v]
    return (ids, dist, cnt), tuple(stats)


_want = {}


@pytest.mark.parametrize("metric", gsa.METRICS)
@pytest.mark.parametrize("d,kg", [(24, 10), (200, 64)])
def test_graph_search_dense(rp, ctx, d, kg, metric):
    X, Q, per, Ds = gsa.dense_case(rp, ctx, d)
    if metric not in Ds:
        Ds[metric] = sref.query_matrix(X, Q, metric)
    gids, gcnt = gsa.make_graph(np.random.default_rng(10), N, kg)
    seeds = gsa.make_seeds(np.random.default_rng(66), NQ, N, 8)
    masks, group = gref.standing_masks(N), gref.standing_group(NQ)
    words = rp.allowBitmaps(masks, N)
    k = 10
    for ef, width in EF_WIDTH:
        key = (metric, d, kg, ef, width)
        if key not in _want:
            _want[key] = gref.group_answers(X, Q, gids, gcnt, seeds, k, ef, width, masks, group, metric, D=Ds[metric])
        want, exp, offered, upper = _want[key]
        for dtype in ("f64", "f32", "bf16"):
            tag = "%s %s d %d kg %d ef %d width %d" % (metric, dtype, d, kg, ef, width)
            ds, qarr = per[dtype]
            got = rp.graphSearchAllowGroup(masks if dtype == "f64" else words, group, (gids, gcnt), ds, qarr, k, ef=ef,
                                           width=width, seeds=seeds, metric=gsa.distf(rp, metric))
            g_exp, g_eval = rp.graphSearchLast(ctx)
            sref.assert_same_answer(got, want, tag)
            gsa.check_padding(got, k)
            assert g_exp == exp and offered <= g_eval <= upper, tag
            assert np.all(got[2][group == 4] == 0) and got[2][7] == 0, tag          # the empty bitmap; no seeds
            calls, _ = per_group_search(rp, ctx, masks, group, (gids, gcnt), ds, qarr, k, ef, width, seeds, metric)
            same(got, calls, tag + ", per-group calls")
            with option(ctx, "graph_search_nofilter", 1):
                bare = rp.graphSearchAllowGroup(words, group, (gids, gcnt), ds, qarr, k, ef=ef, width=width,
                                                seeds=seeds, metric=gsa.distf(rp, metric))
                bare_stats = rp.graphSearchLast(ctx)
                _, call_stats = per_group_search(rp, ctx, masks, group, (gids, gcnt), ds, qarr, k, ef, width, seeds,
                                                 metric)
            same(bare, got, tag + ", graph_search_nofilter")
            assert bare_stats == call_stats and bare_stats[0] == exp, tag            # `evaluated` too, without the hash


# ------------------------------------------------------------------ B. graph search, CSR rows
@pytest.mark.parametrize("metric", gsa.METRICS)
def test_graph_search_csr(rp, ctx, metric):
    csrX, csrQ, Ds = gsa.csr_case()
    if metric not in Ds:
        Ds[metric] = gsa.csr_distances(csrX, csrQ, metric)
    kg, k = 10, 10
    gids, gcnt = gsa.make_graph(np.random.default_rng(10), N, kg)
    seeds = gsa.make_seeds(np.random.default_rng(66), NQ, N, 8)
    masks, group = gref.standing_masks(N), gref.standing_group(NQ)
    X0, Q0 = np.zeros((N, 1)), np.zeros((NQ, 1))           # the restatement takes its distances from D
    for ef, width in EF_WIDTH:
        want, exp, offered, upper = gref.group_answers(X0, Q0, gids, gcnt, seeds, k, ef, width, masks, group, metric,
                                                       D=Ds[metric])
        for dtype in ("f64", "f32"):
            tag = "csr %s %s ef %d width %d" % (metric, dtype, ef, width)
            ds, qs = rp.Dataset.csr(ctx, *gsa.csr_as(csrX, dtype)), gsa.csr_as(csrQ, dtype)
            got = rp.graphSearchAllowGroup(masks, group, (gids, gcnt), ds, qs, k, ef=ef, width=width, seeds=seeds,
                                           metric=gsa.distf(rp, metric))
            g_exp, g_eval = rp.graphSearchLast(ctx)
            sref.assert_same_answer(got, want, tag)
            gsa.check_padding(got, k)
            assert g_exp == exp and offered <= g_eval <= upper, tag
            calls, _ = per_group_search(rp, ctx, masks, group, (gids, gcnt), ds, qs, k, ef, width, seeds, metric)
            same(got, calls, tag + ", per-group calls")
            with option(ctx, "graph_search_csr_stream", 1):
                again = rp.graphSearchAllowGroup(masks, group, (gids, gcnt), ds, qs, k, ef=ef, width=width, seeds=seeds,
                                                 metric=gsa.distf(rp, metric))
                assert rp.graphSearchLast(ctx) == (g_exp, g_eval), tag
            same(again, got, tag + ", graph_search_csr_stream")
            with option(ctx, "graph_search_nofilter", 1):
                bare = rp.graphSearchAllowGroup(masks, group, (gids, gcnt), ds, qs, k, ef=ef, width=width, seeds=seeds,
                                                metric=gsa.distf(rp, metric))
                bare_stats = rp.graphSearchLast(ctx)
                _, call_stats = per_group_search(rp, ctx, masks, group, (gids, gcnt), ds, qs, k, ef, width, seeds, metric)
            same(bare, got, tag + ", graph_search_nofilter")
            assert bare_stats == call_stats, tag
            ds.close()


@pytest.mark.parametrize("metric", gsa.METRICS)
def test_graph_search_csr_stored_inf_and_nan(rp, ctx, metric):
    """the rows of test_stored_inf_and_nan_follow_dots under three bitmaps and no bitmap"""
    n, nq, d, kg = 300, 24, 40, 8
    rowptr, col, val, _ = gm.make_csr(9, n, d, 0.3)
    val = val.copy()
    val[rowptr[30]] = np.inf
    val[rowptr[31]] = -np.inf
    val[rowptr[32]] = np.nan
    csrX = (rowptr, col, val, d)
    qrows = [(c.copy(), v.copy()) for c, v in gm.rows_of(gm.make_csr(10, nq, d, 0.3))]
    qrows[0] = gm.rows_of(csrX)[30]
    qrows[1] = gm.rows_of(csrX)[32]
    qrows[2] = (qrows[2][0], np.concatenate([[np.inf], qrows[2][1][1:]]))
    csrQ = gm.from_rows(qrows, d)
    rng = np.random.default_rng(2)
    gids, gcnt = gsa.make_graph(rng, n, kg)
    gids[:, 0] = rng.choice([30, 31, 32], size=n)          # every row leads to the awkward ones
    seeds = rng.integers(0, n, size=(nq, 4)).astype(np.int32)
    with_them = rng.random(n) < 0.4
    with_them[[30, 31, 32]] = True
    without = rng.random(n) < 0.4
    without[[30, 31, 32]] = False
    masks = [with_them, without, np.zeros(n, dtype=bool)]
    group = gref.interleaved_group(nq, 3)
    assert set(group[:3].tolist()) == {2, -1, 0}
    ds = rp.Dataset.csr(ctx, *csrX)
    D = gsa.csr_distances(csrX, csrQ, metric)
    got = rp.graphSearchAllowGroup(masks, group, (gids, gcnt), ds, csrQ, 10, ef=24, width=90, seeds=seeds,
                                   metric=gsa.distf(rp, metric))
    stats = rp.graphSearchLast(ctx)
    want, exp, offered, upper = gref.group_answers(np.zeros((n, 1)), np.zeros((nq, 1)), gids, gcnt, seeds, 10, 24, 90,
                                                   masks, group, metric, D=D)
    sref.assert_same_answer(got, want, "stored inf / NaN, " + metric)
    assert stats[0] == exp and offered <= stats[1] <= upper
    calls, _ = per_group_search(rp, ctx, masks, group, (gids, gcnt), ds, csrQ, 10, 24, 90, seeds, metric)
    same(got, calls, "stored inf / NaN, per-group calls, " + metric)


# ------------------------------------------------------------------ C. the forest query
def cell_forest(rp, ctx, oracle, cell):
    """-> (forest, queries, knnAllow's keywords) of a (layout, dtype, distance) cell"""
    kind, dtype, metric = cell.split("_")
    kw = gka.metric_kw(rp, metric)
    if kind in ("dense", "streamed"):
        ds, _, qs = gka.dense_cell(rp, ctx, oracle, dtype)
        L, pnz, R = gka.hyperplanes(oracle, gka.N, gka.D, gka.ML)
        if kind == "streamed":
            X, _ = gka.dense_rows(oracle)
            return rp.forest(0, L, gka.ML, T, 700, pnz, gka.D, X, ctx=ctx, hyperplanes=R), qs, kw
        return rp._build(ctx, ds, R.reshape(T, L, gka.D), L, gka.ML, rp.RPT_PROJ_AUTO), qs, kw
    data, queries, d = gka.sparse_rows()                    # the sparse 600 x 12 golden forest's rows
    npd = np.float64 if dtype == "f64" else np.float32
    data = (data[0], data[1], data[2].astype(npd))
    queries = (queries[0], queries[1], queries[2].astype(npd))
    cfg = rp.rpTreeCfg(gka.ML, len(data[0]) - 1, d)
    f = rp.forestBatch(9, cfg.fpMaxTreeDepth, gka.ML, T, cfg.fpProjNzDensity, d, data + (d,), ctx=ctx)
    return f, queries + (d,), kw


def group_case(n, nq):
    """test_gpu_knn_allow's eight masks (the last as words with every bit behind n set) plus -1, interleaved"""
    ms = gka.masks(n)
    names = ("half", "tenth", "hundredth", "all", "none", "one", "last_word", "tail_bits")
    given = [ms[name][0] for name in names]
    masks = [np.asarray(ms[name][1], dtype=bool) for name in names]
    return given, masks, gref.interleaved_group(nq, 8)


FOREST_CELLS = ["dense_f64_l2", "dense_f32_cosine", "dense_bf16_inner", "csr_f64_l2", "csr_f64_reference",
                "csr_f64_cosine", "csr_f32_inner", "streamed_f64_l2"]


@pytest.mark.parametrize("mode", ["default", "slice7"])
@pytest.mark.parametrize("cell", FOREST_CELLS)
def test_forest_query(rp, ctx, oracle, cell, mode):
    f, qs, kw = cell_forest(rp, ctx, oracle, cell)
    n = f.data.n
    assert n % 32 != 0
    off, cids = rp.candidatesBatch(f, qs)
    nq = (len(off) - 1) // T
    given, masks, group = group_case(n, nq)
    assert nq > 8 and set(group.tolist()) == set(range(-1, 8))
    k = 10
    per_query = off[T::T] - off[:-1:T]
    exact = per_query.max() <= 1024
    if exact:       # every candidate entry, ranked, with the cell's own distance bits
        ai, ad, ac = rp.knnBatch(1024, f, qs, dedup=False, **kw)
        assert np.array_equal(ac, per_query)
    else:           # (the streamed forest's Tips are large) the same listing on metricDDL2's fold in numpy
        assert cell == "streamed_f64_l2"
        X, _ = gka.dense_rows(oracle)
        ac = per_query.astype(np.int32)
        ai = np.full((nq, int(ac.max())), -1, dtype=np.int32)
        ad = np.full((nq, int(ac.max())), np.inf)
        for i in range(nq):
            c = cids[off[i * T]:off[(i + 1) * T]]
            dv = kref.l2_f64(X[c], qs[i])
            o = kref.rank(dv)
            ai[i, :ac[i]], ad[i, :ac[i]] = c[o], dv[o]
    rules = gka.RULE_ARG.items() if cell == "dense_f64_l2" else [(kref.EACH_ID_ONCE, True)]
    with option(ctx, "knn_allow_slice", 7 if mode == "slice7" else 0):     # slices mix groups; seams inside a group
        for rule, dedup in rules:
            tag = "%s %s rule %d" % (cell, mode, rule)
            got = rp.knnAllowGroup(given, group, k, f, qs, dedup=dedup, **kw)
            stats = rp.knnAllowLast(ctx)
            want = gref.knn_group_answers(ai, ad, ac, masks, group, k, rule)
            assert np.array_equal(got[2], want[2]), (tag, np.flatnonzero(got[2] != want[2])[:4])
            assert np.array_equal(got[0], want[0]), tag
            assert kref.same_bits(got[1], want[1]) if exact else np.allclose(got[1], want[1], rtol=1e-12), tag
            sums = [0, 0, 0]

            def call(mask, rows):
                r = rp.knnAllow(mask, k, f, take_queries(qs, rows), dedup=dedup, **kw)
                for i, v in enumerate(rp.knnAllowLast(ctx)):
                    sums[i] += v
                return r
            calls = gref.per_group_calls(call, given, group, nq, [((k,), np.int32), ((k,), np.float64), ((), np.int32)])
            same(got, calls, tag + ", per-group calls")
            assert stats == tuple(sums), (tag, stats, sums)
            assert stats[0] == len(cids) and stats[1] == sum(int(masks[g][cids[off[i * T]:off[(i + 1) * T]]].sum())
                                                            if g >= 0 else int(off[(i + 1) * T] - off[i * T])
                                                            for i, g in enumerate(group.tolist())), tag
        # the allowed lists themselves
        goff, gids = rp.allowGroupCandidates(given, group, f, qs)
        lens = np.zeros(nq, dtype=np.int64)
        parts = [None] * nq
        for g, rows in gref.queries_of(group).items():
            o, ids = rp.allowCandidates(None if g == -1 else given[g], f, take_queries(qs, rows))
            for j, q in enumerate(rows.tolist()):
                parts[q] = ids[o[j]:o[j + 1]]
                lens[q] = o[j + 1] - o[j]
        assert np.array_equal(goff, np.concatenate([[0], np.cumsum(lens)])), cell
        assert np.array_equal(gids, np.concatenate(parts)), cell
        for q in (0, 1, 2, nq - 1):
            assert np.array_equal(parts[q], kref.allowed_list(cids[off[q * T]:off[(q + 1) * T]],
                                                              gref.mask_of_group(masks, int(group[q]), n))), (cell, q)
    f.close()


# ------------------------------------------------------------------ D. the exhaustive kNN
def cell_rows(rp, ctx, oracle, cell):
    """-> (device data set, queries, bruteKnnAllow's keywords)"""
    kind, dtype, metric = cell.split("_")
    kw = gka.metric_kw(rp, metric)
    if kind == "dense":
        ds, _, qs = gka.dense_cell(rp, ctx, oracle, dtype)
        return ds, qs, kw
    data, queries, d = gka.sparse_rows()
    npd = np.float64 if dtype == "f64" else np.float32
    ds = rp.Dataset.csr(ctx, data[0], data[1], data[2].astype(npd), d)
    return ds, (queries[0], queries[1], queries[2].astype(npd), d), kw


def per_group_brute(rp, given, group, ds, qs, k, kw):
    nq = len(group)
    return gref.per_group_calls(lambda mask, rows: rp.bruteKnnAllow(mask, ds, take_queries(qs, rows), k, **kw), given,
                                group, nq, [((k,), np.int32), ((k,), np.float64)])


BRUTE_CELLS = ["dense_%s_%s" % (t, m) for t in ("f64", "f32", "bf16") for m in ("l2", "cosine", "inner")] + \
              ["csr_%s_%s" % (t, m) for t in ("f64", "f32") for m in ("l2", "reference", "cosine", "inner")]


@pytest.mark.parametrize("cell", BRUTE_CELLS)
def test_exhaustive(rp, ctx, oracle, cell):
    """against per-group bruteKnnAllow bit for bit, the true L2 on CSR rows (the tiled kernel, every tile
    size: tiles mix groups) included; knn_allow_group_budget changes no bit.  The lists hold about n / 2,
    n / 10, n / 100, n, 0, 1, a word's worth and n / 2 ids plus the n of the unfiltered queries, 3.1 n in all:
    a budget of n + n / 30 ids (asserted below) takes at least three passes, a budget of 1 one pass per list."""
    ds, qs, kw = cell_rows(rp, ctx, oracle, cell)
    n = ds.n
    nq = len(qs) if not isinstance(qs, tuple) else len(qs[0]) - 1
    given, masks, group = group_case(n, nq)
    given = given + [np.ones(n, dtype=bool)]               # a ninth bitmap that no query names
    k = 10
    want = per_group_brute(rp, given, group, ds, qs, k, kw)
    assert (want[0][group == 4] == -1).all() and np.isposinf(want[1][group == 4]).all()      # an empty group
    assert ((want[0][group == 5] >= 0).sum(axis=1) == 1).all()                               # one id, k = 10
    true_l2 = cell.startswith("csr") and cell.endswith("_l2")
    lens = [int(m.sum()) for m in masks] + [n]                 # the eight lists that are named and the one of all ids
    tight = n + n // 30                                         # 3100 ids at n = 3000: room for any one list
    assert sum(lens) > 2 * tight and max(lens) <= tight         # ... and at least three passes for the nine
    for budget in (0, tight, 1):
        with option(ctx, "knn_allow_group_budget", budget):
            got = rp.bruteKnnAllowGroup(given, group, ds, qs, k, **kw)
        same(got, want, "%s budget %d" % (cell, budget))
    # rpt_knn_last_uncertified is a sum over the queries, whatever the passes: equal to the per-group calls' sum,
    # also where a launch reports every query (the *_exact options)
    if not true_l2:
        def uncertified_sums(budget):
            with option(ctx, "knn_allow_group_budget", budget):
                rp.bruteKnnAllowGroup(given, group, ds, qs, k, **kw)
                mine = rp.knn_last_uncertified(ctx)
            calls = 0
            for g, rows in gref.queries_of(group).items():
                rp.bruteKnnAllow(None if g == -1 else given[g], ds, take_queries(qs, rows), k, **kw)
                calls += rp.knn_last_uncertified(ctx)
            return mine, calls
        for budget in (0, tight, 1):
            mine, calls = uncertified_sums(budget)
            assert mine == calls, (cell, budget, mine, calls)
        exact_opt = "knn_l2_exact" if cell.endswith("_l2") else "knn_metric_exact"
        if cell.startswith("dense") and (not cell.endswith("_l2") or "f64" in cell):
            with option(ctx, exact_opt, 1):
                for budget in (0, 1):
                    mine, calls = uncertified_sums(budget)
                    assert mine == calls, (cell, exact_opt, budget, mine, calls)
    if true_l2:
        for tile in (1, 2, 4, 8):
            with option(ctx, "brute_csr_tile", tile):
                got = rp.bruteKnnAllowGroup(given, group, ds, qs, k, **kw)
            same(got, want, "%s tile %d" % (cell, tile))
    # the restatement: the k best allowed rows by (distance, id), ids (the cell's own distance bits are
    # pinned by the per-group calls above, which tests/test_gpu_knn_allow.py pins in turn)
    for q in range(nq):
        m = gref.mask_of_group(masks, int(group[q]), n)
        ids = got[0][q][got[0][q] >= 0]
        assert len(ids) == min(k, int(m.sum())) and m[ids].all() and len(set(ids.tolist())) == len(ids), (cell, q)
    ds.close()


# ------------------------------------------------------------------ E. recall
@pytest.mark.parametrize("cell", ["dense_f64_l2", "csr_f64_inner"])
def test_recall(rp, ctx, oracle, cell):
    f, qs, kw = cell_forest(rp, ctx, oracle, cell)
    nq = len(qs) if not isinstance(qs, tuple) else len(qs[0]) - 1
    given, masks, group = group_case(f.data.n, nq)
    distf = kw.get("metric", rp.metricL2)
    k = 10
    hits, truth = rp.recallHitsAllowGroup(given, group, distf, f, k, qs)
    want = gref.per_group_calls(lambda mask, rows: rp.recallHitsAllow(mask, distf, f, k, take_queries(qs, rows)), given,
                                group, nq, [((T,), np.int32), ((k,), np.int32)])
    same((hits, truth), want, cell)
    same((truth,), (rp.bruteKnnAllowGroup(given, group, f, qs, k, metric=distf)[0],), cell + ", truth")
    rec = rp.recallWithAllowGroupBatch(given, group, distf, f, k, qs)
    assert np.array_equal(rec, np.array([sum(h / k for h in row) / T for row in hits.tolist()]))
    assert hits.sum() > 0 and (hits[group == 4] == 0).all()
    f.close()


# ------------------------------------------------------------------ F. two calls, device arrays
def test_two_calls_and_the_dev_entry_points_give_the_same_bits(rp, ctx, oracle):
    import torch
    dev = torch.device("cuda", ctx.device)
    f, qs, kw = cell_forest(rp, ctx, oracle, "dense_f64_l2")
    n, nq, k = f.data.n, len(qs), 10
    given, masks, group = group_case(n, nq)
    words = rp.allowBitmaps(given, n)
    G = len(given)
    rng = np.random.default_rng(3)
    kg, s, ef, width = 10, 6, 32, 200
    gids, gcnt = gsa.make_graph(rng, n, kg)
    seeds = rng.integers(0, n, size=(nq, s)).astype(np.int32)
    host = {"graph": rp.graphSearchAllowGroup(words, group, (gids, gcnt), f, qs, k, ef=ef, width=width, seeds=seeds)}
    gstats = rp.graphSearchLast(ctx)
    host["forest"] = rp.knnAllowGroup(words, group, k, f, qs, dedup=True)
    host["brute"] = rp.bruteKnnAllowGroup(words, group, f, qs, k)
    same(rp.graphSearchAllowGroup(given, group, (gids, gcnt), f, qs, k, ef=ef, width=width, seeds=seeds), host["graph"],
         "second call")
    assert rp.graphSearchLast(ctx) == gstats
    same(rp.knnAllowGroup(given, group, k, f, qs, dedup=True), host["forest"], "second call")
    same(rp.bruteKnnAllowGroup(given, group, f, qs, k), host["brute"], "second call")

    tq = torch.from_numpy(np.ascontiguousarray(qs)).to(dev)
    qd = rp.Dataset.from_torch(ctx, tq)
    tw = torch.from_numpy(words.view(np.int32).copy()).to(dev)
    tg, tc, ts = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (gids, gcnt, seeds))
    # the only out-of-range values used: G and -2, which mean "no id allowed" on the _dev entry points
    wild = group.copy()
    wild[3], wild[11] = G, -2
    assert group[3] != 4 and group[11] != 4
    for name, grp in (("valid", group), ("out of range", wild)):
        tgr = torch.from_numpy(grp).to(dev)
        ids = torch.full((nq, k), -7, dtype=torch.int32, device=dev)
        dist = torch.zeros((nq, k), dtype=torch.float64, device=dev)
        cnt = torch.full((nq,), -7, dtype=torch.int32, device=dev)
        out = lambda: (ids.cpu().numpy(), dist.cpu().numpy(), cnt.cpu().numpy())  # noqa: E731

        def check(got, want, what):
            ok = np.ones(nq, dtype=bool)
            if name != "valid":
                ok[[3, 11]] = False
                assert (got[0][~ok] == -1).all() and np.isposinf(got[1][~ok]).all(), what
                if len(got) == 3:
                    assert (got[2][~ok] == 0).all(), what
            same(tuple(a[ok] for a in got), tuple(a[ok] for a in want), "%s, %s group" % (what, name))
        torch.cuda.synchronize(dev)
        rp.graphSearchAllowGroupDev(f.data, qd, kg, tg.data_ptr(), tc.data_ptr(), s, ts.data_ptr(), tw.data_ptr(), G,
                                    tgr.data_ptr(), k, ef, width, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr())
        ctx.sync()
        check(out(), host["graph"], "graphSearchAllowGroupDev")
        if name == "valid":
            assert rp.graphSearchLast(ctx) == gstats
        ids.fill_(-7), dist.zero_(), cnt.fill_(-7)
        torch.cuda.synchronize(dev)
        rp.knnAllowGroupDev(tw.data_ptr(), G, tgr.data_ptr(), k, f, qd, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr(),
                            dedup=True)
        ctx.sync()
        check(out(), host["forest"], "knnAllowGroupDev")
        ids.fill_(-7), dist.zero_()
        torch.cuda.synchronize(dev)
        rp.bruteKnnAllowGroupDev(tw.data_ptr(), G, tgr.data_ptr(), f.data, qd, k, ids.data_ptr(), dist.data_ptr())
        ctx.sync()
        check(out()[:2], host["brute"], "bruteKnnAllowGroupDev")
    # a null group on the _dev entry points: every query unfiltered, whatever allow holds
    ids = torch.full((nq, k), -7, dtype=torch.int32, device=dev)
    dist = torch.zeros((nq, k), dtype=torch.float64, device=dev)
    cnt = torch.full((nq,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    rp.graphSearchAllowGroupDev(f.data, qd, kg, tg.data_ptr(), tc.data_ptr(), s, ts.data_ptr(), tw.data_ptr(), G, 0, k, ef,
                                width, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr())
    ctx.sync()
    same((ids.cpu().numpy(), dist.cpu().numpy(), cnt.cpu().numpy()),
         rp.graphSearch((gids, gcnt), f, qs, k, ef=ef, seeds=seeds), "dev, null group")
    rp.knnAllowGroupDev(tw.data_ptr(), G, 0, k, f, qd, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr(), dedup=True)
    ctx.sync()
    same((ids.cpu().numpy(), dist.cpu().numpy(), cnt.cpu().numpy()), rp.knnBatch(k, f, qs, dedup=True), "dev, null group")
    rp.bruteKnnAllowGroupDev(0, 0, 0, f.data, qd, k, ids.data_ptr(), dist.data_ptr())
    ctx.sync()
    same((ids.cpu().numpy(), dist.cpu().numpy()), rp.bruteKnn(f, qs, k), "dev, G = 0 and a null group")
    f.close()


# ------------------------------------------------------------------ G. identities
def test_identities(rp, ctx, oracle):
    from rptree_amd import _lib
    L = _lib.lib()
    f, qs, kw = cell_forest(rp, ctx, oracle, "dense_f64_l2")
    n, nq, k = f.data.n, len(qs), 10
    half = gka.masks(n)["half"][1]
    rng = np.random.default_rng(4)
    kg, s, ef, width = 10, 6, 32, 128
    gids, gcnt = gsa.make_graph(rng, n, kg)
    seeds = rng.integers(0, n, size=(nq, s)).astype(np.int32)
    zeros, minus = np.zeros(nq, dtype=np.int32), np.full(nq, -1, dtype=np.int32)
    # G = 1 with every query in group 0: the single-bitmap call on the whole batch
    same(rp.graphSearchAllowGroup([half], zeros, (gids, gcnt), f, qs, k, ef=ef, width=width, seeds=seeds),
         rp.graphSearchAllow(half, (gids, gcnt), f, qs, k, ef=ef, width=width, seeds=seeds), "G = 1, graph search")
    same(rp.knnAllowGroup([half], zeros, k, f, qs, dedup=True), rp.knnAllow(half, k, f, qs, dedup=True), "G = 1, forest")
    single_stats = rp.knnAllowLast(ctx)
    rp.knnAllowGroup([half], zeros, k, f, qs, dedup=True)
    assert rp.knnAllowLast(ctx) == single_stats
    same(rp.bruteKnnAllowGroup([half], zeros, f, qs, k), rp.bruteKnnAllow(half, f, qs, k), "G = 1, exhaustive")
    o1, i1 = rp.allowGroupCandidates([half], zeros, f, qs)
    o2, i2 = rp.allowCandidates(half, f, qs)
    assert np.array_equal(o1, o2) and np.array_equal(i1, i2)
    # every query unfiltered: group all -1 (with bitmaps and with G = 0) is the unfiltered entry point
    plain = {"graph": rp.graphSearch((gids, gcnt), f, qs, k, ef=ef, seeds=seeds),
             "forest": rp.knnBatch(k, f, qs, dedup=True), "brute": rp.bruteKnn(f, qs, k)}
    for allow in ([half], None):
        same(rp.graphSearchAllowGroup(allow, minus, (gids, gcnt), f, qs, k, ef=ef, width=width, seeds=seeds),
             plain["graph"], "group -1, graph search")
        same(rp.knnAllowGroup(allow, minus, k, f, qs, dedup=True), plain["forest"], "group -1, forest")
        same(rp.bruteKnnAllowGroup(allow, minus, f, qs, k), plain["brute"], "group -1, exhaustive")
    same(rp.knnAllowGroup([half], None, k, f, qs, dedup=True), plain["forest"], "group None, forest")
    same(rp.bruteKnnAllowGroup([half], None, f, qs, k), plain["brute"], "group None, exhaustive")
    same(rp.graphSearchAllowGroup([half], None, (gids, gcnt), f, qs, k, ef=ef, width=width, seeds=seeds), plain["graph"],
         "group None, graph search")
    # a null group on the _host entry points
    qd, _ = rp._query_dataset(ctx, f.data, qs)
    words = rp.allowBitmaps([half], n)
    ids = np.empty((nq, k), dtype=np.int32)
    dist = np.empty((nq, k))
    cnt = np.empty(nq, dtype=np.int32)
    for wp, G in ((rp._vp(words), 1), (None, 0)):
        assert L.rpt_graph_search_allow_group_host(ctx._h, f.data._h, qd._h, kg, rp._vp(gids), rp._vp(gcnt), s,
                                                   rp._vp(seeds), wp, G, None, k, ef, width, 0, 0, rp._vp(ids),
                                                   rp._vp(dist), rp._vp(cnt)) == 0
        same((ids, dist, cnt), plain["graph"], "null group, graph search")
        assert L.rpt_knn_allow_group_host(ctx._h, f._h, f.data._h, qd._h, wp, G, None, k, rp.RPT_KNN_DEDUP, rp._vp(ids),
                                          rp._vp(dist), rp._vp(cnt)) == 0
        same((ids, dist, cnt), plain["forest"], "null group, forest")
        assert L.rpt_brute_knn_allow_group_host(ctx._h, f.data._h, qd._h, wp, G, None, k, 0, rp._vp(ids),
                                                rp._vp(dist)) == 0
        same((ids, dist), plain["brute"], "null group, exhaustive")
    f.close()


# ------------------------------------------------------------------ H. refusals
def test_refusals_leave_the_context_usable(rp, ctx, oracle):
    from rptree_amd import _lib
    L = _lib.lib()
    f, qs, kw = cell_forest(rp, ctx, oracle, "dense_f64_l2")
    n, nq, k = f.data.n, len(qs), 5
    qd, _ = rp._query_dataset(ctx, f.data, qs)
    q32 = rp.Dataset.dense(ctx, qs.astype(np.float32))
    given, masks, group = group_case(n, nq)
    words = rp.allowBitmaps(given, n)
    G = len(given)
    rng = np.random.default_rng(5)
    kg, s, ef, width = 10, 4, 32, 100
    gids, gcnt = gsa.make_graph(rng, n, kg)
    seeds = rng.integers(0, n, size=(nq, s)).astype(np.int32)
    ids = np.full((nq, 64), 12345, dtype=np.int32)
    dist = np.full((nq, 64), 0.5)
    cnt = np.full(nq, 77, dtype=np.int32)
    hits = np.full((nq, T), 9, dtype=np.int32)
    off = np.zeros(nq + 1, dtype=np.int64)
    total = C.c_int64()

    keep = []                                                   # the group arrays the pointers below point into

    def calls(grp=group, G_=G, wp="words", k_=k, flags=0, width_=width, queries=qd):
        wp = rp._vp(words) if wp == "words" else wp
        keep.append(np.ascontiguousarray(grp, dtype=np.int32))
        gp = rp._vp(keep[-1])
        return {
            "graph": lambda: L.rpt_graph_search_allow_group_host(
                ctx._h, f.data._h, queries._h, kg, rp._vp(gids), rp._vp(gcnt), s, rp._vp(seeds), wp, G_, gp, k_, ef,
                width_, 0, flags, rp._vp(ids), rp._vp(dist), rp._vp(cnt)),
            "forest": lambda: L.rpt_knn_allow_group_host(ctx._h, f._h, f.data._h, queries._h, wp, G_, gp, k_, flags,
                                                         rp._vp(ids), rp._vp(dist), rp._vp(cnt)),
            "lists": lambda: L.rpt_allow_group_candidates_host(ctx._h, f._h, queries._h, wp, G_, gp, rp._vp(off), None, 0,
                                                               C.byref(total)),
            "brute": lambda: L.rpt_brute_knn_allow_group_host(ctx._h, f.data._h, queries._h, wp, G_, gp, k_, flags,
                                                              rp._vp(ids), rp._vp(dist)),
            "recall": lambda: L.rpt_recall_hits_allow_group_host(ctx._h, f._h, f.data._h, queries._h, wp, G_, gp, k_,
                                                                 flags, rp._vp(hits), None)}

    def untouched():
        return np.all(ids == 12345) and np.all(dist == 0.5) and np.all(cnt == 77) and np.all(hits == 9)

    def valid_call_succeeds():
        got = rp.knnAllowGroup(given, group, k, f, qs, dedup=True)
        assert np.array_equal(got[0], good[0]) and kref.same_bits(got[1], good[1])

    good = rp.knnAllowGroup(given, group, k, f, qs, dedup=True)
    bad_G, bad_minus = group.copy(), group.copy()
    bad_G[5], bad_minus[nq - 1] = G, -2
    refusals = [("group value G", dict(grp=bad_G), None), ("group value -2", dict(grp=bad_minus), None),
                ("G < 0", dict(G_=-1), None), ("null allow with G > 0", dict(wp=None), None),
                # what the single-bitmap entry points refuse
                ("k = 0", dict(k_=0), ("graph", "forest", "brute", "recall")),
                ("width below ef", dict(width_=ef - 1), ("graph",)),
                ("unknown flags", dict(flags=1 << 30), ("graph", "forest", "brute", "recall")),
                ("both metric bits", dict(flags=rp.RPT_KNN_METRIC_COSINE | rp.RPT_KNN_METRIC_INNER),
                 ("forest", "brute", "recall")),
                ("the CSR metric on dense rows", dict(flags=rp.RPT_KNN_METRIC_REFERENCE), ("forest", "brute", "recall")),
                ("f32 queries on f64 rows", dict(queries=q32), ("graph", "forest", "brute", "recall"))]
    for what, kwargs, which in refusals:
        for name, call in calls(**kwargs).items():
            if which is not None and name not in which:
                continue
            st = call()
            assert st == RPT_E_ARG, (what, name, st)
            assert len(L.rpt_last_error().decode()) > 8, (what, name)
            assert untouched(), (what, name)                # nothing was written
        valid_call_succeeds()
    assert "group[5]" in (calls(grp=bad_G)["forest"](), L.rpt_last_error().decode())[1]
    st = calls(flags=2 << 8)["forest"]()                       # a RPT_KNN_VOTE field keeps its own code
    assert st == -4, st
    valid_call_succeeds()
    for name, call in calls().items():                         # and the same arguments, valid, succeed
        assert call() == 0, name
    with pytest.raises(ValueError):
        rp.knnAllowGroup(given, group[:-1], k, f, qs)
    with pytest.raises(ValueError):
        rp.knnAllowGroup([masks[0][:-1]], group, k, f, qs)
    f.close()


# ------------------------------------------------------------------ I. degenerate shapes
def test_no_queries_no_points_and_one_point(rp, ctx):
    d = 8
    X = np.random.default_rng(1).standard_normal((50, d))
    ds = rp.Dataset.dense(ctx, X)
    gids = np.array([[(i + 1 + e) % 50 for e in range(3)] for i in range(50)], dtype=np.int32)
    graph = (gids, np.full(50, 3, dtype=np.int32))
    masks = [np.arange(50) % 2 == 0, np.arange(50) % 2 == 1]
    none = np.zeros(0, dtype=np.int32)
    # nq = 0
    ids, dist, cnt = rp.graphSearchAllowGroup(masks, none, graph, ds, np.zeros((0, d)), 5,
                                              seeds=np.zeros((0, 2), dtype=np.int32))
    assert ids.shape == (0, 5) and dist.shape == (0, 5) and cnt.shape == (0,) and rp.graphSearchLast(ctx) == (0, 0)
    ids, dist = rp.bruteKnnAllowGroup(masks, none, ds, np.zeros((0, d)), 5)
    assert ids.shape == (0, 5) and dist.shape == (0, 5)
    # n = 1, allowed, not allowed and unfiltered, in one batch
    Q = X[:4] + 0.01
    one = rp.Dataset.dense(ctx, X[:1])
    g1 = (np.full((1, 2), -1, dtype=np.int32), np.zeros(1, dtype=np.int32))
    seeds = np.array([[0], [-1], [0], [0]], dtype=np.int32)
    m1 = [np.array([True]), np.array([False])]
    group = np.array([0, 0, 1, -1], dtype=np.int32)
    got = rp.graphSearchAllowGroup(m1, group, g1, one, Q, 3, ef=3, width=3, seeds=seeds)
    want = gref.group_answers(X[:1], Q, g1[0], g1[1], seeds, 3, 3, 3, m1, group)
    sref.assert_same_answer(got, want[0], "n = 1")
    assert got[2].tolist() == [1, 0, 0, 1] and rp.graphSearchLast(ctx)[0] == want[1]
    bi, bd = rp.bruteKnnAllowGroup(m1, group, one, Q, 3)
    assert (bi[:, 0] >= 0).tolist() == [True, True, False, True] and (bi[:, 1:] == -1).all()
    # n = 0: every count is 0
    empty = rp.Dataset.dense(ctx, np.zeros((0, d)))
    g0 = (np.zeros((0, 2), dtype=np.int32), np.zeros(0, dtype=np.int32))
    m0 = [np.zeros(0, dtype=bool), np.zeros(0, dtype=bool)]
    got = rp.graphSearchAllowGroup(m0, group % 2, g0, empty, Q, 3, seeds=np.full((4, 2), -1, dtype=np.int32))
    assert np.all(got[2] == 0) and np.all(got[0] == -1)
    bi, bd = rp.bruteKnnAllowGroup(m0, group, empty, Q, 3)
    assert (bi == -1).all() and np.isposinf(bd).all()


@pytest.mark.parametrize("n", [32, 33])
def test_bits_behind_n_are_ignored_in_every_row(rp, ctx, n):
    rng = np.random.default_rng(n)
    X = rng.integers(-2, 3, size=(n, 6)).astype(np.float64)
    Q = X[:9] + 0.5
    ds = rp.Dataset.dense(ctx, X)
    gids, gcnt = gsa.make_graph(rng, n, 4)
    seeds = rng.integers(0, n, size=(9, 2)).astype(np.int32)
    masks = [rng.random(n) < 0.5, rng.random(n) < 0.3, np.zeros(n, dtype=bool)]
    group = gref.interleaved_group(9, 3)
    clean, dirty = gref.words_of_masks(masks, n), gref.words_of_masks(masks, n, tail=True)
    assert clean.shape == (3, (n + 31) // 32) and (n % 32 == 0) == np.array_equal(clean, dirty)
    a = rp.graphSearchAllowGroup(clean, group, (gids, gcnt), ds, Q, 5, ef=6, width=20, seeds=seeds)
    b = rp.graphSearchAllowGroup(dirty, group, (gids, gcnt), ds, Q, 5, ef=6, width=20, seeds=seeds)
    same(a, b, "dirty tail, graph search")
    sref.assert_same_answer(a, gref.group_answers(X, Q, gids, gcnt, seeds, 5, 6, 20, masks, group)[0], "restatement")
    for budget in (0, 1):
        with option(ctx, "knn_allow_group_budget", budget):
            same(rp.bruteKnnAllowGroup(clean, group, ds, Q, 5), rp.bruteKnnAllowGroup(dirty, group, ds, Q, 5),
                 "dirty tail, exhaustive")
    bi, _ = rp.bruteKnnAllowGroup(dirty, group, ds, Q, 5)
    for q in range(9):
        m = gref.mask_of_group(masks, int(group[q]), n)
        assert (bi[q] >= 0).sum() == min(5, int(m.sum())) and m[bi[q][bi[q] >= 0]].all(), q


# ------------------------------------------------------------------ K. the C++ mirror
def test_cpp_example(rp, ctx, tmp_path):
    """host/example_allow_group.cpp serves three tenants from one batch; its own check is the per-tenant
    calls, and the answers it prints are Python's"""
    exe = str(tmp_path / "example_allow_group")
    src = os.path.join(ROOT, "rp-tree_amd", "host", "example_allow_group.cpp")
    lib = os.path.join(ROOT, "rp-tree_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, src, "-L" + lib, "-lrptree_hip",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    rng = np.random.default_rng(12)
    n, nq, d, k = 2000, 40, 16, 5
    X = rng.standard_normal((n, d))
    Q = X[rng.choice(n, nq)] + 0.1 * rng.standard_normal((nq, d))
    for name, a in (("data.bin", X), ("queries.bin", Q)):
        with open(tmp_path / name, "wb") as fh:
            fh.write(np.array(a.shape, dtype=np.int64).tobytes())
            fh.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run(["timeout", "-k", "10", "120", exe, str(tmp_path / "data.bin"), str(tmp_path / "queries.bin"), "4",
                        "40", "10", str(k), "32", "128"], capture_output=True, text=True, timeout=150)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok" and len(lines) == 3 * nq + 1
    masks = [np.arange(n) % 3 == t for t in range(3)]
    group = np.array([-1 if q % 7 == 6 else q % 3 for q in range(nq)], dtype=np.int32)
    ds = rp.Dataset.dense(ctx, X)
    bi, bd = rp.bruteKnnAllowGroup(masks, group, ds, Q, k)
    # the example's forest, graph and seeds, rebuilt here by the same calls: forestBatch(7, ...) draws the
    # same hyperplanes in both mirrors, and the graph steps are functions of (forest, data)
    cfg = rp.rpTreeCfg(40, n, d)
    f = rp.forestBatch(7, cfg.fpMaxTreeDepth, 40, 4, cfg.fpProjNzDensity, d, ds, ctx=ctx)
    graph = rp.graphPrepare(rp.knnGraphRefine(rp.knnGraph(10, f), f, iters=1), f, kout=20)
    fi, fd, _ = rp.knnAllowGroup(masks, group, k, f, Q, dedup=True)
    gi, gd, _ = rp.graphSearchAllowGroup(masks, group, graph, f, Q, k, ef=32, width=128, forest=f)
    python = {"brute": (bi, bd), "forest": (fi, fd), "graph": (gi, gd)}
    seen = 0
    for ln in lines[:-1]:
        head, body = ln.split(":", 1)
        what, q, _, t = head.split()
        q = int(q)
        assert int(t) == group[q]
        pairs = [p.split(":") for p in body.split()]
        ids = np.array([int(p[0]) for p in pairs], dtype=np.int32)
        dist = np.array([float(p[1]) for p in pairs])
        assert len(ids) == k
        if group[q] >= 0:
            assert (ids[ids >= 0] % 3 == group[q]).all(), ln
        pi, pd = python[what]                               # Python's ids and distance bits, all three kinds
        assert np.array_equal(ids, pi[q]) and kref.same_bits(dist, pd[q]), ln
        seen += 1
    assert seen == 3 * nq
    f.close()
