"""NN-descent rounds under the cosine and inner-product distances on the device
(rpt_knn_graph_refine_metric_host / _dev, csrc/graph_refine.hip): ids, counts and distance BITS, and
the statistics of the call, against the numpy restatement in tests/knn_graph_metric_ref.py (a round
is knn_graph_refine_ref.refine_round with the metric's distance matrix)."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_graph_ref as ref  # noqa: E402
import knn_graph_metric_ref as mref  # noqa: E402

RPT_E_ARG, RPT_E_UNSUPPORTED = -1, -4


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


def distf(rp, metric):
    return {"cosine": rp.metricCosine, "inner": rp.metricInner, "l2": rp.metricL2}[metric]


def make_rows(seed, n, d):
    """the recipe of test_gpu_knn_graph.py: finite rows with exact duplicates under other ids, a
    zero row (NaN against everything under the cosine distance) and rows scaled x10"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    if n > 40:
        X[5] = X[17]
        X[n - 3] = X[17]
        X[31] = X[30]
        X[9] = 0.0
        X[20:28] *= 10.0
    return X


def as_dtype(rp, ctx, X, dtype):
    """-> (Dataset, the rows as the exactly widened doubles)"""
    if dtype == "f64":
        return rp.Dataset.dense(ctx, X), X
    if dtype == "f32":
        X32 = X.astype(np.float32)
        return rp.Dataset.dense(ctx, X32), X32.astype(np.float64)
    u = rp.to_bf16(X)
    return rp.Dataset.dense(ctx, u, dtype=rp.RPT_BF16), rp.from_bf16(u).astype(np.float64)


def leaves_of(f):
    return ref.leaf_slices(f.topology())


def check_against_ref(rp, ctx, metric, ds, X64, D, g0, k, reverse, iters, tag, want=None):
    """the call under both kernel shapes against the restatement -> the device's graph"""
    if want is None:
        want = mref.refine_ref(X64, g0, k, reverse, iters, D)
    df = distf(rp, metric)
    before = tuple(np.array(a) for a in g0)
    got = rp.knnGraphRefineMetric(df, g0, ds, iters=iters, reverse=reverse)
    stats = rp.knnGraphRefineLast(ctx)
    for a, b in zip(before, g0):                           # the input tuple is not modified
        assert np.array_equal(a, b, equal_nan=True)
    ref.assert_same_graph(got, want[0], tag)
    print("%s: (rounds, updates, candidates) device %s restatement %s" % (tag, stats, want[1:]))
    assert stats == tuple(want[1:]), tag
    with option(ctx, "graph_refine_general", 1):
        gen = rp.knnGraphRefineMetric(df, g0, ds, iters=iters, reverse=reverse)
        assert rp.knnGraphRefineLast(ctx) == stats
    ref.assert_same_graph(gen, got, tag + ", graph_refine_general")
    pad = np.arange(k)[None, :] >= got[2][:, None]
    assert np.all(got[0][pad] == -1) and np.all(np.isposinf(got[1][pad]))
    return got


# ---------------------------------------------------------------- the grid
_grid = {}


def grid_case(rp, ctx, metric, dtype, d, k, reverse):
    """data set, forest graph and the restatement's first three rounds, built once per case"""
    key = (metric, dtype, d, k, reverse)
    if key not in _grid:
        n, T, minl = 800, 3, 40
        dkey = (dtype, d)
        if dkey not in _grid:
            ds, X64 = as_dtype(rp, ctx, make_rows(d, n, d), dtype)
            cfg = rp.rpTreeCfg(minl, n, d)
            f = rp.forestBatch(1234 + d, cfg.fpMaxTreeDepth, minl, T, cfg.fpProjNzDensity, d, ds, ctx=ctx)
            _grid[dkey] = (ds, X64, f, {m: mref.metric_matrix(X64, m) for m in mref.METRICS})
        ds, X64, f, Ds = _grid[dkey]
        D = Ds[metric]
        g0 = rp.knnGraphMetric(distf(rp, metric), k, f)
        ref.assert_same_graph(g0, mref.knn_graph_metric_ref(X64, f.perm, leaves_of(f), k, D), "the forest's graph")
        rounds, g, tot, u = [], g0, [0, 0, 0], 1
        for _ in range(3):
            if u > 0:                                      # behind a round without updates nothing is applied
                g, r1, u, c = mref.refine_ref(X64, g, k, reverse, 1, D)
                tot = [tot[0] + r1, tot[1] + u, tot[2] + c]
            rounds.append((g,) + tuple(tot))
        _grid[key] = (ds, X64, D, g0, rounds)
    return _grid[key]


@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("d", [3, 16, 33, 128, 200])
@pytest.mark.parametrize("dtype", ["f64", "f32", "bf16"])
@pytest.mark.parametrize("metric", mref.METRICS)
def test_refine_matches_the_definition(rp, ctx, metric, dtype, d, k):
    """two rounds with reverse = k, with graph_refine_general off and on"""
    ds, X64, D, g0, rounds = grid_case(rp, ctx, metric, dtype, d, k, k)
    got = check_against_ref(rp, ctx, metric, ds, X64, D, g0, k, k, 2,
                            "%s %s d %d k %d" % (metric, dtype, d, k), want=rounds[1])
    for i in range(X64.shape[0]):                          # never its own neighbour
        assert i not in got[0][i]


@pytest.mark.parametrize("iters", [1, 2, 3])
@pytest.mark.parametrize("reverse", [0, 3, 10])
@pytest.mark.parametrize("dtype", ["f64", "f32", "bf16"])
@pytest.mark.parametrize("metric", mref.METRICS)
def test_one_to_three_rounds_with_reverse_0_3_k(rp, ctx, metric, dtype, reverse, iters):
    k, d = 10, 33
    ds, X64, D, g0, rounds = grid_case(rp, ctx, metric, dtype, d, k, reverse)
    check_against_ref(rp, ctx, metric, ds, X64, D, g0, k, reverse, iters,
                      "%s %s r %d iters %d" % (metric, dtype, reverse, iters), want=rounds[iters - 1])


@pytest.mark.parametrize("metric", mref.METRICS)
def test_two_calls_give_the_same_bits(rp, ctx, metric):
    """the reverse lists are filled through an atomic cursor: their selection must not show it"""
    n, d, k = 3000, 32, 10
    ds, X64 = as_dtype(rp, ctx, make_rows(77, n, d), "f64")
    f = rp.forestBatch(5, 6, 60, 3, 0.5, d, ds, ctx=ctx)
    df = distf(rp, metric)
    g0 = rp.knnGraphMetric(df, k, f)
    a = rp.knnGraphRefineMetric(df, g0, ds, iters=2, reverse=4)      # reverse < in-degree of many points
    sa = rp.knnGraphRefineLast(ctx)
    b = rp.knnGraphRefineMetric(df, g0, f, iters=2, reverse=4)       # a forest stands for its data set
    assert rp.knnGraphRefineLast(ctx) == sa
    ref.assert_same_graph(a, b, "second call")
    want = mref.refine_ref(X64, g0, k, 4, 2, mref.metric_matrix(X64, metric))
    ref.assert_same_graph(a, want[0], "reverse 4")
    assert sa == tuple(want[1:])


# ---------------------------------------------------------------- short rows, tiny inputs
@pytest.mark.parametrize("metric", mref.METRICS)
def test_short_and_empty_rows(rp, ctx, metric):
    n, d, k = 700, 24, 5
    X = make_rows(n, n, d)
    ds = rp.Dataset.dense(ctx, X)
    D = mref.metric_matrix(X, metric)
    f = rp.forestBatch(77, 12, 2, 1, 0.5, d, ds, ctx=ctx)  # leaves of one and two points
    g0 = rp.knnGraphMetric(distf(rp, metric), k, f)
    assert (g0[2] == 0).any() and (g0[2] == 1).any() and g0[2].max() < k
    for reverse, iters in ((0, 1), (5, 2), (2, 3)):
        check_against_ref(rp, ctx, metric, ds, X, D, g0, k, reverse, iters, "tiny leaves r %d" % reverse)
    empty = (np.full((n, k), -1, dtype=np.int32), np.full((n, k), np.inf), np.zeros(n, dtype=np.int32))
    got = check_against_ref(rp, ctx, metric, ds, X, D, empty, k, 5, 3, "empty graph")
    assert rp.knnGraphRefineLast(ctx) == (1, 0, 0) and np.all(got[2] == 0)


@pytest.mark.parametrize("metric", mref.METRICS)
@pytest.mark.parametrize("n", [0, 1, 2, 3])
def test_tiny_data_sets(rp, ctx, metric, n):
    d, k = 8, 3
    X = np.random.default_rng(n).standard_normal((n, d))
    ds = rp.Dataset.dense(ctx, X)
    D = mref.metric_matrix(X, metric)
    g0 = mref.hand_graph(D, k, {0: [1]} if n >= 2 else {})
    got = rp.knnGraphRefineMetric(distf(rp, metric), g0, ds, iters=4)
    want = mref.refine_ref(X, g0, k, k, 4, D)
    ref.assert_same_graph(got, want[0], "n %d" % n)
    assert got[0].shape == (n, k) and rp.knnGraphRefineLast(ctx) == tuple(want[1:])
    if n == 2:                                             # the reverse neighbour completes row 1
        assert got[0][1, 0] == 0 and got[2].tolist() == [1, 1] and want[1] == 2


def test_zero_row_ranks_last_by_id_under_cosine(rp, ctx):
    """the zero row is NaN against everything: its own list fills up by id, everybody else keeps it last"""
    n, d, k = 300, 24, 10
    X = make_rows(3, n, d)
    ds = rp.Dataset.dense(ctx, X)
    D = mref.metric_matrix(X, "cosine")
    assert np.all(np.isnan(D[9])) and np.all(np.isnan(D[:, 9]))
    full = mref.exact_graph(D, k)
    assert full[0][9].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 10]
    check_against_ref(rp, ctx, "cosine", ds, X, D, full, k, k, 2, "the exact graph is a fixed point")
    rows = {i: [(i + 1) % n, (i + 7) % n] for i in range(n)}
    rows[9] = [250, 260]
    g0 = mref.hand_graph(D, k, rows)
    got = check_against_ref(rp, ctx, "cosine", ds, X, D, g0, k, k, 3, "ring with the zero row")
    c = got[2][9]
    assert np.all(np.isnan(got[1][9, :c])) and got[0][9, :c].tolist() == sorted(got[0][9, :c].tolist())
    for i in [j for j in range(n) if 9 in got[0][j]]:      # NaN behind every number
        row = got[1][i, :got[2][i]]
        assert np.isnan(row[-1]) and not np.isnan(row[:-1]).any()


# ---------------------------------------------------------------- wide ties
def _tie_case(metric):
    """y, 45 rows at exactly the same distance from y, 30 far rows, shuffled (the rows of
    test_gpu_knn_graph_metric.py::test_scaled_copies_tie_exactly)"""
    d, m = 12, 45
    rng = np.random.default_rng(4)
    if metric == "cosine":
        base = rng.standard_normal(d)
        y = base + 0.3 * rng.standard_normal(d)
        copies = np.array([base * 2.0 ** (a - 20) for a in range(m)])
        far = -y[None, :] + 0.1 * rng.standard_normal((30, d))
    else:
        base = np.zeros(d)
        base[:2] = [1.0, 2.0]
        y = np.zeros(d)
        y[:3] = [2.0, -1.0, 5.0]
        copies = np.array([base * (a + 1) for a in range(m)])
        a = np.abs(rng.standard_normal((30, 2)))
        far = np.concatenate([-(a[:, :1] + 1.0), a[:, 1:], np.zeros((30, 1)), rng.standard_normal((30, d - 3))], axis=1)
    X = np.concatenate([y[None, :], far[:10], copies, far[10:]])
    order = rng.permutation(len(X))
    X = X[order]
    origin = int(np.nonzero(order == 0)[0][0])
    tied_ids = np.sort(np.nonzero((order >= 11) & (order < 11 + m))[0])
    far_ids = np.nonzero((order >= 1) & (order < 11))[0][:5]
    return X, origin, tied_ids, far_ids


@pytest.mark.parametrize("metric", mref.METRICS)
def test_wide_ties_enter_by_id(rp, ctx, metric):
    """45 ids at exactly the same distance from the origin reach it through five far neighbours in
    one round; the first k by id stay.  Inner product: the tied distance is -0.0."""
    k = 10
    X, origin, tied_ids, far_ids = _tie_case(metric)
    D = mref.metric_matrix(X, metric)
    assert len(np.unique(ref.bits(D[origin, tied_ids]))) == 1 and len(tied_ids) > 3 * k
    graph = {origin: far_ids.tolist()}
    for a, fid in enumerate(far_ids):
        graph[int(fid)] = tied_ids[9 * a:9 * a + 9].tolist()
    ds = rp.Dataset.dense(ctx, X)
    g0 = mref.hand_graph(D, k, graph)
    got = check_against_ref(rp, ctx, metric, ds, X, D, g0, k, 0, 1, "ties")
    assert got[0][origin].tolist() == tied_ids[:k].tolist()
    if metric == "inner":
        assert np.all(got[1][origin] == 0.0) and np.all(np.signbit(got[1][origin]))
    got = check_against_ref(rp, ctx, metric, ds, X, D, g0, k, k, 2, "ties, reverse")
    assert got[0][origin].tolist() == tied_ids[:k].tolist()


def test_both_zeros_in_one_row(rp, ctx):
    """inner product: a row that stores +0.0 (the caller's) for some ids receives -0.0 (computed) for
    others: they tie, the id decides, the bits stay"""
    k = 12
    X, origin, tied_ids, far_ids = _tie_case("inner")
    D = mref.metric_matrix(X, "inner")
    stored = tied_ids[1:12:2].tolist()                     # six tied ids, kept at +0.0 in row `origin`
    reach = tied_ids[0:12:2].tolist()                      # six more, reached through a far neighbour
    graph = {origin: stored + [int(far_ids[0])], int(far_ids[0]): reach}
    g0 = mref.hand_graph(D, k, graph)
    c = g0[2][origin]
    z = g0[1][origin, :c] == 0.0
    assert z.sum() == 6
    g0[1][origin, :c][z] = 0.0                             # +0.0: same order, other bits
    ds = rp.Dataset.dense(ctx, X)
    got = check_against_ref(rp, ctx, "inner", ds, X, D, g0, k, 0, 1, "both zeros")
    z = got[1][origin] == 0.0
    zi, signs = got[0][origin][z].tolist(), np.signbit(got[1][origin][z])
    assert zi == sorted(stored + reach) and zi == tied_ids[:12].tolist()
    assert all(bool(s) == (j in reach) for s, j in zip(signs, zi))


# ---------------------------------------------------------------- fixed point
@pytest.mark.parametrize("metric", mref.METRICS)
def test_iterating_reaches_a_fixed_point(rp, ctx, metric):
    n, d, k = 120, 6, 4
    X = np.random.default_rng(1).standard_normal((n, d))
    ds = rp.Dataset.dense(ctx, X)
    D = mref.metric_matrix(X, metric)
    g0 = mref.hand_graph(D, k, {i: [(i + 1) % n, (i + 2) % n] for i in range(n)})
    for reverse in (4, 0):
        want = mref.refine_ref(X, g0, k, reverse, 50, D)
        assert 1 < want[1] < 50
        got = check_against_ref(rp, ctx, metric, ds, X, D, g0, k, reverse, 50, "fixed point r %d" % reverse, want=want)
        again = rp.knnGraphRefineMetric(distf(rp, metric), got, ds, iters=1, reverse=reverse)
        assert rp.knnGraphRefineLast(ctx)[:2] == (1, 0)
        ref.assert_same_graph(again, got, "one more call")
        short = mref.refine_ref(X, g0, k, reverse, want[1] - 1, D)
        assert short[1] == want[1] - 1
        check_against_ref(rp, ctx, metric, ds, X, D, g0, k, reverse, want[1] - 1, "short r %d" % reverse, want=short)


@pytest.mark.parametrize("metric", mref.METRICS)
def test_accumulating_the_forest_into_a_refined_graph_changes_nothing(rp, ctx, metric):
    n, d, k = 2000, 32, 10
    ds, X64 = as_dtype(rp, ctx, make_rows(2, n, d), "f32")
    cfg = rp.rpTreeCfg(50, n, d)
    f = rp.forestBatch(9, cfg.fpMaxTreeDepth, 50, 4, cfg.fpProjNzDensity, d, ds, ctx=ctx)
    df = distf(rp, metric)
    refined = rp.knnGraphRefineMetric(df, rp.knnGraphMetric(df, k, f), f, iters=3)
    ref.assert_same_graph(rp.knnGraphMetric(df, k, f, accumulate=refined), refined, "accumulate")


# ---------------------------------------------------------------- metric 0 = the old entry points
@pytest.mark.parametrize("dtype", ["f64", "f32", "bf16"])
def test_metric_zero_gives_the_bits_of_the_old_entry_points(rp, ctx, dtype):
    n, d, k = 1500, 33, 10
    ds, X64 = as_dtype(rp, ctx, make_rows(8, n, d), dtype)
    f = rp.forestBatch(11, 5, 40, 3, 0.5, d, ds, ctx=ctx)
    g0 = rp.knnGraph(k, f)
    for iters, reverse in ((1, None), (3, 3), (2, 0)):
        old = rp.knnGraphRefine(g0, ds, iters=iters, reverse=reverse)
        stats = rp.knnGraphRefineLast(ctx)
        for df in (None, rp.metricL2):
            ref.assert_same_graph(rp.knnGraphRefineMetric(df, g0, ds, iters=iters, reverse=reverse), old, "metric 0")
            assert rp.knnGraphRefineLast(ctx) == stats
        with option(ctx, "graph_refine_general", 1):
            ref.assert_same_graph(rp.knnGraphRefineMetric(None, g0, ds, iters=iters, reverse=reverse), old,
                                  "metric 0, general")
    with pytest.raises(NotImplementedError):
        rp.knnGraphRefineMetric(lambda u, v: 0.0, g0, ds)


# ---------------------------------------------------------------- errors
def test_errors_leave_the_context_usable(rp, ctx):
    from rptree_amd import _lib
    L = _lib.lib()
    n, d, T, minl, k = 1500, 16, 4, 30, 10
    X = np.random.default_rng(12).standard_normal((n, d))
    ds = rp.Dataset.dense(ctx, X)
    f = rp.forestBatch(7, 6, minl, T, 0.5, d, ds, ctx=ctx)
    g0 = rp.knnGraphMetric(rp.metricCosine, k, f)
    rp.knnGraphRefineMetric(rp.metricCosine, g0, ds)
    stats = rp.knnGraphRefineLast(ctx)
    COS, INN, REF = rp.RPT_KNN_METRIC_COSINE, rp.RPT_KNN_METRIC_INNER, rp.RPT_KNN_METRIC_REFERENCE

    def refused(code, data, kk, reverse, iters, metric, flags, graph=g0):
        ids, dist, cnt = (np.array(a) for a in graph)
        keep = (ids.copy(), dist.copy(), cnt.copy())
        st = L.rpt_knn_graph_refine_metric_host(ctx._h, data._h, kk, reverse, iters, metric, flags,
                                                C.c_void_p(ids.ctypes.data), C.c_void_p(dist.ctypes.data),
                                                C.c_void_p(cnt.ctypes.data))
        assert st == code, (st, code)
        msg = L.rpt_last_error().decode()
        assert len(msg) > 8, msg
        for a, b in zip(keep, (ids, dist, cnt)):           # nothing was written
            assert np.array_equal(a, b)
        assert rp.knnGraphRefineLast(ctx) == stats         # nothing was launched
        return msg

    assert "metric" in refused(RPT_E_ARG, ds, k, k, 1, COS | INN, 0)
    assert "metric" in refused(RPT_E_ARG, ds, k, k, 1, REF, 0)
    assert "metric" in refused(RPT_E_ARG, ds, k, k, 1, INN | 1, 0)
    assert "metric" in refused(RPT_E_ARG, ds, k, k, 1, 2, 0)
    assert "flags" in refused(RPT_E_ARG, ds, k, k, 1, COS, 1)
    assert "flags" in refused(RPT_E_ARG, ds, k, k, 1, COS, COS)
    assert "k" in refused(RPT_E_ARG, ds, 0, 0, 1, COS, 0)
    assert "k" in refused(RPT_E_ARG, ds, 65, 0, 1, INN, 0)
    assert "reverse" in refused(RPT_E_ARG, ds, k, 65, 1, COS, 0)
    assert "iters" in refused(RPT_E_ARG, ds, k, k, 0, COS, 0)
    rowptr = np.arange(n + 1, dtype=np.int64)
    csr = rp.Dataset.csr(ctx, rowptr, np.zeros(n, dtype=np.int32), np.ones(n), d)
    for m in (0, COS, INN):
        assert "CSR" in refused(RPT_E_UNSUPPORTED, csr, k, k, 1, m, 0)
    bad = tuple(np.array(a) for a in g0)
    bad[0][700, 2] = n
    assert "row 700" in refused(RPT_E_ARG, ds, k, k, 1, COS, 0, bad)
    bad = tuple(np.array(a) for a in g0)
    bad[0][701, 0] = 701
    assert "row 701" in refused(RPT_E_ARG, ds, k, k, 1, INN, 0, bad)
    with pytest.raises(rp.RPTError) as e:
        rp.knnGraphRefineMetric(rp.metricCosine, g0, ds, iters=0)
    assert e.value.code == RPT_E_ARG
    # the context answers a good call right after
    D = mref.metric_matrix(X, "cosine")
    want = mref.refine_ref(X, g0, k, k, 1, D)
    ref.assert_same_graph(rp.knnGraphRefineMetric(rp.metricCosine, g0, ds), want[0], "after the refusals")
    assert rp.knnGraphRefineLast(ctx) == tuple(want[1:])


# ---------------------------------------------------------------- device arrays, the profile class
@pytest.mark.parametrize("metric", mref.METRICS)
@pytest.mark.parametrize("dtype", ["f64", "bf16"])
def test_dev_entry_point_with_torch_tensors(rp, ctx, metric, dtype):
    import torch
    n, d, T, minl, k = 2500, 64, 3, 50, 10
    X = make_rows(13, n, d)
    dev = torch.device("cuda", ctx.device)
    t = torch.from_numpy(X).to(dev) if dtype == "f64" else torch.from_numpy(X).to(dev).to(torch.bfloat16)
    ds = rp.Dataset.from_torch(ctx, t)
    cfg = rp.rpTreeCfg(minl, n, d)
    f = rp.forestBatch(8, cfg.fpMaxTreeDepth, minl, T, cfg.fpProjNzDensity, d, ds, ctx=ctx)
    df = distf(rp, metric)
    g0 = rp.knnGraphMetric(df, k, f)
    for iters, reverse in ((1, None), (2, 3), (3, 0)):
        ids = torch.from_numpy(g0[0]).to(dev)
        dist = torch.from_numpy(g0[1]).to(dev)
        cnt = torch.from_numpy(g0[2]).to(dev)
        torch.cuda.synchronize(dev)
        rp.knnGraphRefineMetricDev(df, k, ds, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr(), iters=iters,
                                   reverse=reverse)
        ctx.sync()
        stats = rp.knnGraphRefineLast(ctx)
        got = (ids.cpu().numpy(), dist.cpu().numpy(), cnt.cpu().numpy())
        host = rp.knnGraphRefineMetric(df, g0, ds, iters=iters, reverse=reverse)
        assert rp.knnGraphRefineLast(ctx) == stats and stats[0] == iters
        ref.assert_same_graph(got, host, "dev against host, iters %d" % iters)
    X64 = t.to(torch.float64).cpu().numpy()
    want = mref.refine_ref(X64, g0, k, 0, 3, mref.metric_matrix(X64, metric))
    ref.assert_same_graph(got, want[0], "dev")
    assert stats == tuple(want[1:])


def test_prof_class_3_times_the_call(rp, ctx):
    from rptree_amd import _lib
    L = _lib.lib()
    X = make_rows(14, 1000, 16)
    ds = rp.Dataset.dense(ctx, X)
    f = rp.forestBatch(8, 4, 30, 3, 0.5, 16, ds, ctx=ctx)
    _lib.check(L.rpt_prof_enable(ctx._h, 1))
    try:
        for metric in mref.METRICS:
            g0 = rp.knnGraphMetric(distf(rp, metric), 5, f)
            _lib.check(L.rpt_prof_reset(ctx._h))
            rp.knnGraphRefineMetric(distf(rp, metric), g0, ds, iters=2)
            ms, cnt = C.c_double(), C.c_int64()
            _lib.check(L.rpt_prof_get(ctx._h, 3, C.byref(ms), C.byref(cnt)))
            assert cnt.value == 1 and ms.value > 0.0
    finally:
        _lib.check(L.rpt_prof_enable(ctx._h, 0))
