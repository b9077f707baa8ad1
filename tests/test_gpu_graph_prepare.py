"""The search-graph preparation on the device (rpt_graph_prepare_host / _dev, csrc/graph_prepare.hip):
ids, counts and distance BITS, and the three statistics of the call, against the numpy restatement in
tests/graph_prepare_ref.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_graph_metric_ref as mref  # noqa: E402
import graph_search_ref as sref  # noqa: E402
import graph_prepare_ref as pref  # noqa: E402

RPT_E_ARG, RPT_E_UNSUPPORTED = -1, -4
METRICS = ("l2", "cosine", "inner")
FLAGS = (0, 1, 2, 3)


@pytest.fixture(scope="module")
def rp():
    import rptree_amd
    return rptree_amd


@pytest.fixture(scope="module")
def ctx(rp):
    return rp.default_context()


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


def as_dtype(rp, X, dtype):
    """-> (the array to hand to the library, the rows as the exactly widened doubles)"""
    if dtype == "f64":
        return X, X
    if dtype == "f32":
        X32 = X.astype(np.float32)
        return X32, X32.astype(np.float64)
    u = rp.to_bf16(X)
    return u, rp.from_bf16(u).astype(np.float64)


def dataset(rp, ctx, arr, dtype):
    return rp.Dataset.dense(ctx, arr, dtype=rp.RPT_BF16) if dtype == "bf16" else rp.Dataset.dense(ctx, arr)


def prepare(rp, ctx, graph, ds, kout, flags, metric):
    got = rp.graphPrepare(graph, ds, kout=kout, diversify=bool(flags & 1), reverse=bool(flags & 2),
                          metric=distf(rp, metric))
    return got, rp.graphPrepareLast(ctx)


def check_all(rp, ctx, graph, ds, D, metric, kouts, tag, flags=FLAGS):
    """every flag value and every kout against the restatement: the answer's bits and the statistics"""
    for fl in flags:
        unions, (pairs, occluded) = pref.unions_of(graph, D, fl)
        for kout in kouts:
            want, capped = pref.cut_unions(unions, kout)
            got, stats = prepare(rp, ctx, graph, ds, kout, fl, metric)
            t = "%s flags %d kout %d" % (tag, fl, kout)
            print("%s: pairs %d occluded %d capped %d" % (t, stats[0], stats[1], stats[2]))
            pref.assert_same_answer(got, want, t)
            assert stats == (pairs, occluded, capped), t


# ---------------------------------------------------------------- the grid
_data = {}


def grid_data(rp, ctx, dtype, d):
    """data set, forest and per metric the pair distances; only the last (dtype, d) is kept"""
    key = (dtype, d)
    if key not in _data:
        _data.clear()
        n, T, minl = 1500, 3, 40
        arr, X64 = as_dtype(rp, make_rows(d, n, d), dtype)
        ds = dataset(rp, ctx, arr, dtype)
        cfg = rp.rpTreeCfg(minl, n, d)
        f = rp.forestBatch(1234 + d, cfg.fpMaxTreeDepth, minl, T, cfg.fpProjNzDensity, d, ds, ctx=ctx)
        _data[key] = (ds, X64, f, {})
    return _data[key]


@pytest.mark.parametrize("k", [1, 2, 10, 11, 12, 64])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", [24, 200])
@pytest.mark.parametrize("dtype", ["f64", "f32", "bf16"])
def test_prepare_matches_the_definition(rp, ctx, dtype, d, metric, k):
    """k = 11 is the last with one pair per lane, 12 the first with two, 64 has 32"""
    ds, X64, f, Ds = grid_data(rp, ctx, dtype, d)
    if metric not in Ds:
        Ds[metric] = mref.metric_matrix(X64, metric)
    graph = rp.knnGraphMetric(distf(rp, metric), k, f)
    if k == 64:
        assert graph[2].min() < k                          # ragged rows
    kouts = sorted({1, k, min(64, 2 * k), 64})
    check_all(rp, ctx, graph, ds, Ds[metric], metric, kouts, "%s %s d %d k %d" % (metric, dtype, d, k))
    if k == 10:
        # flags 0, kout = k: the input bit for bit; DIVERSIFY's output is a valid input again; with
        # REVERSE and a kout that cuts nothing the graph is symmetric
        same, _ = prepare(rp, ctx, graph, ds, k, 0, metric)
        pref.assert_same_answer(same, graph, "identity")
        once, _ = prepare(rp, ctx, graph, ds, k, 1, metric)
        twice, st = prepare(rp, ctx, once, ds, k, 1, metric)
        want, wst = pref.graph_prepare_ref(once, Ds[metric], k, 1)
        pref.assert_same_answer(twice, want, "second pass")
        assert st == wst
        sym, st = prepare(rp, ctx, graph, ds, 64, 3, metric)
        if st[2] == 0:
            rows = [set(sym[0][i, :sym[2][i]].tolist()) for i in range(len(sym[2]))]
            assert all(i in rows[j] for i in range(len(rows)) for j in rows[i])


# ---------------------------------------------------------------- shapes
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", ["f64", "f32", "bf16"])
@pytest.mark.parametrize("d", [1, 33])
def test_chunk_edges(rp, ctx, d, dtype, metric):
    """d = 1 and d = 33 = one staged chunk plus one column"""
    n, k = 300, 7
    arr, X64 = as_dtype(rp, make_rows(d + 1, n, d), dtype)
    ds = dataset(rp, ctx, arr, dtype)
    D = mref.metric_matrix(X64, metric)
    graph = mref.exact_graph(D, k)
    check_all(rp, ctx, graph, ds, D, metric, [5, 14], "d %d %s %s" % (d, dtype, metric))


def test_wide_rows(rp, ctx):
    """d = 1100: 35 chunks, the accumulators carried through all of them"""
    n, d, k = 200, 1100, 12
    X = np.random.default_rng(11).standard_normal((n, d))
    X[3] = X[77]
    ds = rp.Dataset.dense(ctx, X)
    for metric in METRICS:
        D = mref.metric_matrix(X, metric)
        check_all(rp, ctx, mref.exact_graph(D, k), ds, D, metric, [12, 24], "d 1100 " + metric, flags=(1, 3))


def test_hub_empty_rows_and_tiny_sets(rp, ctx):
    """every row lists point 0: a reverse list of n - 1 against kout = 8; rows of count 0; n = 0, 1"""
    n, d, k = 1500, 16, 4
    X = make_rows(3, n, d)
    ds = rp.Dataset.dense(ctx, X)
    D = mref.metric_matrix(X, "l2")
    rng = np.random.default_rng(4)
    rows = {i: [0] + rng.choice(n, 3, replace=False).tolist() for i in range(1, n)}
    rows[0] = [1, 2, 3]
    graph = mref.hand_graph(D, k, rows)
    for i in (7, 8, 900):                                   # empty rows: only reverse edges reach them
        graph[0][i], graph[1][i], graph[2][i] = -1, np.inf, 0
    check_all(rp, ctx, graph, ds, D, "l2", [8, 64], "hub")
    got, stats = prepare(rp, ctx, graph, ds, 8, 2, "l2")
    assert got[2][0] == 8 and stats[2] >= n - 1 - 3 - 8
    # n = 1 and n = 0
    one = rp.Dataset.dense(ctx, X[:1])
    g1 = (np.full((1, 3), -1, dtype=np.int32), np.full((1, 3), np.inf), np.zeros(1, dtype=np.int32))
    for fl in FLAGS:
        got = rp.graphPrepare(g1, one, kout=2, diversify=bool(fl & 1), reverse=bool(fl & 2))
        assert got[2].tolist() == [0] and np.all(got[0] == -1) and np.all(np.isposinf(got[1]))
        assert rp.graphPrepareLast(ctx) == (0, 0, 0)
    none = rp.Dataset.dense(ctx, np.zeros((0, d)))
    g0 = (np.zeros((0, 3), dtype=np.int32), np.zeros((0, 3)), np.zeros(0, dtype=np.int32))
    for fl in FLAGS:
        got = rp.graphPrepare(g0, none, kout=5, diversify=bool(fl & 1), reverse=bool(fl & 2))
        assert got[0].shape == (0, 5) and got[1].shape == (0, 5) and got[2].shape == (0,)
        assert rp.graphPrepareLast(ctx) == (0, 0, 0)


def test_inconsistent_distances_row_i_wins(rp, ctx):
    """row v lists 0 at another distance than row 0 lists v: each row keeps its own, also where the cap
    cuts the own entry off (the reverse copy must not come back in its place)"""
    n, d, k = 6, 5, 3
    X = np.random.default_rng(6).standard_normal((n, d))
    ds = rp.Dataset.dense(ctx, X)
    D = mref.metric_matrix(X, "l2")
    ids, dist, cnt = mref.hand_graph(D, k, {0: [1, 2, 3], 1: [0, 2], 2: [0, 3], 3: [0, 4], 4: [5], 5: [4]})
    v = int(ids[0, 2])                                      # the farthest of row 0: kout < 3 cuts it off
    c = int(cnt[v])
    s0 = ids[v, :c].tolist().index(0)
    order = [s0] + [x for x in range(c) if x != s0]
    ids[v, :c], dist[v, :c] = ids[v, order], dist[v, order]
    dist[v, 0] = 0.0                                        # row v says 0 is at distance 0, row 0 does not
    graph = (ids, dist, cnt)
    for kout in (1, 2, 8):
        for fl in (2, 3):
            got, stats = prepare(rp, ctx, graph, ds, kout, fl, "l2")
            want, wst = pref.graph_prepare_ref(graph, D, kout, fl)
            pref.assert_same_answer(got, want, "kout %d flags %d" % (kout, fl))
            assert stats == wst


# ---------------------------------------------------------------- determinism, device arrays
@pytest.mark.parametrize("metric", METRICS)
def test_two_calls_and_the_dev_entry_point_give_the_same_bits(rp, ctx, metric):
    import torch
    n, d, k, kout = 2500, 64, 10, 16
    X = make_rows(13, n, d)
    dev = torch.device("cuda", ctx.device)
    t = torch.from_numpy(X).to(dev)
    ds = rp.Dataset.from_torch(ctx, t)
    cfg = rp.rpTreeCfg(50, n, d)
    f = rp.forestBatch(8, cfg.fpMaxTreeDepth, 50, 3, cfg.fpProjNzDensity, d, ds, ctx=ctx)
    df = distf(rp, metric)
    graph = rp.knnGraphMetric(df, k, f)
    a, sa = prepare(rp, ctx, graph, ds, kout, 3, metric)
    b, sb = prepare(rp, ctx, graph, ds, kout, 3, metric)
    pref.assert_same_answer(a, b, "second call")
    assert sa == sb

    def on_device(g, fl):
        ti, td, tc = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in g)
        keep = (ti.clone(), td.clone(), tc.clone())
        oi = torch.empty((n, kout), dtype=torch.int32, device=dev)
        od = torch.empty((n, kout), dtype=torch.float64, device=dev)
        oc = torch.empty(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        rp.graphPrepareDev(k, ds, ti.data_ptr(), td.data_ptr(), tc.data_ptr(), kout, oi.data_ptr(), od.data_ptr(),
                           oc.data_ptr(), diversify=bool(fl & 1), reverse=bool(fl & 2), metric=df)
        ctx.sync()
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip((ti, td, tc), keep))
        return (oi.cpu().numpy(), od.cpu().numpy(), oc.cpu().numpy()), rp.graphPrepareLast(ctx)

    c, sc = on_device(graph, 3)
    pref.assert_same_answer(c, a, "dev against host")
    assert sc == sa
    # _dev does not validate: an id outside [0, n) is skipped, a count is clamped to [0, k]
    ids, dist, cnt = (np.array(x) for x in graph)
    ids[40, 1] = n + 5
    ids[41, 0] = -7
    ids[42, 3] = 2 ** 31 - 1
    full = int(np.argmax(cnt == k))
    cnt[full] = k + 3
    cnt[44] = -2
    X64 = X
    D = mref.metric_matrix(X64, metric)
    clean = pref.clean_graph((ids, dist, cnt), n)
    assert clean[2][40] == graph[2][40] - 1 and clean[2][full] == k and clean[2][44] == 0
    for fl in FLAGS:
        got, sg = on_device((ids, dist, cnt), fl)
        want, wst = pref.graph_prepare_ref(clean, D, kout, fl)
        pref.assert_same_answer(got, want, "planted graph, flags %d" % fl)
        assert sg == wst


# ---------------------------------------------------------------- refusals
def test_refusals_leave_the_context_usable(rp, ctx):
    from rptree_amd import _lib
    L = _lib.lib()
    n, d, T, minl, k, kout = 1500, 16, 4, 30, 10, 12
    X = make_rows(12, n, d)
    ds = rp.Dataset.dense(ctx, X)
    cfg = rp.rpTreeCfg(minl, n, d)
    f = rp.forestBatch(7, cfg.fpMaxTreeDepth, minl, T, cfg.fpProjNzDensity, d, ds, ctx=ctx)
    graph = rp.knnGraph(k, f)
    Q = X[:16] + 0.1
    knn0 = rp.knnBatch(5, f, Q)
    tier = C.c_int32(-1)
    _lib.check(L.rpt_knn_last_tier(ctx._h, C.byref(tier)))
    tier0 = tier.value
    good, stats = prepare(rp, ctx, graph, ds, kout, 3, "l2")
    assert stats[0] > 0
    COS, INN, REF = rp.RPT_KNN_METRIC_COSINE, rp.RPT_KNN_METRIC_INNER, rp.RPT_KNN_METRIC_REFERENCE

    def refused(code, data=ds, k_=k, kout_=kout, metric=0, flags=3, gids=None, gcnt=None):
        gids = np.ascontiguousarray(graph[0] if gids is None else gids, dtype=np.int32)
        gdist = np.ascontiguousarray(graph[1])
        gcnt = np.ascontiguousarray(graph[2] if gcnt is None else gcnt, dtype=np.int32)
        before = (gids.copy(), gdist.copy(), gcnt.copy())
        ids = np.full((n, 64), 12345, dtype=np.int32)
        dist = np.full((n, 64), 0.5)
        cnt = np.full(n, 77, dtype=np.int32)
        st = L.rpt_graph_prepare_host(ctx._h, data._h, k_, C.c_void_p(gids.ctypes.data),
                                      C.c_void_p(gdist.ctypes.data), C.c_void_p(gcnt.ctypes.data), kout_, metric,
                                      flags, C.c_void_p(ids.ctypes.data), C.c_void_p(dist.ctypes.data),
                                      C.c_void_p(cnt.ctypes.data))
        assert st == code, (st, code)
        msg = L.rpt_last_error().decode()
        assert len(msg) > 8, msg
        assert np.all(ids == 12345) and np.all(dist == 0.5) and np.all(cnt == 77)   # nothing was written
        assert all(np.array_equal(x, y) for x, y in zip((gids, gdist, gcnt), before))
        assert rp.graphPrepareLast(ctx) == stats            # nothing was launched
        return msg

    assert "k must" in refused(RPT_E_ARG, k_=0)
    assert "k must" in refused(RPT_E_ARG, k_=65)
    assert "kout" in refused(RPT_E_ARG, kout_=0)
    assert "kout" in refused(RPT_E_ARG, kout_=65)
    assert "flags" in refused(RPT_E_ARG, flags=4)
    assert "flags" in refused(RPT_E_ARG, flags=3 | COS)
    assert "flags" in refused(RPT_E_ARG, flags=-1)
    assert "metric" in refused(RPT_E_ARG, metric=COS | INN)
    assert "metric" in refused(RPT_E_ARG, metric=REF)
    assert "metric" in refused(RPT_E_ARG, metric=2)
    rowptr = np.arange(n + 1, dtype=np.int64)
    csr = rp.Dataset.csr(ctx, rowptr, np.zeros(n, dtype=np.int32), np.ones(n), d)
    for m in (0, COS, INN):
        assert "CSR" in refused(RPT_E_UNSUPPORTED, data=csr, metric=m)
    # _host names the row of the graph that is out of range, as the refinement does
    bad = np.array(graph[2])
    bad[700] = k + 1
    assert "graph row 700: count" in refused(RPT_E_ARG, gcnt=bad)
    bad[700] = -1
    assert "graph row 700: count" in refused(RPT_E_ARG, gcnt=bad)
    bad = np.array(graph[0])
    bad[701, 0] = n
    assert graph[2][701] > 1 and "graph row 701: id" in refused(RPT_E_ARG, gids=bad)
    bad[701, 0] = -1
    assert "graph row 701: id" in refused(RPT_E_ARG, gids=bad)
    bad[701, 0] = 701
    assert "graph row 701 holds its own id" in refused(RPT_E_ARG, gids=bad)
    bad[701, 0] = bad[701, 1]
    assert "graph row 701 holds id" in refused(RPT_E_ARG, gids=bad)
    with pytest.raises(ValueError):
        rp.graphPrepare(graph, ds, kout=65)
    with pytest.raises(ValueError):
        rp.graphPrepare((graph[0][:5], graph[1][:5], graph[2][:5]), ds)
    again, st2 = prepare(rp, ctx, graph, ds, kout, 3, "l2")
    pref.assert_same_answer(again, good, "after the refusals")
    assert st2 == stats
    # kout defaults to min(64, 2 k); the kNN entry points are untouched
    assert rp.graphPrepare(graph, f)[0].shape == (n, 2 * k)
    _lib.check(L.rpt_knn_last_tier(ctx._h, C.byref(tier)))
    assert tier.value == tier0
    knn1 = rp.knnBatch(5, f, Q)
    assert all(np.array_equal(x, y) for x, y in zip(knn0, knn1))


# ---------------------------------------------------------------- end to end, the profile class
@pytest.mark.parametrize("metric", METRICS)
def test_search_on_a_prepared_graph(rp, ctx, metric):
    """graph -> refine -> prepare -> search: graphSearch with kg = kout equals the restatement of the
    search on the prepared graph, which equals the restatement of the preparation"""
    n, d, k, kout, nq = 2000, 32, 10, 16, 50
    arr, X64 = as_dtype(rp, make_rows(21, n, d), "f32")
    ds = rp.Dataset.dense(ctx, arr)
    cfg = rp.rpTreeCfg(60, n, d)
    f = rp.forestBatch(9, cfg.fpMaxTreeDepth, 60, 2, cfg.fpProjNzDensity, d, ds, ctx=ctx)
    df = distf(rp, metric)
    graph = rp.knnGraphRefineMetric(df, rp.knnGraphMetric(df, k, f), f, iters=1)
    flags = 2 if metric == "inner" else 3
    sg, stats = prepare(rp, ctx, graph, ds, kout, flags, metric)
    want, wst = pref.graph_prepare_ref(graph, mref.metric_matrix(X64, metric), kout, flags)
    pref.assert_same_answer(sg, want, "prepared")
    assert stats == wst
    rng = np.random.default_rng(8)
    Q = (X64[rng.choice(n, nq)] + 0.2 * rng.standard_normal((nq, d))).astype(np.float32)
    seeds = rng.integers(0, n, size=(nq, 4)).astype(np.int32)
    got = rp.graphSearch(sg, ds, Q, 10, ef=32, seeds=seeds, metric=df)
    model = sref.graph_search_ref(X64, Q.astype(np.float64), sg[0], sg[2], seeds, 10, 32, metric)
    sref.assert_same_answer(got, model[0], "search on the prepared graph")
    assert rp.graphSearchLast(ctx)[0] == model[1]


def test_prof_class_3_times_the_call(rp, ctx):
    from rptree_amd import _lib
    L = _lib.lib()
    n = 1000
    X = make_rows(14, n, 16)
    ds = rp.Dataset.dense(ctx, X)
    D = mref.metric_matrix(X, "l2")
    graph = mref.exact_graph(D, 5)
    _lib.check(L.rpt_prof_enable(ctx._h, 1))
    try:
        _lib.check(L.rpt_prof_reset(ctx._h))
        rp.graphPrepare(graph, ds, kout=8)
        ms, cnt = C.c_double(), C.c_int64()
        _lib.check(L.rpt_prof_get(ctx._h, 3, C.byref(ms), C.byref(cnt)))
        assert cnt.value == 1 and ms.value > 0.0
    finally:
        _lib.check(L.rpt_prof_enable(ctx._h, 0))
