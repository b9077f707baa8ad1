"""Best-first beam search over the kNN graph on the device (rpt_graph_search_host / _dev,
csrc/graph_search.hip): ids, counts and distance BITS, and the statistics of the call, against the
numpy restatement in tests/graph_search_ref.py."""
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
import graph_search_ref as sref  # noqa: E402

RPT_E_ARG, RPT_E_UNSUPPORTED = -1, -4
METRICS = ("l2", "cosine", "inner")
K_EF = [(1, 1), (10, 10), (10, 32), (64, 64), (10, 65), (10, 256), (64, 256)]


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


def make_queries(X, rng, nq=64):
    """stored rows (the zero row and a duplicated row among them), perturbed rows and one zero query"""
    n = X.shape[0]
    stored = np.concatenate([[9, 17, 5], rng.choice(n, nq // 2 - 3, replace=False)])
    pert = rng.choice(n, nq - len(stored) - 1, replace=False)
    Q = np.concatenate([X[stored], X[pert] + 0.2 * rng.standard_normal((len(pert), X.shape[1])),
                        np.zeros((1, X.shape[1]))])
    assert Q.shape[0] == nq
    return Q


def make_seeds(rng, nq, n, s):
    """random seeds; with s = 8 a repeated id in every row, -1 padding in every third; row 7 has none"""
    seeds = rng.integers(0, n, size=(nq, s)).astype(np.int32)
    if s >= 8:
        seeds[:, 5] = seeds[:, 1]
        seeds[::3, 6:] = -1
        seeds[1, 0] = -1
    seeds[7, :] = -1
    return seeds


def search(rp, ctx, graph, ds, Q, k, ef, seeds, metric):
    got = rp.graphSearch(graph, ds, Q, k, ef=ef, seeds=seeds, metric=distf(rp, metric))
    return got, rp.graphSearchLast(ctx)


def check_padding(got, k):
    pad = np.arange(k)[None, :] >= got[2][:, None]
    assert np.all(got[0][pad] == -1) and np.all(np.isposinf(got[1][pad]))


def cut(want, k):
    """the first k of an answer computed with a larger k"""
    ids, dist, cnt = want
    return ids[:, :k], dist[:, :k], np.minimum(cnt, k).astype(np.int32)


# ---------------------------------------------------------------- the grid
_data = {}


def grid_data(rp, ctx, dtype, d):
    """data set, forest, queries and per metric the query-to-row distances, built once"""
    key = (dtype, d)
    if key not in _data:
        n, T, minl = 1500, 3, 40
        arr, X64 = as_dtype(rp, make_rows(d, n, d), dtype)
        ds = dataset(rp, ctx, arr, dtype)
        cfg = rp.rpTreeCfg(minl, n, d)
        f = rp.forestBatch(1234 + d, cfg.fpMaxTreeDepth, minl, T, cfg.fpProjNzDensity, d, ds, ctx=ctx)
        qarr, Q64 = as_dtype(rp, make_queries(X64, np.random.default_rng(100 + d)), dtype)
        _data[key] = (ds, X64, f, qarr, Q64, {}, {})
    return _data[key]


@pytest.mark.parametrize("s", [1, 8])
@pytest.mark.parametrize("kg", [10, 64])
@pytest.mark.parametrize("d", [24, 200])
@pytest.mark.parametrize("dtype", ["f64", "f32", "bf16"])
@pytest.mark.parametrize("metric", METRICS)
def test_search_matches_the_definition(rp, ctx, metric, dtype, d, kg, s):
    ds, X64, f, qarr, Q64, Ds, graphs = grid_data(rp, ctx, dtype, d)
    n, nq = X64.shape[0], Q64.shape[0]
    if metric not in Ds:
        Ds[metric] = sref.query_matrix(X64, Q64, metric)
    if (metric, kg) not in graphs:
        graphs[(metric, kg)] = rp.knnGraphMetric(distf(rp, metric), kg, f)
    graph = graphs[(metric, kg)]
    if kg == 64:
        assert graph[2].min() < kg                         # ragged rows
    seeds = make_seeds(np.random.default_rng(7 * s + kg), nq, n, s)
    wants = {}
    for k, ef in K_EF:
        tag = "%s %s d %d kg %d s %d k %d ef %d" % (metric, dtype, d, kg, s, k, ef)
        if ef not in wants:
            wants[ef] = sref.graph_search_ref(X64, Q64, graph[0], graph[2], seeds, min(ef, 64), ef, metric,
                                              D=Ds[metric])
        want, exp, offered, upper = wants[ef]
        got, (g_exp, g_eval) = search(rp, ctx, graph, ds, qarr, k, ef, seeds, metric)
        print("%s: expansions %d, evaluated %d in [%d, %d]" % (tag, g_exp, g_eval, offered, upper))
        sref.assert_same_answer(got, cut(want, k), tag)
        check_padding(got, k)
        assert got[2][7] == 0
        assert g_exp == exp, tag
        assert offered <= g_eval <= upper, tag
        with option(ctx, "graph_search_nofilter", 1):
            got2, (n_exp, n_eval) = search(rp, ctx, graph, ds, qarr, k, ef, seeds, metric)
        sref.assert_same_answer(got2, got, tag + ", graph_search_nofilter")
        assert n_exp == exp and n_eval >= g_eval and n_eval <= upper, tag


# ---------------------------------------------------------------- the exhaustive case
@pytest.mark.parametrize("metric,dtype", [("l2", "f64")] + [(m, t) for m in ("cosine", "inner")
                                                          for t in ("f64", "f32", "bf16")])
def test_complete_graph_gives_the_brute_force_answer(rp, ctx, metric, dtype):
    """n = 60, every point lists all others, ef = 64, one seed: the beam ends up holding every point
    and the answer is bruteKnn's bit for bit (L2: on f64 rows, where brute force is this fold too)"""
    n, d, k = 60, 19, 60
    rng = np.random.default_rng(60)
    X = rng.standard_normal((n, d))
    X[11] = X[40]
    arr, X64 = as_dtype(rp, X, dtype)
    ds = dataset(rp, ctx, arr, dtype)
    qarr, Q64 = as_dtype(rp, np.concatenate([X64[:8], rng.standard_normal((8, d))]), dtype)
    gids = np.array([[j for j in range(n) if j != i] for i in range(n)], dtype=np.int32)
    gcnt = np.full(n, n - 1, dtype=np.int32)
    seeds = rng.integers(0, n, size=(16, 1)).astype(np.int32)
    got, (exp, evaluated) = search(rp, ctx, (gids, gcnt), ds, qarr, k, 64, seeds, metric)
    bi, bd = rp.bruteKnn(ds, qarr, k, metric=distf(rp, metric))
    sref.assert_same_answer(got, (bi, bd, np.full(16, k, dtype=np.int32)), "brute force")
    want, w_exp, offered, upper = sref.graph_search_ref(X64, Q64, gids, gcnt, seeds, k, 64, metric)
    sref.assert_same_answer(got, want, "restatement")
    assert exp == w_exp == 16 * n and offered == evaluated == 16 * n


# ---------------------------------------------------------------- shapes
def _ring_graph(n, kg):
    gids = np.array([[(i + 1 + e) % n for e in range(kg)] for i in range(n)], dtype=np.int32)
    return gids, np.full(n, kg, dtype=np.int32)


def test_no_queries_one_point_and_no_seeds(rp, ctx):
    d = 8
    X = np.random.default_rng(1).standard_normal((50, d))
    ds = rp.Dataset.dense(ctx, X)
    graph = _ring_graph(50, 3)
    ids, dist, cnt = rp.graphSearch(graph, ds, np.zeros((0, d)), 5, seeds=np.zeros((0, 2), dtype=np.int32))
    assert ids.shape == (0, 5) and dist.shape == (0, 5) and cnt.shape == (0,)
    assert rp.graphSearchLast(ctx) == (0, 0)
    # every seed -1: count 0
    Q = X[:4] + 0.01
    got = rp.graphSearch(graph, ds, Q, 5, seeds=np.full((4, 3), -1, dtype=np.int32))
    assert np.all(got[2] == 0) and np.all(got[0] == -1) and np.all(np.isposinf(got[1]))
    assert rp.graphSearchLast(ctx) == (0, 0)
    # n = 1
    one = rp.Dataset.dense(ctx, X[:1])
    g1 = (np.full((1, 2), -1, dtype=np.int32), np.zeros(1, dtype=np.int32))
    seeds = np.array([[0], [-1], [0], [0]], dtype=np.int32)
    got = rp.graphSearch(g1, one, Q, 3, ef=3, seeds=seeds)
    want = sref.graph_search_ref(X[:1], Q, g1[0], g1[1], seeds, 3, 3)
    sref.assert_same_answer(got, want[0], "n = 1")
    assert got[2].tolist() == [1, 0, 1, 1] and rp.graphSearchLast(ctx) == (3, 3)
    # n = 0: every count is 0
    none = rp.Dataset.dense(ctx, np.zeros((0, d)))
    g0 = (np.zeros((0, 2), dtype=np.int32), np.zeros(0, dtype=np.int32))
    got = rp.graphSearch(g0, none, Q, 3, seeds=np.full((4, 2), -1, dtype=np.int32))
    assert np.all(got[2] == 0) and np.all(got[0] == -1)


def test_seed_with_an_empty_row_and_disconnected_halves(rp, ctx):
    n, d, k = 40, 12, 10
    X = np.random.default_rng(2).standard_normal((n, d))
    ds = rp.Dataset.dense(ctx, X)
    # half A = ids 0 .. 5 (smaller than k), half B = the rest; row 3 and row 20 are empty
    gids = np.full((n, 6), -1, dtype=np.int32)
    gcnt = np.zeros(n, dtype=np.int32)
    for i in range(n):
        half = [j for j in (range(6) if i < 6 else range(6, n)) if j != i]
        row = half[:5] if i < 6 else [half[(i + e) % len(half)] for e in range(6)]
        row = sorted(set(row))
        gids[i, :len(row)], gcnt[i] = row, len(row)
    gcnt[3] = 0
    gcnt[20] = 0
    Q = np.concatenate([X[:3] + 0.05, X[30:33] + 0.05])
    seeds = np.array([[3, -1], [3, 4], [0, 0], [20, -1], [20, 21], [39, 7]], dtype=np.int32)
    got = rp.graphSearch((gids, gcnt), ds, Q, k, ef=16, seeds=seeds)
    stats = rp.graphSearchLast(ctx)
    want, exp, offered, upper = sref.graph_search_ref(X, Q, gids, gcnt, seeds, k, 16)
    sref.assert_same_answer(got, want, "halves")
    assert stats[0] == exp and offered <= stats[1] <= upper
    assert got[2].tolist() == [1, 6, 6, 1, 10, 10]          # an empty row leads nowhere; A holds 6 points
    assert got[0][0, 0] == 3 and got[0][3, 0] == 20
    for i in range(6):
        c = got[2][i]
        assert np.all(got[0][i, :c] < 6) if i < 3 else np.all(got[0][i, :c] >= 6)
    check_padding(got, k)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", ["f64", "f32", "bf16"])
@pytest.mark.parametrize("d", [1, 33])
def test_chunk_edges(rp, ctx, d, dtype, metric):
    """d = 1 and d = 33 = one staged chunk plus one column"""
    n, kg, k, ef = 300, 7, 5, 12
    arr, X64 = as_dtype(rp, make_rows(d + 1, n, d), dtype)
    ds = dataset(rp, ctx, arr, dtype)
    rng = np.random.default_rng(d)
    qarr, Q64 = as_dtype(rp, X64[rng.choice(n, 20)] + 0.3 * rng.standard_normal((20, d)), dtype)
    graph = _ring_graph(n, kg)
    graph[0][:, 3] = rng.integers(0, n, size=n)            # a random chord: the ring alone is a long walk
    seeds = rng.integers(0, n, size=(20, 4)).astype(np.int32)
    got, stats = search(rp, ctx, graph, ds, qarr, k, ef, seeds, metric)
    want, exp, offered, upper = sref.graph_search_ref(X64, Q64, graph[0], graph[1], seeds, k, ef, metric)
    sref.assert_same_answer(got, want, "d %d %s %s" % (d, dtype, metric))
    assert stats[0] == exp and offered <= stats[1] <= upper


def test_wide_rows_beyond_the_resident_query(rp, ctx):
    """d = 1100: the query no longer stays in LDS whole, its chunks are staged next to the rows'"""
    n, d, kg, k, ef = 200, 1100, 6, 8, 20
    rng = np.random.default_rng(11)
    X = rng.standard_normal((n, d))
    ds = rp.Dataset.dense(ctx, X)
    Q = X[:10] + 0.5 * rng.standard_normal((10, d))
    graph = _ring_graph(n, kg)
    graph[0][:, 2] = rng.integers(0, n, size=n)
    seeds = rng.integers(0, n, size=(10, 3)).astype(np.int32)
    for metric in METRICS:
        got, stats = search(rp, ctx, graph, ds, Q, k, ef, seeds, metric)
        want, exp, offered, upper = sref.graph_search_ref(X, Q, graph[0], graph[1], seeds, k, ef, metric)
        sref.assert_same_answer(got, want, "d 1100 " + metric)
        assert stats[0] == exp and offered <= stats[1] <= upper


# ---------------------------------------------------------------- determinism, device arrays
@pytest.mark.parametrize("metric", METRICS)
def test_two_calls_and_the_dev_entry_point_give_the_same_bits(rp, ctx, metric):
    import torch
    n, d, kg, k, ef, s, nq = 2500, 64, 10, 10, 48, 6, 200
    X = make_rows(13, n, d)
    dev = torch.device("cuda", ctx.device)
    t = torch.from_numpy(X).to(dev)
    ds = rp.Dataset.from_torch(ctx, t)
    cfg = rp.rpTreeCfg(50, n, d)
    f = rp.forestBatch(8, cfg.fpMaxTreeDepth, 50, 3, cfg.fpProjNzDensity, d, ds, ctx=ctx)
    df = distf(rp, metric)
    graph = rp.knnGraphMetric(df, kg, f)
    rng = np.random.default_rng(5)
    Q = X[rng.choice(n, nq)] + 0.2 * rng.standard_normal((nq, d))
    seeds = rng.integers(0, n, size=(nq, s)).astype(np.int32)
    a, sa = search(rp, ctx, graph, ds, Q, k, ef, seeds, metric)
    b, sb = search(rp, ctx, graph, ds, Q, k, ef, seeds, metric)
    sref.assert_same_answer(a, b, "second call")
    assert sa == sb

    def on_device(gids, gcnt):
        tq = torch.from_numpy(Q).to(dev)
        qd = rp.Dataset.from_torch(ctx, tq)
        tg, tc, ts = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (gids, gcnt, seeds))
        ids = torch.empty((nq, k), dtype=torch.int32, device=dev)
        dist = torch.empty((nq, k), dtype=torch.float64, device=dev)
        cnt = torch.empty(nq, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        rp.graphSearchDev(ds, qd, kg, tg.data_ptr(), tc.data_ptr(), s, ts.data_ptr(), k, ef, ids.data_ptr(),
                          dist.data_ptr(), cnt.data_ptr(), metric=df)
        ctx.sync()
        return (ids.cpu().numpy(), dist.cpu().numpy(), cnt.cpu().numpy()), rp.graphSearchLast(ctx)

    c, sc = on_device(graph[0], graph[2])
    sref.assert_same_answer(c, a, "dev against host")
    assert sc == sa
    # _dev does not validate: an id >= n, a negative id and a count > kg are skipped, never followed
    gids, gcnt = np.array(graph[0]), np.array(graph[2])
    hub = int(a[0][0, 0])                                  # rows that the searches do reach
    gids[hub, 1] = n + 5
    gids[int(a[0][1, 0]), 0] = -7
    gcnt[int(a[0][2, 0])] = kg + 3
    gids[17, 0] = 2 ** 31 - 1
    got, sg = on_device(gids, gcnt)
    X64 = X
    want, exp, offered, upper = sref.graph_search_ref(X64, Q, gids, gcnt, seeds, k, ef, metric)
    sref.assert_same_answer(got, want, "planted graph")
    assert sg[0] == exp and offered <= sg[1] <= upper
    clean_ids = np.full_like(gids, -1)
    clean_cnt = np.zeros_like(gcnt)
    for i in range(n):                                     # the cleaned graph: what is skipped, removed
        row = [v for v in gids[i, :gcnt[i]].tolist() if 0 <= v < n] if 0 <= gcnt[i] <= kg else []
        clean_ids[i, :len(row)], clean_cnt[i] = row, len(row)
    want2 = sref.graph_search_ref(X64, Q, clean_ids, clean_cnt, seeds, k, ef, metric)
    sref.assert_same_answer(got, want2[0], "cleaned graph")
    assert want2[1] == exp


# ---------------------------------------------------------------- refusals
def test_refusals_leave_the_context_usable(rp, ctx, oracle):
    from rptree_amd import _lib
    L = _lib.lib()
    n, d, T, minl, kg, k, s, nq = 1500, 16, 4, 30, 10, 10, 4, 16
    X = oracle.data_normal_dense2(12, n, d)
    ds = rp.Dataset.dense(ctx, X)
    cfg = rp.rpTreeCfg(minl, n, d)
    f = rp.forestBatch(7, cfg.fpMaxTreeDepth, minl, T, cfg.fpProjNzDensity, d, ds, ctx=ctx)
    graph = rp.knnGraph(kg, f)
    Q = oracle.data_normal_dense2(13, nq, d)
    qd = rp.Dataset.dense(ctx, Q)
    seeds0 = np.random.default_rng(3).integers(0, n, size=(nq, s)).astype(np.int32)

    def knn_matches_the_oracle():
        fo = oracle.forest_build_dense(X, f.R, minl)
        ids, dist, cnt = rp.knnBatch(k, f, Q)
        for i in range(nq):
            wi, wd = oracle.knn_dense(fo, X, Q[i], k)
            assert np.array_equal(ids[i, :cnt[i]], wi)
            assert np.allclose(dist[i, :cnt[i]], wd, rtol=1e-12)

    knn_matches_the_oracle()
    tier = C.c_int32(-1)
    _lib.check(L.rpt_knn_last_tier(ctx._h, C.byref(tier)))
    tier0 = tier.value
    good = rp.graphSearch(graph, ds, Q, k, ef=32, seeds=seeds0)
    stats = rp.graphSearchLast(ctx)
    COS, INN, REF = rp.RPT_KNN_METRIC_COSINE, rp.RPT_KNN_METRIC_INNER, rp.RPT_KNN_METRIC_REFERENCE

    def refused(code, data=ds, queries=qd, kg_=kg, s_=s, k_=k, ef_=32, metric=0, flags=0, gids=None, gcnt=None,
                seeds=None):
        gids = np.ascontiguousarray(graph[0] if gids is None else gids, dtype=np.int32)
        gcnt = np.ascontiguousarray(graph[2] if gcnt is None else gcnt, dtype=np.int32)
        seeds = np.ascontiguousarray(seeds0 if seeds is None else seeds, dtype=np.int32)
        ids = np.full((nq, 64), 12345, dtype=np.int32)
        dist = np.full((nq, 64), 0.5)
        cnt = np.full(nq, 77, dtype=np.int32)
        st = L.rpt_graph_search_host(ctx._h, data._h, queries._h, kg_, C.c_void_p(gids.ctypes.data),
                                     C.c_void_p(gcnt.ctypes.data), s_, C.c_void_p(seeds.ctypes.data), k_, ef_,
                                     metric, flags, C.c_void_p(ids.ctypes.data), C.c_void_p(dist.ctypes.data),
                                     C.c_void_p(cnt.ctypes.data))
        assert st == code, (st, code)
        msg = L.rpt_last_error().decode()
        assert len(msg) > 8, msg
        assert np.all(ids == 12345) and np.all(dist == 0.5) and np.all(cnt == 77)   # nothing was written
        assert rp.graphSearchLast(ctx) == stats            # nothing was launched
        return msg

    assert "k" in refused(RPT_E_ARG, k_=0)
    assert "k" in refused(RPT_E_ARG, k_=65, ef_=100)
    assert "ef" in refused(RPT_E_ARG, ef_=257)
    assert "ef" in refused(RPT_E_ARG, k_=10, ef_=9)
    assert "s " in refused(RPT_E_ARG, s_=0)
    assert "s " in refused(RPT_E_ARG, s_=65)
    assert "kg" in refused(RPT_E_ARG, kg_=0)
    assert "kg" in refused(RPT_E_ARG, kg_=65)
    assert "flags" in refused(RPT_E_ARG, flags=1)
    assert "flags" in refused(RPT_E_ARG, flags=COS)
    assert "metric" in refused(RPT_E_ARG, metric=COS | INN)
    assert "metric" in refused(RPT_E_ARG, metric=REF)
    assert "metric" in refused(RPT_E_ARG, metric=2)
    assert "metric" in refused(RPT_E_ARG, metric=INN | 1)
    q_d = rp.Dataset.dense(ctx, np.zeros((nq, d + 1)))
    assert "d or dtype" in refused(RPT_E_ARG, queries=q_d)
    q_32 = rp.Dataset.dense(ctx, Q.astype(np.float32))
    assert "d or dtype" in refused(RPT_E_ARG, queries=q_32)
    rowptr = np.arange(n + 1, dtype=np.int64)
    csr = rp.Dataset.csr(ctx, rowptr, np.zeros(n, dtype=np.int32), np.ones(n), d)
    qptr = np.arange(nq + 1, dtype=np.int64)
    qcsr = rp.Dataset.csr(ctx, qptr, np.zeros(nq, dtype=np.int32), np.ones(nq), d)
    assert "both" in refused(RPT_E_ARG, queries=qcsr)
    assert "both" in refused(RPT_E_ARG, data=csr)
    for m in (0, COS, INN):
        assert "CSR" in refused(RPT_E_UNSUPPORTED, data=csr, queries=qcsr, metric=m)
    # _host names the row of the graph or of the seeds that is out of range
    bad = np.array(graph[2])
    bad[700] = kg + 1
    assert "graph row 700" in refused(RPT_E_ARG, gcnt=bad)
    bad[700] = -1
    assert "graph row 700" in refused(RPT_E_ARG, gcnt=bad)
    bad = np.array(graph[0])
    bad[701, 0] = n
    assert graph[2][701] > 0 and "graph row 701" in refused(RPT_E_ARG, gids=bad)
    bad[701, 0] = -1
    assert "graph row 701" in refused(RPT_E_ARG, gids=bad)
    bad = seeds0.copy()
    bad[5, 2] = n
    assert "seeds row 5" in refused(RPT_E_ARG, seeds=bad)
    bad[5, 2] = -2
    assert "seeds row 5" in refused(RPT_E_ARG, seeds=bad)
    # ids behind a row's count are not looked at
    fine = np.array(graph[0])
    short = int(np.argmin(graph[2]))
    if graph[2][short] < kg:
        fine[short, kg - 1] = n + 9
    again = rp.graphSearch((fine, graph[2]), ds, Q, k, ef=32, seeds=seeds0)
    sref.assert_same_answer(again, good, "after the refusals")
    with pytest.raises(rp.RPTError) as e:
        rp.graphSearch(graph, ds, Q, k, ef=5, seeds=seeds0)
    assert e.value.code == RPT_E_ARG
    with pytest.raises(ValueError):
        rp.graphSearch(graph, ds, Q, k)                    # neither seeds nor a forest
    # the kNN entry points are untouched
    _lib.check(L.rpt_knn_last_tier(ctx._h, C.byref(tier)))
    assert tier.value == tier0
    knn_matches_the_oracle()


# ---------------------------------------------------------------- seeds from a forest, the profile class
@pytest.mark.parametrize("metric", METRICS)
def test_seeds_from_a_forest(rp, ctx, metric):
    n, d, kg, k = 3000, 32, 10, 10
    arr, X64 = as_dtype(rp, make_rows(21, n, d), "f32")
    ds = rp.Dataset.dense(ctx, arr)
    cfg = rp.rpTreeCfg(60, n, d)
    f = rp.forestBatch(9, cfg.fpMaxTreeDepth, 60, 2, cfg.fpProjNzDensity, d, ds, ctx=ctx)
    df = distf(rp, metric)
    graph = rp.knnGraphRefineMetric(df, rp.knnGraphMetric(df, kg, f), f, iters=1)
    rng = np.random.default_rng(8)
    Q = (X64[rng.choice(n, 50)] + 0.2 * rng.standard_normal((50, d))).astype(np.float32)
    got = rp.graphSearch(graph, f, Q, k, ef=32, forest=f, metric=df)
    stats = rp.graphSearchLast(ctx)
    sid, _, scnt = rp.knnBatch(8, f, Q, dedup=True, metric=df)
    seeds = np.where(np.arange(8)[None, :] < scnt[:, None], sid, -1).astype(np.int32)
    want = rp.graphSearch(graph, ds, Q, k, ef=32, seeds=seeds, metric=df)
    sref.assert_same_answer(got, want, "forest seeds")
    assert rp.graphSearchLast(ctx) == stats
    model, exp, offered, upper = sref.graph_search_ref(X64, Q.astype(np.float64), graph[0], graph[2], seeds, k, 32,
                                                       metric)
    sref.assert_same_answer(got, model, "restatement")
    assert stats[0] == exp and offered <= stats[1] <= upper
    # ef = None means max(k, 32)
    sref.assert_same_answer(rp.graphSearch(graph, ds, Q, k, seeds=seeds, metric=df), want, "default ef")


def test_prof_class_3_times_the_call(rp, ctx):
    from rptree_amd import _lib
    L = _lib.lib()
    X = make_rows(14, 1000, 16)
    ds = rp.Dataset.dense(ctx, X)
    graph = _ring_graph(1000, 5)
    seeds = np.arange(40, dtype=np.int32).reshape(20, 2)
    _lib.check(L.rpt_prof_enable(ctx._h, 1))
    try:
        _lib.check(L.rpt_prof_reset(ctx._h))
        rp.graphSearch(graph, ds, X[:20], 5, ef=8, seeds=seeds)
        ms, cnt = C.c_double(), C.c_int64()
        _lib.check(L.rpt_prof_get(ctx._h, 3, C.byref(ms), C.byref(cnt)))
        assert cnt.value == 1 and ms.value > 0.0
    finally:
        _lib.check(L.rpt_prof_enable(ctx._h, 0))
