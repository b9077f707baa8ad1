"""Beam search over an allow-list of ids on the device (rpt_graph_search_allow_host / _dev; the F
switch of csrc/graph_dev.h's beam, graph_search_allow_kernel and graph_search_csr_allow_kernel): ids,
counts, distance BITS and `expansions` against the numpy restatement in tests/graph_search_allow_ref.py
and, with every id allowed, against the unfiltered entry points.  No tolerance anywhere.

The grid's rows are lattice points (small integers, queries at half-integers), which f64, f32 and bf16
hold exactly: the three dtypes share one matrix of distances and one restatement per case, ties are
heavy, and one insertion really drops several beam entries."""
import contextlib
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graph_search_ref as sref  # noqa: E402
import graph_search_allow_ref as aref  # noqa: E402
import graph_metric_csr_ref as gm  # noqa: E402

RPT_E_ARG = -1
METRICS = ("l2", "cosine", "inner")
NP = {"f64": np.float64, "f32": np.float32}
EF_WIDTH = [(10, 10), (10, 64), (32, 65), (32, 256), (64, 257), (256, 1024)]     # the lane-block edges 64 | 65, 256 | 257
ALLOW = ("null", "ones", "half", "tenth", "one", "zero")
N, NQ = 500, 64                                                                   # n is no multiple of 32


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


def lattice_rows(seed, n, d):
    """integers in [-2, 2]: exact duplicates under other ids, a zero row (NaN from everything under cosine)"""
    X = np.random.default_rng(seed).integers(-2, 3, size=(n, d)).astype(np.float64)
    if n > 40:
        X[5] = X[17]
        X[n - 3] = X[17]
        X[31] = X[30]
        X[9] = 0.0
    return X


def lattice_queries(X, rng, nq):
    """stored rows (the zero row and a duplicated row among them), rows moved by half-integers, a zero query"""
    n = X.shape[0]
    stored = np.concatenate([[9, 17, 5], rng.choice(n, nq // 2 - 3, replace=False)])
    pert = rng.choice(n, nq - len(stored) - 1, replace=False)
    Q = np.concatenate([X[stored], X[pert] + 0.5 * rng.integers(-1, 2, size=(len(pert), X.shape[1])),
                        np.zeros((1, X.shape[1]))])
    assert Q.shape[0] == nq
    return Q


def make_graph(rng, n, kg):
    """every row lists successors on the ring and random chords; ragged counts"""
    gids = np.array([[(i + 1 + e) % n for e in range(kg)] for i in range(n)], dtype=np.int32)
    chord = rng.random((n, kg)) < 0.5
    gids[chord] = rng.integers(0, n, size=int(chord.sum()))
    gcnt = rng.integers(max(1, kg // 2), kg + 1, size=n).astype(np.int32)
    gcnt[3] = 0
    return gids, gcnt


def make_seeds(rng, nq, n, s):
    """random seeds; with s = 8 a repeated id in every row, -1 padding in every third; row 7 has none"""
    seeds = rng.integers(0, n, size=(nq, s)).astype(np.int32)
    if s >= 8:
        seeds[:, 5] = seeds[:, 1]
        seeds[::3, 6:] = -1
        seeds[1, 0] = -1
    seeds[7, :] = -1
    return seeds


def allow_of(kind, n):
    """-> (what graphSearchAllow is handed, the bool mask of the restatement)"""
    rng = np.random.default_rng(77)
    if kind == "null":
        return None, np.ones(n, dtype=bool)
    if kind == "ones":
        return np.ones(n, dtype=bool), np.ones(n, dtype=bool)
    if kind == "half":
        m = rng.random(n) < 0.5
    elif kind == "tenth":
        m = rng.random(n) < 0.1
    elif kind == "one":
        m = np.zeros(n, dtype=bool)
        m[n - 2] = True                                    # in the last, partial word
    else:
        m = np.zeros(n, dtype=bool)
    return m, m


def check_padding(got, k):
    pad = np.arange(k)[None, :] >= got[2][:, None]
    assert np.all(got[0][pad] == -1) and np.all(np.isposinf(got[1][pad]))


def k_of(ef):
    return 10 if ef < 64 else 64


# ---------------------------------------------------------------- the definition, dense rows
_dense, _want = {}, {}


def dense_case(rp, ctx, d):
    """per d: the lattice rows and queries, one Dataset pair per dtype, the distances per metric"""
    if d not in _dense:
        X = lattice_rows(d, N, d)
        Q = lattice_queries(X, np.random.default_rng(100 + d), NQ)
        per = {}
        for dtype in ("f64", "f32", "bf16"):
            arr, X64 = as_dtype(rp, X, dtype)
            qarr, Q64 = as_dtype(rp, Q, dtype)
            assert np.array_equal(X64, X) and np.array_equal(Q64, Q)          # the lattice is exact in every dtype
            per[dtype] = (dataset(rp, ctx, arr, dtype), qarr)
        _dense[d] = (X, Q, per, {})
    return _dense[d]


@pytest.mark.parametrize("allow", ALLOW)
@pytest.mark.parametrize("s", [1, 8])
@pytest.mark.parametrize("kg", [10, 64])
@pytest.mark.parametrize("d", [24, 200])
@pytest.mark.parametrize("metric", METRICS)
def test_search_matches_the_definition(rp, ctx, metric, d, kg, s, allow):
    X, Q, per, Ds = dense_case(rp, ctx, d)
    if metric not in Ds:
        Ds[metric] = sref.query_matrix(X, Q, metric)
    gids, gcnt = make_graph(np.random.default_rng(kg), N, kg)
    seeds = make_seeds(np.random.default_rng(7 * s + kg), NQ, N, s)
    given, mask = allow_of(allow, N)
    for ef, width in EF_WIDTH:
        k = k_of(ef)
        key = (metric, d, kg, s, ef, width, "all" if mask.all() else allow)
        if key not in _want:
            _want[key] = aref.graph_search_allow_ref(X, Q, gids, gcnt, seeds, k, ef, width, mask, metric, D=Ds[metric])
        want, exp, offered, upper = _want[key]
        for dtype in ("f64", "f32", "bf16"):
            tag = "%s %s d %d kg %d s %d ef %d width %d allow %s" % (metric, dtype, d, kg, s, ef, width, allow)
            ds, qarr = per[dtype]
            got = rp.graphSearchAllow(given, (gids, gcnt), ds, qarr, k, ef=ef, width=width, seeds=seeds,
                                      metric=distf(rp, metric))
            g_exp, g_eval = rp.graphSearchLast(ctx)
            sref.assert_same_answer(got, want, tag)
            check_padding(got, k)
            assert got[2][7] == 0
            assert g_exp == exp, tag
            assert offered <= g_eval <= upper, tag
        if allow == "zero":
            assert np.all(want[2] == 0)


# ---------------------------------------------------------------- the definition, CSR rows
_csr = {}


def lattice_csr(seed, n, d, density, dtype=np.float64):
    """gm.make_csr's supports with values rounded to integers in [-3, 3] (a stored zero among them)"""
    rowptr, col, val, dd = gm.make_csr(seed, n, d, density, dtype)
    return rowptr, col, np.clip(np.rint(2.0 * val), -3, 3).astype(dtype), dd


def csr_case():
    if not _csr:
        d = 70
        csrX = lattice_csr(70, N, d, 0.2)
        rows = gm.rows_of(csrX)
        qrows = [(c.copy(), v.copy()) for c, v in gm.rows_of(lattice_csr(71, NQ, d, 0.2))]
        for i, j in enumerate((17, 5, 400)):
            qrows[i] = rows[j]
        qrows[3] = (np.zeros(0, dtype=np.int32), np.zeros(0))
        csrQ = gm.from_rows(qrows, d)
        _csr["case"] = (csrX, csrQ, {})
    return _csr["case"]


def csr_distances(csrX, csrQ, metric):
    """L2: the fold over the dense-ified rows (rpt_graph_search_csr_*); cosine / inner product: dotS"""
    return gm.dense_query_matrix(csrX, csrQ, "l2") if metric == "l2" else gm.query_matrix(csrX, csrQ, metric)


def csr_as(csr, dtype):
    return csr[0], csr[1], csr[2].astype(NP[dtype]), csr[3]


@pytest.mark.parametrize("allow", ALLOW)
@pytest.mark.parametrize("metric", METRICS)
def test_search_matches_the_definition_on_csr_rows(rp, ctx, metric, allow):
    csrX, csrQ, Ds = csr_case()
    if metric not in Ds:
        Ds[metric] = csr_distances(csrX, csrQ, metric)
    kg, s = 10, 8
    gids, gcnt = make_graph(np.random.default_rng(kg), N, kg)
    seeds = make_seeds(np.random.default_rng(7 * s + kg), NQ, N, s)
    given, mask = allow_of(allow, N)
    X0, Q0 = np.zeros((N, 1)), np.zeros((NQ, 1))           # the restatement takes its distances from D
    for ef, width in EF_WIDTH:
        k = k_of(ef)
        want, exp, offered, upper = aref.graph_search_allow_ref(X0, Q0, gids, gcnt, seeds, k, ef, width, mask, metric,
                                                                D=Ds[metric])
        for dtype in ("f64", "f32"):
            tag = "csr %s %s ef %d width %d allow %s" % (metric, dtype, ef, width, allow)
            ds = rp.Dataset.csr(ctx, *csr_as(csrX, dtype))
            got = rp.graphSearchAllow(given, (gids, gcnt), ds, csr_as(csrQ, dtype), k, ef=ef, width=width, seeds=seeds,
                                      metric=distf(rp, metric))
            g_exp, g_eval = rp.graphSearchLast(ctx)
            sref.assert_same_answer(got, want, tag)
            check_padding(got, k)
            assert g_exp == exp and offered <= g_eval <= upper, tag
            with option(ctx, "graph_search_csr_stream", 1):
                again = rp.graphSearchAllow(given, (gids, gcnt), ds, csr_as(csrQ, dtype), k, ef=ef, width=width,
                                            seeds=seeds, metric=distf(rp, metric))
            sref.assert_same_answer(again, got, tag + ", graph_search_csr_stream")
            assert rp.graphSearchLast(ctx) == (g_exp, g_eval), tag


# ---------------------------------------------------------------- identity with every id allowed
@pytest.mark.parametrize("dtype", ["f64", "f32", "bf16"])
@pytest.mark.parametrize("metric", METRICS)
def test_every_id_allowed_is_the_unfiltered_entry_point(rp, ctx, metric, dtype):
    X, Q, per, _ = dense_case(rp, ctx, 24)
    ds, qarr = per[dtype]
    gids, gcnt = make_graph(np.random.default_rng(10), N, 10)
    seeds = make_seeds(np.random.default_rng(66), NQ, N, 8)
    for ef in (10, 70):
        want = rp.graphSearch((gids, gcnt), ds, qarr, 10, ef=ef, seeds=seeds, metric=distf(rp, metric))
        stats = rp.graphSearchLast(ctx)
        with option(ctx, "graph_search_nofilter", 1):
            rp.graphSearch((gids, gcnt), ds, qarr, 10, ef=ef, seeds=seeds, metric=distf(rp, metric))
            bare = rp.graphSearchLast(ctx)
        for width in (ef, 1024):
            for given in (None, np.ones(N, dtype=bool)):
                tag = "%s %s ef %d width %d" % (metric, dtype, ef, width)
                got = rp.graphSearchAllow(given, (gids, gcnt), ds, qarr, 10, ef=ef, width=width, seeds=seeds,
                                          metric=distf(rp, metric))
                sref.assert_same_answer(got, want, tag)
                assert rp.graphSearchLast(ctx)[0] == stats[0], tag
                with option(ctx, "graph_search_nofilter", 1):
                    got = rp.graphSearchAllow(given, (gids, gcnt), ds, qarr, 10, ef=ef, width=width, seeds=seeds,
                                              metric=distf(rp, metric))
                    sref.assert_same_answer(got, want, tag + ", graph_search_nofilter")
                    assert rp.graphSearchLast(ctx) == bare, tag       # `evaluated` too, without the hash


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("metric", METRICS)
def test_every_id_allowed_is_the_unfiltered_entry_point_on_csr_rows(rp, ctx, metric, dtype):
    csrX, csrQ, _ = csr_case()
    ds, qs = rp.Dataset.csr(ctx, *csr_as(csrX, dtype)), csr_as(csrQ, dtype)
    gids, gcnt = make_graph(np.random.default_rng(10), N, 10)
    seeds = make_seeds(np.random.default_rng(66), NQ, N, 8)
    ef = 32
    want = rp.graphSearchMetricSV(distf(rp, metric), (gids, gcnt), ds, qs, 10, ef=ef, seeds=seeds)
    stats = rp.graphSearchLast(ctx)
    if metric == "l2":
        sref.assert_same_answer(rp.graphSearchSV((gids, gcnt), ds, qs, 10, ef=ef, seeds=seeds), want, "graphSearchSV")
        assert rp.graphSearchLast(ctx) == stats
    for width in (ef, 1024):
        for given in (None, np.ones(N, dtype=bool)):
            got = rp.graphSearchAllow(given, (gids, gcnt), ds, qs, 10, ef=ef, width=width, seeds=seeds,
                                      metric=distf(rp, metric))
            sref.assert_same_answer(got, want, "csr %s %s width %d" % (metric, dtype, width))
            assert rp.graphSearchLast(ctx)[0] == stats[0]


# ---------------------------------------------------------------- every valid shape launches
@pytest.mark.parametrize("d", [1024, 1025])
def test_a_wide_beam_beside_a_resident_query_and_a_full_graph_row(rp, ctx, d):
    """kg = 64, width = 1024 and a query of 1024 columns in LDS (d = 1025: streamed): about 46 KB per wave,
    more than four waves may take together"""
    n, nq, kg, k, ef, width = 200, 12, 64, 10, 40, 1024
    rng = np.random.default_rng(d)
    X = rng.integers(-2, 3, size=(n, d)).astype(np.float64)
    Q = X[rng.choice(n, nq)] + 0.5 * rng.integers(-1, 2, size=(nq, d))
    ds = rp.Dataset.dense(ctx, X)
    gids, gcnt = make_graph(rng, n, kg)
    seeds = rng.integers(0, n, size=(nq, 3)).astype(np.int32)
    mask = rng.random(n) < 0.3
    got = rp.graphSearchAllow(mask, (gids, gcnt), ds, Q, k, ef=ef, width=width, seeds=seeds)
    stats = rp.graphSearchLast(ctx)
    want, exp, offered, upper = aref.graph_search_allow_ref(X, Q, gids, gcnt, seeds, k, ef, width, mask)
    sref.assert_same_answer(got, want, "d %d" % d)
    assert stats[0] == exp and offered <= stats[1] <= upper


@pytest.mark.parametrize("qnnz", [2048, 2049])
def test_a_wide_beam_beside_a_long_csr_query(rp, ctx, qnnz):
    """d = 4096, queries of 2048 entries (resident) and of 2049 (streamed), width = 1024, kg = 64"""
    n, nq, d, kg, k, ef, width = 200, 6, 4096, 64, 10, 40, 1024
    rng = np.random.default_rng(qnnz)
    csrX = lattice_csr(5, n, d, 0.02)
    qrows = []
    for _ in range(nq):
        cols = np.sort(rng.choice(d, size=qnnz, replace=False)).astype(np.int32)
        qrows.append((cols, rng.integers(-2, 3, size=qnnz).astype(np.float64)))
    csrQ = gm.from_rows(qrows, d)
    gids, gcnt = make_graph(rng, n, kg)
    seeds = rng.integers(0, n, size=(nq, 3)).astype(np.int32)
    mask = rng.random(n) < 0.3
    ds = rp.Dataset.csr(ctx, *csrX)
    for metric in METRICS:
        D = csr_distances(csrX, csrQ, metric)
        got = rp.graphSearchAllow(mask, (gids, gcnt), ds, csrQ, k, ef=ef, width=width, seeds=seeds,
                                  metric=distf(rp, metric))
        stats = rp.graphSearchLast(ctx)
        want, exp, offered, upper = aref.graph_search_allow_ref(np.zeros((n, 1)), np.zeros((nq, 1)), gids, gcnt, seeds,
                                                                k, ef, width, mask, metric, D=D)
        sref.assert_same_answer(got, want, "query of %d entries, %s" % (qnnz, metric))
        assert stats[0] == exp and offered <= stats[1] <= upper


# ---------------------------------------------------------------- options, determinism, device arrays
def test_the_visited_filter_changes_no_bit(rp, ctx):
    X, Q, per, _ = dense_case(rp, ctx, 24)
    ds, qarr = per["f64"]
    gids, gcnt = make_graph(np.random.default_rng(10), N, 10)
    seeds = make_seeds(np.random.default_rng(5), NQ, N, 8)
    _, mask = allow_of("tenth", N)
    for ef, width in ((10, 64), (32, 300)):
        got = rp.graphSearchAllow(mask, (gids, gcnt), ds, qarr, 10, ef=ef, width=width, seeds=seeds)
        exp, ev = rp.graphSearchLast(ctx)
        with option(ctx, "graph_search_nofilter", 1):
            bare = rp.graphSearchAllow(mask, (gids, gcnt), ds, qarr, 10, ef=ef, width=width, seeds=seeds)
            b_exp, b_ev = rp.graphSearchLast(ctx)
        sref.assert_same_answer(bare, got, "graph_search_nofilter")
        assert b_exp == exp and b_ev >= ev


def test_two_calls_and_the_dev_entry_point_give_the_same_bits(rp, ctx):
    import torch
    n, d, kg, k, ef, width, s, nq = 2500, 64, 10, 10, 32, 200, 6, 200
    X = lattice_rows(13, n, d)
    dev = torch.device("cuda", ctx.device)
    t = torch.from_numpy(X).to(dev)
    ds = rp.Dataset.from_torch(ctx, t)
    rng = np.random.default_rng(5)
    gids, gcnt = make_graph(rng, n, kg)
    Q = X[rng.choice(n, nq)] + 0.5 * rng.integers(-1, 2, size=(nq, d))
    seeds = rng.integers(0, n, size=(nq, s)).astype(np.int32)
    mask = rng.random(n) < 0.2
    a = rp.graphSearchAllow(mask, (gids, gcnt), ds, Q, k, ef=ef, width=width, seeds=seeds)
    sa = rp.graphSearchLast(ctx)
    b = rp.graphSearchAllow(rp.allowBitmap(mask, n), (gids, gcnt), ds, Q, k, ef=ef, width=width, seeds=seeds)
    sref.assert_same_answer(a, b, "second call, the words")
    assert rp.graphSearchLast(ctx) == sa
    want, exp, offered, upper = aref.graph_search_allow_ref(X, Q, gids, gcnt, seeds, k, ef, width, mask)
    sref.assert_same_answer(a, want, "restatement")
    assert sa[0] == exp and offered <= sa[1] <= upper
    tq = torch.from_numpy(Q).to(dev)
    qd = rp.Dataset.from_torch(ctx, tq)
    words = rp.allowBitmap(mask, n).view(np.int32)
    tg, tc, ts, tw = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (gids, gcnt, seeds, words))
    ids = torch.empty((nq, k), dtype=torch.int32, device=dev)
    dist = torch.empty((nq, k), dtype=torch.float64, device=dev)
    cnt = torch.empty(nq, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    rp.graphSearchAllowDev(ds, qd, kg, tg.data_ptr(), tc.data_ptr(), s, ts.data_ptr(), tw.data_ptr(), k, ef, width,
                           ids.data_ptr(), dist.data_ptr(), cnt.data_ptr())
    ctx.sync()
    sref.assert_same_answer((ids.cpu().numpy(), dist.cpu().numpy(), cnt.cpu().numpy()), a, "dev against host")
    assert rp.graphSearchLast(ctx) == sa
    rp.graphSearchAllowDev(ds, qd, kg, tg.data_ptr(), tc.data_ptr(), s, ts.data_ptr(), 0, k, ef, width,
                           ids.data_ptr(), dist.data_ptr(), cnt.data_ptr())          # no bitmap: every id
    ctx.sync()
    plain = rp.graphSearch((gids, gcnt), ds, Q, k, ef=ef, seeds=seeds)
    sref.assert_same_answer((ids.cpu().numpy(), dist.cpu().numpy(), cnt.cpu().numpy()), plain, "dev, null bitmap")


def test_seeds_from_a_forest(rp, ctx):
    n, d, kg, k = 3000, 32, 10, 10
    X = np.random.default_rng(21).standard_normal((n, d))
    ds = rp.Dataset.dense(ctx, X)
    cfg = rp.rpTreeCfg(60, n, d)
    f = rp.forestBatch(9, cfg.fpMaxTreeDepth, 60, 2, cfg.fpProjNzDensity, d, ds, ctx=ctx)
    graph = rp.graphPrepare(rp.knnGraphRefine(rp.knnGraph(kg, f), f, iters=1), f)
    rng = np.random.default_rng(8)
    Q = X[rng.choice(n, 50)] + 0.2 * rng.standard_normal((50, d))
    mask = rng.random(n) < 0.1
    got = rp.graphSearchAllow(mask, graph, f, Q, k, forest=f)                 # ef 32, width 256
    stats = rp.graphSearchLast(ctx)
    sid, _, scnt = rp.knnBatch(8, f, Q, dedup=True)
    seeds = np.where(np.arange(8)[None, :] < scnt[:, None], sid, -1).astype(np.int32)
    assert not mask[seeds[seeds >= 0]].all()                                  # seeds need not be allowed
    want, exp, offered, upper = aref.graph_search_allow_ref(X, Q, graph[0], graph[2], seeds, k, 32, 256, mask)
    sref.assert_same_answer(got, want, "forest seeds, default ef and width")
    assert stats[0] == exp and offered <= stats[1] <= upper
    assert mask[got[0][got[0] >= 0]].all()
    D = sref.query_matrix(X, Q, "l2")
    idx = np.flatnonzero(mask)
    hits = sum(len(set(got[0][i].tolist()) & set(idx[np.lexsort((idx, D[i, idx]))[:k]].tolist())) for i in range(50))
    print("recall@10 among the allowed rows: %.3f" % (hits / (50 * k)))


# ---------------------------------------------------------------- refusals, degenerate sizes
def test_refusals_leave_the_context_usable(rp, ctx):
    from rptree_amd import _lib
    L = _lib.lib()
    X, Q, per, _ = dense_case(rp, ctx, 24)
    ds, _ = per["f64"]
    nq, kg, s, k = 16, 10, 4, 10
    qd = rp.Dataset.dense(ctx, Q[:nq])
    gids, gcnt = make_graph(np.random.default_rng(10), N, kg)
    seeds0 = np.random.default_rng(3).integers(0, N, size=(nq, s)).astype(np.int32)
    mask = np.random.default_rng(4).random(N) < 0.5
    words = rp.allowBitmap(mask, N)
    good = rp.graphSearchAllow(mask, (gids, gcnt), ds, qd, k, ef=32, width=100, seeds=seeds0)
    stats = rp.graphSearchLast(ctx)
    COS, INN, REF = rp.RPT_KNN_METRIC_COSINE, rp.RPT_KNN_METRIC_INNER, rp.RPT_KNN_METRIC_REFERENCE

    def refused(data=ds, queries=qd, kg_=kg, s_=s, k_=k, ef_=32, width_=100, metric=0, flags=0, g=None):
        g = np.ascontiguousarray(gids if g is None else g, dtype=np.int32)
        ids = np.full((nq, 64), 12345, dtype=np.int32)
        dist = np.full((nq, 64), 0.5)
        cnt = np.full(nq, 77, dtype=np.int32)
        st = L.rpt_graph_search_allow_host(ctx._h, data._h, queries._h, kg_, C.c_void_p(g.ctypes.data),
                                           C.c_void_p(gcnt.ctypes.data), s_, C.c_void_p(seeds0.ctypes.data),
                                           C.c_void_p(words.ctypes.data), k_, ef_, width_, metric, flags,
                                           C.c_void_p(ids.ctypes.data), C.c_void_p(dist.ctypes.data),
                                           C.c_void_p(cnt.ctypes.data))
        assert st == RPT_E_ARG, st
        msg = L.rpt_last_error().decode()
        assert len(msg) > 8, msg
        assert np.all(ids == 12345) and np.all(dist == 0.5) and np.all(cnt == 77)   # nothing was written
        assert rp.graphSearchLast(ctx) == stats            # nothing was launched
        return msg

    for w in (31, 0, -1, 1025):
        assert "width" in refused(width_=w)
    assert "ef" in refused(ef_=257, width_=300)
    assert "ef" in refused(ef_=9)
    assert "k" in refused(k_=65, ef_=100)
    assert "kg" in refused(kg_=65) and "s " in refused(s_=65)
    for m in (COS | INN, REF, 2, -1):
        assert "metric" in refused(metric=m)
    for fl in (1, COS, REF):
        assert "flags" in refused(flags=fl)
    csr = rp.Dataset.csr(ctx, *gm.make_csr(3, N, 24, 0.3))
    qcsr = rp.Dataset.csr(ctx, *gm.make_csr(4, nq, 24, 0.3))
    assert "both" in refused(queries=qcsr) and "both" in refused(data=csr)
    bad = np.array(gids)
    bad[401, 0] = N
    assert gcnt[401] > 0 and "graph row 401" in refused(g=bad)                # before any upload
    with pytest.raises(ValueError):
        rp.graphSearchAllow(mask, (gids, gcnt), ds, qd, k)                   # neither seeds nor a forest
    with pytest.raises(ValueError):
        rp.graphSearchAllow(mask[:-1], (gids, gcnt), ds, qd, k, seeds=seeds0)
    again = rp.graphSearchAllow(words, (gids, gcnt), ds, qd, k, ef=32, width=100, seeds=seeds0)
    sref.assert_same_answer(again, good, "after the refusals")
    assert rp.graphSearchLast(ctx) == stats
    # the CSR pair itself is served
    both = rp.graphSearchAllow(mask, (gids, gcnt), csr, qcsr, k, ef=32, width=100, seeds=seeds0)
    assert mask[both[0][both[0] >= 0]].all()


def test_no_queries_no_points_and_one_point(rp, ctx):
    d = 8
    X = np.random.default_rng(1).standard_normal((50, d))
    ds = rp.Dataset.dense(ctx, X)
    gids = np.array([[(i + 1 + e) % 50 for e in range(3)] for i in range(50)], dtype=np.int32)
    graph = (gids, np.full(50, 3, dtype=np.int32))
    mask = np.arange(50) % 2 == 0
    ids, dist, cnt = rp.graphSearchAllow(mask, graph, ds, np.zeros((0, d)), 5, seeds=np.zeros((0, 2), dtype=np.int32))
    assert ids.shape == (0, 5) and dist.shape == (0, 5) and cnt.shape == (0,)
    assert rp.graphSearchLast(ctx) == (0, 0)
    Q = X[:4] + 0.01
    got = rp.graphSearchAllow(mask, graph, ds, Q, 5, seeds=np.full((4, 3), -1, dtype=np.int32))    # every seed -1
    assert np.all(got[2] == 0) and np.all(got[0] == -1) and np.all(np.isposinf(got[1]))
    # n = 1, allowed and not
    one = rp.Dataset.dense(ctx, X[:1])
    g1 = (np.full((1, 2), -1, dtype=np.int32), np.zeros(1, dtype=np.int32))
    seeds = np.array([[0], [-1], [0], [0]], dtype=np.int32)
    for m1, counts in ((np.array([True]), [1, 0, 1, 1]), (np.array([False]), [0, 0, 0, 0]), (None, [1, 0, 1, 1])):
        got = rp.graphSearchAllow(m1, g1, one, Q, 3, ef=3, width=3, seeds=seeds)
        want = aref.graph_search_allow_ref(X[:1], Q, g1[0], g1[1], seeds, 3, 3, 3, m1)
        sref.assert_same_answer(got, want[0], "n = 1")
        assert got[2].tolist() == counts and rp.graphSearchLast(ctx) == (3, 3)
    # n = 0: every count is 0, with an empty bitmap and with none
    none = rp.Dataset.dense(ctx, np.zeros((0, d)))
    g0 = (np.zeros((0, 2), dtype=np.int32), np.zeros(0, dtype=np.int32))
    for m0 in (np.zeros(0, dtype=bool), None):
        got = rp.graphSearchAllow(m0, g0, none, Q, 3, seeds=np.full((4, 2), -1, dtype=np.int32))
        assert np.all(got[2] == 0) and np.all(got[0] == -1)


@pytest.mark.parametrize("n", [33, 64])
def test_bits_beyond_n_are_ignored(rp, ctx, n):
    rng = np.random.default_rng(n)
    X = rng.integers(-2, 3, size=(n, 6)).astype(np.float64)
    Q = X[:8] + 0.5
    ds = rp.Dataset.dense(ctx, X)
    gids, gcnt = make_graph(rng, n, 4)
    seeds = rng.integers(0, n, size=(8, 2)).astype(np.int32)
    mask = rng.random(n) < 0.5
    words = rp.allowBitmap(mask, n)
    dirty = words.copy()
    if n % 32:
        dirty[-1] |= np.uint32((0xffffffff << (n % 32)) & 0xffffffff)
    a = rp.graphSearchAllow(words, (gids, gcnt), ds, Q, 5, ef=6, width=20, seeds=seeds)
    b = rp.graphSearchAllow(dirty, (gids, gcnt), ds, Q, 5, ef=6, width=20, seeds=seeds)
    sref.assert_same_answer(a, b, "dirty tail")
    want = aref.graph_search_allow_ref(X, Q, gids, gcnt, seeds, 5, 6, 20, mask)
    sref.assert_same_answer(a, want[0], "restatement")


# ---------------------------------------------------------------- CSR values that store an inf or a NaN
@pytest.mark.parametrize("metric", METRICS)
def test_stored_inf_and_nan_follow_dots(rp, ctx, metric):
    """a stored inf or NaN meets only what the other row stores: the answer is dotS's, the one of
    graphSearchMetricSV, with and without an allow-list"""
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
    gids, gcnt = make_graph(rng, n, kg)
    gids[:, 0] = rng.choice([30, 31, 32], size=n)          # every row leads to the awkward ones
    seeds = rng.integers(0, n, size=(nq, 4)).astype(np.int32)
    ds = rp.Dataset.csr(ctx, *csrX)
    D = csr_distances(csrX, csrQ, metric)
    twin = rp.graphSearchMetricSV(distf(rp, metric), (gids, gcnt), ds, csrQ, 10, ef=24, seeds=seeds)
    got = rp.graphSearchAllow(None, (gids, gcnt), ds, csrQ, 10, ef=24, width=24, seeds=seeds, metric=distf(rp, metric))
    sref.assert_same_answer(got, twin, "every id, " + metric)
    mask = rng.random(n) < 0.4
    mask[[30, 31, 32]] = True
    got = rp.graphSearchAllow(mask, (gids, gcnt), ds, csrQ, 10, ef=24, width=90, seeds=seeds, metric=distf(rp, metric))
    stats = rp.graphSearchLast(ctx)
    want, exp, offered, upper = aref.graph_search_allow_ref(np.zeros((n, 1)), np.zeros((nq, 1)), gids, gcnt, seeds, 10,
                                                            24, 90, mask, metric, D=D)
    sref.assert_same_answer(got, want, "allow-list, " + metric)
    assert stats[0] == exp and offered <= stats[1] <= upper


# ---------------------------------------------------------------- the C++ mirror
def test_cpp_example(tmp_path):
    """host/example_graph_search_allow.cpp: a tombstone bitmap over a graph built once; no deleted row is
    answered, every distance is the row's, nothing deleted gives graphSearch's bits"""
    exe = str(tmp_path / "example_graph_search_allow")
    src = os.path.join(ROOT, "rp-tree_amd", "host", "example_graph_search_allow.cpp")
    lib = os.path.join(ROOT, "rp-tree_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, src, "-L" + lib, "-lrptree_hip",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    rng = np.random.default_rng(12)
    n, nq, d = 2000, 40, 16
    X = rng.standard_normal((n, d))
    Q = X[rng.choice(n, nq)] + 0.1 * rng.standard_normal((nq, d))
    for name, a in (("data.bin", X), ("queries.bin", Q)):
        with open(tmp_path / name, "wb") as fh:
            fh.write(np.array(a.shape, dtype=np.int64).tobytes())
            fh.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, str(tmp_path / "data.bin"), str(tmp_path / "queries.bin"), "4", "40", "10", "10", "32",
                        "128", "3"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok" and lines[0] == "deleted 667 of 2000 rows"
    assert any(ln.startswith("recall@10") for ln in lines)
    print(r.stdout)
