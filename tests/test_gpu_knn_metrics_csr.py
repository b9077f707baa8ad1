"""Cosine and inner-product kNN on SVector (CSR) rows on the device: rpt_brute_knn_csr_metric_*,
rpt_knn_csr_metric_*, rpt_recall_hits_csr_metric_host and the Python routes to them against the numpy
restatement tests/knn_metric_csr_ref.py — ids and distance BITS, both metrics, f64 and f32 values."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import knn_metric_csr_ref as ref

pytestmark = pytest.mark.gpu

RPT_E_ARG, RPT_E_UNSUPPORTED = -1, -4
METRICS = [ref.INNER, ref.COSINE]
DTYPES = [np.float64, np.float32]


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
    return rp.metricInner if metric == ref.INNER else rp.metricCosine


def flag(rp, metric):
    return rp.RPT_KNN_METRIC_INNER if metric == ref.INNER else rp.RPT_KNN_METRIC_COSINE


def same_bits(a, b):
    """equal as bit patterns, any NaN equal to any NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def last_candidates(ctx):
    from rptree_amd import _lib
    v = C.c_int64()
    _lib.check(_lib.lib().rpt_knn_last_candidates(ctx._h, C.byref(v)))
    return int(v.value)


def knn_restated(rp, metric, f, data, queries, d, k, dedup):
    """the restatement over candidatesBatch's ids -> (ids, dist, count, candidates in all)"""
    X, P = ref.dense(*data, d)
    Q, QP = ref.dense(*queries, d)
    Xd = (X, P, ref.self_dots(X, P))
    off, cand = rp.candidatesBatch(f, queries + (d,))
    nq, T = Q.shape[0], f.T
    ids = np.empty((nq, k), dtype=np.int32)
    dist = np.empty((nq, k))
    cnt = np.empty(nq, dtype=np.int32)
    for i in range(nq):
        ids[i], dist[i], cnt[i] = ref.knn_candidates(metric, Xd, cand[off[i * T]:off[(i + 1) * T]], Q[i], QP[i],
                                                     k, dedup)
    return ids, dist, cnt, len(cand)


# ------------------------------------------------------------------ A. brute force
@pytest.fixture(scope="module", params=DTYPES, ids=["f64", "f32"])
def fixture_a(request):
    data, queries, d = ref.fixture_a(request.param)
    want = {(m, k): ref.brute(m, data, queries, d, k) for m in METRICS for k in (1, 10, 200)}
    return data, queries, d, want


@pytest.mark.parametrize("metric", METRICS)
def test_brute_force_is_the_definition(rp, ctx, fixture_a, metric):
    """9 000 x 70 rows, 13 queries (stored rows, an empty query, an empty row, duplicates, a full row, a
    short last row): the restatement's ids and bits for every k and brute_csr_tile, the dense entry
    point's on the dense-ified data, at most nq / 4 uncertified queries, and the same bits from the
    exact kernel alone"""
    data, queries, d, want = fixture_a
    ds = rp.Dataset.csr(ctx, *data, d)
    qs = queries + (d,)
    nq = len(queries[0]) - 1
    Xdense = ref.dense(*data, d)[0].astype(data[2].dtype)
    Qdense = ref.dense(*queries, d)[0].astype(data[2].dtype)
    dd = rp.Dataset.dense(ctx, Xdense)
    for k in (1, 10, 200):
        wi, wd = want[(metric, k)]
        for tile in (0, 1, 2, 8):
            with option(ctx, "brute_csr_tile", tile):
                gi, gd = rp.bruteKnn(ds, qs, k, metric=distf(rp, metric))
            unc = rp.knn_last_uncertified(ctx)
            assert np.array_equal(gi, wi), (k, tile)
            assert same_bits(gd, wd), (k, tile)
            assert unc <= nq / 4, (k, tile, unc)
        di, dv = rp.bruteKnn(dd, Qdense, k, metric=distf(rp, metric))
        assert np.array_equal(di, wi) and same_bits(dv, wd), k
        with option(ctx, "knn_metric_exact", 1):
            gi, gd = rp.bruteKnn(ds, qs, k, metric=distf(rp, metric))
            assert rp.knn_last_uncertified(ctx) == nq
        assert np.array_equal(gi, wi) and same_bits(gd, wd), k


@pytest.mark.parametrize("metric", METRICS)
def test_brute_force_where_the_tile_does_not_fit(rp, ctx, metric):
    """d = 11 000: with k = 1024 one query's tile does not fit the LDS budget next to the finalize
    arrays and the exhaustive search runs the forest kernels in identity mode; with k = 10 it is the
    tiled stream.  Both are the definition; k = 1024 of 1 100 rows ranks nearly every row."""
    rng = np.random.default_rng(77)
    n, d, nq = 1100, 11000, 3
    data = ref.random_csr(rng, n, d, 0.004)
    queries = ref.random_csr(rng, nq, d, 0.02)
    ds = rp.Dataset.csr(ctx, *data, d)
    for k in (10, 1024):
        wi, wd = ref.brute(metric, data, queries, d, k)
        gi, gd = rp.bruteKnn(ds, queries + (d,), k, metric=distf(rp, metric))
        assert np.array_equal(gi, wi) and same_bits(gd, wd), k


def test_cpp_sparse_metric_example(tmp_path):
    """host/example_sparse_metric.cpp: the C++ Metric overloads on SVector data against its own host fold"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "example_sparse_metric")
    src = os.path.join(root, "rp-tree_amd", "host", "example_sparse_metric.cpp")
    lib = os.path.join(root, "rp-tree_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, src, "-L" + lib,
                           "-lrptree_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, "3000", "40", "0.25", "4", "30", "12"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok" and len([x for x in lines if " recall " in x]) == 4


# ------------------------------------------------------------------ B. ties wider than the margin
def lattice(dtype):
    rng = np.random.default_rng(33)
    n, d = 3000, 24
    mask = rng.random((n + 12, d)) < 0.15
    vals = rng.integers(-2, 3, (n + 12, d)).astype(dtype)
    rowptr = np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.int64)
    col, val = np.nonzero(mask)[1].astype(np.int32), vals[mask]
    e = rowptr[n]
    return (rowptr[:n + 1], col[:e], val[:e]), (rowptr[n:] - e, col[e:], val[e:]), d


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("metric", METRICS)
def test_ties_wider_than_the_margin(rp, ctx, metric, dtype):
    """lattice rows: the dots are small integers, most of them 0 — the cut falls inside a run of equal
    values longer than the margin, the exact kernel answers"""
    data, queries, d = lattice(dtype)
    k = 10
    f = rp.forestBatch(7, 5, 40, 3, 0.5, d, data + (d,), ctx=ctx)
    qs = queries + (d,)
    wi, wd = ref.brute(metric, data, queries, d, k)
    gi, gd = rp.bruteKnn(f, qs, k, metric=distf(rp, metric))
    assert rp.knn_last_uncertified(ctx) > 0
    assert np.array_equal(gi, wi) and same_bits(gd, wd)
    total_unc = 0
    for dedup in (0, 1, rp.RPT_KNN_DEDUP_DISTANCE):
        wi, wd, wc, _ = knn_restated(rp, metric, f, data, queries, d, k, dedup)
        gi, gd, gc = rp.knnBatch(k, f, qs, dedup=dedup, metric=distf(rp, metric))
        total_unc += rp.knn_last_uncertified(ctx)
        assert np.array_equal(gc, wc), dedup
        assert np.array_equal(gi, wi) and same_bits(gd, wd), dedup
    assert total_unc > 0
    f.close()


# ------------------------------------------------------------------ C. non-finite values
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("metric", METRICS)
def test_stored_inf_and_nan(rp, ctx, metric, dtype):
    """an inf and a NaN stored in a row and in a query: a column counts only where both rows store
    it (the restatement alone is the truth here: the dense-ified fold meets inf * 0)"""
    rng = np.random.default_rng(44)
    n, d, nq = 200, 30, 6
    rowptr, col, val = ref.random_csr(rng, n, d, 0.3, dtype)
    qr, qc, qv = ref.random_csr(rng, nq, d, 0.3, dtype)
    val[rowptr[5]] = np.inf
    val[rowptr[9] + 1] = np.nan
    qv[qr[1]] = np.nan
    qv[qr[2] + 1] = -np.inf
    data, queries = (rowptr, col, val), (qr, qc, qv)
    ds = rp.Dataset.csr(ctx, *data, d)
    for k in (5, 200):                       # k = 200 = n: nothing is left out, every row is ranked
        wi, wd = ref.brute(metric, data, queries, d, k)
        gi, gd = rp.bruteKnn(ds, queries + (d,), k, metric=distf(rp, metric))
        assert np.array_equal(gi, wi) and same_bits(gd, wd), k
    f = rp.forestBatch(3, 2, 30, 2, 0.5, d, data + (d,), ctx=ctx)
    for dedup in (0, 1, rp.RPT_KNN_DEDUP_DISTANCE):
        wi, wd, wc, _ = knn_restated(rp, metric, f, data, queries, d, 5, dedup)
        gi, gd, gc = rp.knnBatch(5, f, queries + (d,), dedup=dedup, metric=distf(rp, metric))
        assert np.array_equal(gc, wc) and np.array_equal(gi, wi) and same_bits(gd, wd), dedup
    f.close()


# ------------------------------------------------------------------ D. forest query
@pytest.fixture(scope="module", params=DTYPES, ids=["f64", "f32"])
def fixture_d(request):
    rng = np.random.default_rng(55)
    n, d, nq = 3000, 64, 40
    data = ref.random_csr(rng, n, d, 0.2, request.param)
    fresh = ref.random_csr(rng, nq, d, 0.2, request.param)
    # the first 12 queries are stored rows
    lens = np.diff(fresh[0])
    lens[:12] = np.diff(data[0])[:12]
    parts_c, parts_v = [], []
    for i in range(nq):
        src, r = (data, i) if i < 12 else (fresh, i)
        parts_c.append(src[1][src[0][r]:src[0][r + 1]])
        parts_v.append(src[2][src[0][r]:src[0][r + 1]])
    queries = (np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), np.concatenate(parts_c),
               np.concatenate(parts_v))
    return data, queries, d


@pytest.mark.parametrize("streamed", [False, True], ids=["batch", "streamed"])
@pytest.mark.parametrize("metric", METRICS)
def test_forest_query_is_the_definition_over_the_candidates(rp, ctx, fixture_d, metric, streamed):
    data, queries, d = fixture_d
    n, T, ml = len(data[0]) - 1, 4, 30
    cfg = rp.rpTreeCfg(ml, n, d)
    if streamed:
        f = rp.forest(9, cfg.fpMaxTreeDepth, ml, T, 700, cfg.fpProjNzDensity, d, data + (d,), ctx=ctx)
    else:
        f = rp.forestBatch(9, cfg.fpMaxTreeDepth, ml, T, cfg.fpProjNzDensity, d, data + (d,), ctx=ctx)
    qs = queries + (d,)
    for k in (10, 200):
        for dedup in (0, 1, rp.RPT_KNN_DEDUP_DISTANCE):
            wi, wd, wc, ncand = knn_restated(rp, metric, f, data, queries, d, k, dedup)
            gi, gd, gc = rp.knnBatch(k, f, qs, dedup=dedup, metric=distf(rp, metric))
            assert last_candidates(ctx) == ncand
            assert np.array_equal(gc, wc), (k, dedup)
            assert np.array_equal(gi, wi) and same_bits(gd, wd), (k, dedup)
    # knn / knnPQ: the one-query forms
    q0 = rp.SVector(d, queries[1][:queries[0][1]], queries[2][:queries[0][1]])
    wi, wd, wc, _ = knn_restated(rp, metric, f, data, queries, d, 10, 0)
    got = rp.knn(distf(rp, metric), 10, f, q0)
    assert [i for _, i in got] == wi[0, :wc[0]].tolist() and same_bits([v for v, _ in got], wd[0, :wc[0]])
    wi, wd, wc, _ = knn_restated(rp, metric, f, data, queries, d, 10, 2)
    got = rp.knnPQ(distf(rp, metric), 10, f, q0)
    assert [i for _, i in got] == wi[0, :wc[0]].tolist() and same_bits([v for v, _ in got], wd[0, :wc[0]])
    f.close()


# ------------------------------------------------------------------ E. recall
@pytest.mark.parametrize("metric", METRICS)
def test_recall_hits(rp, ctx, fixture_d, metric):
    data, queries, d = fixture_d
    n, T, ml, k = len(data[0]) - 1, 4, 30, 12
    cfg = rp.rpTreeCfg(ml, n, d)
    f = rp.forestBatch(9, cfg.fpMaxTreeDepth, ml, T, cfg.fpProjNzDensity, d, data + (d,), ctx=ctx)
    qs = queries + (d,)
    nq = len(queries[0]) - 1
    hits, truth = rp.recallHits(distf(rp, metric), f, k, qs)
    bi, _ = rp.bruteKnn(f, qs, k, metric=distf(rp, metric))
    assert np.array_equal(truth, bi)
    assert np.array_equal(bi, ref.brute(metric, data, queries, d, k)[0])
    off, cand = rp.candidatesBatch(f, qs)
    want = np.array([[len(set(cand[off[i * T + t]:off[i * T + t + 1]].tolist()) & set(truth[i].tolist()))
                      for t in range(T)] for i in range(nq)], dtype=np.int32)
    assert np.array_equal(hits, want) and hits.sum() > 0
    rec = rp.recallWithBatch(distf(rp, metric), f, k, qs)
    for i in (0, 13, nq - 1):
        a, b = queries[0][i], queries[0][i + 1]
        r1 = rp.recallWith(distf(rp, metric), f, k, rp.SVector(d, queries[1][a:b], queries[2][a:b]))
        assert r1 == rec[i] == sum(int(h) / k for h in hits[i]) / T
    with pytest.raises(ValueError):
        rp.recallHits(distf(rp, metric), f, k, qs, reference_metric=True)
    with pytest.raises(ValueError):
        rp.knnBatch(k, f, qs, metric=distf(rp, metric), reference_metric=True)
    with pytest.raises(rp.RPTError):
        rp.knnBatch(k, f, qs, metric=distf(rp, metric), vote=2)
    f.close()


# ------------------------------------------------------------------ F. device and host entry points
@pytest.mark.parametrize("metric", METRICS)
def test_dev_entry_points_match_host(rp, ctx, fixture_d, metric):
    import torch
    from rptree_amd import _lib
    L = _lib.lib()
    data, queries, d = fixture_d
    n, T, ml, k = len(data[0]) - 1, 4, 30, 7
    nq = len(queries[0]) - 1
    cfg = rp.rpTreeCfg(ml, n, d)
    f = rp.forestBatch(9, cfg.fpMaxTreeDepth, ml, T, cfg.fpProjNzDensity, d, data + (d,), ctx=ctx)
    qd, _ = rp._query_dataset(ctx, f.data, queries + (d,))
    fl = flag(rp, metric)

    def buffers():
        ti = torch.full((nq, k), -7, dtype=torch.int32, device="cuda")
        td = torch.full((nq, k), -3.0, dtype=torch.float64, device="cuda")
        tc = torch.full((nq,), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        return ti, td, tc

    wi, wd = rp.bruteKnn(f, qd, k, metric=distf(rp, metric))
    ti, td, _ = buffers()
    st = L.rpt_brute_knn_csr_metric_dev(ctx._h, f.data._h, qd._h, k, fl, C.c_void_p(ti.data_ptr()),
                                        C.c_void_p(td.data_ptr()))
    assert st == 0, L.rpt_last_error()
    ctx.sync()
    assert np.array_equal(ti.cpu().numpy(), wi) and same_bits(td.cpu().numpy(), wd)
    for dedup in (0, 1, 2):
        wi, wd, wc = rp.knnBatch(k, f, qd, dedup=dedup, metric=distf(rp, metric))
        ti, td, tc = buffers()
        st = L.rpt_knn_csr_metric_dev(ctx._h, f._h, f.data._h, qd._h, k, fl | dedup, C.c_void_p(ti.data_ptr()),
                                      C.c_void_p(td.data_ptr()), C.c_void_p(tc.data_ptr()))
        assert st == 0, L.rpt_last_error()
        ctx.sync()
        assert np.array_equal(tc.cpu().numpy(), wc), dedup
        assert np.array_equal(ti.cpu().numpy(), wi) and same_bits(td.cpu().numpy(), wd), dedup
    f.close()


# ------------------------------------------------------------------ G. refusals
def test_refusals_leave_the_context_usable(rp, ctx):
    from rptree_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(66)
    n, d, k, nq = 500, 30, 5, 4
    data = ref.random_csr(rng, n, d, 0.3)
    queries = ref.random_csr(rng, nq, d, 0.3)
    f = rp.forestBatch(4, 4, 30, 2, 0.5, d, data + (d,), ctx=ctx)
    ds = f.data
    qc, _ = rp._query_dataset(ctx, ds, queries + (d,))
    q32 = rp.Dataset.csr(ctx, queries[0], queries[1], queries[2].astype(np.float32), d)
    Xd = ref.dense(*data, d)[0]
    dd, qdn = rp.Dataset.dense(ctx, Xd), rp.Dataset.dense(ctx, ref.dense(*queries, d)[0])
    ids = np.empty((nq, k), dtype=np.int32)
    dist = np.empty((nq, k), dtype=np.float64)
    cnt = np.empty(nq, dtype=np.int32)
    hits = np.empty((nq, 2), dtype=np.int32)
    pi, pd, pc, ph = (C.c_void_p(a.ctypes.data) for a in (ids, dist, cnt, hits))
    cos, inn, refm = rp.RPT_KNN_METRIC_COSINE, rp.RPT_KNN_METRIC_INNER, rp.RPT_KNN_METRIC_REFERENCE
    before = rp.knnBatch(k, f, qc)

    def message():
        return L.rpt_last_error().decode()

    def knn(data_, q_, flags):
        return L.rpt_knn_csr_metric_host(ctx._h, f._h, data_._h, q_._h, k, flags, pi, pd, pc)

    def brute(data_, q_, flags):
        return L.rpt_brute_knn_csr_metric_host(ctx._h, data_._h, q_._h, k, flags, pi, pd)

    def recall(data_, q_, flags):
        return L.rpt_recall_hits_csr_metric_host(ctx._h, f._h, data_._h, q_._h, k, flags, ph, None)

    def usable():
        after = rp.knnBatch(k, f, qc)
        assert all(np.array_equal(a, b) for a, b in zip(before, after))

    for flags in (0, 1, cos | inn):                     # neither metric bit, or both
        assert knn(ds, qc, flags) == RPT_E_ARG and "rpt_knn_*" in message()
        usable()
    for flags in (0, cos | inn):
        assert brute(ds, qc, flags) == RPT_E_ARG and "rpt_brute_knn_*" in message()
        assert recall(ds, qc, flags) == RPT_E_ARG and message()
        usable()
    for data_, q_ in ((dd, qdn), (dd, qc), (ds, qdn)):  # dense data, or a dense / CSR mix
        assert knn(data_, q_, cos) == RPT_E_ARG and "rpt_knn_*" in message()
        assert brute(data_, q_, inn) == RPT_E_ARG and "rpt_brute_knn_metric_*" in message()
        assert recall(data_, q_, inn) == RPT_E_ARG and message()
        usable()
    for m in (cos, inn):
        assert knn(ds, qc, m | refm) == RPT_E_ARG and message()
        assert brute(ds, qc, m | refm) == RPT_E_ARG and message()
        assert recall(ds, qc, m | refm) == RPT_E_ARG and message()
        assert knn(ds, qc, m | (2 << 8)) == RPT_E_UNSUPPORTED and "VOTE" in message()
        assert knn(ds, q32, m) == RPT_E_ARG and message()        # dtype mismatch
        assert brute(ds, q32, m) == RPT_E_ARG and message()
        assert brute(ds, qc, m | 1) == RPT_E_ARG and message()   # the brute force has no duplicate rule
        usable()
    # a projection-type mismatch against the forest: f32 rows under a forest of f64 projections
    d32 = rp.Dataset.csr(ctx, data[0], data[1], data[2].astype(np.float32), d)
    assert knn(d32, q32, cos) == RPT_E_ARG and "projection type" in message()
    usable()
    for kk in (0, 1025):
        assert L.rpt_brute_knn_csr_metric_host(ctx._h, ds._h, qc._h, kk, cos, pi, pd) == RPT_E_ARG
        assert "k must be" in message()
    # the existing entry points keep refusing
    assert L.rpt_knn_host(ctx._h, f._h, ds._h, qc._h, k, cos, pi, pd, pc) == RPT_E_UNSUPPORTED
    assert L.rpt_brute_knn_metric_host(ctx._h, ds._h, qc._h, k, cos, pi, pd) == RPT_E_UNSUPPORTED
    usable()
    # and a good call right after: served, with the statistics
    assert knn(ds, qc, cos | 1) == 0, message()
    tier, retries = C.c_int32(-1), C.c_int64(-1)
    assert L.rpt_knn_last_tier(ctx._h, C.byref(tier)) == 0 and tier.value == 0
    assert L.rpt_knn_last_retries(ctx._h, C.byref(retries)) == 0 and retries.value == 0
    f.close()
