"""Exhaustive kNN over SVector (CSR) rows on the device (rpt_brute_knn_host / _metric_host / _dev on
CSR handles: the query-tiled brute_csr_kernel) and the batched recallWith built on it
(rpt_recall_hits_host, recallWithBatch).

Truth of the true-L2 legs: numpy on the dense-ified rows, sqrt(sum((x - q)**2)); f32 values are
widened first.  Tolerance rtol = 1e-9, atol = 1e-12, the one the CSR kNN tests use.  Ids are compared
at every position whose truth distance is separated from both neighbours by more than 1e-9
relative; at most 1 % of the (query, position) pairs may be left out by that rule.
Truth of the reference-metric leg: oracle.metric_ss (the pinned truncating metricSSL2) over all
rows, selected by (distance, id), bit for bit."""
import contextlib
import os
import struct
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, ATOL = 1e-9, 1e-12
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


# ------------------------------------------------------------------ CSR helpers
def densify(rowptr, col, val, d):
    n = len(rowptr) - 1
    X = np.zeros((n, d), dtype=np.float64)
    X[np.repeat(np.arange(n), np.diff(rowptr)), col] = np.asarray(val).astype(np.float64)
    return X


def take_rows(rowptr, col, val, rows):
    """the CSR of the listed rows of a CSR (a row may be listed more than once)"""
    lens = np.array([rowptr[r + 1] - rowptr[r] for r in rows], dtype=np.int64)
    rp_ = np.zeros(len(rows) + 1, dtype=np.int64)
    rp_[1:] = np.cumsum(lens)
    idx = (np.concatenate([np.arange(rowptr[r], rowptr[r + 1]) for r in rows])
           if len(rows) else np.zeros(0, dtype=np.int64)).astype(np.int64)
    return rp_, col[idx], val[idx]


def stack(a, b):
    return (np.concatenate([a[0], b[0][1:] + a[0][-1]]), np.concatenate([a[1], b[1]]),
            np.concatenate([a[2], b[2]]))


def queries_with_stored_rows(oracle, data, d, density, nq, seed, stored=8):
    """nq queries: the first `stored` are rows 0 .. stored-1 of the data, the rest fresh rows"""
    fresh = oracle.data_normal_sparse2(seed, nq, d, density)
    return stack(take_rows(*data, list(range(stored))), take_rows(*fresh, list(range(stored, nq))))


def true_distances(X, Q):
    return np.stack([np.sqrt(((X - q[None, :]) ** 2).sum(axis=1)) for q in Q])


def check_l2(ids, dist, D, k, tag):
    """the assertions of the true-L2 legs for one answer; -> (pairs left out, pairs)"""
    nq, n = D.shape
    m = min(k, n)
    left = 0
    for i in range(nq):
        order = np.lexsort((np.arange(n), D[i]))
        td = D[i][order[:m + 1]]
        gi, gd = ids[i, :m], dist[i, :m]
        assert np.all(ids[i, m:] == -1) and np.all(np.isposinf(dist[i, m:])), (tag, i)
        assert np.allclose(gd, td[:m], rtol=RTOL, atol=ATOL), (tag, i, np.abs(gd - td[:m]).max())
        # always
        assert np.all(np.diff(gd) >= 0), (tag, i)
        assert np.all(gi >= 0) and np.all(gi < n) and len(set(gi.tolist())) == m, (tag, i)
        eq = gd[1:] == gd[:-1]
        assert np.all(gi[1:][eq] > gi[:-1][eq]), (tag, i)
        outside = np.ones(n, dtype=bool)
        outside[gi] = False
        if outside.any():
            nearest = D[i][outside].min()
            assert nearest >= gd[-1] - (RTOL * max(nearest, gd[-1]) + ATOL), (tag, i)
        # ids where the truth is separated from both neighbours
        gap = np.diff(td) > 1e-9 * td[1:]                # gap[p]: td[p] < td[p + 1], separated
        right = np.ones(m, dtype=bool)
        right[:len(gap)] = gap[:m]
        leftn = np.ones(m, dtype=bool)
        leftn[1:] = gap[:m - 1]
        sep = right & leftn
        assert np.array_equal(gi[sep], order[:m][sep]), (tag, i)
        left += int((~sep).sum())
    return left, nq * m


# ------------------------------------------------------------------ 1. true L2 against numpy
@pytest.mark.parametrize("n,d,density", [(20000, 200, 0.2), (3000, 30, 0.3)])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_brute_csr_true_l2_matches_numpy(rp, ctx, oracle, n, d, density, dtype):
    rowptr, col, val = oracle.data_normal_sparse2(5, n, d, density)
    val = val.astype(dtype)
    data = (rowptr, col, val)
    qr, qc, qv = queries_with_stored_rows(oracle, data, d, density, 64, 6)
    qv = qv.astype(dtype)
    X, Q = densify(rowptr, col, val, d), densify(qr, qc, qv, d)
    D = true_distances(X, Q)
    ds = rp.Dataset.csr(ctx, rowptr, col, val, d)
    for k in (1, 10, 25, 200):
        ids, dist = rp.bruteKnn(ds, (qr, qc, qv, d), k)
        left, pairs = check_l2(ids, dist, D, k, (n, d, dtype.__name__, k))
        print("n=%d d=%d %s k=%d: %d of %d pairs left out" % (n, d, dtype.__name__, k, left, pairs))
        assert left <= 0.01 * pairs
        assert np.all(dist[:8, 0] == 0.0) and np.array_equal(ids[:8, 0], np.arange(8))  # stored rows


# ------------------------------------------------------------------ 2. planted exact ties
def test_brute_csr_planted_ties(rp, ctx, oracle):
    n, d, density = 3000, 30, 0.3
    rowptr, col, val = oracle.data_normal_sparse2(5, n, d, density)
    rng = np.random.default_rng(3)
    pick = 4 + rng.permutation(n - 4)[:80]
    src, dst = pick[:40], pick[40:]
    src[:4] = [0, 1, 2, 3]                              # copies of rows that are queries too
    rows = np.arange(n)
    rows[dst] = src
    body = take_rows(rowptr, col, val, rows.tolist())
    empty = (np.zeros(6, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0))
    rowptr, col, val = stack(body, empty)               # + 5 empty rows
    n += 5
    q = queries_with_stored_rows(oracle, (rowptr, col, val), d, density, 63, 6)
    qr, qc, qv = stack(q, (np.zeros(2, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0)))
    X, Q = densify(rowptr, col, val, d), densify(qr, qc, qv, d)
    D = true_distances(X, Q)
    ds = rp.Dataset.csr(ctx, rowptr, col, val, d)
    for k in (1, 5, 10, 25, 200):
        ids, dist = rp.bruteKnn(ds, (qr, qc, qv, d), k)
        check_l2(ids, dist, D, k, ("ties", k))
        for i in range(64):
            eq = dist[i, 1:] == dist[i, :-1]
            assert np.all(ids[i, 1:][eq] > ids[i, :-1][eq]), (k, i)
            order = np.lexsort((np.arange(n), D[i]))
            if D[i][order[k]] - D[i][order[k - 1]] > 1e-9 * D[i][order[k]]:
                assert set(ids[i].tolist()) == set(order[:k].tolist()), (k, i)
    # a copied row and its source are at bit-equal distances from every query: ascending ids
    ids, dist = rp.bruteKnn(ds, (qr, qc, qv, d), 200)
    pairs = 0
    for i in range(64):
        pos = {int(v): p for p, v in enumerate(ids[i])}
        for s, t in zip(src.tolist(), dst.tolist()):
            if s in pos and t in pos:
                assert dist[i, pos[s]] == dist[i, pos[t]], (i, s, t)
                assert (pos[s] < pos[t]) == (s < t), (i, s, t)
                pairs += 1
    assert pairs >= 40
    # the empty query: distance = |x|, the five empty rows first (distance 0, ascending id)
    assert np.array_equal(ids[63, :5], np.arange(n - 5, n)) and np.all(dist[63, :5] == 0.0)


# ------------------------------------------------------------------ 3. reference metric, bit-exact
def reference_truth(oracle, rowptr, col, val, qc, qv, k):
    n = len(rowptr) - 1
    v = np.array([oracle.metric_ss(col[rowptr[r]:rowptr[r + 1]], val[rowptr[r]:rowptr[r + 1]], qc, qv)
                  for r in range(n)])
    order = np.lexsort((np.arange(n), v))[:k]
    return order.astype(np.int32), v[order]


def test_brute_csr_reference_metric_is_bit_identical(rp, ctx, oracle):
    n, d = 3000, 30
    rowptr, col, val = oracle.data_normal_sparse2(5, n, d, 0.3)
    qr, qc, qv = oracle.data_normal_sparse2(6, 8, d, 0.3)
    ds = rp.Dataset.csr(ctx, rowptr, col, val, d)
    differs = 0
    for k in (1, 7, 50):
        ids, dist = rp.bruteKnn(ds, (qr, qc, qv, d), k, reference_metric=True)
        t_ids, t_dist = rp.bruteKnn(ds, (qr, qc, qv, d), k)
        for i in range(8):
            a, b = qr[i], qr[i + 1]
            wi, wd = reference_truth(oracle, rowptr, col, val, qc[a:b], qv[a:b], k)
            assert np.array_equal(ids[i], wi), (k, i)
            assert np.array_equal(dist[i].view(np.uint64), wd.view(np.uint64)), (k, i)
            differs += int(not np.array_equal(t_dist[i], dist[i]))
    assert differs >= 1                     # the truncated tails matter on this data


# ------------------------------------------------------------------ 4. tile independence
@pytest.mark.parametrize("n,d,density", [(20000, 200, 0.2), (3000, 30, 0.3)])
def test_brute_csr_tile_independence(rp, ctx, oracle, n, d, density):
    """n = 20 000 splits the rows over several workgroups per tile and merges the partial lists,
    n = 3 000 is the plain path; nq = 5 and 300 end in a partial tile"""
    rowptr, col, val = oracle.data_normal_sparse2(5, n, d, density)
    ds = rp.Dataset.csr(ctx, rowptr, col, val, d)
    allq = queries_with_stored_rows(oracle, (rowptr, col, val), d, density, 300, 6)
    for nq in (1, 5, 64, 300):
        qr, qc, qv = take_rows(*allq, list(range(nq)))
        for refm, k in ((False, 10), (False, 200), (True, 10)):
            got = {}
            for tile in (1, 2, 0):
                with option(ctx, "brute_csr_tile", tile):
                    got[tile] = rp.bruteKnn(ds, (qr, qc, qv, d), k, reference_metric=refm)
            for tile in (1, 2):
                assert np.array_equal(got[tile][0], got[0][0]), (nq, refm, k, tile)
                assert np.array_equal(got[tile][1].view(np.uint64), got[0][1].view(np.uint64)), (nq, refm, k, tile)
    assert ctx.get_option("brute_csr_tile") == 0


# ------------------------------------------------------------------ 5. agreement with the forest kNN
def csr_forest(rp, ctx, oracle, n, d, density, T, ml, seed=9):
    rowptr, col, val = oracle.data_normal_sparse2(5, n, d, density)
    L, _, pnz = oracle.tree_cfg(ml, n, d)
    R, _ = oracle.forest_hyperplanes(seed, T, L, pnz, d)
    f = rp.forestBatch(seed, L, ml, T, pnz, d, (rowptr, col, val, d), ctx=ctx, hyperplanes=R)
    return f, R, (rowptr, col, val)


def test_brute_csr_agrees_with_forest_knn(rp, ctx, oracle):
    """Fresh queries: the forest kernels sum |q|^2 in another order than a row's terms, so at
    distance 0 (a stored row as the query) they carry their documented 1e-8 |q| absolute error and
    are not comparable at atol = 1e-12; everywhere else both evaluate the same formula."""
    n, d, T, ml, k = 20000, 200, 8, 40, 10
    f, _, _ = csr_forest(rp, ctx, oracle, n, d, 0.2, T, ml)
    qr, qc, qv = oracle.data_normal_sparse2(6, 48, d, 0.2)
    qs = (qr, qc, qv, d)
    ids, dist, cnt = rp.knnBatch(k, f, qs, dedup=True)
    bi, bd = rp.bruteKnn(f, qs, k)
    common = 0
    for i in range(48):
        assert cnt[i] == k
        where = {int(v): p for p, v in enumerate(bi[i])}
        for p in range(k):
            j = where.get(int(ids[i, p]))
            if j is not None:
                assert np.isclose(dist[i, p], bd[i, j], rtol=RTOL, atol=ATOL), (i, p)
                common += 1
        assert np.all(dist[i] >= bd[i] - (RTOL * bd[i] + ATOL)), i
    assert common > 0


# ------------------------------------------------------------------ 6. recallWithBatch
def host_hits(rp, f, qs, truth):
    off, cids = rp.candidatesBatch(f, qs)
    nq, T = truth.shape[0], f.T
    hits = np.zeros((nq, T), dtype=np.int32)
    for i in range(nq):
        tr = set(int(v) for v in truth[i] if v >= 0)
        for t in range(T):
            hits[i, t] = len(set(cids[off[i * T + t]:off[i * T + t + 1]].tolist()) & tr)
    return hits


def test_recall_hits_csr_forest(rp, ctx, oracle):
    n, d, T, ml, k = 20000, 200, 8, 40, 10
    f, R, (rowptr, col, val) = csr_forest(rp, ctx, oracle, n, d, 0.2, T, ml)
    fo = oracle.forest_build_csr(rowptr, col, val, d, R, ml)
    assert np.array_equal(f.perm, fo.perm)
    qr, qc, qv = queries_with_stored_rows(oracle, (rowptr, col, val), d, 0.2, 48, 6)
    qs = (qr, qc, qv, d)
    for refm in (False, True):
        hits, truth = rp.recallHits(rp.metricL2, f, k, qs, reference_metric=refm)
        bi, _ = rp.bruteKnn(f, qs, k, reference_metric=refm)
        assert np.array_equal(truth, bi)
        assert np.array_equal(hits, host_hits(rp, f, qs, truth)), refm
        for i in range(0, 48, 5):                        # ... and on the oracle's candidates
            a, b = qr[i], qr[i + 1]
            tr = set(truth[i].tolist())
            for t in range(T):
                want = oracle.candidates_sparse(fo, qc[a:b], qv[a:b], t)
                assert hits[i, t] == len(set(want.tolist()) & tr), (refm, i, t)
        rec = rp.recallWithBatch(rp.metricL2, f, k, qs, reference_metric=refm)
        assert rec.shape == (48,)
        for i in range(48):
            assert rec[i] == sum(int(h) / k for h in hits[i]) / T
        for i in (0, 9, 47):
            one = take_rows(qr, qc, qv, [i])
            r1 = rp.recallWith(rp.metricL2, f, k, one + (d,), reference_metric=refm)
            assert np.float64(r1).view(np.uint64) == rec[i].view(np.uint64)
            sv = rp.SVector(d, one[1], one[2])
            assert rp.recallWith(rp.metricL2, f, k, sv, reference_metric=refm) == r1
        if not refm:
            assert np.all(hits[:8].min(axis=1) >= 1)     # a stored row is in its own leaf of every tree


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_recall_hits_dense_forest_all_metrics(rp, ctx, oracle, dtype):
    n, d, T, ml, k, nq = 3000, 16, 4, 30, 12, 24         # test_cpp_knn_cosine's shape
    X = oracle.data_normal_dense2(41, n, d).astype(dtype)
    cfg = rp.rpTreeCfg(ml, n, d)
    f = rp.forestBatch(5, cfg.fpMaxTreeDepth, ml, T, cfg.fpProjNzDensity, d, X, ctx=ctx)
    Q = oracle.data_normal_dense2(3, nq, d).astype(dtype)
    Q[:4] = X[:4]
    for distf in (rp.metricL2, rp.metricCosine, rp.metricInner):
        hits, truth = rp.recallHits(distf, f, k, Q)
        bi, _ = rp.bruteKnn(f, Q, k, metric=distf)
        assert np.array_equal(truth, bi)
        assert np.array_equal(hits, host_hits(rp, f, Q, truth))
        rec = rp.recallWithBatch(distf, f, k, Q)
        for i in (0, 5, nq - 1):
            r1 = rp.recallWith(distf, f, k, Q[i])
            assert np.float64(r1).view(np.uint64) == rec[i].view(np.uint64)
            assert r1 == sum(int(h) / k for h in hits[i]) / T


def test_recall_hits_streamed_forest(rp, ctx, oracle):
    n, d, T, ml, k, nq, chunk = 3000, 16, 4, 30, 12, 24, 700
    X = oracle.data_normal_dense2(41, n, d)
    cfg = rp.rpTreeCfg(ml, n, d)
    f = rp.forest(5, cfg.fpMaxTreeDepth, ml, T, chunk, cfg.fpProjNzDensity, d, X, ctx=ctx)
    Q = oracle.data_normal_dense2(3, nq, d)
    Q[:4] = X[:4]
    hits, truth = rp.recallHits(rp.metricL2, f, k, Q)
    assert np.array_equal(hits, host_hits(rp, f, Q, truth))
    assert hits.sum() > 0


def test_recall_hits_c3_shape(rp, ctx):
    """1M x 784, density 0.19, 32 trees, 256 queries, k = 10: hits against the host intersection on
    16 sampled queries; prints the mean recall"""
    n, d, T, ml, k, nq = 1_000_000, 784, 32, 128, 10, 256
    rng = np.random.default_rng(1234)
    cols, counts = [], []
    for r0 in range(0, n + nq, 50_000):
        m = rng.random((min(50_000, n + nq - r0), d), dtype=np.float32) < 0.19
        counts.append(m.sum(axis=1))
        cols.append(np.nonzero(m)[1].astype(np.int32))
    col = np.concatenate(cols)
    rowptr = np.zeros(n + nq + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(np.concatenate(counts))
    val = 1.0 - rng.random(int(rowptr[-1]))
    e = rowptr[n]
    qr, qc, qv = rowptr[n:] - e, col[e:], val[e:]
    rowptr, col, val = rowptr[:n + 1], col[:e], val[:e]
    cfg = rp.rpTreeCfg(ml, n, d)
    f = rp.forestBatch(1235137, cfg.fpMaxTreeDepth, ml, T, cfg.fpProjNzDensity, d, (rowptr, col, val, d),
                       ctx=ctx)
    qs = (qr, qc, qv, d)
    hits, truth = rp.recallHits(rp.metricL2, f, k, qs)
    assert hits.shape == (nq, T) and np.all(truth >= 0) and np.all(hits >= 0) and np.all(hits <= k)
    sample = list(range(0, nq, 16))
    sub = take_rows(qr, qc, qv, sample) + (d,)
    assert np.array_equal(hits[sample], host_hits(rp, f, sub, truth[sample]))
    # the truth of the sampled queries against numpy, on the rows the device named and a random sample
    Qd = densify(sub[0], sub[1], sub[2], d)
    probe = np.random.default_rng(1).integers(0, n, 2000)
    for j, i in enumerate(sample[:4]):
        rows = np.concatenate([truth[i], probe])
        Xd = densify(*take_rows(rowptr, col, val, rows.tolist()), d)
        dd = np.sqrt(((Xd - Qd[j][None, :]) ** 2).sum(axis=1))
        assert np.all(np.diff(dd[:k]) >= -RTOL * dd[:k - 1])
        outside = ~np.isin(probe, truth[i])
        assert dd[k:][outside].min() >= dd[k - 1] * (1 - RTOL)
    rec = rp.recallWithBatch(rp.metricL2, f, k, qs)
    print("C3 shape: mean recall@%d over %d queries, %d trees = %.4f" % (k, nq, T, rec.mean()))
    assert np.array_equal(rec, np.array([sum(int(h) / k for h in row) / T for row in hits]))


# ------------------------------------------------------------------ 7. argument rules
def test_brute_csr_argument_rules(rp, ctx, oracle):
    import ctypes as C
    from rptree_amd import _lib
    n, d, k = 500, 30, 5
    rowptr, col, val = oracle.data_normal_sparse2(5, n, d, 0.3)
    f = rp.forestBatch(4, 4, 30, 2, 0.5, d, (rowptr, col, val, d), ctx=ctx)
    ds = f.data
    dd = rp.Dataset.dense(ctx, densify(rowptr, col, val, d))
    qc_ = rp.Dataset.csr(ctx, rowptr[:5], col[:rowptr[4]], val[:rowptr[4]], d)
    qd_ = rp.Dataset.dense(ctx, densify(rowptr[:5], col[:rowptr[4]], val[:rowptr[4]], d))
    ids = np.empty((4, 2048), dtype=np.int32)
    dist = np.empty((4, 2048), dtype=np.float64)
    pi, pd = C.c_void_p(ids.ctypes.data), C.c_void_p(dist.ctypes.data)
    L = _lib.lib()

    def message():
        return L.rpt_last_error().decode()

    for data, q in ((ds, qd_), (dd, qc_)):               # a dense / CSR mix
        assert L.rpt_brute_knn_host(ctx._h, data._h, q._h, k, pi, pd) == RPT_E_ARG and message()
        assert L.rpt_brute_knn_metric_host(ctx._h, data._h, q._h, k, 0, pi, pd) == RPT_E_ARG and message()
    for flag in (rp.RPT_KNN_METRIC_COSINE, rp.RPT_KNN_METRIC_INNER):
        assert L.rpt_brute_knn_metric_host(ctx._h, ds._h, qc_._h, k, flag, pi, pd) == RPT_E_UNSUPPORTED
        assert "dense data only" in message()
    assert L.rpt_brute_knn_metric_host(ctx._h, dd._h, qd_._h, k, rp.RPT_KNN_METRIC_REFERENCE, pi,
                                       pd) == RPT_E_ARG and message()      # dense: the rule of before
    for kk in (0, 1025):
        assert L.rpt_brute_knn_host(ctx._h, ds._h, qc_._h, kk, pi, pd) == RPT_E_ARG and "k must be" in message()
    hits = np.empty((4, 2), dtype=np.int32)
    ph = C.c_void_p(hits.ctypes.data)
    assert L.rpt_recall_hits_host(ctx._h, f._h, ds._h, qd_._h, k, 0, ph, None) == RPT_E_ARG and message()
    assert L.rpt_recall_hits_host(ctx._h, f._h, ds._h, qc_._h, 1025, 0, ph, None) == RPT_E_ARG and message()
    assert L.rpt_recall_hits_host(ctx._h, f._h, ds._h, qc_._h, k, rp.RPT_KNN_METRIC_COSINE, ph,
                                  None) == RPT_E_UNSUPPORTED and message()
    # the context is usable afterwards; k > n pads with id -1 / +inf; k = 1024 is accepted
    got_i, got_d = rp.bruteKnn(ds, (rowptr[:5], col[:rowptr[4]], val[:rowptr[4]], d), 1024)
    assert np.array_equal(np.sort(got_i[:, :n], axis=1), np.tile(np.arange(n), (4, 1)))
    assert np.all(got_i[:, n:] == -1) and np.all(np.isposinf(got_d[:, n:]))
    assert np.all(got_d[:, 0] == 0.0) and np.array_equal(got_i[:, 0], np.arange(4))
    assert L.rpt_recall_hits_host(ctx._h, f._h, ds._h, qc_._h, k, 0, ph, None) == 0
    assert np.all(hits >= 1)


def test_brute_knn_dev_matches_host(rp, ctx, oracle):
    """rpt_brute_knn_dev writes the host entry points' answer into device arrays (CSR and dense)"""
    import ctypes as C
    import torch
    from rptree_amd import _lib
    n, d, k, nq = 3000, 30, 7, 9
    rowptr, col, val = oracle.data_normal_sparse2(5, n, d, 0.3)
    qr, qc, qv = oracle.data_normal_sparse2(6, nq, d, 0.3)
    cases = [(rp.Dataset.csr(ctx, rowptr, col, val, d), (qr, qc, qv, d), 0, {}),
             (rp.Dataset.csr(ctx, rowptr, col, val, d), (qr, qc, qv, d), rp.RPT_KNN_METRIC_REFERENCE,
              {"reference_metric": True}),
             (rp.Dataset.dense(ctx, densify(rowptr, col, val, d)), densify(qr, qc, qv, d), 0, {}),
             (rp.Dataset.dense(ctx, densify(rowptr, col, val, d)), densify(qr, qc, qv, d),
              rp.RPT_KNN_METRIC_COSINE, {"metric": rp.metricCosine})]
    for ds, qs, flags, kw in cases:
        want_i, want_d = rp.bruteKnn(ds, qs, k, **kw)
        qd, _ = rp._query_dataset(ctx, ds, qs)
        ti = torch.full((nq, k), -7, dtype=torch.int32, device="cuda")
        td = torch.zeros((nq, k), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        st = _lib.lib().rpt_brute_knn_dev(ctx._h, ds._h, qd._h, k, flags, C.c_void_p(ti.data_ptr()),
                                          C.c_void_p(td.data_ptr()))
        assert st == 0, _lib.lib().rpt_last_error()
        ctx.sync()
        assert np.array_equal(ti.cpu().numpy(), want_i), flags
        assert np.array_equal(td.cpu().numpy().view(np.uint64), want_d.view(np.uint64)), flags


# ------------------------------------------------------------------ 8. C++ example
def test_cpp_sparse_recall(rp, ctx, oracle, tmp_path):
    n, d, T, ml, k = 3000, 30, 4, 30, 12
    rowptr, col, val = oracle.data_normal_sparse2(5, n, d, 0.3)
    qr, qc, qv = oracle.data_normal_sparse2(6, 1, d, 0.3)
    data = tmp_path / "csr.bin"
    data.write_bytes(struct.pack("<qiq", n, d, int(rowptr[-1])) + rowptr.astype(np.int64).tobytes() +
                     col.astype(np.int32).tobytes() + val.astype(np.float64).tobytes() +
                     struct.pack("<i", len(qc)) + qc.astype(np.int32).tobytes() + qv.astype(np.float64).tobytes())
    exe = str(tmp_path / "example_sparse_recall")
    src = os.path.join(ROOT, "rp-tree_amd", "host", "example_sparse_recall.cpp")
    lib = os.path.join(ROOT, "rp-tree_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, src, "-L" + lib, "-lrptree_hip",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, str(data), str(T), str(ml), str(k)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok"

    def ints(prefix):
        ln = [x for x in lines if x.startswith(prefix)]
        assert len(ln) == 1, prefix
        return [int(v) for v in ln[0].split(":")[1].split()]

    cands = [set(ints("cand %d:" % t)) for t in range(T)]
    ds = rp.Dataset.csr(ctx, rowptr, col, val, d)
    for ref in (0, 1):
        truth = ints("truth %d:" % ref)
        want, _ = rp.bruteKnn(ds, (qr, qc, qv, d), k, reference_metric=bool(ref))
        assert truth == want[0].tolist()
        hits = ints("hits %d:" % ref)
        assert hits == [len(c & set(truth)) for c in cands]
        bits = [x for x in lines if x.startswith("recall %d:" % ref)][0].split(":")[1].strip()
        rec = np.array([int(bits, 16)], dtype=np.uint64).view(np.float64)[0]
        assert rec == sum(h / k for h in hits) / T
