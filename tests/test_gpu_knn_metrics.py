"""knn under the cosine and inner-product distances (RPT_KNN_METRIC_COSINE / _INNER) on the device
against a host restatement of their definitions, bit for bit:

    dot(x, q) = ((0 + x0 q0) + x1 q1) + ...      innerDD, Internal.hs:384-385, in Double
    inner     = -dot(x, q)
    cosine    = 1 - dot(x, q) / (sqrt(dot(x, x)) * sqrt(dot(q, q)))

candidates concatenated in tree order, then leaf order (RPTree.hs:176), ranked by (distance,
candidate position) with NaN behind every number, the duplicate rule, the first k.  The forest only
decides the candidates: f64 forests are checked against the oracle's candidates; f32 / bf16
forests rank their own (f32 query projections) and the answer is checked on those."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (1, 10, 64, 200)
DEDUPS = (0, 1, 2)          # keep, RPT_KNN_DEDUP, RPT_KNN_DEDUP_DISTANCE


@pytest.fixture(scope="module")
def rp():
    import rptree_amd
    return rptree_amd


@pytest.fixture(scope="module")
def ctx(rp):
    return rp.default_context()


# ------------------------------------------------------------------ host restatement
def fold_dots(Xc, q):
    """left-fold dots of every row of Xc with q, from +0.0 (numpy's cumsum is sequential)"""
    P = Xc * q[None, :]
    P = np.concatenate([np.zeros((P.shape[0], 1)), P], axis=1)
    return np.cumsum(P, axis=1)[:, -1]


def fold_self(Xc):
    P = Xc * Xc
    P = np.concatenate([np.zeros((P.shape[0], 1)), P], axis=1)
    return np.cumsum(P, axis=1)[:, -1]


def metric_values(metric, Xc, q, xx=None):
    dot = fold_dots(Xc, q)
    if metric == "inner":
        return -dot
    if xx is None:
        xx = fold_self(Xc)
    qq = fold_self(q[None, :])[0]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return 1.0 - dot / (np.sqrt(xx) * np.sqrt(qq))


def select(ids, vals, k, dedup):
    """stable order by (NaN last, value, position), the duplicate rule, the first k"""
    nan = np.isnan(vals)
    order = np.lexsort((np.arange(len(vals)), np.where(nan, 0.0, vals), nan))
    out_i, out_v, seen, last = [], [], set(), None
    for j in order:
        i, v = int(ids[j]), vals[j]
        if dedup == 1:
            if i in seen:
                continue
            seen.add(i)
        elif dedup == 2 and out_v and v == last:
            continue
        out_i.append(i)
        out_v.append(v)
        last = v
        if len(out_i) == k:
            break
    return np.array(out_i, dtype=np.int32), np.array(out_v, dtype=np.float64)


def same_bits(a, b):
    """bit-equal doubles; a NaN only has to be a NaN (the sign and payload of a NaN an operation
    makes are the platform's: x86 makes 0xfff8..., the GPU 0x7ff8...)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64),
                                                                            b[~nb].view(np.uint64))


def assert_answer(ids, dist, cnt, want, k, tag):
    wi, wv = want
    assert cnt == len(wi), (tag, cnt, len(wi))
    assert np.array_equal(ids[:cnt], wi), tag
    assert same_bits(dist[:cnt], wv), tag
    assert np.all(ids[cnt:] == -1) and np.all(np.isposinf(dist[cnt:])), tag


def flag_of(rp, metric):
    return rp.RPT_KNN_METRIC_COSINE if metric == "cosine" else rp.RPT_KNN_METRIC_INNER


def distf_of(rp, metric):
    return rp.metricCosine if metric == "cosine" else rp.metricInner


# ------------------------------------------------------------------ 1. parity grid
NAN_QUERY = 7


def dataset(oracle, n, d):
    X = oracle.data_normal_dense2(4000 + d, n, d)
    rng = np.random.default_rng(d)
    src = rng.integers(0, n, 60)
    X[rng.integers(0, n, 60)] = X[src]            # exact duplicate rows
    X[17] = 0.0                                   # a zero row: cosine NaN
    X[rng.integers(0, n, 40)] *= 10.0             # rows of other norms (inner product prefers them)
    return X


def queries(X, nq, d):
    rng = np.random.default_rng(d + 1)
    Q = rng.standard_normal((nq, d))
    Q[:6] = X[[0, 17, 99, 1234, 5000, 17]]        # stored points, the zero row
    Q[6] = 0.0                                    # a zero query: cosine NaN everywhere
    Q[NAN_QUERY] = rng.standard_normal(d)
    Q[NAN_QUERY, 3] = np.nan                      # a NaN query: NaN distances, ranked by position
    Q[8] = X[3] * 2.0
    return Q


@pytest.mark.parametrize("d", [48, 128])
@pytest.mark.parametrize("dtype", ["f64", "f32", "bf16"])
def test_metric_parity_grid(rp, ctx, oracle, d, dtype):
    n, T, ml, nq = 20_000, 8, 100, 24
    X = dataset(oracle, n, d)
    Q = queries(X, nq, d)
    cfg = rp.rpTreeCfg(ml, n, d)
    L = cfg.fpMaxTreeDepth
    _, R = rp.gen.forest_hyperplanes(77, T, L, cfg.fpProjNzDensity, d)
    if dtype == "f64":
        Xh, Qh = X, Q
        ds = rp.Dataset.dense(ctx, X)
    elif dtype == "f32":
        Xh, Qh = X.astype(np.float32).astype(np.float64), Q.astype(np.float32).astype(np.float64)
        ds = rp.Dataset.dense(ctx, X.astype(np.float32))
    else:
        Xb = rp.to_bf16(X.astype(np.float32))
        Xh = rp.from_bf16(Xb).astype(np.float64)
        Qh = rp.from_bf16(rp.to_bf16(Q.astype(np.float32))).astype(np.float64)
        ds = rp.Dataset.dense(ctx, Xb, dtype=rp.RPT_BF16)
    f = rp._build(ctx, ds, R, L, ml, rp.RPT_PROJ_AUTO)
    off, cids = rp.candidatesBatch(f, Q)
    cands = [cids[off[i * T]:off[(i + 1) * T]] for i in range(nq)]
    if dtype == "f64":                            # the oracle's candidates, tree order then leaf order
        fo = oracle.forest_build_dense(X, R, ml)
        assert np.array_equal(f.perm, fo.perm)
        for i in range(nq):
            if i == NAN_QUERY:      # (which leaves a NaN projection reaches is the walk's business, not
                continue            # the metric's: the answer is checked on the device's own candidates)
            want = np.concatenate([oracle.candidates_dense(fo, Q[i], t) for t in range(T)])
            assert np.array_equal(cands[i], want), i
            cands[i] = want
    xx = fold_self(Xh)
    for metric in ("cosine", "inner"):
        vals = [metric_values(metric, Xh[c], Qh[i], xx[c]) for i, c in enumerate(cands)]
        for dedup in DEDUPS:
            for k in KS:
                ids, dist, cnt = rp.knnBatch(k, f, Q, dedup=dedup, metric=distf_of(rp, metric))
                for i in range(nq):
                    want = select(cands[i], vals[i], k, dedup)
                    assert_answer(ids[i], dist[i], cnt[i], want, k, (dtype, d, metric, dedup, k, i))
    # the public knn / knnPQ of one query
    for metric in ("cosine", "inner"):
        got = rp.knn(distf_of(rp, metric), 10, f, Q[0])
        wi, wv = select(cands[0], metric_values(metric, Xh[cands[0]], Qh[0], xx[cands[0]]), 10, 0)
        assert [g[1] for g in got] == wi.tolist()
        assert same_bits([g[0] for g in got], wv)
        got = rp.knnPQ(distf_of(rp, metric), 10, f, Q[0])
        wi, wv = select(cands[0], metric_values(metric, Xh[cands[0]], Qh[0], xx[cands[0]]), 10, 2)
        assert [g[1] for g in got] == wi.tolist()
    # host functions agree with the device values (f64 rows: bits)
    if dtype == "f64":
        ids, dist, cnt = rp.knnBatch(5, f, Q[:1], metric=rp.metricCosine)
        for j in range(cnt[0]):
            assert dist[0, j] == rp.metricCosine(X[ids[0, j]], Q[0])
    f.close()
    ds.close()


# ------------------------------------------------------------------ 2. streamed forest
def test_metric_on_a_streamed_forest(rp, ctx, oracle):
    n, d, T, ml, chunk, nq = 8000, 48, 6, 40, 700, 20
    X = dataset(oracle, n, d)
    Q = queries(X, nq, d)
    L, _, pnz = oracle.tree_cfg(ml, n, d)
    R, _ = oracle.forest_hyperplanes(19, T, L, pnz, d)
    f = rp.forest(0, L, ml, T, chunk, pnz, d, X, ctx=ctx, hyperplanes=R)
    so = oracle.stream_forest_dense(X, R, ml, chunk)
    cands = [np.concatenate([oracle.stream_candidates_dense(so, R, Q[i], t) for t in range(T)])
             for i in range(nq)]
    off, cids = rp.candidatesBatch(f, Q)
    for i in range(nq):
        if i == NAN_QUERY:
            cands[i] = cids[off[i * T]:off[(i + 1) * T]]
        assert np.array_equal(cids[off[i * T]:off[(i + 1) * T]], cands[i]), i
    xx = fold_self(X)
    for metric in ("cosine", "inner"):
        vals = [metric_values(metric, X[c], Q[i], xx[c]) for i, c in enumerate(cands)]
        for dedup in DEDUPS:
            for k in (1, 10, 64):
                ids, dist, cnt = rp.knnBatch(k, f, Q, dedup=dedup, metric=distf_of(rp, metric))
                for i in range(nq):
                    assert_answer(ids[i], dist[i], cnt[i], select(cands[i], vals[i], k, dedup), k,
                                  (metric, dedup, k, i))
    f.close()


# ------------------------------------------------------------------ 3. C2 scale
def test_metric_c2_scale(rp, ctx, oracle):
    n, d, T, nq, k = 1_000_000, 128, 32, 256, 10
    X = oracle.data_normal_dense2(2, n, d)
    cfg = rp.rpTreeCfg(256, n, d)
    f = rp.forestBatch(1, cfg.fpMaxTreeDepth, 256, T, cfg.fpProjNzDensity, d, X, ctx=ctx)
    Q = oracle.data_normal_dense2(3, nq, d)
    Q[:8] = X[:8]
    off, cids = rp.candidatesBatch(f, Q)
    rng = np.random.default_rng(0)
    for metric in ("cosine", "inner"):
        ids, dist, cnt = rp.knnBatch(k, f, Q, metric=distf_of(rp, metric))
        cand = 0
        for i in range(nq):
            c = cids[off[i * T]:off[(i + 1) * T]]
            cand += len(c)
            vals = metric_values(metric, X[c], Q[i])
            assert_answer(ids[i], dist[i], cnt[i], select(c, vals, k, 0), k, (metric, i))
        # the numpy fold is innerDD: cross-check a sample against the oracle's pinned one
        for i in rng.integers(0, nq, 4):
            j = int(ids[i, 0])
            dq = oracle.inner_dd(X[j], Q[i])
            want = -dq if metric == "inner" else 1.0 - np.float64(dq) / (
                np.float64(math.sqrt(oracle.inner_dd(X[j], X[j]))) * math.sqrt(oracle.inner_dd(Q[i], Q[i])))
            assert np.float64(want).view(np.uint64) == dist[i, 0].view(np.uint64)
        assert cand == int(off[-1])
    f.close()


# ------------------------------------------------------------------ 4. brute force, recallWith
@pytest.mark.parametrize("dtype", ["f64", "f32", "bf16"])
def test_metric_brute_force(rp, ctx, oracle, dtype):
    import ctypes as C
    n, d, nq, k = 20_000, 48, 10, 25
    X = dataset(oracle, n, d)
    Q = queries(X, nq, d)
    if dtype == "f64":
        Xh, Qh, ds = X, Q, rp.Dataset.dense(ctx, X)
    elif dtype == "f32":
        Xh, Qh = X.astype(np.float32).astype(np.float64), Q.astype(np.float32).astype(np.float64)
        ds = rp.Dataset.dense(ctx, X.astype(np.float32))
    else:
        Xb = rp.to_bf16(X.astype(np.float32))
        Xh = rp.from_bf16(Xb).astype(np.float64)
        Qh = rp.from_bf16(rp.to_bf16(Q.astype(np.float32))).astype(np.float64)
        ds = rp.Dataset.dense(ctx, Xb, dtype=rp.RPT_BF16)
    xx = fold_self(Xh)
    allids = np.arange(n, dtype=np.int32)
    for metric in ("cosine", "inner"):
        ids, dist = rp.bruteKnn(ds, Q, k, metric=distf_of(rp, metric))
        for i in range(nq):
            wi, wv = select(allids, metric_values(metric, Xh, Qh[i], xx), k, 0)
            assert np.array_equal(ids[i, :len(wi)], wi), (metric, i)
            assert same_bits(dist[i, :len(wi)], wv)
        # the C entry point directly, and flag 0 = L2 (rpt_brute_knn_host)
        from rptree_amd import _lib
        qd, _ = rp._query_dataset(ctx, ds, Q)
        ids2 = np.empty((nq, k), dtype=np.int32)
        dist2 = np.empty((nq, k), dtype=np.float64)
        _lib.check(_lib.lib().rpt_brute_knn_metric_host(ctx._h, ds._h, qd._h, k, flag_of(rp, metric),
                                                        C.c_void_p(ids2.ctypes.data),
                                                        C.c_void_p(dist2.ctypes.data)))
        assert np.array_equal(ids2, ids) and same_bits(dist2, dist)
    li, ld = rp.bruteKnn(ds, Q, k)
    ids2 = np.empty((nq, k), dtype=np.int32)
    dist2 = np.empty((nq, k), dtype=np.float64)
    qd, _ = rp._query_dataset(ctx, ds, Q)
    from rptree_amd import _lib
    _lib.check(_lib.lib().rpt_brute_knn_metric_host(ctx._h, ds._h, qd._h, k, 0,
                                                    C.c_void_p(ids2.ctypes.data), C.c_void_p(dist2.ctypes.data)))
    assert np.array_equal(ids2, li) and same_bits(dist2, ld)
    with pytest.raises(rp.RPTError):
        _lib.check(_lib.lib().rpt_brute_knn_metric_host(
            ctx._h, ds._h, qd._h, k, rp.RPT_KNN_METRIC_COSINE | rp.RPT_KNN_METRIC_INNER,
            C.c_void_p(ids2.ctypes.data), C.c_void_p(dist2.ctypes.data)))
    ds.close()


def test_recall_with_cosine(rp, ctx, oracle):
    n, d, T, ml, k = 20_000, 48, 8, 100, 20
    X = dataset(oracle, n, d)
    cfg = rp.rpTreeCfg(ml, n, d)
    f = rp.forestBatch(5, cfg.fpMaxTreeDepth, ml, T, cfg.fpProjNzDensity, d, X, ctx=ctx)
    xx = fold_self(X)
    for q in (X[5] * 1.5, np.random.default_rng(4).standard_normal(d)):
        for metric in ("cosine", "inner"):
            truth, _ = select(np.arange(n, dtype=np.int32), metric_values(metric, X, q, xx), k, 0)
            off, cids = rp.candidatesBatch(f, q)
            want = sum(len(set(cids[off[t]:off[t + 1]].tolist()) & set(truth.tolist())) / k
                       for t in range(T)) / T
            assert rp.recallWith(distf_of(rp, metric), f, k, q) == want
    f.close()


# ------------------------------------------------------------------ 5. sharded path, merges
def test_metric_sharded_forced_exchange(rp, ctx, oracle):
    from rptree_amd import sharded
    n, d, T, ml, nq, k = 20_000, 48, 8, 100, 64, 10
    X = dataset(oracle, n, d)
    Q = queries(X, nq, d)
    cfg = rp.rpTreeCfg(ml, n, d)
    _, R = rp.gen.forest_hyperplanes(3, T, cfg.fpMaxTreeDepth, cfg.fpProjNzDensity, d)
    comm = sharded.Comm.rank(ctx, 1, 0, sharded.Comm.unique_id())
    old = ctx.set_option("comm_force_exchange", 1)
    try:
        ds = rp.Dataset.dense(ctx, X)
        sf = sharded.ShardedForest(comm, [ds], R, cfg.fpMaxTreeDepth, ml)
        plain, _, _ = sf.local(0)
        qs = rp.Dataset.dense(ctx, Q)
        for metric in (rp.metricCosine, rp.metricInner):
            for dedup in (False, True):
                si, sd, sc = sf.knn([qs], k, dedup=dedup, metric=metric)
                wi, wd, wc = rp.knnBatch(k, plain, qs, dedup=dedup, metric=metric)
                assert np.array_equal(si, wi) and np.array_equal(sc, wc)
                assert same_bits(sd, wd)
        qs.close()
        sf.close()
        ds.close()
    finally:
        ctx.set_option("comm_force_exchange", old)
        comm.close()


def host_merge(ids, dist, cnt, k, dedup):
    """G shard lists -> one: (NaN last, value, shard position) order, the duplicate rule"""
    G, nq, _ = ids.shape
    out = []
    for q in range(nq):
        ii = np.concatenate([ids[g, q, :cnt[g, q]] for g in range(G)])
        vv = np.concatenate([dist[g, q, :cnt[g, q]] for g in range(G)])
        out.append(select(ii, vv, k, dedup))
    return out


def test_merge_orders_negative_and_nan_distances(rp, ctx):
    import torch
    from rptree_amd import _lib
    G, nq, k = 3, 5, 6
    rng = np.random.default_rng(8)
    # every shard's list sorted as a device answer: numbers (negative ones among them: the inner
    # metric), then NaN; ids distinct except one id found by two shards with its one distance
    dist = np.sort(rng.integers(-4, 3, (G, nq, k)).astype(np.float64) * 0.5, axis=2)
    dist[0, 0, 4:] = np.nan
    dist[1, 0, 3:] = np.nan
    dist[2, 1, :] = np.nan                    # a shard whose answers are all NaN (a NaN query)
    ids = np.broadcast_to(np.arange(G * k, dtype=np.int32).reshape(G, 1, k), (G, nq, k)).copy()
    ids[1, 2, 0] = ids[0, 2, 0]
    dist[1, 2, 0] = dist[0, 2, 0]             # (the merge takes its lists in any order)
    cnt = np.full((G, nq), k, dtype=np.int32)
    cnt[2, 3] = 2
    cnt[0, 4] = 0
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    di, dd, dc = dev(ids), dev(dist), dev(cnt)
    oi = torch.empty((nq, k), dtype=torch.int32, device="cuda")
    od = torch.empty((nq, k), dtype=torch.float64, device="cuda")
    oc = torch.empty((nq,), dtype=torch.int32, device="cuda")
    for dedup in (0, 1, 2):
        torch.cuda.synchronize()
        _lib.check(_lib.lib().rpt_knn_merge_dev(ctx._h, di.data_ptr(), dd.data_ptr(), dc.data_ptr(), G, nq, k,
                                                dedup, oi.data_ptr(), od.data_ptr(), oc.data_ptr()))
        ctx.sync()
        gi, gd, gc = oi.cpu().numpy(), od.cpu().numpy(), oc.cpu().numpy()
        for q, (wi, wv) in enumerate(host_merge(ids, dist, cnt, k, dedup)):
            assert gc[q] == len(wi), (dedup, q)
            assert np.array_equal(gi[q, :gc[q]], wi), (dedup, q, gi[q], wi)
            assert same_bits(gd[q, :gc[q]], wv), (dedup, q)


# ------------------------------------------------------------------ 6. argument rules
def test_metric_argument_rules(rp, ctx, oracle):
    import ctypes as C
    from rptree_amd import _lib
    n, d, T, ml, k = 5000, 16, 4, 40, 5
    X = oracle.data_normal_dense2(31, n, d)
    cfg = rp.rpTreeCfg(ml, n, d)
    f = rp.forestBatch(2, cfg.fpMaxTreeDepth, ml, T, cfg.fpProjNzDensity, d, X, ctx=ctx)
    Q = oracle.data_normal_dense2(32, 8, d)
    qd, nq = rp._query_dataset(ctx, f.data, Q)
    ids = np.empty((nq, k), dtype=np.int32)
    dist = np.empty((nq, k), dtype=np.float64)
    cnt = np.empty(nq, dtype=np.int32)

    def call(flags):
        return _lib.lib().rpt_knn_host(ctx._h, f._h, f.data._h, qd._h, k, flags, C.c_void_p(ids.ctypes.data),
                                       C.c_void_p(dist.ctypes.data), C.c_void_p(cnt.ctypes.data))

    RPT_E_ARG, RPT_E_UNSUPPORTED = -1, -4
    cos, inn = rp.RPT_KNN_METRIC_COSINE, rp.RPT_KNN_METRIC_INNER
    assert call(cos | inn) == RPT_E_ARG
    assert call(cos | rp.RPT_KNN_METRIC_REFERENCE) == RPT_E_ARG
    assert call(inn | rp.RPT_KNN_METRIC_REFERENCE) == RPT_E_ARG
    assert call(cos | (2 << 8)) == RPT_E_UNSUPPORTED
    assert "VOTE" in _lib.lib().rpt_last_error().decode()
    assert call(inn | (1 << 8)) == RPT_E_UNSUPPORTED
    # SVector rows
    rowptr, col, val = oracle.data_sparse_uniform(33, 3000, 64, 0.2)
    fc = rp.forestBatch(4, 8, 30, 2, 0.5, 64, (rowptr, col, val, 64), ctx=ctx)
    qc, nqc = rp._query_dataset(ctx, fc.data, (rowptr[:5], col[:rowptr[4]], val[:rowptr[4]], 64))
    ci = np.empty((nqc, k), dtype=np.int32)
    cd = np.empty((nqc, k), dtype=np.float64)
    cc = np.empty(nqc, dtype=np.int32)
    for flag in (cos, inn):
        st = _lib.lib().rpt_knn_host(ctx._h, fc._h, fc.data._h, qc._h, k, flag, C.c_void_p(ci.ctypes.data),
                                     C.c_void_p(cd.ctypes.data), C.c_void_p(cc.ctypes.data))
        assert st == RPT_E_UNSUPPORTED
        assert "dense" in _lib.lib().rpt_last_error().decode()
    fc.close()
    # the context is still usable: an L2 query right after equals the oracle
    fo = oracle.forest_build_dense(X, f.R, ml)
    li, ldist, lc = rp.knnBatch(k, f, Q)
    for i in range(len(Q)):
        wi, wd = oracle.knn_dense(fo, X, Q[i], k)
        assert np.array_equal(li[i, :lc[i]], wi)
        assert np.allclose(ldist[i, :lc[i]], wd, rtol=1e-12)
    f.close()


# ------------------------------------------------------------------ 7. C++ mirror
def _compile_cpp(out):
    src = os.path.join(ROOT, "rp-tree_amd", "host", "example_metric.cpp")
    lib = os.path.join(ROOT, "rp-tree_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", out, src, "-L" + lib, "-lrptree_hip",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])


def test_cpp_knn_cosine(rp, oracle, tmp_path):
    n, d, T, ml, k = 3000, 16, 4, 30, 12
    X = oracle.data_normal_dense2(41, n, d)
    q = X[7] * 0.5 + X[8] * 0.5
    data = tmp_path / "data.bin"
    data.write_bytes(struct.pack("<qi", n, d) + X.tobytes() + q.tobytes())
    exe = str(tmp_path / "example_metric")
    _compile_cpp(exe)
    r = subprocess.run([exe, str(data), str(T), str(ml), str(k)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok"
    cands = np.concatenate([np.array([int(v) for v in ln.split(":")[1].split()], dtype=np.int32)
                            for ln in lines if ln.startswith("cand ")])
    got = [tuple(x.split(":")) for x in lines[-2].split()[1:]]
    wi, wv = select(cands, metric_values("cosine", X[cands], q), k, 0)
    assert [int(i) for i, _ in got] == wi.tolist()
    assert same_bits(np.array([int(b, 16) for _, b in got], dtype=np.uint64).view(np.float64), wv)
