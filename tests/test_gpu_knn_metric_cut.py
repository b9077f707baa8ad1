"""The cut of the cosine / inner-product kNN (RPT_KNN_METRIC_COSINE / _INNER) on inputs chosen to
break it, against a host restatement of the definition, bit for bit:

    dot(x, q) = ((0 + x0 q0) + x1 q1) + ...      innerDD, Internal.hs:384-385, in Double
    inner     = -dot(x, q)
    cosine    = 1 - dot(x, q) / (sqrt(dot(x, x)) * sqrt(dot(q, q)))

every candidate ranked by (NaN last, value, candidate position), the duplicate rule on those values,
the first k (RPTree.hs:174-176).  The device ranks on a differently ordered f64 sum and keeps a
margin; these inputs make the two sums disagree by far more than an ulp (cancellation), tie many
different rows exactly (permutations), give rows equal sums in one order and not the other (swaps
inside one load, under knnPQ's `nub`), and put k at the LDS ceiling.  Every point is a candidate:
maxDepth-0 forests (one Tip per tree), T trees = T copies of every point."""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DTYPES = ("f64", "f32", "bf16")
METRICS = ("cosine", "inner")
DEDUPS = (0, 1, 2)          # keep, RPT_KNN_DEDUP, RPT_KNN_DEDUP_DISTANCE


@pytest.fixture(scope="module")
def rp():
    import rptree_amd
    return rptree_amd


@pytest.fixture(scope="module")
def ctx(rp):
    return rp.default_context()


@pytest.fixture
def option(ctx):
    """option(name, value): context manager switching one option of the context for the enclosed calls"""
    @contextlib.contextmanager
    def switch(name, value):
        old = ctx.set_option(name, value)
        try:
            yield
        finally:
            ctx.set_option(name, old)
    return switch


# ------------------------------------------------------------------ host restatement
def fold_dots(Xc, q):
    """left-fold dots of every row of Xc with q, from +0.0 (numpy's cumsum is sequential)"""
    P = Xc * q[None, :]
    P = np.concatenate([np.zeros((P.shape[0], 1)), P], axis=1)
    return np.cumsum(P, axis=1)[:, -1]


def fold_self(Xc):
    P = np.concatenate([np.zeros((Xc.shape[0], 1)), Xc * Xc], axis=1)
    return np.cumsum(P, axis=1)[:, -1]


def metric_values(metric, Xc, q):
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        dot = fold_dots(Xc, q)
        if metric == "inner":
            return -dot
        qq = fold_self(q[None, :])[0]
        return 1.0 - dot / (np.sqrt(fold_self(Xc)) * np.sqrt(qq))


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
    """bit-equal doubles; a NaN only has to be a NaN (its sign and payload are the platform's)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64),
                                                                            b[~nb].view(np.uint64))


def mismatch(ids, dist, cnt, want):
    """None when one device answer is the wanted one, else a short reason"""
    wi, wv = want
    k = len(ids)
    if cnt != len(wi):
        return "count %d, want %d" % (cnt, len(wi))
    if not np.array_equal(ids[:cnt], wi):
        j = int(np.argmax(ids[:cnt] != wi))
        return "id %d at rank %d, want %d" % (ids[j], j, wi[j])
    if not same_bits(dist[:cnt], wv):
        return "distance bits"
    if not (np.all(ids[cnt:k] == -1) and np.all(np.isposinf(dist[cnt:k]))):
        return "padding"
    return None


def distf_of(rp, metric):
    return rp.metricCosine if metric == "cosine" else rp.metricInner


def rounded(rp, X, dtype):
    """X rounded to dtype, as f64 (exactly what the device reads)"""
    if dtype == "f64":
        return np.array(X, dtype=np.float64)
    if dtype == "f32":
        return np.asarray(X, dtype=np.float32).astype(np.float64)
    return rp.from_bf16(rp.to_bf16(np.asarray(X, dtype=np.float32))).astype(np.float64)


def device_data(rp, ctx, Xh, dtype):
    if dtype == "f64":
        return rp.Dataset.dense(ctx, np.ascontiguousarray(Xh))
    if dtype == "f32":
        return rp.Dataset.dense(ctx, np.ascontiguousarray(Xh.astype(np.float32)))
    return rp.Dataset.dense(ctx, rp.to_bf16(np.ascontiguousarray(Xh.astype(np.float32))), dtype=rp.RPT_BF16)


class Flat:
    """every point a candidate: a maxDepth-0 forest of T trees over dtype rows Xh (f64 values that
    are exact in dtype); the candidate list of a query is T copies of 0 .. n-1"""

    def __init__(self, rp, ctx, Xh, dtype, T):
        self.Xh, self.dtype, self.T = Xh, dtype, T
        n, d = Xh.shape
        self.ds = device_data(rp, ctx, Xh, dtype)
        self.f = rp._build(ctx, self.ds, np.zeros((T, 0, d)), 0, 1, rp.RPT_PROJ_AUTO)
        self.cands = np.tile(np.arange(n, dtype=np.int32), T)

    def close(self):
        self.f.close()
        self.ds.close()


def check_knn(rp, ctx, f, Xh, Qh, cands, metrics, dedups, ks, tag):
    """every (metric, dedup, k) of knnBatch against the definition on the given candidate lists;
    returns (the failures, the uncertified counts per call)"""
    bad, unc = [], {}
    nq = len(Qh)
    for metric in metrics:
        vals = [metric_values(metric, Xh[cands[i]], Qh[i]) for i in range(nq)]
        for dedup in dedups:
            for k in ks:
                ids, dist, cnt = rp.knnBatch(k, f, Qh, dedup=dedup, metric=distf_of(rp, metric))
                unc[(metric, dedup, k)] = rp.knn_last_uncertified(ctx)
                for i in range(nq):
                    why = mismatch(ids[i], dist[i], cnt[i], select(cands[i], vals[i], k, dedup))
                    if why:
                        bad.append((tag, metric, dedup, k, i, why))
    return bad, unc


def check_exact_option(rp, f, Q, metrics, dedups, ks, option):
    """knn_metric_exact = 1 (every query on the exact variant) answers as the default path"""
    bad = []
    for metric in metrics:
        for dedup in dedups:
            for k in ks:
                a = rp.knnBatch(k, f, Q, dedup=dedup, metric=distf_of(rp, metric))
                with option("knn_metric_exact", 1):
                    b = rp.knnBatch(k, f, Q, dedup=dedup, metric=distf_of(rp, metric))
                if not (np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and same_bits(a[1], b[1])):
                    bad.append((metric, dedup, k))
    return bad


# ------------------------------------------------------------------ adversarial data
def cancellation_set(rp, dtype, M, n=600, d=128, nq=6, seed=1):
    """rows M e + v with e = e_0 - e_70 (two large components in different loads of a row) and
    queries with q_0 = q_70: q . e = 0 exactly, the products of size M cancel, and what is left
    of the sum depends on the order of the additions"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.5, 1.5, n)
    X = rng.standard_normal((n, d))
    X[:, 0] += M * a
    X[:, 70] -= M * a
    Q = rng.standard_normal((nq, d))
    Q[:, 70] = Q[:, 0]
    return rounded(rp, X, dtype), rounded(rp, Q, dtype)


def spread_row(rng, d, dtype):
    """a positive row whose partial sums round whatever the element type: the shorter the
    significand, the wider the range of exponents"""
    e = {"f64": 2, "f32": 16, "bf16": 26}[dtype]
    return rng.uniform(1.0, 2.0, d) * np.exp2(rng.integers(-e, e + 1, d))


def tie_set(rp, dtype, k, nperm=60, d=128, seed=2):
    """nperm different rows, coordinate permutations of one row (equal exact dots with a constant
    query, and with a query constant on four blocks when the permutations stay inside the blocks),
    placed around the k-th place: k - 3 rows clearly nearer, 150 clearly farther"""
    rng = np.random.default_rng(seed + k)
    b = rounded(rp, spread_row(rng, d, dtype)[None, :], dtype)[0]
    b = np.abs(b)                                    # dot with a positive query: positive
    blk = d // 4
    perms = []
    for j in range(nperm):
        p = np.concatenate([rng.permutation(blk) + blk * t for t in range(4)])
        perms.append(b[p])
    near = [b * 2.0 for _ in range(max(0, k - 3))]
    near = [rounded(rp, (x * (1.0 + 0.01 * j))[None, :], dtype)[0] for j, x in enumerate(near)]
    far = [rounded(rp, (b * 0.5 * (1.0 - 0.001 * j))[None, :], dtype)[0] for j in range(150)]
    X = np.array(near + perms + far)
    X = X[rng.permutation(len(X))]
    Q = np.ones((3, d))
    Q[1] *= 0.75
    Q[2] = np.repeat([1.0, 0.5, 2.0, 0.25], blk)
    return X, Q


def swap_set(rp, dtype, d=128, nswap=200, seed=3):
    """rows that differ from one row by swaps of two elements inside one 16-byte load, with a query
    equal in the swapped coordinates: equal exact dots, sums that round differently when a partial
    sum crosses a binade in one order and not in the other (mixed signs make that common); under
    dedup 2 the reference keeps one row per VALUE, so such rows all count"""
    V = {"f64": 2, "f32": 4, "bf16": 8}[dtype]
    rng = np.random.default_rng(seed)
    b = rounded(rp, (spread_row(rng, d, dtype) * rng.choice([-1.0, 1.0], d))[None, :], dtype)[0]
    rows = [b]
    for _ in range(nswap):
        x = b.copy()
        for _ in range(rng.integers(4, 13)):
            g = rng.integers(0, d // V)
            i, j = g * V + rng.choice(V, 2, replace=False)
            x[i], x[j] = x[j], x[i]
        rows.append(x)
    qv = np.abs(rounded(rp, rng.standard_normal(d // V)[None, :], dtype)[0]) + 0.5
    Q = rounded(rp, np.vstack([np.repeat(qv, V), np.ones(d)]), dtype)
    # 100 rows clearly beyond: pointing away from both queries, far larger than the others
    far = -rounded(rp, (np.abs(rng.standard_normal((100, d))) + 1.0) * np.abs(b).sum(), dtype)
    return rounded(rp, np.vstack([np.array(rows), far]), dtype), Q


def ceiling_set(rp, dtype, d=64, seed=4):
    """k at the LDS ceiling: 1100 distinct rows clearly ordered, then a band of 80 permutations of
    one row around rank 1016 .. 1024 with a constant query, then 60 farther rows"""
    rng = np.random.default_rng(seed)
    b = np.abs(rounded(rp, spread_row(rng, d, dtype)[None, :], dtype)[0])
    s = b.sum()
    near = [rounded(rp, (b * (2.0 + 0.002 * j) + rng.uniform(0, 1e-3, d) * s / d)[None, :], dtype)[0]
            for j in range(990)]
    band = [b[rng.permutation(d)] for _ in range(80)]
    far = [rounded(rp, (b * (0.5 - 0.001 * j))[None, :], dtype)[0] for j in range(60)]
    X = np.array(near + band + far)
    p = rng.permutation(len(X))
    Q = np.ones((2, d))
    Q[1] *= 3.0
    return X[p], Q, np.isin(p, np.arange(990, 1070))


# ------------------------------------------------------------------ 1. cancellation
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M", [1e8, 1e12, 1e16])
def test_cut_under_cancellation(rp, ctx, option, dtype, M):
    Xh, Qh = cancellation_set(rp, dtype, M)
    fl = Flat(rp, ctx, Xh, dtype, 2)
    try:
        bad, unc = check_knn(rp, ctx, fl.f, Xh, Qh, [fl.cands] * len(Qh), METRICS, DEDUPS, (1, 10, 33),
                             ("cancel", dtype, M))
        assert not bad, bad[:20]
        assert not check_exact_option(rp, fl.f, Qh, METRICS, (0, 2), (10,), option)
    finally:
        fl.close()
    if M >= 1e16:      # the two sums are far apart: the fast path must have given up on some queries
        assert max(unc.values()) > 0, unc


# ------------------------------------------------------------------ 2. wide ties
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [1, 10, 33])
def test_cut_on_wide_ties(rp, ctx, option, dtype, k):
    Xh, Qh = tie_set(rp, dtype, k)
    fold = fold_dots(Xh, Qh[0])
    assert len(np.unique(fold)) >= len(Xh) // 3      # the permutations really differ in their bits
    fl = Flat(rp, ctx, Xh, dtype, 2)
    try:
        bad, unc = check_knn(rp, ctx, fl.f, Xh, Qh, [fl.cands] * len(Qh), METRICS, DEDUPS, (k,),
                             ("ties", dtype, k))
        assert not bad, bad[:20]
        assert not check_exact_option(rp, fl.f, Qh, METRICS, DEDUPS, (k,), option)
    finally:
        fl.close()
    assert max(unc.values()) > 0, unc


# ------------------------------------------------------------------ 3. equal sums in one order, nub
@pytest.mark.parametrize("dtype", DTYPES)
def test_cut_nub_on_swapped_lanes(rp, ctx, option, dtype):
    Xh, Qh = swap_set(rp, dtype)
    fl = Flat(rp, ctx, Xh, dtype, 1)
    try:
        # the data exercises the rule: several DIFFERENT swap rows kept for their distinct values
        # among the k best
        kept = [int(np.sum(select(fl.cands, metric_values(m, Xh, q), 33, 2)[0] <= 200))
                for m in METRICS for q in Qh]
        assert max(kept) >= 3, kept
        bad, unc = check_knn(rp, ctx, fl.f, Xh, Qh, [fl.cands] * len(Qh), METRICS, DEDUPS, (1, 10, 33),
                             ("swap", dtype))
        assert not bad, bad[:20]
        assert not check_exact_option(rp, fl.f, Qh, METRICS, (2,), (10, 33), option)
    finally:
        fl.close()


# ------------------------------------------------------------------ 4. k at the LDS ceiling
@pytest.mark.parametrize("dtype", DTYPES)
def test_cut_at_the_lds_ceiling(rp, ctx, option, dtype):
    Xh, Qh, band = ceiling_set(rp, dtype)
    assert len(Xh) > 1100 and len(np.unique(Xh, axis=0)) == len(Xh)
    # under the inner product the band of permutations holds the ranks around every cut, and its
    # members differ in their bits
    r = np.argsort(metric_values("inner", Xh, Qh[0]), kind="stable")
    assert band[r[1000:1030]].all()
    assert len(np.unique(fold_dots(Xh[band], Qh[0]))) >= 3
    fl = Flat(rp, ctx, Xh, dtype, 2)
    try:
        ks = (1016, 1020, 1024)
        bad, unc = check_knn(rp, ctx, fl.f, Xh, Qh, [fl.cands] * len(Qh), METRICS, DEDUPS, ks,
                             ("ceiling", dtype))
        assert not bad, bad[:20]
        assert not check_exact_option(rp, fl.f, Qh, METRICS, (0,), (1024,), option)
    finally:
        fl.close()


# ------------------------------------------------------------------ 5. shape grid on Gaussian data
GRID_D = (1, 3, 7, 8, 31, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 768, 1000)


def gaussian_set(rp, dtype, n, d, nq, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    X[5] = 0.0                                    # a zero row: cosine NaN
    Q = rng.standard_normal((nq, d))
    Q[0] = 0.0                                    # a zero query: cosine NaN, inner -0 everywhere
    Q[1, d // 2] = np.nan                         # a NaN query: NaN everywhere, ranked by position
    Q[2] = X[7]                                   # a stored point
    return rounded(rp, X, dtype), rounded(rp, Q, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", GRID_D)
def test_cut_shape_grid(rp, ctx, option, dtype, d):
    Xh, Qh = gaussian_set(rp, dtype, 300, d, 6, 100 + d)
    fl = Flat(rp, ctx, Xh, dtype, 3)
    try:
        bad, unc = check_knn(rp, ctx, fl.f, Xh, Qh, [fl.cands] * len(Qh), METRICS, DEDUPS, (1, 10, 33),
                             ("grid", dtype, d))
        assert not bad, bad[:20]
        assert not check_exact_option(rp, fl.f, Qh, METRICS, (0, 2), (10,), option)
    finally:
        fl.close()
    # only the zero and the NaN query may fall back to the exact variant (at d = 1 every cosine is 0
    # or 2: ties everywhere, nothing to certify)
    assert max(v for key, v in unc.items() if d > 1 or key[0] == "inner") <= 2, unc


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", [65, 200])
def test_cut_many_ranges(rp, ctx, option, dtype, T):
    """more than kMW = 64 leaf ranges per query (the range window refilled inside a batch) and
    candidate lists many times longer than the merge buffer: a maxDepth-0 forest of T trees, and a
    forest of small leaves over T trees"""
    d = 40
    Xh, Qh = gaussian_set(rp, dtype, 90, d, 5, 7 + T)
    fl = Flat(rp, ctx, Xh, dtype, T)
    try:
        bad, _ = check_knn(rp, ctx, fl.f, Xh, Qh, [fl.cands] * len(Qh), METRICS, DEDUPS, (1, 10, 33),
                           ("flat", dtype, T))
        assert not bad, bad[:20]
    finally:
        fl.close()
    Xh, Qh = gaussian_set(rp, dtype, 3000, d, 5, 9 + T)
    ds = device_data(rp, ctx, Xh, dtype)
    L, ml = 4, 8
    _, R = rp.gen.forest_hyperplanes(5, T, L, 1.0, d)
    f = rp._build(ctx, ds, R, L, ml, rp.RPT_PROJ_AUTO)
    try:
        off, cids = rp.candidatesBatch(f, Qh)
        cands = [cids[off[i * T]:off[(i + 1) * T]] for i in range(len(Qh))]
        assert min(len(c) for c in cands) > 2048
        bad, _ = check_knn(rp, ctx, f, Xh, Qh, cands, METRICS, DEDUPS, (1, 10, 64), ("forest", dtype, T))
        assert not bad, bad[:20]
    finally:
        f.close()
        ds.close()


def test_cut_parity_grid_data_certifies(rp, ctx, oracle):
    """test_gpu_knn_metrics' parity-grid data (Gaussian rows with exact duplicates, rows of other
    norms, queries that are stored points): every query but the zero and the NaN one is answered
    by the fast path"""
    n, d, T, ml, nq = 20_000, 128, 8, 100, 24
    X = oracle.data_normal_dense2(4000 + d, n, d)
    rng = np.random.default_rng(d)
    src = rng.integers(0, n, 60)
    X[rng.integers(0, n, 60)] = X[src]
    X[17] = 0.0
    X[rng.integers(0, n, 40)] *= 10.0
    rng = np.random.default_rng(d + 1)
    Q = rng.standard_normal((nq, d))
    Q[:6] = X[[0, 17, 99, 1234, 5000, 17]]
    Q[6] = 0.0
    Q[7] = rng.standard_normal(d)
    Q[7, 3] = np.nan
    Q[8] = X[3] * 2.0
    cfg = rp.rpTreeCfg(ml, n, d)
    _, R = rp.gen.forest_hyperplanes(77, T, cfg.fpMaxTreeDepth, cfg.fpProjNzDensity, d)
    for dtype in DTYPES:
        Xh, Qh = rounded(rp, X, dtype), rounded(rp, Q, dtype)
        ds = device_data(rp, ctx, Xh, dtype)
        f = rp._build(ctx, ds, R, cfg.fpMaxTreeDepth, ml, rp.RPT_PROJ_AUTO)
        try:
            off, cids = rp.candidatesBatch(f, Qh)
            cands = [cids[off[i * T]:off[(i + 1) * T]] for i in range(nq)]
            bad, unc = check_knn(rp, ctx, f, Xh, Qh, cands, METRICS, DEDUPS, (1, 10, 64, 200), ("parity", dtype))
            assert not bad, bad[:20]
            # the zero query (cosine NaN, inner all -0), the NaN query, and the zero row as a query
            # (Q[1], Q[5]: cosine NaN) may fall back
            assert max(unc.values()) <= 4, (dtype, unc)
        finally:
            f.close()
            ds.close()


# ------------------------------------------------------------------ 6. brute force
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [5, 511, 513, 1025])
def test_cut_brute_force(rp, ctx, dtype, N):
    import ctypes as C
    from rptree_amd import _lib
    Xc, Qc = cancellation_set(rp, dtype, 1e16, n=1100)
    Xt, Qt = tie_set(rp, dtype, 10)
    d = Xc.shape[1]
    nt = min(N // 2, len(Xt)) if N > 5 else N     # cancellation rows and a band of ties
    Xh = np.vstack([Xc[:N - nt], Xt[:nt]])
    Qh = np.vstack([Qc[:3], Qt])
    assert Xh.shape == (N, d)
    ds = device_data(rp, ctx, Xh, dtype)
    allids = np.arange(N, dtype=np.int32)
    bad = []
    try:
        for metric in METRICS:
            for k in sorted({1, 10, min(N + 3, 1024), min(N, 1024)}):
                ids, dist = rp.bruteKnn(ds, Qh, k, metric=distf_of(rp, metric))
                qd, nq = rp._query_dataset(ctx, ds, Qh)
                ids2 = np.empty((nq, k), dtype=np.int32)
                dist2 = np.empty((nq, k), dtype=np.float64)
                flag = rp.RPT_KNN_METRIC_COSINE if metric == "cosine" else rp.RPT_KNN_METRIC_INNER
                _lib.check(_lib.lib().rpt_brute_knn_metric_host(ctx._h, ds._h, qd._h, k, flag,
                                                                C.c_void_p(ids2.ctypes.data),
                                                                C.c_void_p(dist2.ctypes.data)))
                assert np.array_equal(ids2, ids) and same_bits(dist2, dist)
                for i in range(nq):
                    wi, wv = select(allids, metric_values(metric, Xh, Qh[i]), k, 0)
                    why = mismatch(ids[i], dist[i], len(wi), (wi, wv))
                    if why:
                        bad.append((metric, k, i, why))
    finally:
        ds.close()
    assert not bad, bad[:20]


# ------------------------------------------------------------------ 7. sharded path
def test_cut_sharded_forced_exchange(rp, ctx):
    """one rank through the exchange: the shard's answer (and so the merged one) is already exact"""
    from rptree_amd import sharded
    Xh, Qh = cancellation_set(rp, "f64", 1e16, n=3000, nq=16)
    n, d = Xh.shape
    T, ml, k = 4, 100, 10
    cfg = rp.rpTreeCfg(ml, n, d)
    _, R = rp.gen.forest_hyperplanes(3, T, cfg.fpMaxTreeDepth, cfg.fpProjNzDensity, d)
    comm = sharded.Comm.rank(ctx, 1, 0, sharded.Comm.unique_id())
    old = ctx.set_option("comm_force_exchange", 1)
    bad = []
    try:
        ds = rp.Dataset.dense(ctx, Xh)
        sf = sharded.ShardedForest(comm, [ds], R, cfg.fpMaxTreeDepth, ml)
        plain, _, _ = sf.local(0)
        off, cids = rp.candidatesBatch(plain, Qh)
        qs = rp.Dataset.dense(ctx, Qh)
        for metric in METRICS:
            for dedup in (False, True):
                si, sd, sc = sf.knn([qs], k, dedup=dedup, metric=distf_of(rp, metric))
                for i in range(len(Qh)):
                    c = cids[off[i * T]:off[(i + 1) * T]]
                    want = select(c, metric_values(metric, Xh[c], Qh[i]), k, int(dedup))
                    why = mismatch(si[i], sd[i], sc[i], want)
                    if why:
                        bad.append((metric, dedup, i, why))
        qs.close()
        sf.close()
        ds.close()
    finally:
        ctx.set_option("comm_force_exchange", old)
        comm.close()
    assert not bad, bad[:20]
