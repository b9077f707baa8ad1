"""kNN graph under the cosine and inner-product distances on the device (rpt_knn_graph_metric_host /
_dev, csrc/graph.hip): ids, counts and distance BITS against the numpy restatement in
tests/knn_graph_metric_ref.py (mates and order of knn_graph_ref, the dot as np.cumsum over
[0, a b ...])."""
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


def model_pairs(f, ordered=False):
    tot = sum(s * (s - 1) // 2 for _, s in leaves_of(f))
    return f.T * tot * (2 if ordered else 1)


def both_kernels(rp, ctx, metric, k, f, want, tag):
    """the call on the leaf (or, for large leaves, tiled) kernel and under graph_general"""
    got = rp.knnGraphMetric(distf(rp, metric), k, f)
    ref.assert_same_graph(got, want, tag)
    with option(ctx, "graph_general", 1):
        tiled = rp.knnGraphMetric(distf(rp, metric), k, f)
        assert rp.knnGraphLastPairs(ctx) == model_pairs(f, ordered=True)
    ref.assert_same_graph(tiled, want, tag + ", graph_general")
    pad = np.arange(k)[None, :] >= got[2][:, None]
    assert np.all(got[0][pad] == -1) and np.all(np.isposinf(got[1][pad]))
    return got


# ---------------------------------------------------------------- the grid, both kernels
_grid = {}


def grid_case(rp, ctx, dtype, d):
    """data set, forest, mates and the dot matrix, once per (dtype, d)"""
    key = (dtype, d)
    if key not in _grid:
        n, T, minl = 1200, 3 + (d % 3), 40
        ds, X64 = as_dtype(rp, ctx, make_rows(d, n, d), dtype)
        cfg = rp.rpTreeCfg(minl, n, d)
        f = rp.forestBatch(1234 + d, cfg.fpMaxTreeDepth, minl, T, cfg.fpProjNzDensity, d, ds, ctx=ctx)
        _grid[key] = (ds, X64, f, {m: mref.metric_matrix(X64, m) for m in mref.METRICS})
    return _grid[key]


@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("d", [3, 16, 33, 128, 200])
@pytest.mark.parametrize("dtype", ["f64", "f32", "bf16"])
@pytest.mark.parametrize("metric", mref.METRICS)
def test_graph_matches_the_definition(rp, ctx, metric, dtype, d, k):
    ds, X64, f, D = grid_case(rp, ctx, dtype, d)
    want = mref.knn_graph_metric_ref(X64, f.perm, leaves_of(f), k, D[metric])
    got = both_kernels(rp, ctx, metric, k, f, want, "%s %s d %d k %d" % (metric, dtype, d, k))
    n = X64.shape[0]
    for i in range(n):                                     # never its own neighbour
        assert i not in got[0][i]
    if metric == "cosine":                                 # the zero row: NaN both ways, last, by id
        assert np.all(np.isnan(got[1][9, :got[2][9]]))
        row = got[0][9, :got[2][9]].tolist()
        assert row == sorted(row)


def test_restatement_matrix_is_the_cumsum_fold(rp):
    """the column-by-column matrix of the restatement against its np.cumsum fold and the host
    functions of the package, bit for bit"""
    X = make_rows(1, 60, 33)
    for metric in mref.METRICS:
        D = mref.metric_matrix(X, metric)
        for i in (0, 9, 17, 25):
            assert np.array_equal(ref.bits(D[i]), ref.bits(mref.metric_dist(metric, X[i], X)))
            for j in (5, 9, 20, 59):
                assert ref.bits(np.array([distf(rp, metric)(X[i], X[j])]))[0] == ref.bits(D[i, j:j + 1])[0]


# ---------------------------------------------------------------- depth 0, large leaves, tiny inputs
@pytest.mark.parametrize("metric", mref.METRICS)
@pytest.mark.parametrize("n,maxd,k", [(300, 0, 10), (100, 0, 64), (4500, 1, 10), (0, 2, 3), (1, 3, 4), (2, 0, 1),
                                      (3, 0, 4), (130, 1, 64)])
def test_depth_zero_large_leaves_and_tiny_inputs(rp, ctx, metric, n, maxd, k):
    d = 24
    X = make_rows(n + 1, n, d)
    ds = rp.Dataset.dense(ctx, X)
    f = rp.forestBatch(77, maxd, 10 if n > 3 else 1, 2, 0.5, d, ds, ctx=ctx)
    if n == 4500:
        assert min(s for _, s in leaves_of(f)) > 2000      # a depth cap: leaves far above 128
    if maxd == 0 and n:
        assert leaves_of(f) == [(0, n)]
    if n == 0:
        ids, dist, cnt = rp.knnGraphMetric(distf(rp, metric), k, f)
        assert ids.shape == (0, k) and dist.shape == (0, k) and cnt.shape == (0,)
        assert rp.knnGraphLastPairs(ctx) == 0
        return
    D = mref.metric_matrix(X, metric)
    want = mref.knn_graph_metric_ref(X, f.perm, leaves_of(f), k, D)
    both_kernels(rp, ctx, metric, k, f, want, "%s n %d depth %d" % (metric, n, maxd))


# ---------------------------------------------------------------- consistency with bruteKnn
@pytest.mark.parametrize("metric", mref.METRICS)
@pytest.mark.parametrize("dtype", ["f64", "f32", "bf16"])
@pytest.mark.parametrize("n", [100, 300])
def test_depth_zero_row_is_brute_knn_without_the_point(rp, ctx, metric, dtype, n):
    """row i of the all-pairs graph is bruteKnn under the same metric with k + 1 and i dropped: ids
    and distance bits (both are the same fold, ties by ascending id in both)"""
    d, k = 24, 10
    ds, X64 = as_dtype(rp, ctx, make_rows(n, n, d), dtype)
    f = rp.forestBatch(5, 0, 10, 1, 0.5, d, ds, ctx=ctx)
    got = rp.knnGraphMetric(distf(rp, metric), k, f)
    bi, bd = rp.bruteKnn(ds, ds, k + 1, metric=distf(rp, metric))
    for i in range(n):
        keep = [j for j in range(k + 1) if bi[i, j] != i][:k]
        assert bi[i, keep].tolist() == got[0][i].tolist(), (metric, dtype, i)
        assert np.array_equal(ref.bits(bd[i, keep]), ref.bits(got[1][i])), (metric, dtype, i)


# ---------------------------------------------------------------- wide ties
@pytest.mark.parametrize("metric", mref.METRICS)
@pytest.mark.parametrize("n", [120, 400])
def test_small_integer_rows_tie_widely(rp, ctx, metric, n):
    """rows of 0 / 1 entries in 6 columns: an inner product takes one of seven values, so the widest
    tie from point 0 is far above 3 k among 120 points and in the hundreds among 400 (many equal
    cosines too), and for most points the tie straddles the k-th place: ranked by id"""
    d, k = 6, 10
    X = np.random.default_rng(n).integers(0, 2, size=(n, d)).astype(np.float64)
    X[X.any(axis=1) == 0] = 1.0                            # no zero row here
    D = mref.metric_matrix(X, metric)
    if metric == "inner":
        vals, counts = np.unique(D[0], return_counts=True)
        assert counts.max() > (3 * k if n == 120 else 100)
    S = np.sort(np.where(np.eye(n, dtype=bool), np.inf, D), axis=1)
    assert (S[:, k - 1] == S[:, k]).mean() > 0.5           # the cut falls inside a tie
    f = rp.forestBatch(3, 0, 10, 2, 0.5, d, rp.Dataset.dense(ctx, X), ctx=ctx)
    want = mref.knn_graph_metric_ref(X, f.perm, leaves_of(f), k, D)
    both_kernels(rp, ctx, metric, k, f, want, "integer rows %s" % metric)


def test_orthogonal_rows_give_negative_zero_and_ties_by_id(rp, ctx):
    """rows +-e_j: the inner-product distance of two orthogonal rows is -dot = -0.0 (the fold starts
    at +0.0 and +0.0 + -0.0 is +0.0, so a computed dot is never -0.0 and a computed zero distance
    is always -0.0).  +0.0 meets it in one list through RPT_GRAPH_ACCUMULATE, whose stored distances
    are taken as stored: the two tie as numbers, the id decides, every entry keeps its bits."""
    d, n, k = 16, 64, 40
    X = np.zeros((n, d))
    for i in range(n):
        X[i, i % d] = 1.0 if (i // d) % 2 == 0 else -1.0
    D = mref.metric_matrix(X, "inner")
    off = np.arange(n)[:, None] % d != np.arange(n)[None, :] % d
    assert np.all(D[off] == 0.0) and np.all(np.signbit(D[off]))
    ds = rp.Dataset.dense(ctx, X)
    f = rp.forestBatch(3, 0, 10, 1, 0.5, d, ds, ctx=ctx)
    want = mref.knn_graph_metric_ref(X, f.perm, leaves_of(f), k, D)
    got = both_kernels(rp, ctx, "inner", k, f, want, "orthogonal rows")
    zero = got[1][0] == 0.0                                # row 0 = +e_0: -1 with its copies, 1 with -e_0, else -0.0
    assert zero.sum() > 30 and np.all(np.signbit(got[1][0][zero]))
    zi = got[0][0][zero].tolist()
    assert zi == sorted(zi)
    # A forest with small leaves, and a prior whose rows hold the orthogonal ids that are NOT leaf
    # mates at +0.0 (stored distances are the caller's): one list with both zeros.
    f2 = rp.forestBatch(3, 2, 4, 1, 0.5, d, ds, ctx=ctx)
    mates = ref.mates_of(f2.perm, leaves_of(f2), n)
    rows = {i: [j for j in range(n) if off[i, j] and j not in set(mates[i].tolist())] for i in range(n)}
    prior = mref.hand_graph(np.abs(D), k, rows)
    assert not np.signbit(prior[1]).any()
    wantp = mref.knn_graph_metric_ref(X, f2.perm, leaves_of(f2), k, D, prior=prior)
    for general in (0, 1):
        with option(ctx, "graph_general", general):
            gotp = rp.knnGraphMetric(rp.metricInner, k, f2, accumulate=prior)
        ref.assert_same_graph(gotp, wantp, "both zeros, general %d" % general)
    mixed = 0
    for i in range(n):
        c = gotp[2][i]
        z = gotp[1][i, :c] == 0.0
        signs, zi = np.signbit(gotp[1][i, :c][z]), gotp[0][i, :c][z].tolist()
        assert zi == sorted(zi)                            # -0.0 and +0.0 tie: the id decides ...
        assert all(bool(sg) == (j in set(mates[i].tolist())) for sg, j in zip(signs, zi))  # ... the bits stay
        mixed += int(signs.any() and not signs.all())
    assert mixed > 0                                       # some list holds both


@pytest.mark.parametrize("metric", mref.METRICS)
def test_scaled_copies_tie_exactly(rp, ctx, metric):
    """cosine: copies of a row scaled by powers of two are at exactly the same distance from every
    point (the scale leaves dot / (sqrt * sqrt) bit for bit); inner product: positively scaled
    copies of a row orthogonal to y tie at -0.0 from y.  45 tied ids, the first k by id stay."""
    d, k, m = 12, 10, 45
    rng = np.random.default_rng(4)
    if metric == "cosine":
        base = rng.standard_normal(d)
        y = base + 0.3 * rng.standard_normal(d)
        copies = np.array([base * 2.0 ** (a - 20) for a in range(m)])
    else:
        base = np.zeros(d)
        base[:2] = [1.0, 2.0]
        y = np.zeros(d)
        y[:3] = [2.0, -1.0, 5.0]
        copies = np.array([base * (a + 1) for a in range(m)])
    if metric == "cosine":                                 # far: cosine distance near 2 / negative dot with y
        far = -y[None, :] + 0.1 * rng.standard_normal((30, d))
    else:
        a = np.abs(rng.standard_normal((30, 2)))
        far = np.concatenate([-(a[:, :1] + 1.0), a[:, 1:], np.zeros((30, 1)), rng.standard_normal((30, d - 3))], axis=1)
    X = np.concatenate([y[None, :], far[:10], copies, far[10:]])
    order = rng.permutation(len(X))
    X = X[order]
    origin = int(np.nonzero(order == 0)[0][0])
    tied_ids = np.sort(np.nonzero((order >= 11) & (order < 11 + m))[0])
    D = mref.metric_matrix(X, metric)
    assert len(np.unique(ref.bits(D[origin, tied_ids]))) == 1 and m > 3 * k
    f = rp.forestBatch(3, 0, 10, 2, 0.5, d, rp.Dataset.dense(ctx, X), ctx=ctx)
    want = mref.knn_graph_metric_ref(X, f.perm, leaves_of(f), k, D)
    assert want[0][origin].tolist() == tied_ids[:k].tolist()
    got = both_kernels(rp, ctx, metric, k, f, want, "scaled copies %s" % metric)
    assert got[0][origin].tolist() == tied_ids[:k].tolist()


# ---------------------------------------------------------------- accumulate
@pytest.mark.parametrize("metric", mref.METRICS)
@pytest.mark.parametrize("dtype,k", [("f64", 10), ("bf16", 64), ("f32", 3)])
def test_accumulate_folds_forests_in_any_order(rp, ctx, metric, dtype, k):
    n, d, T, minl = 2000, 32, 6, 50
    ds, X64 = as_dtype(rp, ctx, make_rows(2, n, d), dtype)
    cfg = rp.rpTreeCfg(minl, n, d)
    _, R = rp.gen.forest_hyperplanes(99, T, cfg.fpMaxTreeDepth, cfg.fpProjNzDensity, d)
    build = lambda r: rp.forestBatch(0, cfg.fpMaxTreeDepth, minl, len(r), cfg.fpProjNzDensity, d, ds,  # noqa: E731
                                     ctx=ctx, hyperplanes=r)
    whole, fa, fb = build(R), build(R[:T // 2]), build(R[T // 2:])
    df = distf(rp, metric)
    D = mref.metric_matrix(X64, metric)
    g = rp.knnGraphMetric(df, k, whole)
    ref.assert_same_graph(g, mref.knn_graph_metric_ref(X64, whole.perm, leaves_of(whole), k, D), "whole")
    ab = rp.knnGraphMetric(df, k, fb, accumulate=rp.knnGraphMetric(df, k, fa))
    ba = rp.knnGraphMetric(df, k, fa, accumulate=rp.knnGraphMetric(df, k, fb))
    ref.assert_same_graph(ab, g, "a then b")
    ref.assert_same_graph(ba, g, "b then a")
    ref.assert_same_graph(rp.knnGraphMetric(df, k, whole, accumulate=g), g, "into its own result")
    with option(ctx, "graph_general", 1):
        ref.assert_same_graph(rp.knnGraphMetric(df, k, fb, accumulate=rp.knnGraphMetric(df, k, fa)), g,
                              "a then b, tiled")
    half = mref.knn_graph_metric_ref(X64, fa.perm, leaves_of(fa), k, D)
    ref.assert_same_graph(mref.knn_graph_metric_ref(X64, fb.perm, leaves_of(fb), k, D, prior=half), g, "restatement")


# ---------------------------------------------------------------- metric 0 = the old entry points
@pytest.mark.parametrize("dtype", ["f64", "f32", "bf16"])
def test_metric_zero_gives_the_bits_of_the_old_entry_points(rp, ctx, dtype):
    n, d, k = 1500, 33, 10
    ds, X64 = as_dtype(rp, ctx, make_rows(8, n, d), dtype)
    f = rp.forestBatch(11, 5, 40, 4, 0.5, d, ds, ctx=ctx)
    old = rp.knnGraph(k, f)
    for df in (None, rp.metricL2):
        ref.assert_same_graph(rp.knnGraphMetric(df, k, f), old, "metric 0")
    with option(ctx, "graph_general", 1):
        ref.assert_same_graph(rp.knnGraphMetric(None, k, f), old, "metric 0, tiled")
    ref.assert_same_graph(rp.knnGraphMetric(None, k, f, accumulate=old), old, "metric 0, accumulate")
    ref.assert_same_graph(old, ref.knn_graph_ref(X64, f.perm, leaves_of(f), k), "the definition")
    with pytest.raises(NotImplementedError):
        rp.knnGraphMetric(lambda u, v: 0.0, k, f)


# ---------------------------------------------------------------- errors
def test_errors_leave_the_context_usable(rp, ctx):
    from rptree_amd import _lib
    L = _lib.lib()
    n, d, T, minl, k = 1500, 16, 4, 30, 10
    X = np.random.default_rng(12).standard_normal((n, d))
    ds = rp.Dataset.dense(ctx, X)
    cfg = rp.rpTreeCfg(minl, n, d)
    _, R = rp.gen.forest_hyperplanes(7, T, cfg.fpMaxTreeDepth, cfg.fpProjNzDensity, d)
    f = rp.forestBatch(0, cfg.fpMaxTreeDepth, minl, T, cfg.fpProjNzDensity, d, ds, ctx=ctx, hyperplanes=R)
    ids = np.empty((n, 64), dtype=np.int32)
    dist = np.empty((n, 64), dtype=np.float64)
    cnt = np.empty(n, dtype=np.int32)
    COS, INN, REF = rp.RPT_KNN_METRIC_COSINE, rp.RPT_KNN_METRIC_INNER, rp.RPT_KNN_METRIC_REFERENCE

    def refused(code, forest, data, kk, metric, flags):
        st = L.rpt_knn_graph_metric_host(ctx._h, forest._h, data._h, kk, metric, flags, C.c_void_p(ids.ctypes.data),
                                         C.c_void_p(dist.ctypes.data), C.c_void_p(cnt.ctypes.data))
        assert st == code, (st, code)
        msg = L.rpt_last_error().decode()
        assert len(msg) > 8, msg
        return msg

    assert "metric" in refused(RPT_E_ARG, f, ds, k, COS | INN, 0)
    assert "metric" in refused(RPT_E_ARG, f, ds, k, REF, 0)
    assert "metric" in refused(RPT_E_ARG, f, ds, k, COS | 1, 0)
    assert "metric" in refused(RPT_E_ARG, f, ds, k, 1, 0)
    assert "metric" in refused(RPT_E_ARG, f, ds, k, -1, 0)
    assert "flags" in refused(RPT_E_ARG, f, ds, k, COS, COS)
    assert "flags" in refused(RPT_E_ARG, f, ds, k, COS, 2)
    assert "k" in refused(RPT_E_ARG, f, ds, 0, COS, 0)
    assert "k" in refused(RPT_E_ARG, f, ds, 65, INN, 0)
    assert "data set" in refused(RPT_E_ARG, f, rp.Dataset.dense(ctx, X[:-1]), k, COS, 0)
    rowptr = np.arange(n + 1, dtype=np.int64)
    csr = rp.Dataset.csr(ctx, rowptr, np.zeros(n, dtype=np.int32), np.ones(n), d)
    fs = rp.forest(0, cfg.fpMaxTreeDepth, minl, T, 500, cfg.fpProjNzDensity, d, ds, ctx=ctx, hyperplanes=R)
    for m in (0, COS, INN):
        assert "CSR" in refused(RPT_E_UNSUPPORTED, f, csr, k, m, 0)
        assert "streamed" in refused(RPT_E_UNSUPPORTED, fs, ds, k, m, 0)
    with pytest.raises(rp.RPTError) as e:
        rp.knnGraphMetric(rp.metricCosine, 65, f)
    assert e.value.code == RPT_E_ARG
    # the context answers a good call right after, under each metric
    for metric in mref.METRICS:
        want = mref.knn_graph_metric_ref(X, f.perm, leaves_of(f), k, mref.metric_matrix(X, metric))
        ref.assert_same_graph(rp.knnGraphMetric(distf(rp, metric), k, f), want, "after the refusals")
    ref.assert_same_graph(rp.knnGraph(k, f), ref.knn_graph_ref(X, f.perm, leaves_of(f), k), "L2 after the refusals")


# ---------------------------------------------------------------- device arrays, the profile class
@pytest.mark.parametrize("metric", mref.METRICS)
@pytest.mark.parametrize("dtype", ["f64", "bf16"])
def test_dev_entry_point_with_torch_tensors(rp, ctx, metric, dtype):
    import torch
    n, d, T, minl, k = 2500, 64, 4, 50, 10
    X = make_rows(13, n, d)
    dev = torch.device("cuda", ctx.device)
    t = torch.from_numpy(X).to(dev) if dtype == "f64" else torch.from_numpy(X).to(dev).to(torch.bfloat16)
    X64 = t.to(torch.float64).cpu().numpy()
    ds = rp.Dataset.from_torch(ctx, t)
    cfg = rp.rpTreeCfg(minl, n, d)
    f = rp.forestBatch(8, cfg.fpMaxTreeDepth, minl, T, cfg.fpProjNzDensity, d, ds, ctx=ctx)
    ids = torch.full((n, k), 7, dtype=torch.int32, device=dev)
    dist = torch.zeros((n, k), dtype=torch.float64, device=dev)
    cnt = torch.full((n,), 99, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    df = distf(rp, metric)
    rp.knnGraphMetricDev(df, k, f, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr())
    ctx.sync()
    assert rp.knnGraphLastPairs(ctx) == model_pairs(f)
    got = (ids.cpu().numpy(), dist.cpu().numpy(), cnt.cpu().numpy())
    host = rp.knnGraphMetric(df, k, f)
    ref.assert_same_graph(got, host, "dev against host")
    want = mref.knn_graph_metric_ref(X64, f.perm, leaves_of(f), k, mref.metric_matrix(X64, metric))
    ref.assert_same_graph(got, want, "dev")
    rp.knnGraphMetricDev(df, k, f, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr(), accumulate=True)
    ctx.sync()
    ref.assert_same_graph((ids.cpu().numpy(), dist.cpu().numpy(), cnt.cpu().numpy()), host, "dev accumulate")


def test_prof_class_3_times_the_graph(rp, ctx):
    from rptree_amd import _lib
    L = _lib.lib()
    X = make_rows(14, 1000, 16)
    f = rp.forestBatch(8, 4, 30, 3, 0.5, 16, rp.Dataset.dense(ctx, X), ctx=ctx)
    _lib.check(L.rpt_prof_enable(ctx._h, 1))
    try:
        for metric in mref.METRICS:
            _lib.check(L.rpt_prof_reset(ctx._h))
            rp.knnGraphMetric(distf(rp, metric), 5, f)
            ms, cnt = C.c_double(), C.c_int64()
            _lib.check(L.rpt_prof_get(ctx._h, 3, C.byref(ms), C.byref(cnt)))
            assert cnt.value == 1 and ms.value > 0.0
    finally:
        _lib.check(L.rpt_prof_enable(ctx._h, 0))


# ---------------------------------------------------------------- the C++ mirror
def test_cpp_example(rp, ctx, tmp_path):
    n, d, T, minl, k, iters, reverse = 1200, 24, 3, 40, 8, 3, 5
    X = make_rows(15, n, d)
    data = tmp_path / "x.bin"
    data.write_bytes(np.array([n, d], dtype=np.int64).tobytes() + X.tobytes())
    exe = str(tmp_path / "example_knn_graph_metric")
    src = os.path.join(ROOT, "rp-tree_amd", "host", "example_knn_graph_metric.cpp")
    lib = os.path.join(ROOT, "rp-tree_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, src, "-L" + lib, "-lrptree_hip",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    out = tmp_path / "graphs.bin"
    r = subprocess.run([exe, str(data), str(T), str(minl), str(k), str(iters), str(reverse), str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == "ok"
    assert "recall" in r.stdout
    raw = out.read_bytes()
    T2, L = np.frombuffer(raw[:8], dtype=np.int32)
    off = 8
    R = np.frombuffer(raw[off:off + T2 * L * d * 8], dtype=np.float64).reshape(T2, L, d)
    off += R.nbytes
    graphs = []
    for _ in range(2):
        ids = np.frombuffer(raw[off:off + n * k * 4], dtype=np.int32).reshape(n, k)
        off += ids.nbytes
        dist = np.frombuffer(raw[off:off + n * k * 8], dtype=np.float64).reshape(n, k)
        off += dist.nbytes
        cnt = np.frombuffer(raw[off:off + n * 4], dtype=np.int32)
        off += cnt.nbytes
        graphs.append((ids, dist, cnt))
    stats = tuple(int(v) for v in np.frombuffer(raw[off:off + 24], dtype=np.int64))
    r0, r1 = np.frombuffer(raw[off + 24:off + 40], dtype=np.float64)
    ds = rp.Dataset.dense(ctx, X)
    f = rp.forestBatch(0, int(L), minl, int(T2), 0.5, d, ds, ctx=ctx, hyperplanes=R)
    D = mref.metric_matrix(X, "cosine")
    g0 = mref.knn_graph_metric_ref(X, f.perm, leaves_of(f), k, D)
    ref.assert_same_graph(graphs[0], g0, "C++ example, the forest's cosine graph")
    want = mref.refine_ref(X, g0, k, reverse, iters, D)
    ref.assert_same_graph(graphs[1], want[0], "C++ example, refined")
    assert stats == tuple(want[1:])
    assert 0.0 < r0 <= r1 <= 1.0
