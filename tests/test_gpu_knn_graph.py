"""kNN graph of the indexed points on the device (rpt_knn_graph_host / _dev, csrc/graph.hip): ids,
counts and distance BITS against the numpy restatement of the definition in tests/knn_graph_ref.py
(leaf slices of forest.perm from rpt_topology, np.unique of the leaf mates minus the point, the
fold as np.cumsum over [0, (a - b)^2 ...], the order np.lexsort((ids, dist)))."""
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


def make_rows(seed, n, d):
    """finite rows with exact duplicates under other ids, a zero row and rows scaled x10"""
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


# ---------------------------------------------------------------- 1, 4, 8: the grid, both kernels
@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("d", [24, 128, 200])
@pytest.mark.parametrize("dtype", ["f64", "f32", "bf16"])
def test_graph_matches_the_definition(rp, ctx, dtype, d, k):
    n, T, minl = 1500, 4 + (d % 5), 40
    ds, X64 = as_dtype(rp, ctx, make_rows(d + k, n, d), dtype)
    cfg = rp.rpTreeCfg(minl, n, d)
    f = rp.forestBatch(1234 + d, cfg.fpMaxTreeDepth, minl, T, cfg.fpProjNzDensity, d, ds, ctx=ctx)
    want = ref.knn_graph_ref(X64, f.perm, leaves_of(f), k)
    got = rp.knnGraph(k, f)
    ref.assert_same_graph(got, want, "leaf kernel")
    assert rp.knnGraphLastPairs(ctx) == model_pairs(f)
    with option(ctx, "graph_general", 1):
        tiled = rp.knnGraph(k, f)
        assert rp.knnGraphLastPairs(ctx) == model_pairs(f, ordered=True)
    ref.assert_same_graph(tiled, got, "graph_general")
    for i in range(n):                                     # never its own neighbour
        assert i not in got[0][i]


# ---------------------------------------------------------------- 2: leaf sizes around k, tiny inputs
@pytest.mark.parametrize("n,minl,maxd,k", [(3000, 100, 5, 10), (3000, 100, 5, 64), (700, 1, 12, 5),
                                           (1, 1, 3, 4), (2, 1, 3, 4), (2, 1, 0, 1), (130, 10, 1, 64)])
def test_leaf_sizes_and_padding(rp, ctx, n, minl, maxd, k):
    d = 24
    X = make_rows(n, n, d)
    ds = rp.Dataset.dense(ctx, X)
    f = rp.forestBatch(77, maxd, minl, 3, 0.5, d, ds, ctx=ctx)
    want = ref.knn_graph_ref(X, f.perm, leaves_of(f), k)
    got = rp.knnGraph(k, f)
    ref.assert_same_graph(got, want, "n %d" % n)
    pad = np.arange(k)[None, :] >= got[2][:, None]
    assert np.all(got[0][pad] == -1) and np.all(np.isposinf(got[1][pad]))
    with option(ctx, "graph_general", 1):
        ref.assert_same_graph(rp.knnGraph(k, f), want, "n %d tiled" % n)


def test_empty_data_set(rp, ctx):
    """n = 0 is a valid input: nothing is written, nothing is evaluated"""
    ds = rp.Dataset.dense(ctx, np.zeros((0, 8)))
    f = rp.forestBatch(1, 2, 1, 2, 0.5, 8, ds, ctx=ctx)
    ids, dist, cnt = rp.knnGraph(3, f)
    assert ids.shape == (0, 3) and dist.shape == (0, 3) and cnt.shape == (0,)
    assert rp.knnGraphLastPairs(ctx) == 0


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_depth_zero_is_all_pairs(rp, ctx, dtype):
    """maxDepth 0: one leaf, every pair; bruteKnn(X, X, k + 1) minus self is a second witness.  Only
    this case, which projects nothing, carries a row with a NaN: NaN both ways, last, by id."""
    n, d, k = 300, 24, 10
    X = make_rows(3, n, d)
    X[44, 7] = np.nan
    ds, X64 = as_dtype(rp, ctx, X, dtype)
    f = rp.forestBatch(5, 0, 10, 2, 0.5, d, ds, ctx=ctx)
    assert leaves_of(f) == [(0, n)]
    want = ref.knn_graph_ref(X64, f.perm, leaves_of(f), k)
    got = rp.knnGraph(k, f)                                # 300 > 128 points: the tiled kernel
    ref.assert_same_graph(got, want, "depth 0")
    assert np.all(np.isnan(got[1][44])) and got[0][44].tolist() == list(range(k))
    wide = ref.knn_graph_ref(X64, f.perm, leaves_of(f), 64)
    ref.assert_same_graph(rp.knnGraph(64, f), wide, "depth 0, k 64")
    small = X64[100:160].copy()                            # 60 finite rows, then one NaN
    small[24, 3] = np.nan
    ds2 = rp.Dataset.dense(ctx, small)
    f2 = rp.forestBatch(5, 0, 10, 1, 0.5, d, ds2, ctx=ctx)
    g2 = rp.knnGraph(59, f2)                               # 60 points: the leaf kernel; k = n - 1,
                                                           # so every other row ends with the NaN row
    ref.assert_same_graph(g2, ref.knn_graph_ref(small, f2.perm, leaves_of(f2), 59), "depth 0, leaf kernel")
    others = [i for i in range(60) if i != 24]
    assert np.all(g2[0][others, -1] == 24) and np.all(np.isnan(g2[1][others, -1]))
    # second witness: the exhaustive search, the query itself removed
    # The witness is taken on f64 rows only: there bruteKnn's distances are doubles within a few ulp of
    # the fold (1e-12 is generous).  On f32 rows it ranks and reports in f32 arithmetic, and on these
    # rows (some scaled x10) its own list came back out of distance order at two of ten positions
    # (5.801221 ahead of 5.499565 for one point), so it cannot witness an order there.
    if dtype != "f64":
        return
    bi, bd = rp.bruteKnn(ds, ds, k + 1)
    for i in range(n):
        if i == 44 or 44 in want[0][i]:
            continue
        keep = [j for j in range(k + 1) if bi[i, j] != i][:k]
        assert bi[i, keep].tolist() == got[0][i].tolist(), i
        np.testing.assert_allclose(bd[i, keep], got[1][i], rtol=1e-12, atol=0)


# ---------------------------------------------------------------- 3: wide ties
def test_wide_ties_order_by_id(rp, ctx):
    """more than 3 k different ids at exactly the same distance from a point: permuted integer
    coordinates, whose fold sums are equal whatever the order"""
    k, d, m = 10, 24, 45
    rng = np.random.default_rng(8)
    base = np.zeros(d)
    base[:6] = [3, 1, 2, 5, 4, 7]
    rows = {tuple(rng.permutation(base)) for _ in range(4 * m)}
    tied = np.array(sorted(rows))[:m]
    assert len(tied) == m
    far = 50.0 + rng.standard_normal((30, d))
    X = np.concatenate([np.zeros((1, d)), far[:10], tied, far[10:]])
    order = rng.permutation(len(X))
    X = X[order]
    origin = int(np.nonzero(order == 0)[0][0])
    tied_ids = np.sort(np.nonzero((order >= 11) & (order < 11 + m))[0])
    ds = rp.Dataset.dense(ctx, X)
    f = rp.forestBatch(3, 0, 10, 2, 0.5, d, ds, ctx=ctx)
    want = ref.knn_graph_ref(X, f.perm, leaves_of(f), k)
    assert len(np.unique(ref.bits(ref.fold_dist(X[origin], X[tied_ids])))) == 1 and m > 3 * k
    assert want[0][origin].tolist() == tied_ids[:k].tolist()
    for general in (0, 1):
        with option(ctx, "graph_general", general):
            got = rp.knnGraph(k, f)
        ref.assert_same_graph(got, want, "ties, general %d" % general)
        assert got[0][origin].tolist() == tied_ids[:k].tolist()
    # the same inside the leaves of a real forest: duplicate rows are ties of width 40
    n = 1200
    Y = rng.standard_normal((n, d))
    Y[100:140] = Y[100]
    ds = rp.Dataset.dense(ctx, Y)
    f = rp.forestBatch(4, 4, 60, 4, 0.5, d, ds, ctx=ctx)
    want = ref.knn_graph_ref(Y, f.perm, leaves_of(f), k)
    ref.assert_same_graph(rp.knnGraph(k, f), want, "duplicate rows")
    assert want[0][120].tolist() == list(range(100, 110)) and np.all(want[1][120] == 0.0)


# ---------------------------------------------------------------- 4: leaves of thousands of points
def test_depth_cap_leaves_of_thousands(rp, ctx):
    n, d, k = 4500, 24, 10
    X = make_rows(11, n, d)
    ds = rp.Dataset.dense(ctx, X)
    f = rp.forestBatch(21, 1, 10, 2, 0.5, d, ds, ctx=ctx)
    assert min(s for _, s in leaves_of(f)) > 2000
    want = ref.knn_graph_ref(X, f.perm, leaves_of(f), k)
    got = rp.knnGraph(k, f)
    ref.assert_same_graph(got, want, "depth cap")
    with option(ctx, "graph_general", 1):
        ref.assert_same_graph(rp.knnGraph(k, f), got, "depth cap, graph_general")
    assert rp.knnGraphLastPairs(ctx) == model_pairs(f, ordered=True)


# ---------------------------------------------------------------- 5: accumulate
@pytest.mark.parametrize("dtype,k", [("f64", 10), ("bf16", 64), ("f32", 3)])
def test_accumulate_folds_forests_in_any_order(rp, ctx, dtype, k):
    n, d, T, minl = 2000, 32, 6, 50
    ds, X64 = as_dtype(rp, ctx, make_rows(2, n, d), dtype)
    cfg = rp.rpTreeCfg(minl, n, d)
    _, R = rp.gen.forest_hyperplanes(99, T, cfg.fpMaxTreeDepth, cfg.fpProjNzDensity, d)
    build = lambda r: rp.forestBatch(0, cfg.fpMaxTreeDepth, minl, len(r), cfg.fpProjNzDensity, d, ds,  # noqa: E731
                                     ctx=ctx, hyperplanes=r)
    whole, fa, fb = build(R), build(R[:T // 2]), build(R[T // 2:])
    assert np.array_equal(whole.perm, np.concatenate([fa.perm, fb.perm]))
    g = rp.knnGraph(k, whole)
    ref.assert_same_graph(g, ref.knn_graph_ref(X64, whole.perm, leaves_of(whole), k), "whole")
    ab = rp.knnGraph(k, fb, accumulate=rp.knnGraph(k, fa))
    ba = rp.knnGraph(k, fa, accumulate=rp.knnGraph(k, fb))
    ref.assert_same_graph(ab, g, "a then b")
    ref.assert_same_graph(ba, g, "b then a")
    ref.assert_same_graph(rp.knnGraph(k, whole, accumulate=g), g, "into its own result")
    with option(ctx, "graph_general", 1):
        ref.assert_same_graph(rp.knnGraph(k, fb, accumulate=rp.knnGraph(k, fa)), g, "a then b, tiled")
    # the restatement's own accumulate agrees
    half = ref.knn_graph_ref(X64, fa.perm, leaves_of(fa), k)
    ref.assert_same_graph(ref.knn_graph_ref(X64, fb.perm, leaves_of(fb), k, prior=half), g, "restatement")


# ---------------------------------------------------------------- 6: imported forest
def test_imported_forest(rp, ctx, oracle):
    n, d, T, minl, k = 1800, 24, 5, 30, 10
    X = make_rows(6, n, d)
    cfg = rp.rpTreeCfg(minl, n, d)
    _, R = rp.gen.forest_hyperplanes(5, T, cfg.fpMaxTreeDepth, cfg.fpProjNzDensity, d)
    of = oracle.forest_build_dense(X, R, minl)
    f = rp.importForest(ctx, X, R, minl, of.perm, of.thr, of.mglo, of.mghi)
    want = ref.knn_graph_ref(X, of.perm, leaves_of(f), k)
    ref.assert_same_graph(rp.knnGraph(k, f), want, "imported")


# ---------------------------------------------------------------- 7: refusals
def test_refusals_leave_the_context_usable(rp, ctx, oracle):
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

    def call(forest, data, kk, flags):
        return L.rpt_knn_graph_host(ctx._h, forest._h, data._h, kk, flags, C.c_void_p(ids.ctypes.data),
                                    C.c_void_p(dist.ctypes.data), C.c_void_p(cnt.ctypes.data))

    def refused(code, forest, data, kk, flags):
        assert call(forest, data, kk, flags) == code
        msg = L.rpt_last_error().decode()
        assert len(msg) > 8, msg
        return msg

    Q = np.random.default_rng(1).standard_normal((64, d))
    before = rp.knnBatch(k, f, Q)
    tier = C.c_int32(-1)
    _lib.check(L.rpt_knn_last_tier(ctx._h, C.byref(tier)))
    tier_before = tier.value

    assert "k" in refused(RPT_E_ARG, f, ds, 0, 0)
    assert "k" in refused(RPT_E_ARG, f, ds, 65, 0)
    assert "k" in refused(RPT_E_ARG, f, ds, -3, 0)
    assert "data set" in refused(RPT_E_ARG, f, rp.Dataset.dense(ctx, X[:-1]), k, 0)
    assert "data set" in refused(RPT_E_ARG, f, rp.Dataset.dense(ctx, X[:, :-1].copy()), k, 0)
    assert "data set" in refused(RPT_E_ARG, f, rp.Dataset.dense(ctx, X.astype(np.float32)), k, 0)
    refused(RPT_E_ARG, f, ds, k, 2)
    rowptr = np.arange(n + 1, dtype=np.int64)
    csr = rp.Dataset.csr(ctx, rowptr, np.zeros(n, dtype=np.int32), np.ones(n), d)
    assert "CSR" in refused(RPT_E_UNSUPPORTED, f, csr, k, 0)
    fs = rp.forest(0, cfg.fpMaxTreeDepth, minl, T, 500, cfg.fpProjNzDensity, d, ds, ctx=ctx, hyperplanes=R)
    assert "streamed" in refused(RPT_E_UNSUPPORTED, fs, ds, k, 0)
    for flag in (rp.RPT_KNN_METRIC_COSINE, rp.RPT_KNN_METRIC_INNER, rp.RPT_KNN_METRIC_REFERENCE,
                 rp.RPT_KNN_METRIC_COSINE | 1):
        assert "metric" in refused(RPT_E_UNSUPPORTED, f, ds, k, flag)
    with pytest.raises(rp.RPTError) as e:
        rp.knnGraph(65, f)
    assert e.value.code == RPT_E_ARG

    # the context answers an L2 knnBatch right after, as the oracle does
    of = oracle.forest_build_dense(X, R, minl)
    assert np.array_equal(of.perm, f.perm)
    oi, od, oc = oracle.knn_dense_batch(of, X, Q, k)
    gi, gd, gc = rp.knnBatch(k, f, Q)
    assert np.array_equal(gi, oi) and np.array_equal(gc, oc) and np.array_equal(ref.bits(gd), ref.bits(od))

    # ... and a graph call leaves the forest's ranking tiers alone
    g = rp.knnGraph(k, f)
    ref.assert_same_graph(g, ref.knn_graph_ref(X, f.perm, leaves_of(f), k), "after the refusals")
    after = rp.knnBatch(k, f, Q)
    _lib.check(L.rpt_knn_last_tier(ctx._h, C.byref(tier)))
    assert tier.value == tier_before
    for a, b in zip(before, after):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------- 8: device arrays
@pytest.mark.parametrize("dtype", ["f64", "bf16"])
def test_dev_entry_point_with_torch_tensors(rp, ctx, dtype):
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
    rp.knnGraphDev(k, f, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr())
    ctx.sync()
    assert rp.knnGraphLastPairs(ctx) == model_pairs(f)
    got = (ids.cpu().numpy(), dist.cpu().numpy(), cnt.cpu().numpy())
    host = rp.knnGraph(k, f)
    ref.assert_same_graph(got, host, "dev against host")
    ref.assert_same_graph(got, ref.knn_graph_ref(X64, f.perm, leaves_of(f), k), "dev")
    # accumulate on device arrays: folding the same forest in again changes nothing
    rp.knnGraphDev(k, f, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr(), accumulate=True)
    ctx.sync()
    ref.assert_same_graph((ids.cpu().numpy(), dist.cpu().numpy(), cnt.cpu().numpy()), host, "dev accumulate")


def test_prof_class_3_times_the_graph(rp, ctx):
    from rptree_amd import _lib
    L = _lib.lib()
    X = make_rows(14, 1000, 16)
    f = rp.forestBatch(8, 4, 30, 3, 0.5, 16, rp.Dataset.dense(ctx, X), ctx=ctx)
    _lib.check(L.rpt_prof_enable(ctx._h, 1))
    try:
        _lib.check(L.rpt_prof_reset(ctx._h))
        rp.knnGraph(5, f)
        ms, cnt = C.c_double(), C.c_int64()
        _lib.check(L.rpt_prof_get(ctx._h, 3, C.byref(ms), C.byref(cnt)))
        assert cnt.value == 1 and ms.value > 0.0
    finally:
        _lib.check(L.rpt_prof_enable(ctx._h, 0))


# ---------------------------------------------------------------- the C++ mirror
def test_cpp_example(rp, ctx, tmp_path):
    n, d, T, minl, k = 1200, 24, 4, 40, 8
    X = make_rows(15, n, d)
    data = tmp_path / "x.bin"
    data.write_bytes(np.array([n, d], dtype=np.int64).tobytes() + X.tobytes())
    exe = str(tmp_path / "example_knn_graph")
    src = os.path.join(ROOT, "rp-tree_amd", "host", "example_knn_graph.cpp")
    lib = os.path.join(ROOT, "rp-tree_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, src, "-L" + lib, "-lrptree_hip",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    out = tmp_path / "graph.bin"
    r = subprocess.run([exe, str(data), str(T), str(minl), str(k), str(out)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == "ok"
    raw = out.read_bytes()
    T2, L = np.frombuffer(raw[:8], dtype=np.int32)
    off = 8
    R = np.frombuffer(raw[off:off + T2 * L * d * 8], dtype=np.float64).reshape(T2, L, d)
    off += R.nbytes
    ids = np.frombuffer(raw[off:off + n * k * 4], dtype=np.int32).reshape(n, k)
    off += ids.nbytes
    dist = np.frombuffer(raw[off:off + n * k * 8], dtype=np.float64).reshape(n, k)
    off += dist.nbytes
    cnt = np.frombuffer(raw[off:off + n * 4], dtype=np.int32)
    # the same hyperplanes through the Python mirror: the same forest, the same graph
    f = rp.forestBatch(0, int(L), minl, int(T2), 0.5, d, rp.Dataset.dense(ctx, X), ctx=ctx, hyperplanes=R)
    ref.assert_same_graph((ids, dist, cnt), rp.knnGraph(k, f), "C++ example")
    ref.assert_same_graph((ids, dist, cnt), ref.knn_graph_ref(X, f.perm, leaves_of(f), k), "C++ example, def")
